"""fp8 K/V delivered where the caller wants them, as whole poison-filled buffers: in place on
static-cache windows, strided destinations, paged pools (in place and pages-to-dense), ragged
batches, graph capture -- no byte outside rows [0, n) changes -- and the verbatim copy: every NaN
and inf pattern of each format, in K and in V, in the sink, gathered and tail segments, comes out
bit-identical from every copy kernel (the fp8 counterpart of test_nan_payload_gpu, where the
expectation is torch.gather's rewrite; here it is "unchanged")."""
import numpy as np
import pytest
import torch

import fp8_gpu as G
import fp8_util as F
import phase_tables as PT
from kvcompress import _engine as E
from kvcompress import _native as N
from kvcompress import compress_paged
from oracle import oracle

pytestmark = pytest.mark.gpu
POISON = F.POISON8
B, H, D = 2, 2, 128


@pytest.fixture(autouse=True)
def _fresh_memo():
    E.call_memo.clear()
    yield
    E.call_memo.clear()


def pattern_values(shape):
    """V[b, h, s, d] = (s * D + d + 17 * (b * H + h)) % 256: every bit pattern of either format --
    NaNs and infs included -- at every byte lane, in every segment of every output."""
    Bn, Hn, S, Dn = shape
    i = np.arange(S, dtype=np.int64)[:, None] * Dn + np.arange(Dn, dtype=np.int64)[None, :]
    bh = 17 * np.arange(Bn * Hn, dtype=np.int64).reshape(Bn, Hn, 1, 1)
    return ((i[None, None] + bh) % 256).astype(np.uint8)


def pattern_keys(seed, shape, fmt):
    """"normal" keys; every NaN and inf pattern of the format planted in rows of the first 4 (a
    sink), of the last 40 (a tail) and of the middle (the zone: NaN norms are the LARGEST keys, so
    a keep_high selection gathers them)."""
    Bn, Hn, S, Dn = shape
    k = F.gen_keys(seed, shape, fmt, "normal")
    codes = list(F.NAN_CODES[fmt] + F.INF_CODES[fmt])
    rows = [0, 2, S - 1, S - 17] + list(range(100, 100 + 7 * len(codes), 7))
    for j, r in enumerate(rows):  # every code in every planted row, lanes moving with the row
        for e, code in enumerate(codes):
            k[:, :, r, (5 * j + 7 * e) % Dn] = code
    return k


def _window(back, layout, S, start=0):
    v = back if layout == "static" else back.permute(0, 2, 1, 3)
    return v[:, :, start:start + S]


def _cache(shape, layout, pad=9):
    Bn, Hn, S, Dn = shape
    full = (Bn, Hn, S + pad, Dn) if layout == "static" else (Bn, S + pad, Hn, Dn)
    return torch.full(full, POISON, dtype=torch.uint8, device=G.DEV)


def _filled(a8, layout):
    back = _cache(a8.shape, layout)
    win = _window(back, layout, a8.shape[2])
    win.copy_(torch.from_numpy(a8).to(G.DEV))
    assert not win.is_contiguous()
    return back, win


VERBATIM_CALLS = (
    ("h2o_l2", oracle.h2o_l2_compress,
     dict(start_size=4, heavy_hitter_size=64, recent_size=40, skip_layers=[])),
    ("fix_size_l2", oracle.fix_size_l2_compress,
     dict(fix_kv_size=200, keep_ratio=0.2, strategy="keep_high", skip_layers=[])),
)


def _inputs(fmt, S=700, seed=81000):
    shape = (B, H, S, D)
    return pattern_keys(seed, shape, fmt), pattern_values(shape)


def _method(name):
    from kvcompress.methods import get_compress_fn
    return get_compress_fn(name)


@pytest.mark.parametrize("launch", ("fused", "split"))
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_verbatim_default_call(fmt, launch, monkeypatch):
    """select_gather_kernel's gather_row (fused) and gather_kernel (split)."""
    monkeypatch.setattr(E, "split_select_gather", launch == "split")
    k8, v8 = _inputs(fmt)
    for name, ofn, kw in VERBATIM_CALLS:
        (wk, wv), = F.expected(ofn, [(k8, v8)], fmt, **kw)
        codes = set(F.NAN_CODES[fmt] + F.INF_CODES[fmt])
        assert codes <= set(np.unique(wv)) and codes <= set(np.unique(wk)), name
        out = _method(name)([(G.dev8(k8, fmt), G.dev8(v8, fmt))], **kw)
        torch.cuda.synchronize()
        assert np.array_equal(F.to_np(out[0][0]), wk), (name, fmt, launch, "K")
        assert np.array_equal(F.to_np(out[0][1]), wv), (name, fmt, launch, "V")


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_verbatim_few_row_split_copy_and_long_zone(fmt):
    """One (b, h) row with a 9 000-position zone: the 1 024-thread fused kernel with the sink /
    tail rows copied by a second workgroup; 20 000 positions: the global-scratch SELECT and
    gather_kernel."""
    for Z in (9000, 20000):
        S = Z + 44
        k8 = pattern_keys(82000 + Z, (1, 1, S, 64), fmt)
        v8 = pattern_values((1, 1, S, 64))
        kw = dict(start_size=4, heavy_hitter_size=64, recent_size=40, skip_layers=[])
        (wk, wv), = F.expected(oracle.h2o_l2_compress, [(k8, v8)], fmt, **kw)
        out = _method("h2o_l2")([(G.dev8(k8, fmt), G.dev8(v8, fmt))], **kw)
        torch.cuda.synchronize()
        assert np.array_equal(F.to_np(out[0][0]), wk) and np.array_equal(F.to_np(out[0][1]), wv)


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_verbatim_gather_parts_with_caller_indices(fmt):
    """gather_kernel's KVC_FLAG_GATHER_FIXED / _SELECTED parts (external indices; one shared index
    row per (layer, b)): two launches fill one output."""
    S, n_sel = 300, 50
    k8, v8 = _inputs(fmt, S)
    s = PT.spec(S, zone_start=4, zone_len=250, n_select=n_sel, sink=4, tail_start=254, tail_len=46)
    idx = np.sort(np.stack([np.random.default_rng(5 + b).permutation(250)[:n_sel]
                            for b in range(B)]), axis=-1)
    idx[:, :12] = np.arange(96, 108)  # zone rows 100 .. 111: where pattern_keys planted patterns
    idx = np.sort(idx, axis=-1)
    k, v = G.dev8(k8, fmt), G.dev8(v8, fmt)
    n = PT.n_out(s)
    outs = [torch.full((B, H, n, D), POISON, dtype=torch.uint8, device=G.DEV) for _ in range(2)]
    table = np.array([G.layer_row(s, S, k, v, outs[0], outs[1])], dtype=N.LAYER_DTYPE)
    for part in (N.FLAG_GATHER_FIXED, N.FLAG_GATHER_SELECTED):
        L = G.Launch(G.KVC[fmt], B, H, D, PT.ASC, PT.SORT, table.copy(),
                     flags=part | N.FLAG_SHARED_INDEX, external=1)
        iv = L.ws[L.info.index_offset:L.info.index_offset + int(L.info.rows) *
                  int(L.info.index_row_stride) * 4].view(torch.int32)
        iv = iv.view(int(L.info.rows), int(L.info.index_row_stride))
        iv[:B, :n_sel] = torch.from_numpy(idx.astype(np.int32)).to(G.DEV)
        L.run(N.PHASE_GATHER)
    for got, x in ((outs[0], k8), (outs[1], v8)):
        zone = x[:, :, 4:254]
        sel = np.broadcast_to(idx[:, None, :], (B, H, n_sel))
        want = np.concatenate([x[:, :, :4], F.take_rows(zone, sel), x[:, :, 254:300]], axis=2)
        assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_inplace_and_strided_destinations(fmt):
    """gather_dest_kernel through gather_passes: compaction in place on windows of static caches
    (K stored [B, H, S, D], V [B, S, H, D]) and into strided destination windows."""
    k8, v8 = _inputs(fmt)
    t8 = F.torch_dtype(fmt)
    for name, ofn, kw in VERBATIM_CALLS:
        (wk, wv), = F.expected(ofn, [(k8, v8)], fmt, **kw)
        n = wk.shape[2]
        # in place
        (kb, kw_), (vb, vw_) = _filled(k8, "static"), _filled(v8, "bshd")
        was = (kb.clone(), vb.clone())
        out = _method(name)([(kw_.view(t8), vw_.view(t8))], out="inplace", **kw)
        torch.cuda.synchronize()
        assert out[0][0].data_ptr() == kw_.data_ptr() and out[0][0].shape[2] == n
        for back, old, want, layout in ((kb, was[0], wk, "static"), (vb, was[1], wv, "bshd")):
            _window(old, layout, n).copy_(torch.from_numpy(want).to(G.DEV))
            assert torch.equal(back, old), (name, fmt, layout, "in place")
        # strided destinations at row 3 of poisoned caches
        k, v = G.dev8(k8, fmt), G.dev8(v8, fmt)
        kd, vd = _cache((B, H, n + 5, D), "bshd"), _cache((B, H, n + 5, D), "static")
        dst = (_window(kd, "bshd", n + 2, 3).view(t8), _window(vd, "static", n + 2, 3).view(t8))
        was = (kd.clone(), vd.clone())
        out = _method(name)([(k, v)], out=[dst], **kw)
        torch.cuda.synchronize()
        assert out[0][0].data_ptr() == dst[0].data_ptr() and out[0][0].shape[2] == n
        for back, old, want, layout in ((kd, was[0], wk, "bshd"), (vd, was[1], wv, "static")):
            _window(old, layout, n, 3).copy_(torch.from_numpy(want).to(G.DEV))
            assert torch.equal(back, old), (name, fmt, layout, "strided destination")
        assert torch.equal(G.as_u8(k).cpu(), torch.from_numpy(k8))


@pytest.mark.parametrize("P", (1, 16, 64))
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_paged_in_place_and_pages_to_dense(fmt, P):
    """gather_paged_kernel, both pool storages."""
    k8, v8 = _inputs(fmt)
    t8 = F.torch_dtype(fmt)
    for st in G.STORAGES:
        for name, ofn, kw in VERBATIM_CALLS:
            (wk, wv), = F.expected(ofn, [(k8, v8)], fmt, **kw)
            n = wk.shape[2]
            pool = G.Pool((k8, v8), fmt, P, 83000 + P, st)
            snap = pool.snapshot()
            assert compress_paged(name, [pool.paged()], **kw) == [n]
            torch.cuda.synchronize()
            for b in range(B):
                pool.expect(snap, b, wk[b:b + 1], wv[b:b + 1])
            pool.assert_pools(snap, (name, fmt, P, st, "in place"))
            # pages to dense
            pool = G.Pool((k8, v8), fmt, P, 83500 + P, st)
            snap = pool.snapshot()
            kd, vd = _cache((B, H, n, D), "static"), _cache((B, H, n, D), "bshd")
            was = (kd.clone(), vd.clone())
            dst = (_window(kd, "static", n, 2).view(t8), _window(vd, "bshd", n, 2).view(t8))
            out = compress_paged(name, [pool.paged()], out=[dst], **kw)
            torch.cuda.synchronize()
            assert out[0][0].shape[2] == n
            for back, old, want, layout in ((kd, was[0], wk, "static"), (vd, was[1], wv, "bshd")):
                _window(old, layout, n, 2).copy_(torch.from_numpy(want).to(G.DEV))
                assert torch.equal(back, old), (name, fmt, P, st, layout, "pages to dense")
            pool.assert_pools(snap, (name, fmt, P, st, "pool untouched"))


RAGGED_LENS = (0, 37, 512, 513, 1500)


def _ragged_seqs(fmt, seed, Dn=D):
    return [(pattern_keys(seed + b, (1, H, n, Dn), fmt) if n >= 200 else
             F.gen_keys(seed + b, (1, H, n, Dn), fmt, "few"), pattern_values((1, H, n, Dn)))
            for b, n in enumerate(RAGGED_LENS)]


def _ragged_expect(ofn, kw, seqs, fmt):
    """Per sequence (K_out, V_out, kind) of the method on that sequence alone."""
    out = []
    for k8, v8 in seqs:
        kind = ofn([(F.to_bf16_bits(k8, fmt), np.zeros(k8.shape, np.uint16))], **kw)[0][2]
        (wk, wv), = F.expected(ofn, [(k8, v8)], fmt, **kw)
        out.append((wk, wv, kind))
    return out


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_ragged_batch_equals_single_sequence_calls(fmt):
    """gather_ragged_kernel: lengths 0 / 37 / 512 / 513 / 1 500 in one call."""
    seqs = _ragged_seqs(fmt, 84000)
    for (P, st), (name, ofn, kw) in zip(((16, G.STORAGES[0]), (64, G.STORAGES[1])),
                                        VERBATIM_CALLS):
        want = _ragged_expect(ofn, kw, seqs, fmt)
        pool = G.Pool(seqs, fmt, P, 84500 + P, st)
        snap = pool.snapshot()
        lens = compress_paged(name, [pool.paged(ragged=True)], **kw)
        torch.cuda.synchronize()
        assert list(lens[0]) == [w[0].shape[2] for w in want]
        assert {w[2] for w in want} == {"same", "new"}
        for b, (wk, wv, kind) in enumerate(want):
            if kind != "same":
                pool.expect(snap, b, wk, wv)
        pool.assert_pools(snap, (name, fmt, P, st))
        # ... and equal to B single-sequence paged calls
        for b, (k8, v8) in enumerate(seqs):
            if want[b][2] == "same":
                continue
            one = G.Pool([(k8, v8)], fmt, P, 84900 + b, st)
            s1 = one.snapshot()
            assert compress_paged(name, [one.paged()], **kw) == [want[b][0].shape[2]]
            one.expect(s1, 0, want[b][0], want[b][1])
            one.assert_pools(s1, (name, fmt, P, b, "single"))


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_graph_capture_dense_and_ragged(fmt):
    name, ofn, kw = VERBATIM_CALLS[0]
    shape = (B, H, 700, D)
    k = torch.zeros(shape, dtype=torch.uint8, device=G.DEV).view(F.torch_dtype(fmt))
    v = torch.zeros(shape, dtype=torch.uint8, device=G.DEV).view(F.torch_dtype(fmt))

    def fill(f):
        k8, v8 = pattern_keys(85000 + f, shape, fmt), F.gen_values(85000 + f, shape, fmt)
        G.as_u8(k).copy_(torch.from_numpy(k8).to(G.DEV))
        G.as_u8(v).copy_(torch.from_numpy(v8).to(G.DEV))
        return F.expected(ofn, [(k8, v8)], fmt, **kw)[0]

    fill(0)
    _method(name)([(k, v)], **kw)  # the warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _method(name)([(k, v)], **kw)
    for rep in (1, 2):
        wk, wv = fill(rep)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(F.to_np(out[0][0]), wk) and np.array_equal(F.to_np(out[0][1]), wv)
    del g
    torch.cuda.synchronize()
    # ragged (kvc_launch_ragged captured, as tests/test_ragged_gpu.py captures it: compress_paged
    # uploads its records, which a capture cannot hold): the pool is rewritten between replays
    P, st = 16, G.STORAGES[0]
    pool = G.Pool(_ragged_seqs(fmt, 86000), fmt, P, 86500, st)

    def spec_of(n):  # h2o_l2's segments: sink 4, 64 of the middle, the last 40; short: a no-op
        if n <= 108:
            return dict(PT.spec(n, sink=n), S=n)
        return dict(PT.spec(n, zone_start=4, zone_len=n - 44, n_select=64, sink=4,
                            tail_start=n - 40, tail_len=40), S=n)
    specs = [spec_of(n) for n in RAGGED_LENS]
    host, dev = G.seq_records(specs)
    ragged = np.zeros(1, dtype=N.RAGGED_DTYPE)
    ragged[0] = (host.ctypes.data, dev.data_ptr())
    table = np.array([G.layer_row(specs[-1], RAGGED_LENS[-1], pool=pool)], dtype=N.LAYER_DTYPE)
    L = G.Launch(G.KVC[fmt], len(RAGGED_LENS), H, D, PT.ASC, PT.SORT, table,
                 pages=G.pages_row(pool, in_place=1), ragged=ragged)

    def refill(f):
        sq = _ragged_seqs(fmt, 86000 + 10 * f)
        pool.kb.fill_(G.PU.POISON)
        pool.vb.fill_(G.PU.POISON)
        for b, (k8, v8) in enumerate(sq):
            pool.write(pool.k8, b, k8)
            pool.write(pool.v8, b, v8)
        snap = pool.snapshot()
        for b, ((k8, v8), s) in enumerate(zip(sq, specs)):
            if s["n_select"]:
                wk, wv, _ = F.expected_spec(k8, v8, s, PT.ASC, PT.SORT, fmt)
                pool.expect(snap, b, wk, wv)
        return snap

    snap = refill(0)
    L.run(N.PHASE_ALL)  # the warm-up
    pool.assert_pools(snap, (fmt, "ragged eager"))
    refill(1)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        L.run(N.PHASE_ALL, sync=False)
    for rep in (2, 3):
        snap = refill(rep)
        g.replay()
        torch.cuda.synchronize()
        pool.assert_pools(snap, (fmt, "ragged replay", rep))
    assert int(L.status.item()) == 0
    del g
    torch.cuda.synchronize()
