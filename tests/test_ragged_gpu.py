"""Ragged paged batches on the GPU (include/kvc.h, "Ragged paged batches"; PagedKV with a length
per sequence): one compress_paged call over B sequences of different lengths gives, in every pool
byte and in the returned lengths, what the method gives on each sequence alone.

Expected bytes come from the CPU oracle run on each sequence alone (tests/ragged_util.py); whole
backing buffers -- spare pages, rows >= n_out, pages behind -1 table entries -- are compared with
poisoned snapshots.  tests/test_ragged_plan.py shows that these cases cannot pass with the records
ignored.  The status word stays clear (the autouse fixture checks it).
"""
import numpy as np
import pytest
import torch

import paged_util as PU
import prng
import ragged_util as RU
from kvcompress import _native as N

pytestmark = pytest.mark.gpu

DEV = PU.DEV

ALL = [(m, kw, L, g) for m, kw, L in RU.METHOD_CASES for g in RU.GEOMETRIES]


@pytest.mark.parametrize("method, kw, L, geo", ALL,
                         ids=[f"{m}-P{g[0]}-{g[1]}-D{g[2]}" for m, _, _, g in ALL])
def test_every_method(method, kw, L, geo):
    """1: an empty sequence, two passed through, a decode-shaped k = n - 1 selection and an ordinary
    one in one call; layers with a skip list; pages shorter and longer than a 64-token tile."""
    P, dtype, D, storages = geo
    layers_np, pls = RU.build(4100 + 17 * P, RU.LENS, RU.H, D, dtype, P, L, storages=storages)
    lens, ref = RU.check_against_oracle(method, kw, layers_np, pls, (method, P, dtype))
    kinds = {ref[l][b][2] for l in range(L) for b in range(len(RU.LENS))}
    assert "same" in kinds and kinds - {"same"}, kinds  # passed through AND compressed
    for l in range(L):
        assert lens[l][0] == 0 and lens[l][1] == 37


def test_33_layers_cross_the_argument_chunk():
    """33 ragged layers in one launch: the argument chunk of a paged launch holds 32."""
    kw = dict(fix_kv_size=48, keep_ratio=0.25, skip_layers=[])
    layers_np, pls = RU.build(4200, [100, 37], 2, 32, "bf16", 16, 33)
    lens, _ = RU.check_against_oracle("fix_size_l2", kw, layers_np, pls, ("33 layers",))
    assert lens == [[48, 37]] * 33


def test_lengths_given_as_array_and_tensor():
    """numpy and CPU-tensor lengths, an int layer beside ragged ones (B equal lengths), and
    to_dense(b=...) of the compacted rows."""
    from kvcompress import PagedKV, compress_paged
    from gpu_util import to_np
    kw = dict(fix_kv_size=512, keep_ratio=0.25, skip_layers=[])
    lens = [700, 700, 700]
    for lens_as in (lambda x: np.asarray(x, dtype=np.int64), lambda x: torch.tensor(x)):
        layers_np, pls = RU.build(4300, lens, 2, 64, "bf16", 16, 2, lens_as=lens_as)
        ref = RU.oracle_per_sequence("fix_size_l2", kw, layers_np)
        paged = [pls[0].paged, PagedKV(pls[1].k, pls[1].v, pls[1].table, 700)]  # ragged + int
        assert paged[0].ragged and not paged[1].ragged and paged[1].seq_lens == (700,) * 3
        assert paged[0].shape == (3, 2, 700, 64)
        snaps = [pl.snapshot() for pl in pls]
        out = compress_paged("fix_size_l2", paged, **kw)
        torch.cuda.synchronize()
        assert out == [[512] * 3, [512] * 3]
        for l, (pl, snap) in enumerate(zip(pls, snaps)):
            for b in range(3):
                pl.expect(snap, b, ref[l][b][0], ref[l][b][1])
                kd, vd = paged[l].to_dense(512, b=b)
                assert np.array_equal(to_np(kd), ref[l][b][0]) and np.array_equal(to_np(vd), ref[l][b][1])
            pl.assert_pools(snap, ("lens_as", l))


CLASSES = [  # (lengths, H, D): a short row inside the 512-thread, 1 024-thread, global, long kernel
    ([4100, 70], 2, 64), ([8200, 300, 64], 2, 64), ([16390, 1000], 1, 64), ([65600, 129], 1, 32)]
SELECTORS = [
    ("l2_compress", dict(keep_ratio=0.5, prune_after=50, skip_layers=[])),                # sort
    ("snapkv_lite", dict(observation_window=4, keep_size=40, pooling_kernel=5,
                         skip_layers=[])),                                               # top-k
]


@pytest.mark.parametrize("method, kw", SELECTORS, ids=[m for m, _ in SELECTORS])
@pytest.mark.parametrize("lens, H, D", CLASSES, ids=[str(c[0][0]) for c in CLASSES])
def test_short_rows_inside_every_selection_kernel_class(lens, H, D, method, kw):
    """2: the launch's selection kernel is chosen by the longest zone; every other row is far
    below that envelope.  Tie-heavy keys, and one short row carries NaNs."""
    layers_np = [RU.gen_sequences(5200 + lens[0], lens, H, D, "bf16", "few")]
    k = prng.to_bits(layers_np[0][1][0]).copy()
    k[0, 0, 5::7, 3] = 0x7FC1  # NaN norms in head 0 of the short sequence
    layers_np[0][1] = (prng.from_bits(k, "bf16"), layers_np[0][1][1])
    pls = [RU.RaggedLayer(layers_np[0], 16, 5200 + lens[0])]
    RU.check_against_oracle(method, kw, layers_np, pls, (method, lens[0]))


def test_snapkv_lite_on_both_sides_of_its_branches():
    """3: prefixes shorter than the pooling kernel (unpooled scores) beside pooled ones and a
    passed-through sequence in one layer; then keep_size == observation_window, where every longer
    sequence becomes its last window (a copy-only move)."""
    lens = [35, 36, 600, 34, 20, 40]
    kw = dict(observation_window=32, keep_size=34, pooling_kernel=5, skip_layers=[])
    layers_np, pls = RU.build(5300, lens, 2, 64, "bf16", 16, 2)
    got, _ = RU.check_against_oracle("snapkv_lite", kw, layers_np, pls, ("pooling",))
    assert got[0] == [34, 34, 34, 34, 20, 34]
    kw = dict(observation_window=32, keep_size=32, skip_layers=[1])
    layers_np, pls = RU.build(5310, [33, 600, 20], 2, 128, "fp16", 4, 2)
    got, _ = RU.check_against_oracle("snapkv_lite", kw, layers_np, pls, ("views",))
    assert got == [[32, 32, 20], [33, 600, 20]]


def test_stable_tie_policy(monkeypatch):
    from kvcompress import _engine
    monkeypatch.setattr(_engine, "tie_policy", "stable")
    layers_np, pls = RU.build(5400, [1500, 0, 700, 513], 2, 64, "bf16", 16, 1, variant="few")
    kw = dict(fix_kv_size=512, keep_ratio=0.25, skip_layers=[])
    from oracle import oracle
    snaps = [pl.snapshot() for pl in pls]
    from kvcompress import compress_paged
    lens = compress_paged("fix_size_l2", [pl.paged for pl in pls], **kw)
    torch.cuda.synchronize()
    assert lens == [[512, 0, 512, 512]]
    for b, (k, v) in enumerate(layers_np[0]):  # the stable first-k of each sequence alone
        S = k.shape[2]
        if S <= 512:
            continue
        Z = S - 128
        idx = np.sort(oracle.stable_prefix(oracle.as_float(oracle.norms(k[:, :, :Z])), 384), axis=-1)
        pls[0].expect(snaps[0], b, oracle.cat([oracle.gather(k[:, :, :Z], idx), k[:, :, Z:]]),
                      oracle.cat([oracle.gather(v[:, :, :Z], idx), v[:, :, Z:]]))
    pls[0].assert_pools(snaps[0], ("stable",))


def _workaround_inputs():
    lens = [1500, 37, 513, 900]
    return lens, dict(start_size=4, heavy_hitter_size=64, recent_size=444, skip_layers=[1])


def test_equal_to_one_call_per_sequence():
    """4a: the same pools compacted by B single-sequence compress_paged calls."""
    from kvcompress import PagedKV, compress_paged
    lens, kw = _workaround_inputs()
    _, a = RU.build(5500, lens, 2, 64, "bf16", 16, 3)
    _, w = RU.build(5500, lens, 2, 64, "bf16", 16, 3)
    got = compress_paged("h2o_l2", [pl.paged for pl in a], **kw)
    for b, n in enumerate(lens):
        one = compress_paged("h2o_l2", [PagedKV(pl.k, pl.v, pl.table[b:b + 1], n) for pl in w], **kw)
        assert one == [g[b] for g in got]
    torch.cuda.synchronize()
    for l, (x, y) in enumerate(zip(a, w)):
        assert torch.equal(PU.ints(x.kb), PU.ints(y.kb)) and torch.equal(PU.ints(x.vb), PU.ints(y.vb)), l


def _tables(pls, rec, B, entries):
    """kvc_layer_t / kvc_pages_t rows of `entries` [(layer, b) | layer]: (layer, b) is the batch-1
    entry of sequence b (table pointer offset by b rows, segments of its record)."""
    n = len(entries)
    table, pages = np.zeros(n, dtype=N.LAYER_DTYPE), np.zeros(n, dtype=N.PAGES_DTYPE)
    for i, e in enumerate(entries):
        l, b = e if isinstance(e, tuple) else (e, None)
        pl, t = pls[l], table[i]
        t["k"] = t["k_out"] = pl.k.data_ptr()
        t["v"] = t["v_out"] = pl.v.data_ptr()
        t["k_stride"] = (0, pl.k.stride(1), pl.k.stride(2))
        t["v_stride"] = (0, pl.v.stride(1), pl.v.stride(2))
        off = 0 if b is None else b * pl.table.stride(0) * 4
        pages[i] = (pl.table.data_ptr() + off, pl.table.stride(0), pl.k.stride(0), pl.v.stride(0),
                    pl.P, pl.k.size(0), 1, 0)
        if b is not None:
            for f in ("seq_len", "zone_start", "zone_len", "n_select", "sink_len", "tail_start",
                      "tail_len", "score_mode", "pool_kernel"):
                t[f] = rec[l, b][f]
    return table, pages


def _plan_records(method, pls, lens, kw):
    from kvcompress import paged
    from kvcompress.methods import get_compress_fn
    geo = [(pl.k.size(1), pl.k.size(3), pl.k.dtype, pl.k.device) for pl in pls]
    return paged.plan_ragged(get_compress_fn(method), [lens] * len(pls), geo, kw)


def test_equal_to_one_table_entry_per_sequence():
    """4b: through the C ABI, kvc_launch_paged with one batch-1 entry per (layer, sequence) -- the
    version whose launch count grows with B -- leaves the same pool bytes."""
    from kvcompress import _engine as E
    from kvcompress import compress_paged
    lens, kw = _workaround_inputs()
    _, a = RU.build(5500, lens, 2, 64, "bf16", 16, 3)
    _, w = RU.build(5500, lens, 2, 64, "bf16", 16, 3)
    compress_paged("h2o_l2", [pl.paged for pl in a], **kw)
    rec, how, _ = _plan_records("h2o_l2", w, lens, kw)
    entries = sorted(how)
    assert len(entries) == 2 * 3 and len(set(how.values())) == 1  # two layers x three sequences
    order, algo = next(iter(how.values()))
    table, pages = _tables(w, rec, len(lens), entries)
    p = E._params(torch.bfloat16, 1, 2, 64, order, algo, False)
    rc, info = N.plan_paged(p, table, pages, None)
    assert rc == 0
    ws = torch.empty(max(int(info.workspace_bytes), 256), dtype=torch.uint8, device=DEV)
    assert N.launch_paged(p, table, pages, None, ws.data_ptr(), int(info.workspace_bytes),
                          torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    for l, (x, y) in enumerate(zip(a, w)):
        assert torch.equal(PU.ints(x.kb), PU.ints(y.kb)) and torch.equal(PU.ints(x.vb), PU.ints(y.vb)), l


def test_captured_launch_follows_rewritten_records():
    """5: kvc_launch_ragged captured in a CUDA graph; before the replay the pools are refilled with
    other sequences and the device records rewritten to other lengths inside the planned envelope.
    The replay follows the new records (and the new table contents' rows)."""
    from kvcompress import _engine as E
    kw = dict(fix_kv_size=512, keep_ratio=0.25, skip_layers=[])
    room, first, second = [1500, 1500, 600], [1500, 900, 37], [700, 1500, 600]
    L, H, D = 2, 2, 64
    _, pls = RU.build(5600, room, H, D, "bf16", 16, L)  # pages for the longest use of every row
    rec, how, _ = _plan_records("fix_size_l2", pls, first, kw)
    host = np.ascontiguousarray(rec)
    dev = torch.from_numpy(host.view(np.uint8).reshape(-1).copy()).to(DEV)
    table, pages = _tables(pls, rec, 3, list(range(L)))
    ragged = np.zeros(L, dtype=N.RAGGED_DTYPE)
    for l in range(L):
        ragged[l] = (host[l].ctypes.data, dev.data_ptr() + l * 3 * N.SEQ_DTYPE.itemsize)
    p = E._params(torch.bfloat16, 3, H, D, N.KVC_ASC, N.KVC_ALGO_SORT, False)
    rc, info = N.plan_ragged(p, table, pages, ragged)
    assert rc == 0
    ws = torch.empty(max(int(info.workspace_bytes), 256), dtype=torch.uint8, device=DEV)

    def launch():
        return N.launch_ragged(p, table, pages, ragged, ws.data_ptr(), int(info.workspace_bytes),
                               torch.cuda.current_stream().cuda_stream)

    def run(lens, seed, go):
        layers_np = [RU.gen_sequences(seed + 1000 * l, lens, H, D, "bf16") for l in range(L)]
        for pl, seqs in zip(pls, layers_np):
            pl.fill(seqs)
        rec2, _, new = _plan_records("fix_size_l2", pls, lens, kw)
        dev.copy_(torch.from_numpy(np.ascontiguousarray(rec2).view(np.uint8).reshape(-1)))
        snaps = [pl.snapshot() for pl in pls]
        go()
        torch.cuda.synchronize()
        ref = RU.oracle_per_sequence("fix_size_l2", kw, layers_np)
        for l, (pl, snap) in enumerate(zip(pls, snaps)):
            for b in range(3):
                assert new[l][b] == ref[l][b][0].shape[2]
                if ref[l][b][2] != "same":
                    pl.expect(snap, b, ref[l][b][0], ref[l][b][1])
            pl.assert_pools(snap, ("graph", lens, l))

    run(first, 5610, lambda: launch() == 0 or pytest.fail("eager launch"))  # the warm-up
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert launch() == 0
    run(first, 5620, g.replay)
    run(second, 5630, g.replay)


SWEEP = RU.sweep_cases()


@pytest.mark.parametrize("chunk", range(8))
def test_seeded_sweep(chunk):
    """6: 64 seeded random ragged calls, eight per test, each against the per-sequence oracle."""
    for c in SWEEP[8 * chunk:8 * chunk + 8]:
        layers_np, pls = RU.build(c["seed"], c["lens"], c["H"], c["D"], c["dtype"], c["P"], c["L"],
                                  variant=c["variant"], storages=c["storages"])
        RU.check_against_oracle(c["method"], c["kw"], layers_np, pls, (c["id"],))


def test_refusals_leave_the_pools_untouched():
    from kvcompress import compress_paged
    layers_np, pls = RU.build(5700, [1500, 600], 2, 64, "bf16", 16, 2)
    snaps = [pl.snapshot() for pl in pls]
    paged = [pl.paged for pl in pls]
    with pytest.raises(TypeError, match="caller-provided indices"):
        compress_paged("fix_size_l2", paged, fix_kv_size=512, strategy="random", skip_layers=[])
    dst = tuple(torch.zeros(2, 2, 600, 64, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    with pytest.raises(TypeError, match="in place only"):
        compress_paged("fix_size_l2", paged, out=[None, dst], fix_kv_size=512, skip_layers=[])
    with pytest.raises(ValueError, match="cannot be compacted in place"):
        compress_paged("streaming_llm", paged, start_size=4, recent_size=0)
    torch.cuda.synchronize()
    for pl, snap in zip(pls, snaps):
        pl.assert_pools(snap, ("after refusals",))
    # h2o_attention without a manager selects L2 heavy hitters in the engine (no caller indices):
    # it runs on ragged layers, as h2o_l2
    kw = dict(start_size=4, heavy_hitter_size=64, recent_size=100)
    ref = RU.oracle_per_sequence("h2o_l2", dict(skip_layers=[], **kw), layers_np)
    assert compress_paged("h2o_attention", paged, **kw) == [[168, 168]] * 2
    torch.cuda.synchronize()
    for l, (pl, snap) in enumerate(zip(pls, snaps)):
        for b in range(2):
            pl.expect(snap, b, ref[l][b][0], ref[l][b][1])
        pl.assert_pools(snap, ("h2o_attention", l))
