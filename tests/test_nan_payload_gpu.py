"""torch.gather's NaN rewrite on the GPU: every copy kernel on every NaN bit pattern.

The reference builds the kept zone with torch.gather, which on the CPU turns every bf16 NaN into
0xFFFF and sets bit 9 of every fp16 NaN, and the rest of an output with torch.cat, which copies
(oracle.gather; the rule itself is held against torch in tests/test_nan_payload.py).  The engine
restates that in canon_nan_dt (csrc/kvc_device_util.h), called by gather_block / gather_row
(csrc/kvc_gather.h) and by gather_passes (csrc/kvc_gather_dest.h), the pass body of
gather_dest_kernel and of gather_paged_kernel (csrc/kvc_paged.h).  Here each of the four kernels'
paths copies values that run through every NaN pattern of the
dtype in both halves of a 32-bit word, beside NaN and non-NaN halves (prng "patterns"), and keys
with non-canonical NaNs of both signs (prng "payload"); every comparison is of raw bytes against
the CPU oracle, and the device status word stays 0.

That these inputs cannot be passed by a copy that rewrites too little, too much or the wrong
half is proved on the CPU (tests/test_nan_payload.py::test_wrong_copies_cannot_pass).
"""
import functools

import numpy as np
import pytest
import torch

import paged_util as PU
import phase_tables as PT
import prng
from gpu_util import kind_of, to_dev, to_np
from kvcompress import _native as N
from oracle import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"bf16": N.KVC_BF16, "fp16": N.KVC_F16, "fp32": N.KVC_F32}
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
INT = {2: torch.int16, 4: torch.int32}
DTYPES = ("bf16", "fp16", "fp32")
FILL = 0x5A  # every output byte before a launch: a finite value the pattern table does not hold


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(t, want):
    return np.array_equal(_bytes(to_np(t)), _bytes(want))


def _ints(t):
    return t.view(INT[t.element_size()])


def _engine_status_clear():
    from kvcompress import _engine
    assert _engine.device_status(0) == 0


# ------------------------------------------------------------------------------------------
# a. the copy kernels in isolation: caller-written indices through the C ABI
# ------------------------------------------------------------------------------------------
B, H = 2, 3
SPEC = PT.spec(700, zone_start=30, zone_len=500, n_select=260, sink=4, tail_start=545,
               tail_len=150)
N_OUT = PT.n_out(SPEC)
WIDTHS = (32, 80, 256)  # 16-byte chunks per row: 4, 10, 32 (16-bit) and 8, 20, 64 (fp32)


@functools.lru_cache(maxsize=2)
def _copy_inputs(dtype, D):
    """K and V [2, 3, 700, D], both "patterns": K holds V's rows 101 positions on."""
    V = prng.gen_values(0, (B, H, SPEC["S"], D), dtype, "patterns")
    return np.ascontiguousarray(np.roll(V, 101, axis=2)), V


def _picks(seed, n_layers=1, shared=False):
    """[layers, B, H or 1, 260] ascending random zone positions."""
    rng = np.random.default_rng(seed)
    rows = n_layers * B * (1 if shared else H)
    idx = np.stack([np.sort(rng.choice(SPEC["zone_len"], SPEC["n_select"], replace=False))
                    for _ in range(rows)])
    return idx.reshape(n_layers, B, 1 if shared else H, -1).astype(np.int64)


def _expected(dtype, D, idx):
    K, V = _copy_inputs(dtype, D)
    idx = np.broadcast_to(idx, (B, H, idx.shape[-1]))
    return PT.expected_output(K, SPEC, idx), PT.expected_output(V, SPEC, idx)


def _new_outs(dtype, D, n=1):
    return [tuple(torch.full((B, H, N_OUT, D * TDT[dtype].itemsize), FILL, dtype=torch.uint8,
                             device=DEV).view(TDT[dtype]) for _ in range(2)) for _ in range(n)]


def _gather(dtype, D, table, idx, flag_list=(0,), dests=None, pages=None, bh=(B, H)):
    """PHASE_GATHER with external indices: plan, a 0xFF workspace with `idx` in its index rows,
    one launch per entry of flag_list; status 0."""
    B, H = bh
    shared = bool(flag_list[0] & N.FLAG_SHARED_INDEX)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = N.Params(dtype=DT[dtype], batch=B, heads=H, head_dim=D, order=PT.ASC, algo=PT.SORT,
                 phases=N.PHASE_GATHER, external_index=1, flags=flag_list[0],
                 device_status=status.data_ptr())
    rc, info = N.plan_paged(p, table, pages, dests)
    assert rc == 0, rc
    ws = torch.full((max(int(info.workspace_bytes), 256),), PT.POISON, dtype=torch.uint8,
                    device=DEV)
    rows = np.full((int(info.rows), int(info.index_row_stride)), -1, dtype=np.int32)
    for li, t in enumerate(table):
        r0 = int(t["row0"])
        for b in range(B):
            if shared:
                rows[r0 // H + b, :idx.shape[-1]] = idx[li, b, 0]
            else:
                rows[r0 + b * H:r0 + (b + 1) * H, :idx.shape[-1]] = idx[li, b]
    off = int(info.index_offset)
    ws[off:off + rows.size * 4].view(torch.int32).copy_(torch.from_numpy(rows.reshape(-1)))
    for flags in flag_list:
        p.flags = flags
        rc = N.launch_paged(p, table, pages, dests, ws.data_ptr(), int(info.workspace_bytes),
                            torch.cuda.current_stream().cuda_stream)
        assert rc == 0, (rc, flags)
    torch.cuda.synchronize()
    assert int(status.item()) == 0


def _dense_table(dev_layers, outs):
    from test_dest_gpu import _abi_table
    return _abi_table([SPEC] * len(outs), dev_layers, B, H, outs)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_kernel(dtype, D):
    """gather_kernel: all rows in one launch; the fixed and the selected rows as two launches
    over filled outputs, 30 layers so that the fixed rows' launch takes the capped looped grid
    (csrc/kvc.hip launch_gather: more than kFixedGatherBlocks = 512 blocks of kGatherTokens = 64
    rows); one index row shared by the heads of a layer."""
    K, V = _copy_inputs(dtype, D)
    dev = (to_dev(K, DEV), to_dev(V, DEV))
    for name, n, flag_list in (("all", 1, (0,)),
                               ("fixed | selected", 30,
                                (N.FLAG_GATHER_FIXED, N.FLAG_GATHER_SELECTED)),
                               ("shared index", 1, (N.FLAG_SHARED_INDEX,))):
        idx = _picks(len(name) + D, n, shared=name == "shared index")
        outs = _new_outs(dtype, D, n)
        if n > 1:
            fixed = SPEC["sink"] + SPEC["tail_len"]
            assert n * B * H * -(-fixed // 64) > 512
        _gather(dtype, D, _dense_table([dev] * n, outs), idx, flag_list)
        for li, (ko, vo) in enumerate(outs):
            wk, wv = _expected(dtype, D, idx[li])
            assert _same(ko, wk), (name, li, "K")
            assert _same(vo, wv), (name, li, "V")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_every_16_bit_value_in_either_half(dtype):
    """canon_nan_pk on the device over all 65 536 values of each half of a word: head 0 of
    [1, 2, 2050, 32] runs through every 16-bit pattern, head 1 through the same one element on;
    gathered once with identity indices and once every third row."""
    from test_dest_gpu import _abi_table
    S, D, Hh = 2050, 32, 2
    i = np.arange(S * D)
    X = prng.from_bits(np.stack([i % 65536, (i + 65535) % 65536]).astype(np.uint16)
                       .reshape(1, Hh, S, D), dtype)
    b = prng.to_bits(X)
    assert len(np.unique(b[..., 0::2])) == 65536 and len(np.unique(b[..., 1::2])) == 65536
    dev = (to_dev(X, DEV), to_dev(X, DEV))
    for idx in (np.arange(S), np.arange(0, S, 3)):
        s = PT.spec(S, zone_start=0, zone_len=S, n_select=len(idx))
        idx = np.broadcast_to(idx, (1, 1, Hh, len(idx)))
        outs = [tuple(torch.full((1, Hh, len(idx[0, 0, 0]), D * 2), FILL, dtype=torch.uint8,
                                 device=DEV).view(TDT[dtype]) for _ in range(2))]
        _gather(dtype, D, _abi_table([s], [dev], 1, Hh, outs), idx, bh=(1, Hh))
        want = PT.expected_output(X, s, idx[0])
        assert _same(outs[0][0], want) and _same(outs[0][1], want)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_dest_kernel(dtype, D):
    """gather_dest_kernel: into strided destinations (K stored [B, H, S, D], V [B, S, H, D],
    poison on both sides of the rows) and in place at the front of strided caches; the whole
    backing buffers are compared, so rows past n_out and the poison keep their bytes."""
    from test_dest_gpu import DST_START, _dest, _filled, _window
    K, V = _copy_inputs(dtype, D)
    dev = (to_dev(K, DEV), to_dev(V, DEV))
    idx = _picks(50 + D)
    wk, wv = _expected(dtype, D, idx[0])
    dests = np.zeros(1, dtype=N.DEST_DTYPE)
    # strided destinations
    dst = [_dest((B, H, N_OUT + 5, D), TDT[dtype], lay) for lay in ("static", "bshd")]
    was = [back.clone() for back, _ in dst]
    dests["k_stride"][0], dests["v_stride"][0] = dst[0][1].stride()[:3], dst[1][1].stride()[:3]
    _gather(dtype, D, _dense_table([dev], [(dst[0][1], dst[1][1])]), idx, dests=dests)
    for (back, _), exp, want, lay in zip(dst, was, (wk, wv), ("static", "bshd")):
        _window(exp, lay, N_OUT, DST_START[lay]).copy_(to_dev(want, DEV))
        assert torch.equal(_ints(back), _ints(exp)), ("strided", lay)
    # in place
    caches = [_filled(K, "static"), _filled(V, "bshd")]
    was = [back.clone() for back, _ in caches]
    win = (caches[0][1], caches[1][1])
    dests["k_stride"][0], dests["v_stride"][0] = win[0].stride()[:3], win[1].stride()[:3]
    dests["in_place"] = 1
    _gather(dtype, D, _dense_table([win], [win]), idx, dests=dests)
    for (back, _), exp, want, lay in zip(caches, was, (wk, wv), ("static", "bshd")):
        _window(exp, lay, N_OUT).copy_(to_dev(want, DEV))
        assert torch.equal(_ints(back), _ints(exp)), ("in place", lay)


@pytest.mark.parametrize("P", [1, 16])
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_paged_kernel(dtype, D, P):
    """gather_paged_kernel: pages -> dense outputs (the pools unchanged), and compaction into the
    leading pages through a shuffled block table (the whole pools compared)."""
    from test_paged_gpu import _abi_tables
    K, V = _copy_inputs(dtype, D)
    idx = _picks(70 + D + P)
    wk, wv = _expected(dtype, D, idx[0])
    pl = PU.Layer(K, V, P, 500 + D + P)
    snap = pl.snapshot()
    outs = _new_outs(dtype, D)
    table, pages = _abi_tables([SPEC], [pl], False, outs)
    _gather(dtype, D, table, idx, pages=pages)
    assert _same(outs[0][0], wk) and _same(outs[0][1], wv)
    pl.assert_pools(snap, ("dense", dtype, D, P))
    table, pages = _abi_tables([SPEC], [pl], True)
    _gather(dtype, D, table, idx, pages=pages)
    pl.expect(snap, wk, wv)
    pl.assert_pools(snap, ("in place", dtype, D, P))


SHORT = PT.spec(200, zone_start=10, zone_len=130, n_select=40, sink=2, tail_start=150, tail_len=9)


@pytest.mark.parametrize("beside", ["alone", "beside a shorter selecting layer"])
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_select_all_layer_still_rewrites(dtype, D, beside):
    """n_select == zone_len through KVC_PHASE_ALL: no selection runs, the zone is copied in order
    (gather_row with sel == nullptr; with KVC_FLAG_SPLIT_SELECT_GATHER an identity index row and
    gather_kernel) and still rewritten, the sink and tail not.  Alone in its call, and after a
    layer whose selecting zone (130 positions) is shorter than the kept one (500): the plan sizes
    the selection's arrays by the selecting layers alone.  (No registered method issues a
    select-all layer, so no reference golden holds one.)"""
    K, V = _copy_inputs(dtype, D)
    whole = dict(SPEC, n_select=SPEC["zone_len"])
    specs, host = [whole], [(K, V)]
    if beside != "alone":
        shape = (B, H, SHORT["S"], D)
        specs.insert(0, SHORT)
        host.insert(0, (prng.gen_keys(51000 + D, shape, dtype, "payload"),
                        prng.gen_values(0, shape, dtype, "patterns")))
    _check_phase_all(dtype, D, specs, host, (0, N.FLAG_SPLIT_SELECT_GATHER), (B, H))


def _check_phase_all(dtype, D, specs, host, flag_list, bh):
    """One KVC_PHASE_ALL launch per entry of flag_list (engine-selected indices) over filled
    outputs on a 0xFF workspace: every layer's K / V bytes against the CPU, status 0."""
    from test_dest_gpu import _abi_table
    B, H = bh
    dev = [(to_dev(k, DEV), to_dev(v, DEV)) for k, v in host]
    want = [PT.expected_layer(k, v, s, PT.ASC, PT.SORT) for (k, v), s in zip(host, specs)]
    for flags in flag_list:
        outs = [tuple(torch.full((B, H, PT.n_out(s), D * TDT[dtype].itemsize), FILL,
                                 dtype=torch.uint8, device=DEV).view(TDT[dtype])
                      for _ in range(2)) for s in specs]
        table = _abi_table(specs, dev, B, H, outs)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        p = N.Params(dtype=DT[dtype], batch=B, heads=H, head_dim=D, order=PT.ASC, algo=PT.SORT,
                     phases=N.PHASE_ALL, external_index=0, flags=flags,
                     device_status=status.data_ptr())
        rc, info = N.plan(p, table)
        assert rc == 0
        ws = torch.full((max(int(info.workspace_bytes), 256),), PT.POISON, dtype=torch.uint8,
                        device=DEV)
        assert N.launch(p, table, ws.data_ptr(), int(info.workspace_bytes),
                        torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert int(status.item()) == 0, flags
        for li, ((ko, vo), (wk, wv, _)) in enumerate(zip(outs, want)):
            assert _same(ko, wk), (flags, li, "K")
            assert _same(vo, wv), (flags, li, "V")


@pytest.mark.parametrize("zone", [16448, 65600])
def test_select_all_zone_past_a_long_selecting_zone(zone):
    """The same beside a selecting zone past the LDS limit, the kept zone 500 positions longer
    still: the global-scratch selection kernels (u16 positions at 16 448, u32 positions at
    65 600) write the identity index row of a kept zone longer than their scratch rows."""
    Bq, Hq, D, dtype = 1, 2, 32, "bf16"
    sel = PT.spec(zone + 20, zone_start=4, zone_len=zone, n_select=zone // 3, sink=4,
                  tail_start=zone + 8, tail_len=9)
    whole = PT.spec(zone + 600, zone_start=30, zone_len=zone + 500, n_select=zone + 500, sink=4,
                    tail_start=zone + 540, tail_len=50)
    shape = (Bq, Hq, sel["S"], D)
    V = prng.gen_values(0, (Bq, Hq, whole["S"], D), dtype, "patterns")
    host = [(prng.gen_keys(51500 + zone, shape, dtype, "payload"),
             prng.gen_values(0, shape, dtype, "patterns")),
            (np.ascontiguousarray(np.roll(V, 101, axis=2)), V)]
    _check_phase_all(dtype, D, [sel, whole], host, (0,), (Bq, Hq))


# ------------------------------------------------------------------------------------------
# b. the fused select_gather_kernel, through the methods
# ------------------------------------------------------------------------------------------
def _method(name):
    from kvcompress.methods import get_compress_fn
    return get_compress_fn(name)


_V = {}


def _values(shape, dtype):
    key = (shape, dtype)
    if key not in _V:
        _V.clear()
        _V[key] = prng.gen_values(0, shape, dtype, "patterns")
    return _V[key]


def _layers(shape, dtype, seed, n=1):
    """n layers of "payload" keys and "patterns" values (layer i's values start 13 * i rows on)."""
    V = _values(shape, dtype)
    return [(prng.gen_keys(seed + i, shape, dtype, "payload"),
             V if i == 0 else np.ascontiguousarray(np.roll(V, 13 * i, axis=2))) for i in range(n)]


def _check_method(name, kw, layers, what=()):
    tin = [(to_dev(k, DEV), to_dev(v, DEV)) for k, v in layers]
    out = _method(name)(list(tin), **kw)
    torch.cuda.synchronize()
    ref = oracle.METHODS[name](layers, **kw)
    assert len(out) == len(ref)
    for li, ((ki, vi), (ko, vo), (rk, rv, kind)) in enumerate(zip(tin, out, ref)):
        ctx = (name, li) + tuple(what)
        assert kind_of(ki, ko) == kind, ctx
        assert _same(ko, rk), ctx + ("K",)
        assert _same(vo, rv), ctx + ("V",)
    _engine_status_clear()
    return ref


SHAPE = (2, 3, 1500, 64)
METHODS_512 = (
    ("h2o_l2", dict(start_size=4, heavy_hitter_size=1200, recent_size=200, skip_layers=[])),
    ("fix_size_l2", dict(fix_kv_size=1400, keep_ratio=0.0, skip_layers=[])),
    ("snapkv_lite", dict(observation_window=32, keep_size=1200, pooling_kernel=5,
                         skip_layers=[])),
)


@pytest.fixture(params=["fused", "separate", "stable", "replay"])
def path(request, monkeypatch):
    """The launch paths of a method call: SCORE + SELECT_GATHER (default), SCORE / SELECT / GATHER
    as three kernels, the stable tie policy (engine and oracle alike), and the same call three
    times -- the third is replayed natively (kvc_host)."""
    from kvcompress import _engine
    _engine.call_memo.clear()
    if request.param == "separate":
        monkeypatch.setattr(_engine, "split_select_gather", True)
    if request.param == "stable":
        monkeypatch.setattr(_engine, "tie_policy", "stable")
        monkeypatch.setattr(oracle, "TIE", "stable")
    return request.param


@pytest.mark.parametrize("name, kw", METHODS_512, ids=[m[0] for m in METHODS_512])
@pytest.mark.parametrize("dtype", DTYPES)
def test_select_gather_512_thread_rows(dtype, name, kw, path):
    """sink + zone + tail (h2o_l2), a zone alone (fix_size_l2, keep_ratio 0) and topk order
    (snapkv_lite) on [2, 3, 1500, 64]; the selections keep most of the zone, NaN-norm rows
    included."""
    from kvcompress import _engine
    before = _engine.memo_stats["replayed"]
    for rep in range(3 if path == "replay" else 1):
        ref = _check_method(name, kw, _layers(SHAPE, dtype, 52000 + 10 * rep), (dtype, path, rep))
        assert ref[0][2] == "new"
    if path == "replay" and _engine.host_module() is not None:
        assert _engine.memo_stats["replayed"] > before


@pytest.mark.parametrize("dtype", DTYPES)
def test_select_gather_1024_thread_rows_split_copy(dtype):
    """A zone of 8 260 positions with sink and tail, 4 rows: the selecting workgroups copy the
    selected rows (PART_SELECTED), copy-only workgroups the sink and tail (PART_FIXED)."""
    kw = dict(start_size=4, heavy_hitter_size=7800, recent_size=200, skip_layers=[])
    _check_method("h2o_l2", kw, _layers((1, 4, 8464, 32), dtype, 53000), (dtype,))


def test_select_gather_1024_thread_rows_one_workgroup():
    """More than 255 rows (4 layers of [1, 64, 8464, 32], bf16): each row's workgroup selects and
    copies the whole row."""
    kw = dict(start_size=4, heavy_hitter_size=7800, recent_size=200, skip_layers=[])
    _check_method("h2o_l2", kw, _layers((1, 64, 8464, 32), "bf16", 53100, n=4))


@pytest.mark.parametrize("dtype", DTYPES)
def test_zone_over_the_lds_limit(dtype):
    """A zone of 17 000 positions: the global-scratch selection, then gather_kernel."""
    kw = dict(fix_kv_size=16000, keep_ratio=0.0, skip_layers=[])
    _check_method("fix_size_l2", kw, _layers((1, 2, 17000, 32), dtype, 53200), (dtype,))


# ------------------------------------------------------------------------------------------
# c. the Python delivery paths
# ------------------------------------------------------------------------------------------
DELIVERY = (METHODS_512[0], METHODS_512[2])


@pytest.mark.parametrize("name, kw", DELIVERY, ids=[m[0] for m in DELIVERY])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_delivery_paths(dtype, name, kw):
    """out="inplace" on windows of static caches, strided out=[(K, V)], compress_paged in place
    (P = 16) and into dense views: the bytes of the default call's oracle result, and nothing
    else written."""
    from kvcompress import compress_paged
    from test_dest_gpu import DST_START, _dest, _filled, _window
    (K, V), = _layers(SHAPE, dtype, 54000)
    (rk, rv, kind), = oracle.METHODS[name]([(K, V)], **kw)
    n = rk.shape[2]
    assert kind == "new"
    lays = ("static", "bshd")
    # in place at the front of strided caches
    caches = [_filled(K, "static"), _filled(V, "bshd")]
    was = [back.clone() for back, _ in caches]
    out = _method(name)([(caches[0][1], caches[1][1])], out="inplace", **kw)
    torch.cuda.synchronize()
    for j, (want, lay) in enumerate(zip((rk, rv), lays)):
        assert out[0][j].data_ptr() == caches[j][1].data_ptr() and _same(out[0][j], want)
        _window(was[j], lay, n).copy_(to_dev(want, DEV))
        assert torch.equal(_ints(caches[j][0]), _ints(was[j])), ("inplace", lay)
    # strided destinations
    tin = (to_dev(K, DEV), to_dev(V, DEV))
    dst = [_dest((B, H, n + 5, SHAPE[3]), TDT[dtype], lay) for lay in lays]
    was = [back.clone() for back, _ in dst]
    out = _method(name)([tin], out=[(dst[0][1], dst[1][1])], **kw)
    torch.cuda.synchronize()
    for j, (want, lay) in enumerate(zip((rk, rv), lays)):
        assert out[0][j].data_ptr() == dst[j][1].data_ptr() and _same(out[0][j], want)
        _window(was[j], lay, n, DST_START[lay]).copy_(to_dev(want, DEV))
        assert torch.equal(_ints(dst[j][0]), _ints(was[j])), ("strided", lay)
    assert _same(tin[0], K) and _same(tin[1], V)
    # pages -> dense views
    pl = PU.Layer(K, V, 16, 54100)
    snap = pl.snapshot()
    dst = [_dest((B, H, n + 5, SHAPE[3]), TDT[dtype], lay) for lay in lays]
    was = [back.clone() for back, _ in dst]
    out = compress_paged(name, [pl.paged], out=[(dst[0][1], dst[1][1])], **kw)
    torch.cuda.synchronize()
    for j, (want, lay) in enumerate(zip((rk, rv), lays)):
        assert _same(out[0][j], want)
        _window(was[j], lay, n, DST_START[lay]).copy_(to_dev(want, DEV))
        assert torch.equal(_ints(dst[j][0]), _ints(was[j])), ("paged -> dense", lay)
    pl.assert_pools(snap, ("paged -> dense",))
    # pages, in place
    lens = compress_paged(name, [pl.paged], **kw)
    torch.cuda.synchronize()
    assert lens == [n]
    pl.expect(snap, rk, rv)
    pl.assert_pools(snap, ("paged in place",))
    _engine_status_clear()


# ------------------------------------------------------------------------------------------
# d. h2o_attention: the fixed rows copied beside the heavy-hitter selection
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_h2o_attention_manager_steps(dtype):
    """A prefill-shaped step (8 queries) and three decode-shaped ones (repeated step shapes go
    through the engine's native step replay where it plans them) on a middle zone past
    OVERLAP_MIN_ZONE: heavy hitters from the manager through the shared index, the sink and tail
    rows copied beside the selection; accumulations and K / V bytes against the oracle's manager
    per step."""
    import h2o_inputs
    from kvcompress.methods import h2o_attention as HA
    from oracle import h2o_oracle as HO
    Hh, S, D, L = 4, 4700, 64, 2
    kw = dict(start_size=4, heavy_hitter_size=64, recent_size=444)
    assert S - 4 - 444 >= HA.OVERLAP_MIN_ZONE
    kv = _layers((1, Hh, S, D), dtype, 55000, n=L)
    kvd = [(to_dev(k, DEV), to_dev(v, DEV)) for k, v in kv]
    mgr = HA.H2OAttentionManager(num_layers=L, num_heads=Hh, **kw)
    mgr.reduction_threads = 8
    omgr = HO.H2OManager(threads=8, **kw)
    HA.step_memo.clear()
    for st in range(4):
        q = 8 if st == 0 else 1
        atts = [h2o_inputs.attention(55100 + 10 * st + li, Hh, q, S, dtype) for li in range(L)]
        out = HA.h2o_attention_compress(list(kvd), attention_scores=tuple(to_dev(a, DEV) for a in atts),
                                        h2o_manager=mgr, skip_layers=[], **kw)
        torch.cuda.synchronize()
        ref = HO.h2o_attention_compress(kv, atts, omgr, skip_layers=[], **kw)
        for li in range(L):
            assert _same(mgr.accumulated_attention[li], omgr.acc[li]), (st, li, "acc")
            assert _same(out[li][0], ref[li][0]), (st, li, "K")
            assert _same(out[li][1], ref[li][1]), (st, li, "V")
            assert ref[li][0].shape[2] == 4 + 64 + 444
    _engine_status_clear()


# ------------------------------------------------------------------------------------------
# e. a seeded sweep: the fuzz generator's cases on these bytes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(48))
def test_random_configs_on_nan_payloads(case, monkeypatch):
    """tests/test_gpu_fuzz.py's seeded cases (layers of at most 3 000 positions) with "patterns"
    values and the "payload" NaNs written into their keys: D = 32 .. 256, the three dtypes,
    ragged multi-layer calls and every method; the launch paths take turns."""
    from kvcompress import _engine
    from test_gpu_fuzz import _check, _gen_case
    monkeypatch.setattr(_engine, "split_select_gather", case % 2 == 1)
    method, layers, kw, dtype, D = _gen_case(case, max_len=3000)
    layers = [(prng.inject_payload(k, dtype), prng.gen_values(0, k.shape, dtype, "patterns"))
              for k, _ in layers]
    _check(case, method, layers, kw, dtype, D)
    _engine_status_clear()
