"""Compression of paged caches on the GPU (include/kvc.h, "Paged caches"; kvcompress.PagedKV /
compress_paged): compaction into the leading pages through shuffled block tables, dense
destinations, and the two C entries.

Expected bytes come from the CPU oracle on the dense numpy inputs (tests/dest_cases.py); that the
in-place cases cannot pass with the table ignored or misread is shown in tests/test_paged_order.py.
Pools and checks: tests/paged_util.py.
"""
import numpy as np
import pytest
import torch

import dest_cases as DC
import paged_util as PU
import phase_tables as PT
import prng
from gpu_util import to_dev, to_np
from kvcompress import _native as N

pytestmark = pytest.mark.gpu

DEV = PU.DEV


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _policy(monkeypatch, case):
    from kvcompress import _engine
    monkeypatch.setattr(_engine, "tie_policy", case["tie"])


def _layers(case, P, tagged, fill=0):
    layers, ref = DC.reference(case, tagged=tagged, fill=fill)
    pls = [PU.Layer(k, v, P, case["seed"] + 7 * li + fill) for li, (k, v) in enumerate(layers)]
    return pls, ref


def _check_inplace(case, P, fill=0):
    from kvcompress import compress_paged
    pls, ref = _layers(case, P, True, fill)
    snaps = [pl.snapshot() for pl in pls]
    lens = compress_paged(case["method"], [pl.paged for pl in pls], **case["kw"])
    torch.cuda.synchronize()
    assert len(lens) == len(ref)
    for li, (pl, snap, n, (rk, rv, kind)) in enumerate(zip(pls, snaps, lens, ref)):
        ctx = (case["id"], P, fill, li, kind)
        if kind == "same":
            assert n == pl.S, ctx
        else:
            assert n == rk.shape[2], ctx
            pl.expect(snap, rk, rv)
            kd, vd = pl.paged.to_dense(n)
            assert np.array_equal(_bytes(to_np(kd)), _bytes(rk)), ctx + ("to_dense K",)
            assert np.array_equal(_bytes(to_np(vd)), _bytes(rv)), ctx + ("to_dense V",)
        pl.assert_pools(snap, ctx)


EXTRA = ("streaming_llm-shift1", "h2o_l2-4-64-444-D32", "pyramid_kv-512-6layers")
CASES = [(c, P) for c in DC.INPLACE for P in (16, 128)] + \
        [(c, P) for c in DC.INPLACE if c["id"] in EXTRA for P in (1, 4096)]


@pytest.mark.parametrize("case, P", CASES, ids=[f"{c['id']}-P{P}" for c, P in CASES])
def test_compaction_into_the_leading_pages(case, P, monkeypatch):
    """1: every in-place case; those with repeat = 3 run three times on freshly filled pools."""
    _policy(monkeypatch, case)
    for fill in range(case["repeat"]):
        _check_inplace(case, P, fill)


@pytest.mark.parametrize("case", DC.STRIDED, ids=[c["id"] for c in DC.STRIDED])
def test_dense_destinations(case, monkeypatch):
    """2: pages -> strided dense views (K destination stored [B, H, S, D], V [B, S, H, D]); the
    pools stay entirely unchanged."""
    from kvcompress import compress_paged
    from test_dest_gpu import DST_START, _dest, _window
    _policy(monkeypatch, case)
    pls, ref = _layers(case, 16, False)
    snaps = [pl.snapshot() for pl in pls]
    dst = []
    for pl, (rk, rv, kind) in zip(pls, ref):
        B, H, _, D = pl.paged.shape
        shape = (B, H, rk.shape[2] + 5, D)
        dst.append((_dest(shape, pl.k.dtype, "static"), _dest(shape, pl.k.dtype, "bshd")))
    dwas = [(kd[0].clone(), vd[0].clone()) for kd, vd in dst]
    out = compress_paged(case["method"], [pl.paged for pl in pls],
                         out=[(kd[1], vd[1]) for kd, vd in dst], **case["kw"])
    torch.cuda.synchronize()
    for li, ((ko, vo), (rk, rv, kind)) in enumerate(zip(out, ref)):
        n = rk.shape[2]
        for j, (y, want, layout) in enumerate(((ko, rk, "static"), (vo, rv, "bshd"))):
            ctx = (case["id"], li, kind, layout)
            back, win = dst[li][j]
            assert y.data_ptr() == win.data_ptr() and y.stride() == win.stride(), ctx
            assert tuple(y.shape) == want.shape, ctx
            assert np.array_equal(_bytes(to_np(y)), _bytes(want)), ctx
            exp = dwas[li][j]
            _window(exp, layout, n, DST_START[layout]).copy_(to_dev(want, DEV))
            assert torch.equal(PU.ints(back), PU.ints(exp)), ctx + ("poison around the rows",)
        pls[li].assert_pools(snaps[li], (case["id"], li, "pool unchanged"))


def test_random_strategy_in_place():
    """3: caller-side indices; the same seeded draw on the dense tensor gives the expected rows."""
    from kvcompress import compress_paged
    from kvcompress.methods import fix_size_l2_compress
    shape = (DC.B, DC.H, 1500, 64)
    kn, vn = prng.gen_keys(42090, shape, "bf16"), prng.encode_positions(shape, "bf16")
    pl = PU.Layer(kn, vn, 16, 42090)
    kw = dict(fix_kv_size=512, keep_ratio=0.25, strategy="random", skip_layers=[])
    torch.manual_seed(77)
    want = fix_size_l2_compress([(to_dev(kn, DEV), to_dev(vn, DEV))], **kw)
    snap = pl.snapshot()
    torch.manual_seed(77)
    lens = compress_paged("fix_size_l2", [pl.paged], **kw)
    torch.cuda.synchronize()
    assert lens == [512] and want[0][0].shape[2] == 512
    pl.expect(snap, to_np(want[0][0]), to_np(want[0][1]))
    pl.assert_pools(snap, ("random",))
    pos, ok = prng.decode_positions(to_np(pl.paged.to_dense(512)[1]), "bf16")
    assert ok and (np.diff(pos, axis=2) > 0).all() and not (pos[0, 0] == pos[1, 2]).all()


def test_shared_prefix_page():
    """4: both batch rows' table entry 0 names ONE page (P = 4 = start_size: it holds the sink
    rows only, which are never written)."""
    from kvcompress import compress_paged
    from oracle import oracle
    shape = (2, 3, 600, 64)
    kn, vn = prng.gen_keys(42100, shape, "bf16"), prng.gen_values(42100, shape, "bf16")
    kn[1, :, :4], vn[1, :, :4] = kn[0, :, :4], vn[0, :, :4]
    table, n_pages = PU.page_table(2, 600, 4, 42100)
    table[1, 0] = table[0, 0]
    pl = PU.Layer(kn, vn, 4, 0, table=table, n_pages=n_pages)
    kw = dict(start_size=4, heavy_hitter_size=64, recent_size=100, skip_layers=[])
    (rk, rv, kind), = oracle.METHODS["h2o_l2"]([(kn, vn)], **kw)
    snap = pl.snapshot()
    lens = compress_paged("h2o_l2", [pl.paged], **kw)
    torch.cuda.synchronize()
    assert lens == [168] and rk.shape[2] == 168
    pl.expect(snap, rk[:, :, 4:], rv[:, :, 4:], first=4)
    pl.assert_pools(snap, ("shared prefix",))
    kd, vd = pl.paged.to_dense(168)
    assert np.array_equal(_bytes(to_np(kd)), _bytes(rk)) and np.array_equal(_bytes(to_np(vd)), _bytes(rv))


def test_h2o_attention_without_a_manager_and_errors():
    """h2o_attention without a manager selects L2 heavy hitters; with one it is refused.  A bad
    layer leaves every pool of the call untouched."""
    from kvcompress import compress_paged
    from kvcompress.methods import h2o_attention as HA
    from oracle import oracle
    shape = (2, 3, 600, 64)
    layers = [(prng.gen_keys(42200 + i, shape, "bf16"), prng.gen_values(42200 + i, shape, "bf16"))
              for i in range(2)]
    pls = [PU.Layer(k, v, 16, 42200 + i) for i, (k, v) in enumerate(layers)]
    snaps = [pl.snapshot() for pl in pls]
    kw = dict(start_size=4, heavy_hitter_size=64, recent_size=100)
    with pytest.raises(TypeError, match="H2OAttentionManager"):
        compress_paged("h2o_attention", [pl.paged for pl in pls],
                       h2o_manager=HA.H2OAttentionManager(**kw), **kw)
    with pytest.raises(ValueError, match="layer 0: cannot be compacted in place"):
        compress_paged("streaming_llm", [pl.paged for pl in pls], start_size=4, recent_size=0)
    short = tuple(torch.zeros(2, 3, 167, 64, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    with pytest.raises(ValueError, match="layer 1: K destination holds 167 rows, the result has 168"):
        compress_paged("h2o_l2", [pl.paged for pl in pls], out=[None, short], skip_layers=[], **kw)
    inside = pls[1].kb[:2, :, :, :].reshape(2, 3, 16, 64)
    with pytest.raises(ValueError, match="layer 1: K destination overlaps the layer's K pool"):
        compress_paged("recent_only", [pl.paged for pl in pls], window_size=16, skip_layers=[],
                       out=[None, (inside, torch.zeros_like(inside))])
    torch.cuda.synchronize()
    for pl, snap in zip(pls, snaps):
        pl.assert_pools(snap, ("after errors",))
    assert not short[0].any() and not short[1].any()
    ref = oracle.METHODS["h2o_l2"](layers, skip_layers=[], **kw)
    lens = compress_paged("h2o_attention", [pl.paged for pl in pls], **kw)
    torch.cuda.synchronize()
    assert lens == [168, 168]
    for pl, snap, (rk, rv, _) in zip(pls, snaps, ref):
        pl.expect(snap, rk, rv)
        pl.assert_pools(snap, ("h2o_attention",))


def test_status_check_reports_a_bad_page_id():
    """Paged calls go through the opt-in status check: a table entry one past the pool is clamped
    for the loads, the stores through it are dropped, and the call raises naming the bit."""
    from kvcompress import _engine as E
    from kvcompress import compress_paged
    shape = (1, 2, 600, 64)
    pl = PU.Layer(prng.gen_keys(42300, shape, "bf16"), prng.gen_values(42300, shape, "bf16"), 16,
                  42300)
    bad_page = int(pl.table[0, 5])
    pl.table[0, 5] = pl.k.size(0)
    snap = pl.snapshot()
    prev = E.set_status_check(True)
    try:
        with pytest.raises(RuntimeError, match="KVC_DEV_INDEX_RANGE"):
            compress_paged("fix_size_l2", [pl.paged], fix_kv_size=100, keep_ratio=0.25,
                           skip_layers=[])
    finally:
        E.set_status_check(prev)
    assert E.device_status(0) == 0  # read and cleared by the check
    # output rows [80, 96) had no valid page: the page they used to live in keeps its bytes
    assert torch.equal(PU.ints(pl.kb[bad_page]), PU.ints(snap[0][bad_page]))
    assert torch.equal(PU.ints(pl.vb[bad_page]), PU.ints(snap[1][bad_page]))


# ---- the C entries ----------------------------------------------------------------------------
D_ABI = 64


def _abi_tables(specs, pls, inplace, outs=None, num_pages=None):
    table = np.zeros(len(specs), dtype=N.LAYER_DTYPE)
    pages = np.zeros(len(specs), dtype=N.PAGES_DTYPE)
    for i, (t, s, pl) in enumerate(zip(table, specs, pls)):
        t["k"], t["v"] = pl.k.data_ptr(), pl.v.data_ptr()
        t["k_out"], t["v_out"] = (t["k"], t["v"]) if inplace else \
            (outs[i][0].data_ptr(), outs[i][1].data_ptr())
        t["k_stride"] = (0,) + tuple(pl.k.stride()[1:3])
        t["v_stride"] = (0,) + tuple(pl.v.stride()[1:3])
        t["seq_len"], t["zone_start"], t["zone_len"] = s["S"], s["zone_start"], s["zone_len"]
        t["n_select"], t["sink_len"] = s["n_select"], s["sink"]
        t["tail_start"], t["tail_len"] = s["tail_start"], s["tail_len"]
        t["score_mode"], t["pool_kernel"] = s["score_mode"], s["pool"]
        pages[i] = (pl.table.data_ptr(), pl.table.stride(0), pl.k.stride(0), pl.v.stride(0), pl.P,
                    pl.k.size(0) if num_pages is None else num_pages, int(inplace), 0)
    return table, pages


def _params(B, H, status, order=PT.ASC, algo=PT.SORT, **kw):
    d = dict(dtype=N.KVC_BF16, batch=B, heads=H, head_dim=D_ABI, order=order, algo=algo,
             phases=N.PHASE_ALL, external_index=0, flags=0, device_status=status.data_ptr())
    d.update(kw)
    return N.Params(**d)


def _workspace(info):
    return torch.full((max(int(info.workspace_bytes), 256),), PT.POISON, dtype=torch.uint8,
                      device=DEV)


@pytest.mark.parametrize("mode", ["h2o_l2", "snapkv"])
def test_c_abi_separate_phases(mode):
    """5: SCORE, SELECT and GATHER launched one by one on a 0xFF-filled workspace equal one
    launch, in place (through the table) and into contiguous outputs, and equal the oracle."""
    Z = 1000
    B, H = PT.split_geometry(Z)
    if mode == "snapkv":
        specs, order, algo = PT.split_table(Z, PT.SNAPKV, 5), PT.DESC, PT.TOPK
    else:
        specs, order, algo = PT.split_table(Z), PT.ASC, PT.SORT
    host = PT.gen_layers(specs, B, H, D_ABI, "bf16")
    want = [PT.expected_layer(k, v, s, order, algo) for (k, v), s in zip(host, specs)]
    stream = torch.cuda.current_stream().cuda_stream
    for inplace in (True, False):
        for phase_list in ((N.PHASE_SCORE, N.PHASE_SELECT, N.PHASE_GATHER), (N.PHASE_ALL,)):
            pls = [PU.Layer(k, v, 16, 43000 + i) for i, (k, v) in enumerate(host)]
            snaps = [pl.snapshot() for pl in pls]
            outs = [tuple(torch.zeros((B, H, PT.n_out(s), D_ABI), dtype=torch.bfloat16, device=DEV)
                          for _ in range(2)) for s in specs]
            table, pages = _abi_tables(specs, pls, inplace, outs)
            status = torch.zeros(1, dtype=torch.int32, device=DEV)
            p = _params(B, H, status, order, algo)
            rc, info = N.plan_paged(p, table, pages, None)
            assert rc == 0
            ws = _workspace(info)
            for ph in phase_list:
                p.phases = ph
                rc = N.launch_paged(p, table, pages, None, ws.data_ptr(),
                                    int(info.workspace_bytes), stream)
                assert rc == 0, ph
            torch.cuda.synchronize()
            assert int(status.item()) == 0
            for li, (pl, snap, (wk, wv, _), s) in enumerate(zip(pls, snaps, want, specs)):
                ctx = (mode, inplace, len(phase_list), li)
                if inplace:
                    pl.expect(snap, wk, wv)
                else:
                    assert np.array_equal(_bytes(to_np(outs[li][0])), _bytes(wk)), ctx
                    assert np.array_equal(_bytes(to_np(outs[li][1])), _bytes(wv)), ctx
                pl.assert_pools(snap, ctx)


def test_c_abi_chunks_shared_index_and_wide_table():
    """6: 65 layers [1, 1, S_i, 64] with a page permutation each (more than one argument chunk),
    KVC_FLAG_SHARED_INDEX with caller indices, block tables wider than needed."""
    specs = PT.chunk_table(65)
    B, H = 1, 1
    host = PT.gen_layers(specs, B, H, D_ABI, "bf16")
    stream = torch.cuda.current_stream().cuda_stream
    # engine-selected, in place
    want = [PT.expected_layer(k, v, s, PT.ASC, PT.SORT) for (k, v), s in zip(host, specs)]
    pls = [PU.Layer(k, v, 16, 44000 + i, table_cols=20) for i, (k, v) in enumerate(host)]
    assert len({tuple(pl.table_np.reshape(-1)[:4]) for pl in pls}) > 32
    snaps = [pl.snapshot() for pl in pls]
    table, pages = _abi_tables(specs, pls, True)
    assert all(int(g["table_stride"]) == 20 for g in pages)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = _params(B, H, status)
    rc, info = N.plan_paged(p, table, pages, None)
    assert rc == 0
    ws = _workspace(info)
    assert N.launch_paged(p, table, pages, None, ws.data_ptr(), int(info.workspace_bytes),
                          stream) == 0
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    for li, (pl, snap, (wk, wv, _)) in enumerate(zip(pls, snaps, want)):
        pl.expect(snap, wk, wv)
        pl.assert_pools(snap, ("chunks", li))
    # caller indices shared by the heads of a layer (H = 2), into contiguous outputs
    H = 2
    host = PT.gen_layers(specs, B, H, D_ABI, "bf16")
    pls = [PU.Layer(k, v, 16, 45000 + i, table_cols=20) for i, (k, v) in enumerate(host)]
    snaps = [pl.snapshot() for pl in pls]
    outs = [tuple(torch.zeros((B, H, PT.n_out(s), D_ABI), dtype=torch.bfloat16, device=DEV)
                  for _ in range(2)) for s in specs]
    table, pages = _abi_tables(specs, pls, False, outs)
    p = _params(B, H, status, external_index=1, phases=N.PHASE_GATHER, flags=N.FLAG_SHARED_INDEX)
    rc, info = N.plan_paged(p, table, pages, None)
    assert rc == 0
    ws = _workspace(info)
    istride = int(info.index_row_stride)
    rng = np.random.default_rng(6)
    idx_rows = np.full((len(specs) * B, istride), -1, dtype=np.int32)
    shared = []
    for li, s in enumerate(specs):
        idx = np.sort(rng.choice(s["zone_len"], s["n_select"], replace=False)).astype(np.int64)
        idx_rows[li, :len(idx)] = idx
        shared.append(np.broadcast_to(idx, (B, H, len(idx))).copy())
    region = ws[info.index_offset:info.index_offset + idx_rows.size * 4].view(torch.int32)
    region.copy_(torch.from_numpy(idx_rows.reshape(-1)).to(DEV))
    assert N.launch_paged(p, table, pages, None, ws.data_ptr(), int(info.workspace_bytes),
                          stream) == 0
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    for li, ((k, v), s, idx) in enumerate(zip(host, specs, shared)):
        assert np.array_equal(_bytes(to_np(outs[li][0])), _bytes(PT.expected_output(k, s, idx))), li
        assert np.array_equal(_bytes(to_np(outs[li][1])), _bytes(PT.expected_output(v, s, idx))), li
        pls[li].assert_pools(snaps[li], ("shared index", li))


IDENTITY_CASES = [("bf16", 80, PT.NORM), ("bf16", 32, PT.NORM), ("fp32", 128, PT.NORM),
                  ("fp16", 128, PT.SNAPKV)]


@pytest.mark.parametrize("dt, D, score_mode", IDENTITY_CASES,
                         ids=[f"{dt}-D{D}" + ("-snapkv" if m == PT.SNAPKV else "")
                              for dt, D, m in IDENTITY_CASES])
def test_identity_table_equals_dense(dt, D, score_mode):
    """The paged kernels differ from the dense ones in address arithmetic only: SCORE + SELECT +
    GATHER of one dense [1, H, S, D] K / V, and the same call through kvc_launch_paged over the
    SAME memory with the identity block table (page i = rows [iP, (i+1)P), page stride
    P * k_stride[2]), leave byte-identical norms, tile maxima (snapkv), indices and outputs.
    Zone [5, 135): three tiles, the last of 2 tokens, from the middle of page 0 over nine pages."""
    H, S, P = 2, 200, 16
    s = PT.spec(S, zone_start=5, zone_len=130, n_select=40, sink=3, tail_start=190, tail_len=10,
                score_mode=score_mode, pool=5 if score_mode == PT.SNAPKV else 0)
    order, algo = (PT.DESC, PT.TOPK) if score_mode == PT.SNAPKV else (PT.ASC, PT.SORT)
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[dt]
    esz = 4 if dt == "fp32" else 2
    # the last page's slots reach 8 rows past S: backed, so that nothing else lives there
    kv = []
    for gen in (lambda: prng.gen_keys(48000 + D, (1, H, S, D), dt, "normal"),
                lambda: prng.gen_values(48000 + D, (1, H, S, D), dt)):
        flat = torch.zeros(H * S * D + P * D, dtype=tdt, device=DEV)
        flat[:H * S * D] = to_dev(gen(), DEV).reshape(-1)
        kv.append(flat[:H * S * D].view(1, H, S, D))
    k, v = kv
    n_pages = (S + P - 1) // P
    block_table = torch.arange(n_pages, dtype=torch.int32, device=DEV).view(1, n_pages)
    stream = torch.cuda.current_stream().cuda_stream
    runs = []
    for paged in (False, True):
        outs = tuple(torch.zeros((1, H, PT.n_out(s), D), dtype=tdt, device=DEV) for _ in range(2))
        table = np.zeros(1, dtype=N.LAYER_DTYPE)
        t = table[0]
        t["k"], t["v"], t["k_out"], t["v_out"] = (x.data_ptr() for x in (k, v) + outs)
        t["k_stride"] = t["v_stride"] = (0 if paged else H * S * D, S * D, D)
        t["seq_len"], t["zone_start"], t["zone_len"] = S, s["zone_start"], s["zone_len"]
        t["n_select"], t["sink_len"] = s["n_select"], s["sink"]
        t["tail_start"], t["tail_len"] = s["tail_start"], s["tail_len"]
        t["score_mode"], t["pool_kernel"] = s["score_mode"], s["pool"]
        pages = None
        if paged:
            pages = np.zeros(1, dtype=N.PAGES_DTYPE)
            pages[0] = (block_table.data_ptr(), n_pages, P * D, P * D, P, n_pages, 0, 0)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        # SELECT and GATHER as two kernels in the dense run too: the index region is written
        p = _params(1, H, status, order, algo, head_dim=D, flags=N.FLAG_SPLIT_SELECT_GATHER,
                    dtype={"bf16": N.KVC_BF16, "fp16": N.KVC_F16, "fp32": N.KVC_F32}[dt])
        rc, info = N.plan_paged(p, table, pages, None)
        assert rc == 0, (paged, rc)
        ws = _workspace(info)
        assert N.launch_paged(p, table, pages, None, ws.data_ptr(), int(info.workspace_bytes),
                              stream) == 0, paged
        torch.cuda.synchronize()
        assert int(status.item()) == 0, paged
        rows, ns, istr = int(info.rows), int(info.norm_row_stride), int(info.index_row_stride)
        w = ws.cpu().numpy()
        norms = w[info.norm_offset:info.norm_offset + rows * ns * esz].reshape(rows, ns * esz)
        index = w[info.index_offset:info.index_offset + rows * istr * 4]
        toff = (info.index_offset + rows * istr * 4 + 255) // 256 * 256  # csrc/kvc.hip tmax_offset
        tmax = w[toff:toff + rows * (ns // 64) * 4]
        runs.append(dict(norms=norms[:, :s["zone_len"] * esz].copy(), index=index.copy(),
                         tmax=tmax.copy(), k=_bytes(to_np(outs[0])), v=_bytes(to_np(outs[1])),
                         layout=(rows, ns, istr, int(info.workspace_bytes))))
    dense, paged = runs
    assert dense["layout"] == paged["layout"]
    assert dense["index"].view(np.int32).reshape(H, -1)[:, :s["n_select"]].min() >= 0
    for name in ("norms", "index", "k", "v") + (("tmax",) if score_mode == PT.SNAPKV else ()):
        assert dense[name].size and np.array_equal(dense[name], paged[name]), name


@pytest.mark.parametrize("mode", ["copy", "inplace", "select"])
def test_bad_page_id_is_clamped_for_loads_and_dropped_for_stores(mode):
    """7: N pages allocated, num_pages = N - 4 declared, the table's entry of logical page 1 is
    N - 2 (present in memory: an unclamped kernel would read it without a fault).  Loads -- of the
    copy and, in mode "select", of SCORE -- come from page num_pages - 1; an in-place store
    through the bad id is dropped."""
    B, H, S, P = 1, 2, 64, 16
    inplace = mode == "inplace"
    if mode == "select":
        s = PT.spec(S, zone_start=0, zone_len=64, n_select=40, variant="normal")
    else:
        s = PT.spec(S, zone_start=0, zone_len=0, n_select=0, sink=0, tail_start=8, tail_len=40)
    kn = prng.gen_keys(46000, (B, H, S, D_ABI), "bf16")
    vn = prng.gen_values(46000, (B, H, S, D_ABI), "bf16")
    Np = 4 + PU.SPARE + 4
    table = np.array([[0, Np - 2, 2, 3]], dtype=np.int64)
    pl = PU.Layer(kn, vn, P, 0, table=table, n_pages=Np)
    fill_k = prng.gen_keys(46001, (1, H, P, D_ABI), "bf16")
    fill_v = prng.gen_values(46001, (1, H, P, D_ABI), "bf16")
    clamp = Np - 4 - 1
    pl.k[clamp] = to_dev(fill_k, DEV)[0]
    pl.v[clamp] = to_dev(fill_v, DEV)[0]
    snap = pl.snapshot()
    outs = [tuple(torch.zeros((B, H, 40, D_ABI), dtype=torch.bfloat16, device=DEV)
                  for _ in range(2))]
    tab, pages = _abi_tables([s], [pl], inplace, outs, num_pages=Np - 4)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = _params(B, H, status)
    rc, info = N.plan_paged(p, tab, pages, None)
    assert rc == 0
    ws = _workspace(info)
    assert N.launch_paged(p, tab, pages, None, ws.data_ptr(), int(info.workspace_bytes),
                          torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert int(status.item()) == N.DEV_INDEX_RANGE
    # the dense tensor a clamping reader sees: logical rows [16, 32) come from page `clamp`
    seen_k, seen_v = kn.copy(), vn.copy()
    seen_k[:, :, 16:32], seen_v[:, :, 16:32] = fill_k, fill_v
    if mode == "select":
        wk, wv, _ = PT.expected_layer(seen_k, seen_v, s, PT.ASC, PT.SORT)
        assert not np.array_equal(wk, PT.expected_layer(kn, vn, s, PT.ASC, PT.SORT)[0])
    else:
        wk, wv = seen_k[:, :, 8:48], seen_v[:, :, 8:48]
    if not inplace:
        assert np.array_equal(_bytes(to_np(outs[0][0])), _bytes(wk))
        assert np.array_equal(_bytes(to_np(outs[0][1])), _bytes(wv))
    else:  # output rows [16, 32) would go through the bad id: dropped
        pl.expect(snap, wk[:, :, :16], wv[:, :, :16])
        pl.expect(snap, wk[:, :, 32:], wv[:, :, 32:], first=32)
        # (expect() wrote nothing into pages N-4 .. N-1: row 16..31's page is not in its table)
    bad_rows = slice(Np - 4, Np)
    assert torch.equal(PU.ints(pl.kb[bad_rows]), PU.ints(snap[0][bad_rows]))
    pl.assert_pools(snap, ("bad page id", mode))


def test_offsets_past_4_gib():
    """8: a pool view whose page stride puts page 2 more than 4 GiB above the base."""
    from kvcompress import PagedKV, compress_paged
    from oracle import oracle
    B, H, S, P, D = 1, 2, 300, 128, 64
    page_elems = H * P * D
    gap = (1 << 31) // 2 + page_elems           # elements: 2 GiB + one page of bf16 per step
    kn, vn = prng.gen_keys(47000, (B, H, S, D), "bf16"), prng.gen_values(47000, (B, H, S, D), "bf16")
    flat = torch.empty(2 * gap + page_elems, dtype=torch.bfloat16, device=DEV)
    vflat = torch.empty(3 * page_elems, dtype=torch.bfloat16, device=DEV)
    k_pool = flat.as_strided((3, H, P, D), (gap, P * D, D, 1))
    v_pool = vflat.as_strided((3, H, P, D), (page_elems, D, H * D, 1))
    assert 2 * gap * 2 > 1 << 32
    for pool in (k_pool, v_pool):
        pool.fill_(1.5)
    table = torch.tensor([[2, 0, 1]], dtype=torch.int32, device=DEV)
    PU.write_rows(k_pool, table, to_dev(kn, DEV))
    PU.write_rows(v_pool, table, to_dev(vn, DEV))
    snap = (k_pool.clone(), v_pool.clone())
    kw = dict(fix_kv_size=100, keep_ratio=0.25, skip_layers=[])
    (rk, rv, _), = oracle.METHODS["fix_size_l2"]([(kn, vn)], **kw)
    lens = compress_paged("fix_size_l2", [PagedKV(k_pool, v_pool, table, S)], **kw)
    torch.cuda.synchronize()
    assert lens == [100]
    PU.write_rows(snap[0], table, to_dev(rk, DEV))
    PU.write_rows(snap[1], table, to_dev(rv, DEV))
    assert torch.equal(PU.ints(k_pool), PU.ints(snap[0]))
    assert torch.equal(PU.ints(v_pool), PU.ints(snap[1]))
