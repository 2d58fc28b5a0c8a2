"""GPU parity on non-contiguous K / V and attention views (include/kvc.h: "last dim contiguous,
arbitrary element strides for the other three dims", K and V separately).

Kernel results depend on values only, so the reference for a view is the CPU oracle on the
contiguous arrays the view was filled from; the bar is the project's own -- identical output
kinds and byte-identical K / V, no tolerance.  K and V always come in different layouts (or as the
K / V thirds of one fused projection buffer), so their stride triples differ, and everything
around a view is poison (tests/strided_layouts.py).  tests/test_strided_layouts.py proves on the
CPU that a kernel ignoring the strides could not produce the expected bytes for these inputs.

Which kernel path each block reaches (thresholds in csrc/kvc_device_util.h: kSmallZone 8192, kZoneMax 16384,
kZoneMaxGlobal 65536, kSplitCopyRows 255):
  (a) score_tile at its three staging widths and gather_row / gather_block at every row width;
  (b) every layout, the copy-only launches, views and untouched layers;
  (c) the 1 024-thread select_gather rows (split and unsplit copy), select_kernel +
      gather_kernel over the global scratch, select_long_kernel;
  (d) the stable tie policy's kernels;  (e) external and shared indices (gather_kernel
  PART_FIXED / PART_SELECTED);  (f) offsets past 2^31 / 2^32 bytes;  (g) the call memo and plan
  cache;  (h) kvc_attn_accumulate's attention strides.
"""
import numpy as np
import pytest
import torch

import prng
import strided_layouts as SL
from gpu_util import kind_of, to_dev, to_np
from oracle import oracle

pytestmark = pytest.mark.gpu

TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(params=["kernels", "separate"])
def launch_path(request, monkeypatch):
    """Both launch paths of kvc_launch: the default SCORE + SELECT_GATHER kernels ("kernels") and
    SCORE / SELECT / GATHER as three kernels (KVC_FLAG_SPLIT_SELECT_GATHER, "separate")."""
    from kvcompress import _engine
    monkeypatch.setattr(_engine, "split_select_gather", request.param == "separate")
    return request.param


def _method(name):
    from kvcompress.methods import get_compress_fn
    if name == "evict_for_space":  # exported by streaming_llm, not in the registry
        from kvcompress.methods.streaming_llm import evict_for_space
        return evict_for_space
    return get_compress_fn(name)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


_REF = {}


def _inputs_and_reference(case):
    """(numpy layers, oracle result) of a case, computed once (per tie policy) and shared by the
    launch paths; neither is modified afterwards."""
    key = (case["id"], oracle.TIE)
    if key not in _REF:
        layers = SL.case_inputs(case)
        _REF[key] = (layers, oracle.METHODS[case["method"]](layers, **case["kw"]))
    return _REF[key]


def _check_case(case, expect_kinds=None):
    layers, ref = _inputs_and_reference(case)
    tin = [SL.make_pair(case["k_layout"], case["v_layout"], k, v) for k, v in layers]
    for k, v in tin:
        assert not k.is_contiguous() and not v.is_contiguous()
    out = _method(case["method"])(list(tin), **case["kw"])
    torch.cuda.synchronize()
    assert len(out) == len(ref)
    for li, ((ki, vi), (ko, vo), (rk, rv, kind)) in enumerate(zip(tin, out, ref)):
        ctx = (case["id"], li)
        assert kind_of(ki, ko) == kind == kind_of(vi, vo), ctx
        assert tuple(ko.shape) == rk.shape and tuple(vo.shape) == rv.shape, ctx
        assert np.array_equal(_bytes(to_np(ko)), _bytes(rk)), ctx + ("K",)
        assert np.array_equal(_bytes(to_np(vo)), _bytes(rv)), ctx + ("V",)
    if expect_kinds is not None:
        assert {kind for _, _, kind in ref} == expect_kinds, case["id"]


def _params(cases):
    return [pytest.param(c, id=c["id"]) for c in cases]


# ---- (a) every row width through the small fused path -----------------------------------------
@pytest.mark.parametrize("case", _params(SL.CASES_A))
def test_every_row_width_on_strided_views(case, launch_path):
    _check_case(case, {"new"})


# ---- (b) all layouts, one geometry ------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(SL.CASES_B)), ids=[c["id"] for c in SL.CASES_B])
def test_every_layout_through_every_kind_of_call(ci, monkeypatch):
    """Two layers of different lengths per call; the launch paths take turns.  recent_only returns
    views of the strided inputs, a call below its threshold the inputs themselves."""
    from kvcompress import _engine
    case = SL.CASES_B[ci]
    monkeypatch.setattr(_engine, "split_select_gather", ci % 2 == 1)
    kinds = {"recent_only": {"view"}}.get(case["method"], {"new"})
    if case["kw"].get("fix_kv_size") == 1000:
        kinds = {"same"}
    _check_case(case, kinds)


# ---- (c) longer zones -------------------------------------------------------------------------
@pytest.mark.parametrize("case", _params([c for c in SL.CASES_C if c["shapes"][0][2] == 9000]))
def test_mid_zone_rows_on_strided_views(case, launch_path):
    """S = 9 000: the 1 024-thread select_gather instance; h2o_l2's two rows with sink and tail
    take the split-copy workgroups, fix_size_l2 without a recent part copies unsplit."""
    _check_case(case, {"new"})


@pytest.mark.parametrize("case", _params([c for c in SL.CASES_C if c["shapes"][0][2] > 9000]))
def test_long_zone_kernels_on_strided_views(case):
    """S = 20 000: select_kernel over the global scratch + gather_kernel; S = 65 600:
    select_long_kernel + gather_kernel."""
    _check_case(case, {"new"})


# ---- (d) stable tie policy --------------------------------------------------------------------
_STABLE = SL.CASES_D + [c for c in SL.CASES_C if c["shapes"][0][2] == 20000]


@pytest.mark.parametrize("ci", range(len(_STABLE)), ids=[c["id"] for c in _STABLE])
def test_stable_policy_on_strided_views(ci, monkeypatch):
    from kvcompress import _engine
    monkeypatch.setattr(_engine, "split_select_gather", ci % 2 == 0)
    monkeypatch.setattr(_engine, "tie_policy", "stable")
    monkeypatch.setattr(oracle, "TIE", "stable")
    _engine.call_memo.clear()
    _check_case(_STABLE[ci], {"new"})


# ---- (e) external indices ---------------------------------------------------------------------
def test_random_strategy_on_strided_views():
    """strategy='random' (caller-provided indices through gather_kernel) on static / bshd views,
    against the torch restatement of test_random_strategy_matches_torch_restatement."""
    from kvcompress.methods import fix_size_l2_compress
    B, H, S, D = 2, 4, 700, 64
    K, V = SL.make_pair("static", "bshd", prng.gen_keys(5, (B, H, S, D), "bf16"),
                        prng.gen_values(5, (B, H, S, D), "bf16"))
    torch.manual_seed(123)
    out = fix_size_l2_compress([(K, V)], fix_kv_size=200, keep_ratio=0.25, strategy="random",
                               skip_layers=[])
    torch.manual_seed(123)
    P = 50
    Z, keep = S - P, 200 - P
    ind = torch.stack([torch.stack([torch.randperm(Z, device=K.device)[:keep] for _ in range(H)])
                       for _ in range(B)])
    ind, _ = torch.sort(ind, dim=-1)
    e = ind.unsqueeze(-1).expand(B, H, keep, D)
    rk = torch.cat([torch.gather(K[:, :, :Z], 2, e), K[:, :, -P:]], dim=2)
    rv = torch.cat([torch.gather(V[:, :, :Z], 2, e), V[:, :, -P:]], dim=2)
    assert torch.equal(out[0][0].view(torch.int16), rk.contiguous().view(torch.int16))
    assert torch.equal(out[0][1].view(torch.int16), rv.contiguous().view(torch.int16))


def _tie_attention(rng, shape, levels=4):
    """Softmax rows over a few distinct logits (ties within and across heads), fp32."""
    logits = rng.integers(0, levels, size=shape).astype(np.float32) * np.float32(0.7)
    return torch.from_numpy(logits).softmax(dim=-1)


def _h2o_expected(mgr, li, x, start, recent):
    """sinks ++ heavy hitters ++ recent of x, built with torch on the device from the manager's
    own index list (h2o_attention.py:305-361)."""
    S = x.shape[2]
    idx = mgr.get_heavy_hitter_indices(li, S)
    mid = x[:, :, start:S - recent]
    return torch.cat([x[:, :, :start], mid[:, :, idx], x[:, :, -recent:]], dim=2)


@pytest.mark.parametrize("S", [900, 6000])
def test_h2o_attention_shared_index_gather_on_strided_views(S):
    """h2o_attention_compress with a manager: one index list per layer serves every head
    (KVC_FLAG_SHARED_INDEX); at S = 6 000 the middle is >= OVERLAP_MIN_ZONE, so the sink / recent
    rows are copied on the side stream (gather_kernel PART_FIXED beside PART_SELECTED)."""
    from kvcompress.methods import h2o_attention as HA
    rng = np.random.default_rng(S)
    H, D, start, hh, recent = 8, 64, 4, 64, 444
    assert (S - start - recent >= HA.OVERLAP_MIN_ZONE) == (S == 6000)
    kv = [SL.make_pair("static", "head_slice", prng.gen_keys(60 + i, (1, H, S, D), "bf16"),
                       prng.gen_values(60 + i, (1, H, S, D), "bf16")) for i in range(2)]
    att = tuple(_tie_attention(rng, (1, H, 2, S)).to(torch.bfloat16).to("cuda:0") for _ in kv)
    mgr = HA.H2OAttentionManager(start_size=start, heavy_hitter_size=hh, recent_size=recent)
    out = HA.h2o_attention_compress(list(kv), attention_scores=att, h2o_manager=mgr,
                                    start_size=start, heavy_hitter_size=hh, recent_size=recent)
    for li, ((k, v), (ko, vo)) in enumerate(zip(kv, out)):
        assert ko.shape == vo.shape == (1, H, start + hh + recent, D)
        for x, got in ((k, ko), (v, vo)):
            want = _h2o_expected(mgr, li, x, start, recent)
            assert np.array_equal(_bytes(to_np(got)), _bytes(to_np(want))), (S, li)


# ---- (f) offsets beyond 32 bits ---------------------------------------------------------------
@pytest.mark.parametrize("huge", ["k", "v"])
def test_row_offsets_beyond_32_bits(huge, launch_path):
    """A [:, :, 1000:1300] window of a [3, 2, 2^22, 128] bf16 cache (6 GiB, only the window is
    written): the byte offset of row (b = 1, h = 0) is past 2^31, that of (b = 2, h = 1) past 2^32.
    The other tensor is a small static view, so K and V strides differ by orders of magnitude."""
    from kvcompress.methods import fix_size_l2_compress, h2o_l2_compress
    free, _ = torch.cuda.mem_get_info()
    if free < 16 << 30:
        pytest.skip(f"needs 16 GiB of free device memory, {free >> 30} GiB free")
    B, H, S, D, T = 3, 2, 300, 128, 1 << 22
    kn = prng.gen_keys(71, (B, H, S, D), "bf16", "few")
    vn = prng.gen_values(71, (B, H, S, D), "bf16")
    big = torch.empty((B, H, T, D), dtype=torch.bfloat16, device="cuda:0")
    try:
        win = big[:, :, 1000:1000 + S]
        win.copy_(to_dev(kn if huge == "k" else vn))
        es = win.element_size()
        assert (2 * win.stride(0) + win.stride(1)) * es > 1 << 32
        assert win.stride(0) * es >= 1 << 31
        small = SL.make_view("static", vn if huge == "k" else kn)
        k, v = (win, small) if huge == "k" else (small, win)
        for fn, ofn, kw in (
                (fix_size_l2_compress, oracle.fix_size_l2_compress,
                 dict(fix_kv_size=100, keep_ratio=0.25, skip_layers=[])),
                (h2o_l2_compress, oracle.h2o_l2_compress,
                 dict(start_size=4, heavy_hitter_size=40, recent_size=60, skip_layers=[]))):
            out = fn([(k, v)], **kw)
            torch.cuda.synchronize()
            rk, rv, kind = ofn([(kn, vn)], **kw)[0]
            assert kind == "new" == kind_of(k, out[0][0])
            assert np.array_equal(_bytes(to_np(out[0][0])), _bytes(rk)), (fn.__name__, "K")
            assert np.array_equal(_bytes(to_np(out[0][1])), _bytes(rv)), (fn.__name__, "V")
    finally:
        del big
        win = k = v = out = None
        torch.cuda.empty_cache()


# ---- (g) memo and plan cache must not cross layouts -------------------------------------------
def test_call_memo_and_plan_cache_do_not_serve_strided_views():
    """A recorded plain-contiguous call shape is replayed with contiguous strides in its table: a
    call of the same shape on static views must neither be replayed nor cached, and must not
    disturb the recording."""
    from kvcompress import _engine
    from kvcompress.methods import fix_size_l2_compress
    _engine.call_memo.clear()
    _engine.plan_cache.clear()
    kw = dict(fix_kv_size=100, keep_ratio=0.25, skip_layers=[])
    shape = (2, 3, 300, 64)

    def call(step, strided):
        layers = [(prng.gen_keys(7100 + 10 * step + i, shape, "bf16", "few"),
                   prng.gen_values(7100 + 10 * step + i, shape, "bf16")) for i in range(2)]
        if strided:
            tin = [SL.make_pair("static", "bshd", k, v) for k, v in layers]
        else:
            tin = [(to_dev(k), to_dev(v)) for k, v in layers]
        out = fix_size_l2_compress(list(tin), **kw)
        ref = oracle.fix_size_l2_compress(layers, **kw)
        for (ko, vo), (rk, rv, _) in zip(out, ref):
            assert np.array_equal(_bytes(to_np(ko)), _bytes(rk)), (step, strided)
            assert np.array_equal(_bytes(to_np(vo)), _bytes(rv)), (step, strided)

    r0 = _engine.memo_stats["replayed"]
    for step in range(3):
        call(step, False)
    assert _engine.memo_stats["replayed"] - r0 == 1  # first sighting, recorded, replayed
    cached = set(_engine.plan_cache.entries)
    assert cached
    call(3, True)
    assert _engine.memo_stats["replayed"] - r0 == 1
    assert set(_engine.plan_cache.entries) == cached
    call(4, False)
    assert _engine.memo_stats["replayed"] - r0 == 2
    assert set(_engine.plan_cache.entries) == cached


def test_step_replay_does_not_serve_strided_views():
    """h2o_attention_compress's native step replay (a plan with contiguous K / V strides) is not
    taken for strided K / V of the same shape, and serves plain K / V again afterwards."""
    from kvcompress.methods import h2o_attention as HA
    rng = np.random.default_rng(21)
    H, S, D, start, hh, recent = 8, 900, 64, 4, 32, 100
    kw = dict(start_size=start, heavy_hitter_size=hh, recent_size=recent)
    mgr = HA.H2OAttentionManager(**kw)
    HA.step_memo.clear()
    assert HA.replay_steps

    def step(i, strided):
        layers = [(prng.gen_keys(7300 + 10 * i + j, (1, H, S, D), "bf16"),
                   prng.gen_values(7300 + 10 * i + j, (1, H, S, D), "bf16")) for j in range(2)]
        if strided:
            kv = [SL.make_pair("static", "head_slice", k, v) for k, v in layers]
        else:
            kv = [(to_dev(k), to_dev(v)) for k, v in layers]
        att = tuple(_tie_attention(rng, (1, H, 1, S)).to(torch.bfloat16).to("cuda:0") for _ in kv)
        mgr.reset()
        out = HA.h2o_attention_compress(list(kv), attention_scores=att, h2o_manager=mgr, **kw)
        for li, ((k, v), (ko, vo)) in enumerate(zip(kv, out)):
            for x, got in ((k, ko), (v, vo)):
                want = _h2o_expected(mgr, li, x, start, recent)
                assert np.array_equal(_bytes(to_np(got)), _bytes(to_np(want))), (i, strided, li)

    r0 = HA.step_stats["replayed"]
    for i in range(3):
        step(i, False)
    r1 = HA.step_stats["replayed"]
    assert r1 - r0 >= 1  # the plain shape is planned and replayed
    step(3, True)
    assert HA.step_stats["replayed"] == r1
    step(4, False)
    assert HA.step_stats["replayed"] == r1 + 1


# ---- (h) strided attention --------------------------------------------------------------------
ATTN_LAYOUTS = ("kpad", "qpad", "head_slice", "batch_slice", "last_dim_strided")


def _attn_views(layout, a, dt):
    """(device view, CPU view) of attention values `a` [B,H,q,k] (fp32 tensor) with the same
    element strides, both sliced from one backing array (a .to('cuda') of a non-dense view would
    not keep its strides)."""
    B, H, q, k = a.shape
    bshape = {"kpad": (B, H, q, k + 11), "qpad": (B, H, q + 5, k), "head_slice": (B, 2 * H, q, k),
              "batch_slice": (2 * B + 1, H, q, k), "last_dim_strided": (B, H, q, 2 * k)}[layout]
    cut = {"kpad": lambda x: x[..., :k], "qpad": lambda x: x[:, :, :q],
           "head_slice": lambda x: x[:, 1::2], "batch_slice": lambda x: x[1::2],
           "last_dim_strided": lambda x: x[..., ::2]}[layout]
    backing = torch.full(bshape, 0.5, dtype=TORCH_DT[dt])  # softmax values never reach 0.5 + ties
    cut(backing).copy_(a)
    dev = backing.to("cuda:0")
    assert dev.is_contiguous() and dev.stride() == backing.stride()
    dv, cv = cut(dev), cut(backing)
    assert dv.stride() == cv.stride() and dv.stride() != a.stride()
    # (a batch slice of one batch is dense: only its batch stride and start differ)
    assert not dv.is_contiguous() or (layout == "batch_slice" and B == 1)
    return dv, cv


def _reference_step(acc_ref, attn_cpu, decay=0.9):
    """The reference's update (h2o_attention.py:116-151) with torch's CPU ops."""
    B, H, _, k = attn_cpu.shape
    imp = attn_cpu.sum(dim=2)
    if acc_ref is None or acc_ref.size(-1) > k:
        acc_ref = torch.zeros(B, H, k, dtype=attn_cpu.dtype)
    elif acc_ref.size(-1) < k:
        acc_ref = torch.cat([acc_ref * decay, torch.zeros(B, H, k - acc_ref.size(-1),
                                                          dtype=attn_cpu.dtype)], dim=-1)
    else:
        acc_ref = acc_ref * decay
    return acc_ref + imp


def _reference_heavy(acc_ref, k, start, recent, hh):
    m1 = k - recent
    agg = acc_ref[:, :, start:m1].sum(dim=1)
    if acc_ref.shape[0] == 1:
        agg = agg.squeeze(0)
    _, top = torch.topk(agg, min(hh, m1 - start), dim=-1)
    return torch.sort(top, dim=-1)[0]


ATTN_SHAPES = ((2, 4, 37, 301), (3, 2, 33, 517), (1, 8, 16, 1501))


@pytest.mark.parametrize("threads", [1, 8, 16])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("layout", ATTN_LAYOUTS)
def test_strided_attention_matches_torch_cpu_ops(layout, dt, threads):
    """update_attention_scores on strided attention (kvc_attn_accumulate's q-stride, the thread
    chunks of _cpu_order.attn_sum_chunk where B and H do not coalesce) and the heavy hitters,
    against torch's CPU ops on a CPU tensor with the same element strides; two steps per shape
    (first, zero-extended).  The last-dim-strided view takes the engine's .contiguous() branch."""
    from kvcompress import _cpu_order as CO
    from kvcompress.methods.h2o_attention import H2OAttentionManager
    rng = np.random.default_rng(100 + threads)
    prev = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        for B, H, q, k in ATTN_SHAPES:
            mgr = H2OAttentionManager(start_size=4, heavy_hitter_size=16, recent_size=50,
                                      decay_factor=0.9)
            mgr.reduction_threads = threads
            acc_ref = None
            for qq, kk in ((q, k), (3, k + 1)):
                dv, cv = _attn_views(layout, _tie_attention(rng, (B, H, qq, kk)), dt)
                if layout == "last_dim_strided":
                    assert dv.stride(3) == 2
                elif layout == "batch_slice" and threads == 8 and (B, H, qq, kk) == ATTN_SHAPES[0]:
                    # B and H do not coalesce: the columns are split over the threads, which the
                    # contiguous tensor's sum does not do -- the case must not degenerate
                    assert CO.attn_sum_chunk(dv, threads) != 0
                    assert CO.attn_sum_chunk(dv.contiguous(), threads) == 0
                mgr.update_attention_scores((dv,))
                acc_ref = _reference_step(acc_ref, cv)
                got = mgr.accumulated_attention[0]
                assert got.shape == acc_ref.shape
                assert np.array_equal(_bytes(to_np(got)), _bytes(to_np(acc_ref))), (B, H, qq, kk)
                top = _reference_heavy(acc_ref, kk, 4, 50, 16)
                assert mgr.get_heavy_hitter_indices(0, kk).cpu().tolist() == top.tolist(), \
                    (B, H, qq, kk)
    finally:
        torch.set_num_threads(prev)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_strided_attention_whose_chunk_rule_shows_in_the_bytes(dt):
    """[2, 4, 120, 37] attention as a batch slice, 8 threads: torch's CPU sum of the strided view
    differs in its bytes (fp32) from the sum of the contiguous copy, because only the strided sum
    splits its columns over the threads (tests/test_strided_layouts.py pins the rule on the CPU).
    The engine, given the device view with the same strides, must give the strided sum's bytes;
    given the contiguous copy, the other's."""
    from kvcompress import _cpu_order as CO
    from kvcompress.methods.h2o_attention import H2OAttentionManager
    cv, cc = SL.chunk_rule_attention(dt)
    dev_backing = cv._base.to("cuda:0")
    dv = dev_backing[1::2]
    assert dv.stride() == cv.stride() and not dv.is_contiguous()
    threads = SL.CHUNK_THREADS
    assert CO.attn_sum_chunk(dv, threads) != 0 and CO.attn_sum_chunk(cc, threads) == 0
    prev = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        want = {"strided": _reference_step(None, cv), "contiguous": _reference_step(None, cc)}
    finally:
        torch.set_num_threads(prev)
    if dt == "fp32":
        assert not np.array_equal(_bytes(to_np(want["strided"])), _bytes(to_np(want["contiguous"])))
    for name, attn in (("strided", dv), ("contiguous", cc.to("cuda:0"))):
        mgr = H2OAttentionManager(start_size=4, heavy_hitter_size=8, recent_size=8)
        mgr.reduction_threads = threads
        mgr.update_attention_scores((attn,))
        got = mgr.accumulated_attention[0]
        assert np.array_equal(_bytes(to_np(got)), _bytes(to_np(want[name]))), name


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_decode_steps_with_strided_attention_are_replayed_natively(dt):
    """A decode sequence (k = 1500, 1501, 1502; q = 1) whose attention rows are [..., :k] windows
    of rows padded to the static cache length, run four times with reset() in between: the
    native step replay (kvc_host.scan_h2o keys the attention strides, run_h2o passes them to
    kvc_attn_accumulate) is taken and every step's accumulation and heavy hitters equal torch's
    CPU ops."""
    from kvcompress.methods import h2o_attention as HA
    rng = np.random.default_rng(31)
    H, D, start, hh, recent = 8, 64, 4, 16, 50
    kw = dict(start_size=start, heavy_hitter_size=hh, recent_size=recent)
    mgr = HA.H2OAttentionManager(decay_factor=0.9, **kw)
    mgr.reduction_threads = torch.get_num_threads()
    HA.step_memo.clear()
    r0 = HA.step_stats["replayed"]
    kvs = {S: (to_dev(prng.gen_keys(80 + S, (1, H, S, D), "bf16")),
               to_dev(prng.gen_values(80 + S, (1, H, S, D), "bf16"))) for S in (1500, 1501, 1502)}
    for run in range(4):
        mgr.reset()
        acc_ref = None
        for S in (1500, 1501, 1502):
            dv, cv = _attn_views("kpad", _tie_attention(rng, (1, H, 1, S)), dt)
            out = HA.h2o_attention_compress([kvs[S]], attention_scores=(dv,), h2o_manager=mgr, **kw)
            acc_ref = _reference_step(acc_ref, cv)
            got = mgr.accumulated_attention[0]
            assert np.array_equal(_bytes(to_np(got)), _bytes(to_np(acc_ref))), (run, S)
            top = _reference_heavy(acc_ref, S, start, recent, hh)
            assert mgr.get_heavy_hitter_indices(0, S).cpu().tolist() == top.tolist(), (run, S)
            for x, y in zip(kvs[S], out[0]):
                mid = x[:, :, start:S - recent]
                want = torch.cat([x[:, :, :start], mid[:, :, top.to(x.device)],
                                  x[:, :, -recent:]], dim=2)
                assert np.array_equal(_bytes(to_np(y)), _bytes(to_np(want))), (run, S)
    assert HA.step_stats["replayed"] - r0 >= 3
