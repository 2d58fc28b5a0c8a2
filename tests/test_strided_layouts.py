"""CPU checks of the strided-layout helper (tests/strided_layouts.py) and of the inputs the GPU
tests in tests/test_strided_inputs.py feed the kernels: every layout has the strides its shape
arithmetic states, the engine's accept / copy decision for it is the intended one, and the CPU
oracle -- run on what a stride-ignoring kernel would read -- gives another result than on the
view, so such a kernel could not pass."""
import numpy as np
import pytest
import torch

import prng
import strided_layouts as SL
from oracle import oracle

SHAPE = (2, 3, 50, 64)
TORCH_DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def _dtypes(layout):
    return ("bf16", "fp16") if layout in ("row_pad", "row_off") else ("bf16", "fp16", "fp32")


def _input(layout, dt, shape=SHAPE, seed=7):
    a = prng.gen_values(seed, shape, dt)
    return SL.expand_input(a) if layout == "expand" else a


@pytest.mark.parametrize("role", ["k", "v"])
@pytest.mark.parametrize("layout", list(SL.LAYOUTS))
def test_geometry_is_the_layouts_shape_arithmetic(layout, role):
    """geometry() against an independent construction: element (b, h, s, d) of the view is
    element `offset + b*st0 + h*st1 + s*st2 + d` of the flat backing, for an index-valued
    backing, and the view never leaves the backing."""
    bshape, off, st = SL.geometry(layout, SHAPE, role)
    n = int(np.prod(bshape))
    flat = np.arange(n, dtype=np.int64)
    B, H, S, D = SHAPE
    b, h, s, d = np.meshgrid(np.arange(B), np.arange(H), np.arange(S), np.arange(D), indexing="ij")
    want = off + b * st[0] + h * st[1] + s * st[2] + d * st[3]
    assert want.min() >= 0 and want.max() < n
    view = SL._carve(flat.reshape(bshape), layout, role, SHAPE, lambda x: x.transpose(0, 2, 1, 3),
                     lambda x: np.broadcast_to(x, SHAPE))
    assert view.shape == SHAPE
    np.testing.assert_array_equal(view, want)
    assert st != SL.contiguous_strides(SHAPE)
    if layout != "expand":  # no two elements share storage
        assert len(np.unique(want)) == want.size


@pytest.mark.parametrize("layout", list(SL.LAYOUTS))
def test_numpy_view_has_the_stated_strides_and_values(layout):
    for dt in _dtypes(layout):
        for role in ("k", "v"):
            a = _input(layout, dt)
            backing, view = SL.make_backing_np(layout, a, role)
            bshape, off, st = SL.geometry(layout, SHAPE, role)
            es = a.dtype.itemsize
            assert backing.shape == bshape and backing.flags["C_CONTIGUOUS"]
            assert tuple(x // es for x in view.strides) == st
            assert np.array_equal(view.view(np.uint8) if view.flags["C_CONTIGUOUS"]
                                  else np.ascontiguousarray(view).view(np.uint8),
                                  a.view(np.uint8))
            # everything outside the view is poison
            mask = np.ones(backing.size, dtype=bool)
            B, H, S, D = SHAPE
            b, h, s, d = np.meshgrid(np.arange(B), np.arange(H), np.arange(S), np.arange(D),
                                     indexing="ij")
            mask[(off + b * st[0] + h * st[1] + s * st[2] + d).reshape(-1)] = False
            outside = backing.reshape(-1)[mask]
            assert (outside.view(np.uint8) == SL.POISON).all()
            if layout not in ("bshd", "expand"):
                assert outside.size > 0


def test_fused_pair_shares_one_backing():
    k, v = _input("fused_qkv", "bf16", seed=1), _input("fused_qkv", "bf16", seed=2)
    (kb, kv), (vb, vv) = SL.make_pair_np("fused_qkv", "fused_qkv", k, v)
    assert kb is vb
    assert np.array_equal(kv, k) and np.array_equal(vv, v)
    B, H, S, D = SHAPE
    assert (kb[..., :D].view(np.uint8) == SL.POISON).all()  # the Q third


@pytest.mark.parametrize("layout", list(SL.LAYOUTS))
def test_engine_prep_decision(layout):
    """_engine._prep on a CPU tensor with the layout's strides: row_pad (seq stride not a
    multiple of 16 bytes) and row_off (pointer 8 bytes off) are copied, every other layout is
    handed to the kernels as it is.  kvc_plan's own stride rules agree (test_abi.py)."""
    from kvcompress import _engine
    for dt in _dtypes(layout):
        for role in ("k", "v"):
            bshape, off, st = SL.geometry(layout, SHAPE, role)
            backing = torch.zeros(bshape, dtype=TORCH_DT[dt])
            assert backing.data_ptr() % 16 == 0
            t = backing.as_strided(SHAPE, st, off)
            es = t.element_size()
            as_is = _engine._prep(t) is t
            assert as_is == (layout not in ("row_pad", "row_off")), (layout, dt, role)
            assert as_is == SL.prep_takes_as_is(st, SHAPE, off, es)
            if not as_is:
                c = _engine._prep(t)
                assert c.is_contiguous() and c.data_ptr() % 16 == 0 and torch.equal(c, t)
    # D = 64 is what makes row_pad's 16-bit rows misaligned: (64 + 4) * 2 = 136 bytes
    assert (SL.geometry("row_pad", SHAPE)[2][2] * 2) % 16 != 0
    assert (SL.geometry("row_off", SHAPE)[2][2] * 2) % 16 == 0 and (SL.geometry("row_off", SHAPE)[1] * 2) % 16


# ---------------------------------------------------------------------------------------------
# The GPU cases' inputs discriminate: the oracle on what a stride-ignoring kernel would read
# ---------------------------------------------------------------------------------------------
def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(ref, got):
    return all(rk.shape == gk.shape and rv.shape == gv.shape and
               np.array_equal(_bytes(rk), _bytes(gk)) and np.array_equal(_bytes(rv), _bytes(gv))
               for (rk, rv, _), (gk, gv, _) in zip(ref, got))


def _unique(cases):
    """One case per (layouts, dtype, shapes, method, kwargs) -- ids are unique already."""
    return [pytest.param(c, id=c["id"]) for c in cases]


def _discriminates(case):
    layers = SL.case_inputs(case)
    fn = oracle.METHODS[case["method"]]
    ref = fn(layers, **case["kw"])
    if all(kind == "same" for _, _, kind in ref):
        return  # a call that touches no layer reads no K/V
    pairs = [SL.make_pair_np(case["k_layout"], case["v_layout"], k, v) for k, v in layers]
    # the views themselves give the contiguous result (the GPU tests' reference)
    assert _same(ref, fn([(kv, vv) for (_, kv), (_, vv) in pairs], **case["kw"]))
    wrong = {"k": [], "v": []}
    for (kb, kv), (vb, vv) in pairs:
        wrong["k"].append((kv if case["k_layout"] == "expand" else SL.misread_np(kb, kv), vv))
        wrong["v"].append((kv, vv if case["v_layout"] == "expand" else SL.misread_np(vb, vv)))
    for side in ("k", "v"):
        if case[side + "_layout"] == "expand":
            continue  # contiguous strides would leave an expand backing
        assert not _same(ref, fn(wrong[side], **case["kw"])), (case["id"], side)


@pytest.mark.parametrize("case", _unique(SL.CASES_A))
def test_row_width_cases_tell_ignored_strides(case):
    _discriminates(case)


@pytest.mark.parametrize("case", _unique(SL.CASES_B))
def test_layout_cases_tell_ignored_strides(case):
    _discriminates(case)


@pytest.mark.parametrize("case", _unique(SL.CASES_C))
def test_long_zone_cases_tell_ignored_strides(case):
    _discriminates(case)


def test_case_tables_cover_what_they_claim():
    """Every row width and every layout pair of block (a) meets all four methods; block (b) names
    every layout as K and as V, with different K / V layouts except for the fused pair; every
    case's K and V stride triples differ."""
    for i, (D, dt) in enumerate(SL.WIDTHS_A):
        got = {c["id"].rsplit("-", 1)[1] for c in SL.CASES_A if c["dtype"] == dt and
               c["shapes"][0][3] == D}
        assert len(got) == 4, (D, dt, got)
    for kl, vl in SL.PAIRS_A:
        got = {c["id"].rsplit("-", 1)[1] for c in SL.CASES_A if c["k_layout"] == kl}
        assert len(got) == 4, (kl, got)
    assert {p[0] for p in SL.PAIRS_B} == set(SL.LAYOUTS) == {p[1] for p in SL.PAIRS_B}
    for c in SL.CASES_A + SL.CASES_B + SL.CASES_C + SL.CASES_D:
        if c["k_layout"] != "fused_qkv":
            assert c["k_layout"] != c["v_layout"]
        for shape in c["shapes"]:
            ks = SL.geometry(c["k_layout"], shape, "k")
            vs = SL.geometry(c["v_layout"], shape, "v")
            assert (ks[1], ks[2]) != (vs[1], vs[2]), c["id"]
            if c["k_layout"] != "fused_qkv":
                assert ks[2][:3] != vs[2][:3], c["id"]
    assert 80 <= 2 * len(SL.CASES_A) <= 120


# ---------------------------------------------------------------------------------------------
# The strided branch of _cpu_order.attn_sum_chunk (B and H do not coalesce)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_attn_sum_chunk_follows_the_strides_like_torch(dt):
    from kvcompress import _cpu_order as CO
    from oracle import h2o_oracle as HO
    view, cont = SL.chunk_rule_attention(dt)
    B, H, q, k = SL.CHUNK_SHAPE
    assert CO.attn_sum_chunk(cont, SL.CHUNK_THREADS) == 0
    assert CO.attn_sum_chunk(view, SL.CHUNK_THREADS) == -(-k // SL.CHUNK_THREADS) == 5
    prev = torch.get_num_threads()
    torch.set_num_threads(SL.CHUNK_THREADS)
    try:
        t_view, t_cont = view.sum(dim=2), cont.sum(dim=2)
    finally:
        torch.set_num_threads(prev)
    raw = (lambda t: t.view(torch.int16).numpy()) if dt == "bf16" else (lambda t: t.numpy())
    x = cont.float().numpy()
    es = cont.element_size()

    def restated(outer):
        ilp = HO.ilp_mask(k, outer, q, es, SL.CHUNK_THREADS, None)
        out = np.stack([np.stack([HO.sum_reduce_first(x[b, h], ilp) for h in range(H)])
                        for b in range(B)])
        return HO.from_f32(out, np.uint16 if dt == "bf16" else np.float32)
    strided, coalesced = restated([H, B]), restated([B * H])
    assert np.array_equal(raw(t_view).view(np.uint8), strided.view(np.uint8))
    assert np.array_equal(raw(t_cont).view(np.uint8), coalesced.view(np.uint8))
    if dt == "fp32":  # the rule is visible in the bytes
        assert not np.array_equal(strided.view(np.uint8), coalesced.view(np.uint8))


@pytest.mark.parametrize("threads", [1, 8, 16])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_last_dim_step_sum_is_atens_scalar_loop(dt, threads):
    """The rule behind KVC_ATTN_SCALAR_SUM (include/kvc.h): torch's CPU sum over q of an
    attention view whose last dim has a step runs the scalar loop -- per loop call the cascade on
    whole groups of FOUR columns, row_sum on the rest -- with attn_sum_chunk's thread chunks at
    unrounded bounds.  Restated with the oracle's two addition orders and compared with torch."""
    from kvcompress import _cpu_order as CO
    from oracle import h2o_oracle as HO
    rng = np.random.default_rng(1)
    prev = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        for B, H, q, k in ((2, 4, 37, 301), (3, 2, 33, 517), (1, 8, 16, 1501), (2, 4, 120, 37)):
            logits = rng.integers(0, 4, size=(B, H, q, k)).astype(np.float32) * np.float32(0.7)
            a = torch.from_numpy(logits).softmax(dim=-1).to(TORCH_DT[dt])
            view = torch.zeros(B, H, q, 2 * k, dtype=a.dtype)[..., ::2]
            view.copy_(a)
            chunk = CO.attn_sum_chunk(view, threads) or k
            ilp = np.zeros(k, bool)
            for s in range(0, k, chunk):
                e = min(k, s + chunk)
                ilp[s + (e - s) // 4 * 4:e] = True
            x = a.float().numpy()
            want = np.stack([np.stack([HO.sum_reduce_first(x[b, h], ilp) for h in range(H)])
                             for b in range(B)])
            got = view.sum(dim=2)
            assert torch.equal(got, torch.from_numpy(want).to(a.dtype)), (B, H, q, k)
    finally:
        torch.set_num_threads(prev)
