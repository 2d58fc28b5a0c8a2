"""fp8 K/V caches, the CPU side: the upcast rule the contract rests on, the C ABI's planners, the
reference goldens (tests/golden/gen_fp8_goldens.py) reproduced by the helper, and the power of the
test inputs against wrong decoders and wrong norm orders.  (GPU: test_fp8_score_gpu.py,
test_fp8_methods_gpu.py, test_fp8_delivery_gpu.py.)"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import fp8_util as F
import prng
from kvcompress import _native as N
from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
KVC = {"e4m3": N.KVC_F8E4M3, "e5m2": N.KVC_F8E5M2}


# ---- 1. the upcast rule ------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_every_pattern_upcasts_to_bf16_exactly(fmt):
    codes = np.arange(256, dtype=np.uint8)
    t8 = torch.from_numpy(codes).view(F.torch_dtype(fmt))
    f32 = t8.to(torch.float32)
    b16 = t8.to(torch.bfloat16)
    nan = torch.isnan(f32)
    assert torch.equal(torch.isnan(b16), nan)
    assert torch.equal(b16.to(torch.float32)[~nan], f32[~nan])  # exact: nothing is rounded
    assert sorted(codes[nan.numpy()]) == sorted(F.NAN_CODES[fmt])
    assert sorted(codes[torch.isinf(f32).numpy()]) == sorted(F.INF_CODES[fmt])
    # the helper's table is torch's conversion (NaNs: as NaNs)
    mine = F.to_f32(codes, fmt)
    assert np.array_equal(np.isnan(mine), nan.numpy())
    assert np.array_equal(mine[~nan.numpy()].view(np.uint32), f32[~nan].numpy().view(np.uint32))
    bits = F.to_bf16_bits(codes, fmt)
    got = b16.view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(bits[~nan.numpy()], got[~nan.numpy()])
    assert ((bits[nan.numpy()] & 0x7FFF) > 0x7F80).all()
    assert float(np.nanmax(np.where(np.isinf(mine), np.nan, mine))) == \
        {"e4m3": 448.0, "e5m2": 57344.0}[fmt]


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_quantize_is_torchs_rounding_on_finite_in_range_values(fmt):
    x = prng.normal_f32(4242, 1 << 16) * np.float32(3.0)
    grid = F.to_f32(np.arange(256, dtype=np.uint8), fmt)
    mids = (grid[1:F.MAX_CODE[fmt] + 1] + grid[:F.MAX_CODE[fmt]]) * np.float32(0.5)  # every tie
    x = np.concatenate([x, mids, -mids, grid[np.isfinite(grid)]]).astype(np.float32)
    want = torch.from_numpy(x).to(F.torch_dtype(fmt)).view(torch.uint8).numpy()
    assert np.array_equal(F.quantize(x, fmt), want)


# ---- 2. the C ABI -----------------------------------------------------------------------------
def _layer(S, zl, k, D, es, sink=0, ts=0, tl=0, B=1, H=4):
    t = np.zeros(1, dtype=N.LAYER_DTYPE)[0]
    t["k"] = t["v"] = t["k_out"] = t["v_out"] = 4096
    t["k_stride"] = t["v_stride"] = (H * S * D, S * D, D)
    t["seq_len"], t["zone_start"], t["zone_len"], t["n_select"] = S, sink, zl, k
    t["sink_len"], t["tail_start"], t["tail_len"] = sink, ts, tl
    return t


def _params(dtype, D, B=1, H=4, **kw):
    d = dict(dtype=dtype, batch=B, heads=H, head_dim=D, order=0, algo=0, phases=N.PHASE_ALL,
             external_index=0)
    d.update(kw)
    return N.Params(**d)


def _table(D):
    return np.array([_layer(1500, 1400, 300, D, 1, sink=4, ts=1404, tl=96),
                     _layer(20000, 20000, 512, D, 1),
                     _layer(300, 0, 0, D, 1, sink=4, ts=200, tl=100)], dtype=N.LAYER_DTYPE)


@pytest.mark.parametrize("fmt", F.FORMATS)
@pytest.mark.parametrize("D", (64, 128, 256))
def test_plan_accepts_fp8_with_the_bf16_workspace(fmt, D):
    t8, t16 = _table(D), _table(D)
    rc8, i8 = N.plan(_params(KVC[fmt], D), t8)
    rc16, i16 = N.plan(_params(N.KVC_BF16, D), t16)
    assert rc8 == 0 and rc16 == 0
    for f in ("norm_offset", "index_offset", "workspace_bytes", "norm_row_stride",
              "index_row_stride", "rows", "score_tiles"):
        assert getattr(i8, f) == getattr(i16, f), f
    assert i8.norm_row_stride == 20032  # 2-byte norm elements: the index region starts behind them
    assert i8.index_offset >= i8.rows * i8.norm_row_stride * 2
    nc = D // 16                        # 16-byte units of a D-byte row
    assert list(t8["n_out"]) == list(t16["n_out"]) == [400, 512, 104]
    assert list(t8["unit0"]) == [0, 2 * 4 * 400 * nc, 2 * 4 * (400 + 512) * nc]
    assert i8.gather_units == 2 * 4 * (400 + 512 + 104) * nc
    assert i16.gather_units == 2 * i8.gather_units
    for f in ("row0", "tile0"):
        assert list(t8[f]) == list(t16[f])


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_plan_refuses_other_head_dims_and_byte_misaligned_strides(fmt):
    for D in (32, 80, 96, 512, 16, 48):
        assert N.plan(_params(KVC[fmt], D), _table(D))[0] == -3, D  # KVC_E_HEADDIM
    # 16-byte aligned as bf16 (8 elements), not as fp8 (8 bytes)
    for dim, B, H in ((0, 2, 4), (1, 1, 4), (2, 1, 4)):
        t = _table(128)
        t["k_stride"][:, dim] += 8
        assert N.plan(_params(N.KVC_BF16, 128, B=B, H=H), t.copy())[0] == 0
        assert N.plan(_params(KVC[fmt], 128, B=B, H=H), t.copy())[0] == -4, dim  # KVC_E_ALIGN
    for bad in (3, 5, 4, 15, 18):  # neighbours of the new codes stay refused
        assert N.plan(_params(bad, 128), _table(128))[0] == -2


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_dest_paged_and_ragged_planners_accept_fp8(fmt):
    D, H, S = 128, 4, 1500
    p = _params(KVC[fmt], D, H=H)
    table = np.array([_layer(S, 1400, 300, D, 1, sink=4, ts=1404, tl=96)], dtype=N.LAYER_DTYPE)
    # strided destination [1, H, 512, D] far from the source
    t = table.copy()
    t["k_out"], t["v_out"] = 1 << 30, 1 << 31
    dests = np.zeros(1, dtype=N.DEST_DTYPE)
    dests[0]["k_stride"] = dests[0]["v_stride"] = (H * 512 * D, 512 * D, D)
    rc, info = N.plan_dest(p, t, dests)
    assert rc == 0 and info.gather_units == 2 * H * 400 * (D // 16)
    dests[0]["k_stride"][2] = D + 8  # 8 bytes: misaligned for 1-byte elements
    assert N.plan_dest(p, t.copy(), dests)[0] == -4
    # in place
    t = table.copy()
    dests = np.zeros(1, dtype=N.DEST_DTYPE)
    dests[0]["k_stride"], dests[0]["v_stride"] = t[0]["k_stride"], t[0]["v_stride"]
    dests[0]["in_place"] = 1
    assert N.plan_dest(p, t, dests)[0] == 0
    # paged, [N, P, H, D] pools of 16-row pages, in place
    P = 16
    npages = -(-S // P)
    t = table.copy()
    t["k_stride"] = t["v_stride"] = (0, D, H * D)
    pages = np.zeros(1, dtype=N.PAGES_DTYPE)
    pages[0] = (8192, npages, P * H * D, P * H * D, P, npages, 1, 0)
    rc, info = N.plan_paged(p, t, pages, None)
    assert rc == 0 and info.norm_row_stride == 1408
    pages[0]["k_page_stride"] += 8
    assert N.plan_paged(p, t.copy(), pages, None)[0] == -4
    pages[0]["k_page_stride"] -= 8
    # ragged: two sequences
    p2 = _params(KVC[fmt], D, B=2, H=H)
    seqs = np.zeros(2, dtype=N.SEQ_DTYPE)
    for i, (s, zl, k) in enumerate(((1500, 1400, 300), (700, 600, 300))):
        seqs[i] = (s, 4, zl, k, 4, 4 + zl, 96, 0, 0, 4 + k + 96, (0, 0))
    ragged = np.zeros(1, dtype=N.RAGGED_DTYPE)
    ragged[0] = (seqs.ctypes.data, 1 << 20)
    paged_table = t.copy()
    rc, info = N.plan_ragged(p2, t, pages, ragged)
    assert rc == 0 and info.rows == 2 * H and info.norm_row_stride == 1408
    rc16, i16 = N.plan_ragged(_params(N.KVC_BF16, D, B=2, H=H), paged_table, pages, ragged)
    assert rc16 == 0 and i16.workspace_bytes == info.workspace_bytes


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_attention_entries_refuse_fp8(fmt):
    import ctypes
    ap = N.AttnParams(dtype=KVC[fmt], batch=1, heads=2, vec_bytes=32, decay=1.0, flags=0,
                      device_status=None)
    hh = np.zeros(1, dtype=N.HH_LAYER_DTYPE)
    hh[0] = (4096, 100, 0, 100, 10, 0, 0)
    assert N.hh_workspace(ap, hh)[0] == -2
    assert N.heavy_hitters(ap, hh, 4096, 16, 4096, 1 << 20, None) == -2
    al = np.zeros(1, dtype=N.ATTN_LAYER_DTYPE)
    al[0] = (4096, (200, 100, 100), 0, 8192, 1, 100, 0, 0)
    assert N.attn_accumulate(ap, al, None) == -2
    del ctypes


# ---- 3. the reference goldens -----------------------------------------------------------------
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def golden_cases():
    with open(os.path.join(HERE, "golden", "fp8_cases.json")) as f:
        return json.load(f)


def golden_positions():
    return np.load(os.path.join(HERE, "golden", "fp8_positions.npz"))


def golden_inputs(c):
    ks = [F.gen_keys(L["kseed"], tuple(L["shape"]), c["fmt"], L["variant"]) for L in c["layers"]]
    vs = [F.gen_values(L["kseed"], tuple(L["shape"]), c["fmt"]) for L in c["layers"]]
    return ks, vs


def test_goldens_cover_every_method_and_format():
    cases = golden_cases()
    assert {(c["method"], c["fmt"]) for c in cases} >= {(m, f) for m in F.METHODS
                                                        for f in F.FORMATS}
    assert {c["layers"][0]["variant"] for c in cases} == {"normal", "few", "special"}
    assert all(len(c["layers"]) == 3 for c in cases)
    sp = [c for c in cases if c["layers"][0]["variant"] == "special"]
    for c in sp:  # NaN rows in both formats, inf rows in e5m2
        k = golden_inputs(c)[0][0]
        assert np.isin(k, F.NAN_CODES[c["fmt"]]).any()
        assert np.isin(k, F.INF_CODES[c["fmt"]]).any() == (c["fmt"] == "e5m2")


@pytest.mark.parametrize("cid", [c["id"] for c in golden_cases()])
def test_helper_reproduces_reference_golden(cid):
    c = next(x for x in golden_cases() if x["id"] == cid)
    pos_file = golden_positions()
    ks, vs = golden_inputs(c)
    fn = F.ORACLE_METHODS[c["method"]][0]
    pos = F.kept_positions(fn, ks, c["fmt"], **c["kwargs"])
    for i, (k, v, p, r) in enumerate(zip(ks, vs, pos, c["layers_out"])):
        assert _sha(k) == r["k_input_sha"] and _sha(v) == r["v_input_sha"], "input recipe drifted"
        assert np.array_equal(p, pos_file[f"{cid}/{i}"].astype(np.int64)), (cid, i)
        assert _sha(F.take_rows(k, p)) == r["k_sha"] and _sha(F.take_rows(v, p)) == r["v_sha"]


# ---- 4. power ---------------------------------------------------------------------------------
def _norm_bits(vals_f32, order, rnd):
    """L2 norms [rows] of float32 [rows, D]: the 8-lane FMA order of torch.norm on bf16 (what the
    oracle restates; here spelled out so that WRONG variants can be built) or fp16's one
    accumulator; rounded to bf16 or fp16 bits.  x*x and the fmas are exact-or-correctly-rounded in
    float64 -> float32 steps: each step rounds a float64 product-sum of float32 values once."""
    rows, D = vals_f32.shape
    x = vals_f32.astype(np.float64)

    def fma(a, acc):
        return (a * a + acc.astype(np.float64)).astype(np.float32)  # a*a exact in fp64
    if order == "8lane":
        acc = np.zeros((rows, 8), dtype=np.float32)
        for j in range(0, D, 8):
            acc = fma(x[:, j:j + 8], acc)
        s = acc[:, 0]
        for j in range(1, 8):
            s = (s + acc[:, j]).astype(np.float32)
    else:
        s = np.zeros(rows, dtype=np.float32)
        for j in range(D):
            s = fma(x[:, j], s)
    r = np.sqrt(s.astype(np.float64)).astype(np.float32)
    if rnd == "bf16":
        return prng.f32_to_bf16_bits(r)
    with np.errstate(over="ignore"):
        return r.astype(np.float16)


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_wrong_implementations_change_norms_and_kept_sets(fmt):
    """On the parity tests' inputs (S = 1500, D = 128; "normal" keys, the "special" keys with
    their NaN, zero and -0 rows, and the "order" keys of fp8_util.order_rows with a decode-shaped
    selection): each wrong decode or wrong reduction changes at least one norm
    byte and at least one kept set, so none could pass them.  (A fnuz decode halves every finite
    value -- an exact scaling keeps every order and tie -- but reads -0 as NaN and 0x7F / 0xFF as
    numbers: it is the special rows that catch it.)"""
    S, D, keep = 1500, 128, 128
    other = "e5m2" if fmt == "e4m3" else "e4m3"
    wrong = {
        "decoded as the other format": lambda k8: (F.decode_table(other)[k8], "8lane", "bf16"),
        "decoded as fnuz": lambda k8: (F.decode_table(fmt, fnuz=True)[k8], "8lane", "bf16"),
        "fp16's single-accumulator order": lambda k8: (F.to_f32(k8, fmt), "serial", "bf16"),
        "norm rounded to fp16": lambda k8: (F.to_f32(k8, fmt), "8lane", "fp16"),
    }
    norm_differs = dict.fromkeys(wrong, False)
    kept_differs = dict.fromkeys(wrong, False)

    def kept(norm_vals):
        return np.sort(oracle.argsort_prefix(norm_vals, keep), axis=-1)
    keeps = {"normal": 128, "special": 128, "order": S - F.ORDER_ROWS}
    for variant in keeps:
        keep = keeps[variant]
        k8 = F.gen_keys_order(9100, (1, 2, S, D), fmt) if variant == "order" else \
            F.gen_keys(9100, (1, 2, S, D), fmt, variant)
        good = F.norms_bf16(k8, fmt)
        with np.errstate(invalid="ignore", over="ignore"):
            right = _norm_bits(F.to_f32(k8, fmt).reshape(-1, D), "8lane", "bf16")
        nan = (good & 0x7FFF) > 0x7F80
        assert np.array_equal(right.reshape(good.shape)[~nan], good[~nan])  # the oracle's reduction
        assert np.array_equal((right.reshape(good.shape) & 0x7FFF) > 0x7F80, nan)
        want = kept(good)
        for name, make in wrong.items():
            vals, order, rnd = make(k8)
            with np.errstate(invalid="ignore", over="ignore"):
                nb = _norm_bits(vals.reshape(-1, D), order, rnd).reshape(good.shape)
            norm_differs[name] |= not np.array_equal(nb.view(np.uint16), good)
            kept_differs[name] |= not np.array_equal(kept(nb), want)
    assert all(norm_differs.values()), norm_differs
    assert all(kept_differs.values()), kept_differs


# ---- 5. the SCORE test's inputs pin the decode ---------------------------------------------------
@pytest.mark.parametrize("D", (64, 128, 256))
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_score_inputs_show_any_wrong_decode_of_any_pattern_at_any_lane(fmt, D):
    """tests/test_fp8_score_gpu.py compares norms rounded to bf16, so a planted pattern is pinned
    only if the expected norm moves when that pattern alone is decoded wrongly.  In the zero-
    background rows it always does: per lane, the expected norms of the 256 patterns are NaN exactly
    for the NaN patterns, inf exactly for the inf patterns, and otherwise one distinct value per
    magnitude -- so decoding a pattern as ANY other magnitude of the format (zero, a neighbour, the
    other format's or a fnuz value) changes a norm byte."""
    k8 = F.score_keys(fmt, D)
    want = F.norms_bf16(F.score_zone(k8), fmt).reshape(-1, F.SCORE_ZONE_LEN)
    vals = np.abs(F.to_f32(np.arange(256, dtype=np.uint8), fmt))
    for lane in range(F.SCORE_LANES):
        n = want[lane, :256]
        nan = (n & 0x7FFF) > 0x7F80
        assert sorted(np.flatnonzero(nan)) == sorted(F.NAN_CODES[fmt])
        assert sorted(np.flatnonzero(n == 0x7F80)) == sorted(F.INF_CODES[fmt])
        by_norm, by_value = {}, {}
        for t in np.flatnonzero(~nan):
            by_norm.setdefault(int(n[t]), set()).add(float(vals[t]))
            by_value.setdefault(float(vals[t]), set()).add(int(n[t]))
        assert all(len(v) == 1 for v in by_norm.values()), (fmt, D, lane)   # norm -> one magnitude
        assert all(len(v) == 1 for v in by_value.values()), (fmt, D, lane)  # and back
        assert len(by_norm) == len(set(vals[~nan].tolist()))
        # the norm is the pattern's own: |x| * sqrt(D / 16), exactly rounded
        x = vals[~nan].astype(np.float64) * np.sqrt(D / 16)
        with np.errstate(over="ignore"):
            assert np.array_equal(prng.f32_to_bf16_bits(x.astype(np.float32)), n[~nan])
    # and the background rows differ from the zero-background ones (they are a case of their own)
    assert not np.array_equal(want[F.SCORE_LANES:, :256], want[:F.SCORE_LANES, :256])
