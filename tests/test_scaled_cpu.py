"""Per-token-scaled fp8 paged caches on the host: the surrogate construction of scaled_util, the
argument checks of PagedKV that need no GPU, kvc_plan_scaled's contract through ctypes, and the
power of the GPU suites' inputs -- numpy models of wrong engines that each change a stored norm AND
a kept set in every tested (layer, b, h) row, or are caught by the pool comparison -- except the
double rounding, which moves a norm in every row (the SCORE test's byte-for-byte norm region) but
a kept set only in some rows.  CPU only."""
import numpy as np
import pytest
import torch

import fp8_util as F
import scaled_util as SU
import test_abi
import test_paged_plan as PP
import test_ragged_plan as RP
from kvcompress import PagedKV
from kvcompress import _native as N
from oracle import oracle

E_ARG, E_DTYPE, E_ALIGN = -1, -2, -4
SCALE_K, SCALE_V = 32 << 20, 40 << 20   # two 4-byte aligned "device" scale pools
NHP = (PP.P, 1)                         # head / slot strides of a scale pool stored [N, H, P]
NPH = (1, PP.H)                         # ... stored [N, P, H]
SPAGE = PP.H * PP.P


# ---- the surrogate --------------------------------------------------------------------------
def test_surrogate_round_trip_is_the_identity_on_its_range():
    """Over all 32 768 non-negative bf16 patterns: a surrogate row's bf16 norm is the pattern for
    0 and for 2^-63 <= t <= 2^63 (t * t is exact in fp32 there), which is the range the method
    tests stay in; outside it the round trip fails somewhere (denormals, tiny, huge, inf)."""
    t = np.arange(0x8000, dtype=np.uint16)
    k = np.zeros((1, 1, t.size, SU.SURROGATE_D), dtype=np.uint16)
    k[0, 0, :, 0] = t
    back = oracle.norms(k)[0, 0]
    inside = SU.in_surrogate_range(t)
    assert inside.sum() == 1 + 126 * 128 + 1
    assert np.array_equal(back[inside], t[inside])
    assert (back[~inside] != t[~inside]).any()
    with pytest.raises(AssertionError):
        SU.surrogate(np.array([[[0x0001]]], dtype=np.uint16))  # a bf16 denormal


def _same_bf16(got, ref):
    """Equal bit patterns, except that a NaN is 0x7FC0 in `got` (c10::BFloat16's scalar
    round_to_nearest_even, the engine's f32_to_bf16_rne) where torch's tensor conversion gives a
    NaN of whichever pattern its vectorised kernel leaves (0xFFFF on AVX2 hosts)."""
    ref = ref.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = (ref & 0x7FFF) > 0x7F80
    return bool((got[nan] == 0x7FC0).all() and np.array_equal(got[~nan], ref[~nan]))


def test_bf16_rne_is_torchs_conversion():
    rng = np.random.default_rng(5)
    u = rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32)
    u = np.concatenate([u, np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000,
                                     0x7F800001, 0x00000001, 0x00008000, 0x00018000, 0x7F7FFFFF],
                                    dtype=np.uint32)])
    assert _same_bf16(SU.bf16_rne(u.view(np.float32)), torch.from_numpy(u.view(np.float32)))
    assert SU.bf16_rne(np.array([np.nan], np.float32))[0] == 0x7FC0


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_stored_norms_are_the_contracts_torch_expression(fmt):
    """scaled_util.stored_norms == bf16(torch.norm(K8.to(float32), dim=-1) * s.abs()) on the SCORE
    test's inputs (specials included), and with no scale it is the unscaled fp8 call's norm."""
    for D in (64, 128, 256):
        k8, s = SU.score_case(fmt, D)
        k = torch.from_numpy(k8).view(F.torch_dtype(fmt)).to(torch.float32)
        ref = torch.norm(k, dim=-1) * torch.from_numpy(s).abs()
        assert _same_bf16(SU.stored_norms(k8, s, fmt), ref), (fmt, D)
        assert np.array_equal(SU.stored_norms(k8, None, fmt), F.norms_bf16(k8, fmt))
        for u in SU.UNIFORM_SCALES:
            ref = (torch.norm(k, dim=-1) * abs(torch.tensor(u, dtype=torch.float32)))
            assert _same_bf16(SU.stored_norms(k8, np.float32(u), fmt), ref), (fmt, D, u)


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_score_inputs_reach_the_edges(fmt):
    """The SCORE inputs hold products that are fp32 denormals, bf16 denormals, NaN from 0 * inf,
    inf, and products whose bf16 rounding is inexact."""
    k8, s = SU.score_case(fmt, 128)
    p = SU.scaled_f32(k8, s, fmt)
    t = SU.stored_norms(k8, s, fmt)
    tiny = (p > 0) & (p < np.float32(2.0 ** -126))
    assert tiny.sum() >= 16
    assert ((t > 0) & (t < 0x0080)).sum() >= 8            # bf16 denormals
    assert (tiny & (t == 0)).any()                          # ... and products that round to zero
    n32 = SU.norms_f32(k8, fmt)
    assert (np.isnan(p) & (n32 == 0) & np.isinf(s)).any()   # 0 * inf
    if fmt == "e5m2":
        assert (np.isnan(p) & np.isinf(n32) & (s == 0)).any()
    assert np.isinf(p).any() and (np.signbit(s) & (s == 0)).any()
    assert ((p.view(np.uint32) & 0xFFFF) != 0)[np.isfinite(p)].mean() > 0.5  # rounding matters
    for b in range(SU.SCORE_B):                             # every tile of every row has specials
        for h in range(SU.SCORE_H):
            assert np.isnan(s[b, h, :64]).any() and np.isnan(s[b, h, 128:]).any()


# ---- PagedKV's argument checks (the ones that come before the device check) -----------------
def _pools(dtype=torch.float8_e4m3fn, npg=9, H=2, P=16, D=64):
    k = torch.zeros((npg, H, P, D), dtype=torch.uint8).view(dtype) if dtype.itemsize == 1 else \
        torch.zeros((npg, H, P, D), dtype=dtype)
    return k, k.clone(), torch.zeros((1, 8), dtype=torch.int32)


def test_pagedkv_scale_argument_errors():
    k, v, bt = _pools()
    good = torch.ones((9, 2, 16), dtype=torch.float32)
    bad = {
        "not a tensor": (TypeError, dict(k_scale=1.0)),
        "fp16 scale": (TypeError, dict(k_scale=good.half())),
        "int scale": (TypeError, dict(v_scale=good.int())),
        "wrong pages": (ValueError, dict(k_scale=torch.ones((8, 2, 16)))),
        "NPH not permuted": (ValueError, dict(k_scale=torch.ones((9, 16, 2)))),
        "two elements": (ValueError, dict(v_scale=torch.ones(2))),
        "4-D": (ValueError, dict(k_scale=torch.ones((9, 2, 16, 1)))),
        "heads share a scale": (ValueError, dict(k_scale=torch.ones((9, 1, 16)).expand(9, 2, 16))),
        "slots share a scale": (ValueError, dict(v_scale=torch.ones((9, 2, 1)).expand(9, 2, 16))),
        "pages share a scale": (ValueError, dict(k_scale=torch.ones((1, 2, 16)).expand(9, 2, 16))),
    }
    for why, (exc, kw) in bad.items():
        with pytest.raises(exc):
            PagedKV(k, v, bt, 100, **kw)
    for dt in (torch.bfloat16, torch.float16, torch.float32):  # scales belong to fp8 pools
        kb, vb, _ = _pools(dt)
        with pytest.raises(TypeError, match="fp8"):
            PagedKV(kb, vb, bt, 100, k_scale=good)
        with pytest.raises(TypeError, match="fp8"):
            PagedKV(kb, vb, bt, 100, v_scale=torch.ones(1))
    # good scales pass these checks and reach the device check (CPU pools: no CPU fallback)
    for kw in (dict(k_scale=good), dict(k_scale=torch.ones(1), v_scale=good),
               dict(k_scale=torch.ones((9, 16, 2)).permute(0, 2, 1))):
        with pytest.raises(ValueError, match="ROCm device"):
            PagedKV(k, v, bt, 100, **kw)


# ---- kvc_plan_scaled ------------------------------------------------------------------------
def _scales(**kw):
    z = np.zeros(1, dtype=N.SCALES_DTYPE)[0]
    z["k_scale"], z["v_scale"] = SCALE_K, SCALE_V
    z["k_page_stride"] = z["v_page_stride"] = SPAGE
    z["k_stride"], z["v_stride"] = NHP, NPH
    for name, val in kw.items():
        z[name] = val
    return z


def _fp8(**kw):
    return PP._params(**dict(dict(dtype=N.KVC_F8E4M3), **kw))


def _plan(scales, layer=None, pages=None, seqs=None, launch=False, **pkw):
    table = np.array([PP._layer(True) if layer is None else layer], dtype=N.LAYER_DTYPE)
    pg = None if pages is False else \
        np.array([PP._pages(True) if pages is None else pages], dtype=N.PAGES_DTYPE)
    rg = None
    if seqs is not None:
        seqs = np.array(seqs, dtype=N.SEQ_DTYPE)
        rg = np.zeros(1, dtype=N.RAGGED_DTYPE)
        rg[0] = (seqs.ctypes.data, RP.SEQS)
    z = None if scales is None else np.array([scales], dtype=N.SCALES_DTYPE)
    p = _fp8(**pkw)
    rc, info = N.plan_scaled(p, table, pg, rg, z)
    if launch and rc == 0:  # the launch re-validates before it touches the (absent) workspace
        rc = N.launch_scaled(p, table, pg, rg, z, None, 0, None)
    return rc, info, table


def test_struct_size_and_declarations():
    assert N.SCALES_DTYPE.itemsize == 72
    assert {"kvc_plan_scaled", "kvc_launch_scaled"} <= set(N.EXPORTS)
    assert {"kvc_plan_scaled", "kvc_launch_scaled"} <= set(test_abi._declared_functions())
    assert N.lib().kvc_version() == 4 and N.lib().kvc_layer_struct_size() == 136
    assert hasattr(N.lib(), "kvc_plan_scaled") and hasattr(N.lib(), "kvc_launch_scaled")


@pytest.mark.parametrize("ragged", (False, True))
def test_scales_null_is_kvc_plan_ragged_and_plan_info_is_the_unscaled_plans(ragged):
    seqs = RP.GOOD if ragged else None
    for dtype in (N.KVC_F8E4M3, N.KVC_F8E5M2):
        rc0, i0, t0 = _plan(None, seqs=seqs, dtype=dtype)
        table = np.array([PP._layer(True)], dtype=N.LAYER_DTYPE)
        pg = np.array([PP._pages(True)], dtype=N.PAGES_DTYPE)
        rg = None
        if ragged:
            host = np.array(seqs, dtype=N.SEQ_DTYPE)
            rg = np.zeros(1, dtype=N.RAGGED_DTYPE)
            rg[0] = (host.ctypes.data, RP.SEQS)
        rc1, i1 = N.plan_ragged(_fp8(dtype=dtype), table, pg, rg)
        assert rc0 == rc1 == 0
        assert PP._info(i0) == PP._info(i1) and t0.tobytes() == table.tobytes()
        for z in (_scales(), _scales(flags=N.SCALE_K_UNIFORM | N.SCALE_V_NONE),
                  _scales(k_stride=NPH, v_stride=NHP)):
            rc2, i2, t2 = _plan(z, seqs=seqs, dtype=dtype)
            assert rc2 == 0 and PP._info(i2) == PP._info(i0) and t2.tobytes() == t0.tobytes()
        # the launch accepts the planned table and stops at the workspace
        assert _plan(_scales(), seqs=seqs, dtype=dtype, launch=True)[0] == -6
    # scales == NULL keeps the unscaled call's own refusals and non-fp8 dtypes
    assert _plan(None, seqs=seqs, dtype=N.KVC_BF16)[0] == 0


REFUSED = {
    "bf16 pools": (E_DTYPE, dict(), dict(dtype=N.KVC_BF16)),
    "fp32 pools": (E_DTYPE, dict(), dict(dtype=N.KVC_F32, head_dim=64)),
    "reserved": (E_ARG, dict(reserved=1), {}),
    "unknown flag": (E_ARG, dict(flags=16), {}),
    "K uniform and absent": (E_ARG, dict(flags=N.SCALE_K_UNIFORM | N.SCALE_K_NONE), {}),
    "V uniform and absent": (E_ARG, dict(flags=N.SCALE_V_UNIFORM | N.SCALE_V_NONE), {}),
    "K pool NULL": (E_ARG, dict(k_scale=0), {}),
    "V pool NULL": (E_ARG, dict(v_scale=0), {}),
    "uniform K NULL": (E_ARG, dict(k_scale=0, flags=N.SCALE_K_UNIFORM), {}),
    "K pool unaligned": (E_ALIGN, dict(k_scale=SCALE_K + 2), {}),
    "V pool unaligned": (E_ALIGN, dict(v_scale=SCALE_V + 1), {}),
    "uniform K unaligned": (E_ALIGN, dict(k_scale=SCALE_K + 2, flags=N.SCALE_K_UNIFORM), {}),
    "K heads share a scale": (E_ARG, dict(k_stride=(0, 1)), {}),
    "V heads share a scale": (E_ARG, dict(v_stride=(0, PP.H)), {}),
    "K slots share a scale": (E_ARG, dict(k_stride=(PP.P, 0)), {}),
    "V slots share a scale": (E_ARG, dict(v_stride=(1, 0)), {}),
    "K pages share a scale": (E_ARG, dict(k_page_stride=0), {}),
    "V pages share a scale": (E_ARG, dict(v_page_stride=0), {}),
}


@pytest.mark.parametrize("ragged", (False, True))
@pytest.mark.parametrize("why", list(REFUSED))
def test_refusals_give_their_status(why, ragged):
    code, zkw, pkw = REFUSED[why]
    seqs = RP.GOOD if ragged else None
    assert _plan(_scales(), seqs=seqs)[0] == 0
    assert _plan(_scales(**zkw), seqs=seqs, **pkw)[0] == code, why


def test_scaled_layers_are_paged_and_in_place():
    assert _plan(_scales(), pages=False)[0] == E_ARG                      # a dense layer
    assert _plan(_scales(), pages=PP._pages(False), layer=PP._layer(False))[0] == E_ARG
    # (the same dense-output call is fine without scales)
    assert _plan(None, pages=PP._pages(False), layer=PP._layer(False))[0] == 0
    # what is not read is not checked: strides and pointers of uniform / absent sides
    none = N.SCALE_K_NONE | N.SCALE_V_NONE
    z = _scales(flags=none, k_scale=0, v_scale=0, k_page_stride=0, v_stride=(0, 0))
    assert _plan(z)[0] == 0
    assert _plan(_scales(flags=N.SCALE_K_UNIFORM | N.SCALE_V_UNIFORM, v_scale=3, k_stride=(0, 0),
                         k_page_stride=0))[0] == 0
    # one head, one page, one slot: strides of dims of size 1 may be zero
    lay = PP._layer(True, seq_len=1, sink=0, zs=0, zl=0, k=0, ts=0, tl=1)
    one = PP._pages(True, num_pages=1, page_size=1, table_stride=1)
    z = _scales(k_stride=(0, 0), v_stride=(0, 0), k_page_stride=0, v_page_stride=0)
    assert _plan(z, layer=lay, pages=one, heads=1, batch=1)[0] == 0
    # external indices work on single-length layers; ragged ones refuse them as without scales
    ext = dict(external_index=1, phases=N.PHASE_GATHER)
    assert _plan(_scales(), **ext)[0] == 0
    assert _plan(_scales(), flags=N.FLAG_SHARED_INDEX, **ext)[0] == 0
    assert _plan(_scales(), seqs=RP.GOOD, **ext)[0] == E_ARG


# ---- the power of the GPU suites' inputs ----------------------------------------------------
KW = dict(fix_kv_size=128, keep_ratio=0.0, skip_layers=[])


def _rows_differ(a, b):
    """[B, H] bool: rows whose last axis (axes) differ."""
    d = a != b
    return d.reshape(d.shape[0], d.shape[1], -1).any(axis=2)


def _kept_sets(norms):
    return [np.sort(p, axis=2) for p in
            SU.kept_positions(oracle.fix_size_l2_compress, norms, **KW)]


@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_wrong_engines_change_a_norm_and_a_kept_set_in_every_row(fmt, D):
    layers = SU.method_layers(91000, D, fmt)
    right = [SU.stored_norms(k8, ks, fmt) for k8, _, ks, _ in layers]
    assert all(SU.in_surrogate_range(t).all() for t in right)
    kept = _kept_sets(right)
    for k8, _, ks, _ in layers:  # the generator: row magnitudes over 2^6, raw fp8 norms alike
        mag = SU.norms_f32(k8, fmt) * np.abs(ks)
        assert (mag.max(axis=2) / mag.min(axis=2) >= 2.0 ** 6).all()
        raw = SU.norms_f32(k8, fmt)
        assert (raw.max(axis=2) / raw.min(axis=2) < 4).all()
        assert (ks < 0).any(axis=2).all()
    wrong = {
        "scales ignored": [SU.stored_norms(k8, None, fmt) for k8, _, _, _ in layers],
        "V scales used": [SU.stored_norms(k8, vs, fmt) for k8, _, _, vs in layers],
    }
    for why, norms in wrong.items():
        sets = _kept_sets(norms)
        for li in range(len(layers)):
            assert _rows_differ(norms[li], right[li]).all(), (why, li, "norms")
            assert _rows_differ(sets[li], kept[li]).all(), (why, li, "kept set")
    # bf16(bf16(norm) * |s|), the double rounding: it moves about a quarter of the stored norms by
    # one bf16 ulp -- in EVERY row, which the SCORE test's byte-for-byte norm region catches -- but
    # a kept set only where a moved norm sits at the selection boundary: in some rows of these
    # layers, not in every one (measured: 1 to 3 of the 4 rows, depending on format and D).  So
    # this one is named as caught by the norm-region comparison, and here by at least one row
    dbl = [SU.bf16_rne(oracle.as_float(SU.stored_norms(k8, None, fmt)) * np.abs(ks))
           for k8, _, ks, _ in layers]
    sets = _kept_sets(dbl)
    moved = 0
    for li in range(len(layers)):
        assert _rows_differ(dbl[li], right[li]).all(), ("double rounding", li, "norms")
        assert 0.1 < (dbl[li] != right[li]).mean() < 0.5
        moved += int(_rows_differ(sets[li], kept[li]).sum())
    assert moved >= 1, "double rounding keeps every kept set"
    # s without the absolute value: negative products sort first under keep_low, so such an engine
    # keeps (one of) the most negative rows of the zone -- the negative-scale row of the LARGEST
    # magnitude -- which the right engine, keeping the smallest magnitudes, does not.  (Negative
    # bf16 bits are outside the surrogate's range: modelled on the floats.)
    keep = KW["fix_kv_size"] - int(KW["fix_kv_size"] * KW["keep_ratio"])
    for li, (k8, _, ks, _) in enumerate(layers):
        signed = oracle.as_float(right[li]) * np.sign(ks)
        zone = signed[:, :, :signed.shape[2] - (KW["fix_kv_size"] - keep)]
        lowest = zone == zone.min(axis=2, keepdims=True)
        assert (zone.min(axis=2) < 0).all(), li
        kept_mask = np.zeros(zone.shape, dtype=bool)
        np.put_along_axis(kept_mask, kept[li][:, :, :keep], True, axis=2)
        assert kept_mask.sum(axis=2).min() == keep
        assert not (lowest & kept_mask).any(axis=2).any(), li


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_wrong_scale_copies_are_caught_by_the_pool_comparison(fmt):
    """Scale words left behind, moved from row t instead of src(t) (the same bytes: row t's own
    scale stays at t), and K / V scale pools swapped: each leaves, in every (layer, b, h) row, a
    scale word that differs from the expectation the methods test compares the pools with."""
    layers = SU.method_layers(91000, 128, fmt)
    right = [SU.stored_norms(k8, ks, fmt) for k8, _, ks, _ in layers]
    pos = SU.kept_positions(oracle.fix_size_l2_compress, right, **KW)
    for p, (k8, v8, ks, vs) in zip(pos, layers):
        _, _, wk, wv = SU.expected_layer(p, k8, v8, ks, vs)
        n = p.shape[2]
        assert _rows_differ(wk, SU.words(ks)[:, :, :n]).all()   # left behind / moved from row t
        assert _rows_differ(wv, SU.words(vs)[:, :, :n]).all()
        assert _rows_differ(wk, SU.take(SU.words(vs), p)).all()  # pools swapped
        assert _rows_differ(wk, wv).all()
