"""torch.gather's NaN rewrite, on the CPU: the rule itself against torch, the engine's scalar
helpers on every 16-bit value, and proofs that the NaN-payload goldens (tests/golden/cases.json,
the cases whose layers carry `vvariant`) cannot be passed by a wrong copy.

The rule (oracle.gather): torch.gather on the CPU turns every bf16 NaN into 0xFFFF and sets bit 9
of every fp16 NaN; fp32 and everything torch.cat / slicing copies keep their bits.  The engine
applies it to the gathered segment of K and V (csrc/kvc_device_util.h canon_nan_dt); the device
side is tests/test_nan_payload_gpu.py.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import fixtures
import prng
from oracle import oracle

DT16 = ("bf16", "fp16")


@pytest.fixture(scope="module")
def model():
    """tests/native/select_model.cpp (the engine's scalar helpers, csrc/kvc_common.h) built into a
    library of this module's own, so that it never races tests/test_select_model.py's build."""
    import test_select_model as M
    out = os.path.join(os.path.dirname(M.OUT), "libselect_model_nan.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = f"{out}.{os.getpid()}.tmp"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-I",
                           os.path.join(M.ROOT, "cs3602-llm-inference-acceleration_amd", "csrc"),
                           M.SRC, "-o", tmp])
    os.replace(tmp, out)
    L = ctypes.CDLL(out)
    L.model_canon_nan_words.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_void_p]
    L.model_canon_nan_words.restype = None
    return L


def rewrite(bits, dtype):
    """The rule on bit patterns, stated once more (numpy only)."""
    bits = np.asarray(bits)
    if dtype == "bf16":
        return np.where((bits & 0x7FFF) > 0x7F80, 0xFFFF, bits).astype(bits.dtype)
    if dtype == "fp16":
        return np.where((bits & 0x7FFF) > 0x7C00, bits | 0x200, bits).astype(bits.dtype)
    return bits


def _torch(a):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.view(torch.int16).view(torch.bfloat16) if a.dtype == np.uint16 else t


def _np_bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()]).numpy().view(
        {2: np.uint16, 4: np.uint32}[t.element_size()])


def _all_patterns(dtype, D):
    """[1, 2, S, D]: head 0 runs through all 65 536 patterns, head 1 through the same shifted by
    one element -- every pattern in both halves of a 32-bit word."""
    if dtype == "fp32":
        T = prng.pattern_table("fp32")
        S = 40
        i = np.arange(S * D)
        return prng.from_bits(np.stack([T[i % len(T)], T[(i + 1) % len(T)]]).reshape(1, 2, S, D),
                              dtype)
    S = -(-65536 // D) + 1
    i = np.arange(S * D)
    x = np.stack([i % 65536, (i + 65535) % 65536]).astype(np.uint16)
    return prng.from_bits(x.reshape(1, 2, S, D), dtype)


# ------------------------------------------------------------------------------------------
# the rule against torch
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("D", [32, 80, 256])
def test_oracle_gather_is_torch_gather_on_every_pattern(dtype, D):
    X = _all_patterns(dtype, D)
    S = X.shape[2]
    rng = np.random.default_rng(D)
    for idx in (np.stack([rng.permutation(S), rng.permutation(S)])[None],           # every row
                np.sort(np.stack([rng.choice(S, S // 3, replace=False) for _ in range(2)]))[None]):
        ti = torch.from_numpy(idx)[..., None].expand(1, 2, idx.shape[2], D)
        want = oracle.gather(X, idx)
        assert np.array_equal(prng.to_bits(want), rewrite(prng.to_bits(X), dtype)[
            0, np.arange(2)[:, None], idx[0]][None])
        for index in (ti, ti.contiguous()):
            got = torch.gather(_torch(X), 2, index)
            assert np.array_equal(_np_bits(got), prng.to_bits(want)), (dtype, D)
    if dtype != "fp32":  # the sweep really holds every pattern in both halves
        b = prng.to_bits(X)
        assert len(np.unique(b[..., 0::2])) == 65536 and len(np.unique(b[..., 1::2])) == 65536


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_oracle_cat_and_slices_are_torch_copies(dtype):
    X = _all_patterns(dtype, 32)
    t = _torch(X)
    S = X.shape[2]
    parts = ((slice(0, 5), slice(S - 300, S)), (slice(0, 0), slice(7, S)), (slice(3, 90),))
    for sl in parts:
        want = oracle.cat([X[:, :, s] for s in sl])
        got = torch.cat([t[:, :, s] for s in sl], dim=2)
        assert np.array_equal(_np_bits(got), prng.to_bits(want))
        assert np.array_equal(prng.to_bits(want),
                              np.concatenate([prng.to_bits(X)[:, :, s] for s in sl], axis=2))
    sliced = t[:, :, -100:].contiguous()
    assert np.array_equal(_np_bits(sliced), prng.to_bits(X)[:, :, -100:])
    picked = t[:, :, torch.arange(0, S, 3)]  # advanced indexing copies too
    assert np.array_equal(_np_bits(picked), prng.to_bits(X)[:, :, ::3])


# ------------------------------------------------------------------------------------------
# the scalar helpers (csrc/kvc_common.h), every value of each half
# ------------------------------------------------------------------------------------------
PARTNERS = (0x0000, 0x8000, 0x3C00, 0x7C00, 0x7C01, 0x7DFF, 0x7E00, 0xFC01, 0x7F80, 0x7F81, 0x7FC0,
            0xFF80, 0xFF81, 0xFFFE, 0xFFFF)


@pytest.mark.parametrize("dtype", DT16)
def test_scalar_helpers_on_every_value_of_each_half(model, dtype):
    every = np.arange(65536, dtype=np.uint32)
    for partner in PARTNERS:
        for lo, hi in ((every, np.full_like(every, partner)), (np.full_like(every, partner), every)):
            w = np.ascontiguousarray(lo | (hi << 16), dtype=np.uint32)
            out = np.empty_like(w)
            model.model_canon_nan_words(w.ctypes.data, len(w), int(dtype == "fp16"),
                                        out.ctypes.data)
            want = rewrite(lo, dtype) | (rewrite(hi, dtype) << 16)
            assert np.array_equal(out, want), (dtype, hex(partner))


# ------------------------------------------------------------------------------------------
# the pattern table and the generators
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_pattern_table(dtype):
    T = prng.pattern_table(dtype)
    nan = prng.is_nan_bits(T, dtype)
    assert len(T) % 2 == 1
    if dtype != "fp32":
        every = np.arange(65536, dtype=np.uint32)
        assert set(T[nan].tolist()) == set(every[prng.is_nan_bits(every, dtype)].tolist())
        assert nan.sum() == {"bf16": 254, "fp16": 2046}[dtype]
    else:
        assert {0x7F800001, 0xFF800001, 0x7FBFFFFF, 0x7FC00000, 0xFFC00001, 0x7FFFFFFF,
                0xFFFFFFFF} <= set(T[nan].tolist())
    assert set(prng.edge_patterns(dtype).tolist()) == set(T[~nan].tolist())
    left, right = np.roll(nan, 1), np.roll(nan, -1)  # cyclic neighbours
    assert (left[nan] != right[nan]).all()  # one NaN and one non-NaN neighbour each
    V = prng.to_bits(prng.gen_values(0, (2, 3, 50, 32), dtype, "patterns"))
    b, h, s, d = 1, 2, 37, 13
    assert V[b, h, s, d] == T[(s * 32 + d + 17 * (b * 3 + h)) % len(T)]


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_payload_keys(dtype):
    K = prng.to_bits(prng.gen_keys(77, (2, 3, 400, 64), dtype, "payload"))
    base = prng.to_bits(prng.gen_keys(77, (2, 3, 400, 64), dtype, "scaled"))
    nan = prng.is_nan_bits(K, dtype)
    rows = nan.any(axis=-1)
    assert (rows == (np.arange(400) % 9 == 4)[None, None]).all()
    assert nan[..., 3].sum() == rows.sum() and 0 < nan[..., 6].sum() < rows.sum()
    assert nan.sum() == nan[..., 3].sum() + nan[..., 6].sum()
    sign = K[nan] >> (K.dtype.itemsize * 8 - 1)
    assert 0 < sign.sum() < sign.size and len(np.unique(K[nan])) >= 8
    changed = (K != base).any(axis=-1)
    assert (K == base)[~changed].all() and changed.sum() < 0.3 * changed.size


# ------------------------------------------------------------------------------------------
# the NaN-payload goldens: segments, coverage conditions, mutants
# ------------------------------------------------------------------------------------------
NAN_CASES = [c["id"] for c in fixtures.cases()["cases"]
             if any("vvariant" in L for L in c["layers"])]


def _traced(case):
    """The oracle's outputs of a case with, per output array, its segments
    [(start, stop, gathered)] -- recorded from the oracle's own gather / cat calls."""
    seg, keep = {}, []
    real_gather, real_cat = oracle.gather, oracle.cat

    def gather(X, idx):
        out = real_gather(X, idx)
        assert out.flags.c_contiguous
        seg[id(out)] = [(0, out.shape[2], True)]
        keep.append(out)
        return out

    def cat(parts):
        out = real_cat(parts)
        at, s = 0, []
        for p in parts:
            if p.shape[2]:
                s.append((at, at + p.shape[2], id(p) in seg))
            at += p.shape[2]
        seg[id(out)] = s
        keep.append(out)
        return out

    oracle.gather, oracle.cat = gather, cat
    try:
        layers = fixtures.make_inputs(case, "data")
        out = oracle.METHODS[case["method"]](layers, **case["kwargs"])
    finally:
        oracle.gather, oracle.cat = real_gather, real_cat
    res = []
    for li, ((K, V), (ko, vo, kind), g) in enumerate(zip(layers, out, case["out"])):
        if kind == "same":
            continue
        pos = fixtures.positions()[g["pos_key"]].astype(np.int64)
        segs = []
        for X, y in ((K, ko), (V, vo)):
            s = seg.get(id(y), [(0, y.shape[2], False)])  # a slice of the input: a plain copy
            assert kind == "new" or not any(x[2] for x in s)
            B, H = X.shape[:2]
            plain = prng.to_bits(X)[np.arange(B)[:, None, None], np.arange(H)[None, :, None], pos]
            segs.append((plain, prng.to_bits(y), s))
        assert segs[0][2] == segs[1][2]
        res.append((li, kind, segs[0], segs[1]))
    return res


_TRACED = {}


def _case(cid):
    if cid not in _TRACED:
        _TRACED[cid] = (fixtures.get_case(cid), _traced(fixtures.get_case(cid)))
    return _TRACED[cid]


def _apply(plain, segs, fn, fixed_too=False):
    """A copy that applies fn to the gathered segments (and, fixed_too, to the others)."""
    out = plain.copy()
    for a, b, gathered in segs:
        if gathered or fixed_too:
            out[:, :, a:b] = fn(plain[:, :, a:b])
    return out


def _words(fn16):
    """A rule on 32-bit words (two 16-bit halves each) as a rule on a 16-bit [.., D] array."""
    def f(x):
        w = np.ascontiguousarray(x).view(np.uint32)
        return np.ascontiguousarray(fn16(w).astype(np.uint32)).view(np.uint16).reshape(x.shape)
    return f


def _pk(nanmin, setbits, carry):
    """canon_nan_pk on words; carry = True: the saturating packed add replaced by one 32-bit add,
    so a low half past 0xFFFF wraps and carries into the high half."""
    def f(w):
        w = w.astype(np.uint64)
        x = w & 0x7FFF7FFF
        c = 0xFFFE - nanmin
        if carry:
            m = (x + (c | (c << 16))) & 0xFFFFFFFF
            lo, hi = m & 0xFFFF, m >> 16
        else:
            lo, hi = np.minimum((x & 0xFFFF) + c, 0xFFFF), np.minimum((x >> 16) + c, 0xFFFF)
        t_lo, t_hi = (lo == 0xFFFF).astype(np.uint64), (hi == 0xFFFF).astype(np.uint64)
        return w | (t_lo * setbits) | ((t_hi * setbits) << 16)
    return f


PK = {"bf16": (0x7F80, 0xFFFF), "fp16": (0x7C00, 0x200)}


def _wide(dtype):
    def f(w):
        lo, hi = w & 0xFFFF, w >> 16
        either = prng.is_nan_bits(lo, dtype) | prng.is_nan_bits(hi, dtype)
        forced = {"bf16": np.uint32(0xFFFFFFFF), "fp16": w | np.uint32(0x02000200)}[dtype]
        return np.where(either, forced, w)
    return f


def _mutants(dtype):
    """name -> (rule on K, rule on V, applied to the fixed segments too)."""
    true = lambda x: rewrite(x, dtype)  # noqa: E731
    none = lambda x: x  # noqa: E731
    if dtype == "fp32":  # nothing is rewritten: the bf16 rule on its halves is the mutant (the
        # fp16 rule sets bit 9, which the high half of every fp32 NaN / inf already has)
        return {"bf16 rule on fp32": (_h(rewrite, "bf16"),) * 2 + (False,)}
    other = {"bf16": "fp16", "fp16": "bf16"}[dtype]
    inf = {"bf16": 0x7F80, "fp16": 0x7C00}[dtype]
    pos_only = lambda x: np.where(x & 0x8000, x, rewrite(x, dtype))  # noqa: E731
    ge_inf = lambda x: rewrite(np.where((x & 0x7FFF) == inf, x | 1, x), dtype)  # noqa: E731
    m = {
        "no rewrite": (none, none, False),
        "rewrite in sink and tail too": (true, true, True),
        "rewrite K only": (true, none, False),
        "rewrite V only": (none, true, False),
        "positive NaNs only": (pos_only, pos_only, False),
        "threshold >= inf": (ge_inf, ge_inf, False),
        f"{other} rule": (lambda x: rewrite(x, other),) * 2 + (False,),
        "word-wide rewrite": (_words(_wide(dtype)),) * 2 + (False,),
        "carry from the low half": (_words(_pk(*PK[dtype], carry=True)),) * 2 + (False,),
    }
    return m


def _h(fn, dtype16):
    """A 16-bit rule applied to the two halves of fp32 elements."""
    def f(x):
        h = np.ascontiguousarray(x).view(np.uint16)
        return np.ascontiguousarray(fn(h, dtype16)).view(np.uint32).reshape(x.shape)
    return f


def test_packed_form_model_equals_the_rule():
    """The numpy model of canon_nan_pk used for the carry mutant: without the carry it IS the
    rule, on every value of each half beside every partner."""
    every = np.arange(65536, dtype=np.uint32)
    for dtype in DT16:
        for partner in PARTNERS:
            for lo, hi in ((every, np.full_like(every, partner)),
                           (np.full_like(every, partner), every)):
                w = lo | (hi << 16)
                want = rewrite(lo, dtype) | (rewrite(hi, dtype) << 16)
                assert np.array_equal(_pk(*PK[dtype], carry=False)(w), want)


@pytest.mark.parametrize("cid", NAN_CASES)
def test_segments_rebuild_the_oracle_output(cid):
    """The harness below is sound: source rows at the golden positions, with the rule on the
    segments the oracle gathered, are the oracle's (= the reference's) bytes."""
    case, layers = _case(cid)
    assert layers, cid
    for li, kind, k, v in layers:
        for plain, want, segs in (k, v):
            got = _apply(plain, segs, lambda x: rewrite(x, case["dtype"]))
            assert np.array_equal(got, want), (cid, li)


def _non_canonical(bits, dtype):
    nan = prng.is_nan_bits(bits, dtype)
    if dtype == "bf16":
        return nan & (bits != 0x7FC0) & (bits != 0xFFFF)
    if dtype == "fp16":
        return nan & ((bits & 0x200) == 0)
    return nan & (bits != 0x7FC00000)


@pytest.mark.parametrize("cid", NAN_CASES)
def test_coverage_conditions(cid):
    case, layers = _case(cid)
    dt = case["dtype"]
    sign = 1 << (8 * prng.BITS[dt]().itemsize - 1)
    T = prng.pattern_table(dt)
    all_nans = set(T[prng.is_nan_bits(T, dt)].tolist())
    lo_seen, hi_seen, partner = set(), set(), set()
    k_rewritten = {0: 0, 1: 0}
    has_gather = False
    for li, kind, (kp, kw, segs), (vp, vw, _) in layers:
        for a, b, gathered in segs:
            v, k = vp[:, :, a:b], kp[:, :, a:b]
            if gathered:
                has_gather = True
                lo, hi = v[..., 0::2], v[..., 1::2]
                ln, hn = prng.is_nan_bits(lo, dt), prng.is_nan_bits(hi, dt)
                lo_seen |= set(lo[ln].tolist())
                hi_seen |= set(hi[hn].tolist())
                for name, m in (("lo nan, hi nan", ln & hn), ("lo nan, hi not", ln & ~hn),
                                ("hi nan, lo not", hn & ~ln)):
                    if m.any():
                        partner.add(name)
                changed = kp[:, :, a:b] != kw[:, :, a:b]
                assert (changed <= prng.is_nan_bits(k, dt)).all()
                if dt == "fp32":
                    changed = prng.is_nan_bits(k, dt)  # nothing is rewritten: count the NaNs
                k_rewritten[0] += int(changed[..., 0::2].sum())
                k_rewritten[1] += int(changed[..., 1::2].sum())
            else:  # sink, tail or slice: payloads kept, of both signs
                for name, x in (("V", v),) + ((("K", k),) if b - a >= 18 else ()):
                    nc = x[_non_canonical(x, dt)]
                    assert (nc & sign).any() and (~nc & sign).any(), (cid, li, a, b, name)
    if not has_gather:
        assert case["method"] in ("streaming_llm", "recent_only", "evict_for_space")
        return
    assert lo_seen == all_nans and hi_seen == all_nans, (cid, len(lo_seen), len(hi_seen))
    assert partner == {"lo nan, hi nan", "lo nan, hi not", "hi nan, lo not"}, (cid, partner)
    assert k_rewritten[0] >= 10 and k_rewritten[1] >= 10 and sum(k_rewritten.values()) >= 20, \
        (cid, k_rewritten)


@pytest.mark.parametrize("cid", NAN_CASES)
def test_wrong_copies_cannot_pass(cid):
    """Every mutant of the copy differs from the oracle's bytes on every layer of every case
    that has the segment the mutant is wrong on."""
    case, layers = _case(cid)
    dt = case["dtype"]
    for li, kind, (kp, kw, segs), (vp, vw, _) in layers:
        has_g = any(g for _, _, g in segs)
        has_f = any(not g for _, _, g in segs)
        if kind != "new":
            continue  # a view of the input: no copy runs
        for name, (fk, fv, fixed_too) in _mutants(dt).items():
            if not (has_f if fixed_too else has_g):
                continue
            gk, gv = _apply(kp, segs, fk, fixed_too), _apply(vp, segs, fv, fixed_too)
            same_k, same_v = np.array_equal(gk, kw), np.array_equal(gv, vw)
            if name == "rewrite K only":
                assert same_k and not same_v, (cid, li, name)
            elif name == "rewrite V only":
                assert same_v and not same_k, (cid, li, name)
            elif name in ("word-wide rewrite", "carry from the low half", "rewrite in sink and tail too",
                          "positive NaNs only", "no rewrite") or "rule" in name:
                assert not same_k and not same_v, (cid, li, name)
            else:  # +-inf rows: V always holds them; K where a kept row is an inf row
                assert not same_v, (cid, li, name)
