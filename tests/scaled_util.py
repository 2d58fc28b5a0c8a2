"""Per-token-scaled fp8 paged caches: inputs and CPU expectations of the test_scaled_* suites.

The contract (include/kvc.h, "Per-token-scaled fp8 paged caches"): SCORE's stored norm of a key
row with scale s is

    bf16( torch.norm(K8.to(float32), dim=-1) * |s| )

-- the fp32 norm, ONE fp32 multiply, ONE bf16 rounding -- and everything behind it is the bf16
call on those stored norms; GATHER moves the kept rows' bytes and the 4 bytes of their K and V
scales.  So every expectation here is

    1. t = stored_norms(k8, s): oracle.norms on the exact fp32 upcast, one fp32 multiply by |s|,
       round to nearest even to bf16 bits (written out below in integers);
    2. the existing oracle method on SURROGATE bf16 keys [B, H, S, 32] whose element 0 is t and
       whose other elements are 0 (a surrogate row's bf16 norm is t itself whenever t * t is exact
       in fp32: 0 and 2^-63 <= t <= 2^63; `surrogate` asserts the round trip on every t it takes),
       with position-encoding V, as fp8_util.kept_positions works;
    3. the K / V bytes and the scale words at the kept positions.

Nothing is computed by the engine.  Numpy only; fp8 tensors are uint8 arrays of bit patterns,
scales float32 arrays whose words are compared as uint32.
"""
import numpy as np

import fp8_util as F
import prng
from oracle import oracle

SURROGATE_D = 32
AMAX = {"e4m3": 448.0, "e5m2": 57344.0}  # the formats' largest finite values


def bf16_rne(x):
    """float32 -> bf16 bit patterns (uint16): c10::BFloat16's round to nearest even, every NaN
    0x7FC0.  Integer arithmetic: no dependence on the host's FP mode."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + ((u >> 16) & 1) + 0x7FFF) >> 16).astype(np.uint16)
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, np.uint16(0x7FC0), r)


def norms_f32(k8, fmt):
    """torch.norm(K8.to(float32), dim=-1): [B, H, S] float32 (the 8-lane order, unrounded)."""
    return oracle.norms(F.to_f32(k8, fmt))


def scaled_f32(k8, s, fmt):
    """The fp32 product norm * |s| of the contract ([B, H, S]; s broadcasts: a uniform scale is
    one element).  numpy keeps fp32 denormal products, as torch on the CPU does."""
    with np.errstate(all="ignore"):
        return (norms_f32(k8, fmt) * np.abs(np.asarray(s, dtype=np.float32))).astype(np.float32)


def stored_norms(k8, s, fmt):
    """The norm region of the contract: [B, H, S] bf16 bit patterns.  s None: no K scale."""
    if s is None:
        return bf16_rne(norms_f32(k8, fmt))
    return bf16_rne(scaled_f32(k8, s, fmt))


def surrogate(t):
    """bf16 keys [B, H, S, 32] whose rows' bf16 norms are the bit patterns t [B, H, S]."""
    t = np.asarray(t, dtype=np.uint16)
    k = np.zeros(t.shape + (SURROGATE_D,), dtype=np.uint16)
    k[..., 0] = t
    assert np.array_equal(oracle.norms(k), t), "a stored norm outside the surrogate's exact range"
    return k


def in_surrogate_range(t):
    """The patterns whose round trip is the identity by construction: 0 and 2^-63 .. 2^63."""
    t = np.asarray(t, dtype=np.uint16)
    return (t == 0) | ((t >= ((127 - 63) << 7)) & (t <= ((127 + 63) << 7)))


def kept_positions(oracle_fn, norms, **kwargs):
    """Per layer the source position of every output row [B, H, n_out] of the oracle method on
    layers whose stored norms are `norms` (a list of [B, H, S] bf16 bit patterns)."""
    layers = [(surrogate(t), prng.encode_positions(t.shape + (SURROGATE_D,), "bf16"))
              for t in norms]
    out = []
    for (_, v, _) in oracle_fn(layers, **kwargs):
        pos, ok = prng.decode_positions(v, "bf16")
        assert ok
        out.append(pos)
    return out


def take(x, pos):
    """x[b, h, pos[b, h, t]] for rows [B, H, S, D] or scale words [B, H, S]."""
    if x.ndim == 4:
        return F.take_rows(x, pos)
    return np.take_along_axis(x, pos.astype(np.int64), axis=2)


# ---- inputs ---------------------------------------------------------------------------------
def quantize_per_token(x, fmt):
    """Per-token quantisation of float32 rows [..., D]: s = amax / max finite (fp32), codes of
    x / s.  Returns (uint8 codes, float32 scales [...]); an all-zero row gets scale 1."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    amax = np.abs(x).max(axis=-1)
    s = (amax / np.float32(AMAX[fmt])).astype(np.float32)
    s = np.where(s == 0, np.float32(1), s).astype(np.float32)
    return F.quantize((x / s[..., None]).astype(np.float32), fmt), s


def gen_layer(seed, shape, fmt, spread=6):
    """(k8, v8, ks, vs): keys and values whose row magnitudes spread over 2^spread (a seeded
    exponent per row, uniform in [-spread / 2, spread / 2]), per-token quantised.  The raw fp8
    norms are then all about equal and the ranking lives in the scales."""
    B, H, S, D = shape
    rng = np.random.default_rng(seed)

    def one(sd, sub):
        x = prng.gen_keys(sd, shape, "fp32", "normal") if sub == 0 else \
            prng.gen_values(sd, shape, "fp32")
        mag = np.exp2(rng.uniform(-spread / 2, spread / 2, (B, H, S))).astype(np.float32)
        return quantize_per_token((x * mag[..., None]).astype(np.float32), fmt)
    k8, ks = one(seed, 0)
    v8, vs = one(seed, 1)
    return k8, v8, ks, vs


# ---- the inputs of the SCORE test (tests/test_scaled_score_gpu.py) ---------------------------
SCORE_B, SCORE_H, SCORE_S = 2, 2, 130  # two full 64-token tiles and a 2-token one
NAN_PAYLOAD = 0x7FC12345
UNIFORM_SCALES = (0.37, -1.5, 2.0 ** -134, float("inf"))


def score_case(fmt, D):
    """(k8 [2, 2, 130, D], s [2, 2, 130] float32): quantised normal keys with a zero row (token 5)
    and -- e5m2 -- a row with an inf element (token 6); scales that are powers of two (row 0),
    ordinary values whose product needs rounding (rows 1 .. 3, a quarter of them negative), and at
    tokens 0 .. 15 and in the 2-token tile of EVERY row the special ones: +-0, inf, -inf, a NaN
    with a payload, and scales that make norm * |s| an fp32 denormal that is a bf16 denormal
    (about 2^-128 .. 2^-133) or that rounds to bf16 zero or to the smallest bf16 denormal."""
    B, H, S = SCORE_B, SCORE_H, SCORE_S
    k8 = F.gen_keys(81000 + D, (B, H, S, D), fmt, "normal")
    assert not np.isin(k8, F.NAN_CODES[fmt] + F.INF_CODES[fmt]).any()
    k8[:, :, 5] = 0
    if fmt == "e5m2":
        k8[:, :, 6, 3] = 0x7C
    rng = np.random.default_rng(82000 + D)
    s = rng.uniform(1e-3, 3.0, (B, H, S)).astype(np.float32)
    s = np.where(rng.random((B, H, S)) < 0.25, -s, s).astype(np.float32)
    s[0, 0] = np.exp2(rng.integers(-40, 41, S)).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, np.inf, 0.0,
                        2.0 ** -130, 2.0 ** -133, 1.37 * 2.0 ** -134, 2.0 ** -137,
                        -(2.0 ** -139), 1.9 * 2.0 ** -141, 2.0 ** -145, 2.0 ** -149, -2.5],
                       dtype=np.float32)
    special.view(np.uint32)[4] = NAN_PAYLOAD
    s[:, :, :16] = special        # tokens 5 / 6: inf * 0 (the zero row), 0 * inf (e5m2's inf row)
    s[:, :, 128] = np.float32(1.37 * 2.0 ** -134)
    s[:, :, 129].view(np.uint32)[...] = NAN_PAYLOAD | 0x80000000
    return k8, s


METHOD_H = 2
METHOD_LENS = (600, 1500)        # the single-length layers of the method tests
RAGGED_LENS = (0, 37, 512, 513, 1500)


def method_layer(seed, S, D, fmt, H=METHOD_H):
    """gen_layer [1, H, S, D] with the sign of a seeded eighth of the K scales flipped: a negative
    scale counts by its magnitude, so an engine that drops the fabs ranks those rows first."""
    k8, v8, ks, vs = gen_layer(seed, (1, H, S, D), fmt)
    flip = np.random.default_rng(seed ^ 0x5CA1E).random(ks.shape) < 0.125
    return k8, v8, np.where(flip, -ks, ks).astype(np.float32), vs


def method_layers(seed, D, fmt, lens=METHOD_LENS):
    return [method_layer(seed + 17 * i, S, D, fmt) for i, S in enumerate(lens)]


def words(s):
    """float32 scales as their uint32 words."""
    return np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)


def expected_layer(pos, k8, v8, ks, vs):
    """(K rows, V rows, K scale words, V scale words) of the output rows at kept positions `pos`
    [B, H, n]; ks / vs may be None (nothing moves on that side)."""
    return (take(k8, pos), take(v8, pos),
            None if ks is None else take(words(ks), pos),
            None if vs is None else take(words(vs), pos))


ORACLE_FNS = dict({m: fn for m, (fn, _) in F.ORACLE_METHODS.items()},
                  evict_for_space=oracle.evict_for_space)
KWARGS = dict({m: kw for m, (_, kw) in F.ORACLE_METHODS.items()},
              evict_for_space=dict(num_coming=1, start_size=4, recent_size=252, skip_layers=[]))
