"""fp8 K/V caches: formats, inputs and CPU expectations of the test_fp8_* suites.

The contract (include/kvc.h, enum kvc_dtype): an fp8 call keeps the
positions the engine's bf16 semantics keep on K.to(bfloat16) -- an exact upcast -- and copies the
kept rows' BYTES of K and V.  So every expectation here is

    1. decode the fp8 bytes to bf16 bit patterns (the table below, checked against torch),
    2. run the existing oracle on (K_bf16, position-encoding V) and read the kept positions back,
    3. take the fp8 bytes of K and V at those positions,

and nothing is computed by the engine.  Numpy only; fp8 tensors are uint8 arrays of bit patterns.
"""
import numpy as np

import prng
from oracle import oracle

FORMATS = ("e4m3", "e5m2")  # OCP float8_e4m3fn / float8_e5m2
_GEOM = {"e4m3": (4, 3, 7), "e5m2": (5, 2, 15)}  # exponent bits, mantissa bits, bias
NAN_CODES = {"e4m3": (0x7F, 0xFF), "e5m2": (0x7D, 0x7E, 0x7F, 0xFD, 0xFE, 0xFF)}
INF_CODES = {"e4m3": (), "e5m2": (0x7C, 0xFC)}
MAX_CODE = {"e4m3": 0x7E, "e5m2": 0x7B}  # largest finite: 448 / 57344
POISON8 = 0xA5  # output pre-fill of the delivery tests: a finite value no generator favours


def decode_table(fmt, bias_shift=0, fnuz=False):
    """float32 value of each of the 256 bit patterns, from the format's definition.  bias_shift /
    fnuz build the WRONG decoders of the power test (the fnuz formats: bias one larger, no inf,
    0x80 the only NaN)."""
    ebits, mbits, bias = _GEOM[fmt]
    bias += bias_shift + (1 if fnuz else 0)
    out = np.empty(256, dtype=np.float32)
    for b in range(256):
        sign = -1.0 if b & 0x80 else 1.0
        e = (b >> mbits) & ((1 << ebits) - 1)
        m = b & ((1 << mbits) - 1)
        if fnuz:
            if b == 0x80:
                out[b] = np.nan
                continue
        elif fmt == "e4m3" and (b & 0x7F) == 0x7F:
            out[b] = np.nan
            continue
        elif fmt == "e5m2" and e == 31:
            out[b] = np.nan if m else sign * np.inf
            continue
        if e == 0:
            out[b] = sign * m * 2.0 ** (1 - bias - mbits)
        else:
            out[b] = sign * (1.0 + m * 2.0 ** -mbits) * 2.0 ** (e - bias)
    return out


_F32 = {f: decode_table(f) for f in FORMATS}


def to_f32(a8, fmt):
    return _F32[fmt][np.asarray(a8, dtype=np.uint8)]


def bf16_table(fmt):
    """bf16 bit pattern of each fp8 pattern: the upper half of its float32 (exact: at most 3
    mantissa bits, exponents inside bf16's), NaNs as torch's conversion leaves them."""
    bits = _F32[fmt].view(np.uint32)
    assert not (bits & 0xFFFF).any()
    return (bits >> 16).astype(np.uint16)


_BF16 = {f: bf16_table(f) for f in FORMATS}


def to_bf16_bits(a8, fmt):
    """uint8 fp8 patterns -> uint16 bf16 bit patterns of K.to(torch.bfloat16)."""
    return _BF16[fmt][np.asarray(a8, dtype=np.uint8)]


def quantize(x, fmt):
    """float32 -> fp8 bit patterns by round-to-nearest-even written out: the nearest finite value of
    the format, a tie to the even code, magnitudes beyond the largest finite value saturated to it
    (e5m2: +-inf stays inf), NaN to the canonical NaN.  Host-independent: comparisons of exactly
    representable numbers only."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    grid = _F32[fmt][:MAX_CODE[fmt] + 1].astype(np.float64)  # codes 0 .. max finite, ascending
    a = np.abs(x).astype(np.float64)
    hi = np.clip(np.searchsorted(grid, a, side="left"), 1, len(grid) - 1)
    lo = hi - 1
    dlo, dhi = a - grid[lo], grid[hi] - a
    code = np.where(dlo < dhi, lo, np.where(dhi < dlo, hi, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(a >= grid[-1], len(grid) - 1, code).astype(np.uint8)
    if fmt == "e5m2":
        code = np.where(np.isinf(x), 0x7C, code).astype(np.uint8)
    code = np.where(np.isnan(x), 0x7F if fmt == "e4m3" else 0x7E, code).astype(np.uint8)
    return (code | np.where(np.signbit(x), 0x80, 0).astype(np.uint8)).astype(np.uint8)


def gen_keys(seed, shape, fmt, variant="normal"):
    """prng.gen_keys' float32 recipe of `variant`, quantised.  "special" carries NaN rows, zero
    rows and -- e5m2 -- inf rows (e4m3 has no inf: those rows saturate to +-448)."""
    return quantize(prng.gen_keys(seed, shape, "fp32", variant), fmt)


def order_rows(D, fmt):
    """(C, R): two rows [D] of fp8 patterns with norms next to the bf16 rounding boundary 257.
    R is 256 and zeros: norm 256 in any summation order.  C starts with 256, carries mid-sized
    elements that bring the sum of squares just BELOW 257^2 = 2^16 + 2^9 + 1, and is filled with
    2^-5: squares of 2^-10, an eighth of an fp32 ulp at 2^16.  One accumulator in element order
    (fp16's torch.norm) loses every one of them behind the leading 2^16 and rounds the norm down
    to 256; torch.norm's eight lanes on bf16 sum them apart from it in lanes 1..7, cross the
    boundary and give 258.  (An fp8 square has at most 8 significant bits, so sums of ordinary
    rows are exact in fp32 in any order: only rows like C can tell the orders apart.)"""
    mid = [16.0, 16.0, 0.75, 0.5, 0.25, 0.25] + ([0.125, 0.125] if D < 128 else [])
    c = np.full(D, 2.0 ** -5, dtype=np.float32)
    c[0] = 256.0
    c[1:1 + len(mid)] = mid
    r = np.zeros(D, dtype=np.float32)
    r[0] = 256.0
    C, R = quantize(c, fmt), quantize(r, fmt)
    assert np.array_equal(to_f32(C, fmt), c) and np.array_equal(to_f32(R, fmt), r)
    return C, R


ORDER_ROWS = 10  # rows of each kind that the "order" variant plants


def gen_keys_order(seed, shape, fmt):
    """"normal" keys with ORDER_ROWS C rows and as many R rows (order_rows) interleaved at seeded
    positions of every (b, h): keeping all but the ORDER_ROWS largest norms drops exactly the C
    rows (258 > 256) -- and a tie group of 2 * ORDER_ROWS rows at 256 under a wrong order."""
    B, H, S, D = shape
    k = gen_keys(seed, shape, fmt, "normal")
    C, R = order_rows(D, fmt)
    for r in range(B * H):
        at = np.random.default_rng(seed + r).permutation(S)[:2 * ORDER_ROWS]
        k.reshape(B * H, S, D)[r, at[0::2]] = C
        k.reshape(B * H, S, D)[r, at[1::2]] = R
    return k


# ---- the inputs of the SCORE test (tests/test_fp8_score_gpu.py; their power: test_fp8_cpu.py) ----
SCORE_B, SCORE_H = 16, 2
SCORE_ZONE_START, SCORE_ZONE_LEN = 5, 257
SCORE_S = SCORE_ZONE_START + SCORE_ZONE_LEN + 3
SCORE_LANES = 16  # byte lanes of a 16-byte chunk = the first 16 (b, h) rows


def score_keys(fmt, D):
    """Keys [16, 2, S, D] whose zone [5, 262) holds, at token t < 256 of (b, h) row r,
      r < 16   bit pattern t at every element d with d % 16 == r and ZERO elsewhere: the pattern
               alone at byte lane r of every chunk, norm |x| * sqrt(D / 16) -- which bf16 tells
               apart for every magnitude of the format, so any wrong decode of any pattern at any
               lane shows (a sign cannot: the norm squares it; NaN and inf show as such);
      r >= 16  the same pattern at lane r - 16 over quantised normal values: the decode inside
               torch.norm's accumulator order with every lane busy.
    Token 256 -- the 1-token tile -- holds the further rows: all +0, all -0, all largest / smallest
    subnormal, all +-max, the summation-order probes of order_rows, one NaN, one +-inf (e5m2)."""
    B, H, S = SCORE_B, SCORE_H, SCORE_S
    k = gen_keys(61000 + D, (B, H, S, D), fmt, "normal")
    assert not np.isin(k, NAN_CODES[fmt] + INF_CODES[fmt]).any()
    z = k[:, :, SCORE_ZONE_START:SCORE_ZONE_START + SCORE_ZONE_LEN].reshape(B * H, SCORE_ZONE_LEN, D)
    z[:SCORE_LANES, :256] = 0
    for r in range(B * H):
        z[r, :256, r % SCORE_LANES::16] = np.arange(256, dtype=np.uint8)[:, None]
    C, R = order_rows(D, fmt)
    sub = 0x07 if fmt == "e4m3" else 0x03  # the largest subnormal
    last = [np.zeros(D, np.uint8), np.full(D, 0x80, np.uint8), np.full(D, sub, np.uint8),
            np.full(D, 0x01, np.uint8), np.full(D, MAX_CODE[fmt], np.uint8),
            np.full(D, MAX_CODE[fmt] | 0x80, np.uint8), C, R]
    one_nan = k[0, 0, 0].copy()
    one_nan[D - 1] = NAN_CODES[fmt][0]
    last.append(one_nan)
    for code in INF_CODES[fmt]:
        one_inf = k[0, 0, 1].copy()
        one_inf[7] = code
        last.append(one_inf)
    for r, row in enumerate(last):
        z[r, 256] = row
    k[:, :, SCORE_ZONE_START:SCORE_ZONE_START + SCORE_ZONE_LEN] = z.reshape(B, H, SCORE_ZONE_LEN, D)
    return k


def score_zone(k8):
    return k8[:, :, SCORE_ZONE_START:SCORE_ZONE_START + SCORE_ZONE_LEN]


def gen_values(seed, shape, fmt):
    return quantize(prng.gen_values(seed, shape, "fp32"), fmt)


def torch_dtype(fmt):
    import torch
    return {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}[fmt]


def to_dev(a8, fmt, device="cuda:0"):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a8)).view(torch_dtype(fmt)).to(device)


def to_np(t):
    import torch
    return t.detach().contiguous().view(torch.uint8).cpu().numpy()


# ----------------------------------------------------------------------------------------------
# expectations
# ----------------------------------------------------------------------------------------------
def kept_positions(oracle_fn, keys8, fmt, **kwargs):
    """Per layer the source position of every output row [B, H, n_out], as gen_goldens.py recovers
    them: the oracle method on (K upcast to bf16, V encoding its own positions).  S <= 65 536."""
    layers = [(to_bf16_bits(k, fmt), prng.encode_positions(k.shape, "bf16")) for k in keys8]
    out = []
    for (_, v, _) in oracle_fn(layers, **kwargs):
        pos, ok = prng.decode_positions(v, "bf16")
        assert ok
        out.append(pos)
    return out


def take_rows(x8, pos):
    """x8[b, h, pos[b, h, t], :] -- the bytes of the kept rows."""
    return np.take_along_axis(x8, pos[..., None].astype(np.int64), axis=2)


def expected(oracle_fn, layers8, fmt, **kwargs):
    """[(K_out, V_out)] uint8 of the method on fp8 layers [(K, V)]."""
    pos = kept_positions(oracle_fn, [k for k, _ in layers8], fmt, **kwargs)
    return [(take_rows(k, p), take_rows(v, p)) for (k, v), p in zip(layers8, pos)]


def expected_spec(k8, v8, s, order, algo, fmt):
    """phase_tables.expected_layer for one fp8 layer spec (zones of any length): indices on the
    upcast keys, bytes copied verbatim (no gather NaN rewrite)."""
    import phase_tables as PT
    idx = PT.expected_indices(to_bf16_bits(k8, fmt), s, order, algo)

    def out(x):
        parts = [x[:, :, :s["sink"]]]
        if s["n_select"]:
            zone = x[:, :, s["zone_start"]:s["zone_start"] + s["zone_len"]]
            parts.append(take_rows(zone, idx))
        parts.append(x[:, :, s["tail_start"]:s["tail_start"] + s["tail_len"]])
        return np.concatenate(parts, axis=2)
    return out(k8), out(v8), idx


def norms_bf16(k8, fmt):
    """oracle.norms on the upcast keys: [B, H, Z] bf16 bit patterns."""
    return oracle.norms(to_bf16_bits(k8, fmt))


ORACLE_METHODS = {
    "l2_compress": (oracle.l2_compress, dict(keep_ratio=0.8, prune_after=100, skip_layers=[])),
    "fix_size_l2": (oracle.fix_size_l2_compress,
                    dict(fix_kv_size=256, keep_ratio=0.5, strategy="keep_low", skip_layers=[])),
    "streaming_llm": (oracle.streaming_llm_compress, dict(start_size=4, recent_size=252)),
    "recent_only": (oracle.recent_only_compress, dict(window_size=256, skip_layers=[])),
    "h2o_l2": (oracle.h2o_l2_compress,
               dict(start_size=4, heavy_hitter_size=64, recent_size=188, skip_layers=[])),
    "snapkv_lite": (oracle.snapkv_lite_compress,
                    dict(observation_window=32, keep_size=256, pooling_kernel=5, skip_layers=[])),
    "pyramid_kv": (oracle.pyramid_kv_compress,
                   dict(base_size=256, layer_decay=0.9, skip_layers=[])),
    "adaptive_l2": (oracle.adaptive_l2_compress, dict(target_size=256, skip_layers=[])),
}
METHODS = tuple(ORACLE_METHODS)  # the eight methods of the README, in registry order
