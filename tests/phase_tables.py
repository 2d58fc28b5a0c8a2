"""Layer tables, inputs and CPU expectations of the C-ABI phase-contract tests
(tests/test_phase_contract.py on the GPU, tests/test_phase_tables.py as their CPU proof).

include/kvc.h describes SCORE, SELECT and GATHER as phases that talk through the workspace.  The
tables below are built to be launched phase by phase on a workspace filled with 0xFF, and their
expected outputs come from the oracle's primitives alone -- norms, argsort_prefix / topk_indices
/ stable_prefix, snapkv_scores, gather (on the selected segment only: its NaN rewrite) and cat --
never from the engine.  Numpy only: nothing here needs a GPU.

Representation as in oracle/oracle.py: bf16 arrays are uint16 bit patterns.
"""
import numpy as np

import prng
from oracle import oracle

ASC, DESC = 0, 1
SORT, TOPK, STABLE = 0, 1, 2
NORM, SNAPKV = 0, 1

POISON = 0xFF  # every workspace byte before the first launch: a NaN as bf16 / fp16 / fp32, -1 as int32
# output pre-fill, as the integer of one element: signalling NaNs with a payload that neither the
# generators (0x7FC0 / 0x7E00 / 0x7FC00000) nor torch.gather's NaN rewrite (0xFFFF, bit 9 set)
# produce, so a surviving element cannot be mistaken for data
SENTINEL = {"bf16": 0x7FA5, "fp16": 0x7DA5, "fp32": 0x7FA5A5A5}
BITS = {"bf16": np.uint16, "fp16": np.uint16, "fp32": np.uint32}

# the selection kernel kvc_launch dispatches for a call whose longest selecting zone is n
# (csrc/kvc.hip launch_select; csrc/kvc_device_util.h kSmallZone 8 192, kZoneMax 16 384,
# kZoneMaxGlobal 65 536)
KERNEL_EDGES = ((8192, "512-thread LDS"), (16384, "1024-thread LDS"),
                (65536, "global scratch, u16 positions"), (1 << 24, "global scratch, u32 positions"))


def kernel_for(zone_len):
    n_cap = zone_len + (-zone_len % 64)
    for edge, name in KERNEL_EDGES:
        if n_cap <= edge:
            return name
    raise ValueError(zone_len)


def spec(S, zone_start=0, zone_len=0, n_select=0, sink=0, tail_start=0, tail_len=0,
         score_mode=NORM, pool=0, variant="normal", seed=0):
    assert 0 <= zone_start and zone_start + zone_len <= S and 0 <= n_select <= zone_len
    assert sink <= S and tail_start + tail_len <= S
    return dict(S=S, zone_start=zone_start, zone_len=zone_len, n_select=n_select, sink=sink,
                tail_start=tail_start, tail_len=tail_len, score_mode=score_mode, pool=pool,
                variant=variant, seed=seed)


def n_out(s):
    return s["sink"] + s["n_select"] + s["tail_len"]


# ----------------------------------------------------------------------------------------------
# expectations
# ----------------------------------------------------------------------------------------------
def expected_indices(K, s, order, algo):
    """Ascending zone-local indices [B, H, n_select] of layer spec `s` on keys K [B, H, S, D]."""
    B, H = K.shape[:2]
    n, k = s["zone_len"], s["n_select"]
    if k == 0:
        return np.zeros((B, H, 0), dtype=np.int64)
    if k == n:  # nothing to decide: every zone position, in order
        return np.broadcast_to(np.arange(n, dtype=np.int64), (B, H, n)).copy()
    nrm = oracle.norms(K[:, :, s["zone_start"]:s["zone_start"] + n])
    if s["score_mode"] == SNAPKV:  # snapkv_lite.py:99-121
        pool = s["pool"]
        nrm = oracle.snapkv_scores(nrm, pool if pool > 1 and n >= pool else 0)
    return np.sort(select(nrm, k, order, algo), axis=-1)


def select(vals, k, order, algo):
    """The kept positions (in sort order) of kvc_order / kvc_algo on score rows [B, H, n]."""
    if algo == STABLE:
        return oracle.stable_prefix(vals, k, descending=order == DESC)
    if algo == TOPK:
        assert order == DESC  # torch.topk(largest=True): the only topk the methods issue
        return oracle.topk_indices(vals, k)
    return oracle.argsort_prefix(vals, k, descending=order == DESC)


def expected_output(X, s, idx):
    """sink ++ zone[idx] ++ tail of X [B, H, S, D] (K or V); the selected segment goes through
    oracle.gather (torch.gather's NaN rewrite), the other two are plain copies."""
    parts = [X[:, :, :s["sink"]]]
    if s["n_select"]:
        zone = X[:, :, s["zone_start"]:s["zone_start"] + s["zone_len"]]
        parts.append(oracle.gather(zone, idx))
    parts.append(X[:, :, s["tail_start"]:s["tail_start"] + s["tail_len"]])
    return oracle.cat(parts)


def expected_layer(K, V, s, order, algo):
    idx = expected_indices(K, s, order, algo)
    return expected_output(K, s, idx), expected_output(V, s, idx), idx


def gen_keys(s, B, H, D, dtype):
    shape = (B, H, s["S"], D)
    if s["variant"] == "special+scaled":  # batch 0 "special", the other batches "scaled"
        K = prng.gen_keys(s["seed"], shape, dtype, "special")
        K[1:] = prng.gen_keys(s["seed"], shape, dtype, "scaled")[1:]
        return K
    return prng.gen_keys(s["seed"], shape, dtype, s["variant"])


def gen_layers(specs, B, H, D, dtype):
    return [(gen_keys(s, B, H, D, dtype), prng.gen_values(s["seed"], (B, H, s["S"], D), dtype))
            for s in specs]


# ----------------------------------------------------------------------------------------------
# item 1: four ragged layers, the longest zone at a selection kernel's first length
# ----------------------------------------------------------------------------------------------
SPLIT_ZONES = (1000, 8256, 16448, 65600)


def split_geometry(Z):
    """(B, H) of the four-layer call whose longest zone is Z."""
    return (2, 2) if Z <= 8256 else (1, 2)


def split_table(Z, score_mode=NORM, pool=0):
    """Layer 0 selects from the longest zone (tie-heavy keys); layer 1 only copies (n_select 0,
    sink 3, tail 5); layer 2 keeps its whole zone; layer 3 selects few rows (the heap-select side
    of topk's k * 64 <= n) from a shorter zone whose keys carry NaN / inf / zero rows, its tail
    apart from the zone.  No zone but the longest is a multiple of 64.  In a snapkv table only
    batch 0 of layer 3 keeps those keys and batch 1 gets spread norms ("scaled"): one NaN norm
    makes every snapkv score of its row NaN (the row maximum is NaN), which alone would leave
    that layer nothing to tell a wrong scoring by."""
    z3 = Z // 2 + 37
    v3 = "special" if score_mode == NORM else "special+scaled"
    return [
        spec(Z + 11, zone_start=4, zone_len=Z, n_select=Z // 3, sink=4, tail_start=Z + 4,
             tail_len=7, score_mode=score_mode, pool=pool, variant="few", seed=7100 + Z),
        spec(300, zone_start=3, zone_len=292, n_select=0, sink=3, tail_start=295, tail_len=5,
             variant="normal", seed=7200 + Z),
        spec(140, zone_start=2, zone_len=130, n_select=130, sink=2, tail_start=137, tail_len=3,
             variant="normal", seed=7300 + Z),
        spec(z3 + 30, zone_start=1, zone_len=z3, n_select=max(1, z3 // 80), sink=1,
             tail_start=z3 + 21, tail_len=9, score_mode=score_mode, pool=pool, variant=v3,
             seed=7400 + Z),
    ]


def split_cases():
    """(Z, dtype, order, algo) in an order that keeps one (Z, dtype)'s cases together."""
    out = []
    for Z in SPLIT_ZONES:
        for dt in ("bf16", "fp32") + (("fp16",) if Z == SPLIT_ZONES[0] else ()):
            modes = [(ASC, SORT), (DESC, SORT), (DESC, TOPK)]
            if Z in (1000, 16448):  # KVC_ALGO_STABLE: zones of at most 65 536 positions
                modes += [(ASC, STABLE), (DESC, STABLE)]
            out += [(Z, dt, o, a) for o, a in modes]
    return out


def snapkv_cases():
    return [(Z, dt, pool) for Z in (1000, 8256) for dt in ("bf16", "fp16") for pool in (1, 5)]


# ----------------------------------------------------------------------------------------------
# item 2: more layers than one argument chunk (kArgLayers = 64)
# ----------------------------------------------------------------------------------------------
def chunk_table(n_layers):
    """[1, 1, S_i, 64] layers, S_i cycling through 70, 130, 200 (zones of 67, 127 and 197
    positions: two, two and four SCORE tiles, the last one partial), so the second and third
    chunks start at tile 170 and 340, workspace rows 64 and 128."""
    out = []
    for i in range(n_layers):
        S = (70, 130, 200)[i % 3]
        zl = S - 3
        out.append(spec(S, zone_start=1, zone_len=zl, n_select=zl // 3 + i % 5, sink=1,
                        tail_start=S - 2, tail_len=2, variant=("few", "normal")[i % 2],
                        seed=7600 + i))
    return out


# ----------------------------------------------------------------------------------------------
# item 3: SELECT from a norm region the caller wrote
# ----------------------------------------------------------------------------------------------
NORM_ZONES = (1, 2, 63, 64, 65, 8191, 8192, 8193, 16383, 16384, 16385, 65535, 65536, 65537)
NORM_MODES = ((ASC, SORT), (DESC, TOPK))
# the two rows (heads) of one input: what a norm can be
NORM_PAIRS = (("finite", "ties8"), ("inf", "nan"), ("subnormal", "equal"))
PADS = ("poison", "zero", "inf")


def norm_selects(n):
    """n_select in {1, n // 64, n // 2, n - 1} where something is left to decide: both sides of
    torch.topk's k * 64 <= n (heap select | introselect)."""
    return sorted(k for k in {1, n // 64, n // 2, n - 1} if 0 < k < n)


def _norm_row(kind, n, seed):
    """n values a key norm can take, float32 (exactly representable in `dtype`)."""
    u = prng.uniform(seed, n).astype(np.float32)
    few = sorted({n // 5, n // 2, n - 1})  # a handful of special values, never most of a row
    if kind == "finite":
        x = np.float32(0.25) + u * np.float32(12.0)
    elif kind == "ties8":
        x = (1.0 + (prng.splitmix64(seed ^ 0x52, n) % np.uint64(8)).astype(np.float32)) * 0.5
    elif kind == "inf":
        x = u * np.float32(12.0)
        x[few] = np.inf
    elif kind == "nan":
        x = u * np.float32(12.0)
        x[few] = np.nan
    elif kind == "subnormal":  # below the smallest normal of bf16 / fp32 (2^-126)
        x = (1.0 + np.floor(u * 100.0)).astype(np.float32) * np.float32(2.0 ** -133)
    elif kind == "equal":
        x = np.full(n, 3.25, dtype=np.float32)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def norm_rows(n, dtype, pair):
    """[1, 2, n] norm values of input (n, dtype, pair) in storage representation."""
    rows = [_norm_row(kind, n, 8100 + 31 * n + 7 * pair + h)
            for h, kind in enumerate(NORM_PAIRS[pair])]
    return prng.to_dtype(np.stack(rows).reshape(-1), dtype).reshape(1, 2, n)


def pad_value(pad, dtype):
    """One padding element, in storage representation."""
    if pad == "poison":  # 0xFF bytes read as the key type: a NaN
        return np.uint16(0xFFFF) if dtype == "bf16" else np.frombuffer(b"\xff" * 4, np.float32)[0]
    return prng.to_dtype(np.array([0.0 if pad == "zero" else np.inf], dtype=np.float32), dtype)[0]


def norm_inputs():
    """Every item-3 input (n, dtype, pair, k, order, algo)."""
    return [(n, dt, pair, k, o, a) for n in NORM_ZONES for dt in ("bf16", "fp32")
            for pair in range(len(NORM_PAIRS)) for k in norm_selects(n) for o, a in NORM_MODES]


def padding_matters(inp, rows=None):
    """True when, for both rows of the input, selecting over the row with ONE padding column
    included gives another index set than over the row alone for at least one of the padding
    values -- so a kernel that let the padding take part could not pass on all three."""
    n, dt, pair, k, o, a = inp
    vals = norm_rows(n, dt, pair) if rows is None else rows
    want = np.sort(select(vals, k, o, a), axis=-1)
    differs = np.zeros(2, dtype=bool)
    for pad in PADS:
        ext = np.concatenate([vals, np.full((1, 2, 1), pad_value(pad, dt), dtype=vals.dtype)], axis=2)
        got = np.sort(select(ext, k, o, a), axis=-1)
        differs |= (got != want).any(axis=-1)[0]
    return bool(differs.all())


# Inputs for which padding_matters() is False (tests/test_phase_tables.py recomputes the list and
# holds it to 10 % of the inputs whose zone is no multiple of 64); the GPU test leaves them out.
# They are the "nan" row's largest single value (k = 1, DESC + TOPK): its NaN already is the
# maximum, and a NaN or +inf behind the row only ties with it.  (Zero norms, which tie with a zero
# padding in the same way, take part in item 1's "special" keys instead.)
NORM_DROPPED = frozenset((n, dt, 1, 1, DESC, TOPK) for dt in ("bf16", "fp32")
                         for n in (2, 65, 8191, 8193, 16383, 16385, 65535, 65537))


def norm_cases():
    return [i for i in norm_inputs() if i not in NORM_DROPPED]
