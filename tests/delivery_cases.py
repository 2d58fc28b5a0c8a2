"""Case generator of the delivery-path fuzz (tests/test_delivery_fuzz_gpu.py on the GPU,
tests/test_delivery_cases.py as its CPU proof).  Numpy only.

A case is one compress call whose results leave the engine through one of four delivery paths:

  inplace        dense K / V, out="inplace"
  strided        dense K / V, out=[(K_dst, V_dst) | None | "inplace", ...]
  paged_inplace  compress_paged(...): compaction into the leading pages
  paged_dense    compress_paged(..., out=[(K_dst, V_dst) | None, ...])

The generator is STRATIFIED, not drawn: the path is case % 4 and, with idx = case // 4 the case's
number on its path, the (dtype, D) combination, the method, the length stratum S0, the page size,
the K input layout and the tie policy are rotations of idx (gen() below).  The rotations that
must meet each other do not move in step: every K layout meets every S0, every width several
methods.  B, H, the layer count, the ragged lengths around S0, kwargs, key variants and the
remaining layout choices come from the case's seeded rng.  The kwargs follow
test_gpu_fuzz._kwargs with their size ranges narrowed in three cases of four (sizes below
S / 2), so that most calls change a layer.  One case in ten is long (S0 9 000 or 17 000, lengths
S0 .. 1.25 S0): its method is one of the six that select and its sizes stay below S / 8, so
that the zone keeps the length the case exists for.  What the ranges have to achieve is asserted
on the oracle alone in tests/test_delivery_cases.py.
"""
import numpy as np

import prng
import strided_layouts as SL
from oracle import oracle

N_CASES = 320
PATHS = ("inplace", "strided", "paged_inplace", "paged_dense")
METHODS = ("fix_size_l2", "l2_compress", "streaming_llm", "h2o_l2", "snapkv_lite", "pyramid_kv",
           "adaptive_l2", "recent_only")
WIDTHS = tuple((dt, D) for dt in ("bf16", "fp16", "fp32") for D in (32, 64, 80, 128, 256))
VARIANTS = ("normal", "scaled", "few", "equal", "special", "tiny")
S0S = (20, 100, 300, 700, 2000)
LONG_S0S = (9000, 17000)
PAGE_SIZES = (1, 2, 8, 16, 32, 64, 128, 1024)
STORAGES = ("nhpd", "nphd")
SPARE = 7
SELECTING_METHODS = ("fix_size_l2", "l2_compress", "h2o_l2", "snapkv_lite", "pyramid_kv",
                     "adaptive_l2")
# input layouts out="inplace" accepts (the engine takes them as they are); fused_qkv: K and V both
INPLACE_LAYOUTS = ("static", "bshd", "head_slice", "batch_slice", "fused_qkv")
COPIED_LAYOUTS = ("expand", "row_pad", "row_off")  # the engine copies these first (16-bit D64)
DST_LAYOUTS = ("static", "bshd")
DST_EXTRA = 5      # a destination holds n + 5 rows
DST_PAD = SL.STATIC_PAD
DST_START = {"static": SL.STATIC_START, "bshd": 7}
ESZ = {"bf16": 2, "fp16": 2, "fp32": 4}


def nc_of(dtype, D):
    """16-byte chunks per row: the copy / score kernels' NC."""
    return D * ESZ[dtype] // 16


def dest_pass_rows(nc):
    """csrc/kvc_gather_dest.h dest_pass_rows: output rows of one copy pass."""
    return 1024 // nc


def _kwargs(rng, method, S, narrow):
    """test_gpu_fuzz._kwargs; narrow = 1: every size below S / 2 (S / 4 where two sizes add
    up); narrow = 2 (the long cases): below S / 8 (S / 16)."""
    r = lambda lo, hi: int(rng.integers(lo, max(lo, hi) + 1))  # noqa: E731
    if narrow == 2:
        S, narrow = S // 4, 1
    top = S // 2 if narrow else S
    if method == "fix_size_l2":
        return dict(fix_kv_size=r(1, top), keep_ratio=float(rng.choice([0.0, 0.25, 0.5, 0.9])),
                    strategy=str(rng.choice(["keep_low", "keep_high"])))
    if method == "l2_compress":
        return dict(keep_ratio=float(rng.choice([0.1, 0.5, 0.8, 0.95])),
                    prune_after=r(0, S // 2 if narrow else S))
    if method == "streaming_llm":
        return dict(start_size=r(0, 8), recent_size=r(0, top))
    if method == "h2o_l2":
        return dict(start_size=r(0, 8), heavy_hitter_size=r(1, min(200, S // 4) if narrow else 200),
                    recent_size=r(0, S // 4 if narrow else S // 2))
    if method == "snapkv_lite":
        return dict(observation_window=r(0, min(64, S // 4) if narrow else 64), keep_size=r(1, top),
                    pooling_kernel=int(rng.choice([1, 2, 3, 5, 7])))
    if method == "pyramid_kv":
        return dict(base_size=r(8, top), layer_decay=float(rng.choice([0.5, 0.9, 1.0])),
                    min_size=r(1, min(64, S // 4) if narrow else 64),
                    profile=str(rng.choice(["exponential", "linear", "constant"])))
    if method == "adaptive_l2":
        soft = r(2, top)
        return dict(target_size=r(1, top), soft_limit=soft,
                    hard_limit=r(soft + 1, S if narrow else 2 * S))
    return dict(window_size=r(1, top))  # recent_only


def _table(rng, B, S, P, wide):
    """(int64 table [B, ceil(S / P)] of distinct page ids, pool size, device table columns): a
    seeded permutation; with more than one page per sequence no table is left all
    ascending-consecutive (an engine that ignored the table would read the same rows)."""
    npp = -(-S // P)
    n_pages = B * npp + SPARE
    tab = rng.permutation(n_pages)[:B * npp].reshape(B, npp).astype(np.int64)
    if npp > 1 and all((np.diff(row) == 1).all() for row in tab):
        tab[0, [0, 1]] = tab[0, [1, 0]]
    return tab, n_pages, npp + (3 if wide else 0)


def values(c, li, shape):
    """V of layer li of case `c` (tagged with its positions on the two in-place paths; else prng
    values, every third layer holding every NaN pattern of the dtype: torch.gather's rewrite)."""
    if c["path"] in ("inplace", "paged_inplace"):
        return prng.encode_positions(shape, c["dtype"])
    v = prng.gen_values(200000 + 100 * c["case"] + li, shape, c["dtype"],
                        "patterns" if c["v_patterns"][li] else "normal")
    return SL.expand_input(v) if c["v_layout"] == "expand" else v


def gen(case, tagged=False):
    """The case as a dict (numpy layers included).  Deterministic in `case` alone.  tagged: V
    position-tagged on every path (what the CPU survey reads row maps off; values() gives the
    case's own V)."""
    path = PATHS[case % 4]
    idx = case // 4
    rng = np.random.default_rng(77000 + case)
    dtype, D = WIDTHS[(idx + idx // 15) % 15]
    method = METHODS[(idx + 3 * (idx // 15)) % 8]  # a width's cases: consecutive methods
    long = idx % 10 == 3
    tie = "stable" if idx % 8 == 5 else "reference"
    inplace_path = path in ("inplace", "paged_inplace")
    if long:
        B, H = 1, int(rng.integers(1, 3))
        n_layers = int(rng.integers(1, 3))
        j = idx // 10
        method = SELECTING_METHODS[j % 6]
        S0 = int(LONG_S0S[(j + j // 4) % 2])
    else:
        B, H = int(rng.integers(1, 3)), int(rng.integers(1, 5))
        n_layers = int(rng.integers(1, 5))
        S0 = int(S0S[(idx + idx // 5) % 5])
    # CPU budget (the oracle runs over every case without a GPU too): at most about 2M key
    # elements per call -- fewer layers first, then fewer heads
    while B * H * n_layers * S0 * D > 2_000_000 and n_layers > 1:
        n_layers -= 1
    while B * H * S0 * D > 2_000_000 and H > 1:
        H -= 1
    # dense input layouts
    k_layout = INPLACE_LAYOUTS[(2 * idx + idx // 5) % 5]  # meets every S0 stratum
    v_layout = "fused_qkv" if k_layout == "fused_qkv" else str(rng.choice(INPLACE_LAYOUTS[:4]))
    if path == "strided" and D == 64 and dtype != "fp32":
        pick = int(rng.integers(0, 3))  # one side (or both) of a layout the engine copies first
        copied = [str(x) for x in rng.choice(COPIED_LAYOUTS[B == 1:], size=2)]  # expand: B > 1
        if k_layout == "fused_qkv":
            k_layout = v_layout = "static"
        if pick in (0, 2):
            k_layout = copied[0]
        if pick in (1, 2):
            v_layout = copied[1]
    layers = []
    v_patterns = [(idx + li) % 3 == 0 for li in range(n_layers)]
    for li in range(n_layers):
        S = max(1, S0 + int(rng.integers(0 if long else -S0 // 4, S0 // 4 + 1)))
        shape = (B, H, S, D)
        seed = 200000 + 100 * case + li
        k = prng.gen_keys(seed, shape, dtype, str(rng.choice(VARIANTS)))
        if path == "strided" and k_layout == "expand":
            k = SL.expand_input(k)
        layers.append((k, None))
    kw = _kwargs(rng, method, S0, narrow=2 if long else int(bool(rng.integers(0, 4))))
    n_skip = int(rng.integers(0, 2)) if not (long and n_layers == 1) else 0
    kw["skip_layers"] = [int(x) for x in rng.choice(n_layers, size=n_skip, replace=False)]
    c = dict(case=case, path=path, idx=idx, method=method, kw=kw, dtype=dtype, D=D,
             nc=nc_of(dtype, D), tie=tie, long=long, S0=S0, layers=layers, k_layout=k_layout,
             v_layout=v_layout if path in ("inplace", "strided") else None,
             v_patterns=[p and not inplace_path for p in v_patterns])
    # (a tagged V has four columns: all the oracle's gather of V needs to carry a row's position)
    c["layers"] = [(k, prng.encode_positions(k.shape[:3] + (4,), dtype) if tagged
                    else values(c, li, k.shape)) for li, (k, _) in enumerate(layers)]
    # destinations: K and V windows in different layouts; sometimes one layer without a pair
    if not inplace_path:
        kd = str(rng.choice(DST_LAYOUTS))
        c["dst_layouts"] = (kd, "bshd" if kd == "static" else "static")
        c["no_pair"] = None  # (layer, what its `out` entry is)
        if n_layers > 1 and rng.integers(0, 3) == 0:
            li = int(rng.integers(0, n_layers))
            # compress_paged: None = in place.  Dense: None = the default call's result,
            # "inplace" = in place -- unless the layer's layout is one the engine must copy
            entry = None
            if path == "strided" and rng.integers(0, 2) and \
                    k_layout not in COPIED_LAYOUTS and v_layout not in COPIED_LAYOUTS:
                entry = "inplace"
            c["no_pair"] = (li, entry)
    if path.startswith("paged"):
        c["P"] = P = PAGE_SIZES[(idx + idx // 8) % 8]
        c["k_storage"], c["v_storage"] = (str(rng.choice(STORAGES)) for _ in range(2))
        c["tables"] = [_table(rng, B, k.shape[2], P, bool(rng.integers(0, 2))) for k, _ in layers]
    return c


def inplace_layers(c):
    """The layers of case `c` whose result is compacted in place."""
    n = len(c["layers"])
    if c["path"] in ("inplace", "paged_inplace"):
        return list(range(n))
    if c["no_pair"] is None:
        return []
    li, entry = c["no_pair"]
    return [li] if c["path"] == "paged_dense" or entry == "inplace" else []


def _run(c, layers):
    prev = oracle.TIE
    oracle.TIE = c["tie"]
    try:
        return oracle.METHODS[c["method"]](layers, **c["kw"])
    finally:
        oracle.TIE = prev


def reference(c):
    """The oracle's [(K, V, kind)] on the case's dense numpy layers under its tie policy -- or the
    exception instance the oracle raised."""
    try:
        return _run(c, c["layers"])
    except Exception as e:  # the engine must raise the same type
        return e


def row_maps(c, ref=None):
    """[src [B, H, n] | None] per layer: which input row every output row is, read off the
    oracle's V output on position-tagged V (V takes no part in any selection).  None for an
    untouched ("same") layer.  On the two in-place paths V is tagged already and `ref` serves."""
    if ref is None or c["path"] not in ("inplace", "paged_inplace"):
        ref = _run(c, tagged_layers(c))
    return decode_row_maps(ref, c["dtype"])


def tagged_layers(c):
    """The case's layers with position-tagged V."""
    return [(k, prng.encode_positions(k.shape, c["dtype"])) for k, _ in c["layers"]]


def decode_row_maps(ref, dtype):
    """row_maps() of an oracle result on position-tagged V."""
    out = []
    for rk, rv, kind in ref:
        if kind == "same":
            out.append(None)
            continue
        pos, ok = prng.decode_positions(np.asarray(rv), dtype)
        assert ok
        out.append(pos)
    return out


def selecting(src):
    """True when a row map can only come from a selection inside a zone: sink ++ zone ++ tail
    with the zone kept whole (or absent) is at most two runs of consecutive rows, the same for
    every (b, h); a map with two gaps in some row, or one that differs between rows, is not."""
    if src is None or src.shape[2] < 2:
        return False
    gaps = (np.diff(src, axis=2) != 1).sum(axis=2)
    return bool(gaps.max() >= 2 or (src != src[:1, :1]).any())


def refusable(src, S):
    """What kvc_plan_dest may refuse to compact in place: a row map that is not strictly
    increasing, or a result longer than its input."""
    return src is not None and bool(src.shape[2] > S or (np.diff(src, axis=2) <= 0).any())
