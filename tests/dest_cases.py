"""Case tables of the destination tests (tests/test_dest_gpu.py on the GPU, tests/test_dest_order.py
as their CPU proof).  Numpy only.

Every in-place case is a call whose compressed layers are compacted at the front of their own
memory.  Its V rows carry their own position (prng.encode_positions: (s // 256, s % 256), exact
in bf16 / fp16 / fp32) -- V takes no part in any selection, so the row map src(t) of a layer can
be read off the oracle's V output, which is what the ordering proof needs.  Shapes: the smallest
whose outputs are several passes long for any plausible pass size (a pass of the copy kernel is
1024 16-byte units of K and V: 32 to 256 rows).
"""
import numpy as np

import prng
from oracle import oracle

B, H = 2, 3


def _case(id, method, kw, S, D, dtype, layers=1, variant="few", seed=0, bh=(B, H), repeat=1,
          tie="reference"):
    return dict(id=id, method=method, kw=kw, dtype=dtype, variant=variant, seed=seed,
                shapes=[bh + (S, D)] * layers if isinstance(S, int) else [bh + (s, D) for s in S],
                repeat=repeat, tie=tie)


INPLACE = [
    # 1 / 2: shift-by-one (by three) memmove across pass boundaries
    _case("streaming_llm-shift1", "streaming_llm",
          dict(start_size=4, recent_size=2300, skip_layers=[]), 2305, 64, "bf16", seed=41000,
          repeat=3),
    _case("evict_for_space-shift3", "evict_for_space",
          dict(num_coming=3, start_size=4, recent_size=2301, skip_layers=[]), 2305, 64, "bf16",
          seed=41010),
    # 3: dense small shifts, 160-byte rows
    _case("l2_compress-kr0.9-fp16-D80", "l2_compress", dict(keep_ratio=0.9, skip_layers=()),
          2500, 80, "fp16", seed=41020, repeat=3),
    # 4: zone + tail, 512-byte rows
    _case("fix_size_l2-512-kr0.5-fp32-D128", "fix_size_l2",
          dict(fix_kv_size=512, keep_ratio=0.5, skip_layers=[]), 3000, 128, "fp32", seed=41030,
          repeat=3),
    # 5: sink + zone + tail, 64-byte rows
    _case("h2o_l2-4-64-444-D32", "h2o_l2",
          dict(start_size=4, heavy_hitter_size=64, recent_size=444, skip_layers=[]), 1200, 32,
          "bf16", seed=41040),
    # 6: topk rows; the snapkv SELECT after SCORE on one workspace
    _case("snapkv_lite-32-512-5", "snapkv_lite",
          dict(observation_window=32, keep_size=512, pooling_kernel=5, skip_layers=[]), 1500, 64,
          "bf16", seed=41050, variant="normal"),
    # 7: n_out differs per layer
    _case("pyramid_kv-512-6layers", "pyramid_kv", dict(base_size=512, skip_layers=[]), 1500, 128,
          "bf16", layers=6, seed=41060, repeat=3),
    # 8: both branches of adaptive_l2
    _case("adaptive_l2-hard", "adaptive_l2", dict(skip_layers=[]), 1500, 64, "bf16", seed=41070),
    _case("adaptive_l2-gradual", "adaptive_l2", dict(hard_limit=2048, skip_layers=[]), 1500, 64,
          "bf16", seed=41080, variant="special"),
    # 10: results that are slices of the input, moved to the front
    _case("recent_only-512", "recent_only", dict(window_size=512, skip_layers=[]), 1500, 64,
          "bf16", seed=41100),
    _case("snapkv_lite-window-only", "snapkv_lite",
          dict(observation_window=512, keep_size=512, skip_layers=[]), 1500, 64, "bf16",
          seed=41110),
    # 11: global-scratch select, long rows
    _case("fix_size_l2-512-S17000", "fix_size_l2",
          dict(fix_kv_size=512, keep_ratio=0.0, skip_layers=[]), 17000, 32, "bf16", seed=41120,
          bh=(1, 2), variant="normal"),  # kept rows all over the sequence, some below row 512
    _case("l2_compress-kr0.95-S17000", "l2_compress", dict(keep_ratio=0.95, skip_layers=()),
          17000, 32, "bf16", seed=41130, bh=(1, 2)),
    # 12: case 4 on tie-heavy bf16 keys under the stable tie policy
    _case("fix_size_l2-512-kr0.5-stable", "fix_size_l2",
          dict(fix_kv_size=512, keep_ratio=0.5, skip_layers=[]), 3000, 128, "bf16", seed=41140,
          tie="stable"),
    # 14: untouched layers (a skipped one, one below the threshold) stay the same objects
    _case("fix_size_l2-skip0-and-short", "fix_size_l2",
          dict(fix_kv_size=512, keep_ratio=0.25, skip_layers=[0]), (1500, 1400, 300, 1500), 64,
          "bf16", seed=41150),
]

# the strided-destination cases: 3, 4, 7, 11 and 14
STRIDED = [c for c in INPLACE if c["id"] in (
    "l2_compress-kr0.9-fp16-D80", "fix_size_l2-512-kr0.5-fp32-D128", "pyramid_kv-512-6layers",
    "fix_size_l2-512-S17000", "l2_compress-kr0.95-S17000", "fix_size_l2-skip0-and-short")]


def inputs(case, tagged=True, fill=0):
    """[(K, V)] numpy layers of a case; `fill` varies the keys between repeated runs.  tagged: V
    rows carry their position (the in-place cases), else prng values."""
    layers = []
    for li, shape in enumerate(case["shapes"]):
        seed = case["seed"] + li + 100 * fill
        k = prng.gen_keys(seed, shape, case["dtype"], case["variant"])
        v = (prng.encode_positions(shape, case["dtype"]) if tagged
             else prng.gen_values(seed, shape, case["dtype"]))
        layers.append((k, v))
    return layers


_REF = {}


def reference(case, tagged=True, fill=0):
    """(numpy layers, oracle result) of a case, computed once and never modified."""
    key = (case["id"], tagged, fill)
    if key not in _REF:
        layers = inputs(case, tagged, fill)
        prev = oracle.TIE
        oracle.TIE = case["tie"]
        try:
            _REF[key] = (layers, oracle.METHODS[case["method"]](layers, **case["kw"]))
        finally:
            oracle.TIE = prev
    return _REF[key]


def row_map(case, v_out):
    """src(t) [B, H, n] of a layer's oracle V output (position-tagged V)."""
    pos, ok = prng.decode_positions(np.asarray(v_out), case["dtype"])
    assert ok
    return pos
