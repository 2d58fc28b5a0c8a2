"""Generate golden fixtures by running the UNMODIFIED reference kvcompress (build container only).

    cd /root/repo && PYTHONPATH=/root/reference PYTHONDONTWRITEBYTECODE=1 \
        python tests/golden/gen_goldens.py [--prims-only | --append]

--append runs only the cases added after the last generation (ids are positional, so new cases
are only ever appended) and merges them into cases.json / positions.*.npz; the earlier cases'
definitions must be unchanged (checked).

The reference is imported from /root/reference (read-only); nothing of it is copied.  Outputs
(data only) go to tests/golden/:
  cases.json     - per case: method, kwargs, input recipe (seeds/shapes/dtype/variant), and per
                   layer the output kind (same/view/new), shapes and SHA-256 of K_out/V_out bytes
  positions.*.npz - per case/layer: source sequence position of every output row [B,H,n_out],
                   recovered by re-running the reference with position-encoding values (stored
                   in parts under 1 MiB each, like the prims: npz_parts.py)
  prims.json / prims.*.npz - torch.norm / argsort / topk outputs on tie-heavy rows, and the
                   snapkv_lite scoring tensors (max + 1e-6, scores, pooled) per dtype
Inputs are regenerated from tests/golden/prng.py recipes (hashes stored to detect drift: of K for
every case, of V too -- `v_input_sha` -- for the cases generated since layer recipes can carry a
`vvariant`, the variant of prng.gen_values).
"""
import hashlib
import json
import os
import sys
import traceback

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import npz_parts  # noqa: E402
import prng  # noqa: E402

assert os.path.abspath(os.environ.get("PYTHONPATH", "").split(":")[0]) == "/root/reference", \
    "run with PYTHONPATH=/root/reference"
import kvcompress  # noqa: E402  (the reference)
from kvcompress.methods import get_compress_fn, list_methods  # noqa: E402
from kvcompress.methods.streaming_llm import evict_for_space  # noqa: E402  (exported, unregistered)

torch.set_num_threads(8)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def to_torch(a, dtype):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.view(torch.bfloat16) if dtype == "bf16" else t  # fp16: numpy float16 -> torch.half


def to_np(t, dtype):
    t = t.contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if dtype == "bf16" else t.numpy()


def make_layers(case, values="data"):
    out = []
    for L in case["layers"]:
        shape = tuple(L["shape"])
        K = prng.gen_keys(L["kseed"], shape, case["dtype"], L.get("variant", "normal"))
        if values == "data":
            V = prng.gen_values(L["kseed"], shape, case["dtype"], L.get("vvariant", "normal"))
        else:
            V = prng.encode_positions(shape, case["dtype"])
        out.append((K, V))
    return out


def kind_of(tin, tout):
    if tout is tin:
        return "same"
    if tout.untyped_storage().data_ptr() == tin.untyped_storage().data_ptr():
        return "view"
    return "new"


CASES = []


def add(method, kwargs, dtype, layers, tag=""):
    cid = f"{len(CASES):03d}_{method}_{dtype}{('_' + tag) if tag else ''}"
    CASES.append({"id": cid, "method": method, "kwargs": kwargs, "dtype": dtype,
                  "layers": layers})


def L(shape, seed, variant="normal", vvariant=None):
    """One layer's recipe; `vvariant` (prng.gen_values' variant) is stored only when given, so the
    recipes of the earlier cases stay as they were."""
    r = {"shape": list(shape), "kseed": seed, "variant": variant}
    if vvariant is not None:
        r["vvariant"] = vvariant
    return r


def build_cases():
    s = 1000
    # ---- fix_size_l2 (BASELINE cfg2 + headline geometry, and edges) ----
    add("fix_size_l2", {"fix_kv_size": 512, "keep_ratio": 0.0, "strategy": "keep_low",
                        "skip_layers": []}, "bf16", [L((1, 32, 4096, 128), s + 1)], "cfg2")
    add("fix_size_l2", {"fix_kv_size": 512, "keep_ratio": 0.0, "strategy": "keep_low",
                        "skip_layers": []}, "bf16", [L((1, 32, 16384, 128), s + 2)], "headline")
    for dt in ("bf16", "fp32"):
        for D in (64, 80, 128):
            for var in ("normal", "scaled", "few", "special"):
                add("fix_size_l2", {"fix_kv_size": 256, "keep_ratio": 0.5, "strategy": "keep_low"},
                    dt, [L((1, 4, 700, D), s + 10 + D), L((1, 4, 900, D), s + 11 + D),
                         L((2, 3, 1500, D), s + 12 + D, var)], f"D{D}_{var}")
        add("fix_size_l2", {"fix_kv_size": 300, "keep_ratio": 0.0, "strategy": "keep_high",
                            "skip_layers": [1]}, dt,
            [L((1, 4, 1000, 128), s + 20), L((1, 4, 1000, 128), s + 21),
             L((1, 4, 2000, 128), s + 22, "few")], "keep_high")
        add("fix_size_l2", {"fix_kv_size": 64, "keep_ratio": 0.3, "strategy": "keep_low",
                            "skip_layers": []}, dt,
            [L((1, 2, 5000, 64), s + 23, "equal"), L((1, 2, 65, 64), s + 24),
             L((1, 2, 64, 64), s + 25)], "equal_edge")
    add("fix_size_l2", {"fix_kv_size": 100, "keep_ratio": 1.0, "skip_layers": []}, "bf16",
        [L((1, 2, 300, 64), s + 30)], "keep_le0_view")
    add("fix_size_l2", {"fix_kv_size": 0, "keep_ratio": 0.5, "skip_layers": []}, "bf16",
        [L((1, 2, 40, 64), s + 31)], "fix0_quirk")
    add("fix_size_l2", {"fix_kv_size": 32, "strategy": "bogus", "skip_layers": []}, "bf16",
        [L((1, 2, 40, 64), s + 32)], "bad_strategy")
    # ---- l2_compress ----
    for dt in ("bf16", "fp32"):
        add("l2_compress", {"keep_ratio": 0.8, "prune_after": 100}, dt,
            [L((1, 4, 1000, 128), s + 40), L((1, 4, 1000, 128), s + 41),
             L((1, 4, 1000, 128), s + 42, "special"), L((1, 4, 90, 128), s + 43)], "cfg1")
        add("l2_compress", {"keep_ratio": 0.3, "prune_after": 10, "skip_layers": []}, dt,
            [L((2, 2, 777, 80), s + 44, "few")], "kr03")
    add("l2_compress", {"keep_ratio": 1.0}, "bf16", [L((1, 2, 2000, 64), s + 45)], "passthrough")
    add("l2_compress", {"keep_ratio": 0.0, "prune_after": 10, "skip_layers": []}, "bf16",
        [L((1, 2, 50, 64), s + 46)], "kr0_empty")
    add("l2_compress", {"keep_ratio": 0.8, "prune_after": 100, "skip_layers": []}, "bf16",
        [L((1, 32, 16384, 128), s + 47)], "S16384")
    # ---- streaming_llm ----
    for dt in ("bf16", "fp32"):
        add("streaming_llm", {"start_size": 4, "recent_size": 1020}, dt,
            [L((1, 4, 2048, 128), s + 50), L((1, 4, 1000, 128), s + 51)], "cfg3")
    add("streaming_llm", {"start_size": 4, "recent_size": 0, "skip_layers": [1]}, "bf16",
        [L((1, 2, 30, 64), s + 52), L((1, 2, 30, 64), s + 53)], "recent0_quirk")
    # ---- h2o_l2 ----
    for dt in ("bf16", "fp32"):
        for D in (64, 80, 128):
            add("h2o_l2", {"start_size": 4, "heavy_hitter_size": 64, "recent_size": 444}, dt,
                [L((1, 4, 2048, D), s + 60 + D), L((1, 4, 600, D), s + 61 + D, "few"),
                 L((1, 4, 513, D), s + 62 + D)], f"cfg4_D{D}")
    add("h2o_l2", {"start_size": 4, "heavy_hitter_size": 64, "recent_size": 444}, "bf16",
        [L((1, 32, 16384, 128), s + 63)], "S16384")
    add("h2o_l2", {"start_size": 4, "heavy_hitter_size": 64, "recent_size": 0}, "bf16",
        [L((1, 2, 100, 64), s + 64)], "recent0_quirk")
    add("h2o_l2", {"start_size": 2, "heavy_hitter_size": 30, "recent_size": 10}, "bf16",
        [L((1, 2, 300, 64), s + 65, "equal"), L((1, 2, 300, 64), s + 66, "special")], "ties")
    # ---- snapkv_lite ----
    for dt in ("bf16", "fp32"):
        for var in ("normal", "few", "tiny", "zero", "special"):
            add("snapkv_lite", {"observation_window": 32, "keep_size": 512, "pooling_kernel": 5},
                dt, [L((1, 4, 2048, 128), s + 70), L((1, 4, 1500, 80), s + 71, var)],
                f"cfg5_{var}")
        add("snapkv_lite", {"observation_window": 8, "keep_size": 40, "pooling_kernel": 4}, dt,
            [L((1, 4, 4096, 64), s + 72), L((1, 2, 2048, 64), s + 73, "few")], "partialsort_even")
        add("snapkv_lite", {"observation_window": 16, "keep_size": 100, "pooling_kernel": 1}, dt,
            [L((1, 4, 600, 64), s + 74)], "nopool")
    add("snapkv_lite", {"observation_window": 0, "keep_size": 50, "pooling_kernel": 5}, "bf16",
        [L((1, 2, 120, 64), s + 75)], "obs0_quirk")
    add("snapkv_lite", {"observation_window": 60, "keep_size": 50, "pooling_kernel": 5}, "bf16",
        [L((1, 2, 120, 64), s + 76), L((1, 2, 55, 64), s + 77)], "keep_le_obs")
    add("snapkv_lite", {"observation_window": 32, "keep_size": 512, "pooling_kernel": 7}, "bf16",
        [L((1, 32, 16384, 128), s + 78)], "S16384")
    # ---- pyramid_kv ----
    for dt in ("bf16", "fp32"):
        add("pyramid_kv", {"base_size": 512, "layer_decay": 0.9}, dt,
            [L((1, 4, 1024, 128), s + 80 + j) for j in range(6)], "cfg5")
    add("pyramid_kv", {"base_size": 300, "min_size": 40, "profile": "linear"}, "bf16",
        [L((1, 2, 400, 64), s + 90 + j) for j in range(5)], "linear")
    add("pyramid_kv", {"base_size": 200, "profile": "constant", "skip_layers": [0]}, "bf16",
        [L((1, 2, 400, 64), s + 96 + j) for j in range(3)], "constant")
    add("pyramid_kv", {"base_size": 16, "min_size": 1, "layer_decay": 0.5}, "bf16",
        [L((1, 2, 40, 64), s + 100 + j) for j in range(6)], "tiny_sizes")
    # ---- adaptive_l2 ----
    for dt in ("bf16", "fp32"):
        add("adaptive_l2", {"target_size": 512}, dt,
            [L((1, 4, 2048, 128), s + 110), L((1, 4, 600, 128), s + 111),
             L((1, 4, 1024, 128), s + 112, "few"), L((1, 4, 200, 128), s + 113)], "mixed")
    add("adaptive_l2", {"target_size": 6, "soft_limit": 2, "hard_limit": 64}, "bf16",
        [L((1, 2, 100, 64), s + 114), L((1, 2, 3, 64), s + 115), L((1, 2, 30, 64), s + 116)],
        "edges")
    add("adaptive_l2", {"target_size": 512}, "bf16", [L((1, 32, 16384, 128), s + 117)], "S16384")
    # ---- recent_only ----
    add("recent_only", {"window_size": 512}, "bf16",
        [L((1, 2, 1024, 64), s + 120), L((1, 2, 1024, 64), s + 121),
         L((1, 2, 1024, 64), s + 122), L((1, 2, 300, 64), s + 123)], "default")
    # ---- fp16 K/V (what transformers 5 loads pythia checkpoints as: dtype="auto" -> float16)
    # and the snapkv epsilon at the bottom of each dtype's range (appended: earlier ids stay) ----
    f = "fp16"
    add("fix_size_l2", {"fix_kv_size": 512, "keep_ratio": 0.0, "strategy": "keep_low",
                        "skip_layers": []}, f, [L((1, 32, 4096, 128), s + 130)], "cfg2")
    for D in (64, 80, 128):
        for var in ("normal", "scaled", "few", "special"):
            add("fix_size_l2", {"fix_kv_size": 256, "keep_ratio": 0.5, "strategy": "keep_low"},
                f, [L((1, 4, 700, D), s + 131 + D), L((2, 3, 1500, D), s + 132 + D, var)],
                f"D{D}_{var}")
    add("fix_size_l2", {"fix_kv_size": 300, "keep_ratio": 0.0, "strategy": "keep_high",
                        "skip_layers": [1]}, f,
        [L((1, 4, 1000, 128), s + 133), L((1, 4, 1000, 128), s + 134),
         L((1, 4, 2000, 128), s + 135, "few")], "keep_high")
    add("fix_size_l2", {"fix_kv_size": 64, "keep_ratio": 0.3, "strategy": "keep_low",
                        "skip_layers": []}, f,
        [L((1, 2, 5000, 64), s + 136, "equal"), L((1, 2, 65, 64), s + 137)], "equal_edge")
    add("l2_compress", {"keep_ratio": 0.8, "prune_after": 100}, f,
        [L((1, 4, 1000, 128), s + 140), L((1, 4, 1000, 128), s + 141),
         L((1, 4, 1000, 128), s + 142, "special"), L((1, 4, 90, 128), s + 143)], "cfg1")
    add("streaming_llm", {"start_size": 4, "recent_size": 1020}, f,
        [L((1, 4, 2048, 128), s + 144), L((1, 4, 1000, 128), s + 145, "special")], "cfg3")
    for D in (64, 80, 128):
        add("h2o_l2", {"start_size": 4, "heavy_hitter_size": 64, "recent_size": 444}, f,
            [L((1, 4, 2048, D), s + 150 + D), L((1, 4, 600, D), s + 151 + D, "few"),
             L((1, 4, 513, D), s + 152 + D, "special")], f"cfg4_D{D}")
    for var in ("normal", "few", "tiny", "micro", "zero", "special"):
        add("snapkv_lite", {"observation_window": 32, "keep_size": 512, "pooling_kernel": 5},
            f, [L((1, 4, 2048, 128), s + 160), L((1, 4, 1500, 80), s + 161, var)],
            f"cfg5_{var}")
    add("snapkv_lite", {"observation_window": 8, "keep_size": 40, "pooling_kernel": 4}, f,
        [L((1, 4, 4096, 64), s + 162), L((1, 2, 2048, 64), s + 163, "few")], "partialsort_even")
    for dt in ("bf16", "fp32"):
        add("snapkv_lite", {"observation_window": 32, "keep_size": 512, "pooling_kernel": 5},
            dt, [L((1, 4, 1500, 80), s + 164, "micro"), L((1, 4, 700, 128), s + 165, "micro")],
            "cfg5_micro")
    add("pyramid_kv", {"base_size": 512, "layer_decay": 0.9}, f,
        [L((1, 4, 1024, 128), s + 170 + j) for j in range(6)], "cfg5")
    add("adaptive_l2", {"target_size": 512}, f,
        [L((1, 4, 2048, 128), s + 180), L((1, 4, 600, 128), s + 181),
         L((1, 4, 1024, 128), s + 182, "few"), L((1, 4, 200, 128), s + 183)], "mixed")
    add("fix_size_l2", {"fix_kv_size": 512, "keep_ratio": 0.0, "strategy": "keep_low",
                        "skip_layers": []}, f, [L((1, 32, 16384, 128), s + 184)], "headline")
    # ---- the rest of the pythia family's head dims: D = 32 (14m/31m), D = 256 (1b) ----
    for dt in ("bf16", "fp16", "fp32"):
        for D in (32, 256):
            add("fix_size_l2", {"fix_kv_size": 256, "keep_ratio": 0.5, "strategy": "keep_low"},
                dt, [L((1, 4, 700, D), s + 190 + D), L((2, 3, 1500, D), s + 191 + D, "few"),
                     L((1, 4, 900, D), s + 192 + D, "special")], f"D{D}")
            add("snapkv_lite", {"observation_window": 32, "keep_size": 512, "pooling_kernel": 5},
                dt, [L((1, 4, 2048, D), s + 193 + D), L((1, 4, 1500, D), s + 194 + D, "few")],
                f"D{D}")
            add("h2o_l2", {"start_size": 4, "heavy_hitter_size": 64, "recent_size": 444}, dt,
                [L((1, 4, 2048, D), s + 195 + D), L((1, 4, 513, D), s + 196 + D, "scaled")],
                f"D{D}")
    # ---- round 2: the BASELINE configs at their exact geometries (pythia-2.8b: D = 80,
    # pythia-6.9b: D = 128, 32 heads), and evict_for_space (streaming_llm.py:114-170) ----
    add("fix_size_l2", {"fix_kv_size": 512, "keep_ratio": 0.0, "strategy": "keep_low",
                        "skip_layers": []}, "bf16", [L((1, 32, 4096, 80), s + 300)], "cfg2_D80")
    add("h2o_l2", {"start_size": 4, "heavy_hitter_size": 64, "recent_size": 444}, "bf16",
        [L((1, 32, 16384, 80), s + 301)], "cfg4_S16384_D80")
    add("streaming_llm", {"start_size": 4, "recent_size": 1020}, "bf16",
        [L((1, 32, 16384, 80), s + 302)], "cfg3_S16384_D80")
    add("snapkv_lite", {"observation_window": 32, "keep_size": 512, "pooling_kernel": 5}, "bf16",
        [L((1, 32, 16384, 128), s + 303)], "cfg5_S16384_pk5")
    # pyramid_kv over a whole 32-layer pythia-6.9b stack: layers >= 20 hit the min_size clamp
    add("pyramid_kv", {"base_size": 512}, "bf16",
        [L((1, 32, 1500, 128), s + 310 + j) for j in range(32)], "cfg5_32layers")
    for dt in ("bf16", "fp16", "fp32"):
        add("evict_for_space", {"num_coming": 1, "start_size": 4, "recent_size": 508}, dt,
            [L((1, 4, 512, 64), s + 350), L((1, 4, 511, 64), s + 351),
             L((1, 4, 1000, 80), s + 352)], "one")
    add("evict_for_space", {"num_coming": 600, "start_size": 4, "recent_size": 508}, "bf16",
        [L((1, 2, 100, 64), s + 353), L((1, 2, 2000, 64), s + 354)], "coming_gt_recent")
    add("evict_for_space", {"num_coming": 508, "start_size": 4, "recent_size": 508,
                            "skip_layers": [1]}, "bf16",
        [L((1, 2, 700, 64), s + 355), L((1, 2, 700, 64), s + 356), L((1, 2, 3, 64), s + 357)],
        "coming_eq_recent_skip")
    add("evict_for_space", {"num_coming": 0, "start_size": 4, "recent_size": 0}, "bf16",
        [L((1, 2, 30, 64), s + 358)], "recent0_quirk")
    add("evict_for_space", {"num_coming": 100, "start_size": 0, "recent_size": 1020}, "bf16",
        [L((1, 32, 16384, 80), s + 359)], "S16384_D80")
    # ---- round 6: fp32 -- the dtype of the reference's own published runs (scripts/benchmark.py
    # loads the model with no torch_dtype) -- at the BASELINE geometries: the untied radix fast
    # path (headline), fp32 snapkv scoring + introselect (cfg5), h2o_l2's middle (cfg4), and a
    # tie-heavy headline row set that takes the partition chain at 16 384 positions ----
    add("fix_size_l2", {"fix_kv_size": 512, "keep_ratio": 0.0, "strategy": "keep_low",
                        "skip_layers": []}, "fp32", [L((1, 32, 16384, 128), s + 400)],
        "headline_fp32")
    add("snapkv_lite", {"observation_window": 32, "keep_size": 512, "pooling_kernel": 5}, "fp32",
        [L((1, 32, 16384, 128), s + 401)], "cfg5_S16384_pk5_fp32")
    add("h2o_l2", {"start_size": 4, "heavy_hitter_size": 64, "recent_size": 444}, "fp32",
        [L((1, 32, 16384, 80), s + 402)], "cfg4_S16384_D80_fp32")
    add("fix_size_l2", {"fix_kv_size": 512, "keep_ratio": 0.0, "strategy": "keep_low",
                        "skip_layers": []}, "fp32", [L((1, 8, 16384, 128), s + 403, "few")],
        "headline_fp32_ties")
    # ---- NaN payloads (tests/test_nan_payload.py): "payload" keys (non-canonical NaNs of both
    # signs in every 9th row) and "patterns" values (every NaN bit pattern of the dtype, in both
    # halves of a word).  A NaN norm sorts last ascending, so the selections keep nearly the
    # whole zone (or its largest norms first): the gathered segment then holds NaN key rows and
    # enough value rows for every pattern.  No registered method selects a whole zone
    # (n_select == zone_len), so that layer shape has no golden; the GPU tests reach it through
    # the C ABI. ----
    def P(shape, seed):
        return L(shape, seed, "payload", "patterns")

    big = (2, 3, 1500, 64)
    for dt in ("bf16", "fp16"):
        t = "nan"
        add("fix_size_l2", {"fix_kv_size": 1400, "keep_ratio": 0.25, "strategy": "keep_low",
                            "skip_layers": []}, dt, [P(big, s + 500), P((2, 3, 1450, 64), s + 501)], t)
        add("fix_size_l2", {"fix_kv_size": 1200, "keep_ratio": 0.25, "strategy": "keep_high",
                            "skip_layers": []}, dt, [P(big, s + 502)], t + "_keep_high")
        add("l2_compress", {"keep_ratio": 0.95, "prune_after": 100, "skip_layers": []}, dt,
            [P(big, s + 503)], t + "_all_gathered")
        add("streaming_llm", {"start_size": 4, "recent_size": 1020}, dt, [P(big, s + 504)], t)
        add("recent_only", {"window_size": 512, "skip_layers": []}, dt, [P(big, s + 505)], t)
        add("h2o_l2", {"start_size": 4, "heavy_hitter_size": 1200, "recent_size": 200}, dt,
            [P(big, s + 506)], t)
        add("snapkv_lite", {"observation_window": 32, "keep_size": 1200, "pooling_kernel": 5}, dt,
            [P(big, s + 507)], t)
        add("pyramid_kv", {"base_size": 1450, "layer_decay": 1.0}, dt,
            [P(big, s + 508), P(big, s + 509)], t)
        add("adaptive_l2", {"target_size": 1450, "soft_limit": 256, "hard_limit": 1400,
                            "keep_ratio_min": 0.97, "keep_ratio_max": 0.97}, dt,
            [P(big, s + 510), P((2, 3, 1300, 64), s + 511)], t)
        add("evict_for_space", {"num_coming": 1, "start_size": 4, "recent_size": 508}, dt,
            [P(big, s + 512)], t)
    for m, kw in (("fix_size_l2", {"fix_kv_size": 1400, "keep_ratio": 0.25, "strategy": "keep_low",
                                   "skip_layers": []}),
                  ("h2o_l2", {"start_size": 4, "heavy_hitter_size": 1200, "recent_size": 200}),
                  ("snapkv_lite", {"observation_window": 32, "keep_size": 1200,
                                   "pooling_kernel": 5})):
        add(m, kw, "fp32", [P(big, s + 520)], "nan")
    add("fix_size_l2", {"fix_kv_size": 1400, "keep_ratio": 0.0, "strategy": "keep_low",
                        "skip_layers": []}, "bf16", [P(big, s + 530)], "nan_no_tail")
    add("fix_size_l2", {"fix_kv_size": 1400, "keep_ratio": 0.0, "strategy": "keep_low",
                        "skip_layers": []}, "fp16", [P(big, s + 531)], "nan_no_tail")
    add("h2o_l2", {"start_size": 4, "heavy_hitter_size": 1200, "recent_size": 200}, "fp16",
        [P((2, 3, 1500, 80), s + 532)], "nan_D80")
    add("h2o_l2", {"start_size": 4, "heavy_hitter_size": 1200, "recent_size": 200}, "bf16",
        [P((2, 3, 1500, 256), s + 533)], "nan_D256")


def method_fn(name):
    return evict_for_space if name == "evict_for_space" else get_compress_fn(name)


def run_case(case, positions):
    fn = method_fn(case["method"])
    dt = case["dtype"]
    rec = dict(case)
    layers = make_layers(case)
    rec["input_sha"] = [sha(K) for K, _ in layers]
    rec["v_input_sha"] = [sha(V) for _, V in layers]
    tin = [(to_torch(K, dt), to_torch(V, dt)) for K, V in layers]
    try:
        out = fn(list(tin), **case["kwargs"])
    except Exception as e:  # reference raises -> record the exception type
        rec["error"] = type(e).__name__
        rec["out"] = None
        return rec
    rec["error"] = None
    enc = [(to_torch(K, dt), to_torch(prng.encode_positions(K.shape, dt), dt)) for K, _ in layers]
    out_enc = fn(list(enc), **case["kwargs"])
    res = []
    for li, ((ki, vi), (ko, vo), (_, veo)) in enumerate(zip(tin, out, out_enc)):
        kk, kv = kind_of(ki, ko), kind_of(vi, vo)
        assert kk == kv
        r = {"kind": kk, "k_shape": list(ko.shape), "v_shape": list(vo.shape),
             "k_sha": sha(to_np(ko, dt)), "v_sha": sha(to_np(vo, dt))}
        if kk != "same":
            pos, ok = prng.decode_positions(to_np(veo, dt), dt)
            assert ok, case["id"]
            key = f"{case['id']}__L{li}"
            positions[key] = pos.astype(np.int16 if ko.shape[2] and pos.max() < 32768 else np.int32)
            r["pos_key"] = key
        res.append(r)
    rec["out"] = res
    return rec


def gen_prims():
    """Direct fixtures for the torch primitives the oracle restates."""
    meta, arrs = [], {}
    for dt in ("bf16", "fp32", "fp16"):
        for D in (64, 80, 128):
            for var in ("normal", "scaled", "special", "few"):
                seed = 5000 + D + {"bf16": 0, "fp32": 7, "fp16": 3}[dt] + 11 * ("normal", "scaled", "special", "few").index(var)
                K = prng.gen_keys(seed, (1, 4, 2048, D), dt, var)
                n = torch.norm(to_torch(K, dt), p=2, dim=-1)
                nn = to_np(n, dt)
                key = f"norm_{dt}_D{D}_{var}"
                arrs[key] = nn
                asc = n.argsort(dim=-1).numpy().astype(np.int16)
                desc = n.argsort(dim=-1, descending=True).numpy().astype(np.int16)
                arrs[key + "_argsort"] = asc
                arrs[key + "_argsort_desc"] = desc
                tk = {}
                for k in (1, 16, 31, 32, 480, 2047):
                    tk[k] = torch.topk(n, k, dim=-1)[1].numpy().astype(np.int16)
                    arrs[f"{key}_topk{k}"] = tk[k]
                meta.append({"key": key, "dtype": dt, "D": D, "variant": var, "seed": seed,
                             "shape": [1, 4, 2048, D], "input_sha": sha(K),
                             "topk_ks": [1, 16, 31, 32, 480, 2047]})
    return meta, arrs


def gen_snapkv_prims():
    """snapkv_lite's scoring tensors (snapkv_lite.py:96-121: norm, max + 1e-6, subtraction,
    avg_pool1d) evaluated with torch on rows whose maxima sit where the python scalar's dtype
    cast is visible (bf16 [2e-9, 4e-9), fp16 [1.2e-4, 2.4e-4)) and on ordinary rows."""
    meta, arrs = [], {}
    i = 0
    for dt in ("bf16", "fp16", "fp32"):
        for var in ("micro", "tiny", "normal", "special"):
            for pk in (5, 4):
                seed = 7000 + i
                i += 1
                shape = (1, 8, 1000, 80)
                K = prng.gen_keys(seed, shape, dt, var)
                n = torch.norm(to_torch(K, dt), p=2, dim=-1)
                m = n.max(dim=-1, keepdim=True)[0] + 1e-6
                sc = m - n
                pooled = torch.nn.functional.avg_pool1d(sc.view(8, 1, 1000), kernel_size=pk,
                                                        stride=1, padding=pk // 2)[:, :, :1000]
                key = f"snapkv_{dt}_{var}_pk{pk}"
                arrs[key + "_max_eps"] = to_np(m, dt)
                arrs[key + "_scores"] = to_np(sc, dt)
                arrs[key + "_pooled"] = to_np(pooled.view(1, 8, 1000), dt)
                meta.append({"key": key, "dtype": dt, "variant": var, "seed": seed,
                             "shape": list(shape), "pool": pk, "input_sha": sha(K)})
    return meta, arrs


def write_prims(meta):
    pm, pa = gen_prims()
    sm, sa = gen_snapkv_prims()
    with open(os.path.join(HERE, "prims.json"), "w") as f:
        json.dump({"meta": meta, "prims": pm, "snapkv": sm}, f, indent=1)
    npz_parts.save("prims", {**pa, **sa})
    return pm, sm


def append_new():
    with open(os.path.join(HERE, "cases.json")) as f:
        old = json.load(f)
    have = old["cases"]
    build_cases()
    for rec, c in zip(have, CASES):  # earlier definitions must be untouched
        assert rec["id"] == c["id"] and rec["kwargs"] == c["kwargs"] and \
            rec["layers"] == c["layers"], rec["id"]
    positions = npz_parts.load("positions")
    new = []
    for c in CASES[len(have):]:
        new.append(run_case(c, positions))
        print(c["id"], "error" if new[-1]["error"] else "ok", flush=True)
    old["cases"] = have + new
    with open(os.path.join(HERE, "cases.json"), "w") as f:
        json.dump(old, f, indent=1)
    npz_parts.save("positions", positions)
    print("appended", len(new), "cases; total", len(old["cases"]))


def main():
    if "--append" in sys.argv:
        append_new()
        return
    if "--prims-only" in sys.argv:
        with open(os.path.join(HERE, "cases.json")) as f:
            meta = json.load(f)["meta"]
        pm, sm = write_prims(meta)
        print("wrote", len(pm), "prim sets,", len(sm), "snapkv score sets")
        return
    build_cases()
    positions = {}
    recs = []
    for c in CASES:
        try:
            recs.append(run_case(c, positions))
        except Exception:
            traceback.print_exc()
            raise
        print(c["id"], "error" if recs[-1]["error"] else "ok", flush=True)
    meta = {"torch": torch.__version__, "cpu_capability": torch.backends.cpu.get_cpu_capability(),
            "reference_version": kvcompress.__version__, "list_methods": list_methods(),
            "generator": "tests/golden/gen_goldens.py"}
    with open(os.path.join(HERE, "cases.json"), "w") as f:
        json.dump({"meta": meta, "cases": recs}, f, indent=1)
    npz_parts.save("positions", positions)
    pm, sm = write_prims(meta)
    print("wrote", len(recs), "cases,", len(positions), "position arrays,", len(pm), "prim sets,",
          len(sm), "snapkv score sets")


if __name__ == "__main__":
    main()
