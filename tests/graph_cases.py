"""Case tables, seeded fills and CPU expectations of the graph capture tests
(tests/test_graph_capture.py: its GPU tests replay each case, its unmarked tests prove here that
the fills of a case cannot be mistaken for one another).  Numpy only.

A captured graph is replayed over static buffers that are refilled before every replay; `fill`
numbers the seeded contents.  Every expectation comes from the CPU oracle on the contents of
that fill and is computed once per case.
"""
import numpy as np

import dest_cases as DC
import h2o_inputs
import phase_tables as PT
import prng
from oracle import h2o_oracle as HO
from oracle import oracle

D = 64
FILLS = (0, 1)
FILL_STEP = 100003  # seed distance of two fills: no table's seeds are that far apart


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


# ----------------------------------------------------------------------------------------------
# A. layer tables launched through the C ABI
# ----------------------------------------------------------------------------------------------
def _split_keys():
    keys = [("split", Z, "bf16") for Z in PT.SPLIT_ZONES]
    return sorted(keys + [("split", 1000, "fp32"), ("split", 8256, "fp32")], key=lambda k: k[1])


SPLIT_KEYS = _split_keys()
SNAPKV_KEYS = [("snapkv",) + min(PT.snapkv_cases())]
STABLE_KEYS = [("stable", 1000, "bf16"), ("stable", 16448, "bf16")]
CHUNK_KEYS = [("chunk", 65, "bf16")]
TABLE_KEYS = SPLIT_KEYS + SNAPKV_KEYS + STABLE_KEYS + CHUNK_KEYS


def key_id(key):
    return "-".join(str(x) for x in key)


def table_case(key):
    """dict(specs, B, H, dtype, order, algo) of a table key (fill 0's seeds)."""
    kind, n, dtype = key[:3]
    if kind == "chunk":
        return dict(specs=PT.chunk_table(n), B=1, H=1, dtype=dtype, order=PT.ASC, algo=PT.SORT)
    B, H = PT.split_geometry(n)
    if kind == "snapkv":
        return dict(specs=PT.split_table(n, PT.SNAPKV, key[3]), B=B, H=H, dtype=dtype,
                    order=PT.DESC, algo=PT.TOPK)
    if kind == "stable":
        return dict(specs=PT.split_table(n), B=B, H=H, dtype=dtype, order=PT.ASC, algo=PT.STABLE)
    order, algo = (PT.ASC, PT.SORT) if dtype == "bf16" else (PT.DESC, PT.TOPK)
    return dict(specs=PT.split_table(n), B=B, H=H, dtype=dtype, order=order, algo=algo)


_TABLE = {}


def table_expected(key, fill):
    """(host layers [(K, V)], [(K_out, V_out, indices)] from phase_tables' expectations) of one
    fill; the fills of one key stay cached until another key is asked for."""
    if (key, fill) not in _TABLE:
        if any(k != key for k, _ in _TABLE):
            _TABLE.clear()
        c = table_case(key)
        specs = [dict(s, seed=s["seed"] + FILL_STEP * fill) for s in c["specs"]]
        host = PT.gen_layers(specs, c["B"], c["H"], D, c["dtype"])
        want = [PT.expected_layer(k, v, s, c["order"], c["algo"]) for (k, v), s in zip(host, specs)]
        _TABLE[(key, fill)] = (host, want)
    return _TABLE[(key, fill)]


def selects(s):
    return 0 < s["n_select"] < s["zone_len"]


# ----------------------------------------------------------------------------------------------
# A4. destinations: the smallest selecting in-place and strided cases of dest_cases
# ----------------------------------------------------------------------------------------------
def _nbytes(c):
    return sum(int(np.prod(s)) for s in c["shapes"]) * (4 if c["dtype"] == "fp32" else 2)


def _selecting(cases):
    return [c for c in cases if c["method"] not in ("streaming_llm", "evict_for_space",
                                                    "recent_only") and "window-only" not in c["id"]]


DEST_INPLACE = min(_selecting(DC.INPLACE), key=_nbytes)
DEST_STRIDED = min(_selecting(DC.STRIDED), key=_nbytes)


# ----------------------------------------------------------------------------------------------
# A5. an external-index gather with one index behind its zone
# ----------------------------------------------------------------------------------------------
STATUS = dict(H=4, S=256, zone_start=10, zone_len=100, index=(5, 7, 100), clamped=(5, 7, 99))


def status_keys(fill):
    """fp32 [1, H, S, D] keys of a fill; the values are their negation."""
    c = STATUS
    n = c["H"] * c["S"] * D
    return (np.arange(n, dtype=np.float32) + np.float32(n * fill + 1)).reshape(1, c["H"], c["S"], D)


# ----------------------------------------------------------------------------------------------
# A6 / A7. accumulate -> heavy hitters -> shared-index gather
# ----------------------------------------------------------------------------------------------
H2O = dict(L=2, H=4, S=600, q=3, dtype="bf16", start=4, heavy=32, recent=100, decay=0.9)
_H2O = {}


def h2o_expected(fill):
    """dict(layers, atts, out [(K, V)], idx, acc) of one fill: oracle/h2o_oracle.py's manager on a
    first step (no carried accumulation).  q * S * H is below aten's parallel grain, so the sums'
    order does not depend on a thread count."""
    if fill not in _H2O:
        c = H2O
        shape = (1, c["H"], c["S"], D)
        seeds = [9100 + FILL_STEP * fill + li for li in range(c["L"])]
        layers = [(prng.gen_keys(s, shape, c["dtype"]), prng.gen_values(s, shape, c["dtype"]))
                  for s in seeds]
        atts = [h2o_inputs.attention(s, c["H"], c["q"], c["S"], c["dtype"]) for s in seeds]
        kw = dict(start_size=c["start"], heavy_hitter_size=c["heavy"], recent_size=c["recent"])
        mgr = HO.H2OManager(decay_factor=c["decay"], threads=1, capability="AVX2", **kw)
        ref = HO.h2o_attention_compress(layers, attention_scores=atts, h2o_manager=mgr, **kw)
        assert all(kind == "new" for _, _, kind in ref)
        _H2O[fill] = dict(layers=layers, atts=atts, out=[(k, v) for k, v, _ in ref],
                          idx=[mgr.get_heavy_hitter_indices(li, c["S"]) for li in range(c["L"])],
                          acc=[mgr.acc[li] for li in range(c["L"])])
    return _H2O[fill]


# ----------------------------------------------------------------------------------------------
# B. the Python API: B = 1, H = 4, D = 64, four layers
# ----------------------------------------------------------------------------------------------
ORACLE = dict(oracle.METHODS)
ORACLE["fix_size_l2"] = oracle.fix_size_l2_compress

# one compressing configuration of each of the eight registry methods (tests/test_call_memo.py's)
API_LENS = (300, 301, 170, 300)
API_CASES = [
    ("l2_compress", dict(keep_ratio=0.5, prune_after=100, skip_layers=[])),
    ("fix_size_l2", dict(fix_kv_size=128, skip_layers=[0])),
    ("streaming_llm", dict(start_size=4, recent_size=100)),
    ("recent_only", dict(window_size=100, skip_layers=[1])),
    ("h2o_l2", dict(start_size=4, heavy_hitter_size=32, recent_size=60)),
    ("snapkv_lite", dict(observation_window=16, keep_size=120)),
    ("pyramid_kv", dict(base_size=160, min_size=8, skip_layers=[2])),
    ("adaptive_l2", dict(target_size=128, soft_limit=64, hard_limit=200)),
]
# B1: the decode step on static caches; B3: the shape whose workspaces the caches hold
DECODE = ("fix_size_l2", dict(fix_kv_size=512), (513,) * 4)
OWNED = ("fix_size_l2", dict(fix_kv_size=512, keep_ratio=0.5, skip_layers=[]), (2100,) * 4)

_API = {}


def api_expected(name, kw, lens, fill, seed=52000):
    """(numpy layers, oracle result [(K, V, kind)]) of one fill of a Python-API case."""
    key = (name, repr(sorted(kw.items())), tuple(lens), fill, seed)
    if key not in _API:
        layers = [(prng.gen_keys(seed + FILL_STEP * fill + i, (1, 4, S, D), "bf16", "few"),
                   prng.gen_values(seed + FILL_STEP * fill + i, (1, 4, S, D), "bf16"))
                  for i, S in enumerate(lens)]
        _API[key] = (layers, ORACLE[name](layers, **kw))
    return _API[key]
