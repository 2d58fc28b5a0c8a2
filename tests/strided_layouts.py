"""Non-contiguous K/V layouts for the strided-input tests (tests/test_strided_inputs.py on the
GPU, tests/test_strided_layouts.py on the CPU).

A layout carves a [B, H, S, D] view out of a larger contiguous backing buffer.  geometry() states
every layout's backing shape, storage offset and element strides as shape arithmetic; the numpy
and the device helper build their views with ordinary slicing / permuting and both assert that
arithmetic.  Everything of the backing outside the view is filled with 0x7F bytes (bf16 / fp32:
~3.4e38, fp16: a NaN), so an address computed from wrong strides reads recognisably wrong --
and never uninitialised -- data.

Arrays are in the fixtures' representation (bf16 as uint16 bits, tests/golden/prng.py).

The case tables of the GPU parity tests live here too, so that the CPU suite can prove (without a
GPU) that every case's inputs tell a stride-ignoring kernel from a correct one.
"""
import numpy as np

POISON = 0x7F

# name -> what it stresses
LAYOUTS = {
    "static": "[B,H,S+37,D][:, :, 5:5+S] -- head stride != S*D, offset start",
    "fused_qkv": "[B,S,H,3D].permute(0,2,1,3)[..., D:2D] (K) / [..., 2D:] (V) -- seq > head stride",
    "bshd": "[B,S,H,D].permute(0,2,1,3) -- permuted, dense",
    "head_slice": "[B,2H,S,D][:, 1::2] -- head stride doubled",
    "batch_slice": "[2B+1,H,S,D][1::2] -- batch stride doubled",
    "expand": "[1,H,S,D].expand(B,...) -- batch stride 0 (the input repeats batch 0)",
    "row_pad": "[B,H,S,D+4][..., :D] -- 16-bit rows of D = 64: seq stride not 16-B aligned",
    "row_off": "[B,H,S,D+8][..., 4:4+D] -- 16-bit: aligned strides, misaligned pointer",
}
STATIC_PAD, STATIC_START = 37, 5


def geometry(layout, shape, role="k"):
    """(backing shape, storage offset, element strides) of `layout`'s [B,H,S,D] view.  `role`
    ("k" / "v") picks the K or the V third of a fused_qkv row."""
    B, H, S, D = shape
    if layout == "static":
        T = S + STATIC_PAD
        return (B, H, T, D), STATIC_START * D, (H * T * D, T * D, D, 1)
    if layout == "fused_qkv":
        return (B, S, H, 3 * D), (1 if role == "k" else 2) * D, (S * H * 3 * D, 3 * D, H * 3 * D, 1)
    if layout == "bshd":
        return (B, S, H, D), 0, (S * H * D, D, H * D, 1)
    if layout == "head_slice":
        return (B, 2 * H, S, D), S * D, (2 * H * S * D, 2 * S * D, D, 1)
    if layout == "batch_slice":
        return (2 * B + 1, H, S, D), H * S * D, (2 * H * S * D, S * D, D, 1)
    if layout == "expand":
        return (1, H, S, D), 0, (0, S * D, D, 1)
    if layout == "row_pad":
        return (B, H, S, D + 4), 0, (H * S * (D + 4), S * (D + 4), D + 4, 1)
    if layout == "row_off":
        return (B, H, S, D + 8), 4, (H * S * (D + 8), S * (D + 8), D + 8, 1)
    raise ValueError(layout)


def contiguous_strides(shape):
    B, H, S, D = shape
    return (H * S * D, S * D, D, 1)


def prep_takes_as_is(strides, shape, offset, esz, base_aligned=True):
    """_engine._prep's three conditions restated on plain numbers: last dim contiguous, a 16-B
    aligned pointer, and every other stride a multiple of 16 bytes (or its dim of size 1)."""
    return (strides[3] == 1 and base_aligned and (offset * esz) % 16 == 0 and
            all((strides[d] * esz) % 16 == 0 or shape[d] == 1 for d in range(3)))


def _carve(backing, layout, role, shape, permute, expand):
    """The view of `backing` (numpy array or torch tensor: same slicing syntax)."""
    B, H, S, D = shape
    if layout == "static":
        return backing[:, :, STATIC_START:STATIC_START + S]
    if layout == "fused_qkv":
        lo = D if role == "k" else 2 * D
        return permute(backing)[..., lo:lo + D]
    if layout == "bshd":
        return permute(backing)
    if layout == "head_slice":
        return backing[:, 1::2]
    if layout == "batch_slice":
        return backing[1::2]
    if layout == "expand":
        return expand(backing)
    if layout == "row_pad":
        return backing[..., :D]
    if layout == "row_off":
        return backing[..., 4:4 + D]
    raise ValueError(layout)


def _check_input(layout, a_np):
    assert a_np.ndim == 4
    if layout == "expand":
        assert all(np.array_equal(a_np[:1].view(np.uint8), a_np[b:b + 1].view(np.uint8))
                   for b in range(a_np.shape[0])), "an expand input repeats batch 0"


def expand_input(a_np):
    """`a_np` with batch 0 repeated over the batch (the values an `expand` view can hold)."""
    return np.ascontiguousarray(np.broadcast_to(a_np[:1], a_np.shape))


def make_backing_np(layout, a_np, role="k", backing=None):
    """(backing, view): a poisoned numpy backing buffer (or the given one: fused K and V share
    theirs) and the `layout` view of it holding a_np's values."""
    _check_input(layout, a_np)
    a_np = np.ascontiguousarray(a_np)
    bshape, off, strides = geometry(layout, a_np.shape, role)
    if backing is None:
        backing = np.empty(bshape, dtype=a_np.dtype)
        backing.view(np.uint8)[...] = POISON
    assert backing.shape == bshape and backing.dtype == a_np.dtype
    view = _carve(backing, layout, role, a_np.shape, lambda x: x.transpose(0, 2, 1, 3),
                  lambda x: np.broadcast_to(x, a_np.shape))
    if layout == "expand":
        backing[...] = a_np[:1]
    else:
        view[...] = a_np
    es = a_np.dtype.itemsize
    assert tuple(s // es for s in view.strides) == strides
    assert (view.__array_interface__["data"][0] - backing.__array_interface__["data"][0]) == off * es
    return backing, view


def make_view_np(layout, a_np, role="k", backing=None):
    """numpy twin of make_view: a view with the same element strides (CPU tests)."""
    return make_backing_np(layout, a_np, role, backing)[1]


def misread_np(backing, view):
    """What a kernel that ignored the strides would read: the view's shape with CONTIGUOUS
    strides from the view's first element (inside the backing's bounds for every layout but
    `expand`)."""
    es = view.dtype.itemsize
    off = (view.__array_interface__["data"][0] - backing.__array_interface__["data"][0]) // es
    n = int(np.prod(view.shape))
    assert off + n <= backing.size, "contiguous strides would leave the backing"
    flat = backing.reshape(-1)[off:off + n]
    return np.lib.stride_tricks.as_strided(flat, view.shape,
                                           tuple(s * es for s in contiguous_strides(view.shape)),
                                           writeable=False)


def new_backing(layout, shape, dtype, device, role="k"):
    """An all-poison device backing buffer for `layout` views of `shape` (torch dtype)."""
    import torch
    b = torch.empty(geometry(layout, shape, role)[0], dtype=dtype, device=device)
    b.view(torch.uint8).fill_(POISON)
    return b


def make_view(layout, a_np, device="cuda:0", role="k", backing=None):
    """Device view of `layout` holding a_np's values, carved out of a fresh poisoned backing
    buffer (or `backing`, so that a fused K and V share one)."""
    from gpu_util import to_dev
    _check_input(layout, a_np)
    src = to_dev(a_np, device)
    bshape, off, strides = geometry(layout, tuple(src.shape), role)
    if backing is None:
        backing = new_backing(layout, tuple(src.shape), src.dtype, device, role)
    assert tuple(backing.shape) == bshape and backing.dtype == src.dtype
    view = _carve(backing, layout, role, tuple(src.shape), lambda x: x.permute(0, 2, 1, 3),
                  lambda x: x.expand(*src.shape))
    if layout == "expand":
        backing.copy_(src[:1])
    else:
        view.copy_(src)
    assert tuple(view.stride()) == strides and view.storage_offset() - backing.storage_offset() == off
    assert view.untyped_storage().data_ptr() == backing.untyped_storage().data_ptr()
    return view


def make_pair(k_layout, v_layout, k_np, v_np, device="cuda:0"):
    """(K view, V view); two fused_qkv views are the K and V thirds of ONE projection buffer."""
    import torch
    shared = None
    if k_layout == v_layout == "fused_qkv":
        dt = {np.dtype(np.uint16): torch.bfloat16, np.dtype(np.float16): torch.float16,
              np.dtype(np.float32): torch.float32}[k_np.dtype]
        shared = new_backing("fused_qkv", k_np.shape, dt, device)
    return (make_view(k_layout, k_np, device, "k", backing=shared),
            make_view(v_layout, v_np, device, "v", backing=shared))


def make_pair_np(k_layout, v_layout, k_np, v_np):
    """((K backing, K view), (V backing, V view)) -- numpy twin of make_pair."""
    kb, kv = make_backing_np(k_layout, k_np, "k")
    shared = kb if k_layout == v_layout == "fused_qkv" else None
    vb, vv = make_backing_np(v_layout, v_np, "v", backing=shared)
    return (kb, kv), (vb, vv)


# ---------------------------------------------------------------------------------------------
# Case tables of tests/test_strided_inputs.py (shapes: the smallest that reach each kernel path)
# ---------------------------------------------------------------------------------------------
METHODS_A = (
    ("fix_size_l2", dict(fix_kv_size=100, keep_ratio=0.25, strategy="keep_low", skip_layers=[])),
    ("snapkv_lite", dict(observation_window=16, keep_size=100, pooling_kernel=5, skip_layers=[])),
    ("fix_size_l2", dict(fix_kv_size=100, keep_ratio=0.25, strategy="keep_high", skip_layers=[])),
    ("h2o_l2", dict(start_size=4, heavy_hitter_size=40, recent_size=60, skip_layers=[])),
)
# 16-byte chunks per row: 4, 8, 10, 16, 20, 32, 64 (every instance of the copy / score kernels)
WIDTHS_A = ((32, "bf16"), (64, "fp16"), (80, "bf16"), (128, "bf16"), (80, "fp32"), (256, "fp16"),
            (256, "fp32"))
PAIRS_A = (("static", "bshd"), ("fused_qkv", "fused_qkv"), ("head_slice", "batch_slice"))
SHAPE_A = (2, 3, 300)  # B, H, S


def _cases_widths(widths, seed0):
    """Every (row width, layout pair) with two of the four methods each, rotated so that every
    width and every layout pair meets all four."""
    out = []
    for i, (D, dt) in enumerate(widths):
        for j, (kl, vl) in enumerate(PAIRS_A):
            for m in ((i + j) % 4, (i + j + 2) % 4):
                name, kw = METHODS_A[m]
                out.append(dict(id=f"{dt}-D{D}-{kl}-{vl}-{name}{m}", method=name, kw=kw, dtype=dt,
                                k_layout=kl, v_layout=vl, variant=("few", "special")[(i + j) % 2],
                                shapes=[SHAPE_A[:2] + (SHAPE_A[2], D)], seed=seed0 + 10 * i + j))
    return out


CASES_A = _cases_widths(WIDTHS_A, 31000)

# (d) the stable tie policy: the D = 64 and D = 80 16-bit rows
CASES_D = _cases_widths(((64, "bf16"), (64, "fp16"), (80, "bf16")), 34000)

METHODS_B = (
    ("fix_size_l2", dict(fix_kv_size=200, keep_ratio=0.25, skip_layers=[])),
    ("l2_compress", dict(keep_ratio=0.8, prune_after=100, skip_layers=[])),
    ("pyramid_kv", dict(base_size=200, min_size=32, skip_layers=[])),
    ("adaptive_l2", dict(target_size=200, skip_layers=[])),
    ("streaming_llm", dict(start_size=4, recent_size=100, skip_layers=[])),
    ("evict_for_space", dict(num_coming=8, start_size=4, recent_size=100, skip_layers=[])),
    ("recent_only", dict(window_size=50, skip_layers=[])),       # views of the inputs
    ("fix_size_l2", dict(fix_kv_size=1000, skip_layers=[])),     # below the threshold: untouched
)
PAIRS_B = (("static", "bshd", "bf16"), ("fused_qkv", "fused_qkv", "bf16"),
           ("bshd", "head_slice", "bf16"), ("head_slice", "batch_slice", "bf16"),
           ("batch_slice", "expand", "bf16"), ("expand", "static", "bf16"),
           ("row_pad", "row_off", "bf16"), ("row_off", "row_pad", "bf16"),
           ("static", "expand", "fp32"), ("expand", "batch_slice", "fp32"))
CASES_B = [dict(id=f"{dt}-{kl}-{vl}-{name}{m}", method=name, kw=kw, dtype=dt, k_layout=kl,
                v_layout=vl, variant=("few", "special")[(p + m) % 2],
                shapes=[(2, 2, 700, 64), (2, 2, 652, 64)], seed=32000 + 10 * p)
           for p, (kl, vl, dt) in enumerate(PAIRS_B) for m, (name, kw) in enumerate(METHODS_B)]


def _cases_long():
    out = []
    for dt in ("bf16", "fp32"):
        for S, name, kw in (
                # 1 024-thread rows; 2 rows with sink and tail: split-copy workgroups
                (9000, "h2o_l2", dict(start_size=4, heavy_hitter_size=64, recent_size=444,
                                      skip_layers=[])),
                # no fixed rows: unsplit
                (9000, "fix_size_l2", dict(fix_kv_size=512, keep_ratio=0.0, skip_layers=[])),
                # global-scratch select_kernel + gather_kernel
                (20000, "fix_size_l2", dict(fix_kv_size=700, keep_ratio=0.25, skip_layers=[])),
                (20000, "snapkv_lite", dict(observation_window=32, keep_size=20000 // 3,
                                            skip_layers=[])),
                # select_long_kernel
                (65600, "fix_size_l2", dict(fix_kv_size=700, skip_layers=[]))):
            out.append(dict(id=f"{dt}-S{S}-{name}", method=name, kw=kw, dtype=dt,
                            k_layout="static", v_layout="fused_qkv", variant="few",
                            shapes=[(1, 2, S, 64)], seed=33000 + S))
    return out


CASES_C = _cases_long()


def case_inputs(case):
    """[(K, V)] numpy layers of a case (an `expand` side repeats batch 0)."""
    import prng
    layers = []
    for li, shape in enumerate(case["shapes"]):
        k = prng.gen_keys(case["seed"] + li, shape, case["dtype"], case["variant"])
        v = prng.gen_values(case["seed"] + li, shape, case["dtype"])
        if case["k_layout"] == "expand":
            k = expand_input(k)
        if case["v_layout"] == "expand":
            v = expand_input(v)
        layers.append((k, v))
    return layers


# ---------------------------------------------------------------------------------------------
# Attention whose strided q-sum differs from its contiguous copy's (the thread-chunk rule)
# ---------------------------------------------------------------------------------------------
CHUNK_SHAPE, CHUNK_THREADS = (2, 4, 120, 37), 8


def chunk_rule_attention(dt, seed=0):
    """(strided CPU view, its contiguous copy) of tie-heavy attention [2, 4, 120, 37] as a
    batch slice [1::2] of a 5-batch buffer.  At 8 threads torch splits the 37 columns of the
    strided sum over the threads (chunks of 5 columns: the last call covers columns 32..36 with
    the scalar loop) but not those of the contiguous one (B and H coalesce into 8 >= threads), and
    the two sums differ in their bytes -- an input that tells the two chunk rules apart."""
    import torch
    B, H, q, k = CHUNK_SHAPE
    rng = np.random.default_rng(seed)
    logits = rng.integers(0, 4, size=CHUNK_SHAPE).astype(np.float32) * np.float32(0.7)
    a = torch.from_numpy(logits).softmax(dim=-1).to({"fp32": torch.float32, "bf16": torch.bfloat16}[dt])
    backing = torch.full((2 * B + 1, H, q, k), 0.5, dtype=a.dtype)
    view = backing[1::2]
    view.copy_(a)
    return view, a
