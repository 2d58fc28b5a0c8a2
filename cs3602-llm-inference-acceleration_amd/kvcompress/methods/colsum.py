"""Causal attention column sums: what `attentions[i].sum(dim=2)` would be, without the tensor.

An extension (the reference's H2OAttentionManager takes materialised attention only, which no
flash-attention forward returns): for the last q positions' post-RoPE queries [B, Hq, q, D] and the
layer's keys [B, Hkv, L, D] the MFMA kernels of csrc/kvc_colsum.h (kvc_colsum_score in
include/kvc.h) recompute softmax(Q K^T) under the causal mask and sum it over the queries, for any
1 <= q <= L.  Numerical, not bit-exact: there is no reference implementation to match.
"""
import numpy as np
import torch

from .. import _engine as E
from .. import _native as N

_DT = {torch.bfloat16: N.KVC_BF16, torch.float16: N.KVC_F16}
_WHO = "kvcompress (MI355X HIP engine): attention column sums"


def _check_layer(li, k, q, lse):
    """Layer li under kvc_colsum_score's contract: (B, Hkv, Hq, D, L, q_len)."""
    for what, t in (("keys", k), ("queries", q)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise TypeError(f"{_WHO}: layer {li}: {what} must be a 4-D tensor, got "
                            f"{type(t).__name__}")
    if k.dtype not in _DT:
        raise TypeError(f"{_WHO} take bfloat16 or float16 keys (the matrix path); layer {li} "
                        f"has {k.dtype}")
    if q.dtype != k.dtype or q.device != k.device:
        raise TypeError(f"{_WHO}: layer {li}: queries are {q.dtype} on {q.device}, keys "
                        f"{k.dtype} on {k.device}")
    (B, H, L, D), (Bq, Hq, ql, Dq) = k.shape, q.shape
    if Bq != B or Dq != D or Hq % H or not 1 <= ql <= L:
        raise ValueError(f"{_WHO}: layer {li}: queries must be [B={B}, G*{H}, 1..{L}, D={D}]; "
                         f"got {tuple(q.shape)}")
    if lse is not None:
        if not isinstance(lse, torch.Tensor) or tuple(lse.shape) != (B, Hq, ql) or \
                lse.device != k.device or not lse.is_floating_point():
            raise ValueError(f"{_WHO}: layer {li}: lse must be a floating [B={B}, Hq={Hq}, "
                             f"q={ql}] tensor on {k.device}")
    return B, H, Hq, D, L, ql


def column_sums(keys, queries, lses, scale, want_f32, want_dt):
    """One launch set over layers that share B, Hkv, Hq, D, dtype and device: (list of float32
    [B, Hq, L] or None, list of K-dtype [B, Hq, L] or None).  Everything is checked, planned and
    allocated before a kernel is enqueued (on the current stream)."""
    if len(queries) != len(keys) or len(lses) != len(keys):
        raise ValueError(f"{_WHO}: {len(keys)} key layers, {len(queries)} query layers, "
                         f"{len(lses)} lse entries")
    shapes = [_check_layer(i, k, q, l) for i, (k, q, l) in enumerate(zip(keys, queries, lses))]
    if not shapes:
        return ([] if want_f32 else None), ([] if want_dt else None)
    if len({s[:4] for s in shapes}) != 1 or len({(k.device, k.dtype) for k in keys}) != 1:
        raise ValueError(f"{_WHO}: the layers of one call share B, Hkv, Hq, D, dtype and device")
    B, H, Hq, D = shapes[0][:4]
    device, dtype = keys[0].device, keys[0].dtype
    if not keys[0].is_cuda:
        raise RuntimeError(f"{_WHO}: keys and queries are on {device}; the kernels run on ROCm "
                           "GPU tensors only (no CPU fallback).")
    with torch.cuda.device(device):
        # (copies of what the kernels cannot read as it lies stay alive until the launch)
        ks = [k if E._takes_as_is(k) else k.contiguous() for k in keys]
        qs = [q if E._takes_as_is(q) else q.contiguous() for q in queries]
        ls = [None if l is None else l.to(torch.float32).contiguous() for l in lses]
        f32 = [torch.empty((B, Hq, s[4]), dtype=torch.float32, device=device) for s in shapes] \
            if want_f32 else None
        dts = [torch.empty((B, Hq, s[4]), dtype=dtype, device=device) for s in shapes] \
            if want_dt else None
        table = np.zeros(len(ks), dtype=N.COLSUM_LAYER_DTYPE)
        for i, (k, q, l, s) in enumerate(zip(ks, qs, ls, shapes)):
            table[i] = (k.data_ptr(), k.stride()[:3], q.data_ptr(), q.stride()[:3],
                        l.data_ptr() if l is not None else 0,
                        f32[i].data_ptr() if want_f32 else 0, dts[i].data_ptr() if want_dt else 0,
                        s[4], s[4], s[5], 0)
        p = N.ColsumParams(dtype=_DT[dtype], batch=B, heads=H, q_heads=Hq, head_dim=D,
                           scale=scale or 0.0)
        rc, nbytes = N.colsum_plan(p, table)
        N.check(rc, "kvc_colsum_plan")
        scratch = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
        rc = N.colsum_score(p, table, scratch.data_ptr(), nbytes,
                            torch.cuda.current_stream(device).cuda_stream)
        N.check(rc, "kvc_colsum_score")
        del ks, qs, ls, scratch  # (the caching allocator keeps them until the stream has run)
    return f32, dts


def attention_column_sums(keys, queries, *, lse=None, scale=None):
    """float32 [B, Hq, L]: imp[b, hq, j] = sum_i softmax(scale * Q K^T, causal)[b, hq, i, j] for
    keys [B, Hkv, L, D] and queries [B, Hq, q, D], the post-RoPE queries of the LAST q positions
    (1 <= q <= L, Hq = G * Hkv with G <= 16, D in 64 / 80 / 128 / 256, bfloat16 or float16).
    `lse` (optional, [B, Hq, q]): the natural-log-sum-exp of every query row's scaled, masked
    logits, as flash-attention forwards return it; with it K is read once.  `scale` defaults to
    1/sqrt(D).  Lists of layers that share B, Hkv, Hq, D, dtype and device (q and L may differ)
    run as one launch set and give a list."""
    many = isinstance(keys, (list, tuple))
    ks, qs = (list(keys), list(queries)) if many else ([keys], [queries])
    ls = [None] * len(ks) if lse is None else (list(lse) if many else [lse])
    out, _ = column_sums(ks, qs, ls, scale, True, False)
    return out if many else out[0]


__all__ = ["attention_column_sums"]
