"""Shared by tests/test_colsum_edges_gpu.py and tests/test_colsum_abi_gpu.py: the statistics pass's
split arithmetic (csrc/kvc_colsum.h colsum_split, copied so that a change of the heuristics shows
up as a stale case), seeded inputs, and kvc_colsum_layer tables over torch tensors."""
import numpy as np
import torch

from kvcompress import _native as N

HKV = 2
DT = {torch.bfloat16: N.KVC_BF16, torch.float16: N.KVC_F16}


def split(R, q, L):
    """(mb, nqb, tiles, tps, nsplit) of a layer without lse; R = B * Hq."""
    mb = 1 if q <= 32 else 2 if q <= 64 else 4
    nqb, tiles = -(-q // (32 * mb)), -(-L // 128)
    want = min(max(-(-1024 // (R * nqb)), 1), min(32, -(-tiles // 4)))
    tps = -(-tiles // want)
    return mb, nqb, tiles, tps, -(-tiles // tps)


def scratch_bytes(R, q, L):
    """include/kvc.h: the lse rows, then the (max, sum) partials."""
    _, nqb, _, _, nsplit = split(R, q, L)
    return -(-4 * R * q // 256) * 256 + 1024 * R * nqb * nsplit


def randn_inputs(seed, dtype, B, G, L, q, D):
    """K [B, 2, L, D] and Q [B, 2 G, q, D] on the GPU, N(0, 1) rounded to dtype."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(B, HKV, L, D, generator=g).to(dtype).cuda()
    return k, torch.randn(B, HKV * G, q, D, generator=g).to(dtype).cuda()


def table(ks, qs, lses=None, f32=None, dts=None, out_stride=None):
    """COLSUM_LAYER_DTYPE rows as kvcompress.methods.colsum fills them; out_stride defaults to L."""
    t = np.zeros(len(ks), dtype=N.COLSUM_LAYER_DTYPE)
    for i, (k, q) in enumerate(zip(ks, qs)):
        L = k.shape[2]
        t[i] = (k.data_ptr(), k.stride()[:3], q.data_ptr(), q.stride()[:3],
                lses[i].data_ptr() if lses and lses[i] is not None else 0,
                f32[i].data_ptr() if f32 else 0, dts[i].data_ptr() if dts else 0,
                out_stride[i] if out_stride else L, L, q.shape[2], 0)
    return t


def params(k, q, scale=0.0):
    return N.ColsumParams(dtype=DT[k.dtype], batch=k.shape[0], heads=k.shape[1],
                          q_heads=q.shape[1], head_dim=k.shape[3], scale=scale)
