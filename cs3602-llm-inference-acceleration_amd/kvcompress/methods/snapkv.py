"""SnapKV: prefix keys ranked by how much the observation window's queries attend to them.

An extension (the reference has only the norm-based stand-in, kvcompress/methods/snapkv_lite.py):
`snapkv_lite` ranks by key norms because attention weights exist only under eager attention;
the real ranking needs no attention tensor, only the last W post-RoPE queries of every layer.
The score -- softmax(Q_obs K^T) summed over the window's queries and the KV head's query group,
pooled -- runs on the MFMA units (csrc/kvc_observe.h, kvc_observe_score in include/kvc.h) and
lands where the engine's SELECT reads plain-norm scores, so selection and copy are the engine's
usual kernels.  Numerical, not bit-exact: there is no reference implementation to match.
"""
from typing import List, Optional, Tuple

import numpy as np
import torch

from .. import _engine as E
from .. import _native as N
from ..utils import layer_offset, normalize_kv_cache

_POOLING = {"avg": N.OBS_POOL_AVG, "max": N.OBS_POOL_MAX}
_DTYPES = (torch.bfloat16, torch.float16)


def _check_layer(j: E.Segments, q, W):
    """The layer's K/V under the engine's contract and its queries under kvc_observe_score's;
    returns (B, Hkv, D, Hq, queries as the kernels read them)."""
    B, H, S, D = E._check_tensors(j)
    li = j.layer_idx
    if j.keys.dtype not in _DTYPES:
        raise TypeError(f"kvcompress (MI355X HIP engine): observation-window scores take bfloat16 "
                        f"or float16 K/V (the matrix path); layer {li} has {j.keys.dtype}")
    if not isinstance(q, torch.Tensor):
        raise TypeError(f"layer {li}: queries must be a [B, Hq, W, D] tensor, got "
                        f"{type(q).__name__}")
    if q.dim() != 4 or q.shape[0] != B or q.shape[2] != W or q.shape[3] != D or \
            q.shape[1] % H:
        raise ValueError(f"layer {li}: queries must be [B={B}, G*{H}, W={W}, D={D}]; got "
                         f"{tuple(q.shape)}")
    if q.dtype != j.keys.dtype or q.device != j.keys.device:
        raise TypeError(f"layer {li}: queries are {q.dtype} on {q.device}, K is {j.keys.dtype} "
                        f"on {j.keys.device}")
    if not E._takes_as_is(q):  # a window of queries is small: copy what the kernels cannot read
        q = q.clone(memory_format=torch.contiguous_format)
    return B, H, D, q.shape[1], q


def _run_group(device, dtype, B, H, D, Hq, js, qs, W, pool, mode, scale, order_algo, want_f32):
    """Plan, observe-score and (for compressing jobs) SELECT | GATHER one group; returns the
    outputs and, with want_f32, the fp32 score rows [layers * B * H, stride]."""
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device)
        p = E._params(dtype, B, H, D, *order_algo, False)
        table, kos, vos, keep = E._build_table(device, dtype, B, H, D, js)
        rc, info = N.plan(p, table)
        N.check(rc, "kvc_plan")
        otable = np.zeros(len(js), dtype=N.OBSERVE_LAYER_DTYPE)
        for i, q in enumerate(qs):
            otable[i] = (q.data_ptr(), q.stride()[:3], 0)
        fstride = (max(j.zone_len for j in js) + 63) // 64 * 64
        op = N.ObserveParams(q_heads=Hq, window=W, scale=scale or 0.0, pool_kernel=pool,
                             pool_mode=mode, scores_row_stride=fstride)
        rc, sbytes = N.observe_plan(p, op, table, otable)
        N.check(rc, "kvc_observe_plan")
        dev = torch.device("cuda", device)
        ws = torch.empty(max(int(info.workspace_bytes), 256), dtype=torch.uint8, device=dev)
        scratch = torch.empty(max(sbytes, 256), dtype=torch.uint8, device=dev)
        f32 = torch.empty((len(js) * B * H, fstride), dtype=torch.float32, device=dev) \
            if want_f32 else None
        rc = N.observe_score(p, op, table, otable, ws.data_ptr(), int(info.workspace_bytes),
                             scratch.data_ptr(), sbytes, f32.data_ptr() if want_f32 else None,
                             stream.cuda_stream)
        N.check(rc, "kvc_observe_score")
        E._launch(p, table, ws, info, stream, N.PHASE_SELECT | N.PHASE_GATHER)
        del keep
    return kos, vos, f32


def observation_scores(keys, queries, *, zone=(0, None), pooling_kernel: int = 1,
                       pooling: str = "avg", scale: Optional[float] = None):
    """The un-rounded fp32 scores of one layer: float32 [B, Hkv, zone_len] for keys
    [B, Hkv, S, D], queries [B, Hq, W, D] (the last W positions' post-RoPE queries, Hq = G * Hkv)
    and zone = (start, stop) inside the prefix [0, S - W) (stop None: S - W).  Lists of keys and
    queries (layers of one B, Hkv, Hq, W, D) are scored in one launch set and give a list."""
    if pooling not in _POOLING:
        raise ValueError(f"pooling={pooling!r}: expected 'avg' or 'max'")
    many = isinstance(keys, (list, tuple))
    ks, qs = (list(keys), list(queries)) if many else ([keys], [queries])
    W = qs[0].size(2) if isinstance(qs[0], torch.Tensor) else 0
    jobs, checked = [], []
    for i, (k, q) in enumerate(zip(ks, qs)):
        z0, zl = E.py_slice(max(k.size(2) - W, 0), zone[0], zone[1])
        jobs.append(E.Segments(i, k, k, zone_start=z0, zone_len=zl))
        checked.append(_check_layer(jobs[-1], q, W))
    if len({c[:4] for c in checked}) != 1 or len({k.device for k in ks}) != 1:
        raise ValueError("observation_scores: the layers of one call share B, Hkv, D, Hq and device")
    B, H, D, Hq, _ = checked[0]
    if all(j.zone_len == 0 for j in jobs):
        out = [torch.empty((B, H, 0), dtype=torch.float32, device=k.device) for k in ks]
    else:
        _, _, f32 = _run_group(ks[0].get_device(), ks[0].dtype, B, H, D, Hq, jobs,
                               [c[4] for c in checked], W, pooling_kernel, _POOLING[pooling],
                               scale, (N.KVC_DESC, N.KVC_ALGO_TOPK), True)
        f32 = f32.view(len(jobs), B, H, -1)
        out = [f32[i, :, :, :j.zone_len] for i, j in enumerate(jobs)]
    return out if many else out[0]


def _snapkv(past_key_values, queries, observation_window, keep_size, pooling_kernel, pooling,
            sink_size, skip_layers, kwargs) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    past_key_values = list(normalize_kv_cache(past_key_values))
    offset = layer_offset(kwargs)  # global index of layer 0 (layer-sharded callers)
    if not past_key_values:
        return past_key_values
    if pooling not in _POOLING:
        raise ValueError(f"pooling={pooling!r}: expected 'avg' or 'max'")
    if len(queries) != len(past_key_values):
        raise ValueError(f"queries has {len(queries)} entries for {len(past_key_values)} layers")
    jobs = []
    for layer_idx, (keys, values) in enumerate(past_key_values):
        seq_len = keys.size(2)
        if seq_len <= keep_size:
            continue
        if layer_idx + offset in skip_layers or queries[layer_idx] is None:
            continue
        prefix_len = seq_len - observation_window
        if prefix_len <= 0:
            continue
        o0, ol = E.py_slice(seq_len, -observation_window)
        num_prefix_to_keep = min(keep_size - observation_window, prefix_len)
        if num_prefix_to_keep <= 0:  # (views, as snapkv_lite)
            past_key_values[layer_idx] = (keys[:, :, -observation_window:, :],
                                          values[:, :, -observation_window:, :])
            continue
        sink = min(max(sink_size, 0), num_prefix_to_keep)  # sinks count against the prefix budget
        jobs.append(E.Segments(layer_idx, keys, values, sink_len=sink, zone_start=sink,
                               zone_len=prefix_len - sink, n_select=num_prefix_to_keep - sink,
                               tail_start=o0, tail_len=ol))
    algo = N.KVC_ALGO_STABLE if E.tie_policy == "stable" else N.KVC_ALGO_TOPK
    groups = {}
    for j in jobs:
        if E.tie_policy == "stable" and 0 < j.n_select < j.zone_len > E.STABLE_MAX_ZONE:
            raise ValueError(f"kvcompress: the stable tie policy selects from zones of at most "
                             f"{E.STABLE_MAX_ZONE} positions (layer {j.layer_idx}: {j.zone_len})")
        B, H, D, Hq, q = _check_layer(j, queries[j.layer_idx], observation_window)
        groups.setdefault((j.keys.get_device(), j.keys.dtype, B, H, D, Hq), ([], []))
        groups[(j.keys.get_device(), j.keys.dtype, B, H, D, Hq)][0].append(j)
        groups[(j.keys.get_device(), j.keys.dtype, B, H, D, Hq)][1].append(q)
    for (device, dtype, B, H, D, Hq), (js, qs) in groups.items():
        kos, vos, _ = _run_group(device, dtype, B, H, D, Hq, js, qs, observation_window,
                                 pooling_kernel, _POOLING[pooling], None, (N.KVC_DESC, algo), False)
        for j, ko, vo in zip(js, kos, vos):
            past_key_values[j.layer_idx] = (ko, vo)
    return past_key_values


def snapkv_compress(past_key_values, queries, observation_window: int = 32, keep_size: int = 512,
                    pooling_kernel: int = 5, pooling: str = "avg", sink_size: int = 0,
                    skip_layers: List[int] = [], **kwargs
                    ) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """SnapKV over a list of (K, V): every compressed layer becomes
    sink ++ prefix[top-k by observation-window score, per KV head] ++ window, keep_size positions
    in all (snapkv_lite's size arithmetic and early returns).  `queries`: one [B, Hq, W, D] tensor
    per layer (None passes the layer through), the post-RoPE queries of the last
    W = observation_window positions.  Not in the method registry: a registry caller has no
    queries to pass."""
    if kwargs.pop("out", None) is not None:
        raise NotImplementedError("snapkv_compress does not take `out` (destinations) yet")
    if past_key_values is None or queries is None:
        raise TypeError("snapkv_compress needs past_key_values and one query tensor per layer")
    return E._checked_call(
        lambda: _snapkv(past_key_values, list(queries), observation_window, keep_size,
                        pooling_kernel, pooling, sink_size, skip_layers, kwargs),
        E._output_devices)


__all__ = ["observation_scores", "snapkv_compress"]
