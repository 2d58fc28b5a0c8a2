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
from ..paged import PagedKV, _claim_pools, _launch_rows
from ..utils import layer_offset, normalize_kv_cache

_POOLING = {"avg": N.OBS_POOL_AVG, "max": N.OBS_POOL_MAX}
_DTYPES = (torch.bfloat16, torch.float16)


def _check_queries(li, q, kdtype, device, B, H, W, D):
    """Layer li's queries under kvc_observe_score's contract, for K of `kdtype` [B, H, S, D] on
    `device`; returns (Hq, queries as the kernels read them).  fp8 keys take bfloat16 queries."""
    if kdtype not in _DTYPES and not E.is_fp8(kdtype):
        raise TypeError(f"kvcompress (MI355X HIP engine): observation-window scores take bfloat16, "
                        f"float16 or fp8 (float8_e4m3fn / float8_e5m2) K/V (the matrix path); "
                        f"layer {li} has {kdtype}")
    if not isinstance(q, torch.Tensor):
        raise TypeError(f"layer {li}: queries must be a [B, Hq, W, D] tensor, got "
                        f"{type(q).__name__}")
    if q.dim() != 4 or q.shape[0] != B or q.shape[2] != W or q.shape[3] != D or \
            q.shape[1] % H:
        raise ValueError(f"layer {li}: queries must be [B={B}, G*{H}, W={W}, D={D}]; got "
                         f"{tuple(q.shape)}")
    qdtype = torch.bfloat16 if E.is_fp8(kdtype) else kdtype
    if q.dtype != qdtype or q.device != device:
        raise TypeError(f"layer {li}: queries are {q.dtype} on {q.device}, K is {kdtype} on "
                        f"{device}" + (" (fp8 keys are scored as bfloat16: queries must be "
                                       "bfloat16)" if E.is_fp8(kdtype) else ""))
    if not E._takes_as_is(q):  # a window of queries is small: copy what the kernels cannot read
        q = q.clone(memory_format=torch.contiguous_format)
    return q.shape[1], q


def _check_layer(j: E.Segments, q, W):
    """The layer's K/V under the engine's contract and its queries under kvc_observe_score's;
    returns (B, Hkv, D, Hq, queries as the kernels read them)."""
    B, H, S, D = E._check_tensors(j)
    Hq, q = _check_queries(j.layer_idx, q, j.keys.dtype, j.keys.device, B, H, W, D)
    return B, H, D, Hq, q


def _check_paged(li, pk, who):
    """A PagedKV the observe kernels can score: one length, no scales."""
    if pk.ragged:
        raise TypeError(f"{who}: layer {li} is a ragged PagedKV (a length per sequence); "
                        "observation-window scores take single-length paged layers")
    if pk.scaled:
        raise TypeError(f"{who}: layer {li} carries k_scale / v_scale; a per-token scale "
                        "multiplies the logit and has no channel in the observe kernels yet")


def _paged_table(pks, segs):
    """(layer table, N.Tables) of paged layers compacted in place, with the segment fields of
    `segs`: (zone_start, zone_len, n_select, sink_len, tail_start, tail_len) per layer."""
    table, rows = _launch_rows([(pk, None) for pk in pks])
    for t, pk, (z0, zl, ns, sink, t0, tl) in zip(table, pks, segs):
        t["seq_len"], t["zone_start"], t["zone_len"] = pk.seq_len, z0, zl
        t["n_select"], t["sink_len"], t["tail_start"], t["tail_len"] = ns, sink, t0, tl
        t["score_mode"] = N.KVC_SCORE_NORM
    return table, N.Tables(**rows)


class _Group:
    """One planned launch set: kvc_plan (or kvc_plan_paged), the observe plan, workspace and
    scratch -- everything that can fail before a kernel runs.  launch() enqueues the observe
    kernels and SELECT | GATHER on the current stream."""

    def __init__(self, device, dtype, B, H, D, Hq, table, tables, qs, W, pool, mode, scale,
                 order_algo, want_f32):
        self.device, self.table, self.tables = device, table, tables
        with torch.cuda.device(device):
            self.p = p = E._params(dtype, B, H, D, *order_algo, False)
            self.ws, self.info = E._upload(p, table, device, None, B, H, tables)
            self.otable = np.zeros(len(table), dtype=N.OBSERVE_LAYER_DTYPE)
            for i, q in enumerate(qs):
                self.otable[i] = (q.data_ptr(), q.stride()[:3], 0)
            self.qs = qs  # (prepared copies stay alive until the launch)
            fstride = (int(table["zone_len"].max()) + 63) // 64 * 64
            self.op = N.ObserveParams(q_heads=Hq, window=W, scale=scale or 0.0, pool_kernel=pool,
                                      pool_mode=mode, scores_row_stride=fstride)
            G = Hq // H
            if G > 16 or G * W > 256:
                raise ValueError(f"kvcompress: observation-window scores take query groups of "
                                 f"G <= 16 heads per KV head with G * window <= 256; got G = {G} "
                                 f"(Hq = {Hq}, Hkv = {H}) at window {W}")
            # dense 16-bit keys keep their entry pair where it admits the group (G a power of two,
            # G * W <= 128); pages, fp8 keys and every other group take the _paged pair
            self.pages = tables.pages if tables is not None else None
            self.paged_entry = self.pages is not None or E.is_fp8(dtype) or \
                G not in (1, 2, 4, 8) or G * W > 128
            if self.paged_entry:
                rc, self.sbytes = N.observe_plan_paged(p, self.op, table, self.otable, self.pages)
                N.check(rc, "kvc_observe_plan_paged")
            else:
                rc, self.sbytes = N.observe_plan(p, self.op, table, self.otable)
                N.check(rc, "kvc_observe_plan")
            dev = torch.device("cuda", device)
            self.scratch = torch.empty(max(self.sbytes, 256), dtype=torch.uint8, device=dev)
            self.f32 = torch.empty((len(table) * B * H, fstride), dtype=torch.float32,
                                   device=dev) if want_f32 else None

    def launch(self):
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            args = (self.ws.data_ptr(), int(self.info.workspace_bytes), self.scratch.data_ptr(),
                    self.sbytes, self.f32.data_ptr() if self.f32 is not None else None,
                    stream.cuda_stream)
            if self.paged_entry:
                N.check(N.observe_score_paged(self.p, self.op, self.table, self.otable,
                                              self.pages, *args), "kvc_observe_score_paged")
            else:
                N.check(N.observe_score(self.p, self.op, self.table, self.otable, *args),
                        "kvc_observe_score")
            E._launch(self.p, self.table, self.ws, self.info, stream,
                      N.PHASE_SELECT | N.PHASE_GATHER, self.tables)
        return self.f32


def _run_group(device, dtype, B, H, D, Hq, js, qs, W, pool, mode, scale, order_algo, want_f32):
    """Plan, observe-score and (for compressing jobs) SELECT | GATHER one group of dense layers;
    returns the outputs and, with want_f32, the fp32 score rows [layers * B * H, stride]."""
    with torch.cuda.device(device):
        table, kos, vos, keep = E._build_table(device, dtype, B, H, D, js)
    f32 = _Group(device, dtype, B, H, D, Hq, table, None, qs, W, pool, mode, scale, order_algo,
                 want_f32).launch()
    del keep
    return kos, vos, f32


def observation_scores(keys, queries, *, zone=(0, None), pooling_kernel: int = 1,
                       pooling: str = "avg", scale: Optional[float] = None):
    """The un-rounded fp32 scores of one layer: float32 [B, Hkv, zone_len] for keys
    [B, Hkv, S, D], queries [B, Hq, W, D] (the last W positions' post-RoPE queries, Hq = G * Hkv)
    and zone = (start, stop) inside the prefix [0, S - W) (stop None: S - W).  Lists of keys and
    queries (layers of one B, Hkv, Hq, W, D) are scored in one launch set and give a list.

    `keys` may be fp8 (float8_e4m3fn / float8_e5m2) with bfloat16 queries: the scores are those of
    keys.to(bfloat16), bit for bit.  In place of a key tensor a single-length PagedKV without
    scales is scored through its block table (all layers of a call paged, or none): the scores
    are those of the dense tensor the table describes, bit for bit."""
    if pooling not in _POOLING:
        raise ValueError(f"pooling={pooling!r}: expected 'avg' or 'max'")
    many = isinstance(keys, (list, tuple))
    ks, qs = (list(keys), list(queries)) if many else ([keys], [queries])
    W = qs[0].size(2) if isinstance(qs[0], torch.Tensor) else 0
    paged = any(isinstance(k, PagedKV) for k in ks)
    if paged and not all(isinstance(k, PagedKV) for k in ks):
        raise TypeError("observation_scores: the layers of one call are all PagedKV or all tensors")
    jobs, checked, segs = [], [], []
    for i, (k, q) in enumerate(zip(ks, qs)):
        if paged:
            _check_paged(i, k, "observation_scores")
            B, H, S, D = k.shape
            z0, zl = E.py_slice(max(S - W, 0), zone[0], zone[1])
            segs.append((z0, zl, 0, 0, 0, 0))
            checked.append((B, H, D) + _check_queries(i, q, k.k_pool.dtype, k.k_pool.device,
                                                      B, H, W, D))
            continue
        z0, zl = E.py_slice(max(k.size(2) - W, 0), zone[0], zone[1])
        jobs.append(E.Segments(i, k, k, zone_start=z0, zone_len=zl))
        segs.append((z0, zl, 0, 0, 0, 0))
        checked.append(_check_layer(jobs[-1], q, W))
    dev_of = (lambda k: k.k_pool.device) if paged else (lambda k: k.device)
    dt_of = (lambda k: k.k_pool.dtype) if paged else (lambda k: k.dtype)
    if len({c[:4] for c in checked}) != 1 or len({(dev_of(k), dt_of(k)) for k in ks}) != 1:
        raise ValueError("observation_scores: the layers of one call share B, Hkv, D, Hq, dtype "
                         "and device")
    B, H, D, Hq, _ = checked[0]
    device, dtype = dev_of(ks[0]), dt_of(ks[0])
    if all(zl == 0 for _, zl, *_ in segs):
        out = [torch.empty((B, H, 0), dtype=torch.float32, device=device) for k in ks]
    else:
        args = ([c[4] for c in checked], W, pooling_kernel, _POOLING[pooling], scale,
                (N.KVC_DESC, N.KVC_ALGO_TOPK), True)
        if paged:
            table, tables = _paged_table(ks, segs)
            f32 = _Group(device.index, dtype, B, H, D, Hq, table, tables, *args).launch()
        else:
            _, _, f32 = _run_group(device.index, dtype, B, H, D, Hq, jobs, *args)
        f32 = f32.view(len(ks), B, H, -1)
        out = [f32[i, :, :, :zl] for i, (_, zl, *_) in enumerate(segs)]
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


def _snapkv_paged(layers, queries, W, keep_size, pooling_kernel, pooling, sink_size, skip_layers,
                  kwargs):
    offset = layer_offset(kwargs)
    if pooling not in _POOLING:
        raise ValueError(f"pooling={pooling!r}: expected 'avg' or 'max'")
    if len(queries) != len(layers):
        raise ValueError(f"queries has {len(queries)} entries for {len(layers)} layers")
    result = [pk.seq_len for pk in layers]
    algo = N.KVC_ALGO_STABLE if E.tie_policy == "stable" else N.KVC_ALGO_TOPK
    groups, seen = {}, {}
    for li, pk in enumerate(layers):  # snapkv_compress's size arithmetic and early returns
        S = pk.seq_len
        if S <= keep_size or li + offset in skip_layers or queries[li] is None or S - W <= 0:
            continue
        prefix_len, keep = S - W, min(keep_size - W, S - W)
        # keep <= 0: the window alone (snapkv_lite's views), here a copy into the leading pages
        sink = min(max(sink_size, 0), max(keep, 0))
        seg = (sink, prefix_len - sink, keep - sink, sink, S - W, W) if keep > 0 else \
            (0, 0, 0, 0, S - W, W)
        if E.tie_policy == "stable" and 0 < seg[2] < seg[1] > E.STABLE_MAX_ZONE:
            raise ValueError(f"kvcompress: the stable tie policy selects from zones of at most "
                             f"{E.STABLE_MAX_ZONE} positions (layer {li}: {seg[1]})")
        B, H, _, D = pk.shape
        Hq, q = _check_queries(li, queries[li], pk.k_pool.dtype, pk.k_pool.device, B, H, W, D)
        _claim_pools(seen, li, pk)
        g = groups.setdefault((pk.k_pool.get_device(), pk.k_pool.dtype, B, H, D, Hq),
                              ([], [], [], []))
        for lst, x in zip(g, (li, pk, seg, q)):
            lst.append(x)
    planned = []
    for (device, dtype, B, H, D, Hq), (lis, pks, segs, qs) in groups.items():  # plan (and check)
        table, tables = _paged_table(pks, segs)
        planned.append(_Group(device, dtype, B, H, D, Hq, table, tables, qs, W, pooling_kernel,
                              _POOLING[pooling], None, (N.KVC_DESC, algo), False))
        for li, seg in zip(lis, segs):
            result[li] = seg[3] + seg[2] + seg[5]
    for g in planned:
        g.launch()
    return result


def snapkv_compress_paged(layers, queries, observation_window: int = 32, keep_size: int = 512,
                          pooling_kernel: int = 5, pooling: str = "avg", sink_size: int = 0,
                          skip_layers: List[int] = [], **kwargs) -> List[int]:
    """snapkv_compress on `layers`, a list of single-length PagedKV without scales: every
    compressed layer is scored through its block table (kvc_observe_score_paged) and compacted
    into the leading pages of its sequences (kvc_launch_paged, in place), with no dense copy of
    the cache at any point.  Returns the list of new logical lengths; a layer that passes through
    returns its seq_len, and the caller frees the pages from ceil(n / page_size) on.  fp8 pools
    take bfloat16 queries and keep their bytes.  Everything is checked before anything launches:
    an error leaves every pool untouched."""
    if kwargs.pop("out", "inplace") != "inplace":
        raise NotImplementedError("snapkv_compress_paged compacts in place only (out=\"inplace\"): "
                                  "PagedDest and dense destinations are not supported yet")
    if not isinstance(layers, (list, tuple)) or not all(isinstance(x, PagedKV) for x in layers):
        raise TypeError("snapkv_compress_paged: layers must be a list of PagedKV")
    if queries is None:
        raise TypeError("snapkv_compress_paged needs one query tensor per layer")
    for li, pk in enumerate(layers):
        _check_paged(li, pk, "snapkv_compress_paged")
    return E._checked_call(
        lambda: _snapkv_paged(list(layers), list(queries), observation_window, keep_size,
                              pooling_kernel, pooling, sink_size, skip_layers, kwargs))


__all__ = ["observation_scores", "snapkv_compress", "snapkv_compress_paged"]
