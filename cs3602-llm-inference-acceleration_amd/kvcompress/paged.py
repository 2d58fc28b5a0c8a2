"""Compression of paged KV caches (include/kvc.h, "Paged caches").

A serving stack keeps K / V in a page pool addressed through a per-sequence block table.
`PagedKV` describes one layer of such a cache; `compress_paged` runs any compress method on a
list of them WITHOUT gathering the cache into a dense tensor: the engine's SCORE and GATHER kernels
read the rows through the table, and by default the kept rows are compacted into each sequence's
leading pages, so that the caller can free the pages behind them.

The method's own Python runs over stand-in tensors of every layer's shape (nothing proportional
to the cache is allocated; the methods only read shapes), inside the deferred-call context of
the `out` kwarg (_engine.dest_call): every job it records is checked, mapped onto its PagedKV and
only then launched with kvc_launch_paged.  No plan cache, no call memo.
"""
import numpy as np
import torch

from . import _engine as E
from . import _native as N


class PagedKV:
    """One layer of a paged cache: pools `[num_pages, H, page_size, D]` (views of any strides
    with a contiguous last dim and 16-byte aligned pointers and strides; never copied), an int32
    `block_table` [B, >= ceil(seq_len / page_size)] on the same device, and the common logical
    length `seq_len` of its B sequences.  vLLM's [N, P, H, D] cache is `cache.permute(0, 2, 1, 3)`;
    the halves of a fused [2, N, ...] buffer are `kv[0]` and `kv[1]`."""
    __slots__ = ("k_pool", "v_pool", "block_table", "seq_len")

    def __init__(self, k_pool, v_pool, block_table, seq_len):
        for name, t in (("k_pool", k_pool), ("v_pool", v_pool), ("block_table", block_table)):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"PagedKV: {name} must be a tensor, got {type(t).__name__}")
        if k_pool.dim() != 4 or v_pool.shape != k_pool.shape:
            raise ValueError("PagedKV: k_pool / v_pool must both be [num_pages, H, page_size, D]; "
                             f"got {tuple(k_pool.shape)} / {tuple(v_pool.shape)}")
        if k_pool.dtype not in E._SUPPORTED or v_pool.dtype != k_pool.dtype:
            raise ValueError("PagedKV: pools must be bfloat16 / float16 / float32 and of one "
                             f"dtype; got {k_pool.dtype} / {v_pool.dtype}")
        npg, H, P, D = k_pool.shape
        if npg < 1 or H < 1 or D < 1 or P < 1 or P > 65536 or P & (P - 1):
            raise ValueError(f"PagedKV: page_size must be a power of two in [1, 65536] and the "
                             f"pool non-empty; got pools of shape {tuple(k_pool.shape)}")
        if isinstance(seq_len, bool) or not isinstance(seq_len, int) or seq_len < 0:
            raise ValueError(f"PagedKV: seq_len must be a non-negative int, got {seq_len!r}")
        es = k_pool.element_size()
        for name, t in (("k_pool", k_pool), ("v_pool", v_pool)):
            if (t.stride(3) != 1 and D > 1) or (D * es) % 16 or any(
                    (t.stride(d) * es) % 16 and t.size(d) > 1 for d in range(3)):
                raise ValueError(f"PagedKV: {name} needs a contiguous last dim and rows and "
                                 f"strides that are multiples of 16 bytes (a pool is never "
                                 f"copied); strides {tuple(t.stride())}")
            if any(t.stride(d) == 0 and t.size(d) > 1 for d in range(3)):
                raise ValueError(f"PagedKV: {name} has stride 0 on a dim larger than 1")
        if block_table.dtype != torch.int32 or block_table.dim() != 2 or \
                (block_table.stride(1) != 1 and block_table.size(1) > 1):
            raise ValueError("PagedKV: block_table must be an int32 [B, pages per sequence] "
                             "tensor with a contiguous last dim; got "
                             f"{block_table.dtype} {tuple(block_table.shape)}")
        need = -(-seq_len // P)
        if block_table.size(0) < 1 or block_table.size(1) < need:
            raise ValueError(f"PagedKV: block_table {tuple(block_table.shape)} holds fewer than "
                             f"the {need} pages of {seq_len} rows of {P}")
        if not (k_pool.is_cuda and v_pool.is_cuda and block_table.is_cuda) or \
                not (k_pool.device == v_pool.device == block_table.device):
            raise ValueError("PagedKV: pools and block table must be on one ROCm device (no CPU "
                             f"fallback); got {k_pool.device} / {v_pool.device} / "
                             f"{block_table.device}")
        for name, t in (("k_pool", k_pool), ("v_pool", v_pool)):
            if t.data_ptr() % 16:
                raise ValueError(f"PagedKV: {name} pointer not 16-byte aligned (a pool is never "
                                 "copied)")
        self.k_pool, self.v_pool, self.block_table, self.seq_len = k_pool, v_pool, block_table, \
            seq_len

    @property
    def shape(self):
        """The [B, H, seq_len, D] of the dense tensors the table describes."""
        return (self.block_table.size(0), self.k_pool.size(1), self.seq_len, self.k_pool.size(3))

    @property
    def page_size(self):
        return self.k_pool.size(2)

    def to_dense(self, n=None):
        """(K, V) [B, H, n, D] of the first n (default seq_len) logical rows, by torch indexing:
        a convenience for tests and debugging, not on the hot path."""
        n = self.seq_len if n is None else n
        pos = torch.arange(n, device=self.k_pool.device)
        pg = self.block_table[:, :max(-(-n // self.page_size), 1)].long()
        pg = pg[:, pos // self.page_size]            # [B, n] page of every row
        slot = pos % self.page_size                  # [n]
        return tuple(pool[pg, :, slot].permute(0, 2, 1, 3) for pool in (self.k_pool, self.v_pool))


def _resolve(method):
    if callable(method):
        return method
    if not isinstance(method, str):
        raise TypeError(f"compress_paged: method must be a name or a compress function, got "
                        f"{type(method).__name__}")
    if method == "evict_for_space":
        from .methods.streaming_llm import evict_for_space
        return evict_for_space
    from .methods import get_compress_fn
    return get_compress_fn(method)


def _stand_in(pk):
    """(K, V) views of pk's dense shape over 2 * seq_len elements: seq stride 1, every other stride
    0 -- enough for the methods (they read shapes) and for _slice_of (slice offsets)."""
    B, H, S, D = pk.shape
    base = torch.empty(2 * max(S, 1), dtype=pk.k_pool.dtype, device=pk.k_pool.device)
    return (base.as_strided((B, H, S, D), (0, 0, 1, 0), 0),
            base.as_strided((B, H, S, D), (0, 0, 1, 0), max(S, 1)))


def _pool_span(t):
    """Byte span [lo, hi) of a whole pool view (kvc_plan_paged's span)."""
    es = t.element_size()
    ext = [(t.size(d) - 1) * t.stride(d) * es for d in range(3)]
    lo = t.data_ptr() + sum(e for e in ext if e < 0)
    return lo, t.data_ptr() + sum(e for e in ext if e > 0) + t.size(3) * es


def compress_paged(method, layers, out="inplace", **kwargs):
    """Run compress method `method` (a name from list_methods(), "evict_for_space", or the
    function) on `layers`, a list of PagedKV, with `kwargs` as the method's keyword arguments.

    out="inplace" (default): every layer the method changes is compacted into the leading pages
    of its sequences (output row t lands in the slot of logical row t); returns the list of new
    logical lengths -- an untouched layer returns its seq_len -- and the caller frees the pages
    from ceil(n / page_size) on.  out=[(K_dst, V_dst) | None, ...]: a layer with a pair lands in
    K_dst[:, :, :n] / V_dst[:, :, :n] (dense views under the `out` kwarg's rules), whatever the
    method does with it, its pool is not written, and those views are returned; None = in place.

    Everything is checked before anything launches: an error leaves every pool untouched."""
    return E._checked_call(lambda: _compress_paged(method, layers, out, kwargs))


def _compress_paged(method, layers, out, kwargs):
    fn = _resolve(method)
    if kwargs.get("h2o_manager") is not None:
        raise TypeError("compress_paged: h2o_attention with an H2OAttentionManager is not "
                        "supported on paged layers (its replay plans and side-stream copy assume "
                        "dense K/V); call it without a manager (L2 heavy hitters)")
    if not isinstance(layers, (list, tuple)) or not all(isinstance(x, PagedKV) for x in layers):
        raise TypeError("compress_paged: layers must be a list of PagedKV")
    layers = list(layers)
    L = len(layers)
    if isinstance(out, str):
        if out != "inplace":
            raise ValueError(f"out={out!r}: expected \"inplace\" or a list with one "
                             "(K_dst, V_dst) pair or None per layer")
        dests = ["inplace"] * L
    elif isinstance(out, (list, tuple)):
        if len(out) != L:
            raise ValueError(f"out has {len(out)} entries for {L} layers")
        dests = []
        for i, d in enumerate(out):
            if d is None or (isinstance(d, str) and d == "inplace"):
                dests.append("inplace")
            elif isinstance(d, (list, tuple)) and len(d) == 2:
                dests.append(tuple(d))
            else:
                raise TypeError(f"layer {i}: out entry must be a (K_dst, V_dst) pair or None")
    else:
        raise TypeError(f"out must be \"inplace\" or a list, got {type(out).__name__}")
    kvl = [_stand_in(pk) for pk in layers]
    seen = {}
    for i, (pk, (k, v), d) in enumerate(zip(layers, kvl, dests)):  # before anything is enqueued
        if d != "inplace":
            E._check_dest_tensors(i, k, v, d[0], d[1])
            continue
        for name, t in (("K", pk.k_pool), ("V", pk.v_pool)):
            if t.data_ptr() in seen:
                raise ValueError(f"layer {i}: {name} pool shares its memory with "
                                 f"{seen[t.data_ptr()]}: not compacted in place")
            seen[t.data_ptr()] = f"layer {i}'s {name} pool"
    raw = getattr(fn, "__wrapped__", fn)  # the method's own Python: no call memo, no `out`
    ctx = E._DestCall(dests)
    prev = getattr(E._dest_state, "ctx", None)
    try:
        E._dest_state.ctx = ctx
        try:
            res = raw(list(kvl), **kwargs)  # launches nothing: see _engine._defer()
        finally:
            E._dest_state.ctx = prev
        res = list(res)
        moves = E._dest_moves(kvl, res, dests, ctx)
        every = [j for jobs, _, _ in ctx.pending for j in jobs] + moves
        for j in every:
            pk = layers[j.layer_idx]
            if j.keys is not kvl[j.layer_idx][0] or j.k_dest is None:
                raise RuntimeError(f"layer {j.layer_idx}: the method built a job that "
                                   "compress_paged cannot map onto its PagedKV")
            j.paged = pk
            E._check_dest(j)
            j.dest_verified = True
            E._check_tensors(j)
            if j.k_dest is not j.keys:  # a dense destination must not meet the pools
                n = j.sink_len + j.n_select + j.tail_len
                for name, dst in (("K", j.k_dest), ("V", j.v_dest)):
                    lo, hi = E._span(dst, n)
                    for sname, pool in (("K", pk.k_pool), ("V", pk.v_pool)):
                        plo, phi = _pool_span(pool)
                        if n and lo < phi and plo < hi:
                            raise ValueError(f"layer {j.layer_idx}: {name} destination overlaps "
                                             f"the layer's {sname} pool")
    except BaseException:
        for undo in reversed(ctx.rollback):
            undo()
        raise
    scratch = [None] * L
    for _, run, _ in ctx.pending:
        run()  # _engine.execute -> run_jobs
    if moves:
        E.execute(moves, scratch, N.KVC_ASC, N.KVC_ALGO_SORT)
    n_of = {j.layer_idx: j.sink_len + j.n_select + j.tail_len for j in every}
    result = []
    for i, d in enumerate(dests):
        if d == "inplace":
            result.append(n_of[i] if i in n_of else int(res[i][0].size(2)))
        else:
            n = n_of.get(i, 0)
            result.append((d[0].narrow(2, 0, n), d[1].narrow(2, 0, n)))
    return result


def run_jobs(jobs, order, algo):
    """Launch checked paged jobs: one kvc_launch_paged per (device, dtype, B, H, D) group."""
    groups = {}
    for j in jobs:
        B, H, _, D = j.paged.shape
        groups.setdefault((j.keys.get_device(), j.keys.dtype, B, H, D), []).append(j)
    for (device, dtype, B, H, D), js in groups.items():
        external = any(j.ext_index is not None for j in js)
        if external and not all(j.ext_index is not None or j.n_select == 0 for j in js):
            raise RuntimeError("mixed external / engine-selected layers in one group")
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device)
            p = E._params(dtype, B, H, D, order, algo, external)
            n = len(js)
            table = np.zeros(n, dtype=N.LAYER_DTYPE)
            pages = np.zeros(n, dtype=N.PAGES_DTYPE)
            dests = np.zeros(n, dtype=N.DEST_DTYPE)
            dense = False
            for i, j in enumerate(js):
                pk = j.paged
                kp, vp, bt = pk.k_pool, pk.v_pool, pk.block_table
                inplace = j.k_dest is j.keys
                t = table[i]
                t["k"], t["v"] = kp.data_ptr(), vp.data_ptr()
                t["k_stride"] = (0, kp.stride(1), kp.stride(2))
                t["v_stride"] = (0, vp.stride(1), vp.stride(2))
                t["seq_len"], t["zone_start"], t["zone_len"] = pk.seq_len, j.zone_start, j.zone_len
                t["n_select"], t["sink_len"] = j.n_select, j.sink_len
                t["tail_start"], t["tail_len"] = j.tail_start, j.tail_len
                t["pool_kernel"], t["score_mode"] = j.pool_kernel, j.score_mode
                pages[i] = (bt.data_ptr(), bt.stride(0), kp.stride(0), vp.stride(0), kp.size(2),
                            kp.size(0), 1 if inplace else 0, 0)
                if inplace:
                    t["k_out"], t["v_out"] = t["k"], t["v"]
                else:
                    dense = True
                    t["k_out"], t["v_out"] = j.k_dest.data_ptr(), j.v_dest.data_ptr()
                    dests[i] = (j.k_dest.stride()[:3], j.v_dest.stride()[:3], 0, 0)
            dd = dests if dense else None
            ws, info = E._upload(p, table, device, js, B, H, dd, pages)
            E._launch(p, table, ws, info, stream, p.phases, dd, pages)


__all__ = ["PagedKV", "compress_paged"]
