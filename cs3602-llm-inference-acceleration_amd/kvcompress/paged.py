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

A PagedKV may carry a length per sequence (a ragged layer: the rows of a continuous batch).  The
method then runs once per distinct per-layer length profile over B = 1 stand-ins, every job it
records becomes the kvc_seq_t record of its (layer, sequence), and the call is one
kvc_launch_ragged per launch group, whatever B is (plan_ragged, _compress_ragged).
"""
import numpy as np
import torch

from . import _engine as E
from . import _native as N


def _check_pool_view(what, t, device=None):
    """A K / V pool view [num_pages, H, page_size, D] that the kernels can address as it is (a
    pool is never copied): a page size that is a power of two, a contiguous last dim, rows and
    strides of multiples of 16 bytes, no stride 0 over a dim larger than 1, a 16-byte aligned
    pointer -- and, given `device`, on that device.  `what` names the pool: "PagedKV: k_pool"."""
    npg, H, P, D = t.shape
    es = t.element_size()
    if npg < 1 or H < 1 or D < 1 or P < 1 or P > 65536 or P & (P - 1):
        raise ValueError(f"{what}: page_size must be a power of two in [1, 65536] and the pool "
                         f"non-empty; got a pool of shape {tuple(t.shape)}")
    if (t.stride(3) != 1 and D > 1) or (D * es) % 16 or any(
            (t.stride(d) * es) % 16 and t.size(d) > 1 for d in range(3)):
        raise ValueError(f"{what} needs a contiguous last dim and rows and strides that are "
                         f"multiples of 16 bytes (a pool is never copied); strides "
                         f"{tuple(t.stride())}")
    if any(t.stride(d) == 0 and t.size(d) > 1 for d in range(3)):
        raise ValueError(f"{what} has stride 0 on a dim larger than 1")
    if device is not None and t.device != device:
        raise ValueError(f"{what} is on {t.device}, the layer on {device}")
    if t.data_ptr() % 16:
        raise ValueError(f"{what} pointer not 16-byte aligned (a pool is never copied)")


def _check_scale_pool(what, t, shape=None, device=None, uniform_ok=False):
    """A float32 scale tensor.  Given `shape`: it is that [num_pages, H, page_size] pool, no
    stride 0 over a dim larger than 1 (uniform_ok: or it has one element).  Given `device`: it is
    there, its pointer 4-byte aligned.  `what` names it: "PagedKV: k_scale"."""
    if shape is not None:
        if t.dtype != torch.float32:
            raise TypeError(f"{what} must be float32, got {t.dtype}")
        if tuple(t.shape) != tuple(shape) and not (uniform_ok and t.numel() == 1):
            raise ValueError(f"{what} must {'have one element or ' if uniform_ok else ''}be "
                             f"[num_pages, H, page_size] = {tuple(shape)}; got {tuple(t.shape)}")
        if any(t.stride(d) == 0 and t.size(d) > 1 for d in range(t.dim())):
            raise ValueError(f"{what} has stride 0 on a dim larger than 1 (a scale shared by "
                             f"several rows cannot follow one of them); strides "
                             f"{tuple(t.stride())}")
    if device is not None:
        if t.device != device:
            raise ValueError(f"{what} is on {t.device}, the pools on {device}")
        if t.data_ptr() % 4:
            raise ValueError(f"{what} pointer not 4-byte aligned")


class PagedKV:
    """One layer of a paged cache: pools `[num_pages, H, page_size, D]` (views of any strides
    with a contiguous last dim and 16-byte aligned pointers and strides; never copied), an int32
    `block_table` [B, >= ceil(seq_len / page_size)] on the same device, and the common logical
    length `seq_len` of its B sequences.  vLLM's [N, P, H, D] cache is `cache.permute(0, 2, 1, 3)`;
    the halves of a fused [2, N, ...] buffer are `kv[0]` and `kv[1]`.

    A RAGGED layer gives `seq_len` as B non-negative ints instead -- a list, a tuple, a numpy
    integer array or a CPU integer tensor, one length per row of the block table, as a
    continuous-batching server has them.  The lengths are host data (the methods' size arithmetic
    is host Python): a device tensor is refused rather than silently synchronised on.  `seq_len`
    then reads back as the tuple of lengths, `seq_lens` is that tuple for either kind of layer,
    and `shape` is [B, H, max(seq_lens), D]: the envelope of the B sequences, of which sequence b
    fills rows [0, seq_lens[b]).

    A per-token quantised fp8 cache gives its dequantisation scales as `k_scale` / `v_scale`:
    float32 tensors on the pools' device, either a `[num_pages, H, page_size]` view of any
    non-zero strides addressed by the same block table (a pool stored [N, P, H] is
    `scales.permute(0, 2, 1)`), or ONE element -- a scale that is the same for every token
    (vLLM's per-tensor k_scale; read on the device, never synchronised on).  Keys are then ranked
    by bf16(norm(K8) * |k_scale|) and the scales of the kept rows move with them (include/kvc.h,
    "Per-token-scaled fp8 paged caches").  A uniform scale changes a result only through rounding
    ties; a uniform or absent v_scale is ignored.  Scaled layers are compacted in place or delivered
    to a PagedDest (no dense out= pair: it has no channel for the scales).
    A scale tensor of exactly one element counts as uniform whatever its shape -- a
    [1, 1, 1] pool of a one-page, one-head, one-slot cache included: it has one row, whose scale
    need not move.  That the scale pools alias neither each other, nor the K / V pools, nor the
    pools of another layer of the call is the caller's promise: compress_paged's check that no
    two in-place layers share a K / V pool does not look at the scale pools."""
    __slots__ = ("k_pool", "v_pool", "block_table", "seq_len", "seq_lens", "k_scale", "v_scale")

    @staticmethod
    def _lengths(seq_len):
        """None for an int length (checked by the caller), else the tuple of per-sequence ints."""
        if isinstance(seq_len, (bool, int)):
            return None
        if isinstance(seq_len, torch.Tensor):
            if seq_len.device.type != "cpu":
                raise TypeError(f"PagedKV: per-sequence lengths must be host data (a list, a numpy "
                                f"array or a CPU tensor); got a tensor on {seq_len.device} -- the "
                                "methods' size arithmetic runs on the host, and reading a device "
                                "tensor would synchronise silently")
            if seq_len.dim() != 1 or seq_len.dtype == torch.bool or seq_len.is_floating_point() \
                    or seq_len.is_complex():
                raise ValueError("PagedKV: per-sequence lengths must be a 1-D integer tensor; got "
                                 f"{seq_len.dtype} {tuple(seq_len.shape)}")
            vals = seq_len.tolist()
        elif isinstance(seq_len, np.ndarray):
            if seq_len.ndim != 1 or seq_len.dtype.kind not in "iu":
                raise ValueError("PagedKV: per-sequence lengths must be a 1-D integer array; got "
                                 f"{seq_len.dtype} {seq_len.shape}")
            vals = seq_len.tolist()
        elif isinstance(seq_len, (list, tuple)):
            vals = list(seq_len)
        else:
            return None
        for x in vals:
            if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or x < 0:
                raise ValueError("PagedKV: per-sequence lengths must be non-negative ints, got "
                                 f"{x!r}")
        return tuple(int(x) for x in vals)

    @staticmethod
    def _check_scale(name, t, k_pool):
        """A scale tensor against its pools (its device and pointer: the end of __init__)."""
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"PagedKV: {name} must be a tensor, got {type(t).__name__}")
        if not E.is_fp8(k_pool.dtype):
            raise TypeError(f"PagedKV: {name} given with {k_pool.dtype} pools: dequantisation "
                            "scales belong to fp8 (float8_e4m3fn / float8_e5m2) pools")
        _check_scale_pool(f"PagedKV: {name}", t, k_pool.shape[:3], uniform_ok=True)

    def __init__(self, k_pool, v_pool, block_table, seq_len, k_scale=None, v_scale=None):
        for name, t in (("k_pool", k_pool), ("v_pool", v_pool), ("block_table", block_table)):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"PagedKV: {name} must be a tensor, got {type(t).__name__}")
        if k_pool.dim() != 4 or v_pool.shape != k_pool.shape:
            raise ValueError("PagedKV: k_pool / v_pool must both be [num_pages, H, page_size, D]; "
                             f"got {tuple(k_pool.shape)} / {tuple(v_pool.shape)}")
        if k_pool.dtype not in E._SUPPORTED or v_pool.dtype != k_pool.dtype:
            raise ValueError("PagedKV: pools must be bfloat16 / float16 / float32 or fp8 "
                             "(float8_e4m3fn / float8_e5m2) and of one "
                             f"dtype; got {k_pool.dtype} / {v_pool.dtype}")
        P = k_pool.size(2)
        _check_pool_view("PagedKV: k_pool", k_pool)
        _check_pool_view("PagedKV: v_pool", v_pool)
        for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
            if t is not None:
                self._check_scale(name, t, k_pool)
        lens = self._lengths(seq_len)
        if lens is None and (isinstance(seq_len, bool) or not isinstance(seq_len, int) or
                             seq_len < 0):
            raise ValueError(f"PagedKV: seq_len must be a non-negative int (or one per sequence), "
                             f"got {seq_len!r}")
        if block_table.dtype != torch.int32 or block_table.dim() != 2 or \
                (block_table.stride(1) != 1 and block_table.size(1) > 1):
            raise ValueError("PagedKV: block_table must be an int32 [B, pages per sequence] "
                             "tensor with a contiguous last dim; got "
                             f"{block_table.dtype} {tuple(block_table.shape)}")
        if lens is not None and len(lens) != block_table.size(0):
            raise ValueError(f"PagedKV: {len(lens)} sequence lengths for a block table of "
                             f"{block_table.size(0)} rows")
        longest = seq_len if lens is None else max(lens, default=0)
        need = -(-longest // P)
        if block_table.size(0) < 1 or block_table.size(1) < need:
            raise ValueError(f"PagedKV: block_table {tuple(block_table.shape)} holds fewer than "
                             f"the {need} pages of {longest} rows of {P}")
        if not (k_pool.is_cuda and v_pool.is_cuda and block_table.is_cuda) or \
                not (k_pool.device == v_pool.device == block_table.device):
            raise ValueError("PagedKV: pools and block table must be on one ROCm device (no CPU "
                             f"fallback); got {k_pool.device} / {v_pool.device} / "
                             f"{block_table.device}")
        for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
            if t is not None:
                _check_scale_pool(f"PagedKV: {name}", t, device=k_pool.device)
        self.k_pool, self.v_pool, self.block_table = k_pool, v_pool, block_table
        self.k_scale, self.v_scale = k_scale, v_scale
        self.seq_len = seq_len if lens is None else lens
        self.seq_lens = (seq_len,) * block_table.size(0) if lens is None else lens

    @property
    def ragged(self):
        """True when the layer carries a length per sequence."""
        return not isinstance(self.seq_len, int)

    @property
    def shape(self):
        """The [B, H, seq_len, D] of the dense tensors the table describes; for a ragged layer
        seq_len is the longest sequence's (the envelope: sequence b fills rows [0, seq_lens[b]))."""
        return (self.block_table.size(0), self.k_pool.size(1), max(self.seq_lens),
                self.k_pool.size(3))

    @property
    def page_size(self):
        return self.k_pool.size(2)

    @property
    def scaled(self):
        """True when the layer carries a K or a V scale."""
        return self.k_scale is not None or self.v_scale is not None

    def scales_row(self):
        """The layer's kvc_scales_t (a SCALES_DTYPE record)."""
        r = np.zeros(1, dtype=N.SCALES_DTYPE)[0]
        flags = 0
        for side, t, uni, none in (("k", self.k_scale, N.SCALE_K_UNIFORM, N.SCALE_K_NONE),
                                   ("v", self.v_scale, N.SCALE_V_UNIFORM, N.SCALE_V_NONE)):
            if t is None:
                flags |= none
                continue
            r[side + "_scale"] = t.data_ptr()
            if t.numel() == 1:
                flags |= uni
            else:
                r[side + "_page_stride"] = t.stride(0)
                r[side + "_stride"] = (t.stride(1), t.stride(2))
        r["flags"] = flags
        return r

    def scales_to_dense(self, n=None, b=None):
        """(K scales, V scales) [B, H, n] of the first n logical rows, by torch indexing, as
        to_dense gives the rows; a uniform scale is expanded, a missing one is None."""
        pg, slot = self._page_slot("scales_to_dense", n, b)
        H = self.k_pool.size(1)

        def dense(t):
            if t is None:
                return None
            if t.numel() == 1:
                return t.reshape(1, 1, 1).expand(pg.size(0), H, pg.size(1))
            return t[pg, :, slot].permute(0, 2, 1)
        return dense(self.k_scale), dense(self.v_scale)

    def _page_slot(self, who, n, b):
        """(page [B, n], slot [n]) of the first n logical rows -- by default all of them, or
        sequence b's -- of every sequence, or of sequence b alone ([1, n])."""
        if n is None:
            if b is None and self.ragged:
                raise ValueError(f"PagedKV.{who}: a ragged layer needs b (one sequence) or n")
            n = self.seq_len if b is None else self.seq_lens[b]
        table = self.block_table if b is None else self.block_table[b:b + 1]
        pos = torch.arange(n, device=self.k_pool.device)
        pg = table[:, :max(-(-n // self.page_size), 1)].long()
        return pg[:, pos // self.page_size], pos % self.page_size

    def to_dense(self, n=None, b=None):
        """(K, V) [B, H, n, D] of the first n (default seq_len) logical rows, by torch indexing:
        a convenience for tests and debugging, not on the hot path.  With `b`: sequence b's rows
        alone, [1, H, n, D], n by default its own length (a ragged layer needs `b` or `n`)."""
        pg, slot = self._page_slot("to_dense", n, b)
        return tuple(pool[pg, :, slot].permute(0, 2, 1, 3) for pool in (self.k_pool, self.v_pool))


class PagedDest:
    """Where one paged layer's compressed sequence goes when it must not be compacted in place
    (include/kvc.h, "Paged destinations"): an int32 `block_table` [B, >= ceil(n / page_size)] of
    DESTINATION page ids on the pools' device, and optionally destination pools `k_pool` / `v_pool`
    -- `[num_pages', H, page_size', D]` views of the source's dtype, H and D under PagedKV's stride
    and alignment rules; page size and pool size need not equal the source's.  Without pools the
    rows go into fresh pages of the SOURCE pools (and, for a per-token-scaled layer, the kept rows'
    scales into the source scale pools' slots of those pages).  With pools of its own a
    per-token-scaled layer needs `k_scale` / `v_scale`: float32 `[num_pages', H, page_size']`
    views, given exactly for the sides that are per-token on the source.

    Output row t of sequence b lands in slot t % page_size' of page block_table[b, t // page_size'],
    sink rows included; the source pool is only read, so its pages may be shared between
    sequences (a cached prefix, forked sequences).  The caller promises that a destination page is
    neither a page any sequence of the layer reads, nor a destination page of another (layer,
    sequence), nor a page of the other side (K / V): the tables are device data and are not read
    (kvcompress.paged.check_repage_tables checks host copies of them).  A destination pool is
    either the source's own view or disjoint from both source pools, which IS checked."""
    __slots__ = ("block_table", "k_pool", "v_pool", "k_scale", "v_scale")

    def __init__(self, block_table, k_pool=None, v_pool=None, k_scale=None, v_scale=None):
        for name, t in (("block_table", block_table), ("k_pool", k_pool), ("v_pool", v_pool),
                        ("k_scale", k_scale), ("v_scale", v_scale)):
            if not isinstance(t, torch.Tensor) and not (t is None and name != "block_table"):
                raise TypeError(f"PagedDest: {name} must be a tensor, got {type(t).__name__}")
        if (k_pool is None) != (v_pool is None):
            raise ValueError("PagedDest: give both k_pool and v_pool, or neither (the source's)")
        if k_pool is None and (k_scale is not None or v_scale is not None):
            raise ValueError("PagedDest: k_scale / v_scale belong to destination pools of their "
                             "own; without k_pool / v_pool the source's scale pools are used")
        if block_table.dtype != torch.int32 or block_table.dim() != 2 or \
                (block_table.stride(1) != 1 and block_table.size(1) > 1):
            raise ValueError("PagedDest: block_table must be an int32 [B, pages per sequence] "
                             "tensor with a contiguous last dim; got "
                             f"{block_table.dtype} {tuple(block_table.shape)}")
        if not block_table.is_cuda:
            raise ValueError("PagedDest: block_table must be on the pools' ROCm device; got "
                             f"{block_table.device}")
        self.block_table, self.k_pool, self.v_pool = block_table, k_pool, v_pool
        self.k_scale, self.v_scale = k_scale, v_scale

    def bind(self, i, pk):
        """This destination resolved against layer i's PagedKV and checked: a PagedDest whose
        pools (and scales, for the per-token sides) are tensors.  Raises naming the layer."""
        what = f"layer {i}: PagedDest"
        kp, vp = (pk.k_pool, pk.v_pool) if self.k_pool is None else (self.k_pool, self.v_pool)
        bt = self.block_table
        if bt.device != pk.k_pool.device or bt.size(0) != pk.block_table.size(0):
            raise ValueError(f"{what}: block_table {tuple(bt.shape)} on {bt.device}, the layer has "
                             f"{pk.block_table.size(0)} sequences on {pk.k_pool.device}")
        _, H, _, D = pk.k_pool.shape
        for name, t in (("k_pool", kp), ("v_pool", vp)):
            if t.dtype != pk.k_pool.dtype:
                raise TypeError(f"{what}: {name} has dtype {t.dtype}, the layer {pk.k_pool.dtype}")
            if t.dim() != 4 or t.shape != kp.shape or t.size(1) != H or t.size(3) != D:
                raise ValueError(f"{what}: {name} must be [num_pages, H, page_size, D] with the "
                                 f"layer's H = {H} and D = {D}, K and V alike; got "
                                 f"{tuple(t.shape)}")
        npg, _, P, _ = kp.shape
        _check_pool_view(f"{what}: k_pool", kp, pk.k_pool.device)
        _check_pool_view(f"{what}: v_pool", vp, pk.k_pool.device)
        # a destination pool: the source's own view, or disjoint from both source pools
        same = []
        for name, t, src in (("K", kp, pk.k_pool), ("V", vp, pk.v_pool)):
            own = t is src or (t.data_ptr() == src.data_ptr() and t.shape == src.shape and
                               t.stride() == src.stride())
            same.append(own)
            if own:
                continue
            lo, hi = _pool_span(t)
            for sname, pool in (("K", pk.k_pool), ("V", pk.v_pool)):
                plo, phi = _pool_span(pool)
                if lo < phi and plo < hi:
                    raise ValueError(f"{what}: {name} destination pool overlaps the layer's "
                                     f"{sname} pool without being the same view")
        if not all(same):
            (klo, khi), (vlo, vhi) = _pool_span(kp), _pool_span(vp)
            if klo < vhi and vlo < khi:
                raise ValueError(f"{what}: K and V destination pools overlap")
        # scales: exactly for the sides that are per-token on the source
        scales = []
        for side, src, own in (("k_scale", pk.k_scale, self.k_scale),
                               ("v_scale", pk.v_scale, self.v_scale)):
            per_token = src is not None and src.numel() != 1
            t = src if (self.k_pool is None and per_token) else own
            if per_token and t is None:
                raise ValueError(f"{what}: the layer's {side} is per-token, so destination pools "
                                 f"of their own need a destination {side} [num_pages, H, "
                                 f"page_size] = {(npg, H, P)}")
            if not per_token and t is not None:
                raise ValueError(f"{what}: {side} given, but the layer's {side} is not per-token "
                                 "(nothing of it moves)")
            if t is not None and t is not src:
                _check_scale_pool(f"{what}: {side}", t, (npg, H, P), pk.k_pool.device)
            scales.append(t)
        return PagedDest(bt, kp, vp, *scales)

    # ---- of a bound destination ----
    @property
    def page_size(self):
        return self.k_pool.size(2)

    @property
    def capacity(self):
        """Rows per sequence that the table can address."""
        return self.block_table.size(1) * self.page_size

    def dest_row(self):
        """The kvc_page_dest_t (a PAGE_DEST_DTYPE record)."""
        r = np.zeros(1, dtype=N.PAGE_DEST_DTYPE)[0]
        kp, vp, bt = self.k_pool, self.v_pool, self.block_table
        r["block_table"], r["table_stride"] = bt.data_ptr(), bt.stride(0)
        r["k_page_stride"], r["v_page_stride"] = kp.stride(0), vp.stride(0)
        r["k_stride"], r["v_stride"] = (kp.stride(1), kp.stride(2)), (vp.stride(1), vp.stride(2))
        r["page_size"], r["num_pages"] = kp.size(2), kp.size(0)
        return r

    def scales_row(self, src_row):
        """The destination kvc_scales_t: the source's flags, the per-token sides' pools."""
        r = np.zeros(1, dtype=N.SCALES_DTYPE)[0]
        r["flags"] = src_row["flags"]
        for side, t in (("k", self.k_scale), ("v", self.v_scale)):
            if t is not None:
                r[side + "_scale"] = t.data_ptr()
                r[side + "_page_stride"] = t.stride(0)
                r[side + "_stride"] = (t.stride(1), t.stride(2))
        return r

    def stand_in(self, pk):
        """(K, V) dense stand-ins [B, H, capacity, D] of the destination, as _stand_in's: the
        deferred-call machinery carries them as the job's destination; nothing is read from them."""
        B, H, _, D = pk.shape
        cap = max(self.capacity, 1)
        key = (pk.k_pool.dtype, pk.k_pool.device)
        base = _STAND_INS.get(key)  # one buffer per (dtype, device): no allocation per layer
        if base is None or base.numel() < cap + D:
            base = _STAND_INS[key] = torch.empty(max(cap + D, 1 << 16), dtype=key[0],
                                                 device=key[1])
        return tuple(base.as_strided((B, H, cap, D), (0, 0, 1, 0), 0) for _ in range(2))


# PagedDest.stand_in's storage: the stand-ins of every layer and call are views of one buffer per
# (dtype, device).  They carry shapes only; nothing is ever read from or written to them.
_STAND_INS = {}


def check_repage_tables(src_table, src_lens, P_src, dst_table, new_lens, P_dst):
    """A debugging aid for callers of compress_paged(out=[PagedDest...]) whose destination pages
    are in the SOURCE pool: checks host copies of the tables (numpy integer arrays [B, pages]; the
    lengths one int per sequence, or one int for all) against the caller's promise.  Raises
    ValueError naming the first page that is both a source page within `src_lens` and a
    destination page within `new_lens`, or a destination page used twice; table entries past the
    lengths are ignored.  Pure host function; compress_paged never calls it."""
    src_table, dst_table = np.asarray(src_table), np.asarray(dst_table)
    B = src_table.shape[0]
    if dst_table.shape[0] != B:
        raise ValueError(f"check_repage_tables: {B} source rows, {dst_table.shape[0]} destination "
                         "rows")
    lens = lambda x: [int(x)] * B if np.ndim(x) == 0 else [int(v) for v in x]  # noqa: E731
    src_lens, new_lens = lens(src_lens), lens(new_lens)
    read = {}
    for b in range(B):
        for p in src_table[b, :-(-src_lens[b] // P_src)].tolist():
            read.setdefault(int(p), b)
    written = {}
    for b in range(B):
        for j, p in enumerate(dst_table[b, :-(-new_lens[b] // P_dst)].tolist()):
            p = int(p)
            if p in read:
                raise ValueError(f"check_repage_tables: page {p} is destination page {j} of "
                                 f"sequence {b} and a source page of sequence {read[p]}")
            if p in written:
                raise ValueError(f"check_repage_tables: page {p} is a destination page twice: of "
                                 f"sequence {written[p]} and of sequence {b} (page {j})")
            written[p] = b


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


def _claim_pools(seen, i, pk):
    """Layer i is compacted in place: its pools are no earlier in-place layer's (`seen`)."""
    for name, t in (("K", pk.k_pool), ("V", pk.v_pool)):
        if t.data_ptr() in seen:
            raise ValueError(f"layer {i}: {name} pool shares its memory with "
                             f"{seen[t.data_ptr()]}: not compacted in place")
        seen[t.data_ptr()] = f"layer {i}'s {name} pool"


def _check_capacity(i, pd, n):
    """Layer i's bound PagedDest can address the n rows of its longest result."""
    if n > pd.capacity:
        raise ValueError(f"layer {i}: PagedDest block_table {tuple(pd.block_table.shape)} holds "
                         f"fewer than the {-(-n // pd.page_size)} pages of {n} rows of "
                         f"{pd.page_size}")


def _deferred(raw, kvl, dests, kwargs):
    """_engine._deferred for a method's own Python over stand-ins (it gets a list of its own)."""
    return E._deferred(lambda kv: raw(list(kv), **kwargs), kvl, dests)


def _launch_rows(pairs):
    """The numpy rows of a launch group, from the (PagedKV, bound PagedDest or None) of its
    layers -- a group's layers are all scaled or none is, and all have a PagedDest or none has:
    (layer table, dict of the pages / scales / pdests / dscales arrays, None where the group has
    no such table).  Pools, strides and descriptions are filled; k_out / v_out are the
    destination pools, or the layer's own with in_place = 1.  The segment fields and whatever
    a dense destination changes are the caller's."""
    n = len(pairs)
    sc, repage = pairs[0][0].scaled, pairs[0][1] is not None
    table = np.zeros(n, dtype=N.LAYER_DTYPE)
    rows = dict(pages=np.zeros(n, dtype=N.PAGES_DTYPE),
                scales=np.zeros(n, dtype=N.SCALES_DTYPE) if sc else None,
                pdests=np.zeros(n, dtype=N.PAGE_DEST_DTYPE) if repage else None,
                dscales=np.zeros(n, dtype=N.SCALES_DTYPE) if repage and sc else None)
    for i, (pk, pd) in enumerate(pairs):
        kp, vp, bt = pk.k_pool, pk.v_pool, pk.block_table
        t = table[i]
        t["k"] = t["k_out"] = kp.data_ptr()
        t["v"] = t["v_out"] = vp.data_ptr()
        t["k_stride"] = (0, kp.stride(1), kp.stride(2))
        t["v_stride"] = (0, vp.stride(1), vp.stride(2))
        rows["pages"][i] = (bt.data_ptr(), bt.stride(0), kp.stride(0), vp.stride(0), kp.size(2),
                            kp.size(0), 0 if repage else 1, 0)
        if sc:
            rows["scales"][i] = pk.scales_row()
        if repage:  # through the destination table: kvc_launch_repage
            t["k_out"], t["v_out"] = pd.k_pool.data_ptr(), pd.v_pool.data_ptr()
            rows["pdests"][i] = pd.dest_row()
            if sc:
                rows["dscales"][i] = pd.scales_row(rows["scales"][i])
    return table, rows


def compress_paged(method, layers, out="inplace", **kwargs):
    """Run compress method `method` (a name from list_methods(), "evict_for_space", or the
    function) on `layers`, a list of PagedKV, with `kwargs` as the method's keyword arguments.

    out="inplace" (default): every layer the method changes is compacted into the leading pages
    of its sequences (output row t lands in the slot of logical row t); returns the list of new
    logical lengths -- an untouched layer returns its seq_len -- and the caller frees the pages
    from ceil(n / page_size) on.  out=[(K_dst, V_dst) | None, ...]: a layer with a pair lands in
    K_dst[:, :, :n] / V_dst[:, :, :n] (dense views under the `out` kwarg's rules), whatever the
    method does with it, its pool is not written, and those views are returned; None = in place.

    Ragged layers (PagedKV with a length per sequence): when any layer is ragged, all layers share
    one batch B (an int layer counts as B equal lengths), and the result is what the method gives
    on each sequence alone -- every layer restricted to block_table[b:b+1] and seq_lens[b], layer
    indices (skip_layers, pyramid_kv's schedule) unchanged.  In place only; returns per layer the
    list of B new lengths.  The kernel launches do not depend on B: one SCORE / SELECT / GATHER
    set per (device, dtype, H, D, order, algo) group (kvc_launch_ragged).  Caller-provided indices
    (strategy="random", h2o_attention's heavy hitters) and dense `out` pairs raise TypeError.

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
            elif isinstance(d, PagedDest):
                dests.append(d)
            elif isinstance(d, (list, tuple)) and len(d) == 2:
                dests.append(tuple(d))
            else:
                raise TypeError(f"layer {i}: out entry must be a (K_dst, V_dst) pair, a "
                                "PagedDest or None")
    else:
        raise TypeError(f"out must be \"inplace\" or a list, got {type(out).__name__}")
    if any(pk.ragged for pk in layers):
        if any(isinstance(d, tuple) and pk.scaled for pk, d in zip(layers, dests)):
            raise TypeError("compress_paged: a scaled layer (k_scale / v_scale) is compacted in "
                            "place or into a PagedDest only")
        return _compress_ragged(fn, layers, dests, kwargs)
    kvl = [_stand_in(pk) for pk in layers]
    seen = {}
    pdests = [None] * L  # the bound PagedDest of a layer that has one
    for i, (pk, (k, v), d) in enumerate(zip(layers, kvl, dests)):  # before anything is enqueued
        if isinstance(d, PagedDest):
            # the deferred-call machinery carries a dense stand-in pair as the destination
            pdests[i] = d.bind(i, pk)
            dests[i] = pdests[i].stand_in(pk)
            continue
        if d != "inplace" and pk.scaled:
            raise TypeError(f"layer {i}: a scaled layer (k_scale / v_scale) is compacted in "
                            "place or into a PagedDest only: a dense out= pair has no channel "
                            "for the kept rows' scales")
        if d != "inplace":
            E._check_dest_tensors(i, k, v, d[0], d[1])
            continue
        _claim_pools(seen, i, pk)
    raw = getattr(fn, "__wrapped__", fn)  # the method's own Python: no call memo, no `out`
    res, moves, ctx = _deferred(raw, kvl, dests, kwargs)
    with E._rolled_back(ctx):
        every = [j for jobs, _, _ in ctx.pending for j in jobs] + moves
        for j in every:
            pk = layers[j.layer_idx]
            if j.keys is not kvl[j.layer_idx][0] or j.k_dest is None:
                raise RuntimeError(f"layer {j.layer_idx}: the method built a job that "
                                   "compress_paged cannot map onto its PagedKV")
            j.paged = pk
            j.page_dest = pdests[j.layer_idx]
            n = j.sink_len + j.n_select + j.tail_len
            if j.page_dest is not None:
                _check_capacity(j.layer_idx, j.page_dest, n)
            else:  # (a PagedDest's stand-ins say nothing about memory)
                E._check_dest(j)
            j.dest_verified = True
            E._check_tensors(j)
            if j.page_dest is None and j.k_dest is not j.keys:  # dense: must not meet the pools
                for name, dst in (("K", j.k_dest), ("V", j.v_dest)):
                    lo, hi = E._span(dst, n)
                    for sname, pool in (("K", pk.k_pool), ("V", pk.v_pool)):
                        plo, phi = _pool_span(pool)
                        if n and lo < phi and plo < hi:
                            raise ValueError(f"layer {j.layer_idx}: {name} destination overlaps "
                                             f"the layer's {sname} pool")
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
        elif pdests[i] is not None:  # the destination table now describes n rows
            result.append(n_of.get(i, 0))
        else:
            n = n_of.get(i, 0)
            result.append((d[0].narrow(2, 0, n), d[1].narrow(2, 0, n)))
    return result


def plan_ragged(fn, lens, geometry, kwargs, check=True, unordered=()):
    """Host planning of a ragged call (no launch, no device copy): the method's own Python runs
    once per distinct per-layer length profile over B = 1 stand-ins, inside the deferred-call
    context, and every job or move it records becomes the kvc_seq_t record of its (layer,
    sequence).  `lens[l][b]` are the lengths, `geometry[l]` = (H, D, dtype, device) of layer l's
    stand-ins; check=False skips the engine's tensor checks (host-only models of the mapping).
    Returns (records [L][B] SEQ_DTYPE, no-op where nothing moves; how: {(layer, b): (order, algo)
    of an engine job, or None for a copy-only move}; new lengths [L][B])."""
    rec, spans, new_len = _plan_spans(fn, lens, geometry, kwargs, check, unordered)
    return rec, {(li, b): how for li, bs, how in spans for b in bs}, new_len


def _plan_spans(fn, lens, geometry, kwargs, check, unordered=()):
    """plan_ragged with `how` per span: [(layer, [b, ...], (order, algo) | None)], one entry per
    (profile, layer) that an engine job or a move touches.  `unordered`: the layers that are
    written out of place (a PagedDest), which the in-place segment-order rule does not bind."""
    L, B = len(lens), len(lens[0])
    rec = np.zeros((L, B), dtype=N.SEQ_DTYPE)
    for li in range(L):  # the no-op record: every row a sink row
        rec[li]["seq_len"] = rec[li]["sink_len"] = rec[li]["n_out"] = lens[li]
    new_len = [list(l) for l in lens]
    spans = []
    profiles = {}
    for b in range(B):
        profiles.setdefault(tuple(l[b] for l in lens), []).append(b)
    raw = getattr(fn, "__wrapped__", fn)  # the method's own Python: no call memo, no `out`
    dests = ["inplace"] * L
    bases = {}  # one stand-in storage per (dtype, device): K rows at 0, V rows behind them
    for (_, _, dtype, device), l in zip(geometry, lens):
        bases[(dtype, device)] = max(bases.get((dtype, device), 1), max(l))
    bases = {k: (torch.empty(2 * n, dtype=k[0], device=k[1]), n) for k, n in bases.items()}
    for prof, bs in profiles.items():
        kvl = []
        for (H, D, dtype, device), S in zip(geometry, prof):
            base, half = bases[(dtype, device)]
            kvl.append((base.as_strided((1, H, S, D), (0, 0, 1, 0), 0),
                        base.as_strided((1, H, S, D), (0, 0, 1, 0), half)))
        res, moves, ctx = _deferred(raw, kvl, dests, kwargs)
        with E._rolled_back(ctx):
            found = [(j, how) for (jobs, _, _), how in zip(ctx.pending, ctx.how) for j in jobs]
            found += [(j, None) for j in moves]
            done = set()
            for j, how in found:
                li = j.layer_idx
                if j.keys is not kvl[li][0] or j.k_dest is not j.keys or li in done:
                    raise RuntimeError(f"layer {li}: the method built a job that compress_paged "
                                       "cannot map onto its PagedKV")
                if j.ext_index is not None or (how is None and j.n_select):
                    raise TypeError(
                        "compress_paged: ragged layers (per-sequence lengths) do not take "
                        "caller-provided indices (strategy=\"random\", h2o_attention's heavy "
                        "hitters): compress such sequences one by one")
                done.add(li)
                if li not in unordered:
                    E._check_dest(j)  # in place on a stand-in: the segment order
                if check:
                    E._check_tensors(j)
                n = j.sink_len + j.n_select + j.tail_len
                rec[li, bs] = (prof[li], j.zone_start, j.zone_len, j.n_select, j.sink_len,
                               j.tail_start, j.tail_len, j.score_mode, j.pool_kernel, n, (0, 0))
                spans.append((li, bs, how))
                row = new_len[li]
                for b in bs:
                    row[b] = n
            for li in set(range(L)) - done:  # untouched, or already the front view
                n = int(res[li][0].size(2))
                if n != prof[li]:
                    row = new_len[li]
                    for b in bs:
                        row[b] = n
    return rec, spans, new_len


def _compress_ragged(fn, layers, dests, kwargs):
    """compress_paged on layers with per-sequence lengths: plan_ragged, one upload of every
    group's records, one kvc_launch_ragged per (device, dtype, H, D, order, algo) group.  In a
    group's launch every (layer, sequence) that belongs to another group -- or to none -- has the
    no-op record."""
    L = len(layers)
    if any(isinstance(d, tuple) for d in dests):
        raise TypeError("compress_paged: ragged layers (per-sequence lengths) are compacted in "
                        "place only, or delivered to a PagedDest; dense out= pairs are not "
                        "supported")
    if kwargs.get("strategy") == "random":
        raise TypeError("compress_paged: ragged layers (per-sequence lengths) do not take "
                        "caller-provided indices (strategy=\"random\")")
    B = layers[0].block_table.size(0)
    seen = {}
    for i, pk in enumerate(layers):
        if pk.block_table.size(0) != B:
            raise ValueError(f"layer {i}: {pk.block_table.size(0)} sequences, layer 0 has {B}: the "
                             "layers of a ragged call share one batch")
        if not isinstance(dests[i], PagedDest):  # (a PagedDest: the pool is only read)
            _claim_pools(seen, i, pk)
    pdests = [d.bind(i, pk) if isinstance(d, PagedDest) else None
              for i, (pk, d) in enumerate(zip(layers, dests))]
    rec, spans, new_len = _plan_spans(
        fn, [pk.seq_lens for pk in layers],
        [(pk.k_pool.size(1), pk.k_pool.size(3), pk.k_pool.dtype, pk.k_pool.device)
         for pk in layers], kwargs, True, {i for i, d in enumerate(pdests) if d is not None})
    for li, pd in enumerate(pdests):
        if pd is None:
            continue
        _check_capacity(li, pd, max(new_len[li], default=0))
        # a sequence that no job or move touches passes through (or is already its front view):
        # its destination table must describe it, so its rows are copied
        rest = sorted(set(range(B)) - {b for l2, bs, _ in spans if l2 == li for b in bs})
        rest = [b for b in rest if new_len[li][b] > 0]
        if rest:
            for b in rest:
                rec[li, b] = (layers[li].seq_lens[b], 0, 0, 0, new_len[li][b], 0, 0,
                              N.KVC_SCORE_NORM, 0, new_len[li][b], (0, 0))
            spans.append((li, rest, None))
    # launch groups: engine jobs by their (order, algo); copy-only moves ride in a group of their
    # geometry (any order / algo: nothing is selected)
    # (scaled layers launch apart: kvc_launch_scaled takes a scale description per layer)
    # (layers with a PagedDest launch apart as well: kvc_launch_repage)
    geos = [(pk.k_pool.get_device(), pk.k_pool.dtype, pk.k_pool.size(1), pk.k_pool.size(3),
             pk.scaled, pd is not None) for pk, pd in zip(layers, pdests)]
    groups = {}
    for li, bs, how in spans:
        if how is not None:
            groups.setdefault(geos[li] + how, {}).setdefault(li, []).extend(bs)
    for li, bs, how in spans:
        if how is None:
            key = next((k for k in groups if k[:6] == geos[li]),
                       geos[li] + (N.KVC_ASC, N.KVC_ALGO_SORT))
            groups.setdefault(key, {}).setdefault(li, []).extend(bs)
    if not groups:
        return new_len
    # every group's records, all of them in one array per device: one host-to-device copy
    plans, per_dev = [], {}
    for key, members in groups.items():
        lis = sorted(members)
        seqs = np.zeros((len(lis), B), dtype=N.SEQ_DTYPE)
        for i, li in enumerate(lis):
            seqs[i]["seq_len"] = layers[li].seq_lens
            if not key[5]:  # in place: the no-op record.  (A PagedDest layer: n_out = 0, nothing
                seqs[i]["sink_len"] = seqs[i]["n_out"] = layers[li].seq_lens  # is written)
            seqs[i, members[li]] = rec[li, members[li]]
        per_dev.setdefault(key[0], []).append(seqs)
        plans.append((key, lis, len(per_dev[key[0]]) - 1))
    host, dev, start = {}, {}, {}
    for device, arrs in per_dev.items():
        host[device] = np.concatenate([a.reshape(-1) for a in arrs])
        start[device] = np.cumsum([0] + [a.size for a in arrs]) * N.SEQ_DTYPE.itemsize
        dev[device] = torch.from_numpy(host[device].view(np.uint8)).to(
            torch.device("cuda", device))
    launches = []
    for (device, dtype, H, D, _, _, order, algo), lis, slot in plans:  # plan (and check)
        with torch.cuda.device(device):
            p = E._params(dtype, B, H, D, order, algo, False)
            table, rows = _launch_rows([(layers[li], pdests[li]) for li in lis])
            ragged = np.zeros(len(lis), dtype=N.RAGGED_DTYPE)
            off = int(start[device][slot])
            for i in range(len(lis)):  # the layer's B records, on the host and on the device
                step = off + i * B * N.SEQ_DTYPE.itemsize
                ragged[i] = (host[device].ctypes.data + step, dev[device].data_ptr() + step)
            tables = N.Tables(ragged=ragged, **rows)
            ws, info = E._upload(p, table, device, None, B, H, tables)
            launches.append((device, p, table, ws, info, tables))
    for device, p, table, ws, info, tables in launches:
        with torch.cuda.device(device):
            E._launch(p, table, ws, info, torch.cuda.current_stream(device), p.phases, tables)
    return new_len


def run_jobs(jobs, order, algo):
    """Launch checked paged jobs: one kvc_launch_paged per (device, dtype, B, H, D) group --
    kvc_launch_scaled for the group's layers that carry scales."""
    groups = {}
    for j in jobs:
        B, H, _, D = j.paged.shape
        groups.setdefault((j.keys.get_device(), j.keys.dtype, B, H, D, j.paged.scaled,
                           j.page_dest is not None), []).append(j)
    for (device, dtype, B, H, D, sc, repage), js in groups.items():
        external = any(j.ext_index is not None for j in js)
        if external and not all(j.ext_index is not None or j.n_select == 0 for j in js):
            raise RuntimeError("mixed external / engine-selected layers in one group")
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device)
            p = E._params(dtype, B, H, D, order, algo, external)
            table, rows = _launch_rows([(j.paged, j.page_dest) for j in js])
            dests = np.zeros(len(js), dtype=N.DEST_DTYPE)
            dense = False
            for i, j in enumerate(js):
                t = table[i]
                t["seq_len"], t["zone_start"], t["zone_len"] = j.paged.seq_len, j.zone_start, \
                    j.zone_len
                t["n_select"], t["sink_len"] = j.n_select, j.sink_len
                t["tail_start"], t["tail_len"] = j.tail_start, j.tail_len
                t["pool_kernel"], t["score_mode"] = j.pool_kernel, j.score_mode
                if repage or j.k_dest is j.keys:
                    continue
                if sc:  # (compress_paged refuses it before planning)
                    raise TypeError("a scaled layer is compacted in place only")
                dense = True  # a dense destination: the pool is only read
                rows["pages"]["in_place"][i] = 0
                t["k_out"], t["v_out"] = j.k_dest.data_ptr(), j.v_dest.data_ptr()
                dests[i] = (j.k_dest.stride()[:3], j.v_dest.stride()[:3], 0, 0)
            tables = N.Tables(dests=dests if dense else None, **rows)
            ws, info = E._upload(p, table, device, js, B, H, tables)
            E._launch(p, table, ws, info, stream, p.phases, tables)


__all__ = ["PagedKV", "PagedDest", "compress_paged", "check_repage_tables"]
