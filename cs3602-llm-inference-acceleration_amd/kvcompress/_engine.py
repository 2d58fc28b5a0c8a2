"""Batching layer between the reference-shaped compress functions and the HIP engine.

A compress function walks the layers exactly like its reference (same branches, same integer
arithmetic) and, for every layer that the reference would gather/concatenate, records a
`Segments` job instead of issuing torch ops.  `execute()` then runs all jobs of the call as ONE
batched engine launch per (device, dtype, batch, heads, head_dim) group -- score, select and
gather kernels over every layer at once -- and writes the new (K, V) tensors back into the list.
"""
import contextlib
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import _native as N


def py_slice(S, start=None, stop=None):
    """(start, length) of range(S)[start:stop] -- Python/torch slice semantics, incl. `-0:`."""
    r = range(S)[start:stop]
    return r.start, len(r)


@dataclass(slots=True)
class Segments:
    """out = X[:, :, 0:sink_len] ++ X[:, :, zone][selected] ++ X[:, :, tail]  (X = K and V)."""
    layer_idx: int
    keys: torch.Tensor
    values: torch.Tensor
    sink_len: int = 0
    zone_start: int = 0
    zone_len: int = 0
    n_select: int = 0
    tail_start: int = 0
    tail_len: int = 0
    score_mode: int = N.KVC_SCORE_NORM
    pool_kernel: int = 0
    ext_index: Optional[torch.Tensor] = None  # [B, H, n_select] int64 zone-local, ascending
    # caller-provided destination (kvc_launch_dest): [B, H, S_d >= n_out, D] views whose rows
    # [0, n_out) receive the output; the layer's own keys / values = compacted in place
    k_dest: Optional[torch.Tensor] = None
    v_dest: Optional[torch.Tensor] = None
    dest_checked: bool = False  # dest_call() has run _check_dest_tensors on this destination
    dest_verified: bool = False  # ... and _check_dest: the launch does not repeat it
    # compress_paged: the layer's PagedKV.  keys / values are then stand-ins of the layer's shape
    # (nothing is read from them) and the job is launched by paged.run_jobs (kvc_launch_paged)
    paged: Optional[object] = None
    # compress_paged: the layer's PagedDest, already bound to its PagedKV (k_dest / v_dest are
    # then stand-ins too; the job is launched with kvc_launch_repage)
    page_dest: Optional[object] = None


# fp8 K/V: the OCP formats only (gfx950's native fp8, dequantisation scale 1).  Keys are scored
# as their exact bfloat16 upcast, rows are copied as bytes.  The fnuz
# formats and raw uint8 / int8 tensors stay unsupported.
_FP8 = {torch.float8_e4m3fn: N.KVC_F8E4M3, torch.float8_e5m2: N.KVC_F8E5M2}
_SUPPORTED = {torch.bfloat16: N.KVC_BF16, torch.float16: N.KVC_F16, torch.float32: N.KVC_F32,
              **_FP8}
_ESIZE = {torch.bfloat16: 2, torch.float16: 2, torch.float32: 4,
          torch.float8_e4m3fn: 1, torch.float8_e5m2: 1}


def is_fp8(dtype):
    return dtype in _FP8


class HipEvent:
    """A timing event created with hipEventDisableSystemFence, recorded on a raw HIP stream:
    recording it does not write back / invalidate caches the way torch.cuda.Event's default
    events do (measured: split launches with torch events cost the headline step 1.5-2.3 %,
    tools/timer_overhead.py).  Uses the HIP runtime instance torch has loaded (found in the
    process's memory map, whatever its soname); PhaseTimer falls back to torch.cuda.Event when
    it cannot be found."""

    _hip = None
    DISABLE_SYSTEM_FENCE = 0x20000000

    @staticmethod
    def loaded_runtime():
        """Path of the libamdhip64 this process has mapped (torch's), or None."""
        try:
            with open("/proc/self/maps") as f:
                for line in f:
                    path = line.split()[-1]
                    if "/libamdhip64.so" in path:
                        return path
        except OSError:
            pass
        return None

    @classmethod
    def _lib(cls):
        if cls._hip is None:
            import ctypes
            path = cls.loaded_runtime()
            if path is None:
                raise OSError("the HIP runtime is not loaded in this process")
            h = ctypes.CDLL(path)
            h.hipEventCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
            h.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            h.hipEventSynchronize.argtypes = [ctypes.c_void_p]
            h.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p,
                                              ctypes.c_void_p]
            h.hipEventDestroy.argtypes = [ctypes.c_void_p]
            h.hipStreamWaitEvent.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
            cls._hip = h
        return cls._hip

    def __init__(self):
        import ctypes
        self._ev = ctypes.c_void_p()
        rc = self._lib().hipEventCreateWithFlags(ctypes.byref(self._ev), self.DISABLE_SYSTEM_FENCE)
        if rc != 0:
            raise RuntimeError(f"hipEventCreateWithFlags failed ({rc})")

    def record(self, stream):
        rc = self._lib().hipEventRecord(self._ev, stream.cuda_stream)
        if rc != 0:
            raise RuntimeError(f"hipEventRecord failed ({rc})")

    def wait(self, stream):
        """Make `stream` wait for this event's last recorded point (hipStreamWaitEvent)."""
        rc = self._lib().hipStreamWaitEvent(stream.cuda_stream, self._ev, 0)
        if rc != 0:
            raise RuntimeError(f"hipStreamWaitEvent failed ({rc})")

    def elapsed_time(self, end):
        import ctypes
        ms = ctypes.c_float()
        rc = self._lib().hipEventSynchronize(end._ev)
        if rc != 0:
            raise RuntimeError(f"hipEventSynchronize failed ({rc})")
        rc = self._lib().hipEventElapsedTime(ctypes.byref(ms), self._ev, end._ev)
        if rc != 0:
            raise RuntimeError(f"hipEventElapsedTime failed ({rc})")
        return ms.value

    def __del__(self):
        if self._hip is not None and self._ev:
            self._hip.hipEventDestroy(self._ev)


class PhaseTimer:
    """When installed with set_phase_timer(), every engine launch is bracketed by HIP events
    (torch.cuda.Event, recorded on the stream the kernels run on) so kernel durations can be
    measured live (bench.py).  split=True launches the phases of `steps` separately and times
    each: by default SCORE, then SELECT+GATHER (one select_gather kernel, as in an untimed
    call); THREE times SCORE / SELECT / GATHER as separate kernels.  split=False times the
    launch as issued ("all")."""

    DEFAULT = (("score", N.PHASE_SCORE), ("select+gather", N.PHASE_SELECT | N.PHASE_GATHER))
    THREE = (("score", N.PHASE_SCORE), ("select", N.PHASE_SELECT), ("gather", N.PHASE_GATHER))

    def __init__(self, split=True, keep_workspace=False, steps=None, fenceless=False):
        self.split = split
        self.steps = steps or self.DEFAULT
        self.records = []
        self.workspaces = [] if keep_workspace else None  # (ws, info) of each launch (tools)
        torch_event = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
        if fenceless:
            try:
                HipEvent._lib()
            except OSError:
                fenceless = False  # no mapped HIP runtime to call: torch's events
        self.fenceless = fenceless
        self.event = HipEvent if fenceless else torch_event

    def durations_ms(self):
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.records:
            out.setdefault(name, []).append(a.elapsed_time(b))
        return out


_timer = None

# Launch-path switch for tests and tools: False = SCORE + SELECT_GATHER kernels (default), True =
# SCORE, SELECT and GATHER as three kernels (kvc_params.flags KVC_FLAG_SPLIT_SELECT_GATHER).
split_select_gather = False

# Tie policy of the methods' selections (opt-in; not part of the reference).  "reference"
# (default): the reference's first-k sets bit-exactly, libstdc++ tie order included.  "stable":
# tied keys kept in position order -- the first k of argsort(stable=True), for argsort and topk
# callers alike (KVC_ALGO_STABLE: a radix select, no partition chain).  The two differ only
# where a tie straddles the k-th key, i.e. on most bf16 / fp16 rows.  KVC_TIE_POLICY=stable in
# the environment selects it at import, set_tie_policy() at run time.  It covers h2o_attention's
# heavy hitters too (KVC_ATTN_HH_STABLE: the first k of a stable descending sort of the head
# sums).
TIE_POLICIES = ("reference", "stable")
STABLE_MAX_ZONE = 65536  # kvc.h KVC_ALGO_STABLE: the LDS and u16-position global kernels
tie_policy = __import__("os").environ.get("KVC_TIE_POLICY", "reference")
if tie_policy not in TIE_POLICIES:
    raise ValueError(f"KVC_TIE_POLICY={tie_policy!r}: expected one of {TIE_POLICIES}")


def set_tie_policy(policy: str) -> str:
    """Select the tie policy ("reference" or "stable") of later calls; returns the previous one."""
    global tie_policy
    if policy not in TIE_POLICIES:
        raise ValueError(f"tie policy {policy!r}: expected one of {TIE_POLICIES}")
    prev, tie_policy = tie_policy, policy
    return prev


def set_phase_timer(t):
    global _timer
    _timer = t


def _check_tensors(j: Segments):
    """Device / dtype / shape contract of a layer that needs the engine; returns K's shape."""
    k, v = j.keys, j.values
    if not (k.is_cuda and v.is_cuda):
        raise RuntimeError(
            f"kvcompress (MI355X HIP engine): layer {j.layer_idx} needs compression but its K/V "
            f"are on {k.device}/{v.device}; this engine runs on ROCm GPU tensors only "
            "(no CPU fallback).")
    kd = k.dtype
    if kd not in _SUPPORTED or v.dtype != kd:
        raise TypeError(
            f"kvcompress (MI355X HIP engine) supports bfloat16/float16/float32 and fp8 "
            f"(float8_e4m3fn/float8_e5m2) K and V of one dtype; "
            f"layer {j.layer_idx} has {kd}/{v.dtype}")
    shape = k.shape
    if len(shape) != 4 or v.shape != shape:
        raise ValueError(f"layer {j.layer_idx}: K/V must both be [B, H, S, D]; got "
                         f"{tuple(shape)} / {tuple(v.shape)}")
    return shape


def _prep(t):
    """Last dim contiguous and 16-byte aligned rows (else a device-side contiguous copy)."""
    es = t.element_size()
    if t.is_contiguous() and t.data_ptr() % 16 == 0 and (t.size(3) * es) % 16 == 0:
        return t  # the common case, one C call
    ok = (t.stride(3) == 1 and t.data_ptr() % 16 == 0 and
          all((t.stride(d) * es) % 16 == 0 or t.size(d) == 1 for d in range(3)))
    # a fresh allocation is aligned (.contiguous() would return a contiguous-but-misaligned view
    # -- e.g. one at an odd offset into a flat buffer -- as it is)
    return t if ok else t.clone(memory_format=torch.contiguous_format)


def execute(jobs: List[Segments], out_list: list, order: int, algo: int):
    if not jobs:
        return
    if tie_policy == "stable":
        algo = N.KVC_ALGO_STABLE
        for j in jobs:
            if (0 < j.n_select < j.zone_len and j.ext_index is None and
                    j.zone_len > STABLE_MAX_ZONE):
                raise ValueError(f"kvcompress: the stable tie policy selects from zones of at most "
                                 f"{STABLE_MAX_ZONE} positions (layer {j.layer_idx}: "
                                 f"{j.zone_len}); use the reference policy for longer zones")
    if _defer(jobs, lambda: execute(jobs, out_list, order, algo), out_list, (order, algo)):
        return  # a call with `out`: dest_call() launches once every destination is checked
    if jobs[0].paged is not None:  # compress_paged's jobs, checked by it
        from .paged import run_jobs
        run_jobs(jobs, order, algo)
        return
    jobs, dest_jobs = _split_dest_jobs(jobs)
    for j in dest_jobs:  # jobs that carry destinations of their own (no `out` call in progress)
        _check_dest(j)
    if dest_jobs:
        _run_dest(dest_jobs, out_list, order, algo)
        if not jobs:
            return
    fast = _one_plain_group(jobs)
    if fast is not None:
        _run_plain(*fast, jobs, out_list, order, algo)
        return
    groups = {}
    for j in jobs:
        B, H, _, D = _check_tensors(j)
        groups.setdefault((j.keys.get_device(), j.keys.dtype, B, H, D), []).append(j)
    for (device, dtype, B, H, D), js in groups.items():
        _run_group(device, dtype, B, H, D, js, out_list, order, algo)


def _one_plain_group(jobs):
    """The common call in ONE pass over its layers: every layer's K/V on one ROCm device, one
    supported dtype, one (B, H, D), plain contiguous, engine-selected.  Returns the group key,
    the K/V data pointers and the per-layer (S, segment bounds) -- or None for anything else
    (the general path then checks and groups every layer)."""
    k0 = jobs[0].keys
    dt, shape0 = k0.dtype, k0.shape
    if dt not in _SUPPORTED or len(shape0) != 4 or not k0.is_cuda:
        return None
    B, H, _, D = shape0
    if (D * _ESIZE[dt]) % 16:
        return None
    dev = k0.get_device()
    kps, vps, segs = [], [], []
    for j in jobs:
        k, v = j.keys, j.values
        ks = k.shape
        if (j.ext_index is not None or k.dtype is not dt or v.dtype is not dt or
                v.shape != ks or len(ks) != 4 or ks[0] != B or ks[1] != H or ks[3] != D or
                not (k.is_contiguous() and v.is_contiguous()) or k.get_device() != dev or
                v.get_device() != dev):
            return None
        kp, vp = k.data_ptr(), v.data_ptr()
        if (kp | vp) & 15:  # e.g. a contiguous view at an odd offset: the general path copies
            return None
        kps.append(kp)
        vps.append(vp)
        segs.append((ks[2], j.zone_start, j.zone_len, j.n_select, j.sink_len, j.tail_start,
                     j.tail_len, j.pool_kernel, j.score_mode))
    return dev, dt, B, H, D, kps, vps, segs


def _upload(params, table, device, js, B, H, tables=None):
    """Plan one table -- with the call's optional tables, an N.Tables; a dense call has none --
    and allocate its workspace.  The table itself travels in the kernels' arguments;
    caller-provided indices (strategy="random") are copied into the index region here."""
    if tables is None:
        rc, info = N.plan(params, table)
        N.check(rc, "kvc_plan")
    else:
        rc, info = tables.plan(params, table)
        N.check(rc, tables.plan_name)
    ws = torch.empty(max(int(info.workspace_bytes), 256), dtype=torch.uint8, device=device)
    if params.external_index:
        istride = int(info.index_row_stride)
        iv = ws[info.index_offset:info.index_offset + int(info.rows) * istride * 4]
        iv = iv.view(torch.int32).view(int(info.rows), istride)
        for i, j in enumerate(js):
            if j.n_select:
                iv[i * B * H:(i + 1) * B * H, :j.n_select].copy_(
                    j.ext_index.reshape(B * H, j.n_select))
    return ws, info


def _launch(params, table, ws, info, stream, phases, tables=None):
    _touch(ws.get_device())  # a cached plan's Params makes no status_word() call
    # the entry point of the call's tables, resolved once for all of its timed phases
    launch, what = (N.launch, "kvc_launch") if tables is None else \
        (tables.launch, tables.launch_name)
    saved = params.phases
    steps = _timer.steps if _timer is not None and _timer.split else (("all", phases),)
    for name, bits in steps:
        if not phases & bits:
            continue
        params.phases = bits & phases
        if _timer is not None:
            a, b = _timer.event(), _timer.event()
            a.record(stream)
        rc = launch(params, table, ws.data_ptr(), int(info.workspace_bytes), stream.cuda_stream)
        if _timer is not None:
            b.record(stream)
        N.check(rc, what)
        if _timer is not None:
            _timer.records.append((name, a, b))
    params.phases = saved


class _PlanCache:
    """Plans of recent call shapes, so that a repeated call (the per-token decode step: same
    layer count, shapes and segment bounds every step) skips kvc_plan, the layer-table build and
    the workspace allocation and only writes the four pointer columns of its table.

    Key: (device, stream, dtype, B, H, D, order, algo, split flag, per-layer (S, segments)) of a
    group whose K/V are plain contiguous tensors.  Value: the planned table (pointer columns
    zero), kvc_plan_info, the workspace and the params.  A workspace is reused only by calls on
    the SAME stream, which are ordered behind the kernels that used it before.  Calls with
    caller-provided indices (strategy="random") are not cached: their workspace holds per-call
    data.  A call inside a CUDA graph capture may take its table from here but never its
    workspace, and adds no entry ("CUDA graphs").

    Memory: a shape is cached on its SECOND sighting (a one-off call -- a prefill, a decode step
    whose S grows every token -- keeps no workspace), at most `capacity` entries and `max_bytes`
    of workspace are held (least recently used first out), and clear() releases them all."""

    def __init__(self, capacity=8, max_bytes=1 << 30, seen_capacity=64):
        self.capacity = capacity
        self.max_bytes = max_bytes
        self.seen_capacity = seen_capacity
        self.entries = {}
        self.seen = {}
        self.bytes = 0

    def get(self, key):
        e = self.entries.get(key)
        if e is None:
            return None
        if len(self.entries) > 1:  # most recently used last
            del self.entries[key]
            self.entries[key] = e
        return e[0]

    def admit(self, key):
        """True on a key's second sighting (the caller then plans and put()s it)."""
        if key in self.seen:
            del self.seen[key]
            return True
        if len(self.seen) >= self.seen_capacity:
            del self.seen[next(iter(self.seen))]
        self.seen[key] = None
        return False

    def put(self, key, entry, nbytes):
        if nbytes > self.max_bytes:
            return
        while self.entries and (len(self.entries) >= self.capacity or
                                self.bytes + nbytes > self.max_bytes):
            old = self.entries.pop(next(iter(self.entries)))
            self.bytes -= old[1]
        self.entries[key] = (entry, nbytes)
        self.bytes += nbytes

    def clear(self):
        self.entries.clear()
        self.seen.clear()
        self.bytes = 0


plan_cache = _PlanCache()


_status_words = {}


def status_word(device):
    """The per-device word the kernels OR enum kvc_device_status bits into (zeroed once; sticky).
    Read it with device_status()."""
    w = _status_words.get(device)
    if w is None:
        _not_while_capturing("status word", device)
        w = _status_words[device] = _new_status_word(device)
    _touch(device)
    return w


def _not_while_capturing(what, device):
    """The engine's per-device objects (the status word, the side stream and its events) are made
    on first use and live for the process.  Made inside a CUDA graph capture, the word would be
    graph-pool memory that every replay zeroes again, and a stream or event creation can
    invalidate the capture: the first engine call on a device belongs to the warm-up
    ("CUDA graphs")."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(
            f"kvcompress (MI355X HIP engine): the first engine call on cuda:{device} came inside "
            f"a CUDA graph capture, where its {what} cannot be created; make one eager call of "
            "the same kind on this device (the warm-up) before capturing")


def _touch(device):
    """Record a launch on `device`: inside a status-checked call (check on), the outermost call
    reads that device's word at its end.  Every path that enqueues engine kernels calls this --
    _launch, the native replays (kvc_host.run / run_h2o) -- not only the ones that make a word:
    a cached plan carries its word's address in its Params and never asks for it again."""
    t = getattr(_check_state, "touched", None)
    if t is not None:
        t.add(device)


def _new_status_word(device):
    # a normal tensor even when the first call comes inside torch.inference_mode() (the
    # evaluation loops): device_status(clear=True) zeroes it in place from any mode
    with torch.inference_mode(False):
        return torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", device))


def device_status(device=None, clear=False):
    """Synchronises `device` and returns the kvc_device_status bits its kernels have reported
    since the last clear (0 = none).  KVC_DEV_SELECT_BOUNDS means a selection row's output is
    unspecified; KVC_DEV_INDEX_RANGE that a caller-provided index was clamped into its zone."""
    device = torch.cuda.current_device() if device is None else device
    w = status_word(device)
    v = int(w.item())
    if clear:
        w.zero_()
    return v


# Opt-in production check of the device status word: after every compress call (and every
# h2o_attention manager call) the words of the devices the engine has used are read -- one
# synchronisation per call -- and a non-zero word is cleared and raised as RuntimeError naming its
# bits.  Off by default (the read synchronises the device); KVC_CHECK_STATUS=1 in the environment
# turns it on at import, set_status_check() at run time.
import os as _os

check_status = _os.environ.get("KVC_CHECK_STATUS", "") not in ("", "0")

_STATUS_BITS = ((N.DEV_SELECT_BOUNDS, "KVC_DEV_SELECT_BOUNDS (a selection row exceeded its "
                 "kernel's zone capacity: that row's output was left unwritten)"),
                (N.DEV_INDEX_RANGE, "KVC_DEV_INDEX_RANGE (a caller-provided index lay outside its "
                 "zone and was clamped)"),
                (N.DEV_INTERNAL, "KVC_DEV_INTERNAL (an internal invariant of the selection "
                 "failed: that row's output is unspecified)"))

# Per-thread state of the status check: `depth` counts the status-checked calls in progress
# (h2o_attention_compress calls the manager's checked methods: only the outermost call reads
# the words), `touched` collects the devices the outermost call's launches used.
import threading as _threading

_check_state = _threading.local()


def set_status_check(on: bool = True):
    """Turn the per-call device status check on or off; returns the previous setting."""
    global check_status
    prev, check_status = check_status, bool(on)
    return prev


def raise_on_status(devices=None):
    """Read (and clear) the status words of `devices` (default: every device the engine has
    used); RuntimeError if any bit is set."""
    for device in list(_status_words) if devices is None else sorted(devices):
        if device not in _status_words:
            continue
        v = device_status(device, clear=True)
        if v:
            names = [txt for bit, txt in _STATUS_BITS if v & bit] or [f"unknown bits {v:#x}"]
            raise RuntimeError(f"kvcompress (MI355X HIP engine): cuda:{device} reported "
                               f"device status {v:#x}: " + "; ".join(names))


def _checked_call(call, result_devices=None):
    """Run call() as a status-checked entry point: with check_status on, the OUTERMOST such call
    ends by reading the words of the devices its launches touched (_touch() calls during the
    call, plus `result_devices(out)`).
    No read while a CUDA graph is being captured (the read synchronises)."""
    st = _check_state
    if not check_status or getattr(st, "depth", 0) > 0:
        return call()
    st.depth, st.touched = 1, set()
    try:
        out = call()
        touched = st.touched
    finally:
        st.depth, st.touched = 0, None
    if result_devices is not None:
        touched |= result_devices(out)
    if touched and not torch.cuda.is_current_stream_capturing():
        raise_on_status(touched)
    return out


def _output_devices(out):
    """CUDA devices of the tensors of a compress result (a list of (K, V) pairs)."""
    devs = set()
    for kv in out if isinstance(out, (list, tuple)) else ():
        for t in kv if isinstance(kv, (list, tuple)) else ():
            if isinstance(t, torch.Tensor) and t.is_cuda:
                devs.add(t.get_device())
    return devs


def status_checked(fn):
    """Wrap an entry point so that, with check_status on, its calls end with a status read."""
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        return _checked_call(lambda: fn(*args, **kwargs))
    return wrapper


def _params(dtype, B, H, D, order, algo, external, shared=False):
    flags = (N.FLAG_SPLIT_SELECT_GATHER if split_select_gather else 0) | \
        (N.FLAG_SHARED_INDEX if shared else 0)
    return N.Params(dtype=_SUPPORTED[dtype], batch=B, heads=H, head_dim=D, order=order,
                    algo=algo, phases=N.PHASE_GATHER if external else N.PHASE_ALL,
                    external_index=1 if external else 0, flags=flags,
                    device_status=status_word(torch.cuda.current_device()).data_ptr())


def _outputs(device, dtype, B, H, D, n_outs):
    """Fresh contiguous [B,H,n_out,D] K and V per layer, and their data pointers.  All outputs
    of a call share one allocation (decode steps: 64 tensors per token; one torch.empty per
    tensor was most of pyramid_kv's host time); each layer's K / V is a disjoint contiguous view
    of it ("Output tensors")."""
    n = len(n_outs)
    if all(x == n_outs[0] for x in n_outs):
        buf = torch.empty((2 * n, B, H, n_outs[0], D), dtype=dtype, device=device)
        o = buf.unbind(0)
        step = B * H * n_outs[0] * D * _ESIZE[dtype]
        offs = np.arange(2 * n, dtype=np.uint64) * np.uint64(step) + np.uint64(buf.data_ptr())
        return o[:n], o[n:], offs[:n], offs[n:]
    sizes = [B * H * x * D for x in n_outs] * 2  # K outputs, then V outputs
    buf = torch.empty(sum(sizes), dtype=dtype, device=device)
    parts = buf.split(sizes)
    shapes = [(B, H, x, D) for x in n_outs] * 2
    o = [t.view(s) for t, s in zip(parts, shapes)]
    offs = np.concatenate(([0], np.cumsum(sizes[:-1]))).astype(np.uint64)
    offs = offs * np.uint64(_ESIZE[dtype]) + np.uint64(buf.data_ptr())
    return o[:n], o[n:], offs[:n], offs[n:]


def _run_plain(device, dtype, B, H, D, kps, vps, segs, js, out_list, order, algo):
    """One launch for a plain group (see _one_plain_group), its plan taken from plan_cache."""
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device)
        key = (device, stream.cuda_stream, dtype, B, H, D, order, algo, split_select_gather,
               tuple(segs))
        entry = plan_cache.get(key)
        # A captured call owns its workspace: the graph keeps the raw pointer, so it must be
        # memory of the graph's pool (allocated during the capture), never a cached workspace
        # that eviction or clear() can hand back to the allocator and that eager calls on this
        # stream go on using.  The planned table template is reused; nothing is cached.
        capturing = torch.cuda.is_current_stream_capturing()
        if entry is None:
            entry = _plan_plain(dtype, B, H, D, order, algo, segs)
            if entry is None:  # rejected by kvc_plan (e.g. misaligned): general path reports
                _run_general(device, dtype, B, H, D, js, out_list, order, algo, False, stream)
                return
            if not capturing and plan_cache.admit(key):
                plan_cache.put(key, entry, int(entry[2].numel()))
        elif capturing:
            entry = entry[:2] + (torch.empty_like(entry[2]),) + entry[3:]
        tmpl, info, ws, p, n_outs = entry
        if _recording is not None:
            _recording.append((stream.cuda_stream, tmpl, info, ws, p, n_outs,
                               [j.layer_idx for j in js]))
        kos, vos, kops, vops = _outputs(device, dtype, B, H, D, n_outs)
        table = tmpl.copy()
        table["k"] = kps
        table["v"] = vps
        table["k_out"] = kops
        table["v_out"] = vops
        _launch(p, table, ws, info, stream, p.phases)
        if _timer is not None and _timer.workspaces is not None:
            _timer.workspaces.append((ws, info))
    for j, ko, vo in zip(js, kos, vos):
        out_list[j.layer_idx] = (ko, vo)


def _run_group(device, dtype, B, H, D, js, out_list, order, algo):
    if _recording is not None:
        _recording.append(None)  # a general-path launch: this call shape is not replayable
    external = any(j.ext_index is not None for j in js)
    if external and not all(j.ext_index is not None or j.n_select == 0 for j in js):
        raise RuntimeError("mixed external / engine-selected layers in one group")
    with torch.cuda.device(device):
        _run_general(device, dtype, B, H, D, js, out_list, order, algo, external,
                     torch.cuda.current_stream(device))


def _plan_plain(dtype, B, H, D, order, algo, segs):
    """Planned table template of a plain-contiguous group (pointer columns zero), or None when
    kvc_plan rejects it (the general path then reports the error)."""
    table = np.zeros(len(segs), dtype=N.LAYER_DTYPE)
    arr = np.array(segs, dtype=np.int64).reshape(len(segs), 9)
    S = arr[:, 0]
    st = np.stack([H * S * D, S * D, np.full_like(S, D)], axis=1)
    table["k_stride"] = st
    table["v_stride"] = st
    for c, name in enumerate(("seq_len", "zone_start", "zone_len", "n_select", "sink_len",
                              "tail_start", "tail_len", "pool_kernel", "score_mode")):
        table[name] = arr[:, c]
    n_outs = [int(x) for x in arr[:, 4] + arr[:, 3] + arr[:, 6]]
    # plan with stand-in 16-B aligned pointers: the real ones are checked at launch
    for name in ("k", "v", "k_out", "v_out"):
        table[name] = 256
    p = _params(dtype, B, H, D, order, algo, False)
    rc, info = N.plan(p, table)
    if rc != 0:
        return None
    for name in ("k", "v", "k_out", "v_out"):
        table[name] = 0
    ws = torch.empty(max(int(info.workspace_bytes), 256), dtype=torch.uint8,
                     device=torch.cuda.current_device())
    return table, info, ws, p, n_outs


def _build_table(device, dtype, B, H, D, js, dest=False):
    """Layer table of a group (pointers, strides, segment bounds) and its output tensors; `keep`
    holds prepared (contiguous) input copies alive until the launch has been issued.  dest=True
    (every job carries a destination): the outputs are rows [0, n_out) of the jobs' k_dest /
    v_dest, whose strides _dest_table() puts into the kvc_dest_t array."""
    es = _ESIZE[dtype]
    rows_ok = (D * es) % 16 == 0
    n_outs = [j.sink_len + j.n_select + j.tail_len for j in js]
    if dest:
        kos = [j.k_dest.narrow(2, 0, n) for j, n in zip(js, n_outs)]
        vos = [j.v_dest.narrow(2, 0, n) for j, n in zip(js, n_outs)]
        kops, vops = [t.data_ptr() for t in kos], [t.data_ptr() for t in vos]
    else:
        kos, vos, kops, vops = _outputs(device, dtype, B, H, D, n_outs)
    # one pass per layer: pointers, strides, segment bounds (inputs that are not plain
    # contiguous 16-B aligned rows go through _prep; prepared copies stay alive in `keep`)
    rows, keep = [], []
    for i, j in enumerate(js):
        k, v = j.keys, j.values
        kp, vp = k.data_ptr(), v.data_ptr()
        if not (rows_ok and kp % 16 == 0 and k.is_contiguous()):
            k = _prep(k)
            kp = k.data_ptr()
            keep.append(k)
        if not (rows_ok and vp % 16 == 0 and v.is_contiguous()):
            v = _prep(v)
            vp = v.data_ptr()
            keep.append(v)
        kst, vst = k.stride(), v.stride()
        rows.append((kp, vp, int(kops[i]), int(vops[i]), kst[:3], vst[:3], k.shape[2],
                     j.zone_start, j.zone_len, j.n_select, j.sink_len, j.tail_start, j.tail_len,
                     j.pool_kernel, j.score_mode, 0, 0, 0, 0))
    return np.array(rows, dtype=N.LAYER_DTYPE), kos, vos, keep


_side = {}


def side_stream(device):
    """(stream, fork event, join event) of `device` for copies that overlap the current
    stream's work (created once; the events have no timing and no system fence)."""
    e = _side.get(device)
    if e is None:
        _not_while_capturing("side stream", device)
        with torch.cuda.device(device):
            e = (torch.cuda.Stream(device), HipEvent(), HipEvent())
        _side[device] = e
    return e


def execute_shared(jobs: List[Segments], out_list: list, fill, overlap=False):
    """External-index GATHER whose index row (layer, b) serves every head of the layer
    (KVC_FLAG_SHARED_INDEX: h2o_attention's heavy hitters, one index list per layer).  Per group,
    `fill(js, index_region_ptr, row_stride, stream)` writes row (i * B + b) of job i before the
    copy kernel is enqueued on the same stream.  overlap=True: the sink and tail rows (which no
    index decides) are copied on a side stream forked before `fill` and joined after the selected
    rows' copy (KVC_FLAG_GATHER_FIXED / _SELECTED), so they move while `fill` selects."""
    if _defer(jobs, lambda: execute_shared(jobs, out_list, fill, overlap), out_list):
        return  # a call with `out`: dest_call() launches once every destination is checked
    if _recording is not None:
        _recording.append(None)
    for j in jobs:
        if j.k_dest is not None:
            _check_dest(j)
    groups = {}
    for j in jobs:  # jobs with a destination form groups of their own (no side-stream copy)
        B, H, _, D = _check_tensors(j)
        groups.setdefault((j.keys.get_device(), j.keys.dtype, B, H, D, j.k_dest is not None),
                          []).append(j)
    for (device, dtype, B, H, D, dest), js in groups.items():
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device)
            # (the per-device objects first: made on first use, which raises inside a graph
            # capture before _build_table can enqueue a copy of a misaligned input)
            p = _params(dtype, B, H, D, N.KVC_ASC, N.KVC_ALGO_SORT, True, shared=True)
            side = side_stream(device) if overlap and _timer is None and not dest else None
            table, kos, vos, keep = _build_table(device, dtype, B, H, D, js, dest)
            dests = _dest_table(js, table) if dest else None
            rc, info = N.plan_dest(p, table, dests) if dest else N.plan(p, table)
            N.check(rc, "kvc_plan_dest" if dest else "kvc_plan")
            ws = torch.empty(max(int(info.workspace_bytes), 256), dtype=torch.uint8,
                             device=torch.device("cuda", device))
            if side is not None:
                pf = _params(dtype, B, H, D, N.KVC_ASC, N.KVC_ALGO_SORT, True, shared=True)
                pf.flags |= N.FLAG_GATHER_FIXED
                p.flags |= N.FLAG_GATHER_SELECTED
                side[1].record(stream)
                side[1].wait(side[0])
            try:
                if side is not None:
                    _launch(pf, table, ws, info, side[0], pf.phases)
                fill(js, ws.data_ptr() + int(info.index_offset), int(info.index_row_stride),
                     stream)
                _launch(p, table, ws, info, stream, p.phases, N.Tables(dests) if dest else None)
            finally:
                if side is not None:  # `stream` continues only after the side copy, on every
                    side[2].record(side[0])  # exit path (outputs and workspace are freed on it)
                    side[2].wait(stream)
            del keep
        for j, ko, vo in zip(js, kos, vos):
            out_list[j.layer_idx] = (ko, vo)


# ---------------------------------------------------------------------------------------------
# Caller-provided destinations (kvc_plan_dest / kvc_launch_dest; INTEGRATION.md, "Destinations")
# ---------------------------------------------------------------------------------------------
_dest_state = _threading.local()  # .ctx: the _DestCall of the compress call in progress


class _DestCall:
    """Destinations of one compress call (the `out` kwarg): per layer "inplace", a (K_dst, V_dst)
    pair or None.  While the method runs, execute() / execute_shared() launch nothing: they give
    every job its layer's destination and park the launch in `pending` [(jobs, run, out_list)];
    `done` collects the layers whose engine job took its destination.  `rollback` holds what undoes
    the method's side effects (h2o_attention's manager update) when a check then fails.  `how[i]`
    is the (order, algo) of pending[i], or None for a launch with caller-provided indices."""
    __slots__ = ("dests", "done", "pending", "rollback", "how")

    def __init__(self, dests):
        self.dests, self.done, self.pending, self.rollback = dests, set(), [], []
        self.how = []


def dest_call_active():
    """True inside a compress call that carries destinations (such calls bypass the call memo,
    the plan cache and h2o_attention's step replay)."""
    return getattr(_dest_state, "ctx", None) is not None


def on_dest_error(undo):
    """Inside a call with `out`: register undo() to run if the call raises before it launches."""
    ctx = getattr(_dest_state, "ctx", None)
    if ctx is not None:
        ctx.rollback.append(undo)


def _defer(jobs, run, out_list, how=None):
    """Inside a call with `out` (dest_call): give the jobs their layers' destinations, park the
    launch (and its (order, algo), when the engine selects) and return True; otherwise False."""
    ctx = getattr(_dest_state, "ctx", None)
    if ctx is None:
        return False
    for j in jobs:
        d = ctx.dests[j.layer_idx] if j.k_dest is None else None
        if d is not None:
            j.k_dest, j.v_dest = (j.keys, j.values) if d == "inplace" else d
            j.dest_checked = True
            ctx.done.add(j.layer_idx)
    ctx.pending.append((jobs, run, out_list))
    ctx.how.append(how)
    return True


def _split_dest_jobs(jobs):
    """(jobs without, jobs with a destination)."""
    plain = [j for j in jobs if j.k_dest is None]
    if len(plain) == len(jobs):
        return jobs, []
    return plain, [j for j in jobs if j.k_dest is not None]


def _takes_as_is(t):
    """_prep's conditions without the copy: last dim contiguous, 16-B aligned pointer and strides."""
    es = t.element_size()
    return ((t.stride(3) == 1 or t.size(3) == 1) and t.data_ptr() % 16 == 0 and
            (t.size(3) * es) % 16 == 0 and
            all((t.stride(d) * es) % 16 == 0 or t.size(d) == 1 for d in range(3)))


def _is_inplace(src, dst):
    return dst is src or (dst.data_ptr() == src.data_ptr() and dst.stride() == src.stride()
                          and dst.shape == src.shape)


def _check_dest_tensors(li, k, v, kd, vd):
    """Everything about layer `li`'s destination that does not depend on the output length.
    Raises ValueError / TypeError naming the layer; nothing is copied or enqueued."""
    for name, src, dst in (("K", k, kd), ("V", v, vd)):
        what = f"layer {li}: {name} destination"
        if not isinstance(dst, torch.Tensor):
            raise TypeError(f"{what} must be a tensor, got {type(dst).__name__}")
        if _is_inplace(src, dst):
            if not _takes_as_is(src):
                raise ValueError(
                    f"layer {li}: {name} cannot be compacted in place: the engine would have to "
                    "copy it first (last dim not contiguous, or a pointer / stride that is not "
                    "a multiple of 16 bytes)")
            if any(src.stride(d) == 0 and src.size(d) > 1 for d in range(3)):
                raise ValueError(f"layer {li}: {name} cannot be compacted in place: stride 0 on "
                                 "a dim larger than 1 (an expanded tensor would be written twice)")
            continue
        if dst.dtype != src.dtype:
            raise TypeError(f"{what} has dtype {dst.dtype}, the layer {src.dtype}")
        if dst.dim() != 4 or src.dim() != 4 or (dst.shape[0], dst.shape[1], dst.shape[3]) != \
                (src.shape[0], src.shape[1], src.shape[3]):
            raise ValueError(f"{what} must be [B, H, S_d, D] with the layer's B, H, D "
                             f"{tuple(src.shape)}; got {tuple(dst.shape)}")
        if dst.stride(3) != 1 and dst.size(3) > 1:
            raise ValueError(f"{what}: the last dim must be contiguous (stride "
                             f"{dst.stride(3)})")
        es = dst.element_size()
        if any((dst.stride(d) * es) % 16 and dst.size(d) > 1 for d in range(3)) or \
                (dst.size(3) * es) % 16:
            raise ValueError(f"{what}: strides {tuple(dst.stride())} are not multiples of 16 "
                             "bytes (a destination is never copied)")
        if dst.device != src.device:
            raise ValueError(f"{what} is on {dst.device}, the layer on {src.device}")
        if dst.data_ptr() % 16:
            raise ValueError(f"{what}: pointer not 16-byte aligned (a destination is never "
                             "copied)")
    if _is_inplace(k, kd) != _is_inplace(v, vd):
        raise ValueError(f"layer {li}: K and V must both be compacted in place or neither")


def _span(t, n):
    """Byte span [lo, hi) of rows [0, n) of a [B, H, S, D] view (kvc_plan_dest's span)."""
    es = t.element_size()
    ext = [(sz - 1) * st * es for sz, st in ((t.size(0), t.stride(0)), (t.size(1), t.stride(1)),
                                             (n, t.stride(2)))]
    lo = t.data_ptr() + sum(e for e in ext if e < 0)
    return lo, t.data_ptr() + sum(e for e in ext if e > 0) + t.size(3) * es


def _check_dest(j: Segments):
    """The destination of one job: _check_dest_tensors, then what depends on its segments.
    (compress_paged does not call this for a job with a PagedDest: its k_dest / v_dest are
    stride-0 stand-ins that say nothing about memory, so the span checks below would compare
    meaningless addresses; paged.py checks the table's capacity and the pools' spans itself.)"""
    if j.dest_verified:
        return
    li, k, v = j.layer_idx, j.keys, j.values
    if not j.dest_checked:
        _check_dest_tensors(li, k, v, j.k_dest, j.v_dest)
    n = j.sink_len + j.n_select + j.tail_len
    if n == 0:
        return
    if _is_inplace(k, j.k_dest):
        if k.data_ptr() == v.data_ptr():
            raise ValueError(f"layer {li}: K and V share their memory: not compacted in place")
        ordered = ((j.n_select == 0 or j.sink_len <= j.zone_start) and
                   (j.tail_len == 0 or (j.zone_start + j.zone_len <= j.tail_start and
                                        j.sink_len <= j.tail_start)))
        if not ordered:
            raise ValueError(
                f"layer {li}: cannot be compacted in place: its segments (sink {j.sink_len}, zone "
                f"[{j.zone_start}, {j.zone_start + j.zone_len}), tail [{j.tail_start}, "
                f"{j.tail_start + j.tail_len})) overlap or are out of order (e.g. "
                "streaming_llm with recent_size=0, whose result is longer than its input)")
        return
    for name, dst in (("K", j.k_dest), ("V", j.v_dest)):
        if dst.size(2) < n:
            raise ValueError(f"layer {li}: {name} destination holds {dst.size(2)} rows, the "
                             f"result has {n}")
        lo, hi = _span(dst, n)
        for sname, src in (("K", k), ("V", v)):
            slo, shi = _span(src, src.size(2))
            if lo < shi and slo < hi:
                raise ValueError(f"layer {li}: {name} destination overlaps the layer's {sname} "
                                 "(use out=\"inplace\" to compact a cache onto itself)")


def _dest_table(js, table):
    """kvc_dest_t array of a group whose layer table _build_table(dest=True) made."""
    dests = np.zeros(len(js), dtype=N.DEST_DTYPE)
    for i, j in enumerate(js):
        inplace = _is_inplace(j.keys, j.k_dest)
        # an in-place layer's strides are its (possibly size-1-dim-normalised) input strides
        dests[i] = ((table["k_stride"][i] if inplace else j.k_dest.stride()[:3]),
                    (table["v_stride"][i] if inplace else j.v_dest.stride()[:3]),
                    1 if inplace else 0, 0)
    return dests


def _run_dest(jobs, out_list, order, algo):
    """The jobs of a call that carry destinations (checked by the caller): one kvc_launch_dest
    per (device, dtype, B, H, D) group.  No plan cache, and never recorded for the call memo."""
    if _recording is not None:
        _recording.append(None)
    groups = {}
    for j in jobs:
        B, H, _, D = _check_tensors(j)
        groups.setdefault((j.keys.get_device(), j.keys.dtype, B, H, D), []).append(j)
    for (device, dtype, B, H, D), js in groups.items():
        external = any(j.ext_index is not None for j in js)
        if external and not all(j.ext_index is not None or j.n_select == 0 for j in js):
            raise RuntimeError("mixed external / engine-selected layers in one group")
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device)
            p = _params(dtype, B, H, D, order, algo, external)  # first: see execute_shared
            table, kos, vos, keep = _build_table(device, dtype, B, H, D, js, True)
            dests = N.Tables(_dest_table(js, table))
            ws, info = _upload(p, table, device, js, B, H, dests)
            _launch(p, table, ws, info, stream, p.phases, dests)
            if _timer is not None and _timer.workspaces is not None:
                _timer.workspaces.append((ws, info))
            del keep
        for j, ko, vo in zip(js, kos, vos):
            out_list[j.layer_idx] = (ko, vo)


def _run_general(device, dtype, B, H, D, js, out_list, order, algo, external, stream):
    p = _params(dtype, B, H, D, order, algo, external)  # first: see execute_shared
    table, kos, vos, keep = _build_table(device, dtype, B, H, D, js)
    # One launch (score, select, gather kernels) for every layer of the group.  (Pipelining
    # layer chunks over two streams -- score of chunk c+1 beside select of chunk c -- was
    # measured slower at 2/4/8 chunks: profiles/r01_pipeline_sweep.json.)
    ws, info = _upload(p, table, device, js, B, H)
    _launch(p, table, ws, info, stream, p.phases)
    if _timer is not None and _timer.workspaces is not None:
        _timer.workspaces.append((ws, info))
    for j, ko, vo in zip(js, kos, vos):
        out_list[j.layer_idx] = (ko, vo)


# ---------------------------------------------------------------------------------------------
# Call memo: repeated call shapes replayed by the native host path (csrc/kvc_host.cpp)
# ---------------------------------------------------------------------------------------------
_recording = None  # list while a call is being recorded: one entry per engine launch
_host = None


def host_module():
    """kvc_host.so (built by __graft_entry__.build()), or None when it is not there -- calls then
    take the method's Python path (same engine, same results, more host time per call)."""
    global _host
    if _host is None:
        import importlib.util
        import os
        path = os.path.join(os.path.dirname(N.LIB_PATH), "kvc_host.so")
        _host = False
        # kvc_host.so links the default libkvc.so: a swapped-in build (KVC_LIB, A/B runs) keeps
        # every call on the ctypes path so that all launches use the same library
        if os.path.exists(path) and os.path.basename(N.LIB_PATH) == "libkvc.so":
            spec = importlib.util.spec_from_file_location("kvc_host", path)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            _host = mod
    return _host or None


def _freeze(x):
    if isinstance(x, (list, tuple)):
        return tuple(_freeze(y) for y in x)
    if isinstance(x, (int, float, str, bool, type(None))):
        return x
    raise TypeError  # anything else (a manager object, a tensor): not memoised


class _Replay:
    __slots__ = ("actions", "table", "n_jobs", "n_outs", "params", "ws", "ws_bytes", "keep")


def _slice_of(inp, res):
    """(start, length) when the (K, V) pair `res` is the dim-2 slice [start, start + length) of
    the input pair `inp` (same storage, same strides), else None."""
    k, v = inp
    rk, rv = res
    st = k.stride(2)
    if (rk.untyped_storage().data_ptr() != k.untyped_storage().data_ptr() or
            rk.shape[:2] != k.shape[:2] or rk.shape[3] != k.shape[3] or
            rk.stride() != k.stride() or st == 0 or
            (rk.storage_offset() - k.storage_offset()) % st):
        return None
    start = (rk.storage_offset() - k.storage_offset()) // st
    if not (rv.untyped_storage().data_ptr() == v.untyped_storage().data_ptr() and
            rv.shape == rk.shape and rv.stride() == v.stride() and
            rv.storage_offset() - v.storage_offset() == start * v.stride(2)):
        return None
    return start, rk.shape[2]


def _record(kvl, out, launches):
    """A _Replay of one recorded call, or None when the call is not replayable (a general-path
    launch, more than one launch, or a layer that is neither passed through, a dim-2 slice of
    its input, nor an engine output)."""
    if len(launches) > 1 or any(x is None for x in launches):
        return None
    job_of = {}
    rec = _Replay()
    rec.table, rec.n_jobs, rec.n_outs, rec.params, rec.ws, rec.ws_bytes = 0, 0, [], None, None, 0
    if launches:
        _, tmpl, info, ws, p, n_outs, layer_ids = launches[0]
        job_of = {li: j for j, li in enumerate(layer_ids)}
        rec.table, rec.n_jobs = tmpl.ctypes.data, len(tmpl)
        rec.n_outs, rec.params, rec.ws = [int(x) for x in n_outs], p, ws
        rec.ws_bytes = int(info.workspace_bytes)
        rec.keep = (tmpl, info, ws, p)
    acts = np.zeros((len(kvl), 3), dtype=np.int64)
    for i, (inp, res) in enumerate(zip(kvl, out)):
        if res is inp:
            continue
        if i in job_of:
            acts[i] = (2, job_of[i], 0)
            continue
        sl = _slice_of(inp, res)
        if sl is None:
            return None
        acts[i] = (1, sl[0], sl[1])
    rec.actions = acts
    return rec


call_memo = _PlanCache(capacity=16)
memo_stats = {"replayed": 0, "recorded": 0}


def memoized(fn):
    """Wrap a compress function: a call shape seen before (same function, arguments, per-layer
    shapes / dtype / device / stream) is replayed by kvc_host.run -- one C++ call that fills the
    recorded launch's pointers, allocates the outputs and enqueues the kernels -- instead of
    re-running the reference's per-layer branch logic in Python.  The first sightings run `fn`
    itself; the second records what it did (per layer: passed through, sliced, or engine
    output, and the engine launch's plan).  Results are identical either way."""
    import functools

    @functools.wraps(fn)
    def wrapper(past_key_values, *args, **kwargs):
        out = kwargs.pop("out", None)  # extension kwarg: destinations (dest_call)
        if out is not None:
            return _checked_call(lambda: dest_call(fn, past_key_values, out, args, kwargs),
                                 _output_devices)
        return _checked_call(lambda: _memo_call(past_key_values, *args, **kwargs),
                             _output_devices)

    def _memo_call(past_key_values, *args, **kwargs):
        global _recording
        hm = host_module()
        if hm is None or _timer is not None or _recording is not None:
            return fn(past_key_values, *args, **kwargs)
        from .utils import normalize_kv_cache
        kvl = list(normalize_kv_cache(past_key_values))
        sig = hm.scan(kvl)
        if sig is None:
            return fn(kvl, *args, **kwargs)
        try:
            key = (fn, _freeze(args), _freeze(sorted(kwargs.items())), split_select_gather,
                   tie_policy, torch.cuda.current_stream(sig[4]).cuda_stream, sig)
        except TypeError:
            return fn(kvl, *args, **kwargs)
        rec = call_memo.get(key)
        # inside a CUDA graph capture the replay takes a workspace of the graph's own pool (see
        # _run_plain) and a shape not recorded yet runs `fn` without being recorded
        capturing = torch.cuda.is_current_stream_capturing()
        if rec is not None:
            memo_stats["replayed"] += 1
            if rec.n_jobs:
                _touch(sig[4])
            ws = torch.empty_like(rec.ws) if capturing and rec.n_jobs else rec.ws
            if rec.n_jobs and torch.cuda.current_device() != sig[4]:
                with torch.cuda.device(sig[4]):
                    return hm.run(kvl, rec.actions, rec.table, rec.n_jobs, rec.n_outs,
                                  ctypes_addr(rec.params), ws.data_ptr(), rec.ws_bytes,
                                  key[5])
            return hm.run(kvl, rec.actions, rec.table, rec.n_jobs, rec.n_outs,
                          ctypes_addr(rec.params) if rec.n_jobs else 0,
                          ws.data_ptr() if rec.n_jobs else 0, rec.ws_bytes, key[5])
        if capturing or not call_memo.admit(key):
            return fn(kvl, *args, **kwargs)
        _recording = []
        try:
            out = fn(kvl, *args, **kwargs)
            launches = _recording
        finally:
            _recording = None
        rec = _record(kvl, out, launches)
        if rec is not None and all(l[0] == key[5] for l in launches):
            call_memo.put(key, rec, rec.ws_bytes)
            memo_stats["recorded"] += 1
        return out
    return wrapper


def ctypes_addr(obj):
    import ctypes
    return ctypes.addressof(obj)


# ---------------------------------------------------------------------------------------------
# The `out` kwarg of every compress function ("Destinations")
# ---------------------------------------------------------------------------------------------
def with_out(fn):
    """Give a compress entry point that is not `memoized` the `out` kwarg (dest_call)."""
    import functools

    @functools.wraps(fn)
    def wrapper(past_key_values, *args, **kwargs):
        out = kwargs.pop("out", None)
        if out is None:
            return fn(past_key_values, *args, **kwargs)
        return _checked_call(lambda: dest_call(fn, past_key_values, out, args, kwargs),
                             _output_devices)
    return wrapper


def dest_call(fn, past_key_values, out, args, kwargs):
    """fn(past_key_values, *args, **kwargs) with its results written where `out` says.

    out="inplace": every layer the call changes is compacted at the front of its own K / V
    memory and comes back as (k.narrow(2, 0, n), v.narrow(2, 0, n)); untouched layers come back
    as the same objects.  out=[(K_dst, V_dst) | None, ...], one entry per layer: a layer with an
    entry ends up in K_dst[:, :, :n] / V_dst[:, :, :n] whatever the method does with it
    (gathered, sliced or left alone -- the latter two are copied); None = the default behaviour,
    "inplace" = that layer as under out="inplace".

    The call runs `fn` itself (no call memo, no plan cache, no step replay) with the
    destinations visible to execute() / execute_shared(), then moves the layers that came back
    as the input or as a slice of it with copy-only engine jobs."""
    from .utils import normalize_kv_cache
    kvl = list(normalize_kv_cache(past_key_values))
    L = len(kvl)
    if isinstance(out, str):
        if out != "inplace":
            raise ValueError(f"out={out!r}: expected None, \"inplace\" or a list with one "
                             "(K_dst, V_dst) pair or None per layer")
        dests = ["inplace"] * L
    elif isinstance(out, (list, tuple)):
        if len(out) != L:
            raise ValueError(f"out has {len(out)} entries for {L} layers")
        dests = []
        for i, d in enumerate(out):
            if d is None or (isinstance(d, str) and d == "inplace"):
                dests.append(d)
                continue
            if not (isinstance(d, (list, tuple)) and len(d) == 2):
                raise TypeError(f"layer {i}: out entry must be a (K_dst, V_dst) pair, "
                                "\"inplace\" or None")
            dests.append(tuple(d))
    else:
        raise TypeError(f"out must be None, \"inplace\" or a list, got {type(out).__name__}")
    seen = {}
    for i, ((k, v), d) in enumerate(zip(kvl, dests)):  # before anything is enqueued
        if d is None:
            continue
        kd, vd = (k, v) if d == "inplace" else d
        _check_dest_tensors(i, k, v, kd, vd)
        if d == "inplace" and k.numel() and v.numel():
            for name, t in (("K", k), ("V", v)):
                ptr = t.data_ptr()
                if ptr in seen:
                    raise ValueError(f"layer {i}: {name} shares its memory with {seen[ptr]}: "
                                     "not compacted in place")
                seen[ptr] = f"layer {i}'s {name}"
    res, moves, ctx = _deferred(fn, kvl, dests, args, kwargs)
    with _rolled_back(ctx):
        # every job of the call -- the method's and the copies -- is checked before any launches
        every = [j for jobs, _, _ in ctx.pending for j in jobs] + moves
        for j in every:
            if j.k_dest is not None:
                _check_dest(j)
                j.dest_verified = True
        for j in every:
            _check_tensors(j)
    for jobs, run, out_list in ctx.pending:
        run()
        if out_list is not res:
            for j in jobs:
                res[j.layer_idx] = out_list[j.layer_idx]
    execute(moves, res, N.KVC_ASC, N.KVC_ALGO_SORT)
    return res


@contextlib.contextmanager
def _rolled_back(ctx):
    """The reach of a deferred call's rollback: an exception raised inside runs ctx.rollback,
    newest first, and goes on.  For the checks a caller of _deferred makes before it launches."""
    try:
        yield
    except BaseException:
        for undo in reversed(ctx.rollback):
            undo()
        raise


def _deferred(fn, kvl, dests, args=(), kwargs=None):
    """The deferred call of `fn` on the (K, V) list `kvl` with destinations `dests`: a fresh
    _DestCall installed while fn's own Python runs -- which launches nothing on K / V, see
    _defer() -- the previous context restored, then the copy-only jobs of the layers that no
    engine job delivered.  Returns (fn's result as a list, those moves, the _DestCall with the
    parked launches); an exception on the way is rolled back (_rolled_back)."""
    ctx = _DestCall(dests)
    prev = getattr(_dest_state, "ctx", None)
    with _rolled_back(ctx):
        _dest_state.ctx = ctx
        try:
            res = fn(kvl, *args, **(kwargs or {}))
        finally:
            _dest_state.ctx = prev
        if not isinstance(res, list):
            res = list(res)
        return res, _dest_moves(kvl, res, dests, ctx), ctx


def _dest_moves(kvl, res, dests, ctx):
    """Copy-only jobs for the layers of a call with `out` that came back as the input or as a
    slice of it (an "inplace" layer that is already at the front needs none); zero-length results
    are written into `res` directly."""
    moves = []
    for i, (inp, r) in enumerate(zip(kvl, res)):
        d = dests[i]
        if d is None or i in ctx.done:
            continue
        k, v = inp
        if r is inp or (r[0] is k and r[1] is v):
            if d == "inplace":
                continue  # left alone: the same objects
            start, n = 0, k.size(2)
        else:
            sl = _slice_of(inp, r)
            if sl is None:
                raise RuntimeError(f"layer {i}: the method returned tensors that are neither its "
                                   "input, a slice of it nor an engine output; `out` cannot place them")
            start, n = sl
            if d == "inplace" and start == 0:
                continue  # already the front view
        kd, vd = (k, v) if d == "inplace" else d
        if n == 0:
            res[i] = (kd.narrow(2, 0, 0), vd.narrow(2, 0, 0))
            continue
        moves.append(Segments(i, k, v, tail_start=start, tail_len=n, k_dest=kd, v_dest=vd,
                              dest_checked=True))
    return moves
