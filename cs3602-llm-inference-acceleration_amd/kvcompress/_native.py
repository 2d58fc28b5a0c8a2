"""ctypes binding of libkvc.so (include/kvc.h).

The HIP library is the only compute path of this package: if it is missing or cannot be
loaded, every compressing call raises -- there is no CPU or eager-PyTorch fallback.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libkvc.so")
# diagnostic builds (e.g. the s_memtime-stamped select kernel) may be swapped in by path
LIB_PATH = os.environ.get("KVC_LIB", LIB_PATH)

KVC_F32, KVC_BF16, KVC_F16 = 0, 1, 2
KVC_F8E4M3, KVC_F8E5M2 = 16, 17  # fp8 K/V storage (scored as bf16, copied as bytes)
KVC_ASC, KVC_DESC = 0, 1
KVC_ALGO_SORT, KVC_ALGO_TOPK, KVC_ALGO_STABLE = 0, 1, 2
KVC_SCORE_NORM, KVC_SCORE_SNAPKV = 0, 1
PHASE_SCORE, PHASE_SELECT, PHASE_GATHER, PHASE_ALL = 1, 2, 4, 7
FLAG_SPLIT_SELECT_GATHER, FLAG_SHARED_INDEX, FLAG_GATHER_FIXED, FLAG_GATHER_SELECTED = 1, 2, 4, 8
DEV_SELECT_BOUNDS, DEV_INDEX_RANGE, DEV_INTERNAL = 1, 2, 4  # enum kvc_device_status bits


ATTN_HH_STABLE = 4  # kvc_attn_params.flags: kvc_heavy_hitters with the stable tie order
ATTN_SCALAR_SUM = 8  # kvc_attn_accumulate: the reference summed last-dim-strided attention


def ATTN_OLD_DTYPE(d):
    """kvc_attn_params.flags of kvc_attn_accumulate: acc_old of dtype d (KVC_ATTN_OLD_DTYPE)."""
    return d + 1

ABI_VERSION = 4
KVC_E_TOO_LONG = -5

# struct kvc_layer (include/kvc.h) -- 136 bytes, checked against kvc_layer_struct_size()
LAYER_DTYPE = np.dtype([
    ("k", "<u8"), ("v", "<u8"), ("k_out", "<u8"), ("v_out", "<u8"),
    ("k_stride", "<i8", (3,)), ("v_stride", "<i8", (3,)),
    ("seq_len", "<i4"), ("zone_start", "<i4"), ("zone_len", "<i4"), ("n_select", "<i4"),
    ("sink_len", "<i4"), ("tail_start", "<i4"), ("tail_len", "<i4"), ("pool_kernel", "<i4"),
    ("score_mode", "<i4"), ("n_out", "<i4"), ("row0", "<i4"), ("tile0", "<i4"),
    ("unit0", "<i8"),
])
assert LAYER_DTYPE.itemsize == 136

# struct kvc_dest (include/kvc.h: caller-provided destinations) -- 56 bytes
DEST_DTYPE = np.dtype([
    ("k_stride", "<i8", (3,)), ("v_stride", "<i8", (3,)), ("in_place", "<i4"), ("reserved", "<i4"),
])
assert DEST_DTYPE.itemsize == 56

# struct kvc_pages (include/kvc.h: paged caches) -- 48 bytes
PAGES_DTYPE = np.dtype([
    ("block_table", "<u8"), ("table_stride", "<i8"), ("k_page_stride", "<i8"),
    ("v_page_stride", "<i8"), ("page_size", "<i4"), ("num_pages", "<i4"), ("in_place", "<i4"),
    ("reserved", "<i4"),
])
assert PAGES_DTYPE.itemsize == 48

# struct kvc_seq / kvc_ragged (include/kvc.h: ragged paged batches) -- 48 / 16 bytes
SEQ_DTYPE = np.dtype([
    ("seq_len", "<i4"), ("zone_start", "<i4"), ("zone_len", "<i4"), ("n_select", "<i4"),
    ("sink_len", "<i4"), ("tail_start", "<i4"), ("tail_len", "<i4"), ("score_mode", "<i4"),
    ("pool_kernel", "<i4"), ("n_out", "<i4"), ("reserved", "<i4", (2,)),
])
assert SEQ_DTYPE.itemsize == 48
RAGGED_DTYPE = np.dtype([("host", "<u8"), ("dev", "<u8")])
assert RAGGED_DTYPE.itemsize == 16

# struct kvc_scales (include/kvc.h: per-token-scaled fp8 paged caches) -- 72 bytes
SCALES_DTYPE = np.dtype([
    ("k_scale", "<u8"), ("v_scale", "<u8"), ("k_page_stride", "<i8"), ("v_page_stride", "<i8"),
    ("k_stride", "<i8", (2,)), ("v_stride", "<i8", (2,)), ("flags", "<i4"), ("reserved", "<i4"),
])
assert SCALES_DTYPE.itemsize == 72
SCALE_K_UNIFORM, SCALE_V_UNIFORM, SCALE_K_NONE, SCALE_V_NONE = 1, 2, 4, 8  # enum kvc_scale_flag

# struct kvc_page_dest (include/kvc.h: paged destinations) -- 72 bytes
PAGE_DEST_DTYPE = np.dtype([
    ("block_table", "<u8"), ("table_stride", "<i8"), ("k_page_stride", "<i8"),
    ("v_page_stride", "<i8"), ("k_stride", "<i8", (2,)), ("v_stride", "<i8", (2,)),
    ("page_size", "<i4"), ("num_pages", "<i4"),
])
assert PAGE_DEST_DTYPE.itemsize == 72

# struct kvc_attn_layer / kvc_hh_layer (include/kvc.h: h2o_attention heavy hitters)
ATTN_LAYER_DTYPE = np.dtype([
    ("attn", "<u8"), ("attn_stride", "<i8", (3,)), ("acc_old", "<u8"), ("acc_new", "<u8"),
    ("q_len", "<i4"), ("key_len", "<i4"), ("old_len", "<i4"), ("col_chunk", "<i4"),
])
assert ATTN_LAYER_DTYPE.itemsize == 64
HH_LAYER_DTYPE = np.dtype([
    ("acc", "<u8"), ("acc_len", "<i4"), ("zone_start", "<i4"), ("zone_len", "<i4"),
    ("n_select", "<i4"), ("col_chunk", "<i4"), ("reserved", "<i4"),
])
assert HH_LAYER_DTYPE.itemsize == 32


class Params(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int32), ("batch", ctypes.c_int32), ("heads", ctypes.c_int32),
                ("head_dim", ctypes.c_int32), ("order", ctypes.c_int32), ("algo", ctypes.c_int32),
                ("phases", ctypes.c_int32), ("external_index", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("device_status", ctypes.c_void_p)]


class AttnParams(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int32), ("batch", ctypes.c_int32), ("heads", ctypes.c_int32),
                ("vec_bytes", ctypes.c_int32), ("decay", ctypes.c_float),
                ("flags", ctypes.c_int32), ("device_status", ctypes.c_void_p)]


class PlanInfo(ctypes.Structure):
    _fields_ = [("norm_offset", ctypes.c_size_t),
                ("index_offset", ctypes.c_size_t), ("workspace_bytes", ctypes.c_size_t),
                ("norm_row_stride", ctypes.c_int64), ("index_row_stride", ctypes.c_int64),
                ("rows", ctypes.c_int64), ("score_tiles", ctypes.c_int64),
                ("gather_units", ctypes.c_int64)]


EXPORTS = ("kvc_version", "kvc_layer_struct_size", "kvc_max_zone_len", "kvc_status_string",
           "kvc_source_digest",
           "kvc_plan", "kvc_launch", "kvc_compress", "kvc_attn_accumulate", "kvc_hh_workspace",
           "kvc_heavy_hitters", "kvc_debug_select_capacity", "kvc_plan_dest", "kvc_launch_dest",
           "kvc_plan_paged", "kvc_launch_paged", "kvc_plan_ragged", "kvc_launch_ragged",
           "kvc_plan_scaled", "kvc_launch_scaled", "kvc_plan_repage", "kvc_launch_repage")

_lib = None


class NativeLibraryError(RuntimeError):
    pass


def lib():
    """Load libkvc.so once; raise loudly if it is absent or incompatible."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"HIP engine library not built: {LIB_PATH} is missing. "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950).")
    L = ctypes.CDLL(LIB_PATH)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    L.kvc_version.restype = i32
    L.kvc_layer_struct_size.restype = ctypes.c_size_t
    L.kvc_max_zone_len.restype = i32
    L.kvc_status_string.restype = ctypes.c_char_p
    L.kvc_status_string.argtypes = [i32]
    L.kvc_source_digest.restype = ctypes.c_char_p
    L.kvc_source_digest.argtypes = []
    L.kvc_plan.restype = i32
    L.kvc_plan.argtypes = [ctypes.POINTER(Params), vp, i32, ctypes.POINTER(PlanInfo)]
    L.kvc_launch.restype = i32
    L.kvc_launch.argtypes = [ctypes.POINTER(Params), vp, i32, vp, ctypes.c_size_t, vp]
    # additive within ABI 4: a swapped-in library (KVC_LIB) built before them lacks the two
    # destination entries; plan_dest / launch_dest then raise
    if hasattr(L, "kvc_plan_dest"):
        L.kvc_plan_dest.restype = i32
        L.kvc_plan_dest.argtypes = [ctypes.POINTER(Params), vp, vp, i32,
                                    ctypes.POINTER(PlanInfo)]
        L.kvc_launch_dest.restype = i32
        L.kvc_launch_dest.argtypes = [ctypes.POINTER(Params), vp, vp, i32, vp, ctypes.c_size_t,
                                      vp]
    if hasattr(L, "kvc_plan_paged"):  # additive within ABI 4, like the destination entries
        L.kvc_plan_paged.restype = i32
        L.kvc_plan_paged.argtypes = [ctypes.POINTER(Params), vp, vp, vp, i32,
                                     ctypes.POINTER(PlanInfo)]
        L.kvc_launch_paged.restype = i32
        L.kvc_launch_paged.argtypes = [ctypes.POINTER(Params), vp, vp, vp, i32, vp,
                                       ctypes.c_size_t, vp]
    if hasattr(L, "kvc_plan_ragged"):  # additive within ABI 4, like the paged entries
        L.kvc_plan_ragged.restype = i32
        L.kvc_plan_ragged.argtypes = [ctypes.POINTER(Params), vp, vp, vp, i32,
                                      ctypes.POINTER(PlanInfo)]
        L.kvc_launch_ragged.restype = i32
        L.kvc_launch_ragged.argtypes = [ctypes.POINTER(Params), vp, vp, vp, i32, vp,
                                        ctypes.c_size_t, vp]
    if hasattr(L, "kvc_plan_scaled"):  # additive within ABI 4, like the ragged entries
        L.kvc_plan_scaled.restype = i32
        L.kvc_plan_scaled.argtypes = [ctypes.POINTER(Params), vp, vp, vp, vp, i32,
                                      ctypes.POINTER(PlanInfo)]
        L.kvc_launch_scaled.restype = i32
        L.kvc_launch_scaled.argtypes = [ctypes.POINTER(Params), vp, vp, vp, vp, i32, vp,
                                        ctypes.c_size_t, vp]
    if hasattr(L, "kvc_plan_repage"):  # additive within ABI 4, like the scaled entries
        L.kvc_plan_repage.restype = i32
        L.kvc_plan_repage.argtypes = [ctypes.POINTER(Params), vp, vp, vp, vp, vp, vp, i32,
                                      ctypes.POINTER(PlanInfo)]
        L.kvc_launch_repage.restype = i32
        L.kvc_launch_repage.argtypes = [ctypes.POINTER(Params), vp, vp, vp, vp, vp, vp, i32, vp,
                                        ctypes.c_size_t, vp]
    L.kvc_compress.restype = i32
    L.kvc_compress.argtypes = [ctypes.POINTER(Params), vp, i32, vp, ctypes.c_size_t, vp]
    L.kvc_attn_accumulate.restype = i32
    L.kvc_attn_accumulate.argtypes = [ctypes.POINTER(AttnParams), vp, i32, vp]
    L.kvc_hh_workspace.restype = i32
    L.kvc_hh_workspace.argtypes = [ctypes.POINTER(AttnParams), vp, i32,
                                   ctypes.POINTER(ctypes.c_size_t)]
    L.kvc_heavy_hitters.restype = i32
    L.kvc_heavy_hitters.argtypes = [ctypes.POINTER(AttnParams), vp, i32, vp, ctypes.c_int64, vp,
                                    ctypes.c_size_t, vp]
    L.kvc_debug_select_capacity.restype = i32
    L.kvc_debug_select_capacity.argtypes = [ctypes.POINTER(Params), vp, i32, vp, ctypes.c_size_t,
                                            i32, vp]
    if L.kvc_version() != ABI_VERSION or L.kvc_layer_struct_size() != LAYER_DTYPE.itemsize:
        raise NativeLibraryError("libkvc.so ABI mismatch; rebuild it")
    _lib = L
    return L


def source_digest():
    """SHA-256 of the sources libkvc.so was built from ("unknown" for variant builds)."""
    return lib().kvc_source_digest().decode()


def status_string(rc):
    return lib().kvc_status_string(rc).decode()


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {status_string(rc)} (kvc status {rc})")


def plan(params, table):
    info = PlanInfo()
    rc = lib().kvc_plan(ctypes.byref(params), table.ctypes.data, len(table), ctypes.byref(info))
    return rc, info


def launch(params, table, ws_ptr, ws_bytes, stream_ptr):
    return lib().kvc_launch(ctypes.byref(params), table.ctypes.data, len(table), ws_ptr, ws_bytes,
                            stream_ptr)


def _need_dest_entries():
    if not hasattr(lib(), "kvc_plan_dest"):
        raise NativeLibraryError(f"{LIB_PATH} has no kvc_plan_dest / kvc_launch_dest (built "
                                 "before destinations); destinations need the current library")


def plan_dest(params, table, dests):
    """kvc_plan_dest: `dests` is a DEST_DTYPE array, one entry per layer, or None (= kvc_plan)."""
    info = PlanInfo()
    assert dests is None or (dests.dtype == DEST_DTYPE and len(dests) == len(table))
    _need_dest_entries()
    rc = lib().kvc_plan_dest(ctypes.byref(params), table.ctypes.data,
                             dests.ctypes.data if dests is not None else None, len(table),
                             ctypes.byref(info))
    return rc, info


def launch_dest(params, table, dests, ws_ptr, ws_bytes, stream_ptr):
    """kvc_launch_dest (dests None = kvc_launch)."""
    assert dests is None or (dests.dtype == DEST_DTYPE and len(dests) == len(table))
    _need_dest_entries()
    return lib().kvc_launch_dest(ctypes.byref(params), table.ctypes.data,
                                 dests.ctypes.data if dests is not None else None, len(table),
                                 ws_ptr, ws_bytes, stream_ptr)


def _need_paged_entries():
    if not hasattr(lib(), "kvc_plan_paged"):
        raise NativeLibraryError(f"{LIB_PATH} has no kvc_plan_paged / kvc_launch_paged (built "
                                 "before paged caches); paged caches need the current library")


def _opt(a, dtype, n):
    assert a is None or (a.dtype == dtype and len(a) == n)
    return a.ctypes.data if a is not None else None


def plan_paged(params, table, pages, dests=None):
    """kvc_plan_paged: `pages` is a PAGES_DTYPE array, one entry per layer, or None (=
    kvc_plan_dest); `dests` a DEST_DTYPE array or None."""
    info = PlanInfo()
    _need_paged_entries()
    rc = lib().kvc_plan_paged(ctypes.byref(params), table.ctypes.data,
                              _opt(pages, PAGES_DTYPE, len(table)),
                              _opt(dests, DEST_DTYPE, len(table)), len(table), ctypes.byref(info))
    return rc, info


def launch_paged(params, table, pages, dests, ws_ptr, ws_bytes, stream_ptr):
    """kvc_launch_paged (pages None = kvc_launch_dest)."""
    _need_paged_entries()
    return lib().kvc_launch_paged(ctypes.byref(params), table.ctypes.data,
                                  _opt(pages, PAGES_DTYPE, len(table)),
                                  _opt(dests, DEST_DTYPE, len(table)), len(table), ws_ptr,
                                  ws_bytes, stream_ptr)


def _need_ragged_entries():
    if not hasattr(lib(), "kvc_plan_ragged"):
        raise NativeLibraryError(f"{LIB_PATH} has no kvc_plan_ragged / kvc_launch_ragged (built "
                                 "before ragged batches); they need the current library")


def plan_ragged(params, table, pages, ragged):
    """kvc_plan_ragged: `ragged` is a RAGGED_DTYPE array, one entry per layer (host / device
    addresses of params.batch SEQ_DTYPE records each), or None (= kvc_plan_paged).  Overwrites the
    table's segment fields with the envelope of each layer's records."""
    info = PlanInfo()
    _need_ragged_entries()
    rc = lib().kvc_plan_ragged(ctypes.byref(params), table.ctypes.data,
                               _opt(pages, PAGES_DTYPE, len(table)),
                               _opt(ragged, RAGGED_DTYPE, len(table)), len(table),
                               ctypes.byref(info))
    return rc, info


def launch_ragged(params, table, pages, ragged, ws_ptr, ws_bytes, stream_ptr):
    """kvc_launch_ragged (ragged None = kvc_launch_paged without destinations)."""
    _need_ragged_entries()
    return lib().kvc_launch_ragged(ctypes.byref(params), table.ctypes.data,
                                   _opt(pages, PAGES_DTYPE, len(table)),
                                   _opt(ragged, RAGGED_DTYPE, len(table)), len(table), ws_ptr,
                                   ws_bytes, stream_ptr)


def _need_scaled_entries():
    if not hasattr(lib(), "kvc_plan_scaled"):
        raise NativeLibraryError(f"{LIB_PATH} has no kvc_plan_scaled / kvc_launch_scaled (built "
                                 "before scaled fp8 caches); they need the current library")


def plan_scaled(params, table, pages, ragged, scales):
    """kvc_plan_scaled: `scales` is a SCALES_DTYPE array, one entry per layer, or None (=
    kvc_plan_ragged); `ragged` None plans the single-length paged call."""
    info = PlanInfo()
    _need_scaled_entries()
    rc = lib().kvc_plan_scaled(ctypes.byref(params), table.ctypes.data,
                               _opt(pages, PAGES_DTYPE, len(table)),
                               _opt(ragged, RAGGED_DTYPE, len(table)),
                               _opt(scales, SCALES_DTYPE, len(table)), len(table),
                               ctypes.byref(info))
    return rc, info


def launch_scaled(params, table, pages, ragged, scales, ws_ptr, ws_bytes, stream_ptr):
    """kvc_launch_scaled (scales None = kvc_launch_ragged)."""
    _need_scaled_entries()
    return lib().kvc_launch_scaled(ctypes.byref(params), table.ctypes.data,
                                   _opt(pages, PAGES_DTYPE, len(table)),
                                   _opt(ragged, RAGGED_DTYPE, len(table)),
                                   _opt(scales, SCALES_DTYPE, len(table)), len(table), ws_ptr,
                                   ws_bytes, stream_ptr)


def _need_repage_entries():
    if not hasattr(lib(), "kvc_plan_repage"):
        raise NativeLibraryError(f"{LIB_PATH} has no kvc_plan_repage / kvc_launch_repage (built "
                                 "before paged destinations); they need the current library")


def plan_repage(params, table, pages, ragged, scales, pdests, dscales):
    """kvc_plan_repage: `pdests` is a PAGE_DEST_DTYPE array, one entry per layer, or None (=
    kvc_plan_scaled); `dscales` a SCALES_DTYPE array (the destination scale pools) or None."""
    info = PlanInfo()
    _need_repage_entries()
    n = len(table)
    rc = lib().kvc_plan_repage(ctypes.byref(params), table.ctypes.data,
                               _opt(pages, PAGES_DTYPE, n), _opt(ragged, RAGGED_DTYPE, n),
                               _opt(scales, SCALES_DTYPE, n), _opt(pdests, PAGE_DEST_DTYPE, n),
                               _opt(dscales, SCALES_DTYPE, n), n, ctypes.byref(info))
    return rc, info


def launch_repage(params, table, pages, ragged, scales, pdests, dscales, ws_ptr, ws_bytes,
                  stream_ptr):
    """kvc_launch_repage (pdests None = kvc_launch_scaled)."""
    _need_repage_entries()
    n = len(table)
    return lib().kvc_launch_repage(ctypes.byref(params), table.ctypes.data,
                                   _opt(pages, PAGES_DTYPE, n), _opt(ragged, RAGGED_DTYPE, n),
                                   _opt(scales, SCALES_DTYPE, n),
                                   _opt(pdests, PAGE_DEST_DTYPE, n),
                                   _opt(dscales, SCALES_DTYPE, n), n, ws_ptr, ws_bytes, stream_ptr)


class Tables:
    """The optional tables of one call (csrc/kvc.hip, struct Tables): per field an array of one
    record per layer, or None for a call without that table.  The one place that knows which
    plan / launch pair serves which combination, and under what name its errors are reported
    (`plan_name` / `launch_name`, for check())."""
    __slots__ = ("dests", "pages", "ragged", "scales", "pdests", "dscales", "_entry", "_args")

    def __init__(self, dests=None, pages=None, ragged=None, scales=None, pdests=None,
                 dscales=None):
        self.dests, self.pages, self.ragged = dests, pages, ragged
        self.scales, self.pdests, self.dscales = scales, pdests, dscales
        if pdests is not None:  # paged layers delivered through a second block table
            self._entry, self._args = "_repage", (pages, ragged, scales, pdests, dscales)
        elif scales is not None:  # scaled fp8 paged layers, compacted in place (ragged or not)
            self._entry, self._args = "_scaled", (pages, ragged, scales)
        elif ragged is not None:
            self._entry, self._args = "_ragged", (pages, ragged)
        elif pages is not None:
            self._entry, self._args = "_paged", (pages, dests)
        elif dests is not None:
            self._entry, self._args = "_dest", (dests,)
        else:
            self._entry, self._args = "", ()

    @property
    def plan_name(self):
        return "kvc_plan" + self._entry

    @property
    def launch_name(self):
        return "kvc_launch" + self._entry

    def plan(self, params, table):
        """(rc, PlanInfo) of the combination's kvc_plan* entry (this module's plan* function)."""
        return globals()["plan" + self._entry](params, table, *self._args)

    def launch(self, params, table, ws_ptr, ws_bytes, stream_ptr):
        """rc of the combination's kvc_launch* entry (this module's launch* function)."""
        return globals()["launch" + self._entry](params, table, *self._args, ws_ptr, ws_bytes,
                                                 stream_ptr)


def attn_accumulate(params, table, stream_ptr):
    return lib().kvc_attn_accumulate(ctypes.byref(params), table.ctypes.data, len(table),
                                     stream_ptr)


def hh_workspace(params, table):
    n = ctypes.c_size_t()
    rc = lib().kvc_hh_workspace(ctypes.byref(params), table.ctypes.data, len(table),
                                ctypes.byref(n))
    return rc, n.value


def heavy_hitters(params, table, out_ptr, out_stride, ws_ptr, ws_bytes, stream_ptr):
    return lib().kvc_heavy_hitters(ctypes.byref(params), table.ctypes.data, len(table), out_ptr,
                                   out_stride, ws_ptr, ws_bytes, stream_ptr)


def debug_select_capacity(params, table, ws_ptr, ws_bytes, zone_cap, stream_ptr):
    """kvc_debug_select_capacity: the test hook of the device-side selection bounds check."""
    return lib().kvc_debug_select_capacity(ctypes.byref(params), table.ctypes.data, len(table),
                                           ws_ptr, ws_bytes, zone_cap, stream_ptr)
