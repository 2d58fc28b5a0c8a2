// kvc.hip -- MI355X (gfx950) kernels and C ABI of the KV-cache compression engine.
// ABI documentation: include/kvc.h.  Design and rooflines: DESIGN.md.
//
// Kernels (one launch each, all layers of a compress_fn call batched into every launch):
//   score_kernel  : HBM-streaming key L2 norms.  One wave = one 64-token tile of one (b,h) row;
//                   tiles are read with coalesced 16-B loads, transposed through a padded LDS
//                   slab so each lane owns one token row, and reduced with torch.norm's exact
//                   8-accumulator FMA order (reference: torch.norm at fix_size_l2.py:106 etc.).
//   select_kernel : one 1024-thread workgroup per (layer, b, h) row, the row's keys resident in
//                   LDS.  Reproduces the first-k SET of libstdc++ std::sort (argsort, stable=False)
//                   or std::nth_element / std::partial_sort (torch.topk) by following only the
//                   chain of Hoare partitions that straddle position k; each partition is computed
//                   in parallel from ballot prefix ranks ("Selection").  Emits the
//                   kept zone-local indices in ascending order (= torch.sort(indices) of the
//                   reference, e.g. fix_size_l2.py:129).
//   gather_kernel : segment copy sink ++ zone[selected] ++ tail for K and V (torch.gather +
//                   torch.cat of the reference, e.g. fix_size_l2.py:137-147).
//
// This file is the one translation unit: the device code lives in the headers below, one per
// phase, each needing only the ones before it; here are the host side (kvc_plan's layout, the
// launchers) and the extern "C" entry points.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <tuple>
#include <type_traits>
#include <utility>

#include "kvc.h"
#include "kvc_common.h"
#include "kvc_serial.h"

#include "kvc_device_util.h"    // constants, dtype traits, wave helpers, the selection's layout
#include "kvc_score.h"          // score_kernel
#include "kvc_snapkv_keys.h"    // snapkv_lite scores -> sort keys
#include "kvc_select_chain.h"   // sort / heap helpers, partition_level, run_chain
#include "kvc_select.h"         // select_body, select_kernel, select_global / select_long
#include "kvc_gather.h"         // gather_kernel, select_gather_kernel
#include "kvc_attn.h"           // attn_accumulate / head-sum kernels
#include "kvc_gather_dest.h"    // gather_dest_kernel (kvc_launch_dest)
#include "kvc_paged.h"          // score_paged_kernel, gather_paged_kernel (kvc_launch_paged)
#include "kvc_ragged.h"         // the per-sequence-record kernels (kvc_launch_ragged)
#include "kvc_repage.h"         // GATHER through a destination block table (kvc_launch_repage)

namespace kvc {

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// STORAGE element size: addressing, alignment, span checks, GATHER units
static inline int esize(int dtype) { return dtype == KVC_F32 ? 4 : is_fp8(dtype) ? 1 : 2; }
// SCORE element size: the norm region, the tile maxima and the selection's key class (fp8 keys
// are scored as their exact bf16 upcast)
static inline int score_esize(int dtype) { return esize(score_dt(dtype)); }
// Calls f(std::integral_constant<int, DT>) for the call's storage dtype (validated by plan_impl).
template <typename F>
static int with_dtype(int dtype, F&& f) {
#ifdef KVC_ISA_PROBE  // diagnostic compile for ISA inspection: bf16 instantiations only
  return dtype == KVC_BF16 ? f(std::integral_constant<int, KVC_BF16>()) : KVC_E_DTYPE;
#else
  if (dtype == KVC_BF16) return f(std::integral_constant<int, KVC_BF16>());
  if (dtype == KVC_F16) return f(std::integral_constant<int, KVC_F16>());
  return f(std::integral_constant<int, KVC_F32>());
#endif
}
// with_dtype over the K/V storage dtypes: the fp8 formats as well (the attention entries, whose
// tensors are never fp8, keep with_dtype)
template <typename F>
static int with_kv_dtype(int dtype, F&& f) {
#ifdef KVC_ISA_PROBE  // (bf16 instantiations only: no fp8 kernel to run)
  if (is_fp8(dtype)) return KVC_E_DTYPE;
#else
  if (dtype == KVC_F8E4M3) return f(std::integral_constant<int, KVC_F8E4M3>());
  if (dtype == KVC_F8E5M2) return f(std::integral_constant<int, KVC_F8E5M2>());
#endif
  return with_dtype(dtype, f);
}
static inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
// one row of the global selection scratch (SelArrays for n_cap positions), 256-B aligned rows
static inline size_t sel_scratch_row_bytes(int n_cap, int dtype) {
  if (n_cap > kZoneMaxGlobal) return round_up(sel_long_bytes(n_cap, score_esize(dtype)), 256);
  return round_up(sel_bytes(n_cap, score_esize(dtype), n_cap / 2 + 1), 256);
}

static int plan_impl(const kvc_params_t* p, kvc_layer_t* layers, int nl, kvc_plan_info_t* info,
                     bool fill) {
  if (!p || nl < 0 || (nl > 0 && !layers)) return KVC_E_ARG;
  if (p->dtype != KVC_BF16 && p->dtype != KVC_F16 && p->dtype != KVC_F32 && !is_fp8(p->dtype))
    return KVC_E_DTYPE;
  if (p->batch < 1 || p->heads < 1 || p->head_dim < 1) return KVC_E_ARG;
  if (p->order != KVC_ASC && p->order != KVC_DESC) return KVC_E_ARG;
  if (p->algo != KVC_ALGO_SORT && p->algo != KVC_ALGO_TOPK && p->algo != KVC_ALGO_STABLE)
    return KVC_E_ARG;
  if ((p->flags & ~(KVC_FLAG_SPLIT_SELECT_GATHER | KVC_FLAG_SHARED_INDEX | KVC_FLAG_GATHER_FIXED |
                    KVC_FLAG_GATHER_SELECTED)) || p->reserved != 0)
    return KVC_E_ARG;  // unknown flag bits / reserved field: refuse rather than ignore
  if ((p->flags & KVC_FLAG_GATHER_FIXED) && (p->flags & KVC_FLAG_GATHER_SELECTED))
    return KVC_E_ARG;
  if ((p->flags & KVC_FLAG_SHARED_INDEX) && !p->external_index) return KVC_E_ARG;
  // the two gather parts of one call share its index region: with the engine's own selection
  // each launch would also SCORE and SELECT into the same workspace (a race when the two run
  // concurrently, as the flags intend) -- so only external indices may be split
  if ((p->flags & (KVC_FLAG_GATHER_FIXED | KVC_FLAG_GATHER_SELECTED)) && !p->external_index)
    return KVC_E_ARG;
  const int es = esize(p->dtype);
  const int rowb = p->head_dim * es;
  if (rowb % 16) return KVC_E_HEADDIM;
  const int nc = rowb / 16;
  // 64..1024-byte rows: every pythia geometry (D 32/64/80/128/256) in bf16, fp16 and fp32
  if (nc != 4 && nc != 8 && nc != 10 && nc != 16 && nc != 20 && nc != 32 && nc != 64)
    return KVC_E_HEADDIM;
  // fp8 rows: D = 64 / 128 / 256 only (the widths the fp8 kernels are built and tested for)
  if (is_fp8(p->dtype) && nc != 4 && nc != 8 && nc != 16) return KVC_E_HEADDIM;
  const int64_t BH = (int64_t)p->batch * p->heads;
  if (BH * nl > 0x7FFFFFFF) return KVC_E_ARG;
  int64_t tiles = 0, units = 0, max_zone = 0, max_sel = 0;
  bool snap = false;  // a snapkv row is scored: the per-tile maxima region
  for (int l = 0; l < nl; ++l) {
    kvc_layer_t& y = layers[l];
    const int S = y.seq_len;
    if (S < 0 || y.zone_start < 0 || y.zone_len < 0 || (int64_t)y.zone_start + y.zone_len > S ||
        y.n_select < 0 || y.n_select > y.zone_len || y.sink_len < 0 || y.sink_len > S ||
        y.tail_start < 0 || y.tail_len < 0 || (int64_t)y.tail_start + y.tail_len > S ||
        (y.score_mode != KVC_SCORE_NORM && y.score_mode != KVC_SCORE_SNAPKV))
      return KVC_E_ARG;
    const int64_t n_out = (int64_t)y.sink_len + y.n_select + y.tail_len;
    if (n_out > 0x7FFFFFFF || 2 * BH * n_out * nc > 0x7FFFFFFF) return KVC_E_ARG;
    const bool needs_select = y.n_select > 0 && y.n_select < y.zone_len;
    if (needs_select && y.zone_len > kZoneMaxLong) return KVC_E_TOO_LONG;
    // stable selections: LDS, or the u16-position global scratch (not the u32 long variant)
    if (needs_select && p->algo == KVC_ALGO_STABLE && !p->external_index &&
        y.zone_len > kZoneMaxGlobal)
      return KVC_E_TOO_LONG;
    if (n_out > 0) {
      if (!y.k || !y.v || !y.k_out || !y.v_out) return KVC_E_ARG;
      if (!aligned16(y.k) || !aligned16(y.v) || !aligned16(y.k_out) || !aligned16(y.v_out))
        return KVC_E_ALIGN;
      const int64_t* ks = y.k_stride;
      const int64_t* vs = y.v_stride;
      if ((p->batch > 1 && ((ks[0] * es) % 16 || (vs[0] * es) % 16)) ||
          (p->heads > 1 && ((ks[1] * es) % 16 || (vs[1] * es) % 16)) ||
          (S > 1 && ((ks[2] * es) % 16 || (vs[2] * es) % 16)))
        return KVC_E_ALIGN;
    }
    const int64_t tl = needs_select ? BH * ((y.zone_len + kTile - 1) / kTile) : 0;
    const int64_t ul = 2 * BH * n_out * nc;
    if (fill) {
      y.n_out = (int32_t)n_out;
      y.row0 = (int32_t)(l * BH);
      y.tile0 = (int32_t)tiles;
      y.unit0 = units;
    } else if (y.n_out != n_out || y.row0 != l * BH || y.tile0 != tiles || y.unit0 != units) {
      return KVC_E_ARG;
    }
    if (needs_select && y.zone_len > max_zone) max_zone = y.zone_len;
    snap |= needs_select && y.score_mode == KVC_SCORE_SNAPKV;
    if (y.n_select > max_sel) max_sel = y.n_select;
    tiles += tl;
    units += ul;
    if (tiles > 0x7FFFFFFF) return KVC_E_ARG;
  }
  if (info) {
    const int64_t rows = BH * nl;
    info->rows = rows;
    info->score_tiles = tiles;
    info->gather_units = units;
    info->norm_row_stride = (int64_t)round_up((size_t)max_zone, kTile);
    info->index_row_stride = (int64_t)round_up((size_t)(max_sel > 0 ? max_sel : 1), 16);
    size_t off = 0;
    info->norm_offset = off;
    off = round_up(off + (size_t)rows * info->norm_row_stride * score_esize(p->dtype), 256);
    info->index_offset = off;
    off = round_up(off + (size_t)rows * info->index_row_stride * 4, 256);
    if (max_zone > kZoneMax)  // selection scratch rows for zones longer than the LDS limit
      off += (size_t)rows * sel_scratch_row_bytes((int)info->norm_row_stride, p->dtype);
    // SCORE's per-64-token-tile region (u32 each; tmax_offset()): the norm maximum of a snapkv
    // row's tile.  Reserved for every scored call (the layout does not depend on the score
    // mode); plain-norm rows leave theirs unused
    if (snap || max_zone > 0)
      off += (size_t)rows * (size_t)(info->norm_row_stride / kTile) * 4;
#ifdef KVC_STAMPS
    off += (size_t)rows * 256;  // diagnostic stamp slots (32 x u64 per select row)
#endif
    info->workspace_bytes = off;
  }
  return KVC_OK;
}

// Offset of the snapkv per-tile maxima region (rows x norm_row_stride / 64 u32): after the index
// region and the long-zone selection scratch (plan_impl's layout).
static inline size_t tmax_offset(const kvc_plan_info_t& info, int dtype) {
  size_t off = round_up(info.index_offset + (size_t)info.rows * info.index_row_stride * 4, 256);
  if (info.norm_row_stride > kZoneMax)
    off += (size_t)info.rows * sel_scratch_row_bytes((int)info.norm_row_stride, dtype);
  return off;
}

// ---- checks shared by the dest and paged plans ----
// byte span [lo, hi) of a view with three stepped dims (sizes, element strides) of rows of rowb
// bytes
struct Span {
  uintptr_t lo, hi;
};
static Span span(const void* base, const int64_t (&size)[3], const int64_t (&st)[3], int es,
                 int64_t rowb) {
  int64_t neg = 0, pos = 0;
  for (int d = 0; d < 3; ++d) {
    const int64_t ext = (size[d] - 1) * st[d] * es;
    (ext < 0 ? neg : pos) += ext;
  }
  return {(uintptr_t)base + neg, (uintptr_t)base + pos + rowb};
}
// some destination range meets some source range (K and V of each)
static bool ranges_meet(const Span (&dst)[2], const Span (&src)[2]) {
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b)
      if (dst[a].lo < src[b].hi && src[b].lo < dst[a].hi) return true;
  return false;
}
// every stepped stride of a [B, H, n_out, D] destination is a multiple of 16 bytes
static bool dest_strides_aligned(const kvc_dest_t& d, int64_t B, int64_t H, int64_t n_out, int es) {
  const int64_t n[3] = {B, H, n_out};
  for (int i = 0; i < 3; ++i)
    if (n[i] > 1 && ((d.k_stride[i] * es) % 16 || (d.v_stride[i] * es) % 16)) return false;
  return true;
}
// An in-place copy needs a row map that is strictly increasing with src(t) >= t (gather_passes'
// ordering proof, kvc_gather_dest.h): sink, zone and tail in that order, none overlapping.
static bool in_place_row_map_ok(const kvc_layer_t& y) {
  return !((y.n_select > 0 && y.sink_len > y.zone_start) ||
           (y.tail_len > 0 && ((int64_t)y.zone_start + y.zone_len > y.tail_start ||
                               y.sink_len > y.tail_start)));
}

// The optional tables of one call, as its entry point received them (include/kvc.h): a null
// member means the call has no such table.  pdests != nullptr is "GATHER writes through
// destination block tables" (kvc_plan_repage / kvc_launch_repage): such a call is out of place.
struct Tables {
  const kvc_dest_t* dests;
  const kvc_pages_t* pages;
  const kvc_ragged_t* ragged;
  const kvc_scales_t* scales;
  const kvc_page_dest_t* pdests;
  const kvc_scales_t* dscales;  // with scales and pdests only
};

// A block table over a pool of num_pages pages of page_size slots that holds `rows` logical rows:
// the geometry of a source (kvc_pages_t) or a destination (kvc_page_dest_t) description.
static bool page_geometry_ok(const int32_t* table, int64_t table_stride, int num_pages,
                             int page_size, int64_t rows) {
  if (!table || ((uintptr_t)table & 3u) || num_pages < 1 || page_size < 1 || page_size > 65536 ||
      (page_size & (page_size - 1)))
    return false;
  return table_stride >= (rows + page_size - 1) / page_size;
}

// The page description of one layer with output, and what compaction in place asks of it
// (include/kvc.h, "Paged caches").  row_map: apply the in-place row-map rule to y's segments (a
// ragged layer's rule is checked per record, and y holds their envelope).
static int paged_layer_check(const kvc_params_t* p, const kvc_layer_t& y, const kvc_pages_t& g,
                             bool row_map) {
  const int es = esize(p->dtype);
  const int64_t H = p->heads, P = g.page_size;
  if (g.reserved != 0 || (g.in_place != 0 && g.in_place != 1) ||
      !page_geometry_ok(g.block_table, g.table_stride, g.num_pages, g.page_size, y.seq_len))
    return KVC_E_ARG;
  if (y.k_stride[0] != 0 || y.v_stride[0] != 0) return KVC_E_ARG;  // the table is the batch dim
  // (plan_impl has checked the head and slot strides against heads > 1 / seq_len > 1)
  if (g.num_pages > 1 && ((g.k_page_stride * es) % 16 || (g.v_page_stride * es) % 16))
    return KVC_E_ALIGN;
  if (g.in_place) {
    if (y.k_out != y.k || y.v_out != y.v) return KVC_E_ARG;
    if (row_map && !in_place_row_map_ok(y)) return KVC_E_ARG;
    // a zero stride would make different logical rows one address
    if ((H > 1 && (y.k_stride[1] == 0 || y.v_stride[1] == 0)) ||
        (P > 1 && y.seq_len > 1 && (y.k_stride[2] == 0 || y.v_stride[2] == 0)) ||
        (g.num_pages > 1 && (g.k_page_stride == 0 || g.v_page_stride == 0)))
      return KVC_E_ARG;
  }
  return KVC_OK;
}

// The dense destination of one layer with output (include/kvc.h, "Caller-provided
// destinations"): of a [B, H, S, D] source view or -- g != nullptr -- of the layer's page pools,
// which a dense destination never compacts in place (that is kvc_pages_t.in_place).
static int dest_layer_check(const kvc_params_t* p, const kvc_layer_t& y, const kvc_dest_t& d,
                            const kvc_pages_t* g) {
  const int es = esize(p->dtype);
  const int64_t rowb = (int64_t)p->head_dim * es;
  const int64_t B = p->batch, H = p->heads, n_out = y.n_out;
  if (d.reserved != 0 || (d.in_place != 0 && (g || d.in_place != 1))) return KVC_E_ARG;
  if (!dest_strides_aligned(d, B, H, n_out, es)) return KVC_E_ALIGN;
  const int64_t* ks = d.k_stride;
  const int64_t* vs = d.v_stride;
  if (d.in_place) {
    if (y.k_out != y.k || y.v_out != y.v || memcmp(ks, y.k_stride, sizeof(y.k_stride)) ||
        memcmp(vs, y.v_stride, sizeof(y.v_stride)))
      return KVC_E_ARG;
    if (!in_place_row_map_ok(y)) return KVC_E_ARG;
    // a zero stride (an expanded batch) would be written twice
    if ((B > 1 && (ks[0] == 0 || vs[0] == 0)) || (H > 1 && (ks[1] == 0 || vs[1] == 0)) ||
        (y.seq_len > 1 && (ks[2] == 0 || vs[2] == 0)))
      return KVC_E_ARG;
    return KVC_OK;
  }
  // the source's byte range: the view's, or the whole pools' (pages x heads x slots)
  int64_t ssize[3] = {B, H, y.seq_len};
  int64_t kst[3] = {y.k_stride[0], y.k_stride[1], y.k_stride[2]};
  int64_t vst[3] = {y.v_stride[0], y.v_stride[1], y.v_stride[2]};
  if (g) {
    ssize[0] = g->num_pages, ssize[2] = g->page_size;
    kst[0] = g->k_page_stride, vst[0] = g->v_page_stride;
  }
  const int64_t dsize[3] = {B, H, n_out};
  const Span src[2] = {span(y.k, ssize, kst, es, rowb), span(y.v, ssize, vst, es, rowb)};
  const Span dst[2] = {span(y.k_out, dsize, d.k_stride, es, rowb),
                       span(y.v_out, dsize, d.v_stride, es, rowb)};
  return ranges_meet(dst, src) ? KVC_E_ARG : KVC_OK;
}

// The ragged step of plan_tables (include/kvc.h, "Ragged paged batches"): every host record under
// a layer's rules, the layers' segment fields set to (fill) or compared with (launch) the envelope
// of their records.  The records compact in place -- in_place must be 1, each record under the
// in-place row-map rule -- unless the call writes through destination tables: then in_place must
// be 0 and the records are free of that rule.
static int ragged_envelopes(const kvc_params_t* p, kvc_layer_t* layers, const Tables& t, int nl,
                            bool fill) {
  const bool in_place = !t.pdests;
  if (!p || nl < 0 || (nl > 0 && (!layers || !t.pages)) || p->batch < 1) return KVC_E_ARG;
  if (p->external_index || (p->flags & (KVC_FLAG_SHARED_INDEX | KVC_FLAG_GATHER_FIXED |
                                        KVC_FLAG_GATHER_SELECTED)))
    return KVC_E_ARG;
  for (int l = 0; l < nl; ++l) {
    const kvc_ragged_t& r = t.ragged[l];
    if (!r.host || !r.dev || ((uintptr_t)r.host & 3u) || ((uintptr_t)r.dev & 15u))
      return KVC_E_ARG;
    if (t.pages[l].in_place != (in_place ? 1 : 0)) return KVC_E_ARG;
    kvc_layer_t e = layers[l];  // the envelope
    e.seq_len = e.zone_start = e.zone_len = e.n_select = e.sink_len = e.tail_start = 0;
    e.tail_len = e.pool_kernel = 0;
    e.score_mode = KVC_SCORE_NORM;
    int64_t max_out = 0;
    bool selects = false;
    for (int b = 0; b < p->batch; ++b) {
      const kvc_seq_t& q = r.host[b];
      const int S = q.seq_len;
      if (S < 0 || q.zone_start < 0 || q.zone_len < 0 || (int64_t)q.zone_start + q.zone_len > S ||
          q.n_select < 0 || q.n_select > q.zone_len || q.sink_len < 0 || q.sink_len > S ||
          q.tail_start < 0 || q.tail_len < 0 || (int64_t)q.tail_start + q.tail_len > S ||
          (q.score_mode != KVC_SCORE_NORM && q.score_mode != KVC_SCORE_SNAPKV) ||
          q.reserved[0] != 0 || q.reserved[1] != 0 ||
          (int64_t)q.sink_len + q.n_select + q.tail_len != q.n_out)
        return KVC_E_ARG;
      kvc_layer_t y = e;  // the record as a layer: the row-map rule's argument
      y.zone_start = q.zone_start, y.zone_len = q.zone_len, y.n_select = q.n_select;
      y.sink_len = q.sink_len, y.tail_start = q.tail_start, y.tail_len = q.tail_len;
      if (in_place && !in_place_row_map_ok(y)) return KVC_E_ARG;
      const bool sel = layer_selects(y);
      selects |= sel;
      e.seq_len = S > e.seq_len ? S : e.seq_len;
      e.zone_len = q.zone_len > e.zone_len ? q.zone_len : e.zone_len;
      e.n_select = q.n_select > e.n_select ? q.n_select : e.n_select;
      e.pool_kernel = q.pool_kernel > e.pool_kernel ? q.pool_kernel : e.pool_kernel;
      if (sel && q.score_mode == KVC_SCORE_SNAPKV) e.score_mode = KVC_SCORE_SNAPKV;
      max_out = q.n_out > max_out ? q.n_out : max_out;
    }
    if (selects && e.n_select >= e.zone_len) {  // the envelope of a selecting record selects
      e.zone_len = e.n_select + 1;
      e.seq_len = e.zone_len > e.seq_len ? e.zone_len : e.seq_len;
    }
    e.tail_len = (int32_t)(max_out - e.n_select);
    kvc_layer_t& y = layers[l];
    if (fill) {
      y.seq_len = e.seq_len, y.zone_start = 0, y.zone_len = e.zone_len, y.n_select = e.n_select;
      y.sink_len = 0, y.tail_start = 0, y.tail_len = e.tail_len;
      y.pool_kernel = e.pool_kernel, y.score_mode = e.score_mode;
    } else if (y.seq_len != e.seq_len || y.zone_start != 0 || y.zone_len != e.zone_len ||
               y.n_select != e.n_select || y.sink_len != 0 || y.tail_start != 0 ||
               y.tail_len != e.tail_len || y.pool_kernel != e.pool_kernel ||
               y.score_mode != e.score_mode) {
      return KVC_E_ARG;
    }
  }
  return KVC_OK;
}

// One kvc_scales_t (include/kvc.h, "Per-token-scaled fp8 paged caches") over pools of num_pages
// pages of page_size slots: each side that is read has a pointer, 4-byte aligned, and -- where it
// is a pool -- no zero stride over a dimension longer than one.  A uniform K scale is one word
// that SCORE reads (k_uniform_read; GATHER moves no uniform word, so a destination's is not
// read); a uniform V scale is never read: its pointer may be anything.
static int scale_sides_check(const kvc_scales_t& z, bool k_uniform_read, int64_t num_pages,
                             int64_t heads, int64_t page_size) {
  const struct {
    const float* ptr;
    int64_t page, head, slot;
    bool read, pool;
  } side[2] = {
      {z.k_scale, z.k_page_stride, z.k_stride[0], z.k_stride[1],
       !(z.flags & (KVC_SCALE_K_NONE | (k_uniform_read ? 0 : KVC_SCALE_K_UNIFORM))),
       !(z.flags & (KVC_SCALE_K_NONE | KVC_SCALE_K_UNIFORM))},
      {z.v_scale, z.v_page_stride, z.v_stride[0], z.v_stride[1],
       !(z.flags & (KVC_SCALE_V_NONE | KVC_SCALE_V_UNIFORM)),
       !(z.flags & (KVC_SCALE_V_NONE | KVC_SCALE_V_UNIFORM))}};
  for (const auto& s : side) {
    if (!s.read) continue;
    if (!s.ptr) return KVC_E_ARG;
    if ((uintptr_t)s.ptr & 3u) return KVC_E_ALIGN;
    // a zero stride would make the scales of different rows -- of different heads, each
    // compacted by its own workgroup -- one word
    if (s.pool && ((num_pages > 1 && s.page == 0) || (heads > 1 && s.head == 0) ||
                   (page_size > 1 && s.slot == 0)))
      return KVC_E_ARG;
  }
  return KVC_OK;
}
constexpr int kScaleFlags =
    KVC_SCALE_K_UNIFORM | KVC_SCALE_V_UNIFORM | KVC_SCALE_K_NONE | KVC_SCALE_V_NONE;

// The destination description of one layer with output (include/kvc.h, "Paged destinations");
// y.n_out is a ragged layer's largest record's.
static int page_dest_layer_check(const kvc_params_t* p, const kvc_layer_t& y,
                                 const kvc_page_dest_t& d) {
  const int es = esize(p->dtype);
  if (!page_geometry_ok(d.block_table, d.table_stride, d.num_pages, d.page_size, y.n_out))
    return KVC_E_ARG;
  const bool heads = p->heads > 1, slots = d.page_size > 1 && y.n_out > 1, pgs = d.num_pages > 1;
  // a zero stride would make different output rows one address
  if ((heads && (d.k_stride[0] == 0 || d.v_stride[0] == 0)) ||
      (slots && (d.k_stride[1] == 0 || d.v_stride[1] == 0)) ||
      (pgs && (d.k_page_stride == 0 || d.v_page_stride == 0)))
    return KVC_E_ARG;
  // (plan_impl has checked k_out / v_out themselves)
  if ((heads && ((d.k_stride[0] * es) % 16 || (d.v_stride[0] * es) % 16)) ||
      (slots && ((d.k_stride[1] * es) % 16 || (d.v_stride[1] * es) % 16)) ||
      (pgs && ((d.k_page_stride * es) % 16 || (d.v_page_stride * es) % 16)))
    return KVC_E_ALIGN;
  return KVC_OK;
}

// The plan of every entry point: plan_impl, and around it one step per table the call has, in
// this order (the first fault found is the one reported).  fill: write the layers' planned
// fields (kvc_plan*); otherwise compare them (kvc_launch*).
static int plan_tables(const kvc_params_t* p, kvc_layer_t* layers, const Tables& t, int nl,
                       kvc_plan_info_t* info, bool fill) {
  if (t.pdests && nl > 0 && !t.pages) return KVC_E_ARG;  // a paged destination: a paged layer
  int rc = t.ragged ? ragged_envelopes(p, layers, t, nl, fill) : KVC_OK;
  if (rc != KVC_OK) return rc;
  rc = plan_impl(p, layers, nl, info, fill);  // (ragged: on the envelopes)
  if (rc != KVC_OK) return rc;
  // pages, and dense destinations (never with pdests): layer by layer
  if (t.pages || t.dests) {
    if (p->flags & (KVC_FLAG_GATHER_FIXED | KVC_FLAG_GATHER_SELECTED)) return KVC_E_ARG;
    for (int l = 0; l < nl; ++l) {
      const kvc_layer_t& y = layers[l];
      if (y.n_out == 0) continue;
      const kvc_pages_t* g = t.pages ? &t.pages[l] : nullptr;
      if (g && (rc = paged_layer_check(p, y, *g, !t.ragged)) != KVC_OK) return rc;
      // (without dests, a layer that is not in place has a contiguous k_out / v_out)
      if (t.dests && !(g && g->in_place) &&
          (rc = dest_layer_check(p, y, t.dests[l], g)) != KVC_OK)
        return rc;
    }
  }
  if (t.scales) {
    if (nl > 0 && !t.pages) return KVC_E_ARG;  // every scaled layer is paged
    if (!is_fp8(p->dtype)) return KVC_E_DTYPE;
    for (int l = 0; l < nl; ++l) {
      const kvc_layer_t& y = layers[l];
      const kvc_scales_t& z = t.scales[l];
      const kvc_pages_t& g = t.pages[l];
      // a dense output has no channel for the moved scales (a paged destination has: dscales)
      if (!t.pdests && (g.in_place != 1 || y.k_out != y.k || y.v_out != y.v)) return KVC_E_ARG;
      if ((z.flags & ~kScaleFlags) || z.reserved != 0 ||
          ((z.flags & KVC_SCALE_K_UNIFORM) && (z.flags & KVC_SCALE_K_NONE)) ||
          ((z.flags & KVC_SCALE_V_UNIFORM) && (z.flags & KVC_SCALE_V_NONE)))
        return KVC_E_ARG;
      rc = scale_sides_check(z, true, g.num_pages, p->heads, g.page_size);
      if (rc != KVC_OK) return rc;
    }
  }
  if (t.pdests) {
    if (t.scales && !t.dscales) return KVC_E_ARG;
    for (int l = 0; l < nl; ++l) {
      const kvc_layer_t& y = layers[l];
      if (y.n_out == 0) continue;
      if (t.pages[l].in_place != 0) return KVC_E_ARG;
      const kvc_page_dest_t& d = t.pdests[l];
      rc = page_dest_layer_check(p, y, d);
      if (rc != KVC_OK) return rc;
      if (!t.scales) continue;
      const kvc_scales_t& dz = t.dscales[l];
      if ((dz.flags & ~kScaleFlags) || dz.reserved != 0 || dz.flags != t.scales[l].flags)
        return KVC_E_ARG;
      rc = scale_sides_check(dz, false, d.num_pages, p->heads, d.page_size);
      if (rc != KVC_OK) return rc;
    }
  }
  return KVC_OK;
}

// Every launch goes through hipLaunchKernel, whose return value is this launch's own status (a
// caller's pending HIP error is neither consumed nor reported as ours).
template <typename... P, typename... A>
static int launch_k(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s,
                    A&&... a) {
  std::tuple<P...> args(std::forward<A>(a)...);
  void* ptrs[sizeof...(P)];
  std::apply([&](auto&... x) {
    int i = 0;
    ((ptrs[i++] = static_cast<void*>(&x)), ...);
  }, args);
  return hipLaunchKernel(reinterpret_cast<const void*>(kern), grid, block, ptrs, lds, s) ==
                 hipSuccess
             ? KVC_OK
             : KVC_E_HIP;
}

// Calls f(std::integral_constant<int, NC>()) for a row width in 16-B chunks (validated by
// plan_impl: 64..1024-byte rows).
template <typename F>
static int with_nc(int nc, F&& f) {
#ifdef KVC_ISA_PROBE  // D = 128 bf16 rows only
  return nc == 16 ? f(std::integral_constant<int, 16>()) : KVC_E_HEADDIM;
#else
  switch (nc) {
    case 4: return f(std::integral_constant<int, 4>());
    case 8: return f(std::integral_constant<int, 8>());
    case 10: return f(std::integral_constant<int, 10>());
    case 16: return f(std::integral_constant<int, 16>());
    case 20: return f(std::integral_constant<int, 20>());
    case 32: return f(std::integral_constant<int, 32>());
    case 64: return f(std::integral_constant<int, 64>());
    default: return KVC_E_HEADDIM;
  }
#endif
}

// with_nc for the call's storage dtype: fp8 rows exist in the 64 / 128 / 256-byte widths only
template <int DT, typename F>
static int with_nc_dt(int nc, F&& f) {
  if constexpr (is_fp8(DT)) {
    switch (nc) {
      case 4: return f(std::integral_constant<int, 4>());
      case 8: return f(std::integral_constant<int, 8>());
      case 16: return f(std::integral_constant<int, 16>());
      default: return KVC_E_HEADDIM;
    }
  } else {
    return with_nc(nc, f);
  }
}

// Keys are read once (non-temporal loads) and outputs written once (non-temporal stores): they
// would otherwise evict useful lines from the Infinity Cache.
// (grid: one tile per wave, score_waves(NC) tiles per workgroup)
template <int DT, int NC>
static int launch_score(const LayerChunk& T, int nl, int H, int64_t tile_base,
                        int64_t chunk_tiles, char* norms, int64_t nstride, uint32_t* tmax,
                        hipStream_t s) {
  constexpr int per_wg = score_waves(NC);
  return launch_k(score_kernel<DT, NC>, dim3((unsigned)((chunk_tiles + per_wg - 1) / per_wg)),
                  dim3(per_wg * 64), 0, s, T, nl, H, tile_base, chunk_tiles, norms, nstride, tmax,
                  nstride / kTile);
}
template <int DT, int NC>
static int launch_score_paged(const PagesChunk& C, int nl, int H, int64_t tile_base,
                              int64_t chunk_tiles, char* norms, int64_t nstride, uint32_t* tmax,
                              uint32_t* status, hipStream_t s) {
  constexpr int per_wg = score_waves(NC);
  return launch_k(score_paged_kernel<DT, NC>, dim3((unsigned)((chunk_tiles + per_wg - 1) / per_wg)),
                  dim3(per_wg * 64), 0, s, C, nl, H, tile_base, chunk_tiles, norms, nstride, tmax,
                  nstride / kTile, status);
}

// `work` = max n_out over the chunk's layers; grid = (rows, token blocks)
// KVC_FLAG_GATHER_FIXED launches (copies meant to run beside a selection on another stream) use
// at most this many workgroups: two of four waves per CU
// (A/B: an uncapped grid starves the heap select beside it -- the S = 16 384 h2o_attention call
// 0.155 -> 0.216 ms, 1 024 blocks 0.208; tools/ab_variants.txt fgfull / fg1024)
constexpr int kFixedGatherBlocks = 512;
template <int DT, int NC>
static int launch_gather(const LayerChunk& T, int nl, int H, int BH, const int32_t* idx,
                         int64_t istride, int shared, uint32_t* status, int64_t work, int part,
                         hipStream_t s) {
  const int rows = nl * BH, nby = (int)((work + kGatherTokens - 1) / kGatherTokens);
  if (part == PART_FIXED && (int64_t)rows * nby > kFixedGatherBlocks)
    return launch_k(gather_kernel<DT, NC>, dim3(kFixedGatherBlocks), dim3(kGatherThreads), 0, s, T,
                    H, BH, idx, istride, shared, status, part, rows, nby);
  return launch_k(gather_kernel<DT, NC>, dim3((unsigned)rows, (unsigned)nby),
                  dim3(kGatherThreads), 0, s, T, H, BH, idx, istride, shared, status, part, 0, nby);
}

// Grid of a gather_passes kernel: (rows, passes of the longest output that is not in place); an
// in-place row (in_place(l) != 0) is one workgroup's
template <int NC, typename F>
static dim3 pass_grid(const kvc_layer_t* layers, int nl, int BH, F&& in_place) {
  int64_t work = 0;  // longest output copied by token blocks
  for (int l = 0; l < nl; ++l)
    if (!in_place(l) && layers[l].n_out > work) work = layers[l].n_out;
  constexpr int rows_per = dest_pass_rows(NC);
  const int nby = work > 0 ? (int)((work + rows_per - 1) / rows_per) : 1;
  return dim3((unsigned)(nl * BH), (unsigned)nby);
}

// GATHER of a dest launch
template <int DT, int NC>
static int launch_gather_dest(const LayerChunk& T, const kvc_dest_t* dests, int nl, int H, int BH,
                              const int32_t* idx, int64_t istride, int shared, uint32_t* status,
                              hipStream_t s) {
  DestChunk D;
  memset(&D, 0, sizeof(D));
  memcpy(D.d, dests, (size_t)nl * sizeof(kvc_dest_t));
  const dim3 grid = pass_grid<NC>(T.l, nl, BH, [&](int l) { return dests[l].in_place; });
  return launch_k(gather_dest_kernel<DT, NC>, grid, dim3(kGatherThreads), 0, s, T, D, H, BH, idx,
                  istride, shared, status);
}

// The by-value tables of a paged chunk (<= kPagedLayers layers): layers, page descriptions, and
// the dense outputs' strides -- the caller's kvc_dest_t, or those of a contiguous k_out / v_out.
static void fill_pages_chunk(PagesChunk* C, const kvc_params_t* p, const kvc_layer_t* layers,
                             const kvc_pages_t* pages, const kvc_dest_t* dests, int nl) {
  memset(C, 0, sizeof(*C));
  memcpy(C->l, layers, (size_t)nl * sizeof(kvc_layer_t));
  memcpy(C->p, pages, (size_t)nl * sizeof(kvc_pages_t));
  for (int l = 0; l < nl; ++l) {
    if (pages[l].in_place) continue;
    if (dests) {
      C->d[l] = dests[l];
      continue;
    }
    const int64_t n = layers[l].n_out, D = p->head_dim;
    const int64_t st[3] = {(int64_t)p->heads * n * D, n * D, D};
    memcpy(C->d[l].k_stride, st, sizeof(st));
    memcpy(C->d[l].v_stride, st, sizeof(st));
  }
}

// GATHER of a paged launch
template <int DT, int NC>
static int launch_gather_paged(const PagesChunk& C, int nl, int H, int BH, const int32_t* idx,
                               int64_t istride, int shared, uint32_t* status, hipStream_t s) {
  const dim3 grid = pass_grid<NC>(C.l, nl, BH, [&](int l) { return C.p[l].in_place; });
  return launch_k(gather_paged_kernel<DT, NC>, grid, dim3(kGatherThreads), 0, s, C, H, BH, idx,
                  istride, shared, status);
}

// GATHER of a repage chunk (kvc_repage.h): grid (rows, passes of the chunk's longest output --
// a ragged layer's envelope), the chunk's tables by value; the scale-carrying instances (fp8 rows,
// cn <= kRepageScLayers) when scales move.  The chunk is layers c0 .. c0 + cn of the tables.
template <typename C>
static void fill_repage_tables(C* c, const kvc_layer_t* layers, const kvc_pages_t* pages,
                               const kvc_page_dest_t* pdests, int cn) {
  memset(c, 0, sizeof(*c));
  memcpy(c->l, layers, (size_t)cn * sizeof(kvc_layer_t));
  memcpy(c->p, pages, (size_t)cn * sizeof(kvc_pages_t));
  memcpy(c->d, pdests, (size_t)cn * sizeof(kvc_page_dest_t));
}
template <int DT, int NC>
static int launch_gather_repage(const kvc_layer_t* all_layers, const Tables& t, int c0, int cn,
                                int H, int BH, const int32_t* idx, int64_t istride, int shared,
                                uint32_t* status, hipStream_t s) {
  const kvc_layer_t* layers = all_layers + c0;
  const kvc_pages_t* pages = t.pages + c0;
  const kvc_page_dest_t* pdests = t.pdests + c0;
  const kvc_ragged_t* ragged = t.ragged ? t.ragged + c0 : nullptr;
  const kvc_scales_t* scales = t.scales ? t.scales + c0 : nullptr;
  const kvc_scales_t* dscales = t.scales ? t.dscales + c0 : nullptr;
  const dim3 grid = pass_grid<NC>(layers, cn, BH, [](int) { return 0; });
  if (scales) {
    if constexpr (is_fp8(DT)) {
      if (cn > kRepageScLayers) return KVC_E_ARG;
      if (ragged) {
        RepageRaggedScChunk C;
        fill_repage_tables(&C, layers, pages, pdests, cn);
        memcpy(C.z, scales, (size_t)cn * sizeof(kvc_scales_t));
        memcpy(C.dz, dscales, (size_t)cn * sizeof(kvc_scales_t));
        for (int l = 0; l < cn; ++l) C.s[l] = ragged[l].dev;
        return launch_k(gather_repage_ragged_sc_kernel<DT, NC>, grid, dim3(kGatherThreads), 0, s,
                        C, H, BH, idx, istride, status);
      }
      RepageScChunk C;
      fill_repage_tables(&C, layers, pages, pdests, cn);
      memcpy(C.z, scales, (size_t)cn * sizeof(kvc_scales_t));
      memcpy(C.dz, dscales, (size_t)cn * sizeof(kvc_scales_t));
      return launch_k(gather_repage_sc_kernel<DT, NC>, grid, dim3(kGatherThreads), 0, s, C, H, BH,
                      idx, istride, shared, status);
    } else {
      return KVC_E_DTYPE;  // (plan_tables: scales belong to fp8 rows)
    }
  }
  if (ragged) {
    RepageRaggedChunk C;
    fill_repage_tables(&C, layers, pages, pdests, cn);
    for (int l = 0; l < cn; ++l) C.s[l] = ragged[l].dev;
    return launch_k(gather_repage_ragged_kernel<DT, NC>, grid, dim3(kGatherThreads), 0, s, C, H,
                    BH, idx, istride, status);
  }
  RepageChunk C;
  fill_repage_tables(&C, layers, pages, pdests, cn);
  return launch_k(gather_repage_kernel<DT, NC>, grid, dim3(kGatherThreads), 0, s, C, H, BH, idx,
                  istride, shared, status);
}

// The 512-thread selection kernels (zones up to kSmallZone) over n_cap positions: the candidate
// capacity that fits the LDS budget (*cap) and the dynamic LDS bytes; wave segment kWaveSegSmall
static size_t small_sel_lds(int n_cap, int key_size, int* cap) {
  *cap = sel_cap(n_cap, key_size, kSmallBudget);
  return sel_bytes(n_cap, key_size, *cap);
}

// SELECT over the rows of a chunk (BH rows per layer, workspace row ly->row0 + blockIdx % BH):
// the LDS kernels (512-thread rows for zones up to kSmallZone, else 1 024-thread rows) or, for
// zones longer than kZoneMax, the global-scratch kernels (u32 positions beyond kZoneMaxGlobal).
template <int KC, bool HH = false>
static int launch_select(const LayerChunk& T, int cn, int BH, int dt, int order, int algo,
                         const char* norms, int64_t nstride, int32_t* idx, int64_t istride,
                         bool long_zone, char* scratch, uint64_t* stamps, uint32_t* status,
                         hipStream_t s, const uint32_t* tmax = nullptr) {
  typedef typename DTypeTraits<KC>::key_t KeyT;
  const dim3 rows_grid((unsigned)(cn * BH));
  const int n_cap = (int)nstride;  // longest zone of the call, rounded to 64
  if (long_zone) {
    const int64_t rb = (int64_t)sel_scratch_row_bytes(n_cap, KC);
    if (n_cap > kZoneMaxGlobal)  // u32 positions (the call's longest zone decides)
      return launch_k(select_long_kernel<KC>, rows_grid, dim3(kSelThreads), 0, s, T, BH, dt,
                      order, algo, norms, nstride, idx, istride, scratch, rb, n_cap, status);
    if (algo == KVC_ALGO_STABLE)
      return launch_k(select_global_kernel<KC, true>, rows_grid, dim3(kSelThreads), 0, s, T, BH,
                      dt, order, algo, norms, nstride, idx, istride, kWaveSeg, scratch, rb, n_cap,
                      status);
    return launch_k(select_global_kernel<KC>, rows_grid, dim3(kSelThreads), 0, s, T, BH, dt,
                    order, algo, norms, nstride, idx, istride, kWaveSeg, scratch, rb, n_cap,
                    status);
  }
  const int ks = (int)sizeof(KeyT);
  const auto go = [&](auto stable) {
    constexpr bool ST = decltype(stable)::value;
    if (n_cap <= kSmallZone) {
      int cap;
      const size_t lds = small_sel_lds(n_cap, ks, &cap);
      return launch_k(select_kernel<KC, kSelThreadsSmall, HH, ST>, rows_grid,
                      dim3(kSelThreadsSmall), lds, s, T, BH, dt, order, algo, norms, nstride, idx,
                      istride, kWaveSegSmall, n_cap, cap, stamps, status, tmax);
    }
    return launch_k(select_kernel<KC, kSelThreads, HH, ST>, rows_grid, dim3(kSelThreads), 0, s, T,
                    BH, dt, order, algo, norms, nstride, idx, istride, kWaveSeg, n_cap, 0, stamps,
                    status, tmax);
  };
  if (algo == KVC_ALGO_STABLE) return go(std::true_type());
  return go(std::false_type());
}

// What a chunk's launcher reads off the plan and the chunk's layers (c0 .. c0 + cn of nl) before
// it launches anything: the workspace regions, the chunk's range of SCORE tiles, what its layers
// ask of SELECT and GATHER, and the chunk's scale descriptions by value.
struct ChunkPlan {
  int H, BH;
  char* norms;
  int32_t* idx;
  int64_t nstride, istride;     // of the norm / index rows
  int64_t tile_base, tile_end;  // the chunk's SCORE tiles
  int part;                     // KVC_FLAG_GATHER_FIXED / _SELECTED launches: the rows they copy
  bool sel, snap, long_zone;    // some layer keeps selected rows / scores snapkv / needs scratch
  int64_t max_out, max_part;    // longest output; longest output of this launch's `part`
  uint32_t* status;
  uint32_t* tmax;   // snapkv rows: SCORE's per-tile norm maxima (plan_impl reserved them)
  ScalesChunk ZC;   // filled for scaled launches only (fp8: plan_tables)
};
static ChunkPlan chunk_plan(const kvc_params_t* p, const kvc_plan_info_t& info,
                            const kvc_layer_t* layers, const Tables& t, int nl, int c0, int cn,
                            char* w) {
  ChunkPlan c;
  c.H = p->heads, c.BH = p->batch * p->heads;
  c.norms = w + info.norm_offset;
  c.idx = reinterpret_cast<int32_t*>(w + info.index_offset);
  c.nstride = info.norm_row_stride, c.istride = info.index_row_stride;
  c.tile_base = layers[c0].tile0;
  c.tile_end = c0 + cn < nl ? (int64_t)layers[c0 + cn].tile0 : info.score_tiles;
  c.part = (p->flags & KVC_FLAG_GATHER_FIXED)      ? PART_FIXED
           : (p->flags & KVC_FLAG_GATHER_SELECTED) ? PART_SELECTED
                                                   : PART_ALL;
  c.sel = c.long_zone = c.snap = false;
  c.max_out = c.max_part = 0;
  for (int l = c0; l < c0 + cn; ++l) {
    c.sel |= layers[l].n_select > 0;
    c.snap |= layer_selects(layers[l]) && layers[l].score_mode == KVC_SCORE_SNAPKV;
    c.long_zone |= layer_selects(layers[l]) && layers[l].zone_len > kZoneMax;
    c.max_out = layers[l].n_out > c.max_out ? layers[l].n_out : c.max_out;
    const int64_t pr = part_rows(layers[l], c.part);
    c.max_part = pr > c.max_part ? pr : c.max_part;
  }
  c.status = p->device_status;
  c.tmax = c.snap && !p->external_index
               ? reinterpret_cast<uint32_t*>(w + tmax_offset(info, p->dtype))
               : nullptr;
  if (t.scales) {
    memset(&c.ZC, 0, sizeof(c.ZC));
    memcpy(c.ZC.s, t.scales + c0, (size_t)cn * sizeof(kvc_scales_t));
  }
  return c;
}

// One chunk of <= kArgLayers layers: SCORE, then SELECT_GATHER (or SELECT and GATHER as two
// kernels with KVC_FLAG_SPLIT_SELECT_GATHER, or GATHER alone for copy-only / external-index
// calls), each kernel with the chunk's table by value.
// t.dests (kvc_launch_dest): SELECT and GATHER always as two kernels, the GATHER into the layers'
// destinations (gather_dest_kernel).
// t.pages (kvc_launch_paged; cn <= kPagedLayers): SCORE and GATHER read K / V through the layers'
// block tables (kvc_paged.h), SELECT as with dests.
// t.scales (kvc_launch_scaled; fp8, paged): SCORE and GATHER are the scaled instances, which also
// read / move the layers' scale words.
// t.pdests (kvc_launch_repage; paged, out of place): SCORE and SELECT as above, GATHER through the
// layers' destination tables (launch_gather_repage).
template <int DT, int NC>
static int launch_chunk(const kvc_params_t* p, const kvc_plan_info_t& info, const kvc_layer_t* layers,
                        const Tables& t, int nl, int c0, int cn, char* w, hipStream_t s) {
  typedef typename DTypeTraits<DT>::key_t KeyT;
  constexpr int KC = DT == KVC_F32 ? KVC_F32 : KVC_BF16;  // selection binary: the key class
  constexpr int SDT = score_dt(DT);  // the selection's runtime dtype (bf16 for fp8 rows)
  constexpr bool F8 = is_fp8(DT);    // the fused kernel's row copy: bytes, no NaN rewrite
  const ChunkPlan c = chunk_plan(p, info, layers, t, nl, c0, cn, w);
  const int H = c.H, BH = c.BH, part = c.part;
  char* const norms = c.norms;
  int32_t* const idx = c.idx;
  const int64_t nstride = c.nstride, istride = c.istride;
  const int64_t tile_base = c.tile_base, tile_end = c.tile_end;
  uint32_t* const status = c.status;
  uint32_t* const tmax = c.tmax;
  const kvc_dest_t* dests = t.dests;
  const kvc_pages_t* pages = t.pages;
  const kvc_scales_t* scales = t.scales;
#ifdef KVC_STAMPS
  uint64_t* stamps = reinterpret_cast<uint64_t*>(w + info.workspace_bytes - info.rows * 256);
#else
  uint64_t* stamps = nullptr;
#endif
  LayerChunk T;
  memcpy(T.l, layers + c0, (size_t)cn * sizeof(kvc_layer_t));
  const bool ext = p->external_index != 0;
  int rc = KVC_OK;
  PagesChunk PC;  // filled for paged launches only
  if (pages) fill_pages_chunk(&PC, p, layers + c0, pages + c0, dests ? dests + c0 : nullptr, cn);
  const ScalesChunk& ZC = c.ZC;
  if constexpr (is_fp8(DT)) {
    if (scales && (p->phases & KVC_PHASE_SCORE) && tile_end > tile_base && !ext) {
      constexpr int per_wg = score_waves(NC);
      const int64_t chunk_tiles = tile_end - tile_base;
      rc = launch_k(score_paged_scaled_kernel<DT, NC>,
                    dim3((unsigned)((chunk_tiles + per_wg - 1) / per_wg)), dim3(per_wg * 64), 0, s,
                    PC, ZC, cn, H, tile_base, chunk_tiles, norms, nstride, tmax, nstride / kTile,
                    status);
    }
  }
  if ((p->phases & KVC_PHASE_SCORE) && tile_end > tile_base && !ext && !scales)
    rc = pages ? launch_score_paged<DT, NC>(PC, cn, H, tile_base, tile_end - tile_base, norms,
                                            nstride, tmax, status, s)
               : launch_score<DT, NC>(T, cn, H, tile_base, tile_end - tile_base, norms, nstride,
                                      tmax, s);
  if (rc != KVC_OK) return rc;
  const int n_cap = (int)nstride;  // longest zone of the call, rounded to 64
  if ((p->phases & KVC_PHASE_SELECT) && c.sel && !ext) {
    const bool fuse_sg = (p->phases & KVC_PHASE_GATHER) && c.max_out > 0 && !stamps &&
                         !c.long_zone && part == PART_ALL && !dests && !pages &&
                         !(p->flags & KVC_FLAG_SPLIT_SELECT_GATHER);
    if (fuse_sg) {  // this chunk's gather happens inside the select kernel
      const int rows = cn * BH;
      const dim3 rows_grid((unsigned)rows);
      const int ks = (int)sizeof(KeyT);
      const auto go = [&](auto stable) {
        constexpr bool ST = decltype(stable)::value;
        if (n_cap <= kSmallZone) {
          int cap;
          const size_t lds = small_sel_lds(n_cap, ks, &cap);
          return launch_k(select_gather_kernel<KC, kSelThreadsSmall, NC, ST, true, F8>, rows_grid,
                          dim3(kSelThreadsSmall), lds, s, T, H, BH, SDT, p->order, p->algo, norms,
                          nstride, kWaveSegSmall, n_cap, cap, status, 0, tmax);
        }
        // fewer rows than CUs (e.g. 4 layers per GPU of an 8-way layer split): one row per CU
        // and idle CUs -- the sink / tail rows get copy-only workgroups of their own
        bool fixed = false, plain = false;
        for (int l = c0; l < c0 + cn; ++l) {
          fixed |= layer_selects(layers[l]) && layers[l].sink_len + layers[l].tail_len > 0;
          plain |= layer_selects(layers[l]) && layers[l].score_mode == KVC_SCORE_NORM;
        }
        const int split = fixed && rows <= kSplitCopyRows ? rows : 0;
        const dim3 grid((unsigned)(split ? 2 * rows : rows));
        // Level 0's idx-region rank tables (run_chain) pay on launches with plain-norm rows;
        // snapkv-only launches run faster in the instance without that code
        // (profiles/r06_h_l0t_instance_ab.jsonl: headline snapkv 0.1770 -> 0.1715 ms; with one
        // row per CU the tables still win for cfg4 ranks, 0.0467 -> 0.0427, and lose 2 us for
        // cfg5 pyramid ones)
        if constexpr (!ST) {
          if (plain)
            return launch_k(select_gather_kernel<KC, kSelThreads, NC, ST, true, F8>, grid,
                            dim3(kSelThreads), 0, s, T, H, BH, SDT, p->order, p->algo, norms,
                            nstride, kWaveSeg, n_cap, 0, status, split, tmax);
        }
        return launch_k(select_gather_kernel<KC, kSelThreads, NC, ST, false, F8>, grid,
                        dim3(kSelThreads), 0, s, T, H, BH, SDT, p->order, p->algo, norms, nstride,
                        kWaveSeg, n_cap, 0, status, split, tmax);
      };
      return p->algo == KVC_ALGO_STABLE ? go(std::true_type()) : go(std::false_type());
    }
    char* scratch = w + round_up(info.index_offset + (size_t)info.rows * istride * 4, 256);
    uint64_t* st = stamps ? stamps + (size_t)layers[c0].row0 * 32 : nullptr;
    rc = launch_select<KC>(T, cn, BH, SDT, p->order, p->algo, norms, nstride, idx, istride,
                           c.long_zone, scratch, st, status, s, tmax);
  }
  if (rc != KVC_OK) return rc;
  if (!((p->phases & KVC_PHASE_GATHER) && c.max_part > 0)) return rc;  // no GATHER to run
  const int shared = (p->flags & KVC_FLAG_SHARED_INDEX) ? 1 : 0;
  if (t.pdests)
    return launch_gather_repage<DT, NC>(layers, t, c0, cn, H, BH, idx, istride, shared, status, s);
  if constexpr (is_fp8(DT)) {
    if (scales)  // every layer in place
      return launch_k(gather_paged_scaled_kernel<DT, NC>, dim3((unsigned)(cn * BH)),
                      dim3(kGatherThreads), 0, s, PC, ZC, H, BH, static_cast<const int32_t*>(idx),
                      istride, shared, status);
  }
  if (pages) return launch_gather_paged<DT, NC>(PC, cn, H, BH, idx, istride, shared, status, s);
  if (dests)
    return launch_gather_dest<DT, NC>(T, dests + c0, cn, H, BH, idx, istride, shared, status, s);
  return launch_gather<DT, NC>(T, cn, H, BH, idx, istride, shared, status, c.max_part, part, s);
}

// SELECT of a ragged chunk: launch_select's choice of kernel class by the call's longest
// (envelope) zone, with the instances that read each row's bounds from its record.
template <int KC>
static int launch_select_ragged(const RaggedChunk& C, int cn, int H, int BH, int dt, int order,
                                int algo, const char* norms, int64_t nstride, int32_t* idx,
                                int64_t istride, bool long_zone, char* scratch, uint32_t* status,
                                hipStream_t s, const uint32_t* tmax) {
  typedef typename DTypeTraits<KC>::key_t KeyT;
  const dim3 rows_grid((unsigned)(cn * BH));
  const int n_cap = (int)nstride;
  if (long_zone) {
    const int64_t rb = (int64_t)sel_scratch_row_bytes(n_cap, KC);
    if (n_cap > kZoneMaxGlobal)
      return launch_k(select_long_ragged_kernel<KC>, rows_grid, dim3(kSelThreads), 0, s, C, H, BH,
                      dt, order, algo, norms, nstride, idx, istride, scratch, rb, n_cap, status);
    if (algo == KVC_ALGO_STABLE)
      return launch_k(select_global_ragged_kernel<KC, true>, rows_grid, dim3(kSelThreads), 0, s, C,
                      H, BH, dt, order, algo, norms, nstride, idx, istride, kWaveSeg, scratch, rb,
                      n_cap, status);
    return launch_k(select_global_ragged_kernel<KC>, rows_grid, dim3(kSelThreads), 0, s, C, H, BH,
                    dt, order, algo, norms, nstride, idx, istride, kWaveSeg, scratch, rb, n_cap,
                    status);
  }
  const auto go = [&](auto stable) {
    constexpr bool ST = decltype(stable)::value;
    if (n_cap <= kSmallZone) {
      int cap;
      const size_t lds = small_sel_lds(n_cap, (int)sizeof(KeyT), &cap);
      return launch_k(select_ragged_kernel<KC, kSelThreadsSmall, ST>, rows_grid,
                      dim3(kSelThreadsSmall), lds, s, C, H, BH, dt, order, algo, norms, nstride,
                      idx, istride, kWaveSegSmall, n_cap, cap, status, tmax);
    }
    return launch_k(select_ragged_kernel<KC, kSelThreads, ST>, rows_grid, dim3(kSelThreads), 0, s,
                    C, H, BH, dt, order, algo, norms, nstride, idx, istride, kWaveSeg, n_cap, 0,
                    status, tmax);
  };
  if (algo == KVC_ALGO_STABLE) return go(std::true_type());
  return go(std::false_type());
}

// One chunk of <= kPagedLayers ragged layers: SCORE, SELECT and GATHER as three kernels, grids and
// kernel classes by the layers' envelopes (what plan_tables' ragged step left in the table), each
// row's bounds from its device record.  (A ragged call has no external index and copies every
// part: ChunkPlan's tmax and max_part are the plain ones.)
template <int DT, int NC>
static int launch_chunk_ragged(const kvc_params_t* p, const kvc_plan_info_t& info,
                               const kvc_layer_t* layers, const Tables& t, int nl, int c0, int cn,
                               char* w, hipStream_t s) {
  constexpr int KC = DT == KVC_F32 ? KVC_F32 : KVC_BF16;
  const ChunkPlan c = chunk_plan(p, info, layers, t, nl, c0, cn, w);
  const int H = c.H, BH = c.BH;
  char* const norms = c.norms;
  int32_t* const idx = c.idx;
  const int64_t nstride = c.nstride, istride = c.istride;
  uint32_t* const status = c.status;
  uint32_t* const tmax = c.tmax;
  const ScalesChunk& ZC = c.ZC;
  RaggedChunk C;
  memset(&C, 0, sizeof(C));
  memcpy(C.l, layers + c0, (size_t)cn * sizeof(kvc_layer_t));
  memcpy(C.p, t.pages + c0, (size_t)cn * sizeof(kvc_pages_t));
  for (int l = 0; l < cn; ++l) C.s[l] = t.ragged[c0 + l].dev;
  int rc = KVC_OK;
  if ((p->phases & KVC_PHASE_SCORE) && c.tile_end > c.tile_base) {  // some envelope selects
    int64_t zmax = 0;  // the chunk's longest selecting envelope zone
    for (int l = c0; l < c0 + cn; ++l)
      if (layer_selects(layers[l]) && layers[l].zone_len > zmax) zmax = layers[l].zone_len;
    const int64_t per_block = (int64_t)kRaggedTiles * kTile;
    const dim3 grid((unsigned)(cn * BH), (unsigned)((zmax + per_block - 1) / per_block));
    bool done = false;
    if constexpr (is_fp8(DT)) {
      if (t.scales) {
        rc = launch_k(score_ragged_scaled_kernel<DT, NC>, grid, dim3(score_waves(NC) * 64), 0, s,
                      C, ZC, H, BH, norms, nstride, tmax, nstride / kTile, status);
        done = true;
      }
    }
    if (!done)
      rc = launch_k(score_ragged_kernel<DT, NC>, grid, dim3(score_waves(NC) * 64), 0, s, C, H, BH,
                    norms, nstride, tmax, nstride / kTile, status);
  }
  if (rc != KVC_OK) return rc;
  if ((p->phases & KVC_PHASE_SELECT) && c.sel) {
    char* scratch = w + round_up(info.index_offset + (size_t)info.rows * istride * 4, 256);
    rc = launch_select_ragged<KC>(C, cn, H, BH, score_dt(DT), p->order, p->algo, norms, nstride, idx,
                                  istride, c.long_zone, scratch, status, s, tmax);
  }
  if (rc != KVC_OK) return rc;
  if (!((p->phases & KVC_PHASE_GATHER) && c.max_out > 0)) return rc;  // no GATHER to run
  if (t.pdests)  // out of place, through the destination tables (every row has its own indices)
    return launch_gather_repage<DT, NC>(layers, t, c0, cn, H, BH, idx, istride, 0, status, s);
  if constexpr (is_fp8(DT)) {
    if (t.scales)
      return launch_k(gather_ragged_scaled_kernel<DT, NC>, dim3((unsigned)(cn * BH)),
                      dim3(kGatherThreads), 0, s, C, ZC, H, BH, static_cast<const int32_t*>(idx),
                      istride, status);
  }
  return launch_k(gather_ragged_kernel<DT, NC>, dim3((unsigned)(cn * BH)), dim3(kGatherThreads), 0,
                  s, C, H, BH, static_cast<const int32_t*>(idx), istride, status);
}

// The launch of every entry point: the plan again (comparing, not filling), then the layers in
// argument chunks, each through the launcher of its dtype and row width.
static int launch_tables(const kvc_params_t* p, const kvc_layer_t* layers, const Tables& t, int nl,
                         void* ws, size_t ws_bytes, kvc_stream_t stream) {
  kvc_plan_info_t info;
  int rc = plan_tables(p, const_cast<kvc_layer_t*>(layers), t, nl, &info, false);
  if (rc != KVC_OK) return rc;
  if (nl == 0) return KVC_OK;
  if (!ws || ws_bytes < info.workspace_bytes) return KVC_E_WORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(ws);
  const int nc = p->head_dim * esize(p->dtype) / 16;
  // layers per argument chunk: paged chunks carry more tables per layer, and the scale-carrying
  // copy through destination tables two scale descriptions as well
  const int step = !t.pages ? kArgLayers : (t.pdests && t.scales) ? kRepageScLayers : kPagedLayers;
  for (int c0 = 0; c0 < nl && rc == KVC_OK; c0 += step) {
    const int cn = nl - c0 < step ? nl - c0 : step;
    rc = with_kv_dtype(p->dtype, [&](auto dt) {
      return with_nc_dt<decltype(dt)::value>(nc, [&](auto ncv) {
        constexpr int DT = decltype(dt)::value, NC = decltype(ncv)::value;
        if (t.ragged) return launch_chunk_ragged<DT, NC>(p, info, layers, t, nl, c0, cn, w, s);
        return launch_chunk<DT, NC>(p, info, layers, t, nl, c0, cn, w, s);
      });
    });
  }
  return rc;
}

// kvc_debug_select_capacity: the 512-thread SELECT / SELECT_GATHER kernels of one chunk with a
// caller-chosen zone capacity (the device-side bounds check's test hook)
static int debug_select_impl(const kvc_params_t* p, const kvc_layer_t* layers, int nl, char* w,
                             size_t wbytes, int zone_cap, hipStream_t s) {
  kvc_plan_info_t info;
  int rc = plan_impl(p, const_cast<kvc_layer_t*>(layers), nl, &info, false);
  if (rc != KVC_OK) return rc;
  if (nl < 1 || nl > kArgLayers || zone_cap < kTile || zone_cap > kSmallZone ||
      zone_cap % kTile || p->external_index || p->algo == KVC_ALGO_STABLE ||
      (p->phases != KVC_PHASE_SELECT && p->phases != (KVC_PHASE_SELECT | KVC_PHASE_GATHER)))
    return KVC_E_ARG;
  if (!w || wbytes < info.workspace_bytes) return KVC_E_WORKSPACE;
  LayerChunk T;
  memcpy(T.l, layers, (size_t)nl * sizeof(kvc_layer_t));
  const int H = p->heads, BH = p->batch * p->heads;
  const char* norms = w + info.norm_offset;
  int32_t* idx = reinterpret_cast<int32_t*>(w + info.index_offset);
  const dim3 grid((unsigned)(nl * BH));
  const int nc = p->head_dim * esize(p->dtype) / 16;
  return with_kv_dtype(p->dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    constexpr int KC = DT == KVC_F32 ? KVC_F32 : KVC_BF16;
    constexpr int SDT = score_dt(DT);
    int cap;
    const size_t lds = small_sel_lds(zone_cap, (int)sizeof(typename DTypeTraits<KC>::key_t), &cap);
    if (p->phases == KVC_PHASE_SELECT)
      return launch_k(select_kernel<KC, kSelThreadsSmall>, grid, dim3(kSelThreadsSmall), lds, s,
                      T, BH, SDT, p->order, p->algo, norms, info.norm_row_stride, idx,
                      info.index_row_stride, kWaveSegSmall, zone_cap, cap,
                      static_cast<uint64_t*>(nullptr), p->device_status,
                      static_cast<const uint32_t*>(nullptr));
    return with_nc_dt<DT>(nc, [&](auto ncv) {
      return launch_k(select_gather_kernel<KC, kSelThreadsSmall, decltype(ncv)::value, false, true,
                                           is_fp8(DT)>,
                      grid, dim3(kSelThreadsSmall), lds, s, T, H, BH, SDT, p->order, p->algo, norms,
                      info.norm_row_stride, kWaveSegSmall, zone_cap, cap, p->device_status, 0,
                      static_cast<const uint32_t*>(nullptr));
    });
  });
}

// ---- h2o_attention host side ----------------------------------------------------------------
static int attn_params_check(const kvc_attn_params_t* p, bool accumulate = false) {
  if (!p) return KVC_E_ARG;
  if (p->dtype != KVC_BF16 && p->dtype != KVC_F16 && p->dtype != KVC_F32) return KVC_E_DTYPE;
  if (p->batch < 1 || p->heads < 1) return KVC_E_ARG;
  // flags: kvc_attn_accumulate's KVC_ATTN_OLD_DTYPE(d) only (d a dtype other than p->dtype)
  // flags: KVC_ATTN_HH_STABLE (both entry points: one params struct serves a decode step's
  // accumulate and heavy-hitter calls) | kvc_attn_accumulate's KVC_ATTN_OLD_DTYPE(d), bits 0-1,
  // d a dtype other than p->dtype
  // KVC_ATTN_SCALAR_SUM: kvc_attn_accumulate only
  const int od = p->flags & 3;
  if ((p->flags & ~(3 | KVC_ATTN_HH_STABLE | (accumulate ? KVC_ATTN_SCALAR_SUM : 0))) ||
      (od && (!accumulate || od == KVC_ATTN_OLD_DTYPE(p->dtype))))
    return KVC_E_ARG;
  if (p->vec_bytes < 16 || p->vec_bytes > 64 || p->vec_bytes % 16) return KVC_E_ARG;
  if ((int64_t)p->batch * p->heads > 0x7FFFFFFF / kArgLayers) return KVC_E_ARG;
  return KVC_OK;
}

static int accumulate_impl(const kvc_attn_params_t* p, const kvc_attn_layer_t* layers, int nl,
                           hipStream_t s) {
  int rc = attn_params_check(p, true);
  if (rc != KVC_OK) return rc;
  if (nl < 0 || (nl > 0 && !layers)) return KVC_E_ARG;
  const int es = esize(p->dtype);
  const int od = p->flags & 3;                 // KVC_ATTN_OLD_DTYPE bits
  const int odt = od ? od - 1 : p->dtype;      // acc_old's dtype
  const int oes = esize(odt), nes = od ? 4 : es;
  for (int l = 0; l < nl; ++l) {
    const kvc_attn_layer_t& y = layers[l];
    if (!y.attn || !y.acc_new || y.q_len < 1 || y.key_len < 1 || y.old_len < 0 ||
        y.old_len > y.key_len || (y.old_len > 0 && !y.acc_old) || y.col_chunk < 0 ||
        (od && y.old_len == 0) || (uintptr_t)y.attn % es ||
        (uintptr_t)y.acc_new % nes || (uintptr_t)y.acc_old % oes)
      return KVC_E_ARG;
    if ((y.key_len + kColThreads * kAccCols - 1) / (kColThreads * kAccCols) > 65535)
      return KVC_E_TOO_LONG;
  }
  const int H = p->heads, BH = p->batch * p->heads;
  // KVC_ATTN_SCALAR_SUM (the reference summed a last-dim-strided tensor): aten's scalar outer
  // loop -- groups of four columns in every call, thread chunk bounds not rounded
  const bool scalar = (p->flags & KVC_ATTN_SCALAR_SUM) != 0;
  const int group = scalar ? 4 : 4 * (p->vec_bytes / 4), vec_min = scalar ? 1 : p->vec_bytes / es;
  const int rnd = scalar ? 1 : 128 / es;
  for (int c0 = 0; c0 < nl && rc == KVC_OK; c0 += kArgLayers) {
    const int cn = nl - c0 < kArgLayers ? nl - c0 : kArgLayers;
    AttnChunk T;
    memcpy(T.l, layers + c0, (size_t)cn * sizeof(kvc_attn_layer_t));
    int kmax = 0;
    for (int l = 0; l < cn; ++l) kmax = T.l[l].key_len > kmax ? T.l[l].key_len : kmax;
    const int cols = kColThreads * kAccCols;
    const dim3 grid((unsigned)(cn * BH), (unsigned)((kmax + cols - 1) / cols));
    rc = with_dtype(p->dtype, [&](auto dt) {
      return with_dtype(odt, [&](auto od) {
        return launch_k(attn_accum_kernel<decltype(dt)::value, decltype(od)::value>, grid,
                        dim3(kColThreads), 0, s, T, H, BH, p->decay, group, vec_min, rnd);
      });
    });
  }
  return rc;
}

// Workspace of kvc_heavy_hitters: head-summed rows [layers * batch, nstride] of dtype, then the
// global selection scratch rows when a zone is longer than kZoneMax.
static int hh_layout(const kvc_attn_params_t* p, const kvc_hh_layer_t* layers, int nl,
                     int64_t* nstride, size_t* sums_bytes, size_t* total) {
  int rc = attn_params_check(p);
  if (rc != KVC_OK) return rc;
  if (nl < 0 || (nl > 0 && !layers)) return KVC_E_ARG;
  int64_t mmax = 1;
  for (int l = 0; l < nl; ++l) {
    const kvc_hh_layer_t& y = layers[l];
    if (!y.acc || y.acc_len < 1 || y.zone_start < 0 || y.zone_len < 1 ||
        (int64_t)y.zone_start + y.zone_len > y.acc_len || y.n_select < 0 ||
        y.n_select > y.zone_len || y.col_chunk < 0 || y.reserved != 0 ||
        (uintptr_t)y.acc % esize(p->dtype))
      return KVC_E_ARG;
    if (y.zone_len > kZoneMaxLong) return KVC_E_TOO_LONG;
    if ((p->flags & KVC_ATTN_HH_STABLE) && y.n_select < y.zone_len && y.zone_len > kZoneMaxGlobal)
      return KVC_E_TOO_LONG;  // the stable selection's longest zone, as kvc_plan
    mmax = y.zone_len > mmax ? y.zone_len : mmax;
  }
  const int64_t rows = (int64_t)nl * p->batch;
  *nstride = (int64_t)round_up((size_t)mmax, kTile);
  *sums_bytes = round_up((size_t)rows * *nstride * esize(p->dtype), 256);
  *total = *sums_bytes;
  if (mmax > kZoneMax) *total += (size_t)rows * sel_scratch_row_bytes((int)*nstride, p->dtype);
  return KVC_OK;
}

static int heavy_hitters_impl(const kvc_attn_params_t* p, const kvc_hh_layer_t* layers, int nl,
                              int32_t* out, int64_t ostride, char* w, size_t wbytes,
                              hipStream_t s) {
  int64_t nstride;
  size_t sums_bytes, total;
  int rc = hh_layout(p, layers, nl, &nstride, &sums_bytes, &total);
  if (rc != KVC_OK) return rc;
  if (nl == 0) return KVC_OK;
  if (!w || wbytes < total) return KVC_E_WORKSPACE;
  if (!out) return KVC_E_ARG;
  for (int l = 0; l < nl; ++l)
    if (layers[l].n_select > ostride) return KVC_E_ARG;
  const int B = p->batch, H = p->heads, es = esize(p->dtype);
  const int group = 4 * (p->vec_bytes / 4), vec_min = p->vec_bytes / es;
  for (int c0 = 0; c0 < nl && rc == KVC_OK; c0 += kArgLayers) {
    const int cn = nl - c0 < kArgLayers ? nl - c0 : kArgLayers;
    HHChunk T;
    memcpy(T.l, layers + c0, (size_t)cn * sizeof(kvc_hh_layer_t));
    LayerChunk S;  // the selection rows: zone = the head-summed row, chunk-local row0
    memset(&S, 0, sizeof(S));
    int mmax = 0;
    bool long_zone = false;
    for (int l = 0; l < cn; ++l) {
      S.l[l].zone_len = T.l[l].zone_len;
      S.l[l].n_select = T.l[l].n_select;
      S.l[l].seq_len = T.l[l].zone_len;
      S.l[l].score_mode = KVC_SCORE_NORM;
      S.l[l].row0 = l * B;
      mmax = T.l[l].zone_len > mmax ? T.l[l].zone_len : mmax;
      long_zone |= T.l[l].zone_len > kZoneMax;
    }
    char* sums = w + (size_t)c0 * B * nstride * es;
    char* scratch = w + sums_bytes + (size_t)c0 * B * sel_scratch_row_bytes((int)nstride, p->dtype);
    int32_t* o = out + (int64_t)c0 * B * ostride;
    const dim3 grid((unsigned)(cn * B), (unsigned)((mmax + kColThreads - 1) / kColThreads));
    rc = with_dtype(p->dtype, [&](auto dt) {
      constexpr int DT = decltype(dt)::value;
      constexpr int KC = DT == KVC_F32 ? KVC_F32 : KVC_BF16;
      int r = launch_k(head_sum_kernel<DT>, grid, dim3(kColThreads), 0, s, T, H, B, group,
                       vec_min, sums, nstride);
      if (r != KVC_OK) return r;
      // torch.topk(largest=True) + torch.sort: the descending TOPK selection, ascending indices
      const int algo = (p->flags & KVC_ATTN_HH_STABLE) ? KVC_ALGO_STABLE : KVC_ALGO_TOPK;
      return launch_select<KC, true>(S, cn, B, DT, KVC_DESC, algo, sums, nstride, o, ostride,
                               long_zone, scratch, nullptr, p->device_status, s);
    });
  }
  return rc;
}

}  // namespace kvc

extern "C" {

int kvc_version(void) { return KVC_ABI_VERSION; }
size_t kvc_layer_struct_size(void) { return sizeof(kvc_layer_t); }
int kvc_max_zone_len(void) { return kvc::kZoneMaxLong; }

#ifndef KVC_SOURCE_DIGEST
#define KVC_SOURCE_DIGEST "unknown"
#endif
const char* kvc_source_digest(void) { return KVC_SOURCE_DIGEST; }

const char* kvc_status_string(int s) {
  switch (s) {
    case KVC_OK: return "ok";
    case KVC_E_ARG: return "invalid argument";
    case KVC_E_DTYPE: return "unsupported dtype (bf16/fp16/fp32, fp8 e4m3fn/e5m2 K/V only)";
    case KVC_E_HEADDIM: return "unsupported head_dim";
    case KVC_E_ALIGN: return "pointer or stride not 16-byte aligned";
    case KVC_E_TOO_LONG: return "scored zone longer than kvc_max_zone_len()";
    case KVC_E_WORKSPACE: return "workspace too small";
    case KVC_E_HIP: return "HIP launch failure";
    default: return "unknown status";
  }
}

// The plan / launch pairs: each names the tables it has (kvc::Tables' order: dests, pages,
// ragged, scales, pdests, dscales) for kvc::plan_tables / kvc::launch_tables.
int kvc_plan(const kvc_params_t* params, kvc_layer_t* layers, int num_layers,
             kvc_plan_info_t* info) {
  return kvc::plan_tables(params, layers, {}, num_layers, info, true);
}

int kvc_launch(const kvc_params_t* p, const kvc_layer_t* layers, int nl, void* ws,
               size_t ws_bytes, kvc_stream_t stream) {
  return kvc::launch_tables(p, layers, {}, nl, ws, ws_bytes, stream);
}

int kvc_plan_dest(const kvc_params_t* params, kvc_layer_t* layers, const kvc_dest_t* dests,
                  int num_layers, kvc_plan_info_t* info) {
  return kvc::plan_tables(params, layers, {dests}, num_layers, info, true);
}

int kvc_launch_dest(const kvc_params_t* p, const kvc_layer_t* layers, const kvc_dest_t* dests,
                    int nl, void* ws, size_t ws_bytes, kvc_stream_t stream) {
  return kvc::launch_tables(p, layers, {dests}, nl, ws, ws_bytes, stream);
}

int kvc_plan_paged(const kvc_params_t* params, kvc_layer_t* layers, const kvc_pages_t* pages,
                   const kvc_dest_t* dests, int num_layers, kvc_plan_info_t* info) {
  return kvc::plan_tables(params, layers, {dests, pages}, num_layers, info, true);
}

int kvc_launch_paged(const kvc_params_t* p, const kvc_layer_t* layers, const kvc_pages_t* pages,
                     const kvc_dest_t* dests, int nl, void* ws, size_t ws_bytes,
                     kvc_stream_t stream) {
  return kvc::launch_tables(p, layers, {dests, pages}, nl, ws, ws_bytes, stream);
}

int kvc_plan_ragged(const kvc_params_t* params, kvc_layer_t* layers, const kvc_pages_t* pages,
                    const kvc_ragged_t* ragged, int num_layers, kvc_plan_info_t* info) {
  return kvc::plan_tables(params, layers, {nullptr, pages, ragged}, num_layers, info, true);
}

int kvc_launch_ragged(const kvc_params_t* p, const kvc_layer_t* layers, const kvc_pages_t* pages,
                      const kvc_ragged_t* ragged, int nl, void* ws, size_t ws_bytes,
                      kvc_stream_t stream) {
  return kvc::launch_tables(p, layers, {nullptr, pages, ragged}, nl, ws, ws_bytes, stream);
}

int kvc_plan_scaled(const kvc_params_t* params, kvc_layer_t* layers, const kvc_pages_t* pages,
                    const kvc_ragged_t* ragged, const kvc_scales_t* scales, int num_layers,
                    kvc_plan_info_t* info) {
  return kvc::plan_tables(params, layers, {nullptr, pages, ragged, scales}, num_layers, info,
                          true);
}

int kvc_launch_scaled(const kvc_params_t* p, const kvc_layer_t* layers, const kvc_pages_t* pages,
                      const kvc_ragged_t* ragged, const kvc_scales_t* scales, int nl, void* ws,
                      size_t ws_bytes, kvc_stream_t stream) {
  return kvc::launch_tables(p, layers, {nullptr, pages, ragged, scales}, nl, ws, ws_bytes,
                            stream);
}

int kvc_plan_repage(const kvc_params_t* params, kvc_layer_t* layers, const kvc_pages_t* pages,
                    const kvc_ragged_t* ragged, const kvc_scales_t* scales,
                    const kvc_page_dest_t* pdests, const kvc_scales_t* dscales, int num_layers,
                    kvc_plan_info_t* info) {
  return kvc::plan_tables(params, layers, {nullptr, pages, ragged, scales, pdests, dscales},
                          num_layers, info, true);
}

int kvc_launch_repage(const kvc_params_t* p, const kvc_layer_t* layers, const kvc_pages_t* pages,
                      const kvc_ragged_t* ragged, const kvc_scales_t* scales,
                      const kvc_page_dest_t* pdests, const kvc_scales_t* dscales, int nl, void* ws,
                      size_t ws_bytes, kvc_stream_t stream) {
  return kvc::launch_tables(p, layers, {nullptr, pages, ragged, scales, pdests, dscales}, nl, ws,
                            ws_bytes, stream);
}

int kvc_compress(const kvc_params_t* params, kvc_layer_t* layers, int num_layers, void* ws,
                 size_t ws_bytes, kvc_stream_t stream) {
  kvc_plan_info_t info;
  const int rc = kvc::plan_impl(params, layers, num_layers, &info, true);
  if (rc != KVC_OK) return rc;
  return kvc_launch(params, layers, num_layers, ws, ws_bytes, stream);
}

int kvc_debug_select_capacity(const kvc_params_t* params, const kvc_layer_t* layers,
                              int num_layers, void* workspace, size_t workspace_bytes,
                              int zone_cap, kvc_stream_t stream) {
  return kvc::debug_select_impl(params, layers, num_layers, static_cast<char*>(workspace),
                                workspace_bytes, zone_cap, reinterpret_cast<hipStream_t>(stream));
}

int kvc_attn_accumulate(const kvc_attn_params_t* params, const kvc_attn_layer_t* layers,
                        int num_layers, kvc_stream_t stream) {
  return kvc::accumulate_impl(params, layers, num_layers, reinterpret_cast<hipStream_t>(stream));
}

int kvc_hh_workspace(const kvc_attn_params_t* params, const kvc_hh_layer_t* layers,
                     int num_layers, size_t* bytes) {
  int64_t nstride;
  size_t sums, total;
  if (!bytes) return KVC_E_ARG;
  const int rc = kvc::hh_layout(params, layers, num_layers, &nstride, &sums, &total);
  if (rc == KVC_OK) *bytes = total;
  return rc;
}

int kvc_heavy_hitters(const kvc_attn_params_t* params, const kvc_hh_layer_t* layers,
                      int num_layers, int32_t* out_idx, int64_t out_row_stride, void* workspace,
                      size_t workspace_bytes, kvc_stream_t stream) {
  return kvc::heavy_hitters_impl(params, layers, num_layers, out_idx, out_row_stride,
                                 static_cast<char*>(workspace), workspace_bytes,
                                 reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
