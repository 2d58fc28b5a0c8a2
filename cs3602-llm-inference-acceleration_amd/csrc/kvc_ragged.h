// kvc_ragged.h -- ragged paged batches (kvc_launch_ragged): SCORE, SELECT and GATHER of paged
// layers whose B sequences each have their own length and segments (include/kvc.h, "Ragged paged
// batches").  The grids are those of the layer's ENVELOPE (kvc_plan_ragged: the longest zone,
// selection and output of its records); every workgroup or wave takes its row's bounds from the
// device record of (layer, b) -- one uniform 48-byte load -- and runs the paged tile, the
// selection bodies and the in-place pass schedule unchanged on a kvc_layer_t that carries them.
// Work past a sequence's own bounds returns before any other global load.
#pragma once

#include "kvc_paged.h"
#include "kvc_select.h"

namespace kvc {

// A ragged chunk's layers, page tables and device record pointers travel by value (6 KiB).
struct RaggedChunk {
  kvc_layer_t l[kPagedLayers];
  kvc_pages_t p[kPagedLayers];
  const kvc_seq_t* s[kPagedLayers];  // device: `batch` records of the layer
};

// Record *p (16-byte aligned, the same address in every lane), every field wave-uniform.
__device__ __forceinline__ kvc_seq_t load_seq(const kvc_seq_t* p) {
  static_assert(sizeof(kvc_seq_t) == 48, "three 16-byte loads");
  const int4* q = reinterpret_cast<const int4*>(p);
  const int4 a = q[0], b = q[1], c = q[2];
  kvc_seq_t r;
  r.seq_len = uni(a.x);
  r.zone_start = uni(a.y);
  r.zone_len = uni(a.z);
  r.n_select = uni(a.w);
  r.sink_len = uni(b.x);
  r.tail_start = uni(b.y);
  r.tail_len = uni(b.z);
  r.score_mode = uni(b.w);
  r.pool_kernel = uni(c.x);
  r.n_out = uni(c.y);
  r.reserved[0] = r.reserved[1] = 0;
  return r;
}

// The layer as sequence b sees it: pointers, strides and workspace rows of the (envelope) layer,
// segments of the record.  Callers read a handful of its fields; the rest is never materialised.
__device__ __forceinline__ kvc_layer_t seq_layer(const kvc_layer_t* ly, const kvc_seq_t& q) {
  kvc_layer_t y = *ly;
  y.seq_len = q.seq_len;
  y.zone_start = q.zone_start;
  y.zone_len = q.zone_len;
  y.n_select = q.n_select;
  y.sink_len = q.sink_len;
  y.tail_start = q.tail_start;
  y.tail_len = q.tail_len;
  y.score_mode = q.score_mode;
  y.pool_kernel = q.pool_kernel;
  y.n_out = q.n_out;
  return y;
}

// SCORE: score_paged_tile on a grid of (rows of the chunk, blocks of kRaggedTiles tiles of the
// longest envelope zone).  A workgroup's waves share out the tiles of its block that lie inside
// the row's OWN zone; a row that does not select, and the blocks past a row's zone, return after
// the record load.  Whole blocks rather than single tiles are the unit that can be idle: with one
// workgroup per 8 tiles a 600-row sequence beside a 16 384-row one launched 31 idle workgroups
// per row (each holding its LDS slab while it found that out), with blocks it launches 3.
// Norm and tile-maximum slots past a row's zone are never written and never read.
constexpr int kRaggedTiles = 64;
template <int DT, int NC>
__global__ void __launch_bounds__(score_waves(NC) * 64)
    score_ragged_kernel(const RaggedChunk T, int H, int BH, char* __restrict__ norms,
                        int64_t norm_stride, uint32_t* __restrict__ tmax, int64_t tmax_stride,
                        uint32_t* status) {
  constexpr int CP = score_cp(NC);
  constexpr int ROWB = score_rowb(CP);
  constexpr int kScoreWaves = score_waves(NC);
  __shared__ __attribute__((aligned(16))) char lds[kScoreWaves][kTile * ROWB];
  const int li = (int)blockIdx.x / BH, r = (int)blockIdx.x - li * BH;
  const kvc_seq_t q = load_seq(T.s[li] + r / H);
  if (!(q.n_select > 0 && q.n_select < q.zone_len)) return;
  // (never past the planned norm row, whatever a rewritten record says)
  const int ntile = min((q.zone_len + kTile - 1) / kTile, (int)tmax_stride);
  const int t0 = (int)blockIdx.y * kRaggedTiles;
  if (t0 >= ntile) return;
  const int t1 = min(ntile, t0 + kRaggedTiles);
  const kvc_layer_t y = seq_layer(T.l + li, q);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int tt = t0 + wid; tt < t1; tt += kScoreWaves)
    score_paged_tile<DT, NC>(&y, T.p + li, r, tt, H, lds[wid], norms, norm_stride, tmax,
                             tmax_stride, status);
}

// score_ragged_kernel for scaled fp8 layers (score_paged_tile<SC>), under a name of its own.  Its
// prologue is a COPY of score_ragged_kernel's, deliberately: as one __device__ body over the SC
// flag, called from two thin kernels, 47 of the existing score_paged_kernel / score_ragged_kernel
// instances compile to other code than before (tools/isa_diff.py: an instruction and an SGPR here
// and there), and the existing instances are to stay what they were.  A fix to one prologue is a
// fix to both.
template <int DT, int NC>
__global__ void __launch_bounds__(score_waves(NC) * 64)
    score_ragged_scaled_kernel(const RaggedChunk T, const ScalesChunk Z, int H, int BH,
                               char* __restrict__ norms, int64_t norm_stride,
                               uint32_t* __restrict__ tmax, int64_t tmax_stride,
                               uint32_t* status) {
  constexpr int CP = score_cp(NC);
  constexpr int ROWB = score_rowb(CP);
  constexpr int kScoreWaves = score_waves(NC);
  __shared__ __attribute__((aligned(16))) char lds[kScoreWaves][kTile * ROWB];
  const int li = (int)blockIdx.x / BH, r = (int)blockIdx.x - li * BH;
  const kvc_seq_t q = load_seq(T.s[li] + r / H);
  if (!(q.n_select > 0 && q.n_select < q.zone_len)) return;
  // (never past the planned norm row, whatever a rewritten record says)
  const int ntile = min((q.zone_len + kTile - 1) / kTile, (int)tmax_stride);
  const int t0 = (int)blockIdx.y * kRaggedTiles;
  if (t0 >= ntile) return;
  const int t1 = min(ntile, t0 + kRaggedTiles);
  const kvc_layer_t y = seq_layer(T.l + li, q);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int tt = t0 + wid; tt < t1; tt += kScoreWaves)
    score_paged_tile<DT, NC, true>(&y, T.p + li, r, tt, H, lds[wid], norms, norm_stride, tmax,
                                   tmax_stride, status, Z.s + li);
}

// SELECT: the workgroups of select_kernel / select_global_kernel / select_long_kernel, one per
// (layer, b, h) row of the envelope's row numbering, with zone_len, n_select, score_mode and
// pool_kernel of the row's record.  n_cap is the launch's capacity (the envelope's zone): a
// record beyond it sets KVC_DEV_SELECT_BOUNDS like any row beyond its kernel's capacity.
template <int KC, int NT, bool STABLE = false>
__global__ void __launch_bounds__(NT, sel_waves_per_eu(KC, NT))
    select_ragged_kernel(const RaggedChunk T, int H, int BH, int dt, int order, int algo,
                         const char* __restrict__ norms, int64_t norm_stride,
                         int32_t* __restrict__ out_idx, int64_t idx_stride, int wave_seg,
                         int n_cap, int cap, uint32_t* status,
                         const uint32_t* __restrict__ tmax) {
  typedef typename DTypeTraits<KC>::key_t KeyT;
  constexpr int ESZ = DTypeTraits<KC>::esz;
  constexpr int MAXN = NT == kSelThreads ? kZoneMax : NT * 16;
  __shared__ SelScalars<KeyT> sc;
  const int li = (int)blockIdx.x / BH, r = (int)blockIdx.x - li * BH;
  const kvc_seq_t q = load_seq(T.s[li] + r / H);
  const kvc_layer_t y = seq_layer(T.l + li, q);
  const int row = y.row0 + r;  // global workspace row
  const uint32_t* trow = tmax ? tmax + (int64_t)row * (norm_stride / kTile) : nullptr;
  if constexpr (NT == kSelThreads) {
    __shared__ __attribute__((aligned(16))) char smem[kSelBytesBig<KeyT>];
    select_body<KC, false, MAXN, NT, false, STABLE>(
        &y, dt, order, algo, norms + (int64_t)row * norm_stride * ESZ,
        out_idx + (int64_t)row * idx_stride, nullptr, smem, kZoneMax, kSelCapBig<KeyT>, sc,
        wave_seg, nullptr, status, trow);
  } else {
    extern __shared__ __attribute__((aligned(16))) char dsmem[];
    select_body<KC, false, MAXN, NT, false, STABLE>(
        &y, dt, order, algo, norms + (int64_t)row * norm_stride * ESZ,
        out_idx + (int64_t)row * idx_stride, nullptr, dsmem, n_cap, cap, sc, wave_seg, nullptr,
        status, trow);
  }
}

template <int KC, bool STABLE = false>
__global__ void __launch_bounds__(kSelThreads)
    select_global_ragged_kernel(const RaggedChunk T, int H, int BH, int dt, int order, int algo,
                                const char* __restrict__ norms, int64_t norm_stride,
                                int32_t* __restrict__ out_idx, int64_t idx_stride, int wave_seg,
                                char* __restrict__ scratch, int64_t scratch_row_bytes, int n_cap,
                                uint32_t* status) {
  typedef typename DTypeTraits<KC>::key_t KeyT;
  constexpr int ESZ = DTypeTraits<KC>::esz;
  __shared__ SelScalars<KeyT> sc;
  const int li = (int)blockIdx.x / BH, r = (int)blockIdx.x - li * BH;
  const kvc_seq_t q = load_seq(T.s[li] + r / H);
  const kvc_layer_t y = seq_layer(T.l + li, q);
  const int row = y.row0 + r;
  select_body<KC, false, kZoneMaxGlobal, kSelThreads, false, STABLE>(
      &y, dt, order, algo, norms + (int64_t)row * norm_stride * ESZ,
      out_idx + (int64_t)row * idx_stride, nullptr, scratch + (int64_t)row * scratch_row_bytes,
      n_cap, n_cap / 2 + 1, sc, wave_seg, nullptr, status);
}

template <int KC>
__global__ void __launch_bounds__(kSelThreads)
    select_long_ragged_kernel(const RaggedChunk T, int H, int BH, int dt, int order, int algo,
                              const char* __restrict__ norms, int64_t norm_stride,
                              int32_t* __restrict__ out_idx, int64_t idx_stride,
                              char* __restrict__ scratch, int64_t scratch_row_bytes, int n_cap,
                              uint32_t* status) {
  __shared__ SelScalars<typename DTypeTraits<KC>::key_t> ssc;
  __shared__ LongScalars sc;
  const int li = (int)blockIdx.x / BH, r = (int)blockIdx.x - li * BH;
  const kvc_seq_t q = load_seq(T.s[li] + r / H);
  const kvc_layer_t y = seq_layer(T.l + li, q);
  select_long_body<KC>(&y, y.row0 + r, dt, order, algo, norms, norm_stride, out_idx, idx_stride,
                       scratch, scratch_row_bytes, n_cap, status, ssc, sc);
}

// GATHER: gather_passes (kvc_gather_dest.h) in place, PagedRows as source and destination, one
// workgroup per (layer, b, h) row; n_out, sink_len, n_select, the zone and tail_start are the
// record's.  The ordering proof is gather_passes' own and the memory argument kvc_paged.h's: both
// speak about ONE (b, h) sequence's rows and its table row, and neither uses that the sequences
// of a layer are equally long.  A no-op record (n_out == sink_len) moves nothing.
template <int DT, int NC>
__global__ void __launch_bounds__(kGatherThreads)
    gather_ragged_kernel(const RaggedChunk T, int H, int BH, const int32_t* __restrict__ gidx,
                         int64_t idx_stride, uint32_t* status) {
  const int li = (int)blockIdx.x / BH, r = (int)blockIdx.x - li * BH;
  const int b = r / H, h = r - (r / H) * H;
  const kvc_seq_t q = load_seq(T.s[li] + b);
  if (q.n_out <= q.sink_len) return;
  const kvc_layer_t y = seq_layer(T.l + li, q);
  constexpr int ESZ = DTypeTraits<DT>::esz;
  const PagedRows rows(ESZ, &y, T.p + li, b, h);
  gather_passes<DT, NC>(&y, r, H, true, rows, rows, gidx, idx_stride, 0, status);
}

// gather_ragged_kernel for scaled fp8 layers: the rows' scale words move with them
// (gather_passes<SC> over ScaledPagedRows), under a name of its own.
template <int DT, int NC>
__global__ void __launch_bounds__(kGatherThreads, 8)
    gather_ragged_scaled_kernel(const RaggedChunk T, const ScalesChunk Z, int H, int BH,
                                const int32_t* __restrict__ gidx, int64_t idx_stride,
                                uint32_t* status) {
  const int li = (int)blockIdx.x / BH, r = (int)blockIdx.x - li * BH;
  const int b = r / H, h = r - (r / H) * H;
  const kvc_seq_t q = load_seq(T.s[li] + b);
  if (q.n_out <= q.sink_len) return;
  const kvc_layer_t y = seq_layer(T.l + li, q);
  constexpr int ESZ = DTypeTraits<DT>::esz;
  const ScaledPagedRows rows(ESZ, &y, T.p + li, Z.s + li, b, h);
  gather_passes<DT, NC, true>(&y, r, H, true, rows, rows, gidx, idx_stride, 0, status);
}

}  // namespace kvc
