// kvc_repage.h -- paged DESTINATIONS (kvc_launch_repage): GATHER of paged layers whose compressed
// sequence is written through a second block table into pages the caller chose (include/kvc.h,
// "Paged destinations").  SCORE and SELECT of such a launch are the kernels of kvc_paged.h /
// kvc_ragged.h / kvc_select.h, called as they are; only the copy is new, and it is gather_passes
// (kvc_gather_dest.h) out of place: PagedRows as the source, the policy below as the destination.
#pragma once

#include "kvc_ragged.h"

namespace kvc {

// Rows of one (b, h) sequence of a paged DESTINATION: output row t lives at
//   k_out + (dtable[t >> lg] * page_stride + h * stride[0] + (t & (Pd - 1)) * stride[1]) * esz
// with the destination's own table row, page size and pool size.  A page id outside
// [0, num_pages) makes locate() return false: gather_passes drops the row's stores and reports
// KVC_DEV_INDEX_RANGE (the clamped address it still gets is never dereferenced).
struct DestPagedRows {
  const int32_t* tab;  // dest block_table + b * table_stride
  int lg, mask, np;
  char* kb;
  char* vb;
  int64_t kss, vss, kps, vps;
  __device__ __forceinline__ DestPagedRows(int esz, const kvc_layer_t* ly,
                                           const kvc_page_dest_t* pd, int b, int h)
      : tab(pd->block_table + (int64_t)b * pd->table_stride),
        lg(31 - __builtin_clz((unsigned)pd->page_size)),
        mask(pd->page_size - 1),
        np(pd->num_pages),
        kb((char*)ly->k_out + (int64_t)h * pd->k_stride[0] * esz),
        vb((char*)ly->v_out + (int64_t)h * pd->v_stride[0] * esz),
        kss(pd->k_stride[1] * esz),
        vss(pd->v_stride[1] * esz),
        kps(pd->k_page_stride * esz),
        vps(pd->v_page_stride * esz) {}
  // clamped page id of output row t; *ok = it was in range
  __device__ __forceinline__ int page_of(int t, bool* ok) const {
    const int id = tab[t >> lg];
    *ok = id >= 0 && id < np;
    return min(max(id, 0), np - 1);
  }
  __device__ __forceinline__ bool locate(int t, char** k, char** v) const {
    bool ok;
    const int64_t id = page_of(t, &ok);
    const int slot = t & mask;
    *k = kb + id * kps + slot * kss;
    *v = vb + id * vps + slot * vss;
    return ok;
  }
};

// DestPagedRows of a scale-carrying layer: scales_at() gives the slots of output row t's K and V
// scale words in the DESTINATION scale pools (kvc_launch_repage's dscales) -- nullptr for a side
// whose scale is uniform or absent, as ScaledPagedRows does for the source.
struct DestScaledPagedRows : DestPagedRows {
  uint32_t* ksb;
  uint32_t* vsb;
  int64_t ksp, kss1, vsp, vss1;
  __device__ __forceinline__ DestScaledPagedRows(int esz, const kvc_layer_t* ly,
                                                 const kvc_page_dest_t* pd, const kvc_scales_t* sc,
                                                 int b, int h)
      : DestPagedRows(esz, ly, pd, b, h),
        ksb((sc->flags & (KVC_SCALE_K_UNIFORM | KVC_SCALE_K_NONE))
                ? nullptr
                : reinterpret_cast<uint32_t*>(sc->k_scale) + (int64_t)h * sc->k_stride[0]),
        vsb((sc->flags & (KVC_SCALE_V_UNIFORM | KVC_SCALE_V_NONE))
                ? nullptr
                : reinterpret_cast<uint32_t*>(sc->v_scale) + (int64_t)h * sc->v_stride[0]),
        ksp(sc->k_page_stride),
        kss1(sc->k_stride[1]),
        vsp(sc->v_page_stride),
        vss1(sc->v_stride[1]) {}
  __device__ __forceinline__ void scales_at(int64_t id, int t, uint32_t** sk,
                                            uint32_t** sv) const {
    const int slot = t & mask;
    *sk = ksb ? ksb + id * ksp + slot * kss1 : nullptr;
    *sv = vsb ? vsb + id * vsp + slot * vss1 : nullptr;
  }
};

// The by-value tables of a repage chunk.  Sizes are part of the design: the project launches
// kernels with up to 12 288 B of arguments (kvc_paged.h, kPagedLayers), so the chunks that also
// carry two scale descriptions per layer hold kRepageScLayers layers instead of kPagedLayers.
struct RepageChunk {
  kvc_layer_t l[kPagedLayers];
  kvc_pages_t p[kPagedLayers];
  kvc_page_dest_t d[kPagedLayers];
};
static_assert(sizeof(RepageChunk) == 8192, "32 layers x (136 + 48 + 72) B");
struct RepageRaggedChunk {
  kvc_layer_t l[kPagedLayers];
  kvc_pages_t p[kPagedLayers];
  kvc_page_dest_t d[kPagedLayers];
  const kvc_seq_t* s[kPagedLayers];  // device: `batch` records of the layer
};
static_assert(sizeof(RepageRaggedChunk) == 8448, "RepageChunk + 32 record pointers");

constexpr int kRepageScLayers = 16;
struct RepageScChunk {
  kvc_layer_t l[kRepageScLayers];
  kvc_pages_t p[kRepageScLayers];
  kvc_page_dest_t d[kRepageScLayers];
  kvc_scales_t z[kRepageScLayers];   // source scale pools
  kvc_scales_t dz[kRepageScLayers];  // destination scale pools
};
static_assert(sizeof(RepageScChunk) == 6400, "16 layers x (136 + 48 + 72 + 72 + 72) B");
struct RepageRaggedScChunk {
  kvc_layer_t l[kRepageScLayers];
  kvc_pages_t p[kRepageScLayers];
  kvc_page_dest_t d[kRepageScLayers];
  kvc_scales_t z[kRepageScLayers];
  kvc_scales_t dz[kRepageScLayers];
  const kvc_seq_t* s[kRepageScLayers];
};
static_assert(sizeof(RepageRaggedScChunk) == 6528, "RepageScChunk + 16 record pointers");
static_assert(sizeof(RepageRaggedChunk) <= 12288 && sizeof(RepageRaggedScChunk) <= 12288 &&
                  32 * (136 + 48 + 72 + 72 + 72) > 12288,
              "kernel arguments stay at or below the 12 KiB known to launch; 32 scale-carrying "
              "layers would not");

// Single-length layers.  grid = (rows of the chunk, passes of the longest output): block (row, by)
// copies the one pass of dest_pass_rows(NC) output rows from by * dest_pass_rows(NC) on --
// gather_passes' out-of-place schedule, which has no ordering constraint because the caller
// promises that no destination page is a source page.  Sink rows are copied like every other row.
template <int DT, int NC>
__global__ void __launch_bounds__(kGatherThreads)
    gather_repage_kernel(const RepageChunk T, int H, int BH, const int32_t* __restrict__ gidx,
                         int64_t idx_stride, int shared, uint32_t* status) {
  const int li = (int)blockIdx.x / BH;
  const kvc_layer_t* ly = T.l + li;
  const int r = (int)blockIdx.x - li * BH;
  const int b = r / H, h = r - (r / H) * H;
  constexpr int ESZ = DTypeTraits<DT>::esz;
  const PagedRows src(ESZ, ly, T.p + li, b, h);
  const DestPagedRows dst(ESZ, ly, T.d + li, b, h);
  gather_passes<DT, NC>(ly, r, H, false, src, dst, gidx, idx_stride, shared, status);
}

// Ragged layers: the same grid, sized by the envelope's n_out.  Every block loads its row's record
// first (one uniform 48-byte load) and returns, before any other load from device memory, when its
// pass starts at or beyond the record's n_out -- so a 600-row sequence beside a 16 384-row one
// costs its idle blocks one load each.  The in-place ragged copy is one workgroup per row because
// its passes are ordered; out of place they are independent, so they run side by side.  A record's
// n_out is capped at the planned envelope's (whatever a rewritten record says: the destination
// table is only that wide).  n_out == 0 writes nothing; sink_len = n_out = seq_len copies the
// sequence.
template <int DT, int NC>
__global__ void __launch_bounds__(kGatherThreads)
    gather_repage_ragged_kernel(const RepageRaggedChunk T, int H, int BH,
                                const int32_t* __restrict__ gidx, int64_t idx_stride,
                                uint32_t* status) {
  const int li = (int)blockIdx.x / BH, r = (int)blockIdx.x - li * BH;
  const int b = r / H, h = r - (r / H) * H;
  const kvc_seq_t q = load_seq(T.s[li] + b);
  const int n_out = min(q.n_out, T.l[li].n_out);
  if ((int)blockIdx.y * dest_pass_rows(NC) >= n_out) return;
  kvc_layer_t y = seq_layer(T.l + li, q);
  y.n_out = n_out;
  constexpr int ESZ = DTypeTraits<DT>::esz;
  const PagedRows src(ESZ, &y, T.p + li, b, h);
  const DestPagedRows dst(ESZ, &y, T.d + li, b, h);
  gather_passes<DT, NC>(&y, r, H, false, src, dst, gidx, idx_stride, 0, status);
}

// The scale-carrying twins (fp8 rows only): gather_passes<SC> over ScaledPagedRows and
// DestScaledPagedRows -- thread j of a block carries the two scale words of pass row j beside the
// units' loads (the SC comment in kvc_gather_dest.h) and stores them into the destination's scale
// slots.  Kernels of their own names, bodies copied, so that the kernels above and every existing
// instance stay what they are.
template <int DT, int NC>
__global__ void __launch_bounds__(kGatherThreads, 8)
    gather_repage_sc_kernel(const RepageScChunk T, int H, int BH,
                            const int32_t* __restrict__ gidx, int64_t idx_stride, int shared,
                            uint32_t* status) {
  const int li = (int)blockIdx.x / BH;
  const kvc_layer_t* ly = T.l + li;
  const int r = (int)blockIdx.x - li * BH;
  const int b = r / H, h = r - (r / H) * H;
  constexpr int ESZ = DTypeTraits<DT>::esz;
  const ScaledPagedRows src(ESZ, ly, T.p + li, T.z + li, b, h);
  const DestScaledPagedRows dst(ESZ, ly, T.d + li, T.dz + li, b, h);
  gather_passes<DT, NC, true>(ly, r, H, false, src, dst, gidx, idx_stride, shared, status);
}

template <int DT, int NC>
__global__ void __launch_bounds__(kGatherThreads, 8)
    gather_repage_ragged_sc_kernel(const RepageRaggedScChunk T, int H, int BH,
                                   const int32_t* __restrict__ gidx, int64_t idx_stride,
                                   uint32_t* status) {
  const int li = (int)blockIdx.x / BH, r = (int)blockIdx.x - li * BH;
  const int b = r / H, h = r - (r / H) * H;
  const kvc_seq_t q = load_seq(T.s[li] + b);
  const int n_out = min(q.n_out, T.l[li].n_out);
  if ((int)blockIdx.y * dest_pass_rows(NC) >= n_out) return;
  kvc_layer_t y = seq_layer(T.l + li, q);
  y.n_out = n_out;
  constexpr int ESZ = DTypeTraits<DT>::esz;
  const ScaledPagedRows src(ESZ, &y, T.p + li, T.z + li, b, h);
  const DestScaledPagedRows dst(ESZ, &y, T.d + li, T.dz + li, b, h);
  gather_passes<DT, NC, true>(&y, r, H, false, src, dst, gidx, idx_stride, 0, status);
}

}  // namespace kvc
