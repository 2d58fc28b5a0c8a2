// kvc_paged.h -- paged K/V sources (kvc_launch_paged): SCORE and GATHER of layers whose rows live
// in a page pool addressed through a per-sequence block table (include/kvc.h, "Paged caches").
// GATHER is the pass schedule of kvc_gather_dest.h over the block-table policy below.  SELECT
// reads the workspace only and runs the kernels of kvc_select.h unchanged.
#pragma once

#include "kvc_gather_dest.h"
#include "kvc_score.h"

namespace kvc {

// Paged launches run in chunks of kPagedLayers: a chunk's layers, page tables and destinations
// travel by value in ONE struct of 7.5 KiB -- below the 12.2 KiB (LayerChunk + DestChunk) that
// kvc_launch_dest's copy kernel is known to launch with.  (Three 64-entry tables would be 15 KiB
// of kernel arguments; no host-to-device table copy instead: see kArgLayers.)
constexpr int kPagedLayers = 32;
struct PagesChunk {
  kvc_layer_t l[kPagedLayers];
  kvc_pages_t p[kPagedLayers];
  kvc_dest_t d[kPagedLayers];  // dense outputs: their strides (a contiguous k_out's as well)
};

// Address arithmetic of one (layer, b, h) row of a paged K or V: logical row s lives at
//   pool + (table[s >> lg] * page_stride + h * stride[1] + (s & (P - 1)) * stride[2]) * esz.
// A page id outside [0, num_pages) is clamped for loads (KVC_DEV_INDEX_RANGE); `ok` says whether
// it was in range (an in-place store through a bad id is dropped).
struct PageRow {
  const int32_t* tab;  // block_table + b * table_stride
  int lg, mask, np;
  __device__ __forceinline__ PageRow(const kvc_pages_t* pg, int b)
      : tab(pg->block_table + (int64_t)b * pg->table_stride),
        lg(31 - __builtin_clz((unsigned)pg->page_size)),
        mask(pg->page_size - 1),
        np(pg->num_pages) {}
  // page id of logical row s, clamped; *ok = it was in range
  __device__ __forceinline__ int page(int s, bool* ok) const {
    const int id = tab[s >> lg];
    *ok = id >= 0 && id < np;
    return min(max(id, 0), np - 1);
  }
};

// ---------------------------------------------------------------------------------------------
// SCORE of paged keys: score_tile (kvc_score.h) with the row address of every staged token taken
// through the block table.  Same tile structure (one wave = 64 consecutive zone tokens of one
// (layer, b, h) row), LDS slab, FMA order, non-temporal loads, norm stores and snapkv tile
// maxima; a tile may start anywhere in a page and span many pages or a fraction of one.  Each lane
// stages CP (token, 16-B chunk) units per phase, of CP / gcd distinct tokens; the page id of a
// unit's token is looked up ONCE, before the phases, and kept as the unit's row pointer.
// The tile is a COPY of score_tile from `float acc[8]` on, deliberately: as one body over a
// row-source policy (tried with valid/ptr and with load methods, by value, by reference and over a
// local pointer array) score_paged_kernel<*, 20> takes 150 VGPRs instead of 130-132 and the
// CP = 10 instances 36-77 more instructions, and a reordered score_kernel is all the dense side
// gains.  A fix to one tile is a fix to both.
// ---------------------------------------------------------------------------------------------
//
// SC (per-token-scaled fp8 caches, include/kvc.h): the lane that owns token `lane` of the tile
// loads that token's K scale -- through one more lookup of the same clamped page id, issued before
// the phases so that the load is in flight behind the key loads -- or the layer's one uniform
// float, and the stored norm is bf16(r * |s|): ONE fp32 multiply between the sqrt and the bf16
// rounding.  The tile maximum is taken from those bits.  Every SC line is behind `if constexpr`:
// the unscaled instances compile from the code they had.
template <int DT, int NC, bool SC = false>
__device__ __forceinline__ void score_paged_tile(const kvc_layer_t* ly, const kvc_pages_t* pg,
                                                 int row, int tt, int H, char* wl, char* norms,
                                                 int64_t norm_stride, uint32_t* tmax,
                                                 int64_t tmax_stride, uint32_t* status,
                                                 const kvc_scales_t* sc = nullptr) {
  constexpr int ESZ = DTypeTraits<DT>::esz;
  constexpr int SDT = score_dt(DT);  // the norm region's dtype (bf16 for fp8 keys)
  constexpr int CP = score_cp(NC);
  constexpr int NPH = NC / CP;
  constexpr int ROWB = score_rowb(CP);
  const int lane = threadIdx.x & 63;
  const int zlen = ly->zone_len;
  const int b = row / H, h = row - (row / H) * H;
  const int tok0 = tt * kTile;
  const int ntok = min(kTile, zlen - tok0);
  const int64_t sbytes = ly->k_stride[2] * ESZ, pbytes = pg->k_page_stride * ESZ;
  const char* base = static_cast<const char*>(ly->k) + (int64_t)h * ly->k_stride[1] * ESZ;
  const PageRow pr(pg, b);
  const int s0 = ly->zone_start + tok0;
  const char* rowp[CP];  // row pointer of the token of unit `it` (nullptr past the zone)
  bool bad = false;
#pragma unroll
  for (int it = 0; it < CP; ++it) {
    const int q = it * 64 + lane;
    const int tok = q / CP;
    rowp[it] = nullptr;
    if (tok < ntok) {
      const int s = s0 + tok;
      bool ok;
      const int id = pr.page(s, &ok);
      bad |= !ok;
      rowp[it] = base + (int64_t)id * pbytes + (int64_t)(s & pr.mask) * sbytes;
    }
  }
  float kscale = 1.0f;  // SC: this lane's token's scale (1: KVC_SCALE_K_NONE, lanes past the zone)
  if constexpr (SC) {
    if (sc->flags & KVC_SCALE_K_UNIFORM) {
      kscale = *sc->k_scale;
    } else if (!(sc->flags & KVC_SCALE_K_NONE) && lane < ntok) {
      const int s = s0 + lane;
      bool ok;
      const int64_t id = pr.page(s, &ok);
      bad |= !ok;
      // (a plain load: in a pool stored [N, P, H] the heads' scales of a token share a cache
      // line, which the waves of the other heads come for)
      kscale = sc->k_scale[id * sc->k_page_stride + (int64_t)h * sc->k_stride[0] +
                           (int64_t)(s & pr.mask) * sc->k_stride[1]];
    }
  }
  if (bad && status) atomicOr(status, (uint32_t)KVC_DEV_INDEX_RANGE);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ph = 0; ph < NPH; ++ph) {
    uint4 v[CP];
#pragma unroll
    for (int it = 0; it < CP; ++it) {
      const int q = it * 64 + lane;
      const int c = q - (q / CP) * CP;
      if (rowp[it]) {
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 w = __builtin_nontemporal_load(
            reinterpret_cast<const u32x4*>(rowp[it] + (ph * CP + c) * 16));
        v[it] = make_uint4(w.x, w.y, w.z, w.w);
      } else {
        v[it] = make_uint4(0, 0, 0, 0);
      }
    }
#pragma unroll
    for (int it = 0; it < CP; ++it) {
      const int q = it * 64 + lane;
      const int tok = q / CP, c = q - (q / CP) * CP;
      *reinterpret_cast<uint4*>(wl + tok * ROWB + c * 16) = v[it];
    }
    wave_sync();
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      const uint4 x = *reinterpret_cast<const uint4*>(wl + lane * ROWB + c * 16);
      accum_chunk<DT, NC>(acc, x, ph * CP + c);
    }
    wave_sync();
  }
  uint32_t bits = 0;  // the stored norm's bits (0 for lanes past the zone)
  if (lane < ntok) {
    float s = acc[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) s = s + acc[j];
    float r = __builtin_sqrtf(s);
    if constexpr (SC) r = r * __builtin_fabsf(kscale);
    char* nrow = norms + (int64_t)(ly->row0 + row) * norm_stride * DTypeTraits<SDT>::esz;
    if constexpr (DT != KVC_F32) {
      bits = bits16_dt<SDT>(r);
      __builtin_nontemporal_store((uint16_t)bits, reinterpret_cast<uint16_t*>(nrow) + tok0 + lane);
    } else {
      bits = f32_to_bits(r);
      __builtin_nontemporal_store(r, reinterpret_cast<float*>(nrow) + tok0 + lane);
    }
  }
  if (ly->score_mode == KVC_SCORE_SNAPKV && tmax) {  // wave-uniform
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bits = max(bits, (uint32_t)__shfl_xor((int)bits, o, 64));
    if (lane == 0) tmax[(int64_t)(ly->row0 + row) * tmax_stride + tt] = bits;
  }
}

template <int DT, int NC>
__global__ void __launch_bounds__(score_waves(NC) * 64)
    score_paged_kernel(const PagesChunk T, int nl, int H, int64_t tile_base, int64_t chunk_tiles,
                       char* __restrict__ norms, int64_t norm_stride, uint32_t* __restrict__ tmax,
                       int64_t tmax_stride, uint32_t* status) {
  constexpr int CP = score_cp(NC);
  constexpr int ROWB = score_rowb(CP);
  constexpr int kScoreWaves = score_waves(NC);
  __shared__ __attribute__((aligned(16))) char lds[kScoreWaves][kTile * ROWB];
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t stride = (int64_t)gridDim.x * kScoreWaves;
  for (int64_t gl = (int64_t)blockIdx.x * kScoreWaves + wid; gl < chunk_tiles; gl += stride) {
    const TileAt at = locate_tile(T.l, nl, tile_base + gl);
    score_paged_tile<DT, NC>(T.l + at.layer, T.p + at.layer, at.row, at.tile, H, lds[wid], norms,
                             norm_stride, tmax, tmax_stride, status);
  }
}

// The scale descriptions of a chunk's layers travel by value beside its PagesChunk / RaggedChunk
// (2.25 KiB: 9.75 KiB of kernel arguments with a PagesChunk, below the 12.2 KiB known to launch).
struct ScalesChunk {
  kvc_scales_t s[kPagedLayers];
};

// score_paged_kernel for scaled fp8 layers: the same grid-stride loop over score_paged_tile<SC>.
// A kernel of its own name, so that score_paged_kernel's instances stay what they were; the loop
// is a copy for the same reason (kvc_ragged.h, score_ragged_scaled_kernel: a shared body changed
// the existing instances' code).
template <int DT, int NC>
__global__ void __launch_bounds__(score_waves(NC) * 64)
    score_paged_scaled_kernel(const PagesChunk T, const ScalesChunk Z, int nl, int H,
                              int64_t tile_base, int64_t chunk_tiles, char* __restrict__ norms,
                              int64_t norm_stride, uint32_t* __restrict__ tmax,
                              int64_t tmax_stride, uint32_t* status) {
  constexpr int CP = score_cp(NC);
  constexpr int ROWB = score_rowb(CP);
  constexpr int kScoreWaves = score_waves(NC);
  __shared__ __attribute__((aligned(16))) char lds[kScoreWaves][kTile * ROWB];
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t stride = (int64_t)gridDim.x * kScoreWaves;
  for (int64_t gl = (int64_t)blockIdx.x * kScoreWaves + wid; gl < chunk_tiles; gl += stride) {
    const TileAt at = locate_tile(T.l, nl, tile_base + gl);
    score_paged_tile<DT, NC, true>(T.l + at.layer, T.p + at.layer, at.row, at.tile, H, lds[wid],
                                   norms, norm_stride, tmax, tmax_stride, status, Z.s + at.layer);
  }
}

// ---------------------------------------------------------------------------------------------
// GATHER of paged sources: gather_passes (kvc_gather_dest.h) reading through the block table, into
//   * a dense destination (kvc_pages_t.in_place == 0): b * os0 + h * os1 + t * os2 of T.d -- the
//     layer's kvc_dest_t, or the strides of a contiguous k_out / v_out;
//   * the pool itself (in_place == 1): output row t goes to the slot of LOGICAL row t through the
//     same table, on the in-place schedule.
//
// Why that is still a correct memmove: what gather_passes' proof needs from memory is that
// DIFFERENT logical rows of one (b, h) sequence are different bytes (kvc_plan_paged applies the
// same row-map rule).  With a block table, logical row s is (page table[s >> lg], slot
// s & (P-1)): distinct page ids within a table row (the caller's promise) and non-zero,
// non-overlapping strides make s -> address injective, whatever order the pages have in the pool
// -- a shuffled table permutes addresses, not rows.  Different (b, h) rows, K and V, and layers
// share no written page (the promise), so workgroups do not meet.  The table is only read.  Sink
// rows have src == dst and are not touched, so pages holding only sink rows may be shared between
// sequences.
// An in-place store through a page id outside [0, num_pages) is DROPPED (loads are clamped).
//
// Ragged batches (kvc_ragged.h) run the same schedule with every (b, h) row's n_out, sink, zone
// and tail taken from its own record.  Nothing above changes: the argument is about the logical
// rows of ONE sequence behind ONE table row, the row-map rule is applied to every record, and no
// step uses that the sequences of a layer have a common length -- gather_passes needs nothing
// from memory beyond what this paragraph already asks.
// ---------------------------------------------------------------------------------------------
// Rows of one (b, h) sequence of a paged K and V.
struct PagedRows {
  PageRow pr;
  char* kb;
  char* vb;
  int64_t kss, vss, kps, vps;
  // bad page ids and indices fold into one flag: one atomicOr per thread
  static constexpr bool kFoldStatus = true;
  __device__ __forceinline__ PagedRows(int esz, const kvc_layer_t* ly, const kvc_pages_t* pg,
                                       int b, int h)
      : pr(pg, b),
        kb((char*)ly->k + (int64_t)h * ly->k_stride[1] * esz),
        vb((char*)ly->v + (int64_t)h * ly->v_stride[1] * esz),
        kss(ly->k_stride[2] * esz),
        vss(ly->v_stride[2] * esz),
        kps(pg->k_page_stride * esz),
        vps(pg->v_page_stride * esz) {}
  // addresses of logical row s through the clamped page id; false: the id was out of range
  __device__ __forceinline__ bool locate(int s, char** k, char** v) const {
    bool ok;
    const int64_t id = pr.page(s, &ok);
    const int slot = s & pr.mask;
    *k = kb + id * kps + slot * kss;
    *v = vb + id * vps + slot * vss;
    return ok;
  }
};

// PagedRows of a scaled layer: page_of() / scales_at() give the addresses of a row's K and V
// scale words through the page id that locate() gives its K and V bytes through -- nullptr for a
// side whose scale is uniform or absent (nothing of it moves).
struct ScaledPagedRows : PagedRows {
  uint32_t* ksb;
  uint32_t* vsb;
  int64_t ksp, kss1, vsp, vss1;
  __device__ __forceinline__ ScaledPagedRows(int esz, const kvc_layer_t* ly, const kvc_pages_t* pg,
                                             const kvc_scales_t* sc, int b, int h)
      : PagedRows(esz, ly, pg, b, h),
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
  // the clamped page id of logical row s, as locate() looks it up (*ok: it was in range)
  __device__ __forceinline__ int page_of(int s, bool* ok = nullptr) const {
    bool in_range;
    const int id = pr.page(s, &in_range);
    if (ok) *ok = in_range;
    return id;
  }
  // addresses of the scale words of logical row s, which lives in page `id`
  __device__ __forceinline__ void scales_at(int64_t id, int s, uint32_t** sk,
                                            uint32_t** sv) const {
    const int slot = s & pr.mask;
    *sk = ksb ? ksb + id * ksp + slot * kss1 : nullptr;
    *sv = vsb ? vsb + id * vsp + slot * vss1 : nullptr;
  }
};

// gather_paged_kernel for scaled fp8 layers (always in place: kvc_plan_scaled): gather_passes<SC>
// over ScaledPagedRows.  A kernel of its own name, as score_paged_scaled_kernel.
template <int DT, int NC>
__global__ void __launch_bounds__(kGatherThreads, 8)
    gather_paged_scaled_kernel(const PagesChunk T, const ScalesChunk Z, int H, int BH,
                               const int32_t* __restrict__ gidx, int64_t idx_stride, int shared,
                               uint32_t* status) {
  const int li = (int)blockIdx.x / BH;
  const kvc_layer_t* ly = T.l + li;
  const int r = (int)blockIdx.x - li * BH;
  const int b = r / H, h = r - (r / H) * H;
  constexpr int ESZ = DTypeTraits<DT>::esz;
  const ScaledPagedRows rows(ESZ, ly, T.p + li, Z.s + li, b, h);
  gather_passes<DT, NC, true>(ly, r, H, true, rows, rows, gidx, idx_stride, shared, status);
}

template <int DT, int NC>
__global__ void __launch_bounds__(kGatherThreads)
    gather_paged_kernel(const PagesChunk T, int H, int BH, const int32_t* __restrict__ gidx,
                        int64_t idx_stride, int shared, uint32_t* status) {
  const int li = (int)blockIdx.x / BH;
  const kvc_layer_t* ly = T.l + li;
  const kvc_pages_t* pg = T.p + li;
  const kvc_dest_t* de = T.d + li;
  const int r = (int)blockIdx.x - li * BH;
  const int b = r / H, h = r - (r / H) * H;
  const bool inplace = pg->in_place != 0;
  constexpr int ESZ = DTypeTraits<DT>::esz;
  const PagedRows src(ESZ, ly, pg, b, h);
  const DenseRows dense(ESZ, ly->k_out, ly->v_out, de->k_stride, de->v_stride, b, h);
  const EitherRows<PagedRows, DenseRows> dst = {inplace, src, dense};
  gather_passes<DT, NC>(ly, r, H, inplace, src, dst, gidx, idx_stride, shared, status);
}

}  // namespace kvc
