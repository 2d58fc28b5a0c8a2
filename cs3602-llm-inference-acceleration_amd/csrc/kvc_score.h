// kvc_score.h -- SCORE: the HBM-streaming key L2 norms (score_kernel).
#pragma once

#include "kvc_device_util.h"

namespace kvc {

// ---------------------------------------------------------------------------------------------
// SCORE
// ---------------------------------------------------------------------------------------------
template <int DT, int NC>
__device__ __forceinline__ void accum_chunk(float (&acc)[8], const uint4 x, int gchunk) {
  if constexpr (is_fp8(DT)) {
    // chunk c holds the 16 elements 16c..16c+15: element e feeds accumulator e % 8, so dword q
    // (elements 4q..4q+3) feeds accumulators 4*(q&1)..+3, dwords 0,1 before dwords 2,3 -- ascending
    // element order per accumulator, torch.norm's order on the bf16 upcast.  The decode is gfx950's
    // packed OCP converts (v_cvt_pk_f32_fp8 = e4m3fn, v_cvt_pk_f32_bf8 = e5m2): exact on all 256
    // patterns, subnormals, NaN and e5m2's inf included.  test_fp8_score_gpu pins that: every
    // pattern alone at every byte lane of an otherwise zero row, whose norm |x| * sqrt(D / 16)
    // tells every magnitude of the format apart (a norm cannot see a sign; NaN and inf show as
    // such).  x*x of an fp8 x is exact in fp32 either way.
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x2 lo, hi;
      if constexpr (DT == KVC_F8E4M3) {
        lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[q], false);
        hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[q], true);
      } else {
        lo = __builtin_amdgcn_cvt_pk_f32_bf8((int)w[q], false);
        hi = __builtin_amdgcn_cvt_pk_f32_bf8((int)w[q], true);
      }
      const int j0 = (q & 1) * 4;
      acc[j0] = __builtin_fmaf(lo.x, lo.x, acc[j0]);
      acc[j0 + 1] = __builtin_fmaf(lo.y, lo.y, acc[j0 + 1]);
      acc[j0 + 2] = __builtin_fmaf(hi.x, hi.x, acc[j0 + 2]);
      acc[j0 + 3] = __builtin_fmaf(hi.y, hi.y, acc[j0 + 3]);
    }
  } else if constexpr (DT == KVC_F16) {
    // NormTwoOps<Half, float> (binary_kernel_reduce): ONE accumulator in dim order; x*x is exact
    // in fp32 for an fp16 x, so the fma equals torch's acc + x*x.  (acc[1..7] stay 0: the final
    // lane sum adds +0 to a non-negative sum, which changes nothing.)
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float e0 = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[q] & 0xFFFFu));
      const float e1 = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[q] >> 16));
      acc[0] = __builtin_fmaf(e0, e0, acc[0]);
      acc[0] = __builtin_fmaf(e1, e1, acc[0]);
    }
  } else if constexpr (DT == KVC_BF16) {
    // chunk c holds elements 8c..8c+7: element e feeds accumulator e
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float e0 = bits_to_f32(w[q] << 16);
      const float e1 = bits_to_f32(w[q] & 0xFFFF0000u);
      acc[2 * q] = __builtin_fmaf(e0, e0, acc[2 * q]);
      acc[2 * q + 1] = __builtin_fmaf(e1, e1, acc[2 * q + 1]);
    }
  } else {
    // chunk c holds elements 4c..4c+3: accumulators 4*(c&1) + e
    const int j0 = (gchunk & 1) * 4;
    const float e[4] = {bits_to_f32(x.x), bits_to_f32(x.y), bits_to_f32(x.z), bits_to_f32(x.w)};
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[j0 + q] = __builtin_fmaf(e[q], e[q], acc[j0 + q]);
  }
}

// 16-B chunks of a token row staged per phase: 4 (64-B rows), 8 (multiples of 128 B), 10 (160 B
// multiples); a row of NC chunks takes NC / CP phases.
__host__ __device__ constexpr int score_cp(int nc) { return nc == 4 ? 4 : (nc % 8 == 0 ? 8 : 10); }
// padded LDS row of CP chunks: an odd number of 16-B granules keeps every lane's ds_read_b128 of
// its own token row conflict-free
__host__ __device__ constexpr int score_rowb(int cp) { return (cp + (cp % 2 == 0 ? 1 : 2)) * 16; }
// waves (tiles) per workgroup: 8 for CP-8 rows (9.2 KB slab per wave: two 74 KB workgroups per
// CU, 2.5% faster than four 4-wave ones); 2 for CP-10 rows (11.3 KB per wave: seven 2-wave
// workgroups per CU, 14 waves -- D = 80 score 0.1049 -> 0.1011 ms against three 4-wave ones
// (12 waves); two 7-wave ones, also 14 waves, 0.1063; 8-wave ones 45% slower); 4 for 64-B
// rows.  A/B in profiles/r03_j_score_variants_ab.jsonl and r03_l_select_variants.json.
__host__ __device__ constexpr int score_waves(int nc) {
  return score_cp(nc) == 8 ? 8 : score_cp(nc) == 10 ? 2 : 4;
}

// One 64-token tile of one (layer, b, h) row: coalesced 16-B loads -> per-wave LDS slab ->
// one lane per token, torch.norm's 8-accumulator FMA order (fp16: its serial order).  `wl` is
// this wave's slab (kTile * ROWB bytes).
// snapkv_lite rows (KVC_SCORE_SNAPKV) also get each tile's maximum stored norm, as the bits of
// the stored value (u16 for 16-bit dtypes, u32 for fp32) in tmax[row * tmax_stride + tile]: a
// norm is never negative (nor -0: the accumulators start at +0 and add squares), so the bit
// order is the value order and every NaN's bits exceed +inf's.  The select kernel forms the
// row's `max(norms)` (snapkv_lite.py:99) from them without a block reduction.
template <int DT, int NC>
__device__ __forceinline__ void score_tile(const kvc_layer_t* ly, int row, int tt, int H,
                                           char* wl, char* norms, int64_t norm_stride,
                                           uint32_t* tmax, int64_t tmax_stride) {
  constexpr int ESZ = DTypeTraits<DT>::esz;
  constexpr int SDT = score_dt(DT);  // the norm region's dtype (bf16 for fp8 keys)
  constexpr int CP = score_cp(NC);  // 16-B chunks per token per phase
  constexpr int NPH = NC / CP;
  constexpr int ROWB = score_rowb(CP);  // padded LDS row: conflict-free ds_read_b128 per lane
  const int lane = threadIdx.x & 63;
  const int zlen = ly->zone_len;
  const int b = row / H, h = row - (row / H) * H;
  const int tok0 = tt * kTile;
  const int ntok = min(kTile, zlen - tok0);
  const int64_t sbytes = ly->k_stride[2] * ESZ;
  const char* base = static_cast<const char*>(ly->k) +
                     ((int64_t)b * ly->k_stride[0] + (int64_t)h * ly->k_stride[1] +
                      (int64_t)(ly->zone_start + tok0) * ly->k_stride[2]) * ESZ;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ph = 0; ph < NPH; ++ph) {
    uint4 v[CP];
#pragma unroll
    for (int it = 0; it < CP; ++it) {
      const int q = it * 64 + lane;
      const int tok = q / CP, c = q - (q / CP) * CP;
      const char* src = base + tok * sbytes + (ph * CP + c) * 16;
      if (tok < ntok) {
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 w = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src));
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
    const float r = __builtin_sqrtf(s);
    char* nrow = norms + (int64_t)(ly->row0 + row) * norm_stride * DTypeTraits<SDT>::esz;
    // non-temporal: the select phase reads the norms back from the Infinity Cache, not from
    // this XCD's L2, so keeping them in L2 only evicts key lines (2.5% faster score pass)
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

// Global tile g (kvc_plan's tile0 numbering) of a chunk of nl layers: its layer, the layer's
// (b, h) row and the tile within the row.
struct TileAt {
  int layer, row, tile;
};
__device__ __forceinline__ TileAt locate_tile(const kvc_layer_t* L, int nl, int64_t g) {
  int lo = 0, hi = nl - 1;  // largest layer with tile0 <= g
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (L[mid].tile0 <= g)
      lo = mid;
    else
      hi = mid - 1;
  }
  const int tpr = (L[lo].zone_len + kTile - 1) / kTile;
  const int local = (int)(g - L[lo].tile0);
  const int row = local / tpr;
  return {lo, row, local - row * tpr};
}

template <int DT, int NC>
__global__ void __launch_bounds__(score_waves(NC) * 64)
    score_kernel(const LayerChunk T, int nl, int H, int64_t tile_base, int64_t chunk_tiles,
                 char* __restrict__ norms, int64_t norm_stride, uint32_t* __restrict__ tmax,
                 int64_t tmax_stride) {
  constexpr int CP = score_cp(NC);
  constexpr int ROWB = score_rowb(CP);
  constexpr int kScoreWaves = score_waves(NC);
  __shared__ __attribute__((aligned(16))) char lds[kScoreWaves][kTile * ROWB];
  const kvc_layer_t* L = T.l;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // one tile per wave (default grid); a smaller grid makes the waves stride over the tiles
  const int64_t stride = (int64_t)gridDim.x * kScoreWaves;
  for (int64_t gl = (int64_t)blockIdx.x * kScoreWaves + wid; gl < chunk_tiles; gl += stride) {
    const TileAt at = locate_tile(L, nl, tile_base + gl);
    score_tile<DT, NC>(L + at.layer, at.row, at.tile, H, lds[wid], norms, norm_stride, tmax,
                       tmax_stride);
  }
}

}  // namespace kvc
