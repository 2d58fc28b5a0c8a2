// kvc_attn.h -- h2o_attention: the accumulate / head-sum kernels (torch's CPU sums restated).
#pragma once

#include "kvc_device_util.h"

namespace kvc {

// ---------------------------------------------------------------------------------------------
// h2o_attention heavy hitters: torch's CPU sums restated per output column
// ---------------------------------------------------------------------------------------------
// aten cascade_sum (SumKernel.cpp) adds the rows of one output column in one of two orders:
//   cascade (multi_row_sum): four accumulator levels; rows go one by one into level 0, and after
//     every 2^p rows (p = max(4, CeilLog2(n) / 4)) level j-1 is folded into level j while the row
//     counter's j-th p-bit digit is zero; result ((a0 + a1) + a2) + a3.
//   ilp4 (row_sum): four interleaved lanes (row i -> lane i % 4), each a cascade over n / 4 rows,
//     leftover rows into lane 0, then ((l0 + l1) + l2) + l3.
// Which columns take ilp4 depends on the loop calls the reference made (col_class).
__device__ __forceinline__ int ceil_log2_i(int x) { return x <= 2 ? 1 : 32 - __clz(x - 1); }

template <typename LD>
__device__ __forceinline__ float cascade_sum(const LD& ld, int n, int off, int mul) {
  const int lp = max(4, ceil_log2_i(n) / 4);
  const int step = 1 << lp, mask = step - 1;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int i = 0;
  while (i + step <= n) {
    if (step == 16) {  // the common level size: loads first, then the dependent adds
      float x[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) x[t] = ld(off + (i + t) * mul);
#pragma unroll
      for (int t = 0; t < 16; ++t) a0 = a0 + x[t];
      i += 16;
    } else {
      for (int t = 0; t < step; ++t, ++i) a0 = a0 + ld(off + i * mul);
    }
    a1 = a1 + a0;
    a0 = 0.f;
    if ((i & (mask << lp)) == 0) {
      a2 = a2 + a1;
      a1 = 0.f;
      if ((i & (mask << (2 * lp))) == 0) {
        a3 = a3 + a2;
        a2 = 0.f;
      }
    }
  }
  for (; i < n; ++i) a0 = a0 + ld(off + i * mul);
  a0 = a0 + a1;
  a0 = a0 + a2;
  return a0 + a3;
}

template <typename LD>
__device__ __forceinline__ float ilp4_sum(const LD& ld, int n) {
  const int n4 = n >> 2;
  float p0 = cascade_sum(ld, n4, 0, 4);
  const float p1 = cascade_sum(ld, n4, 1, 4);
  const float p2 = cascade_sum(ld, n4, 2, 4);
  const float p3 = cascade_sum(ld, n4, 3, 4);
  for (int i = 4 * n4; i < n; ++i) p0 = p0 + ld(i);
  p0 = p0 + p1;
  p0 = p0 + p2;
  return p0 + p3;
}

// Does column j of `cols` take the ilp4 order?  The reference's loop calls cover the columns in
// chunks: one call [0, cols) (chunk == 0), or parallel_dim_reduction's thread chunks of `chunk`
// columns with bounds rounded down to `rnd` columns (128 bytes; the final end stays cols).  In a
// call of L columns the vectorised loop (L >= vec_min = one Vectorized<scalar_t>) sums whole
// groups of `group` columns (four Vectorized<float>) with the cascade and the rest with row_sum;
// a shorter call sums groups of four columns with the cascade and the rest with row_sum.
__device__ __forceinline__ bool col_ilp(int j, int cols, int chunk, int rnd, int group,
                                        int vec_min) {
  int s = 0, e = cols;
  if (chunk > 0) {
    const int T = (cols + chunk - 1) / chunk;  // threads that start below cols
    int t = j / chunk;
    while (t + 1 < T && ((t + 1) * chunk) / rnd * rnd <= j) ++t;
    s = (t * chunk) / rnd * rnd;
    e = t + 1 < T ? ((t + 1) * chunk) / rnd * rnd : cols;
  }
  const int L = e - s;
  const int g = L >= vec_min ? group : 4;
  return j - s >= L / g * g;
}

template <int DT>
__device__ __forceinline__ uint32_t store_bits(float f) {
  if constexpr (DT == KVC_F32)
    return f32_to_bits(f);
  else
    return bits16_dt<DT>(f);
}
template <int DT>
__device__ __forceinline__ void store_dt(void* base, int64_t i, float f) {
  if constexpr (DT == KVC_F32)
    reinterpret_cast<float*>(base)[i] = f;
  else
    reinterpret_cast<uint16_t*>(base)[i] = (uint16_t)bits16_dt<DT>(f);
}

struct AttnChunk {
  kvc_attn_layer_t l[kArgLayers];
};
struct HHChunk {
  kvc_hh_layer_t l[kArgLayers];
};
constexpr int kColThreads = 256;

// update_attention_scores (h2o_attention.py:100-151) for every layer of the chunk: grid
// (layer * batch * heads rows, column blocks); one thread per key column:
//   imp = dt(0 + sum_q attn[b,h,q,j])                     attn.sum(dim=2)           (:116)
//   acc_new = dt(base + imp), base = dt(acc_old*decay) for j < old_len, else 0  (:118-151)
// Reads of attn are coalesced across the block's columns (q rows of stride attn_stride[2]).
// ODT: dtype of acc_old.  ODT != DT (the carried accumulation and the new attention differ in
// dtype, every layer carried): base is rounded to ODT, and acc_new is fp32 -- torch's promotion
// of two different float dtypes through torch.cat / + (:129-151) -- holding fp32(base) + fp32(imp).
// V consecutive elements of dtype DT at element offset i of `base` as floats: one 16-B load when
// the span is whole and 16-B aligned, else element by element (n valid, the rest 0).
template <int DT, int V>
__device__ __forceinline__ void load_vec(const char* base, int64_t i, int n, float (&x)[V]) {
  constexpr int ESZ = DTypeTraits<DT>::esz;
  constexpr int PER = 16 / ESZ;  // elements per 16-B load
  const char* p = base + i * ESZ;
  if (n == V && V % PER == 0 && ((uintptr_t)p & 15u) == 0) {
#pragma unroll
    for (int c = 0; c < V / PER; ++c) {
      const uint4 w = reinterpret_cast<const uint4*>(p)[c];
      const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        if constexpr (DT == KVC_F32) x[c * PER + e] = bits_to_f32(u[e]);
        else if constexpr (DT == KVC_BF16)
          x[c * PER + e] = bf16_to_f32((u[e / 2] >> (16 * (e & 1))) & 0xFFFFu);
        else x[c * PER + e] = f16_to_f32((u[e / 2] >> (16 * (e & 1))) & 0xFFFFu);
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) x[e] = e < n ? load_dt<DT>(p, e) : 0.f;
  }
}

// The first n of V floats stored as dtype DT at element offset i of `base` (rounded as
// store_dt): 16-B stores when the span is whole and aligned.
template <int DT, int V>
__device__ __forceinline__ void store_vec(void* base, int64_t i, int n, const float (&x)[V]) {
  constexpr int ESZ = DTypeTraits<DT>::esz;
  char* p = static_cast<char*>(base) + i * ESZ;
  constexpr int PER = 16 / ESZ;  // elements per 16-B store
  if (n == V && V % PER == 0 && ((uintptr_t)p & 15u) == 0) {
#pragma unroll
    for (int c = 0; c < V / PER; ++c) {
      uint32_t u[4];
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        if constexpr (DT == KVC_F32) u[w] = f32_to_bits(x[c * PER + w]);
        else u[w] = store_bits<DT>(x[c * PER + 2 * w]) | (store_bits<DT>(x[c * PER + 2 * w + 1]) << 16);
      }
      *reinterpret_cast<uint4*>(p + c * 16) = make_uint4(u[0], u[1], u[2], u[3]);
    }
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e)
      if (e < n) store_dt<DT>(base, i + e, x[e]);
  }
}

// ODT: dtype of acc_old.  ODT != DT (the carried accumulation and the new attention differ in
// dtype, every layer carried): base is rounded to ODT, and acc_new is fp32 -- torch's promotion
// of two different float dtypes through torch.cat / + (:129-151) -- holding fp32(base) + fp32(imp).
// One thread per kAccCols consecutive key columns (16-B loads and stores where aligned): with one
// column per thread a 32-layer decode step's [32, 16 384] rows took 65 536 workgroups and the
// launch ~130 us, bound by workgroup turnover, not bytes.
constexpr int kAccCols = 8;
template <int DT, int ODT>
__global__ void __launch_bounds__(kColThreads)
    attn_accum_kernel(const AttnChunk T, int H, int BH, float decay, int group, int vec_min,
                      int rnd) {
  constexpr int ESZ = DTypeTraits<DT>::esz;
  constexpr int NDT = ODT == DT ? DT : KVC_F32;  // acc_new's dtype
  constexpr int V = kAccCols;
  const kvc_attn_layer_t* ly = T.l + blockIdx.x / BH;
  const int r = (int)(blockIdx.x % BH);
  const int j0 = ((int)blockIdx.y * kColThreads + (int)threadIdx.x) * V;
  const int k = ly->key_len;
  if (j0 >= k) return;
  const int n = min(V, k - j0);
  const int b = r / H, h = r - (r / H) * H;
  const char* a = static_cast<const char*>(ly->attn) +
                  ((int64_t)b * ly->attn_stride[0] + (int64_t)h * ly->attn_stride[1]) * ESZ;
  const int64_t qs = ly->attn_stride[2] * ESZ;
  const int q = ly->q_len;
  float s[V];
  if (q == 1) {  // no reduction: the elementwise out = 0 + x
    load_vec<DT, V>(a, j0, n, s);
#pragma unroll
    for (int e = 0; e < V; ++e) s[e] = 0.f + s[e];
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int j = j0 + e;
      if (e >= n) {
        s[e] = 0.f;
        continue;
      }
      const auto ld = [&](int i) { return load_dt<DT>(a + (int64_t)i * qs, j); };
      // the accumulating store adds to the zero-filled output
      s[e] = col_ilp(j, k, ly->col_chunk, rnd, group, vec_min) ? 0.f + ilp4_sum(ld, q)
                                                                      : 0.f + cascade_sum(ld, q, 0, 1);
    }
  }
  float base[V];
  const int nold = min(n, ly->old_len - j0);  // carried columns of this thread (may be <= 0)
  if (nold > 0)
    load_vec<ODT, V>(static_cast<const char*>(ly->acc_old), (int64_t)r * ly->old_len + j0, nold,
                     base);
  float out[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const float bse = e < nold ? round_dt<ODT>(base[e] * decay) : 0.f;
    out[e] = bse + round_dt<DT>(s[e]);
  }
  store_vec<NDT, V>(ly->acc_new, (int64_t)r * k + j0, n, out);
}

// get_heavy_hitter_indices' head sum (h2o_attention.py:194-198) for every layer of the chunk:
// grid (layer * batch rows, column blocks); row l*batch + b of `sums` (dtype, row stride
// `stride`) receives dt(0 + sum_h acc[b, h, m0 + j]) for j < zone_len.
template <int DT>
__global__ void __launch_bounds__(kColThreads)
    head_sum_kernel(const HHChunk T, int H, int B, int group, int vec_min, char* sums,
                    int64_t stride) {
  constexpr int ESZ = DTypeTraits<DT>::esz;
  const int l = (int)(blockIdx.x / B), b = (int)(blockIdx.x % B);
  const kvc_hh_layer_t* ly = T.l + l;
  const int j = (int)blockIdx.y * kColThreads + (int)threadIdx.x;
  const int m = ly->zone_len;
  if (j >= m) return;
  const char* a = static_cast<const char*>(ly->acc) +
                  ((int64_t)b * H * ly->acc_len + ly->zone_start + j) * ESZ;
  const int64_t hs = (int64_t)ly->acc_len * ESZ;
  const auto ld = [&](int i) { return load_dt<DT>(a + (int64_t)i * hs, 0); };
  float s;
  if (H == 1)
    s = 0.f + ld(0);
  else if (col_ilp(j, m, ly->col_chunk, 128 / ESZ, group, vec_min))
    s = 0.f + ilp4_sum(ld, H);
  else
    s = 0.f + cascade_sum(ld, H, 0, 1);
  store_dt<DT>(sums + (int64_t)blockIdx.x * stride * ESZ, j, s);
}

}  // namespace kvc
