// kvc_snapkv_keys.h -- snapkv_lite importance scores, pooled and mapped to sort keys (the key
// phase of a snapkv row's selection).
#pragma once

#include "kvc_device_util.h"

namespace kvc {

// 16-bit score conversions of the snapkv keys: bf16 by the c10 bit arithmetic, fp16 by the
// hardware converts (kvc_common.h: c10-exact except NaN payloads, which the keys never see --
// every NaN maps to the one NaN key).
template <int DT>
__device__ __forceinline__ float in16(uint32_t u) {
  if constexpr (DT == KVC_BF16) return bf16_to_f32(u);
  else return f16_to_f32_hw(u);
}
template <int DT>
__device__ __forceinline__ uint32_t out16(float f) {
  if constexpr (DT == KVC_BF16) return f32_to_bf16_rne(f);
  else return f32_to_f16_hw(f);
}

// snapkv_lite importance scores (snapkv_lite.py:96-121) computed from the row's norms and
// written as sort keys:  m = dt(max(norms) + 1e-6);  s = dt(m - norm);
// pooled_i = dt(sum_{window} s / pool_size) (avg_pool1d, zero pad, count_include_pad).
template <int DT, typename KeyT, int NT>
__device__ void snapkv_keys(const char* nrow, int n, int pool_k, bool desc, KeyT* key,
                            char* tmp, SelScalars<KeyT>& sc) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  float mx = -__builtin_huge_valf();
  int has_nan = 0;
  for (int i = tid; i < n; i += NT) {
    const float v = load_dt<DT>(nrow, i);
    if (v != v) has_nan = 1;
    else if (v > mx) mx = v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float y = __shfl_xor(mx, o, 64);
    mx = y > mx ? y : mx;
    has_nan |= __shfl_xor(has_nan, o, 64);
  }
  if (lane == 0) {
    sc.fmax[wid] = mx;
    sc.fnan[wid] = has_nan;
  }
  __syncthreads();
  mx = sc.fmax[0];
  has_nan = sc.fnan[0];
  for (int w = 1; w < NT / 64; ++w) {
    mx = sc.fmax[w] > mx ? sc.fmax[w] : mx;
    has_nan |= sc.fnan[w];
  }
  if (has_nan) mx = __builtin_nanf("");
  // `max + 1e-6` (snapkv_lite.py:99): the python scalar takes the tensor's dtype first
  const float m = round_dt<DT>(mx + round_dt<DT>(1e-6f));
  for (int i = tid; i < n; i += NT) {
    const float s = round_dt<DT>(m - load_dt<DT>(nrow, i));
    if constexpr (DT != KVC_F32)
      reinterpret_cast<uint16_t*>(tmp)[i] = (uint16_t)bits16_dt<DT>(s);
    else
      reinterpret_cast<float*>(tmp)[i] = s;
  }
  __syncthreads();
  const bool pool = pool_k > 1 && n >= pool_k;
  const int pad = pool_k / 2;
  for (int i = tid; i < n; i += NT) {
    float r;
    if (pool) {
      int hs = i - pad;
      int he = min(hs + pool_k, n + pad);
      const int psize = he - hs;
      hs = max(hs, 0);
      he = min(he, n);
      float sum = 0.f;
      for (int j = hs; j < he; ++j) sum = sum + load_dt<DT>(tmp, j);
      r = sum / (float)psize;
    } else {
      r = load_dt<DT>(tmp, i);
    }
    key[i] = key_of<DT>(r, desc);
  }
}

// x / 5 correctly rounded (= the IEEE division avg_pool1d performs), without the division
// sequence: q0 = x * RN(1/5), residual r = x - 5 q0 exact in one FMA, q1 = q0 + r * RN(1/5);
// q0 itself where r == 0 (keeps -0) or q0 is infinite.  Checked against x / 5.0f for all 2^32
// fp32 patterns (tests/native/div5_check.c; tests/test_native_abi.py runs a strided sample).
__device__ __forceinline__ float div5_rn(float x) {
  const float q0 = x * 0.2f;
  const float r = __builtin_fmaf(-q0, 5.0f, x);
  return (r == 0.0f || __builtin_isinf(q0)) ? q0 : __builtin_fmaf(r, 0.2f, q0);
}

// The pooled key vector of positions 8v .. 8v+7 (default pooling kernel 5, or none) from the
// 16-bit scores of positions 8v-8 .. 8v+15 as floats in sw[0..24) (only 8v-2 .. 8v+9 are read;
// terms outside [hs, he) are skipped): avg_pool1d's window sums in its order, / 5 by div5_rn,
// rounded to the dtype, mapped to sort keys; positions past n get 0.
// nonneg (bf16): every score of the row is finite and >= +0 -- the row max is finite, so m >=
// every norm, and a finite norm is at most sqrt(FLT_MAX) < 2e19, so no whole-window sum (<= 5 m)
// overflows.  div5_rn's guards then never fire but for r == 0, which only decides the sign of a
// zero quotient (the keys equate +0 and -0), the division runs as packed fp32 ops, and a value
// >= +0 maps to key 0x8000 | bits, key_bf16x2's code for it.
template <int DT>
__device__ __forceinline__ uint4 snapkv_pool_vec(const float (&sw)[24], int v, int n, bool pool,
                                                 bool desc, bool nonneg = false) {
  uint32_t o[4] = {0, 0, 0, 0};
  if constexpr (DT == KVC_BF16) {
    // bf16: pairs of positions with packed fp32 adds, one hardware convert and one packed key
    // map per pair (key_bf16x2 codes for every key of the row).  The window sums drop
    // avg_pool1d's leading 0 + s: it only turns a -0 into +0, and the keys equate the two.
    typedef float f2 __attribute__((ext_vector_type(2)));
    const bool inner = pool && v >= 1 && v * 8 + 10 <= n;  // every window of the vector whole
    if (inner && nonneg) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        f2 acc = f2{sw[2 * p + 6], sw[2 * p + 7]};
#pragma unroll
        for (int t = 1; t < 5; ++t) acc = acc + f2{sw[2 * p + 6 + t], sw[2 * p + 7 + t]};
        const f2 q0 = acc * f2{0.2f, 0.2f};
        const f2 r = __builtin_elementwise_fma(-q0, f2{5.0f, 5.0f}, acc);
        const f2 q = __builtin_elementwise_fma(r, f2{0.2f, 0.2f}, q0);
        const uint32_t k = f32x2_to_bf16x2_hw(q.x, q.y) | 0x80008000u;
        o[p] = desc ? ~k : k;  // inner: all 8 positions < n
      }
      return make_uint4(o[0], o[1], o[2], o[3]);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      f2 r;
      if (inner) {
        f2 acc = f2{sw[2 * p + 6], sw[2 * p + 7]};
#pragma unroll
        for (int t = 1; t < 5; ++t) acc = acc + f2{sw[2 * p + 6 + t], sw[2 * p + 7 + t]};
        r = f2{div5_rn(acc.x), div5_rn(acc.y)};
      } else {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int e = 2 * p + b, i = v * 8 + e;
          float x = sw[8 + e];
          if (pool) {  // pool_k == 5, pad 2: window [i - 2, i + 3) clipped to [0, n), / 5
            int hs = i - 2;
            int he = min(hs + 5, n + 2);
            const int psize = he - hs;
            hs = max(hs, 0);
            he = min(he, n);
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < 5; ++t) {
              const int j = i - 2 + t;
              if (j >= hs && j < he) sum = sum + sw[8 + e - 2 + t];
            }
            x = psize == 5 ? div5_rn(sum) : sum / (float)psize;
          }
          r[b] = x;
        }
      }
      const int i0 = v * 8 + 2 * p;
      o[p] = key_bf16x2(f32x2_to_bf16x2_hw(r.x, r.y), desc) &
             (i0 + 1 < n ? 0xFFFFFFFFu : i0 < n ? 0x0000FFFFu : 0u);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int i = v * 8 + e;
      float r;
      if (pool) {  // pool_k == 5, pad 2: window [i - 2, i + 3) clipped to [0, n), / 5
        int hs = i - 2;
        int he = min(hs + 5, n + 2);
        const int psize = he - hs;
        hs = max(hs, 0);
        he = min(he, n);
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
          const int j = i - 2 + t;
          if (j >= hs && j < he) sum = sum + sw[8 + e - 2 + t];
        }
        r = psize == 5 ? div5_rn(sum) : sum / (float)psize;
      } else {
        r = sw[8 + e];
      }
      o[e >> 1] |= (i < n ? (uint32_t)key16_dt<DT>(out16<DT>(r), desc) : 0u) << (16 * (e & 1));
    }
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

// 16-bit scores s = dt(m - norm) of the two positions of a norm dword (the positions' order in
// the dword kept): bf16 by one hardware convert per pair (NaN payloads unobserved), fp16 by the
// hardware converts.
template <int DT>
__device__ __forceinline__ uint32_t snapkv_score_pair(float m, uint32_t w) {
  if constexpr (DT == KVC_BF16)
    return f32x2_to_bf16x2_hw(m - bf16_to_f32(w), m - bits_to_f32(w & 0xFFFF0000u));
  else
    return out16<DT>(m - in16<DT>(w & 0xFFFFu)) | (out16<DT>(m - in16<DT>(w >> 16)) << 16);
}

// snapkv_keys for 16-bit scores on LDS rows (n <= MAXV * 8 * NT): the same arithmetic per
// position (snapkv_lite.py:96-121), each thread making the keys of 8 consecutive positions.
// `key`, `idx`, `tmp` and `nrow` are 16-B aligned; norm rows are padded to a multiple of 64
// elements (a vector or dword past n stays inside the row; its values are never used).
//  * With `trow` (SCORE's per-tile maxima of this row, score_tile) and the default pooling kernel
//    5 (or none): no block barrier and no scores round trip -- every wave reduces the tile
//    maxima to `max(norms)` itself, and each thread forms the scores of its 8 positions and the
//    two on either side (a 16-B load of its norms and two 4-B halo loads) in registers, pools
//    them and writes its keys AND its index vector (returns true: idx is initialised).
//  * Otherwise (rounds 2-5 form): the row's norms read once as 16-B vectors (kept in registers
//    for the max and the scores), a block max, scores stored to `tmp` as 16-B vectors, and each
//    thread pooling 8 positions from three 16-B reads of them (kernel 5; other kernels one
//    position at a time as snapkv_keys).  Returns false: the caller initialises idx (tmp
//    aliases it).
template <int DT, int NT, int MAXV>
__device__ __forceinline__ bool snapkv_keys16(const char* nrow, const uint32_t* trow, int n,
                                              int pool_k, bool desc, uint16_t* key, uint16_t* idx,
                                              uint16_t* tmp, SelScalars<uint16_t>& sc,
                                              uint64_t* stamps = nullptr) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nvec = (n + 7) >> 3;
  constexpr uint32_t kInf = DT == KVC_BF16 ? 0x7F80u : 0x7C00u;
  const bool pool = pool_k > 1 && n >= pool_k;
  if (trow && (pool_k == 5 || !pool)) {
    // max(norms) from the tile maxima (bits of the stored norms, at most 256 tiles: <= 4 loads
    // per lane), one wave reduction; a NaN's bits exceed +inf's.  (Issuing every norm load
    // before this reduction measured the same: profiles/r06_b_snapkv_ab.jsonl, snap2.)
    uint32_t mb = 0;
    const int nt = (n + kTile - 1) / kTile;
    for (int t = lane; t < nt; t += 64) mb = max(mb, trow[t]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mb = max(mb, (uint32_t)__shfl_xor((int)mb, o, 64));
    const float mx = mb > kInf ? __builtin_nanf("") : in16<DT>(mb);
    // `max + 1e-6` (snapkv_lite.py:99): the python scalar takes the tensor's dtype first
    const float m = in16<DT>(out16<DT>(mx + in16<DT>(out16<DT>(1e-6f))));
    const bool nonneg = mb < kInf;  // finite max: every score m - norm is finite and >= +0
    KVC_STAMP(26);
    const uint32_t* nw = reinterpret_cast<const uint32_t*>(nrow);
#pragma unroll
    for (int q = 0; q < MAXV; ++q) {
      const int v = tid + q * NT;
      if (v >= nvec) continue;
      const uint4 c = reinterpret_cast<const uint4*>(nrow)[v];
      const uint32_t wp = v > 0 ? nw[4 * v - 1] : 0u;          // positions 8v-2, 8v-1
      const uint32_t wn = v + 1 < nvec ? nw[4 * v + 4] : 0u;   // positions 8v+8, 8v+9
      const uint32_t sc6[6] = {snapkv_score_pair<DT>(m, wp), snapkv_score_pair<DT>(m, c.x),
                               snapkv_score_pair<DT>(m, c.y), snapkv_score_pair<DT>(m, c.z),
                               snapkv_score_pair<DT>(m, c.w), snapkv_score_pair<DT>(m, wn)};
      float sw[24];
#pragma unroll
      for (int e = 0; e < 24; ++e) sw[e] = 0.f;
#pragma unroll
      for (int d = 0; d < 6; ++d) {  // scores of positions 8v - 2 + 2d, +1 at sw[6 + 2d], +1
        sw[6 + 2 * d] = in16<DT>(sc6[d] & 0xFFFFu);
        sw[7 + 2 * d] = in16<DT>(sc6[d] >> 16);
      }
      reinterpret_cast<uint4*>(key)[v] = snapkv_pool_vec<DT>(sw, v, n, pool, desc, nonneg);
      const uint32_t b = (uint32_t)v * 8;
      reinterpret_cast<uint4*>(idx)[v] =
          make_uint4(b | (b + 1) << 16, (b + 2) | (b + 3) << 16, (b + 4) | (b + 5) << 16,
                     (b + 6) | (b + 7) << 16);
    }
    KVC_STAMP(29);
    return true;
  }
  uint4 raw[MAXV];
  float mx = -__builtin_huge_valf();
  // Branch-free local max: the NaN-ignoring float max (v_max_f32) of every element, NaN
  // detected apart as the packed-u16 max magnitude above inf.  Positions past n read as -inf.
  // (A signed zero max is harmless: m = dt(max + 1e-6) is the same for -0 and +0.)
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  u16x2 mag = (u16x2)0;
#pragma unroll
  for (int q = 0; q < MAXV; ++q) {
    const int v = tid + q * NT;
    raw[q] = v < nvec ? reinterpret_cast<const uint4*>(nrow)[v] : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (int q = 0; q < MAXV; ++q) {
    const int v = tid + q * NT;
    const uint32_t w[4] = {raw[q].x, raw[q].y, raw[q].z, raw[q].w};
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int i0 = v * 8 + 2 * h;
      const uint32_t ninf = 0x8000u | kInf;  // -inf
      const uint32_t x = i0 + 1 < n ? w[h] : i0 < n ? (w[h] & 0xFFFFu) | (ninf << 16)
                                                     : ninf | (ninf << 16);
      mx = __builtin_fmaxf(mx, __builtin_fmaxf(in16<DT>(x & 0xFFFFu), in16<DT>(x >> 16)));
      mag = __builtin_elementwise_max(mag, __builtin_bit_cast(u16x2, x & 0x7FFF7FFFu));
    }
  }
  int has_nan = (mag.x > kInf || mag.y > kInf) ? 1 : 0;
  KVC_STAMP(26);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float y = __shfl_xor(mx, o, 64);
    mx = __builtin_fmaxf(mx, y);
    has_nan |= __shfl_xor(has_nan, o, 64);
  }
  if (lane == 0) {
    sc.fmax[wid] = mx;
    sc.fnan[wid] = has_nan;
  }
  __syncthreads();
  mx = sc.fmax[0];
  has_nan = sc.fnan[0];
  for (int w = 1; w < NT / 64; ++w) {
    mx = __builtin_fmaxf(mx, sc.fmax[w]);
    has_nan |= sc.fnan[w];
  }
  if (has_nan) mx = __builtin_nanf("");
  // `max + 1e-6` (snapkv_lite.py:99): the python scalar takes the tensor's dtype first
  const float m = in16<DT>(out16<DT>(mx + in16<DT>(out16<DT>(1e-6f))));
  KVC_STAMP(27);
#pragma unroll
  for (int q = 0; q < MAXV; ++q) {
    const int v = tid + q * NT;
    if (v >= nvec) continue;
    const uint32_t w[4] = {raw[q].x, raw[q].y, raw[q].z, raw[q].w};
    uint32_t o[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int i0 = v * 8 + 2 * h;
      o[h] = snapkv_score_pair<DT>(m, w[h]) &
             (i0 + 1 < n ? 0xFFFFFFFFu : i0 < n ? 0x0000FFFFu : 0u);
    }
    reinterpret_cast<uint4*>(tmp)[v] = make_uint4(o[0], o[1], o[2], o[3]);
  }
  __syncthreads();
  KVC_STAMP(28);
  if (pool && pool_k != 5) {  // other kernels: one position at a time (snapkv_keys)
    const int pad = pool_k / 2;
    for (int i = tid; i < n; i += NT) {
      int hs = i - pad;
      int he = min(hs + pool_k, n + pad);
      const int psize = he - hs;
      hs = max(hs, 0);
      he = min(he, n);
      float sum = 0.f;
      for (int j = hs; j < he; ++j) sum = sum + in16<DT>(tmp[j]);
      key[i] = key16_dt<DT>(out16<DT>(sum / (float)psize), desc);
    }
    return false;
  }
  const uint4* tv = reinterpret_cast<const uint4*>(tmp);
#pragma unroll
  for (int q = 0; q < MAXV; ++q) {
    const int v = tid + q * NT;
    if (v >= nvec) continue;
    // scores of positions 8v - 8 .. 8v + 15 (zero outside the row: never summed)
    float sw[24];
    const uint4 c3[3] = {v > 0 ? tv[v - 1] : make_uint4(0, 0, 0, 0), tv[v],
                         v + 1 < nvec ? tv[v + 1] : make_uint4(0, 0, 0, 0)};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t w[4] = {c3[c].x, c3[c].y, c3[c].z, c3[c].w};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t u = (w[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
        sw[c * 8 + e] = in16<DT>(u);
      }
    }
    reinterpret_cast<uint4*>(key)[v] = snapkv_pool_vec<DT>(sw, v, n, pool, desc);
  }
  KVC_STAMP(29);
  return false;
}

}  // namespace kvc
