// kvc_observe.h -- observation-window scores (SnapKV): how much a layer's last W queries attend
// to each zone key, written where SELECT reads plain-norm scores (kvc_observe_score, include/kvc.h).
//
// Per (layer, b, kv head) row the work is the GEMM  Q_obs (M = G*W queries x D)  .  K^T (D x S)
// with a softmax across S and a column sum over the M queries.  The S x M logits are never
// stored (4 MiB per row at S = 16 384): K is streamed twice and the logits are recomputed.
//
//   observe_pass_kernel<.., 1>  statistics: grid (rows, 1 024-key chunks).  Online (max, sum) of
//                               every query row over the chunk's keys -> one partial per
//                               (row, chunk, wave, query) in scratch.
//   observe_pass_kernel<.., 2>  column sums: the same grid over the chunks that meet the zone.
//                               Combines the row's partials into lse_i, recomputes the logits,
//                               sums exp(s - lse_i) over the queries -> fp32 imp[row][zone col].
//   observe_pool_kernel         pools imp across tile and chunk boundaries (zero / -inf padding
//                               inside the zone), rounds, stores into the norm region.
//
// How a workgroup (4 waves) splits a 128-key tile.  Queries lie on the MFMA's M dimension
// (v_mfma_f32_32x32x16: A = 32 queries x 16 dims, B = 16 dims x 32 keys), so a lane owns ONE key
// column of the 32 x 32 logit block and 16 of its 32 query rows: the column sum over queries is
// 16 in-register adds and one exchange between the wave's halves, and a query row's (max, sum)
// stays per lane until the chunk ends (one butterfly over 32 lanes per chunk, not per tile).
// M = G*W is 16 .. 128, i.e. MB = 1, 2 or 4 blocks of 32 query rows (M = 16: half a block of zero
// rows, masked out through lse = +inf).  Every wave holds ONE block's Q fragments in registers for
// the whole chunk (D / 16 k-steps x 4 VGPRs: 32 at D = 128) and takes MB of the tile's MB * 4
// (block, 32-key sub-tile) items: wave w has block w % MB and sub-tiles w / MB + i * (4 / MB).
// An M = 128 accumulator set in one wave (64 VGPRs of logits, 256 of statistics) is never formed.
//
// Data movement.  The tile's 128 keys x D are loaded with coalesced 16-B loads (the next tile's
// into registers while this one is multiplied), stored to LDS rows of D*2 + 16 bytes, and read
// back as B operands with ds_read_b128: lane l reads row l % 32 at chunk 2*kk + l / 32.  A row
// stride of an odd number of 16-B granules (NC + 1) sends the 16 lanes of one ds_read_b128 phase
// to 16 different granules of the 256-B bank line -- rows r and r + 16 first share one, and they
// are in different phases -- the rule kvc_score.h's slab uses; checked the same way, by the
// addresses: (r * (NC + 1) + c) mod 16 is a bijection of r in [0, 16) for even NC.
//
// Paged and fp8 keys (kvc_observe_score_paged) run the pass kernel of kvc_observe_src.h: a COPY of
// observe_pass_kernel with another tile loader, kept apart so that the dense 16-bit instances stay
// the code they were.  A fix to one pass body is a fix to both.
#pragma once

#include "kvc_device_util.h"
#include "kvc_gather.h"  // layer_selects

namespace kvc {

constexpr int kObsLayers = 32;    // layers per argument chunk (176 B of tables per layer)
constexpr int kObsThreads = 256;  // 4 waves
constexpr int kObsWaves = 4;
constexpr int kObsTile = 128;     // keys per LDS tile: four 32-key MFMA sub-tiles
constexpr int kObsChunk = 1024;   // keys per workgroup
constexpr int kObsMaxM = 128;     // G * W
constexpr int kPoolThreads = 256;
// pass 2 is the last reader of the keys: non-temporal loads (measured against default loads,
// the headline set 2.03 -> 1.80 ms, the G = 4 point unchanged)
constexpr bool kObsPass2NT = true;

struct ObserveChunk {
  kvc_layer_t l[kObsLayers];
  kvc_observe_layer_t q[kObsLayers];
};

struct ObserveArgs {
  int H, BH;         // kv heads; batch * kv heads (rows per layer)
  int G, W, M, MB;   // group size, window, G * W, 32-row query blocks
  float scale2;      // scale * log2(e): the softmax runs on exp2
  int pool, pool_max;
  int64_t nstride;   // norm row stride (elements of the call's dtype)
  int64_t pstride;   // partial slots per row: chunks of the longest layer * kObsWaves
  int64_t istride;   // imp floats per row
  int64_t fstride;   // scores_f32 floats per row
  float2* part;      // [rows][pstride][32] (max, sum) in the exp2 domain
  float* imp;        // [rows][istride]
  char* norms;
  float* f32;        // optional un-rounded scores
};

// A layer the kernels score: it has a zone, and someone reads the result.
__host__ __device__ __forceinline__ bool observe_scored(const kvc_layer_t& y, bool f32) {
  return y.zone_len > 0 && (layer_selects(y) || f32);
}

typedef float f32x16 __attribute__((ext_vector_type(16)));
template <int DT>
__device__ __forceinline__ f32x16 obs_mfma(uint4 a, uint4 b, f32x16 c) {
  if constexpr (DT == KVC_BF16) {
    typedef __bf16 v8 __attribute__((ext_vector_type(8)));
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8, a),
                                                   __builtin_bit_cast(v8, b), c, 0, 0, 0);
  } else {
    typedef _Float16 v8 __attribute__((ext_vector_type(8)));
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8, a),
                                                  __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
}

// Packed fp32 instructions (v_pk_*_f32) are kept out of these kernels.  The per-row updates of
// neighbouring accumulator registers are isomorphic, and the SLP vectoriser pairs them; an empty
// asm on a value ends such a pair (it emits no instruction).
__device__ __forceinline__ float obs_single(float x) {
  asm("" : "+v"(x));
  return x;
}

// (max, sum) of a softmax row merged with another part of the same row, exp2 domain.  Finite
// "nothing seen yet" maximum: exp2(kObsNone - kObsNone) is 1 and the sums it scales are 0.
constexpr float kObsNone = -1e30f;
__device__ __forceinline__ void obs_merge(float& m, float& s, float om, float os) {
  const float mm = fmaxf(m, om);
  const float a = obs_single(s * __builtin_amdgcn_exp2f(obs_single(m - mm)));
  const float b = obs_single(os * __builtin_amdgcn_exp2f(obs_single(om - mm)));
  s = obs_single(a + b);
  m = mm;
}

// PASS 1: statistics.  PASS 2: column sums.  NT: K with non-temporal loads.
template <int DT, int NC, int PASS, bool NT>
__global__ void __launch_bounds__(kObsThreads)
    observe_pass_kernel(const ObserveChunk T, const ObserveArgs A) {
  constexpr int ROWB = (NC + 1) * 16;                // padded LDS row (see the head of this file)
  constexpr int KS = NC / 2;                         // MFMA k-steps: 16 elements = two 16-B chunks
  constexpr int LPT = kObsTile * NC / kObsThreads;   // 16-B loads per thread and tile
  static_assert(NC == 8 || NC == 16 || NC == 32, "16-bit rows of D = 64 / 128 / 256");
  __shared__ __attribute__((aligned(16))) char tile[kObsTile * ROWB];
  __shared__ float lse[PASS == 2 ? kObsMaxM : 1];
  __shared__ float colp[PASS == 2 ? kObsWaves : 1][kObsTile];  // [query block][tile key]

  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l32 = lane & 31;
  const int wid = uni(tid >> 6);
  const int li = blockIdx.x / A.BH, row = blockIdx.x - li * A.BH;
  const kvc_layer_t* ly = &T.l[li];
  const kvc_observe_layer_t* ql = &T.q[li];
  if (!observe_scored(*ly, A.f32 != nullptr)) return;
  const int S = ly->seq_len, W = A.W, MB = A.MB;
  const int key0 = blockIdx.y * kObsChunk;
  if (key0 >= S) return;
  const int kend = min(S, key0 + kObsChunk);
  int t_first = 0, t_last = (kend - key0 + kObsTile - 1) / kObsTile;
  const int z0 = ly->zone_start, z1 = z0 + ly->zone_len;
  if constexpr (PASS == 2) {  // only the tiles that hold zone keys
    if (kend <= z0 || key0 >= z1) return;
    t_first = max(0, z0 - key0) / kObsTile;
    t_last = (min(kend, z1) - key0 + kObsTile - 1) / kObsTile;
  }
  const int b = row / A.H, h = row - b * A.H;
  const int64_t grow = (int64_t)ly->row0 + row;  // the row's index in workspace and scratch
  const char* kbase = static_cast<const char*>(ly->k) +
                      ((int64_t)b * ly->k_stride[0] + (int64_t)h * ly->k_stride[1]) * 2;
  const int64_t sbytes = ly->k_stride[2] * 2;

  // this wave's query block: A-operand fragments, row l32 of the block, chunk 2*kk + half
  const int mbk = wid % MB;
  uint4 qf[KS];
  {
    const int m = mbk * 32 + l32;
    const int g = m / W, i = m - g * W;
    const char* qrow = static_cast<const char*>(ql->q) +
                       ((int64_t)b * ql->q_stride[0] + (int64_t)(h * A.G + g) * ql->q_stride[1] +
                        (int64_t)i * ql->q_stride[2]) * 2;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
      qf[kk] = m < A.M ? *reinterpret_cast<const uint4*>(qrow + (2 * kk + half) * 16)
                       : make_uint4(0, 0, 0, 0);
  }

  float mx[16], sm[16];  // PASS 1: this lane's key columns, rows 8*(v/4) + 4*half + v%4
  float ls[16];          // PASS 2: lse of those rows
  if constexpr (PASS == 1) {
#pragma unroll
    for (int v = 0; v < 16; ++v) mx[v] = kObsNone, sm[v] = 0.f;
  } else {
    // lse_i of the row's M queries from the partials of every chunk and of the waves that hold
    // block i / 32 (w % MB == i / 32), in one fixed order
    if (tid < kObsMaxM) {
      float m = kObsNone, s = 0.f;
      const int mb = tid >> 5;
      if (mb < MB) {
        const int nch = (S + kObsChunk - 1) / kObsChunk;
        const float2* pr = A.part + grow * A.pstride * 32 + (tid & 31);
        for (int c = 0; c < nch; ++c)
          for (int w = mb; w < kObsWaves; w += MB) {
            const float2 x = pr[(int64_t)(c * kObsWaves + w) * 32];
            obs_merge(m, s, x.x, x.y);
          }
      }
      // rows past M (the zero rows of a half-filled block) never count: exp2(s - inf) = 0
      lse[tid] = tid < A.M ? m + __builtin_log2f(s) : __builtin_inff();
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < 16; ++v) ls[v] = lse[mbk * 32 + 8 * (v >> 2) + 4 * half + (v & 3)];
  }

  // one tile: thread q = it * 256 + tid moves chunk q % NC of key row q / NC
  uint4 stage[LPT];
  const auto load_tile = [&](int t) {
#pragma unroll
    for (int it = 0; it < LPT; ++it) {
      const int q = it * kObsThreads + tid;
      const int key = key0 + t * kObsTile + q / NC;
      const char* src = kbase + (int64_t)key * sbytes + (q % NC) * 16;
      if (key < S) {  // never past row S - 1
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 w = NT ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src))
                           : *reinterpret_cast<const u32x4*>(src);
        stage[it] = make_uint4(w.x, w.y, w.z, w.w);
      } else {
        stage[it] = make_uint4(0, 0, 0, 0);
      }
    }
  };
  load_tile(t_first);
  for (int t = t_first; t < t_last; ++t) {
#pragma unroll
    for (int it = 0; it < LPT; ++it) {
      const int q = it * kObsThreads + tid;
      *reinterpret_cast<uint4*>(tile + (q / NC) * ROWB + (q % NC) * 16) = stage[it];
    }
    __syncthreads();
    if (t + 1 < t_last) load_tile(t + 1);  // in flight while this tile is multiplied
    const int tkey = key0 + t * kObsTile;
    // the causal mask (and the keys past S - 1, which it covers: S - W + i <= S - 1) touches
    // only tiles that reach into the last W keys
    const bool masked = tkey + kObsTile > S - W;  // uniform
    for (int it = 0; it < MB; ++it) {
      const int sub = wid / MB + it * (kObsWaves / MB);
      const char* brow = tile + (sub * 32 + l32) * ROWB + half * 16;
      f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KS; ++kk)
        acc = obs_mfma<DT>(qf[kk], *reinterpret_cast<const uint4*>(brow + kk * 32), acc);
      const int key = tkey + sub * 32 + l32;  // this lane's column
      float col = 0.f;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        float s = obs_single(acc[v] * A.scale2);
        bool ok = true;
        if (masked) {
          const int i = (mbk * 32 + 8 * (v >> 2) + 4 * half + (v & 3)) & (W - 1);
          ok = key <= S - W + i;
        }
        if constexpr (PASS == 1) {
          // online (max, sum) with one exp2: of the two rescale factors one is always 1
          s = ok ? s : -__builtin_inff();
          const float d = obs_single(s - mx[v]);
          const float e = __builtin_amdgcn_exp2f(-__builtin_fabsf(d));
          const float grown = obs_single(__builtin_fmaf(sm[v], e, 1.f));
          const float same = obs_single(sm[v] + e);
          sm[v] = d > 0.f ? grown : same;
          mx[v] = fmaxf(mx[v], s);
        } else {
          const float p = __builtin_amdgcn_exp2f(obs_single(s - ls[v]));
          col = col + (ok ? p : 0.f);
        }
      }
      if constexpr (PASS == 2) {
        col = col + __shfl_xor(col, 32, 64);  // the other 16 query rows of the block
        if (half == 0) colp[mbk][sub * 32 + l32] = col;
      }
    }
    if constexpr (PASS == 2) {
      __syncthreads();
      if (tid < kObsTile) {  // the query blocks in order: a fixed sum
        float imp = colp[0][tid];
        for (int mb = 1; mb < MB; ++mb) imp = imp + colp[mb][tid];
        const int zc = tkey + tid - z0;
        if (zc >= 0 && zc < ly->zone_len) A.imp[grow * A.istride + zc] = imp;
      }
    }
    __syncthreads();  // the tile (and colp) are read: the next one may be stored
  }

  if constexpr (PASS == 1) {
    // the 32 lanes of a half hold the same 16 rows over different keys
#pragma unroll
    for (int v = 0; v < 16; ++v)
#pragma unroll
      for (int o = 1; o < 32; o <<= 1)
        obs_merge(mx[v], sm[v], __shfl_xor(mx[v], o, 64), __shfl_xor(sm[v], o, 64));
    if (l32 == 0) {
      float2* pr = A.part + (grow * A.pstride + (int64_t)blockIdx.y * kObsWaves + wid) * 32;
#pragma unroll
      for (int v = 0; v < 16; ++v) pr[8 * (v >> 2) + 4 * half + (v & 3)] = make_float2(mx[v], sm[v]);
    }
  }
}

// score[j] = pool(imp)[j] inside the zone -> the norm region (rounded to DT) and, optionally, the
// caller's fp32 rows.  avg: the window sum in position order over P, zero padding counted; max:
// the window maximum (padding never wins).  grid (rows, blocks of 256 zone columns).
template <int DT>
__global__ void __launch_bounds__(kPoolThreads)
    observe_pool_kernel(const ObserveChunk T, const ObserveArgs A) {
  const int li = blockIdx.x / A.BH, row = blockIdx.x - li * A.BH;
  const kvc_layer_t* ly = &T.l[li];
  if (!observe_scored(*ly, A.f32 != nullptr)) return;
  const int zl = ly->zone_len, col = blockIdx.y * kPoolThreads + threadIdx.x;
  if (col >= zl) return;
  const int64_t grow = (int64_t)ly->row0 + row;
  const float* imp = A.imp + grow * A.istride;
  const int r = A.pool >> 1;
  float acc = A.pool_max ? -__builtin_inff() : 0.f;
  for (int d = -r; d <= r; ++d) {
    const int c = col + d;
    if (c < 0 || c >= zl) continue;
    acc = A.pool_max ? fmaxf(acc, imp[c]) : acc + imp[c];
  }
  const float score = A.pool_max ? acc : acc / (float)A.pool;
  if (layer_selects(*ly))
    reinterpret_cast<uint16_t*>(A.norms)[grow * A.nstride + col] = (uint16_t)bits16_dt<DT>(score);
  if (A.f32) A.f32[grow * A.fstride + col] = score;
}

}  // namespace kvc
