// kvc_observe_src.h -- observation-window scores of paged and fp8 keys (kvc_observe_score_paged).
// observe_src_kernel is observe_pass_kernel (kvc_observe.h: the work split, the MFMA schedule, the
// statistics, the partial layout and the pass-2 combine are described there) with two compile-time
// switches that touch nothing but how a K tile reaches LDS.  The body is a COPY of the dense one,
// deliberately: as one shared body the dense 16-bit pass-2 instances came out 1 - 5 instructions
// longer and pass 1 reordered.  A fix to one is a fix to both.  The pooling kernel is shared.
//   PAGED  K rows behind a block table (kvc_pages_t).  A workgroup's chunk starts at a multiple of
//          1 024 keys and P is a power of two, so the chunk meets max(1, 1024 / P) consecutive table
//          entries, all below ceil(S / P).  They are loaded ONCE per workgroup with coalesced loads,
//          clamped (one KVC_DEV_INDEX_RANGE OR per workgroup) and kept in LDS (4 KiB at P = 1);
//          load_tile takes a unit's page from there, and ONE page id per tile when P >= 128 (a
//          128-key tile then lies inside one page).  No table entry at or past ceil(S / P) is read.
//   fp8    K rows of D bytes (e4m3fn / e5m2): half the 16-B loads and staging registers per tile.
//          Each staged chunk is widened to sixteen bf16 values on its way to LDS (the packed OCP
//          converts, then a truncating pack: every fp8 value is exact in bf16) and stored as two
//          16-B LDS chunks.  The LDS tile, the B-operand reads and the bf16 MFMA are those of the
//          bf16 call on K.to(bf16), and so are the scores' bits.
#pragma once

#include "kvc_observe.h"

namespace kvc {

// sixteen fp8 values (one 16-B chunk of a K row) -> sixteen bf16: two 16-B LDS chunks.  The
// convert is exact and every fp8 value fits bf16's 8 significand bits, so keeping the high half of
// the fp32 pattern IS the bf16 upcast.
template <int DT>
__device__ __forceinline__ void obs_widen(const uint4 x, uint4& lo, uint4& hi) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const uint32_t w[4] = {x.x, x.y, x.z, x.w};
  uint32_t o[8];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f32x2 f[2];  // elements 4q, 4q+1 (the low 16 bits) and 4q+2, 4q+3
    if constexpr (DT == KVC_F8E4M3) {
      f[0] = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[q], false);
      f[1] = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[q], true);
    } else {
      f[0] = __builtin_amdgcn_cvt_pk_f32_bf8((int)w[q], false);
      f[1] = __builtin_amdgcn_cvt_pk_f32_bf8((int)w[q], true);
    }
#pragma unroll
    for (int hw = 0; hw < 2; ++hw) {
      // (scalars first: a bit cast straight from a vector element read element 0 for both)
      const float a = f[hw].x, b = f[hw].y;
      o[2 * q + hw] = (__float_as_uint(a) >> 16) | (__float_as_uint(b) & 0xffff0000u);
    }
  }
  lo = make_uint4(o[0], o[1], o[2], o[3]);
  hi = make_uint4(o[4], o[5], o[6], o[7]);
}

// The page tables of a chunk's layers, by value beside its ObserveChunk (1.5 KiB: 7.2 KiB of
// kernel arguments in all, below the 7.5 KiB PagesChunk that the paged launches are known to run
// with -- so the chunk stays kObsLayers = 32 layers).
struct ObservePages {
  kvc_pages_t p[kObsLayers];
};

// PASS 1: statistics.  PASS 2: column sums.  NT: K with non-temporal loads.  DT: K's dtype (Q and
// the MFMA are score_dt(DT): bf16 for fp8 keys).  NC: 16-B chunks of an LDS row (D * 2 / 16).
// PAGED: K rows through G's block tables (dense fp8 K: G is not read).  See the head of this file.
// fp8 pass 1 at D = 128 came out at 172 registers, four past the 168 of the dense instance's three
// waves per SIMD; asked for three, it takes 162 and still no scratch.
template <int DT, int NC, int PASS, bool NT, bool PAGED>
__global__ void __launch_bounds__(kObsThreads, (is_fp8(DT) && NC == 16 && PASS == 1) ? 3 : 1)
    observe_src_kernel(const ObserveChunk T, const ObservePages G, const ObserveArgs A,
                       uint32_t* status) {
  constexpr bool F8 = is_fp8(DT);
  constexpr int MDT = score_dt(DT);                  // the MFMA's (and Q's) dtype
  constexpr int ESZ = F8 ? 1 : 2;
  constexpr int NCG = F8 ? NC / 2 : NC;              // 16-B chunks of a K row in memory
  constexpr int ROWB = (NC + 1) * 16;                // padded LDS row (kvc_observe.h)
  constexpr int KS = NC / 2;                         // MFMA k-steps: 16 elements = two 16-B chunks
  constexpr int LPT = kObsTile * NCG / kObsThreads;  // 16-B loads per thread and tile
  static_assert(NC == 8 || NC == 16 || NC == 32, "rows of D = 64 / 128 / 256");
  __shared__ __attribute__((aligned(16))) char tile[kObsTile * ROWB];
  __shared__ float lse[PASS == 2 ? kObsMaxM : 1];
  __shared__ float colp[PASS == 2 ? kObsWaves : 1][kObsTile];  // [query block][tile key]
  __shared__ int pgid[PAGED ? kObsChunk : 1];  // clamped page ids of the chunk's table entries

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
  // (paged: the table is the batch dim, k_stride[0] is 0)
  const char* kbase = static_cast<const char*>(ly->k) +
                      ((int64_t)b * ly->k_stride[0] + (int64_t)h * ly->k_stride[1]) * ESZ;
  const int64_t sbytes = ly->k_stride[2] * ESZ;
  int lg = 0, pmask = 0;
  int64_t pbytes = 0;
  if constexpr (PAGED) {
    // the chunk's table entries [key0 >> lg, (kend - 1) >> lg]: at most kObsChunk >> lg of them,
    // every one below ceil(S / P)
    const kvc_pages_t* pg = &G.p[li];
    lg = 31 - __builtin_clz((unsigned)pg->page_size), pmask = pg->page_size - 1;
    pbytes = pg->k_page_stride * ESZ;
    const int32_t* tab = pg->block_table + (int64_t)b * pg->table_stride + (key0 >> lg);
    const int ne = ((kend - 1) >> lg) - (key0 >> lg) + 1, np = pg->num_pages;
    int bad = 0;
    for (int i = tid; i < ne; i += kObsThreads) {
      const int id = tab[i];
      bad |= id < 0 || id >= np;
      pgid[i] = min(max(id, 0), np - 1);
    }
    bad = __syncthreads_or(bad);  // (and pgid is staged)
    if (bad && tid == 0 && status) atomicOr(status, (uint32_t)KVC_DEV_INDEX_RANGE);
  }

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

  // one tile: thread q = it * 256 + tid moves chunk q % NCG of key row q / NCG
  uint4 stage[LPT];
  const auto load_tile = [&](int t) {
    int tpage = 0;  // PAGED, P >= 128: the tile's one page (its first key is below S)
    if constexpr (PAGED) tpage = lg >= 7 ? pgid[(t * kObsTile) >> lg] : 0;
#pragma unroll
    for (int it = 0; it < LPT; ++it) {
      const int q = it * kObsThreads + tid;
      const int key = key0 + t * kObsTile + q / NCG;
      const char* src = kbase + (int64_t)key * sbytes + (q % NCG) * 16;
      if constexpr (PAGED) {
        const int id = lg >= 7 ? tpage : (key < S ? pgid[(key - key0) >> lg] : 0);
        src = kbase + (int64_t)id * pbytes + (int64_t)(key & pmask) * sbytes + (q % NCG) * 16;
      }
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
      if constexpr (F8) {
        uint4 lo, hi;
        obs_widen<DT>(stage[it], lo, hi);
        char* dst = tile + (q / NCG) * ROWB + (q % NCG) * 32;
        *reinterpret_cast<uint4*>(dst) = lo;
        *reinterpret_cast<uint4*>(dst + 16) = hi;
      } else {
        *reinterpret_cast<uint4*>(tile + (q / NC) * ROWB + (q % NC) * 16) = stage[it];
      }
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
        acc = obs_mfma<MDT>(qf[kk], *reinterpret_cast<const uint4*>(brow + kk * 32), acc);
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

}  // namespace kvc
