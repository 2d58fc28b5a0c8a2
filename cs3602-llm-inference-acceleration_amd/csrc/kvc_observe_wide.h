// kvc_observe_wide.h -- observation-window scores of wide query groups: every G in [1, 16] with
// M = G * W <= 256, i.e. MB = 1 .. 8 blocks of 32 query rows (kvc_observe_score_paged; the shapes
// observe_pass_kernel / observe_src_kernel serve -- G a power of two, MB in {1, 2, 4} -- keep
// running those kernels).  The arithmetic, the K tile path (128-key tiles of a 1 024-key chunk, the
// next tile in flight, LDS rows of (NC + 1) * 16 bytes read as B operands) and the three loaders
// are those of kvc_observe.h / kvc_observe_src.h; what differs is who owns what.
//
// Ownership.  A K tile is fetched and staged ONCE per workgroup, whatever MB is.  Still 4 waves:
//   MB >= 3  wave w owns query blocks w and w + 4 (where they exist) and all four 32-key sub-tiles
//            of the tile.  A B fragment is read from LDS once per (sub-tile, k-step) and multiplied
//            into both owned blocks' accumulators: the LDS reads per tile are those of the old
//            MB = 4 schedule, with up to twice the MFMA and exp work behind each.  MB = 5 .. 7 is
//            uneven (waves below MB - 4 own two blocks, the others one); MB = 3 leaves wave 3 to
//            load and stage only.
//   MB <= 2  (G = 3 at W = 16) the old split: wave w owns block w % MB and the sub-tiles
//            w / MB + i * (4 / MB).
// Pass 1 keeps 32 VGPRs of (max, sum) per owned block and lane for the whole chunk, beside that
// block's Q fragments (KS * 4 VGPRs); the accumulators of the two blocks are live together only
// across one sub-tile's MFMA chain.
//
// Statistics scratch: 8 slots of 32 (max, sum) per (row, chunk).  MB >= 3: slot = block (written by
// wave block % 4); MB <= 2: slot = wave, block = slot % MB.  Slots nobody owns are neither written
// nor read.  Pass 2 merges a row's slots chunk by chunk in slot order, then sums the blocks'
// column partials (colp) in block order: no atomics, one fixed order, the same bits every call.
#pragma once

#include "kvc_observe_src.h"

namespace kvc {

constexpr int kObsWideMaxM = 256;   // G * W
constexpr int kObsWideBlocks = 8;   // query blocks, and statistics slots per (row, chunk)

// Whether a (G, MB) call runs these kernels and not the 4-block schedule of kvc_observe.h.
__host__ __device__ __forceinline__ bool observe_wide(int G, int MB) {
  return (G & (G - 1)) != 0 || (MB != 1 && MB != 2 && MB != 4);
}

// PASS 1: statistics.  PASS 2: column sums.  NT: K with non-temporal loads.  DT: K's dtype (Q and
// the MFMA are score_dt(DT)).  NC: 16-B chunks of an LDS row.  PAGED: K rows through G's block
// tables (otherwise G is not read).  A.pstride counts kObsWideBlocks slots per chunk.
// Two workgroups per CU (<= 256 VGPRs) where that fits without scratch -- D = 64, and pass 2 at
// D = 128: a second wave per SIMD runs the softmax's VALU work under the first one's MFMA, LDS and
// load waits.  Pass 1 at D = 128 asked for two spilled 20 - 116 bytes (two blocks of Q fragments,
// statistics and accumulators are 192 VGPRs before the staging registers), also with the two
// blocks multiplied one after the other; at D = 256 the Q fragments alone are 128 VGPRs.
template <int DT, int NC, int PASS, bool NT, bool PAGED>
__global__ void __launch_bounds__(kObsThreads, (NC == 8 || (NC == 16 && PASS == 2)) ? 2 : 1)
    observe_wide_kernel(const ObserveChunk T, const ObservePages G, const ObserveArgs A,
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
  __shared__ float lse[PASS == 2 ? kObsWideMaxM : 1];
  __shared__ float colp[PASS == 2 ? kObsWideBlocks : 1][kObsTile];  // [query block][tile key]
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

  // this wave's items (all wave-uniform): NB owned blocks blk[j], sub-tiles sub0 + i * sstep
  const bool shared = MB <= 2;                          // waves share a block, split its sub-tiles
  const int nb = shared ? 1 : (wid < MB) + (wid + 4 < MB);
  const int blk[2] = {shared ? wid % MB : wid, wid + 4};
  const int sub0 = shared ? wid / MB : 0, sstep = shared ? kObsWaves / MB : 1;
  const int nsub = nb == 0 ? 0 : (shared ? MB : 4);

  // A-operand fragments of the owned blocks: row l32 of the block, chunk 2*kk + half
  uint4 qf[2][KS];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = blk[j] * 32 + l32;
    const bool live = j < nb && m < A.M;  // zero rows: past M, and a block this wave does not own
    const int g = live ? m / W : 0, i = live ? m - g * W : 0;
    const char* qrow = static_cast<const char*>(ql->q) +
                       ((int64_t)b * ql->q_stride[0] + (int64_t)(h * A.G + g) * ql->q_stride[1] +
                        (int64_t)i * ql->q_stride[2]) * 2;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
      qf[j][kk] = live ? *reinterpret_cast<const uint4*>(qrow + (2 * kk + half) * 16)
                       : make_uint4(0, 0, 0, 0);
  }

  float mx[2][16], sm[2][16];  // PASS 1: this lane's key columns, rows 8*(v/4) + 4*half + v%4
  float ls[2][16];             // PASS 2: lse of those rows
  if constexpr (PASS == 1) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v) mx[j][v] = kObsNone, sm[j][v] = 0.f;
  } else {
    // lse_i of the row's M queries from the slots of every chunk that hold block i / 32, in one
    // fixed order: chunk by chunk, slot by slot
    {
      float m = kObsNone, s = 0.f;
      const int mb = tid >> 5;  // kObsThreads == kObsWideMaxM: one query row per thread
      if (mb < MB) {
        const int nch = (S + kObsChunk - 1) / kObsChunk;
        const float2* pr = A.part + grow * A.pstride * 32 + (tid & 31);
        const int s_end = shared ? kObsWaves : mb + 1, s_step = shared ? MB : 1;
        for (int c = 0; c < nch; ++c)
          for (int sl = mb; sl < s_end; sl += s_step) {
            const float2 x = pr[(int64_t)(c * kObsWideBlocks + sl) * 32];
            obs_merge(m, s, x.x, x.y);
          }
      }
      // rows past M (the zero rows of a half-filled block) never count: exp2(s - inf) = 0
      lse[tid] = tid < A.M ? m + __builtin_log2f(s) : __builtin_inff();
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v)
        ls[j][v] = j < nb ? lse[blk[j] * 32 + 8 * (v >> 2) + 4 * half + (v & 3)] : __builtin_inff();
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
    for (int it = 0; it < nsub; ++it) {
      const int sub = sub0 + it * sstep;
      const char* brow = tile + (sub * 32 + l32) * ROWB + half * 16;
      f32x16 acc[2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[j][v] = 0.f;
      if (nb == 2) {  // one B fragment, both owned blocks
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
          const uint4 bf = *reinterpret_cast<const uint4*>(brow + kk * 32);
          acc[0] = obs_mfma<MDT>(qf[0][kk], bf, acc[0]);
          acc[1] = obs_mfma<MDT>(qf[1][kk], bf, acc[1]);
        }
      } else {
#pragma unroll
        for (int kk = 0; kk < KS; ++kk)
          acc[0] = obs_mfma<MDT>(qf[0][kk], *reinterpret_cast<const uint4*>(brow + kk * 32), acc[0]);
      }
      const int key = tkey + sub * 32 + l32;  // this lane's column
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (j < nb) {
          float col = 0.f;
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            float s = obs_single(acc[j][v] * A.scale2);
            bool ok = true;
            if (masked) {
              const int i = (blk[j] * 32 + 8 * (v >> 2) + 4 * half + (v & 3)) & (W - 1);
              ok = key <= S - W + i;
            }
            if constexpr (PASS == 1) {
              // online (max, sum) with one exp2: of the two rescale factors one is always 1
              s = ok ? s : -__builtin_inff();
              const float d = obs_single(s - mx[j][v]);
              const float e = __builtin_amdgcn_exp2f(-__builtin_fabsf(d));
              const float grown = obs_single(__builtin_fmaf(sm[j][v], e, 1.f));
              const float same = obs_single(sm[j][v] + e);
              sm[j][v] = d > 0.f ? grown : same;
              mx[j][v] = fmaxf(mx[j][v], s);
            } else {
              const float p = __builtin_amdgcn_exp2f(obs_single(s - ls[j][v]));
              col = col + (ok ? p : 0.f);
            }
          }
          if constexpr (PASS == 2) {
            col = col + __shfl_xor(col, 32, 64);  // the other 16 query rows of the block
            if (half == 0) colp[blk[j]][sub * 32 + l32] = col;
          }
        }
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
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j < nb) {
        // the 32 lanes of a half hold the same 16 rows over different keys
#pragma unroll
        for (int v = 0; v < 16; ++v)
#pragma unroll
          for (int o = 1; o < 32; o <<= 1)
            obs_merge(mx[j][v], sm[j][v], __shfl_xor(mx[j][v], o, 64), __shfl_xor(sm[j][v], o, 64));
        if (l32 == 0) {
          const int slot = shared ? wid : blk[j];
          float2* pr = A.part +
                       (grow * A.pstride + (int64_t)blockIdx.y * kObsWideBlocks + slot) * 32;
#pragma unroll
          for (int v = 0; v < 16; ++v)
            pr[8 * (v >> 2) + 4 * half + (v & 3)] = make_float2(mx[j][v], sm[j][v]);
        }
      }
    }
  }
}

}  // namespace kvc
