// kvc_colsum.h -- causal attention column sums (H2O scores without an attention tensor):
// imp[b, hq, j] = sum_i softmax_j(scale * Q_i . K_j over j <= L - q + i), for the last q query
// positions of a layer, 1 <= q <= L (kvc_colsum_score, include/kvc.h).  The q x L probabilities
// are never stored: K is read twice and the logits are recomputed, as in kvc_observe.h -- whose
// kernels hold every query row in ONE workgroup (at most 256 rows) and mask the last W keys only.
// Here q is unbounded, so the work is split over query blocks and key chunks, with a diagonal
// band of masked tiles:
//
//   colsum_stats_kernel  QUERY-stationary.  grid (b * hq rows, query blocks, key splits).  A
//                        workgroup keeps MB in {1, 2, 4} blocks of 32 query rows as the MFMA's A
//                        fragments in registers and streams its split's 128-key tiles through LDS
//                        (the observe kernels' tile: rows of D*2 + 16 bytes, ds_read_b128 B reads),
//                        up to the block's causal limit.  Per-lane online (max, sum), one exp2 per
//                        logit -> one partial per (row, block, split, wave, query) in scratch.
//                        Only tiles the diagonal crosses take the masked path (a wave-uniform
//                        test); a sub-tile above the diagonal is skipped.  The heaviest query
//                        blocks (the last ones: they see the most keys) get the lowest block ids.
//   colsum_lse_kernel    merges a query's partials in split order -> lse_i (log2 domain).
//   colsum_sum_kernel    KEY-stationary.  grid (b * kv-head rows, 128-key chunks).  Every wave holds
//                        32 keys x D as the MFMA's A operand in registers (64 VGPRs at D = 256) for
//                        the whole kernel; the queries that can see the chunk -- rows from
//                        max(0, key0 - (L - q)) on -- stream through LDS as B operands, 128 per
//                        tile, with their lse beside them.  A lane then owns ONE query column and
//                        16 key rows of a 32 x 32 logit block and adds exp2(s - lse_i) into 16
//                        per-key accumulators across all query tiles; the 32 lanes of a half are
//                        reduced by one butterfly when the chunk ends.  The G query heads of the
//                        KV head are walked inside the workgroup: K is read once for all of them.
//                        Chunk 0 sees every query and the last chunk few: chunks are blockIdx.y
//                        in key order, so the heavy ones are dispatched first.
//
// Every sum has one fixed order (per-lane sequences, butterflies, split order): no atomics.
// With a caller's lse (what a flash-attention forward returns) the first two kernels do not run.
#pragma once

#include "kvc_observe.h"  // obs_mfma, obs_merge, obs_single, the tile constants

namespace kvc {

constexpr int kColsumLayers = 32;      // layers per argument chunk (144 B of tables per layer)
constexpr int kColsumMaxSplits = 32;   // key splits of the statistics pass, per query block
constexpr int kColsumMinSplitTiles = 4;
constexpr int kColsumTargetWgs = 1024; // statistics workgroups a layer is split towards
constexpr int kLseThreads = 256;

// How the statistics pass splits one layer (host and device agree through this table).
struct ColsumSplit {
  int64_t lse_off;   // floats into the lse scratch: [b * hq rows][q]
  int64_t part_off;  // float2s into the partials: [rows][nqb][nsplit][4 waves][32]
  int mb, nqb;       // 32-row blocks per workgroup; workgroup blocks of 32 * mb query rows
  int nsplit, tps;   // key splits; 128-key tiles per split
};

struct ColsumChunk {
  kvc_colsum_layer_t l[kColsumLayers];
  ColsumSplit s[kColsumLayers];
};

struct ColsumArgs {
  int B, H, Hq, G;
  float scale2;   // scale * log2(e): the softmax runs on exp2
  float2* part;
  float* lse;     // log2 domain
};

// rows = batch * q_heads.  The splits depend on the layer's own shape only: a layer's sums do not
// change with the layers beside it in a call.
inline void colsum_split(int64_t rows, int q, int L, ColsumSplit* s) {
  s->mb = q <= 32 ? 1 : q <= 64 ? 2 : 4;
  s->nqb = (q + 32 * s->mb - 1) / (32 * s->mb);
  const int tiles = (L + kObsTile - 1) / kObsTile;
  int64_t want = (kColsumTargetWgs + rows * s->nqb - 1) / (rows * s->nqb);
  int cap = (tiles + kColsumMinSplitTiles - 1) / kColsumMinSplitTiles;
  cap = cap > kColsumMaxSplits ? kColsumMaxSplits : cap;
  want = want < 1 ? 1 : want > cap ? cap : want;
  s->tps = (tiles + (int)want - 1) / (int)want;
  s->nsplit = (tiles + s->tps - 1) / s->tps;
}

// 128 rows x NC 16-B chunks from global memory into staging registers (rows at or past `nrows`
// read nothing and give zeros), and from there into the padded LDS tile.
template <int NC, int LPT>
__device__ __forceinline__ void colsum_load(uint4 (&stage)[LPT], const char* base, int64_t rowb,
                                            int row0, int nrows, int tid) {
#pragma unroll
  for (int it = 0; it < LPT; ++it) {
    const int u = it * kObsThreads + tid;
    const int r = row0 + u / NC;
    stage[it] = r < nrows ? *reinterpret_cast<const uint4*>(base + (int64_t)r * rowb + (u % NC) * 16)
                          : make_uint4(0, 0, 0, 0);
  }
}
template <int NC, int LPT>
__device__ __forceinline__ void colsum_store(const uint4 (&stage)[LPT], char* tile, int tid) {
#pragma unroll
  for (int it = 0; it < LPT; ++it) {
    const int u = it * kObsThreads + tid;
    *reinterpret_cast<uint4*>(tile + (u / NC) * ((NC + 1) * 16) + (u % NC) * 16) = stage[it];
  }
}

template <int DT, int NC>
__global__ void __launch_bounds__(kObsThreads)
    colsum_stats_kernel(const ColsumChunk T, const ColsumArgs A) {
  constexpr int ROWB = (NC + 1) * 16, KS = NC / 2, LPT = kObsTile * NC / kObsThreads;
  static_assert(NC == 8 || NC == 10 || NC == 16 || NC == 32, "16-bit rows of D = 64/80/128/256");
  __shared__ __attribute__((aligned(16))) char tile[kObsTile * ROWB];

  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l32 = lane & 31;
  const int wid = uni(tid >> 6);
  const int BHq = A.B * A.Hq;
  const int li = blockIdx.x / BHq, row = blockIdx.x - li * BHq;
  const kvc_colsum_layer_t* ly = &T.l[li];
  const ColsumSplit* sp = &T.s[li];
  if (ly->lse) return;  // the caller's lse: no statistics
  if ((int)blockIdx.y >= sp->nqb || (int)blockIdx.z >= sp->nsplit) return;
  const int qb = sp->nqb - 1 - blockIdx.y, split = blockIdx.z, MB = sp->mb;
  const int L = ly->seq_len, q = ly->q_len, off = L - q;
  const int b = row / A.Hq, hq = row - b * A.Hq, h = hq / A.G;
  const char* kbase = static_cast<const char*>(ly->k) +
                      ((int64_t)b * ly->k_stride[0] + (int64_t)h * ly->k_stride[1]) * 2;
  const int64_t kbytes = ly->k_stride[2] * 2;

  // this wave's 32 query rows: A fragments, row l32 of the block, chunk 2*kk + half
  const int mbk = wid % MB;
  const int i0w = (qb * MB + mbk) * 32;
  uint4 qf[KS];
  {
    const int i = i0w + l32;
    const char* qrow = static_cast<const char*>(ly->q) +
                       ((int64_t)b * ly->q_stride[0] + (int64_t)hq * ly->q_stride[1] +
                        (int64_t)i * ly->q_stride[2]) * 2;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
      qf[kk] = i < q ? *reinterpret_cast<const uint4*>(qrow + (2 * kk + half) * 16)
                     : make_uint4(0, 0, 0, 0);
  }
  float mx[16], sm[16];  // rows 8*(v/4) + 4*half + v%4 of the block, over this lane's key columns
#pragma unroll
  for (int v = 0; v < 16; ++v) mx[v] = kObsNone, sm[v] = 0.f;

  // the split's tiles, up to the last key the block's last row sees (<= L - 1)
  const int klast = off + min(q - 1, (qb + 1) * MB * 32 - 1);
  const int t_first = split * sp->tps, t_last = min(t_first + sp->tps, klast / kObsTile + 1);
  uint4 stage[LPT];
  if (t_first < t_last) colsum_load<NC>(stage, kbase, kbytes, t_first * kObsTile, L, tid);
  for (int t = t_first; t < t_last; ++t) {
    colsum_store<NC>(stage, tile, tid);
    __syncthreads();
    if (t + 1 < t_last) colsum_load<NC>(stage, kbase, kbytes, (t + 1) * kObsTile, L, tid);
    const int tkey = t * kObsTile;
    for (int it = 0; it < MB; ++it) {
      const int sub = wid / MB + it * (kObsWaves / MB);
      const int skey = tkey + sub * 32;
      if (skey > off + i0w + 31) continue;          // above the diagonal: no row sees a key
      const bool masked = skey + 31 > off + i0w;    // the diagonal crosses (wave-uniform)
      const char* brow = tile + (sub * 32 + l32) * ROWB + half * 16;
      f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KS; ++kk)
        acc = obs_mfma<DT>(qf[kk], *reinterpret_cast<const uint4*>(brow + kk * 32), acc);
      const int key = skey + l32;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        float s = obs_single(acc[v] * A.scale2);
        if (masked) s = key <= off + i0w + 8 * (v >> 2) + 4 * half + (v & 3) ? s : -__builtin_inff();
        // online (max, sum) with one exp2: of the two rescale factors one is always 1
        const float d = obs_single(s - mx[v]);
        const float e = __builtin_amdgcn_exp2f(-__builtin_fabsf(d));
        const float grown = obs_single(__builtin_fmaf(sm[v], e, 1.f));
        const float same = obs_single(sm[v] + e);
        sm[v] = d > 0.f ? grown : same;
        mx[v] = fmaxf(mx[v], s);
      }
    }
    __syncthreads();  // the tile is read: the next one may be stored
  }
  // the 32 lanes of a half hold the same 16 rows over different keys
#pragma unroll
  for (int v = 0; v < 16; ++v)
#pragma unroll
    for (int o = 1; o < 32; o <<= 1)
      obs_merge(mx[v], sm[v], __shfl_xor(mx[v], o, 64), __shfl_xor(sm[v], o, 64));
  if (l32 == 0) {
    float2* pr = A.part + sp->part_off +
                 ((((int64_t)row * sp->nqb + qb) * sp->nsplit + split) * kObsWaves + wid) * 32;
#pragma unroll
    for (int v = 0; v < 16; ++v) pr[8 * (v >> 2) + 4 * half + (v & 3)] = make_float2(mx[v], sm[v]);
  }
}

// lse_i (log2 domain) of query row i: its partials over the splits, and over the waves that held
// its 32-row block (w % MB == block), in one fixed order.  grid (rows, blocks of 256 queries).
__global__ void __launch_bounds__(kLseThreads)
    colsum_lse_kernel(const ColsumChunk T, const ColsumArgs A) {
  const int BHq = A.B * A.Hq;
  const int li = blockIdx.x / BHq, row = blockIdx.x - li * BHq;
  const kvc_colsum_layer_t* ly = &T.l[li];
  const ColsumSplit* sp = &T.s[li];
  const int i = blockIdx.y * kLseThreads + threadIdx.x;
  if (ly->lse || i >= ly->q_len) return;
  const int MB = sp->mb, qb = i / (32 * MB), r = i - qb * 32 * MB;
  const float2* pr = A.part + sp->part_off +
                     ((int64_t)row * sp->nqb + qb) * sp->nsplit * kObsWaves * 32 + (r & 31);
  float m = kObsNone, s = 0.f;
  for (int c = 0; c < sp->nsplit; ++c)
    for (int w = r >> 5; w < kObsWaves; w += MB) {
      const float2 x = pr[(c * kObsWaves + w) * 32];
      obs_merge(m, s, x.x, x.y);
    }
  A.lse[sp->lse_off + (int64_t)row * ly->q_len + i] = m + __builtin_log2f(s);
}

template <int DT, int NC>
__global__ void __launch_bounds__(kObsThreads)
    colsum_sum_kernel(const ColsumChunk T, const ColsumArgs A) {
  constexpr int ROWB = (NC + 1) * 16, KS = NC / 2, LPT = kObsTile * NC / kObsThreads;
  __shared__ __attribute__((aligned(16))) char tile[kObsTile * ROWB];
  __shared__ float lse_t[kObsTile];

  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l32 = lane & 31;
  const int wid = uni(tid >> 6);
  const int BH = A.B * A.H;
  const int li = blockIdx.x / BH, row = blockIdx.x - li * BH;
  const kvc_colsum_layer_t* ly = &T.l[li];
  const int L = ly->seq_len, q = ly->q_len, off = L - q;
  const int key0 = blockIdx.y * kObsTile;
  if (key0 >= L) return;
  const int b = row / A.H, h = row - b * A.H;
  const int wkey0 = key0 + wid * 32;  // this wave's 32 keys

  // the wave's keys: A fragments, key row l32, chunk 2*kk + half; rows past L - 1 are zero rows
  // whose sums are not stored
  uint4 kf[KS];
  {
    const int key = wkey0 + l32;
    const char* krow = static_cast<const char*>(ly->k) +
                       ((int64_t)b * ly->k_stride[0] + (int64_t)h * ly->k_stride[1] +
                        (int64_t)key * ly->k_stride[2]) * 2;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
      kf[kk] = key < L ? *reinterpret_cast<const uint4*>(krow + (2 * kk + half) * 16)
                       : make_uint4(0, 0, 0, 0);
  }
  // the caller's lse is a natural logarithm, the statistics pass's a binary one
  const float* lse_all = ly->lse ? ly->lse : A.lse + T.s[li].lse_off;
  const float lse_mul = ly->lse ? 1.44269504088896340736f : 1.f;
  // query rows that see a key of the chunk: i >= key0 - off; whole 128-row tiles from there
  const int qt0 = max(0, key0 - off) / kObsTile * kObsTile;
  const int64_t qbytes = ly->q_stride[2] * 2;

  for (int g = 0; g < A.G; ++g) {
    const int hq = h * A.G + g;
    const int64_t orow = (int64_t)b * A.Hq + hq;
    const char* qbase = static_cast<const char*>(ly->q) +
                        ((int64_t)b * ly->q_stride[0] + (int64_t)hq * ly->q_stride[1]) * 2;
    const float* lse_row = lse_all + orow * q;
    float col[16];  // keys 8*(v/4) + 4*half + v%4 of the wave's 32, over this lane's query columns
#pragma unroll
    for (int v = 0; v < 16; ++v) col[v] = 0.f;

    uint4 stage[LPT];
    float lse_stage = 0.f;
    const auto load_tile = [&](int qt) {
      colsum_load<NC>(stage, qbase, qbytes, qt, q, tid);
      // rows past q - 1 (zero rows) never count: exp2(s - inf) = 0
      if (tid < kObsTile)
        lse_stage = qt + tid < q ? obs_single(lse_row[qt + tid] * lse_mul) : __builtin_inff();
    };
    load_tile(qt0);
    for (int qt = qt0; qt < q; qt += kObsTile) {
      colsum_store<NC>(stage, tile, tid);
      if (tid < kObsTile) lse_t[tid] = lse_stage;
      __syncthreads();
      if (qt + kObsTile < q) load_tile(qt + kObsTile);  // in flight while this tile is multiplied
      const int nsub = min(kObsTile, q - qt + 31) / 32;
      for (int sub = 0; sub < nsub; ++sub) {
        const int i0 = qt + sub * 32;
        if (wkey0 > off + i0 + 31) continue;        // below the diagonal: no query sees a key
        const bool masked = wkey0 + 31 > off + i0;  // the diagonal crosses (wave-uniform)
        const char* brow = tile + (sub * 32 + l32) * ROWB + half * 16;
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KS; ++kk)
          acc = obs_mfma<DT>(kf[kk], *reinterpret_cast<const uint4*>(brow + kk * 32), acc);
        const float ls = lse_t[sub * 32 + l32];
        const int vis = off + i0 + l32 - wkey0;  // the last of the wave's keys this query sees
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const float s = obs_single(acc[v] * A.scale2);
          const float p = __builtin_amdgcn_exp2f(obs_single(s - ls));
          const bool ok = !masked || 8 * (v >> 2) + 4 * half + (v & 3) <= vis;
          col[v] = col[v] + (ok ? p : 0.f);
        }
      }
      __syncthreads();  // the tile is read: the next one may be stored
    }
    // the 32 lanes of a half hold the same 16 keys over different queries
#pragma unroll
    for (int v = 0; v < 16; ++v)
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) col[v] = col[v] + __shfl_xor(col[v], o, 64);
    if (l32 == 0) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int key = wkey0 + 8 * (v >> 2) + 4 * half + (v & 3);
        if (key >= L) continue;
        const int64_t o = orow * ly->out_stride + key;
        if (ly->out_f32) ly->out_f32[o] = col[v];
        if (ly->out_dt) static_cast<uint16_t*>(ly->out_dt)[o] = (uint16_t)bits16_dt<DT>(col[v]);
      }
    }
  }
}

}  // namespace kvc
