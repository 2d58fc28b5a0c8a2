// kvc_gather.h -- GATHER and the fused SELECT_GATHER kernel.
#pragma once

#include "kvc_select.h"

namespace kvc {

// ---------------------------------------------------------------------------------------------
// GATHER
// ---------------------------------------------------------------------------------------------
// Output rows a GATHER launch copies (KVC_FLAG_GATHER_FIXED / _SELECTED): all, the sink and
// tail rows, or the selected rows -- as a count of "virtual" rows and the map to output rows.
enum { PART_ALL = 0, PART_FIXED = 1, PART_SELECTED = 2 };
__host__ __device__ __forceinline__ int part_rows(const kvc_layer_t& y, int part) {
  return part == PART_FIXED ? y.sink_len + y.tail_len
                            : part == PART_SELECTED ? y.n_select : y.sink_len + y.n_select +
                                                                       y.tail_len;
}
__device__ __forceinline__ int part_row(int v, int sink, int nsel, int part) {
  return part == PART_FIXED ? (v < sink ? v : v + nsel) : part == PART_SELECTED ? v + sink : v;
}

// One block of the copy: kGatherTokens output rows of K and V of workspace row `grow`
// (layer * BH + b * H + h), token block `by`.
template <int DT, int NC>
__device__ __forceinline__ void gather_block(const kvc_layer_t* __restrict__ L, int H, int BH,
                                             const int32_t* __restrict__ gidx,
                                             int64_t idx_stride, int shared, uint32_t* status,
                                             int part, int grow, int by) {
  constexpr int ESZ = DTypeTraits<DT>::esz;
  constexpr int ITERS = (kGatherTokens * NC + kGatherThreads - 1) / kGatherThreads;
  const kvc_layer_t* ly = L + grow / BH;
  const int r = grow - (grow / BH) * BH;
  const int n_out = ly->n_out;
  const int nv = part_rows(*ly, part);  // rows this launch copies
  const int t0 = by * kGatherTokens;
  if (t0 >= nv) return;
  const int nu = min(kGatherTokens, nv - t0) * NC;
  const int b = r / H, h = r - (r / H) * H;
  const int sink = ly->sink_len, nsel = ly->n_select;
  const char* kb = static_cast<const char*>(ly->k) +
                   ((int64_t)b * ly->k_stride[0] + (int64_t)h * ly->k_stride[1]) * ESZ;
  const char* vb = static_cast<const char*>(ly->v) +
                   ((int64_t)b * ly->v_stride[0] + (int64_t)h * ly->v_stride[1]) * ESZ;
  const int64_t kss = ly->k_stride[2] * ESZ, vss = ly->v_stride[2] * ESZ;
  // index row of (layer, b, h); KVC_FLAG_SHARED_INDEX: (layer, b)'s row serves every head
  const int32_t* irow = gidx + (int64_t)((ly->row0 + r) / (shared ? H : 1)) * idx_stride;
  const int64_t obase = (int64_t)r * n_out * NC * 16;
  char* ko = static_cast<char*>(ly->k_out) + obase;
  char* vo = static_cast<char*>(ly->v_out) + obase;
  uint4 xk[ITERS], xv[ITERS];
  bool gat[ITERS];
  int64_t oofs[ITERS];
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int u = threadIdx.x + i * kGatherThreads;
    gat[i] = false;
    oofs[i] = 0;
    if (u < nu) {
      const int t = part_row(t0 + u / NC, sink, nsel, part), c = u - (u / NC) * NC;
      oofs[i] = ((int64_t)t * NC + c) * 16;
      int src;
      if (t < sink) {
        src = t;
      } else if (t < sink + nsel) {
        int zi = irow[t - sink];
        if ((zi < 0 || zi >= ly->zone_len) && status)  // never read outside the zone: clamp
          atomicOr(status, (uint32_t)KVC_DEV_INDEX_RANGE);
        zi = min(max(zi, 0), ly->zone_len - 1);
        src = ly->zone_start + zi;
        gat[i] = true;
      } else {
        src = ly->tail_start + (t - sink - nsel);
      }
      xk[i] = *reinterpret_cast<const uint4*>(kb + src * kss + c * 16);
      xv[i] = *reinterpret_cast<const uint4*>(vb + src * vss + c * 16);
    }
  }
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int u = threadIdx.x + i * kGatherThreads;
    if (u < nu) {
      uint4 a = xk[i], bq = xv[i];
      if (gat[i]) {  // torch.gather's NaN rewrite (gathered segment only)
        a = canon_nan_dt<DT>(a);
        bq = canon_nan_dt<DT>(bq);
      }
      // written once: non-temporal
      typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
      __builtin_nontemporal_store(u32x4{a.x, a.y, a.z, a.w},
                                  reinterpret_cast<u32x4*>(ko + oofs[i]));
      __builtin_nontemporal_store(u32x4{bq.x, bq.y, bq.z, bq.w},
                                  reinterpret_cast<u32x4*>(vo + oofs[i]));
    }
  }
}

// grid = (rows, output-token blocks), one block each -- or, with loop_rows > 0, a capped 1-D grid
// whose blocks stride over the rows * nby blocks (the fixed rows of h2o_attention copied beside
// its heavy-hitter selection: a few resident workgroups per CU leave room for the selection's).
template <int DT, int NC>
__global__ void __launch_bounds__(kGatherThreads)
    gather_kernel(const LayerChunk T, int H, int BH, const int32_t* __restrict__ gidx,
                  int64_t idx_stride, int shared, uint32_t* status, int part, int loop_rows,
                  int nby) {
  if (loop_rows == 0) {
    gather_block<DT, NC>(T.l, H, BH, gidx, idx_stride, shared, status, part, blockIdx.x,
                         blockIdx.y);
    return;
  }
  const int nvb = loop_rows * nby;
  for (int vb = blockIdx.x; vb < nvb; vb += gridDim.x)
    gather_block<DT, NC>(T.l, H, BH, gidx, idx_stride, shared, status, part, vb % loop_rows,
                         vb / loop_rows);
}

// ---------------------------------------------------------------------------------------------
// Row copy shared by the select+gather kernel
// ---------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ bool layer_selects(const kvc_layer_t& y) {
  return y.n_select > 0 && y.n_select < y.zone_len;
}

// Copy one output row (sink ++ selected ++ tail) of K and V with the whole workgroup.
// sel: ascending zone-local kept indices in LDS, or nullptr when no selection ran.
// Thread tid copies 16-B chunk tid % NC of output tokens tid / NC + i * (NT / NC): the same
// coalesced units as a flat unit loop (consecutive threads, consecutive 16-B units) with the
// chunk and its address offsets fixed per thread; the last NT % NC threads idle.
// part: PART_ALL, or PART_SELECTED / PART_FIXED (the row's copy split between the selecting
// workgroup and a copy-only one, part_rows / part_row).
template <int DT, int NC, int NT = kSelThreads>
__device__ __forceinline__ void gather_row(const kvc_layer_t* __restrict__ ly, int r, int H,
                                           const uint16_t* sel, int part = PART_ALL) {
  constexpr int ESZ = DTypeTraits<DT>::esz;
  constexpr int BATCH = 4;
  constexpr int TPI = NT / NC;  // tokens per pass
  static_assert(TPI >= 1, "a row's chunks must fit the workgroup");
  const int tq = (int)threadIdx.x / NC, c = (int)threadIdx.x - tq * NC;
  if (tq >= TPI) return;
  const int n_out = ly->n_out;
  const int b = r / H, h = r - (r / H) * H;
  const int sink = ly->sink_len, nsel = ly->n_select;
  const int nv = part_rows(*ly, part);  // rows this workgroup copies
  const char* kb = static_cast<const char*>(ly->k) +
                   ((int64_t)b * ly->k_stride[0] + (int64_t)h * ly->k_stride[1]) * ESZ + c * 16;
  const char* vb = static_cast<const char*>(ly->v) +
                   ((int64_t)b * ly->v_stride[0] + (int64_t)h * ly->v_stride[1]) * ESZ + c * 16;
  const int64_t kss = ly->k_stride[2] * ESZ, vss = ly->v_stride[2] * ESZ;
  char* ko = static_cast<char*>(ly->k_out) + (int64_t)r * n_out * NC * 16 + c * 16;
  char* vo = static_cast<char*>(ly->v_out) + (int64_t)r * n_out * NC * 16 + c * 16;
  for (int tb = tq; tb < nv; tb += TPI * BATCH) {
    uint4 xk[BATCH], xv[BATCH];
    bool gat[BATCH];
#pragma unroll
    for (int i = 0; i < BATCH; ++i) {
      const int v = tb + i * TPI;
      const int t = part_row(v, sink, nsel, part);
      gat[i] = false;
      if (v < nv) {
        int src;
        if (t < sink) {
          src = t;
        } else if (t < sink + nsel) {
          int zi = sel ? (int)sel[t - sink] : t - sink;
          zi = min(max(zi, 0), ly->zone_len - 1);
          src = ly->zone_start + zi;
          gat[i] = true;
        } else {
          src = ly->tail_start + (t - sink - nsel);
        }
        // default cache policy: non-temporal kept-row loads measured 5 % slower
        // (profiles/r05_c_copy_policy_ab.jsonl)
        xk[i] = *reinterpret_cast<const uint4*>(kb + src * kss);
        xv[i] = *reinterpret_cast<const uint4*>(vb + src * vss);
      }
    }
#pragma unroll
    for (int i = 0; i < BATCH; ++i) {
      const int v = tb + i * TPI;
      const int t = part_row(v, sink, nsel, part);
      if (v < nv) {
        uint4 a = xk[i], q = xv[i];
        if (gat[i]) {
          a = canon_nan_dt<DT>(a);
          q = canon_nan_dt<DT>(q);
        }
        const int64_t off = (int64_t)t * (NC * 16);
        // written once: non-temporal (temporal stores measured 9 % slower, same profile)
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(u32x4{a.x, a.y, a.z, a.w}, reinterpret_cast<u32x4*>(ko + off));
        __builtin_nontemporal_store(u32x4{q.x, q.y, q.z, q.w}, reinterpret_cast<u32x4*>(vo + off));
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// SELECT + GATHER: one workgroup per (layer, b, h) row selects into LDS and copies the row's
// output (sink ++ selected ++ tail of K and V) straight from the LDS index list.  With two
// workgroups per CU, one row's copy (HBM-bound) overlaps the other's selection (LDS/issue-
// bound), and the index list never round-trips through global memory.  Layout and thread
// counts as select_kernel; rows without a selection only copy.
// ---------------------------------------------------------------------------------------------
// L0T: level 0 may keep its rank tables in the idx region (run_chain); the instance without that
// code runs launches where it does not pay (launch_chunk)
// F8: the rows are fp8 storage (either format: the copy does not interpret them)
template <int KC, int NT, int NC, bool STABLE = false, bool L0T = true, bool F8 = false>
__global__ void __launch_bounds__(NT, sel_waves_per_eu(KC, NT))
    select_gather_kernel(const LayerChunk T, int H, int BH, int dt, int order, int algo,
                         const char* __restrict__ norms, int64_t norm_stride, int wave_seg,
                         int n_cap, int cap, uint32_t* status, int split_rows,
                         const uint32_t* __restrict__ tmax) {
  typedef typename DTypeTraits<KC>::key_t KeyT;
  constexpr int ESZ = DTypeTraits<KC>::esz;
  constexpr int MAXN = NT == kSelThreads ? kZoneMax : NT * 16;
  __shared__ SelScalars<KeyT> sc;
  // split_rows > 0 (few rows: fewer than the CUs): workgroups [split_rows, 2 split_rows) copy the
  // sink / tail rows of row blockIdx - split_rows on otherwise idle CUs while the row's own
  // workgroup selects; the selecting workgroup then copies only the selected rows
  const bool copier = split_rows > 0 && (int)blockIdx.x >= split_rows;
  const int wg = copier ? (int)blockIdx.x - split_rows : (int)blockIdx.x;
  const kvc_layer_t* ly = T.l + wg / BH;
  const int r = wg % BH;
  if (ly->n_out == 0) return;
  const bool selects = layer_selects(*ly);
  if constexpr (NT == kSelThreads) {
    n_cap = kZoneMax;
    cap = kSelCapBig<KeyT>;
  }
  // The row copy runs in the STORAGE dtype: `dt` for 16- and 32-bit rows; fp8 rows (F8: NC chunks
  // of 16 one-byte elements, moved verbatim) select as bf16 -- dt is KVC_BF16 -- and copy as bytes.
  if (copier) {
    // a row over the selecting workgroup's capacity is flagged there and left wholly unwritten
    // (KVC_DEV_SELECT_BOUNDS): its sink / tail rows are not copied either
    if (selects && ly->zone_len <= MAXN && ly->zone_len <= n_cap) {
      if constexpr (F8) {
        gather_row<KVC_F8E4M3, NC, NT>(ly, r, H, nullptr, PART_FIXED);
      } else {
        with_dt<KC>(dt, [&](auto D) {
          gather_row<D.value, NC, NT>(ly, r, H, nullptr, PART_FIXED);
        });
      }
    }
    return;
  }
  const char* nrow = norms + (int64_t)(ly->row0 + r) * norm_stride * ESZ;
  char* arrays;
  if constexpr (NT == kSelThreads) {
    __shared__ __attribute__((aligned(16))) char smem[kSelBytesBig<KeyT>];
    arrays = smem;
  } else {
    extern __shared__ __attribute__((aligned(16))) char dsmem[];
    arrays = dsmem;
  }
  // the kept positions: over the key region, dead after the chain (the stable selection reads
  // its keys to the end: the idx region then)
  uint16_t* sel = reinterpret_cast<uint16_t*>(arrays + (STABLE ? (size_t)n_cap * sizeof(KeyT) : 0));
  if (selects) {
    const uint32_t* trow =
        tmax ? tmax + (int64_t)(ly->row0 + r) * (norm_stride / kTile) : nullptr;
    const bool ok = select_body<KC, true, MAXN, NT, false, STABLE, L0T>(
        ly, dt, order, algo, nrow, nullptr, sel, arrays, n_cap, cap, sc, wave_seg, nullptr, status,
        trow);
    if (!ok) return;  // flagged in *status; the row's output is left unwritten (the copier
                      // workgroup of a split row skips it too)
    __syncthreads();
  }
  if constexpr (F8) {
    gather_row<KVC_F8E4M3, NC, NT>(ly, r, H, selects ? sel : nullptr,
                                   split_rows > 0 && selects ? PART_SELECTED : PART_ALL);
  } else {
    with_dt<KC>(dt, [&](auto D) {
      gather_row<D.value, NC, NT>(ly, r, H, selects ? sel : nullptr,
                                  split_rows > 0 && selects ? PART_SELECTED : PART_ALL);
    });
  }
}

}  // namespace kvc
