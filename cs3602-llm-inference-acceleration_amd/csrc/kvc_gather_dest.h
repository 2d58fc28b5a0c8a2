// kvc_gather_dest.h -- GATHER into caller-provided destinations (kvc_launch_dest): strided
// k_out / v_out views, or the layer's own K / V compacted in place.  gather_passes is the pass
// schedule of every destination-aware copy: this file's dense kernel and kvc_paged.h's.
#pragma once

#include "kvc_gather.h"

namespace kvc {

// The destinations of a chunk's layers travel by value beside its LayerChunk (3.5 KiB).
struct DestChunk {
  kvc_dest_t d[kArgLayers];
};

constexpr int kDestIters = 4;  // 16-B units of K and of V per thread and pass
// output rows of one pass (one workgroup): 64 rows of 256 B, 32 of 512 B, 102 of 160 B
__host__ __device__ constexpr int dest_pass_rows(int nc) {
  return kGatherThreads * kDestIters / nc;
}

// Rows of one (b, h) sequence of a dense K and V -- a source or a destination:
// row s of K is at kb + s * kss.
struct DenseRows {
  char* kb;
  char* vb;
  int64_t kss, vss;
  // a bad index is reported where it is met, one atomicOr per unit (gather_block's form)
  static constexpr bool kFoldStatus = false;
  __device__ __forceinline__ DenseRows(int esz, const void* k, const void* v, const int64_t* ks,
                                       const int64_t* vs, int b, int h)
      : kb((char*)k + ((int64_t)b * ks[0] + (int64_t)h * ks[1]) * esz),
        vb((char*)v + ((int64_t)b * vs[0] + (int64_t)h * vs[1]) * esz),
        kss(ks[2] * esz),
        vss(vs[2] * esz) {}
  // addresses of row s; false: s has no valid address (never, here)
  __device__ __forceinline__ bool locate(int s, char** k, char** v) const {
    *k = kb + s * kss;
    *v = vb + s * vss;
    return true;
  }
};

// The destination of a kernel that decides per layer at run time: `a` if first, else `b`.
template <typename A, typename B>
struct EitherRows {
  bool first;
  const A& a;
  const B& b;
  __device__ __forceinline__ bool locate(int s, char** k, char** v) const {
    return first ? a.locate(s, k, v) : b.locate(s, k, v);
  }
};

// Copies output rows of one (layer, b, h) row: the rows gather_kernel would copy from the same
// index region (PART_ALL), read through `src` and written through `dst` (locate(): a row's K and
// V addresses; false for a row without a valid address -- its load is clamped by the policy, its
// store dropped, and KVC_DEV_INDEX_RANGE reported).
//
// grid = (rows, nby).  A layer that is NOT in place has no ordering constraint: block (row, by)
// copies the one pass of dest_pass_rows(NC) output rows from by * dest_pass_rows(NC) on, like
// gather_block.
//
// An IN-PLACE layer (destination == source) is copied by ONE workgroup per (layer, b, h) row --
// block (row, 0); the others return -- in passes of consecutive output rows, ascending.  Why one
// barrier per pass makes that a correct memmove:
//   * the row map is strictly increasing with src(t) >= t (in_place_row_map_ok, kvc.hip: the
//     plans refuse anything else; ascending indices are the index region's contract), so output
//     row t only ever overwrites a row that is the source of output rows <= t;
//   * within pass p every wave loads its units of K and V into registers, waits until those
//     loads have RETURNED (s_waitcnt vmcnt(0): a bare s_barrier does not wait for outstanding
//     global loads), meets the other waves at the barrier, and only then stores.  So no store of
//     pass p can land before a load of pass p -- of any wave -- has its data;
//   * the sources of pass p+1 lie strictly above every destination of passes <= p (src(t) >= t),
//     so its loads need no ordering against earlier stores; its stores follow its own barrier,
//     which every wave reaches only after its own loads of pass p (and p+1) have returned, so
//     they cannot overtake a load of an earlier pass either.
// The proof speaks about ROWS: from memory it needs only that different rows of one (b, h)
// sequence are different bytes (the layouts' own paragraphs: non-zero strides here, kvc_paged.h).
// Sink rows have src == dst and are not touched.  Rows [n_out, S) are never written.
//
// SC (per-token-scaled fp8 paged caches, include/kvc.h; Src and Dst give page_of() /
// scales_at()): a row's K and V scale words are PART OF THE ROW.  Thread j of the workgroup loads
// the two words of the source row src(t) of pass row t = t0 + j, as uint32, among the loads of the
// pass -- before its s_waitcnt vmcnt(0) and the barrier -- and stores them to the slots of row t
// after it.  So every step of the proof above reads unchanged with "row" meaning a row's D bytes
// of K, of V and its two scale words: the scale slot of row t is only ever overwritten by the
// pass that writes row t, whose loads -- of any wave, scale words included -- have returned; and
// distinct rows have distinct scale slots (kvc_plan_scaled: non-zero scale strides on every dim
// larger than 1, the table's distinct page ids).  A side whose scale is uniform or absent
// (nullptr from scales_at) moves nothing.  A dropped row store (bad destination page id) drops
// its scale stores with it.  All of it is behind `if constexpr (SC)`.
template <int DT, int NC, bool SC = false, typename Src, typename Dst>
__device__ __forceinline__ void gather_passes(const kvc_layer_t* ly, int r, int H, bool inplace,
                                              const Src& src, const Dst& dst,
                                              const int32_t* __restrict__ gidx,
                                              int64_t idx_stride, int shared, uint32_t* status) {
  constexpr int ROWS = dest_pass_rows(NC);
  const int n_out = ly->n_out, sink = ly->sink_len, nsel = ly->n_select;
  const int zone_len = ly->zone_len, zone_start = ly->zone_start, tail_start = ly->tail_start;
  int t_begin, t_end;
  if (inplace) {
    if (blockIdx.y != 0) return;
    t_begin = sink;
    t_end = n_out;
  } else {
    t_begin = (int)blockIdx.y * ROWS;
    t_end = min(n_out, t_begin + ROWS);
  }
  if (t_begin >= t_end) return;
  // index row of (layer, b, h); KVC_FLAG_SHARED_INDEX: (layer, b)'s row serves every head
  const int32_t* irow = gidx + (int64_t)((ly->row0 + r) / (shared ? H : 1)) * idx_stride;
  bool bad = false;  // Src::kFoldStatus: one report per thread, after the passes
  const auto report = [&](bool b) {
    if constexpr (Src::kFoldStatus)
      bad |= b;
    else if (b && status)
      atomicOr(status, (uint32_t)KVC_DEV_INDEX_RANGE);
  };
  for (int t0 = t_begin; t0 < t_end; t0 += ROWS) {  // ascending passes
    const int nu = min(ROWS, t_end - t0) * NC;
    uint4 xk[kDestIters], xv[kDestIters];
    // SC: thread j < rows of the pass carries the two scale words of pass row j (its own index
    // and page lookups: two live registers per thread instead of two per unit, which keeps the
    // scaled instances at their twins' occupancy).  The row's units report a bad index or page id.
    // Its three dependent loads ride beside the units' own: the index with their indices, the
    // page id before their lookups, the scale words behind their K / V loads -- as a chain of its
    // own in front of them it cost the pass three more memory latencies.
    [[maybe_unused]] uint32_t wk = 0, wv = 0;
    [[maybe_unused]] const int trow = t0 + (int)threadIdx.x;
    [[maybe_unused]] const bool has_row = (int)threadIdx.x < ROWS && trow < t_end;
    [[maybe_unused]] int srow = trow, spage = 0;  // the row's source row and its clamped page id
    bool gat[kDestIters];
    int zi[kDestIters];
    // the index loads of all units are issued first.  (The compiler still waits for each unit's
    // index right before that unit's K / V loads -- one s_waitcnt vmcnt(0) per unit in the gfx950
    // ISA -- so the four units' K / V loads do not go out back to back: a known cost, not tuned.)
#pragma unroll
    for (int i = 0; i < kDestIters; ++i) {
      const int u = threadIdx.x + i * kGatherThreads;
      const int t = t0 + u / NC;
      gat[i] = u < nu && t >= sink && t < sink + nsel;
      zi[i] = gat[i] ? irow[t - sink] : 0;
    }
    if constexpr (SC) {
      static_assert(ROWS <= kGatherThreads, "one thread per row of a pass");
      if (has_row) {
        if (trow >= sink && trow < sink + nsel)
          srow = zone_start + min(max(irow[trow - sink], 0), zone_len - 1);
        else if (trow >= sink)
          srow = tail_start + (trow - sink - nsel);
        spage = src.page_of(srow);
      }
    }
#pragma unroll
    for (int i = 0; i < kDestIters; ++i) {
      const int u = threadIdx.x + i * kGatherThreads;
      if (u < nu) {
        const int t = t0 + u / NC, c = u - (u / NC) * NC;
        int s = t;  // sink rows; else zone[index], clamped (never read outside the zone); else tail
        if (gat[i]) {
          report(zi[i] < 0 || zi[i] >= zone_len);
          s = zone_start + min(max(zi[i], 0), zone_len - 1);
        } else if (t >= sink) {
          s = tail_start + (t - sink - nsel);
        }
        char* ks;
        char* vs;
        report(!src.locate(s, &ks, &vs));  // one lookup per (lane, row): K and V share it
        xk[i] = *reinterpret_cast<const uint4*>(ks + c * 16);
        xv[i] = *reinterpret_cast<const uint4*>(vs + c * 16);
      }
    }
    if constexpr (SC) {
      if (has_row) {
        uint32_t* sk;
        uint32_t* sv;
        src.scales_at(spage, srow, &sk, &sv);
        if (sk) wk = *sk;
        if (sv) wv = *sv;
      }
    }
    if (inplace) {  // uniform over the workgroup
      // every load of this pass has returned in this wave, then in all waves, before any store
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    if constexpr (SC) {
      if (has_row) {
        uint32_t* sk;
        uint32_t* sv;
        bool ok;
        dst.scales_at(dst.page_of(trow, &ok), trow, &sk, &sv);
        if (ok) {  // dropped with the row's stores otherwise
          if (sk) __builtin_nontemporal_store(wk, sk);
          if (sv) __builtin_nontemporal_store(wv, sv);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kDestIters; ++i) {
      const int u = threadIdx.x + i * kGatherThreads;
      if (u < nu) {
        const int t = t0 + u / NC, c = u - (u / NC) * NC;
        char* kd;
        char* vd;
        const bool ok = dst.locate(t, &kd, &vd);
        report(!ok);
        uint4 a = xk[i], q = xv[i];
        if (gat[i]) {  // torch.gather's NaN rewrite (gathered segment only)
          a = canon_nan_dt<DT>(a);
          q = canon_nan_dt<DT>(q);
        }
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        if (ok) {  // written once: non-temporal
          __builtin_nontemporal_store(u32x4{a.x, a.y, a.z, a.w},
                                      reinterpret_cast<u32x4*>(kd + c * 16));
          __builtin_nontemporal_store(u32x4{q.x, q.y, q.z, q.w},
                                      reinterpret_cast<u32x4*>(vd + c * 16));
        }
      }
    }
  }
  if constexpr (Src::kFoldStatus) {
    if (bad && status) atomicOr(status, (uint32_t)KVC_DEV_INDEX_RANGE);
  }
}

// Dense sources by their strides, into b * os0 + h * os1 + t * os2 of the layer's kvc_dest_t; in
// place, that is the source itself (kvc_plan_dest: same pointers and strides, none of them zero).
template <int DT, int NC>
__global__ void __launch_bounds__(kGatherThreads)
    gather_dest_kernel(const LayerChunk T, const DestChunk Dd, int H, int BH,
                       const int32_t* __restrict__ gidx, int64_t idx_stride, int shared,
                       uint32_t* status) {
  const int li = (int)blockIdx.x / BH;
  const kvc_layer_t* ly = T.l + li;
  const kvc_dest_t* de = Dd.d + li;
  const int r = (int)blockIdx.x - li * BH;
  const int b = r / H, h = r - (r / H) * H;
  constexpr int ESZ = DTypeTraits<DT>::esz;
  const DenseRows src(ESZ, ly->k, ly->v, ly->k_stride, ly->v_stride, b, h);
  const DenseRows dst(ESZ, ly->k_out, ly->v_out, de->k_stride, de->v_stride, b, h);
  gather_passes<DT, NC>(ly, r, H, de->in_place != 0, src, dst, gidx, idx_stride, shared, status);
}

}  // namespace kvc
