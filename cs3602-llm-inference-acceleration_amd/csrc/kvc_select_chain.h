// kvc_select_chain.h -- the reference-exact selection's partition chain (p1_counts, p2_window0,
// partition_level, run_chain) and its sort / heap helpers.
#pragma once

#include "kvc_device_util.h"
#include "kvc_serial.h"

namespace kvc {

template <int NT>
__device__ __forceinline__ void group_sync() {
  if constexpr (NT == 64)
    wave_sync();
  else
    __syncthreads();
}

// The final insertion sort of a <= 64-element segment [lo, hi) (std::__insertion_sort /
// __unguarded_linear_insert: an element moves left only past strictly greater ones, i.e. a
// STABLE sort by key) computed by one wave in parallel: lane i holds element i and stores it at
// #{key_j < key_i} + #{j < i : key_j == key_i}.  Every lane reads its element before any lane
// of the wave stores (the ranks need all of them), so the in-place stores are race-free.
// Replaces a one-lane loop of dependent LDS accesses.  Call with all 64 lanes of one wave.
template <typename KeyT>
__device__ __forceinline__ void wave_stable_sort(KeyT* key, uint16_t* idx, int lo, int hi) {
  const int lane = threadIdx.x & 63;
  const int m = hi - lo;
  const bool own = lane < m;
  const uint32_t kk = own ? (uint32_t)key[lo + lane] : 0u;
  const uint16_t ii = own ? idx[lo + lane] : (uint16_t)0;
  int r = 0;
  for (int j = 0; j < m; ++j) {  // m is wave-uniform
    const uint32_t kj = (uint32_t)__builtin_amdgcn_readlane((int)kk, j);
    r += (kj < kk || (kj == kk && j < lane)) ? 1 : 0;
  }
  if (own) {
    key[lo + r] = (KeyT)kk;
    idx[lo + r] = ii;
  }
}

// std::__heap_select(first, first + middle, first + len) -- std::partial_sort's selection, which
// torch.topk uses when k * 64 <= n (aten TopKImpl.h) -- run by one wave: lane 0 builds the heap
// and performs every pop_heap exactly as libstdc++ does (kvc_serial.h), while the wave scans the
// candidates 64 at a time: element i enters iff key[i] < key[0] at its turn, and key[0] only
// decreases, so a ballot against the current top leaves exactly the elements the serial loop
// would pop, in index order (re-checked against the new top after each pop).  The scan of the
// n - middle elements no longer costs one dependent LDS round trip each.  For middle <= 64 (the
// h2o heavy hitters' 64) the heap itself lives in the wave's registers (RegHeap) and only its
// final slots are stored; otherwise lane 0 keeps it in LDS.  Call with all 64 lanes of one wave;
// the result is the first `middle` positions (positions >= middle are not part of it).
// The heap of a wave_heap_select with middle <= 64 held in registers: lane j owns heap slot j
// (key hk, index hi).  adjust() is std::__adjust_heap + std::__push_heap (kvc_serial.h
// adjust_heap) computed wave-parallel instead of level by level:
//   * the down phase moves the hole along the path of "chosen" children (the right child unless
//     it is strictly smaller than the left; a lone child at (len-2)/2 for even len) to a leaf,
//     every path node taking its chosen child's entry;
//   * the up phase moves the value back up while its parent is strictly smaller.  Path keys do
//     not increase with depth (heap order), so it stops at depth m = #{path nodes below `top`
//     with !(key < value)}, and its moves undo the down phase below m.
// Net effect: path depths 0..m-1 take their chosen child's entry, depth m takes the value, the
// rest of the heap is unchanged; m is one ballot.
// PACKED (16-bit keys and positions): slot j's entry is one word, key << 16 | index, so each
// pop permutes one register instead of two (the children's keys and indices travel together).
template <bool PACKED>
struct RegHeap {
  uint32_t hk;   // PACKED: key << 16 | index
  uint32_t hi;   // !PACKED: index
  uint64_t anc;  // this slot and its ancestors below the root, as lane bits (fixed per lane)
  int dep;       // this slot's depth
  __device__ __forceinline__ uint32_t key_of(uint32_t x) const { return PACKED ? x >> 16 : x; }
  __device__ __forceinline__ uint32_t k(int j) const {
    return key_of((uint32_t)__builtin_amdgcn_readlane((int)hk, j));
  }
  __device__ __forceinline__ uint32_t i(int j) const {
    const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)(PACKED ? hk : hi), j);
    return PACKED ? x & 0xFFFFu : x;
  }
  __device__ __forceinline__ void set(uint32_t key, uint32_t ix) {
    if constexpr (PACKED) hk = key << 16 | ix;
    else hk = key, hi = ix;
    int a = (int)(threadIdx.x & 63), d = 0;
    uint64_t m = 0;
#pragma unroll
    for (int st = 0; st < 6; ++st) {  // 64 slots: depth <= 6
      m |= a > 0 ? 1ull << a : 0ull;
      d += a > 0 ? 1 : 0;
      a = a > 0 ? (a - 1) >> 1 : 0;
    }
    anc = m;
    dep = d;
  }
  // std::__adjust_heap + std::__push_heap from slot `top` with value (vk, vi), wave-parallel.
  // The only serial chain is: sibling keys by DPP wave shifts -> "my parent chose me" bits ->
  // one ballot B -> the path (each lane: are all links from top down to it in B, one mask test
  // against its ancestor bits) -> m, one ballot.  Both children's entries are fetched with
  // ds_bpermute at the start, off that chain.  (Round 3: a readlane chase of the path and
  // bpermutes of the children's keys before it, ~630 cycles per pop in tools/heap_probe.hip.)
  __device__ __forceinline__ void adjust(int top, int len, uint32_t vk, uint32_t vi) {
    const int lane = (int)(threadIdx.x & 63);
    const int c1 = min(2 * lane + 1, 63), c2 = min(2 * lane + 2, 63);
    const uint32_t pl = (uint32_t)__builtin_amdgcn_ds_bpermute(c1 * 4, (int)hk);
    const uint32_t pr = (uint32_t)__builtin_amdgcn_ds_bpermute(c2 * 4, (int)hk);
    uint32_t il = 0, ir = 0;
    if constexpr (!PACKED) {
      il = (uint32_t)__builtin_amdgcn_ds_bpermute(c1 * 4, (int)hi);
      ir = (uint32_t)__builtin_amdgcn_ds_bpermute(c2 * 4, (int)hi);
    }
    const uint32_t key = key_of(hk);
    const uint32_t kn = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)key, 0x130, 0xF, 0xF, false);  // wave_shl:1: lane + 1
    const uint32_t kp = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)key, 0x138, 0xF, 0xF, false);  // wave_shr:1: lane - 1
    const int p = (lane - 1) >> 1;                              // parent of this lane
    // (bitwise, not short-circuit: && / || here compiled to exec-mask branches)
    const unsigned two = p < (len - 1) / 2 ? 1u : 0u;           // the parent has both children
    const unsigned lone = (len & 1) == 0 && p == (len - 2) / 2 ? 1u : 0u;  // only the left one
    const unsigned in = lane >= 1 && lane < len ? 1u : 0u;
    // the right child unless it is strictly smaller than the left (std::__adjust_heap)
    const unsigned cl = lone | (two & (kn < key ? 1u : 0u));   // left child (odd lane) chosen
    const unsigned cr = two & (key < kp ? 0u : 1u);             // right child (even lane) chosen
    const uint64_t B = __builtin_amdgcn_ballot_w64((in & ((lane & 1) ? cl : cr)) != 0u);
    // on the path from `top`: a descendant of top (or top) whose links below top are all in B
    uint64_t links = anc;
    int d = dep;
    bool desc = true;
    if (top != 0) {  // wave-uniform: make_heap's sift-downs
      const uint64_t at = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)anc, top) |
                          ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(anc >> 32), top) << 32);
      links = anc & ~at;
      d = dep - __builtin_amdgcn_readlane(dep, top);
      desc = (anc >> top) & 1ull;
    }
    const unsigned onpath = desc && (B & links) == links ? 1u : 0u;
    const int m = __popcll(__builtin_amdgcn_ballot_w64(
        (onpath & (d >= 1 ? 1u : 0u) & (key < vk ? 0u : 1u)) != 0u));
    const bool left = (B >> c1) & 1ull;  // this slot's chosen child (path slots above the leaf)
    const uint32_t ck = (uint32_t)vreg((int)(left ? pl : pr));
    const bool up = (onpath & (d < m ? 1u : 0u)) != 0u, here = (onpath & (d == m ? 1u : 0u)) != 0u;
    const uint32_t v = PACKED ? (vk << 16 | vi) : vk;
    hk = up ? ck : here ? v : hk;
    if constexpr (!PACKED) hi = up ? (uint32_t)vreg((int)(left ? il : ir)) : here ? vi : hi;
  }
};

// The register heap of wave_heap_select (middle <= 64), in two steps so that a block can build
// it in one wave while its other waves prefilter the candidates (heap_candidates):
// std::make_heap over the first `middle` slots ...
template <bool PK, typename K, typename I>
__device__ __forceinline__ void reg_heap_make(RegHeap<PK>& h, const K* key, const I* idx,
                                              int middle) {
  const int lane = threadIdx.x & 63;
  h.set(lane < middle ? (uint32_t)key[lane] : 0u, lane < middle ? (uint32_t)idx[lane] : 0u);
  if (middle >= 2)
    for (int parent = (middle - 2) / 2; parent >= 0; --parent)
      h.adjust(parent, middle, h.k(parent), h.i(parent));
}
// ... then the scan of positions [middle, len) -- or only the ascending candidate positions
// `cand[0..ncand)` -- with its pops, and the heap's slots stored to key / idx[0..middle).
template <bool PK, typename K, typename I>
__device__ __forceinline__ void reg_heap_scan(RegHeap<PK>& h, K* key, I* idx, int middle, int len,
                                              const uint16_t* cand, int ncand) {
  const int lane = threadIdx.x & 63;
  uint32_t top = h.k(0);
  // the scan, eight rows of 64 candidates per LDS round trip (the loads do not depend on the
  // heap; only the ballots and pops do).  idx[i] == i on entry (every caller), so a candidate's
  // index is its position.
  constexpr int R = 8;
  const int end = cand ? ncand : len, first = cand ? 0 : middle;
  for (int base = first; base < end; base += 64 * R) {
    uint32_t kq[R], pq[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int i = base + q * 64 + lane;
      pq[q] = cand ? (uint32_t)cand[min(i, end - 1)] : (uint32_t)i;
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int i = base + q * 64 + lane;
      kq[q] = i < end ? (uint32_t)key[pq[q]] : 0xFFFFFFFFu;
    }
    // lanes past the end hold ~0, never below top (16-bit keys are below 2^16); the rows'
    // ballots against the current top first: most groups late in the row hold no candidate
    uint64_t cm[R], any = 0;
#pragma unroll
    for (int q = 0; q < R; ++q) {
      cm[q] = __builtin_amdgcn_ballot_w64(kq[q] < top);
      any |= cm[q];
    }
    if (!any) continue;
#pragma unroll
    for (int q = 0; q < R; ++q) {
      // top only decreases: a row's candidates against the current top are a subset of cm[q]
      uint64_t c = cm[q] & __builtin_amdgcn_ballot_w64(kq[q] < top);
      while (c) {
        const int l = (int)__builtin_ctzll(c);
        // std::__pop_heap(first, middle, i): the old top goes to position i (never read again:
        // only the heap's slots are the result), element i sifts in from the root
        h.adjust(0, middle, (uint32_t)__builtin_amdgcn_readlane((int)kq[q], l),
                 (uint32_t)__builtin_amdgcn_readlane((int)pq[q], l));
        top = h.k(0);
        c &= ~((2ull << l) - 1ull) & __builtin_amdgcn_ballot_w64(kq[q] < top);
      }
    }
  }
  if (lane < middle) {
    key[lane] = (K)h.key_of(h.hk);
    idx[lane] = (I)(PK ? (h.hk & 0xFFFFu) : h.hi);
  }
}

template <typename K, typename I>
__device__ __forceinline__ void wave_heap_select(K* key, I* idx, int middle, int len) {
  const int lane = threadIdx.x & 63;
  if (middle <= 64) {  // the heap in registers (RegHeap): make_heap, then the scan with its pops
    constexpr bool PK = sizeof(K) == 2 && sizeof(I) == 2;
    RegHeap<PK> h;
    reg_heap_make(h, key, idx, middle);
    reg_heap_scan(h, key, idx, middle, len, nullptr, 0);
    wave_sync();
    return;
  }
  if (lane == 0) make_heap(key, idx, middle);
  wave_sync();
  uint32_t top = (uint32_t)key[0];
  for (int base = middle; base < len; base += 64) {
    const int i = base + lane;
    const uint32_t ki = i < len ? (uint32_t)key[i] : 0xFFFFFFFFu;
    uint64_t cand = __builtin_amdgcn_ballot_w64(i < len && ki < top);
    while (cand) {
      const int l = (int)__builtin_ctzll(cand);
      if (lane == 0) pop_heap(key, idx, middle, base + l);
      wave_sync();
      top = (uint32_t)key[0];
      cand &= ~((2ull << l) - 1ull) & __builtin_amdgcn_ballot_w64(ki < top);
    }
  }
  wave_sync();
}

// P1 of a level: the ge / le counts of one wave's stripe, counted per lane on the VALU (packed
// ge | le << 16) and summed once per pass (a 16-lane DPP scan, four readlanes).  Ballot counts
// (s_bcnt + s_add per row on the scalar unit, which all 32 waves of a CU share) cost the
// selection 2 % (SELECT_GATHER 0.1525 -> 0.1494 ms at the headline, 0.187 -> 0.183 snapkv,
// 0.128 -> 0.124 h2o; profiles/r03_zz_valu_counts_ab.jsonl): the kernel is bound by the CU's
// total issue work and the scalar unit carried the larger share.
// WHOLE: every position of the stripe is below hi (unclamped loads with immediate offsets; rows
// j >= J of a JM-row body read at most JM/2 rows past the stripe -- the smallest body, 1 --
// inside the selection arrays).  Otherwise loads are clamped and lanes past hi masked off.
// Position ch is counted with the key it holds (the pivot value); the caller corrects the owner
// wave's counts for the virtual median move.
// A level body of bound JM runs levels with JM/2 < J <= JM, so rows j < JM/2 need no J check.
// The smallest body, JM = 2, also runs the J = 1 levels (less code for the instruction cache;
// smallest bodies of 1 / 2 / 4 / 8 measured within noise of each other,
// profiles/r06_f_itab_ab.jsonl): its one unchecked row, row 0, is there at J = 1 too.
template <int JM>
__device__ constexpr int jm_rows_past() {
  static_assert(JM >= 2, "the smallest level body is JM = 2");
  return JM / 2;
}
template <typename KeyT, int JM, bool WHOLE>
__device__ __forceinline__ void p1_counts(const KeyT* key, int pos0, int J, int hi, uint32_t p,
                                          int& cge, int& cle) {
  constexpr int JB = JM < 16 ? JM : 16;
  uint32_t pc = 0;  // per-lane counts: ge | le << 16 (at most 64 per lane)
  unroll_for<0, JM / JB>([&](auto bc) {
    constexpr int j0 = decltype(bc)::value * JB;
    if (j0 > 0 && j0 >= J) return;
    KeyT kv[JB];
    unroll_for<0, JB>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      const int pos = pos0 + (j0 + q) * 64;
      kv[q] = key[WHOLE ? pos : min(pos, hi - 1)];
    });
    unroll_for<0, JB>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      constexpr int j = j0 + q;
      if (j >= jm_rows_past<JM>() && j >= J) return;
      bool ge = (uint32_t)kv[q] >= p, le = (uint32_t)kv[q] <= p;
      if constexpr (!WHOLE) {
        const bool inb = pos0 + j * 64 < hi;
        ge = ge && inb;
        le = le && inb;
      }
      pc += (ge ? 1u : 0u) + (le ? 0x10000u : 0u);
    });
  });
  const int rs = row_scan16((int)pc);  // per 16-lane row; the four row totals on the scalar unit
  const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane(rs, 15) +
                       (uint32_t)__builtin_amdgcn_readlane(rs, 31) +
                       (uint32_t)__builtin_amdgcn_readlane(rs, 47) +
                       (uint32_t)__builtin_amdgcn_readlane(rs, 63);
  cge += (int)(tot & 0xFFFFu);
  cle += (int)(tot >> 16);
}

// Candidate prefilter of std::__heap_select(first, middle, last) for middle <= 64, by NT
// threads: position i >= middle enters the heap iff key[i] < top_i, and top_i -- the heap's max
// -- is the middle-th smallest key of [0, i) (the heap always holds the `middle` smallest keys
// seen, as a multiset).  Any `middle`-element subset of [0, i) bounds it from above, so with the
// scan range cut into one chunk per wave, U_w = min(max of the first `middle` keys, the
// middle-th smallest key of each earlier chunk) >= top_i for every i of chunk w, and {i in chunk
// w : key[i] < U_w} holds every entering position.  Writes those positions, ascending, to `cand`
// (capacity ccap) and returns their count, or -1 (nothing written) when they do not fit or a
// chunk exceeds 20 rows of 64; ends with a barrier.  The heap scan then visits only them:
// ~1 800 of 15 936 positions for the h2o heavy hitters (k = 64).
template <int NT, bool EXACT = true, typename K>
__device__ int heap_candidates(const K* key, int middle, int len, uint16_t* cand, int ccap,
                               int* wbuf, int* cbuf, int w0 = 0) {
  constexpr int NW = NT / 64, JM = 20;  // 16 384 positions over 15 chunk waves: 17 rows
  static_assert(NW <= 16, "one 16-lane DPP row holds the wave values");
  const int lane = threadIdx.x & 63, wid = uni((int)(threadIdx.x >> 6));
  const int span = len - middle;
  const int rows = (span + 64 * (NW - w0) - 1) / (64 * (NW - w0));  // rows per chunk (uniform)
  if (rows > JM) return -1;
  // waves below w0 (busy elsewhere until the first barrier) hold no chunk
  const int c0 = wid < w0 ? len : middle + (wid - w0) * rows * 64, c1 = min(c0 + rows * 64, len);
  uint32_t kv[JM];
  uint32_t mn = 0xFFFFFFFFu, mx = 0u;
#pragma unroll
  for (int j = 0; j < JM; ++j) {
    const int pos = c0 + j * 64 + lane;
    const bool v = j < rows && pos < c1;
    kv[j] = v ? (uint32_t)key[pos] : 0xFFFFFFFFu;
    mn = v ? min(mn, kv[j]) : mn;
    mx = v ? max(mx, kv[j]) : mx;
  }
  uint32_t q0 = lane < middle ? (uint32_t)key[lane] : 0u;  // max of the first `middle` keys
  if (!EXACT) mx = mn;  // loose bound: the largest lane minimum (>= 64 keys lie at or below it)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    if (EXACT) mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    q0 = max(q0, (uint32_t)__shfl_xor((int)q0, o, 64));
  }
  // this chunk's middle-th smallest key: the smallest v with #(key <= v) >= middle (bisection on
  // the VALU, one wave reduction per step); loose: every lane holds a key (a full first row)
  uint32_t lo = EXACT ? (uint32_t)uni((int)mn) : (uint32_t)uni((int)mx), hi = (uint32_t)uni((int)mx);
  const bool has = EXACT ? c1 - c0 >= middle : c1 - c0 >= 64;
  while (EXACT && has && lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    int cl = 0;
#pragma unroll
    for (int j = 0; j < JM; ++j) cl += kv[j] <= mid ? 1 : 0;  // invalid slots hold ~0u
    const int rs = row_scan16(cl);
    const int c = __builtin_amdgcn_readlane(rs, 15) + __builtin_amdgcn_readlane(rs, 31) +
                  __builtin_amdgcn_readlane(rs, 47) + __builtin_amdgcn_readlane(rs, 63);
    if (c >= middle) hi = mid;
    else lo = mid + 1;
  }
  if (lane == 0) wbuf[wid] = has ? (int)lo : -1;  // -1: no bound (0xFFFFFFFF)
  __syncthreads();
  uint32_t U = (uint32_t)uni((int)q0);
  for (int w = 0; w < wid; ++w) U = min(U, (uint32_t)wbuf[w]);
  int c = 0;
#pragma unroll
  for (int j = 0; j < JM; ++j) c += __popcll(__builtin_amdgcn_ballot_w64(kv[j] < U));
  if (lane == 0) cbuf[wid] = c;
  __syncthreads();
  int before = 0, total = 0;
  for (int w = 0; w < NW; ++w) {
    const int cw = cbuf[w];
    before += w < wid ? cw : 0;
    total += cw;
  }
  if (total > ccap) {
    __syncthreads();  // wbuf / cbuf are free again
    return -1;
  }
#pragma unroll
  for (int j = 0; j < JM; ++j) {
    const uint64_t b = __builtin_amdgcn_ballot_w64(kv[j] < U);
    if (kv[j] < U) cand[before + mbcnt(b, 0)] = (uint16_t)(c0 + j * 64 + lane);
    before += __popcll(b);
  }
  __syncthreads();
  return total;
}

// P2 of a level, rank window 0: scatter the s and g rank -> position tables for ranks <= cap
// and count the swaps (nsw), from re-read keys.  With F(x) = A(x) + Lin(x) (non-decreasing in
// x), a ge position is swapped iff F < tot_le and an le position iff F > tot_le, and only the
// swapped g's and s's plus g_{m+1} are ever read back.  So a whole stripe (MODE):
//   P2_FULL  straddles F = tot_le: records every ge and le rank <= cap, counts its swaps;
//   P2_LEFT  ends at F <= tot_le: every ge swapped (nsw = its ge count, set by the caller), no
//            le swapped -- records the g ranks only;
//   P2_RIGHT starts at F >= tot_le: no ge swapped, every le swapped -- records the s ranks and
//            its first ge position (g_{m+1} when no earlier stripe has an unswapped ge).
// FAST: a whole stripe without the median slot.  Otherwise (always P2_FULL) lanes past hi are
// masked and the median slot ch carries klo's flags (kge / kle): the owner wave moves the
// median physically only after this pass.
enum { P2_FULL = 0, P2_LEFT = 1, P2_RIGHT = 2 };
// P2's running rank bases are scalar popcounts (s_bcnt1 + s_add on the CU's one scalar unit, then
// a v_mov into mbcnt's base operand)
// ISINK: the lane sinks start at spos + ssink / gpos + gsink (level 0's tables in the idx region
// sink into the shared tables); otherwise they are the 64 entries before each table
template <typename KeyT, int JM, bool FAST, int MODE = P2_FULL, bool ISINK = false>
__device__ __forceinline__ void p2_window0(const KeyT* key, uint16_t* spos, uint16_t* gpos,
                                           int lane, int pos0, int wbeg, int J, int hi,
                                           uint32_t p, int ch, bool kge, bool kle, int rge1,
                                           int rle, int tot_le, int cap, int& nsw,
                                           int ssink = -64, int gsink = -64) {
  static_assert(FAST || MODE == P2_FULL, "partial stripes take the full pass");
  const int ssl = ISINK ? ssink + lane : lane - 64, gsl = ISINK ? gsink + lane : lane - 64;
  // keys in flight per lane (register budget: 64 VGPRs); 4 and 16 measured the same
  // (profiles/r03_c_p2_keys_in_flight_ab.jsonl)
  constexpr int JB = JM < 8 ? JM : 8;
  const int t1 = tot_le + 1;
  const int cap1 = cap + 1;  // the dump slot (slots 1..cap are the window's ranks)
  const int g1 = rge1;  // P2_RIGHT: rank of the stripe's first ge position
  int ff = kBig;        // P2_RIGHT: the stripe's first ge position (wave-uniform)
  unroll_for<0, JM / JB>([&](auto bc) {
    constexpr int j0 = decltype(bc)::value * JB;
    if (j0 > 0 && j0 >= J) return;
    KeyT kv[JB];
    unroll_for<0, JB>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      const int pos = pos0 + (j0 + q) * 64;
      kv[q] = key[FAST ? pos : min(pos, hi - 1)];
    });
    unroll_for<0, JB>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      constexpr int j = j0 + q;
      if (j >= jm_rows_past<JM>() && j >= J) return;
      const int pj = pos0 + j * 64;
      bool ge = (uint32_t)kv[q] >= p, le = (uint32_t)kv[q] <= p;
      if constexpr (!FAST) {
        const bool inb = pj < hi, isch = pj == ch;
        ge = inb && (isch ? kge : ge);
        le = inb && (isch ? kle : le);
      }
      // Scatter slots are plain selects (v_min + v_cndmask): a rank past the window goes to the
      // never-read slot cap + 1, a lane without the flag to its sink.  (Written as
      // `flag && rank <= cap ? rank : sink`, the compiler emitted two exec-mask branches per row
      // of 64 positions -- 7 scalar instructions on the CU's one scalar unit.)
      if constexpr (MODE == P2_LEFT) {
        const uint64_t bg = __builtin_amdgcn_ballot_w64(ge);
        const int a1 = vreg(min(mbcnt(bg, rge1), cap1));
        gpos[ge ? a1 : gsl] = (uint16_t)pj;
        rge1 += __popcll(bg);
      } else if constexpr (MODE == P2_RIGHT) {
        const uint64_t bl = __builtin_amdgcn_ballot_w64(le);
        const int sr = vreg(min(t1 - 1 - mbcnt(bl, rle), cap1));  // s rank of an le position
        spos[le ? sr : ssl] = (uint16_t)pj;
        rle += __popcll(bl);
        if (ff == kBig) {
          const uint64_t bg = __builtin_amdgcn_ballot_w64(ge);
          if (bg) ff = pj - lane + (int)__builtin_ctzll(bg);
        }
      } else {
        const uint64_t bg = __builtin_amdgcn_ballot_w64(ge), bl = __builtin_amdgcn_ballot_w64(le);
        const int a1 = vreg(mbcnt(bg, rge1));                   // g rank: A + 1
        const int sr = vreg(t1 - (mbcnt(bl, rle) + (le ? 1 : 0)));  // s rank: tot_le - Lin + 1
        spos[le ? min(sr, cap1) : ssl] = (uint16_t)pj;
        gpos[ge ? min(a1, cap1) : gsl] = (uint16_t)pj;
        // g_t < s_t  <=>  A + Lin < tot_le  <=>  a1 < sr: swapped (a prefix t <= m of the g's)
        nsw += __popcll(bg & __builtin_amdgcn_ballot_w64(a1 < sr));
        rge1 += __popcll(bg);
        rle += __popcll(bl);
      }
    });
  });
  if constexpr (MODE == P2_RIGHT) {
    if (ff != kBig && g1 <= cap && lane == 0) gpos[g1] = (uint16_t)ff;
  }
}

// The chain's last levels, once the segment [lo, hi) holds at most 64 positions, run by one wave
// with the segment in registers: lane i holds position lo + i (key, index).  A level is the same
// libstdc++ step as partition_level (std::__move_median_to_first + std::__unguarded_partition:
// g_t <-> s_t for the prefix t <= m with g_t < s_t, cut = min(g_{m+1}, s_m)), computed from two
// ballots: the g / s rank -> lane tables are built by forward permutes (ds_permute) and each
// swapped lane fetches its partner's entry by a backward permute -- no LDS memory round trips,
// no rank-table stores.  The final stable insertion sort ranks the segment's lanes against each
// other, and every lane writes its entry back once.  depth == 0 (the introsort / introselect
// depth limit) writes the registers back and takes the serial heap path, as run_chain does.
// Returns with the segment's final arrangement in key / idx (only the first-k SET matters).
template <typename KeyT>
__device__ __forceinline__ void wave_tiny_chain(KeyT* key, uint16_t* idx, int k, bool topk,
                                                int thr, int lo, int hi, int depth,
                                                uint32_t* status) {
  const int lane = threadIdx.x & 63;
  const int m = hi - lo;  // <= 64
  const bool own = lane < m;
  uint32_t kk = own ? (uint32_t)key[lo + lane] : 0xFFFFFFFFu;
  uint32_t ii = own ? (uint32_t)idx[lo + lane] : 0u;
  int slo = 0, shi = m;          // the segment, relative to lo
  const int kr = k - lo;         // k relative to lo
  int dest = lane;               // where this lane's entry is written back
  bool heap = false;
  while (true) {
    if (slo == kr || shi == kr) break;  // a partition boundary sits at k
    if (shi - slo <= thr) {  // final stable insertion sort: rank within [slo, shi)
      const bool in = lane >= slo && lane < shi;
      int r = 0;
      for (int j = slo; j < shi; ++j) {  // uniform trip count
        const uint32_t kj = (uint32_t)__builtin_amdgcn_readlane((int)kk, j);
        r += (kj < kk || (kj == kk && j < lane)) ? 1 : 0;
      }
      dest = in ? slo + r : lane;
      break;
    }
    if (depth == 0) {  // depth limit: the serial heap algorithms on LDS
      heap = true;
      break;
    }
    --depth;
    // std::__move_median_to_first(slo, slo + 1, mid, shi - 1)
    const int a = slo + 1, b = slo + (shi - slo) / 2, c = shi - 1;
    const uint32_t ka = (uint32_t)__builtin_amdgcn_readlane((int)kk, a);
    const uint32_t kb = (uint32_t)__builtin_amdgcn_readlane((int)kk, b);
    const uint32_t kc = (uint32_t)__builtin_amdgcn_readlane((int)kk, c);
    int ch;
    if (ka < kb) {
      if (kb < kc) ch = b; else if (ka < kc) ch = c; else ch = a;
    } else if (ka < kc) {
      ch = a;
    } else if (kb < kc) {
      ch = c;
    } else {
      ch = b;
    }
    const uint32_t p = ch == a ? ka : ch == b ? kb : kc;
    const uint32_t klo = (uint32_t)__builtin_amdgcn_readlane((int)kk, slo);
    const uint32_t ich = (uint32_t)__builtin_amdgcn_readlane((int)ii, ch);
    const uint32_t ilo = (uint32_t)__builtin_amdgcn_readlane((int)ii, slo);
    kk = lane == slo ? p : lane == ch ? klo : kk;
    ii = lane == slo ? ich : lane == ch ? ilo : ii;
    // std::__unguarded_partition(slo + 1, shi, pivot = slo)
    const bool inr = lane > slo && lane < shi;
    const bool ge = inr && kk >= p, le = inr && kk <= p;
    const uint64_t GE = __builtin_amdgcn_ballot_w64(ge), LE = __builtin_amdgcn_ballot_w64(le);
    const int tot_le = __popcll(LE);
    const int A = mbcnt(GE, 0);                    // ge lanes below
    const int lin = mbcnt(LE, 0) + (le ? 1 : 0);   // le lanes in (slo, lane]
    const bool sg = ge && A + lin < tot_le;        // g_t (t = A + 1) with g_t < s_t: swapped
    const uint64_t SG = __builtin_amdgcn_ballot_w64(sg);
    const int msw = __popcll(SG);
    // the rank -> lane tables below use lane 63 as the sink of lanes with nothing to record:
    // sound because the swapped pairs are disjoint in (slo, shi), so msw <= 31 ranks (lanes
    // 0..30).  Checked (one scalar compare per level), never expected to fire.
    if (msw > 31 && status && lane == 0) atomicOr(status, (uint32_t)KVC_DEV_INTERNAL);
    const int srk = tot_le - lin + 1;              // s rank of an le lane
    const bool ss = le && srk <= msw;              // s_t, t <= m: swapped
    // rank -> lane tables: lane t - 1 of gt / st receives g_t / s_t (others write lane 63,
    // never read: m <= 31)
    const int gt = __builtin_amdgcn_ds_permute((sg ? A : 63) * 4, lane);
    const int st = __builtin_amdgcn_ds_permute((ss ? srk - 1 : 63) * 4, lane);
    const int tab = gt | (st << 8);
    const int t1 = sg ? A : ss ? srk - 1 : 0;      // this lane's rank - 1
    const int pt = __builtin_amdgcn_ds_bpermute(t1 * 4, tab);
    const int partner = sg ? (pt >> 8) : ss ? (pt & 0xFF) : lane;
    if constexpr (sizeof(KeyT) == 2) {
      const uint32_t w = __builtin_amdgcn_ds_bpermute(partner * 4, (int)(kk << 16 | ii));
      kk = w >> 16;
      ii = w & 0xFFFFu;
    } else {
      const uint32_t nk = __builtin_amdgcn_ds_bpermute(partner * 4, (int)kk);
      ii = __builtin_amdgcn_ds_bpermute(partner * 4, (int)ii);
      kk = nk;
    }
    // cut = min(g_{m+1}, s_m): the first unswapped ge lane, the lowest swapped le lane
    const uint64_t GN = GE & ~SG;
    const int gnext = GN ? (int)__builtin_ctzll(GN) : kBig;
    const uint64_t SS = __builtin_amdgcn_ballot_w64(ss);
    const int cut = min(gnext, SS ? (int)__builtin_ctzll(SS) : kBig);
    const bool right = topk ? cut <= kr - 1 : kr > cut;
    slo = right ? cut : slo;
    shi = right ? shi : cut;
  }
  if (own) {
    key[lo + dest] = (KeyT)kk;
    idx[lo + dest] = (uint16_t)ii;
  }
  if (heap) {
    wave_sync();
    if (lane == 0) {
      if (topk) {
        heap_select(key + lo + slo, idx + lo + slo, kr - slo, shi - slo);
        kv_swap(key, idx, lo + slo, k - 1);
      } else {
        make_heap(key + lo + slo, idx + lo + slo, shi - slo);
        sort_heap(key + lo + slo, idx + lo + slo, shi - slo);
      }
    }
  }
  wave_sync();
}

// One partition level over [lo, hi) with at most JM positions per lane (compile-time bound; the
// passes stop at the segment's own J with a scalar branch).  Returns cut.  See run_chain for
// the algorithm.  P1 and P2 are issue-bound at the long levels (16 waves of 16 rows of 64
// positions), so per-position work is a handful of VALU ops: flags are compare ballots
// (recomputed from the keys in P2 rather than carried), wave counts are scalar popcounts, and
// wave-uniform work -- median of 3, cross-wave prefix sums, swap count, g_{m+1} -- runs on SGPRs.
//
// ITAB (level 0 of a 1 024-thread row, lo = 0, indices still the identity; ihalf = n_cap / 2):
// the rank tables are the two halves of the idx region, whose n_cap / 2 - 1 ranks cover every m
// the level can reach (m <= (hi - lo - 1) / 2): one window.  The median move and P4 then swap keys
// only; after every table read (a barrier) the indices are rebuilt: the identity with the
// median's transposition (lo <-> ch), then (another barrier) each swapped pair's entries from
// the pair kept in registers -- the same arrangement as physical index swaps, without P4's
// index loads and without the second window (and its flag pass).
template <typename KeyT, int NT, int JM, bool ITAB = false>
__device__ __forceinline__ int partition_level(KeyT* key, uint16_t* idx, uint16_t* spos,
                                               uint16_t* gpos, SelScalars<KeyT>& sc, int lo,
                                               int hi, int cap, uint64_t* acc, int ihalf = 0) {
  static_assert(!ITAB || (NT > 64 && sizeof(KeyT) == 2), "ITAB: level 0 of 16-bit block rows");
  constexpr int NW = NT / 64;
  typedef typename std::conditional<(JM > 32), uint64_t, uint32_t>::type MaskT;
  const int lane = threadIdx.x & 63;
  const int wid = (NT == 64) ? 0 : uni((int)(threadIdx.x >> 6));
  const int tid = wid * 64 + lane;
  uint64_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;
  KVC_TICK(t0);
  const int J = (hi - lo - 1 + NT - 1) / NT;  // <= JM
  const int wbeg = lo + 1 + wid * J * 64;
  const int pos0 = wbeg + lane;
  // ---- median of 3 (std::__move_median_to_first), on the scalar unit; the swap into lo is
  // virtual until the owner wave of position ch has read its P2 keys ----
  const int a = lo + 1, b = lo + (hi - lo) / 2, c = hi - 1;
  const uint32_t ka = (uint32_t)uni((int)key[a]), kb = (uint32_t)uni((int)key[b]);
  const uint32_t kc = (uint32_t)uni((int)key[c]), klo = (uint32_t)uni((int)key[lo]);
  int ch;
  if (ka < kb) {
    if (kb < kc) ch = b; else if (ka < kc) ch = c; else ch = a;
  } else if (ka < kc) {
    ch = a;
  } else if (kb < kc) {
    ch = c;
  } else {
    ch = b;
  }
  const uint32_t p = (ch == a) ? ka : (ch == b) ? kb : kc;
  const bool kge = klo >= p, kle = klo <= p;  // flags of the key that moves into slot ch
  const int nval = hi - wbeg;                 // positions of this wave's stripe below hi
  const bool whole = nval >= J * 64;
  const bool owner = ch >= wbeg && ch < wbeg + J * 64;
  uint64_t ta = 0, tb = 0, tc = 0;  // diagnostic build: P1 sub-phases of a J = 16 level
  KVC_TICK(ta);
  // ---- P1: wave ge / le counts ----
  int cge = 0, cle = 0;
  if (whole)
    p1_counts<KeyT, JM, true>(key, pos0, J, hi, p, cge, cle);
  else if (nval > 0)
    p1_counts<KeyT, JM, false>(key, pos0, J, hi, p, cge, cle);
  if (owner) {  // slot ch was counted with the pivot's flags (both set); it holds klo
    cge -= kge ? 0 : 1;
    cle -= kle ? 0 : 1;
  }
  KVC_TICK(tb);
  int ge_before = 0, le_before = 0, tot_le = cle, tot_ge = cge;
  if constexpr (NW > 1) {
    static_assert(NW <= 16, "cross-wave scans use one 16-lane DPP row");
    if (lane == 0)  // sums < 2^16 (positions < 65536): packed
      sc.wa[wid] = (int)((uint32_t)cge | ((uint32_t)cle << 16));
    KVC_TICK(tc);
#ifdef KVC_STAMPS
    if (lane == 0) {  // diagnostic: this wave's level start and P1 end (low 32 bits)
      sc.wb[wid] = (int)(uint32_t)t0;
      sc.fnan[wid] = (int)(uint32_t)tc;
    }
#endif
    __syncthreads();  // B_a
    const int scan = row_scan16(lane < NW ? sc.wa[lane] : 0);
    // unpack unsigned: the le half reaches bit 31 for segments longer than 32767 positions
    const uint32_t before = wid ? (uint32_t)__builtin_amdgcn_readlane(scan, wid - 1) : 0u;
    ge_before = (int)(before & 0xFFFFu);
    le_before = (int)(before >> 16);
    const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane(scan, NW - 1);
    tot_le = (int)(tot >> 16);
    tot_ge = (int)(tot & 0xFFFFu);
  }
  // ITAB: the level's tables in the idx region, sinks in the shared tables
  uint16_t* const shs = spos;
  bool it = false;
  int ssink = -64, gsink = -64;
  if constexpr (ITAB) {
    it = true;
    {
      ssink = (int)(spos - idx);
      gsink = (int)(gpos - (idx + ihalf));
      spos = idx;
      gpos = idx + ihalf;
      cap = ihalf - 1;
    }
  }
  KVC_TICK(t1);
  // ---- P2, rank window 0: s / g rank tables, swap count m, g_{m+1} (stores only) ----
  int nsw = 0;
  if (whole && !owner) {
    if (ge_before + cge + le_before + cle <= tot_le) {  // every ge swapped, no le
      p2_window0<KeyT, JM, true, P2_LEFT, ITAB>(key, spos, gpos, lane, pos0, wbeg, J, hi, p, ch,
                                                kge, kle, ge_before + 1, le_before, tot_le, cap,
                                                nsw, ssink, gsink);
      nsw = cge;
    } else if (ge_before + le_before >= tot_le) {  // no ge swapped, every le
      p2_window0<KeyT, JM, true, P2_RIGHT, ITAB>(key, spos, gpos, lane, pos0, wbeg, J, hi, p, ch,
                                                 kge, kle, ge_before + 1, le_before, tot_le, cap,
                                                 nsw, ssink, gsink);
    } else {
      p2_window0<KeyT, JM, true, P2_FULL, ITAB>(key, spos, gpos, lane, pos0, wbeg, J, hi, p, ch,
                                                kge, kle, ge_before + 1, le_before, tot_le, cap,
                                                nsw, ssink, gsink);
    }
  } else if (nval > 0)
    p2_window0<KeyT, JM, false, P2_FULL, ITAB>(key, spos, gpos, lane, pos0, wbeg, J, hi, p, ch,
                                               kge, kle,
                                ge_before + 1, le_before, tot_le, cap, nsw, ssink, gsink);
  // the median move, made physical by the only wave that reads slot ch (after its P2 loads)
  if (owner && lane == 0) {
    if (ITAB && it) {  // keys only: the idx region holds the tables
      const KeyT t = key[lo];
      key[lo] = key[ch];
      key[ch] = t;
    } else {
      kv_swap(key, idx, lo, ch);
    }
  }
  int msw;
#ifdef KVC_STAMPS
  uint64_t tp2 = 0;
  KVC_TICK(tp2);
  uint32_t wstart[NW > 1 ? NW : 1], wp1[NW > 1 ? NW : 1];
  if constexpr (NW > 1) {
    if (acc && tid == 0 && JM == 16 && J == 16)
      for (int w = 0; w < NW; ++w) {
        wstart[w] = (uint32_t)sc.wb[w];
        wp1[w] = (uint32_t)sc.fnan[w];
      }
    __syncthreads();  // diagnostic: the P1 stamps are read before P2 stamps overwrite them
    if (lane == 0) sc.fnan[wid] = (int)(uint32_t)tp2;
  }
#endif
  if constexpr (NW > 1) {
    if (lane == 0) sc.wm[wid] = nsw;
    __syncthreads();  // B_b
    msw = __builtin_amdgcn_readlane(row_scan16(lane < NW ? sc.wm[lane] : 0), NW - 1);
  } else {
    wave_sync();
    msw = nsw;
  }
  // g_{m+1}, the first unswapped ge position (none when every ge position is swapped)
  int gnext = msw >= tot_ge ? kBig : msw < cap ? uni((int)gpos[msw + 1]) : kBig;
  KVC_TICK(t2);
  // ---- m >= cap (rare): the level's flags, from the keys before any swap (the median slot is
  // physical now), kept in registers for the later windows' scatters (the swapped pairs are
  // disjoint, so earlier windows' swaps do not change them), and g_{m+1} from a flag pass ----
  MaskT gem = 0, lem = 0;
  if (msw >= cap) {
    for (int j = 0; j < J; ++j) {
      const int pos = pos0 + j * 64;
      const bool inb = pos < hi;
      const uint32_t kk = (uint32_t)key[min(pos, hi - 1)];
      gem |= (inb && kk >= p) ? ((MaskT)1 << j) : (MaskT)0;
      lem |= (inb && kk <= p) ? ((MaskT)1 << j) : (MaskT)0;
    }
    int rge = ge_before, rle = le_before, ff = kBig;
    for (int j = 0; j < J && ff == kBig; ++j) {
      const bool ge = (gem >> j) & 1, le = (lem >> j) & 1;
      const uint64_t bg = __builtin_amdgcn_ballot_w64(ge), bl = __builtin_amdgcn_ballot_w64(le);
      const bool cond = mbcnt(bg, rge) + mbcnt(bl, rle) + (le ? 1 : 0) < tot_le;
      const uint64_t bf = bg & ~__builtin_amdgcn_ballot_w64(cond);
      if (bf) ff = wbeg + j * 64 + (int)__builtin_ctzll(bf);
      rge += __popcll(bg);
      rle += __popcll(bl);
    }
    if constexpr (NW > 1) {
      if (lane == 0) sc.wb[wid] = ff == kBig ? 0xFFFF : ff;  // ff < 65535
      __syncthreads();  // every wave has its flags before the first swap
      const uint32_t x = lane < NW ? (uint32_t)sc.wb[lane] : 0xFFFFu;
      // waves in position order: the first one with an unswapped ge position wins
      const uint64_t fb = __builtin_amdgcn_ballot_w64(x != 0xFFFFu);
      gnext = fb ? __builtin_amdgcn_readlane((int)x, (int)__builtin_ctzll(fb)) : kBig;
    } else {
      wave_sync();
      gnext = ff;
    }
  }
  if (ITAB && it) {
    // ---- P4, one window: the m pairs, ranks t = 1 + tid + q NT (q < JM / 2: m <= NT J / 2),
    // kept packed (g | s << 16) for the index rebuild; keys swapped now ----
    constexpr int QM = JM / 2 > 0 ? JM / 2 : 1;
    // q-rows with a rank for this wave (uniform): the rest keep pr = 0 and touch nothing
    const int nq = msw >= 1 + wid * 64 ? uni(min(QM, (msw - 1 - wid * 64) / NT + 1)) : 0;
    uint32_t pr[QM];
    KeyT kg[QM], ks[QM];
#pragma unroll
    for (int q = 0; q < QM; ++q) pr[q] = 0u;
#pragma unroll
    for (int q = 0; q < QM; ++q) {
      if (q >= nq) break;
      const int t = 1 + tid + q * NT;
      const bool v = t <= msw;
      const int ti = v ? t : 0;
      const int g = gpos[ti], sv = spos[ti];
      pr[q] = v ? ((uint32_t)g | (uint32_t)sv << 16) : 0u;  // lo = 0: a self swap of slot 0
    }
    // the cut's s_m, read before the tables are overwritten
    const int sm = msw > 0 ? uni((int)spos[msw]) : kBig;
#pragma unroll
    for (int q = 0; q < QM; ++q) {
      if (q >= nq) break;
      kg[q] = key[pr[q] & 0xFFFFu];
      ks[q] = key[pr[q] >> 16];
    }
#pragma unroll
    for (int q = 0; q < QM; ++q) {
      if (q >= nq) break;
      key[pr[q] & 0xFFFFu] = ks[q];
      key[pr[q] >> 16] = kg[q];
    }
    __syncthreads();  // every table entry is read
    // identity indices with the median's transposition lo <-> ch: 16-B stores, then the two
    // entries by the thread that stored them (same-thread LDS order)
    for (int v = tid; v < (hi + 7) / 8; v += NT) {
      const uint32_t b = (uint32_t)v * 8;
      reinterpret_cast<uint4*>(idx)[v] =
          make_uint4(b | (b + 1) << 16, (b + 2) | (b + 3) << 16, (b + 4) | (b + 5) << 16,
                     (b + 6) | (b + 7) << 16);
      if (v == (lo >> 3)) idx[lo] = (uint16_t)ch;
      if (v == (ch >> 3)) idx[ch] = (uint16_t)lo;
    }
    __syncthreads();
    // the swapped pairs' entries: idx[g] = old idx[s], idx[s] = old idx[g] (old = identity with
    // lo <-> ch; lo is never swapped).  Lanes without a pair write the shared tables' sinks.
    uint16_t* sink = shs + lane;
#pragma unroll
    for (int q = 0; q < QM; ++q) {
      if (q >= nq) break;
      const int g = (int)(pr[q] & 0xFFFFu), sv = (int)(pr[q] >> 16);
      const bool v = pr[q] != 0u;
      (v ? idx + g : sink)[0] = (uint16_t)(sv == ch ? lo : sv);
      (v ? idx + sv : sink)[0] = (uint16_t)(g == ch ? lo : g);
    }
    __syncthreads();  // B_c
    KVC_TICK(t3);
#ifdef KVC_STAMPS
    if (acc && tid == 0) {
      acc[0] += t1 - t0;
      acc[1] += t2 - t1;
      acc[2] += t3 - t2;
      acc[3] += 1;
      acc[4] += (uint64_t)msw;
      acc[25] = (t1 - t0) | ((t2 - t1) << 20) | ((t3 - t2) << 40);
    }
#endif
    return min(gnext, sm);
  }
  int wb = 0;
  while (true) {
    // ---- P4: this window's swaps (disjoint pairs g_t <-> s_t), spread evenly over the NT
    // lanes: rank-table loads, then key/idx loads, then stores ----
    // Lanes past the window's last rank swap the pivot slot lo with itself (lo is never a
    // swapped g_t or s_t: every g_t > lo, and a swapped s_t > g_t), so the loads and stores need
    // no exec-mask branches; q-rows with no rank left for the wave are skipped uniformly.
    const int wend = min(msw, wb + cap);
    for (int base = wb + 1; base <= wend; base += NT * 4) {
      if (base + wid * 64 > wend) break;  // no rank left for this wave
      const int nq = uni(min(4, (wend - base - wid * 64) / NT + 1));  // q-rows with a rank
      int gp[4], sp[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q >= nq) break;
        const int t = base + tid + q * NT;
        const bool v = t <= wend;
        const int ti = v ? t - wb : 0;
        const int g = gpos[ti], sv = spos[ti];
        gp[q] = v ? g : lo;
        sp[q] = v ? sv : lo;
      }
      KeyT kg[4], ks[4];
      uint16_t ig[4], is[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q >= nq) break;
        kg[q] = key[gp[q]];
        ks[q] = key[sp[q]];
        ig[q] = idx[gp[q]];
        is[q] = idx[sp[q]];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q >= nq) break;
        key[gp[q]] = ks[q];
        key[sp[q]] = kg[q];
        idx[gp[q]] = is[q];
        idx[sp[q]] = ig[q];
      }
    }
    if (wend >= msw) break;
    group_sync<NT>();  // the next window overwrites the tables
    wb += cap;
    // ---- scatter of window wb from the flags (ranks (wb, wb + cap]) ----
    int rge = ge_before, rle = le_before;
    for (int j = 0; j < J; ++j) {
      const bool ge = (gem >> j) & 1, le = (lem >> j) & 1;
      const uint64_t bg = __builtin_amdgcn_ballot_w64(ge), bl = __builtin_amdgcn_ballot_w64(le);
      const int A = mbcnt(bg, rge);                   // ge positions before this one
      const int lin = mbcnt(bl, rle) + (le ? 1 : 0);  // le positions in [lo+1, pos]
      const bool cond = A + lin < tot_le;
      const uint16_t pj = (uint16_t)(pos0 + j * 64);
      const int sr = tot_le - lin + 1 - wb;  // s rank within the window
      spos[(le && sr >= 1 && sr <= cap) ? sr : lane - 64] = pj;
      const int gr = A + 1 - wb;             // swapped (cond): g rank A + 1 <= m
      gpos[(ge && cond && gr >= 1 && gr <= cap) ? gr : lane - 64] = pj;
      rge += __popcll(bg);
      rle += __popcll(bl);
    }
    group_sync<NT>();
  }
  group_sync<NT>();  // B_c
  KVC_TICK(t3);
#ifdef KVC_STAMPS
  if (acc && tid == 0) {
    acc[0] += t1 - t0;
    acc[1] += t2 - t1;
    acc[2] += t3 - t2;
    acc[3] += 1;
    acc[4] += (uint64_t)msw;
    if (NT > 64) acc[25] = (t1 - t0) | ((t2 - t1) << 20) | ((t3 - t2) << 40);  // level split
#ifdef KVC_SNAP_STAMPS
    if (false) {  // slots 26..29 hold the snapkv scoring stamps (tools/select_stamps.py with SEL_SNAP_STAMPS)
#else
    if (NT > 64 && JM == 16 && J == 16) {  // level 0 of a 16 384-position row (slots 26..29):
#endif
      // wave start skew, longest wave P1 (start -> counts written), last P1 end after the first
      // start, last P2 end after B_a (wave 0's t1)
      uint32_t s0 = wstart[0], s1 = wstart[0], p1m = 0, e1 = 0, e2 = 0;
      for (int w = 0; w < NW; ++w) {
        s0 = min(s0, wstart[w]);
        s1 = max(s1, wstart[w]);
      }
      for (int w = 0; w < NW; ++w) {
        p1m = max(p1m, wp1[w] - wstart[w]);
        e1 = max(e1, wp1[w] - s0);
        e2 = max(e2, (uint32_t)sc.fnan[w] - (uint32_t)t1);
      }
      acc[21] = s1 - s0;
      acc[22] = p1m;
      acc[23] = e1;
      acc[24] = e2;
    }
  }
#endif
  return min(gnext, msw > 0 ? uni((int)spos[msw - wb]) : kBig);
}

// The partition chain of libstdc++ introsort (topk = false) / introselect (topk = true),
// following only the segment [lo, hi) that straddles position k, run by NT cooperating lanes
// (the whole 1024-thread block, or one wave once the segment is short).  One level is
// std::__move_median_to_first + std::__unguarded_partition(lo+1, hi, pivot=lo) computed in
// parallel:
//   g_t = t-th position (ascending) in [lo+1,hi) with !(key < p)            ("ge")
//   s_t = t-th position (descending) with !(p < key), then the pivot slot lo ("le")
// libstdc++ swaps g_t <-> s_t for every t with g_t < s_t -- a prefix t <= m -- and returns
// cut = min(g_{m+1}, s_m).  With A(x) = #ge before x and Lin(x) = #le in [lo+1, x]:
//   g_t < s_t  <=>  A(g_t) + Lin(g_t) < tot_le
// so m is counted in the same pass that scatters the s rank -> position table (spos).
// Positions are laid out j-major (lane + 64*j within a wave's stripe) so flags are wave ballots;
// each level runs a body specialised on its positions-per-lane bound (2..16, or 64 for the
// global-memory variant of zones longer than kZoneMax).
// Returns 0 when the first-k set is final, 1 when the block hands a short segment to one wave.
template <typename KeyT, int NT, int MAXJ, bool L0T = true>
__device__ __forceinline__ int run_chain(KeyT* key, uint16_t* idx, uint16_t* spos, uint16_t* gpos,
                         SelScalars<KeyT>& sc, int k, bool topk, int thr, int cap, int& lo,
                         int& hi, int& depth, int& level, int wave_seg,
                         uint64_t* acc = nullptr, uint32_t* status = nullptr,
                         int ihalf = 0) {
  const int tid = (NT == 64) ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  while (true) {
    if (lo == k || hi == k) return 0;  // a partition boundary sits at k: the set is final
    if constexpr (NT == 64) {
      if (hi - lo <= 64 && hi - lo > thr) {  // the last levels from registers
        wave_tiny_chain(key, idx, k, topk, thr, lo, hi, depth, status);
        return 0;
      }
    }
    if (hi - lo <= thr) {              // final (stable) insertion sort of the segment
      if (tid < 64) wave_stable_sort(key, idx, lo, hi);
      group_sync<NT>();
      return 0;
    }
    if (NT > 64 && hi - lo <= wave_seg) return 1;
    if (depth == 0) {  // depth limit: libstdc++ switches to heap algorithms
      if (tid == 0) {
        if (topk) {
          heap_select(key + lo, idx + lo, k - lo, hi - lo);
          kv_swap(key, idx, lo, k - 1);
        } else {
          make_heap(key + lo, idx + lo, hi - lo);
          sort_heap(key + lo, idx + lo, hi - lo);
        }
      }
      group_sync<NT>();
      return 0;
    }
    --depth;
    const int J = (hi - lo - 1 + NT - 1) / NT;
    // Unused, and kept on purpose: without this test of level and lo ahead of the level bodies the
    // compiler emits different code for level 0 of the bf16 1 024-thread kernels
    const bool first = level == 0 && lo == 0;
    (void)first;
    int cut;
#ifdef KVC_STAMPS
    const uint64_t tl0 = __builtin_amdgcn_s_memtime();
#endif
    // level 0 of a 1 024-thread row with 16-bit keys keeps its rank tables in the idx region
    // (ihalf = n_cap / 2: n_cap / 2 - 1 ranks per table) when the shared tables could need a
    // second window (partition_level): level-0 swap counts sit around the shared cap (m median
    // 3 667 of cap 3 840 at the headline: 44 % of plain-norm rows took a second window).  The
    // extra barriers and index rebuild measured slower on snapkv rows, so launches without a
    // plain-norm row run the L0T = false instance (launch_chunk; profiles/r06_f_itab_ab.jsonl,
    // profiles/r06_h_l0t_instance_ab.jsonl)
    const bool itab = L0T && NT == kSelThreads && sizeof(KeyT) == 2 && ihalf > 0 && level == 0 &&
                      lo == 0 && J > 4 && (hi - 1) / 2 > cap && hi <= 2 * ihalf;
    if constexpr (L0T && NT == kSelThreads && sizeof(KeyT) == 2) {
      if (itab) {
        if (J <= 8)
          cut = partition_level<KeyT, NT, 8, true>(key, idx, spos, gpos, sc, lo, hi, cap, acc,
                                                   ihalf);
        else
          cut = partition_level<KeyT, NT, 16, true>(key, idx, spos, gpos, sc, lo, hi, cap, acc,
                                                    ihalf);
      }
    }
    if (itab) {
    } else if (J <= 2)
      cut = partition_level<KeyT, NT, 2>(key, idx, spos, gpos, sc, lo, hi, cap, acc);
    else if (J <= 4)
      cut = partition_level<KeyT, NT, 4>(key, idx, spos, gpos, sc, lo, hi, cap, acc);
    else if (J <= 8)
      cut = partition_level<KeyT, NT, 8>(key, idx, spos, gpos, sc, lo, hi, cap, acc);
    else if (MAXJ <= 16 || J <= 16)
      cut = partition_level<KeyT, NT, 16>(key, idx, spos, gpos, sc, lo, hi, cap, acc);
    else if (J <= 32)
      cut = partition_level<KeyT, NT, (MAXJ < 32 ? 16 : 32)>(key, idx, spos, gpos, sc, lo, hi, cap,
                                                               acc);
    else
      cut = partition_level<KeyT, NT, (MAXJ < 64 ? 16 : 64)>(key, idx, spos, gpos, sc, lo, hi, cap,
                                                               acc);
#ifdef KVC_STAMPS
    // per block level (first 8): cycles, and segment length  (slots 16.. of the row)
    if (acc && NT > 64 && tid == 0 && level < 5) {
      acc[11 + 2 * level] = __builtin_amdgcn_s_memtime() - tl0;
      acc[12 + 2 * level] = acc[25];  // P1 | P2 << 20 | P4 << 40 of this level
    }
#endif
    cut = uni(cut);  // uniform by construction; stated, so that lo / hi stay in SGPRs
    // std::__introselect: if (cut <= nth) first = cut; else last = cut;
    // std::__introsort_loop: recurse right, loop on the left part (k <= cut: keep the left).
    // Value selects, not branches: a store through a selected pointer to lo / hi would put
    // them in scratch memory.
    const bool right = topk ? cut <= k - 1 : k > cut;
    lo = right ? cut : lo;
    hi = right ? hi : cut;
    ++level;
  }
}

}  // namespace kvc
