// kvc_select.h -- one row's selection (select_body) and the SELECT kernels.
#pragma once

#include "kvc_select_chain.h"
#include "kvc_snapkv_keys.h"

namespace kvc {

// Exclusive prefix sum of one int per thread over the NT threads of the block (wave scans as
// four 16-lane DPP row scans, wave totals through `buf`); one barrier.
template <int NT>
__device__ __forceinline__ int block_exclusive_scan(int v, int* buf, int lane, int wid) {
  static_assert(NT / 64 <= 16, "one 16-lane DPP row holds the wave totals");
  const int rs = row_scan16(v);  // inclusive within each 16-lane row
  const int r0 = __builtin_amdgcn_readlane(rs, 15), r1 = __builtin_amdgcn_readlane(rs, 31);
  const int r2 = __builtin_amdgcn_readlane(rs, 47), r3 = __builtin_amdgcn_readlane(rs, 63);
  const int row = lane >> 4;
  const int excl = rs - v + (row > 0 ? r0 : 0) + (row > 1 ? r1 : 0) + (row > 2 ? r2 : 0);
  if constexpr (NT == 64) {
    return excl;
  } else {
    if (lane == 0) buf[wid] = r0 + r1 + r2 + r3;
    __syncthreads();
    const int ws = row_scan16(lane < NT / 64 ? buf[lane] : 0);
    const int w = uni(wid);
    return excl + (w ? __builtin_amdgcn_readlane(ws, w - 1) : 0);
  }
}


// Atomic += 1 on an int in LDS (`p` a generic pointer into the workgroup's LDS: its low 32
// bits are the LDS address).  A ds_add_u32 without return; callers wait (lgkmcnt) before the
// barrier that publishes the sums.  (The compiler's own lowering of an atomic through such a
// pointer emits an address-space test gfx950's VALU compare cannot encode.)
__device__ __forceinline__ void lds_add1(int* p) {
  const uint32_t a = (uint32_t)(uintptr_t)p;
  asm volatile("ds_add_u32 %0, %1" ::"v"(a), "v"(1) : "memory");
}

// Block-wide sum of one int per wave (waves of NT threads).  Callers alternate two buffers, so
// consecutive calls need one barrier each (a wave can only rewrite a buffer after every wave has
// passed the barrier of the call in between, i.e. finished reading it).
template <int NT>
__device__ __forceinline__ int block_sum_waves(int v, int* buf, int lane, int wid) {
  static_assert(NT / 64 <= 16, "one 16-lane DPP row holds the wave sums");
  if (lane == 0) buf[wid] = v;
  __syncthreads();
  const int s = row_scan16(lane < NT / 64 ? buf[lane] : 0);  // lanes 0..NW-1 = waves
  return __builtin_amdgcn_readlane(s, NT / 64 - 1);
}

// No-straddling-tie fast path (32-bit keys): the k-th smallest key T by bisection over the key
// values (the row's keys held in registers, one ballot count per step), with c_le = #keys <= T.
// If c_le == k, every key <= T is kept and every other key is not, whatever order libstdc++'s
// sort / nth_element / partial_sort would leave tied elements in -- the first-k SET is fixed by
// the values alone.  fp32 norms essentially never tie at the boundary, so
// this replaces the partition chain for them; bf16 / fp16 rows (tied in nearly every head) skip
// it.  Returns true (and emits) when it applies.
// With `radix`, `hist` (512 ints of LDS scratch: the rank tables, unused before the chain) T is found by
// a radix select over the offsets key - min instead: 8-bit digits from the top, one 256-bin LDS
// histogram of the keys still in the k-th key's bucket per digit (two buffers, each zeroed a pass
// ahead), wave 0 locating the bucket -- two barriers per 8 bits instead of one per bit.
template <int NT, int JM, typename KeyT, bool TO_LDS>
__device__ __forceinline__ bool select_fast_untied(const KeyT* key, int n, int k, SelScalars<KeyT>& sc,
                                   int32_t* out, uint16_t* sel, int* hist, bool radix) {
  const int tid = threadIdx.x, lane = tid & 63, wid = (NT == 64) ? 0 : uni(tid >> 6);
  const int J = (n + NT - 1) / NT;
  if (J > JM) return false;
  const int wbeg = wid * J * 64;
  // the row's keys in registers (every loop below is fully unrolled and predicated on j < J:
  // a runtime trip count would turn kv[] into indexed register accesses)
  uint32_t kv[JM];
  uint32_t mn = 0xFFFFFFFFu, mx = 0u;
#pragma unroll
  for (int j = 0; j < JM; ++j) {
    const int pos = wbeg + j * 64 + lane;
    const bool v = j < J && pos < n;
    kv[j] = v ? (uint32_t)key[min(pos, n - 1)] : 0xFFFFFFFFu;
    mn = v ? min(mn, kv[j]) : mn;
    mx = v ? max(mx, kv[j]) : mx;
  }
  // block min / max of the keys: the bisection range
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
  }
  if (lane == 0) {
    sc.wa[wid] = (int)mn;
    sc.wb[wid] = (int)mx;
  }
  __syncthreads();
  uint32_t lo = 0xFFFFFFFFu, hi = 0u;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    lo = min(lo, (uint32_t)sc.wa[w]);
    hi = max(hi, (uint32_t)sc.wb[w]);
  }
  lo = (uint32_t)uni((int)lo);
  hi = (uint32_t)uni((int)hi);
  __syncthreads();  // sc.wa / sc.wb are the count buffers below
  int c_le = n, parity = 0;
  if (radix) {
    const uint32_t span = hi - lo;
    int rem = span ? 32 - __builtin_clz(span) : 0;  // offset bits still undecided
    uint32_t prefix = 0;  // the decided high bits of the k-th key's offset
    int below = 0;        // #keys whose offset lies below the bucket `prefix`
    for (int i = tid; i < 512; i += NT) hist[i] = 0;
    __syncthreads();
    while (rem > 0) {
      const int w = min(8, rem), sh = rem - w;
      int* h = hist + 256 * parity;
#pragma unroll
      for (int j = 0; j < JM; ++j) {
        const int pos = wbeg + j * 64 + lane;
        const uint32_t d = kv[j] - lo;
        if (j < J && pos < n && (uint32_t)((uint64_t)d >> rem) == prefix)
          lds_add1(h + ((d >> sh) & ((1u << w) - 1u)));
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      // the other buffer's last reader (wave 0, previous pass) finished before the last barrier
      for (int i = tid; i < 256; i += NT) hist[256 * (parity ^ 1) + i] = 0;
      __syncthreads();
      if (wid == 0) {
        const int c0 = h[4 * lane], c1 = h[4 * lane + 1], c2 = h[4 * lane + 2],
                  c3 = h[4 * lane + 3];
        const int s4 = c0 + c1 + c2 + c3;
        const int ex = block_exclusive_scan<64>(s4, nullptr, lane, 0);
        const int need = k - below;  // >= 1: the k-th key lies in this bucket
        const uint64_t b = __builtin_amdgcn_ballot_w64(ex + s4 >= need);
        if (lane == (b ? __builtin_ctzll(b) : 63)) {
          int c = ex, bin = 4 * lane, cnt = c0;
          if (c + c0 < need) {
            c += c0; ++bin; cnt = c1;
            if (c + c1 < need) {
              c += c1; ++bin; cnt = c2;
              if (c + c2 < need) { c += c2; ++bin; cnt = c3; }
            }
          }
          // published in slots the emission below never writes (it writes sc.wm[wid] while a
          // lagging wave may still read this pass's values)
          sc.wa[0] = bin;
          sc.wb[0] = below + c;
          sc.fnan[0] = cnt;
        }
      }
      __syncthreads();
      prefix = (prefix << w) | (uint32_t)sc.wa[0];
      below = sc.wb[0];
      c_le = below + sc.fnan[0];
      rem = sh;
      parity ^= 1;
    }
    lo = lo + prefix;
  }
  // smallest v with #(key <= v) >= k; invariant c_le = #(key <= hi) (= n at hi = max key)
  while (!radix && lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    int cl = 0;  // per-lane count (VALU), one wave reduction per step
#pragma unroll
    for (int j = 0; j < JM; ++j) cl += (kv[j] <= mid) ? 1 : 0;  // invalid slots hold ~0u
    const int rs = row_scan16(cl);
    const int c = __builtin_amdgcn_readlane(rs, 15) + __builtin_amdgcn_readlane(rs, 31) +
                  __builtin_amdgcn_readlane(rs, 47) + __builtin_amdgcn_readlane(rs, 63);
    const int tot = block_sum_waves<NT>(c, parity ? sc.wb : sc.wa, lane, wid);
    parity ^= 1;
    if (tot >= k) {
      hi = mid;
      c_le = tot;
    } else {
      lo = mid + 1;
    }
  }
  if (c_le != k) {
    __syncthreads();  // the chain reuses sc
    return false;
  }
  // ---- emit {pos : key[pos] <= T} ascending ----
  const uint32_t T = lo;
  uint32_t fm = 0;  // kept flags by j
  int c = 0;
#pragma unroll
  for (int j = 0; j < JM; ++j) {
    const int pos = wbeg + j * 64 + lane;
    const bool f = j < J && pos < n && kv[j] <= T;
    fm |= f ? (1u << j) : 0u;
    c += __popcll(__builtin_amdgcn_ballot_w64(f));
  }
  if (lane == 0) sc.wm[wid] = c;
  __syncthreads();
  int run = 0;
  for (int w = 0; w < wid; ++w) run += sc.wm[w];
#pragma unroll
  for (int j = 0; j < JM; ++j) {
    const int pos = wbeg + j * 64 + lane;
    const bool f = (fm >> j) & 1u;
    const uint64_t bf = __builtin_amdgcn_ballot_w64(f);
    if (f) {
      const int r = run + __popcll(bf & lanemask_lt(lane));
      if constexpr (TO_LDS) sel[r] = (uint16_t)pos;
      else out[r] = pos;
    }
    run += __popcll(bf);
  }
  return true;
}

// KVC_ALGO_STABLE (opt-in, not the reference's tie order): the first k of a STABLE sort of the
// row's keys -- every key below T, the k-th smallest key, then the first k - #(key < T) keys
// equal to T in position order.  T by a radix select (8-bit digits of key - min from the top, a
// 256-bin LDS histogram per digit in `hist`, 512 ints: one digit for a bf16 norm row, whose keys
// span < 256 codes) or, for rows whose scratch is shorter, by bisection over the key range; then
// one flag pass and the ascending emission (output slot of a kept position = #(key < T before
// it) + min(#(key == T before it), need)).  Lane positions wid*J*64 + j*64 + lane, j < J <= JM:
// every pass re-reads the keys from LDS with its JM loads issued back to back (nothing but two
// flag words held across barriers).  `sel` must not alias the keys.
template <int NT, int JM, typename KeyT, bool TO_LDS>
__device__ __forceinline__ void stable_select(const KeyT* key, int n, int k, SelScalars<KeyT>& sc,
                                              int32_t* out, uint16_t* sel, int* hist, bool radix,
                                              uint64_t* stamps = nullptr) {
  const int tid = threadIdx.x, lane = tid & 63, wid = (NT == 64) ? 0 : uni(tid >> 6);
  const int J = (n + NT - 1) / NT;
  const int base = wid * J * 64 + lane;
  const int jv = base < n ? min(J, (n - base + 63) >> 6) : 0;  // this lane's valid j
  constexpr int CH = JM < 16 ? JM : 16;  // loads issued together per pass step
  uint32_t mn = 0xFFFFFFFFu, mx = 0u;
#pragma unroll
  for (int j0 = 0; j0 < JM; j0 += CH) {
    uint32_t x[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) x[j] = j0 + j < jv ? (uint32_t)key[base + (j0 + j) * 64] : 0u;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      mn = j0 + j < jv ? min(mn, x[j]) : mn;
      mx = j0 + j < jv ? max(mx, x[j]) : mx;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
  }
  if (lane == 0) {
    sc.wa[wid] = (int)mn;
    sc.wb[wid] = (int)mx;
  }
  if (radix)
    for (int i = tid; i < 512; i += NT) hist[i] = 0;
  __syncthreads();
  uint32_t lo = 0xFFFFFFFFu, hi = 0u;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    lo = min(lo, (uint32_t)sc.wa[w]);
    hi = max(hi, (uint32_t)sc.wb[w]);
  }
  lo = (uint32_t)uni((int)lo);
  hi = (uint32_t)uni((int)hi);
  KVC_STAMP(2);
  int parity = 0;
  if (radix) {
    // the first pass publishes in sc.wa[1] / sc.wb[1], the next in [2] ... (read after its
    // barrier; no slot is rewritten), so the min / max words above may still be being read
    int rem = hi - lo ? 32 - __builtin_clz(hi - lo) : 0;  // offset bits still undecided
    uint32_t prefix = 0;
    int below = 0, slot = 1;
    while (rem > 0) {
      const int w = min(8, rem), sh = rem - w;
      int* h = hist + 256 * parity;
#pragma unroll
      for (int j0 = 0; j0 < JM; j0 += CH) {
        uint32_t x[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) x[j] = j0 + j < jv ? (uint32_t)key[base + (j0 + j) * 64] : 0u;
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const uint32_t d = x[j] - lo;
          if (j0 + j < jv && (rem == 32 ? 0u : d >> rem) == prefix)
            lds_add1(h + ((d >> sh) & ((1u << w) - 1u)));
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      // the other buffer's last reader (wave 0, previous pass) finished before the last barrier
      for (int i = tid; i < 256; i += NT) hist[256 * (parity ^ 1) + i] = 0;
      __syncthreads();
      if (wid == 0) {
        const int c0 = h[4 * lane], c1 = h[4 * lane + 1], c2 = h[4 * lane + 2],
                  c3 = h[4 * lane + 3];
        const int s4 = c0 + c1 + c2 + c3;
        const int ex = block_exclusive_scan<64>(s4, nullptr, lane, 0);
        const int need = k - below;  // >= 1: the k-th key lies in this bucket
        const uint64_t b = __builtin_amdgcn_ballot_w64(ex + s4 >= need);
        if (lane == (b ? __builtin_ctzll(b) : 63)) {
          int c = ex, bin = 4 * lane;
          if (c + c0 < need) {
            c += c0; ++bin;
            if (c + c1 < need) {
              c += c1; ++bin;
              if (c + c2 < need) { c += c2; ++bin; }
            }
          }
          sc.wa[slot] = bin;
          sc.wb[slot] = below + c;
        }
      }
      __syncthreads();
      prefix = (prefix << w) | (uint32_t)sc.wa[slot];
      below = sc.wb[slot];
      ++slot;  // <= 4 passes: slots 1..4 of 16
      rem = sh;
      parity ^= 1;
    }
    lo = lo + prefix;
  } else {
    __syncthreads();  // sc.wa / sc.wb are the bisection's count buffers
  }
  // smallest v with #(key <= v) >= k (bisection; the radix select leaves lo at it)
  while (!radix && lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    int cl = 0;
#pragma unroll
    for (int j0 = 0; j0 < JM; j0 += CH) {
      uint32_t x[CH];
#pragma unroll
      for (int j = 0; j < CH; ++j) x[j] = j0 + j < jv ? (uint32_t)key[base + (j0 + j) * 64] : 0u;
#pragma unroll
      for (int j = 0; j < CH; ++j) cl += (j0 + j < jv && x[j] <= mid) ? 1 : 0;
    }
    const int rs = row_scan16(cl);
    const int c = __builtin_amdgcn_readlane(rs, 15) + __builtin_amdgcn_readlane(rs, 31) +
                  __builtin_amdgcn_readlane(rs, 47) + __builtin_amdgcn_readlane(rs, 63);
    const int tot = block_sum_waves<NT>(c, parity ? sc.wb : sc.wa, lane, wid);
    parity ^= 1;
    if (tot >= k) hi = mid;
    else lo = mid + 1;
  }
  KVC_STAMP(3);
  const uint32_t T = lo;
  typedef typename std::conditional<(JM > 32), uint64_t, uint32_t>::type FlagT;
  FlagT ltm = 0, eqm = 0;  // this lane's flags by j
  int clt = 0, ceq = 0;
#pragma unroll
  for (int j0 = 0; j0 < JM; j0 += CH) {
    uint32_t x[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) x[j] = j0 + j < jv ? (uint32_t)key[base + (j0 + j) * 64] : 0u;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const bool flt = j0 + j < jv && x[j] < T, feq = j0 + j < jv && x[j] == T;
      ltm |= flt ? (FlagT)1 << (j0 + j) : (FlagT)0;
      eqm |= feq ? (FlagT)1 << (j0 + j) : (FlagT)0;
      clt += __popcll(__builtin_amdgcn_ballot_w64(flt));
      ceq += __popcll(__builtin_amdgcn_ballot_w64(feq));
    }
  }
  if (lane == 0) sc.wm[wid] = clt | (ceq << 16);  // each <= kZoneMax < 2^16
  __syncthreads();
  int rlt = 0, req = 0, tlt = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const int x = sc.wm[w];
    rlt += w < wid ? (x & 0xFFFF) : 0;
    req += w < wid ? (x >> 16) : 0;
    tlt += x & 0xFFFF;
  }
  const int need = k - tlt;  // 1 <= need <= #(key == T)
#pragma unroll
  for (int j = 0; j < JM; ++j) {
    const bool flt = (ltm >> j) & 1u, feq = (eqm >> j) & 1u;
    const uint64_t bl = __builtin_amdgcn_ballot_w64(flt), be = __builtin_amdgcn_ballot_w64(feq);
    const int lb = rlt + __popcll(bl & lanemask_lt(lane));
    const int eb = req + __popcll(be & lanemask_lt(lane));
    if (flt || (feq && eb < need)) {
      const int r = lb + min(eb, need);
      if constexpr (TO_LDS) sel[r] = (uint16_t)(base + j * 64);
      else out[r] = base + j * 64;
    }
    rlt += __popcll(bl);
    req += __popcll(be);
  }
}

// Reference-exact selection for one (layer, b, h) row whose zone norms are at `nrow`; working
// arrays at `arrays` (SelArrays layout for n_cap positions and `cap`-rank windows: LDS, or a
// global scratch row for zones longer than kZoneMax) and scalars in `sc`; NT threads (the
// workgroup) cooperate.  Emits the kept zone-local indices in ascending order to `out` (global
// int32) or, with TO_LDS, to `sel` (LDS u16, may alias the key region: keys are dead by then).
// Returns false (and ORs KVC_DEV_SELECT_BOUNDS into *status) when the row exceeds this kernel's
// zone capacity -- nothing is selected then.
template <int KC, bool TO_LDS, int MAXN, int NT, bool HH = false, bool STABLE = false,
          bool L0T = true>
__device__ __forceinline__ bool select_body(const kvc_layer_t* __restrict__ ly, int dt, int order,
                            int algo, const char* __restrict__ nrow, int32_t* out, uint16_t* sel,
                            char* arrays, int n_cap, int cap,
                            SelScalars<typename DTypeTraits<KC>::key_t>& sc,
                            int wave_seg, uint64_t* stamps, uint32_t* status,
                            const uint32_t* trow = nullptr) {
  typedef typename DTypeTraits<KC>::key_t KeyT;
  constexpr int ESZ = DTypeTraits<KC>::esz;
  constexpr int MAXJ = (MAXN + NT - 1) / NT;  // positions per lane, level 0
  const SelArrays<KeyT> A(arrays, n_cap, cap);
  KeyT* key = A.key;
  uint16_t* idx = A.idx;
  uint16_t* spos = A.spos;
  KVC_STAMP(0);
  const int n = ly->zone_len;
  const int k = ly->n_select;
  if constexpr (!TO_LDS) {
    // A row that keeps its whole zone uses none of the arrays, and its zone may be longer than
    // n_cap: the plan sizes that by the selecting layers alone and accepts a kept zone of any
    // length.  Its index row is the identity.
    if (k > 0 && k >= n) {
      for (int i = threadIdx.x; i < n; i += NT) out[i] = i;
      return true;
    }
  }
  if (n > MAXN || n > n_cap) {  // a dispatch bug, never silent: flag it, select nothing
    if (threadIdx.x == 0 && status) atomicOr(status, (uint32_t)KVC_DEV_SELECT_BOUNDS);
    return false;
  }
  if (k <= 0 || n <= 0) return true;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (k >= n) {  // keep everything (e.g. h2o_l2 when the middle is no longer than heavy_hitter)
    for (int i = tid; i < n; i += NT) {
      if constexpr (TO_LDS) sel[i] = (uint16_t)i;
      else out[i] = i;
    }
    return true;
  }
  const bool desc = order == KVC_DESC;
  const bool topk = algo == KVC_ALGO_TOPK;
  const bool partial = topk && (int64_t)k * 64 <= n;  // aten TopKImpl.h: use_partial_sort
  const int thr = topk ? 3 : 16;  // introselect / introsort segment threshold

  // ---- keys ----
  if (ly->score_mode == KVC_SCORE_SNAPKV) {
    // scratch for the unpooled scores from the idx region on: n u16 (bf16), or n floats over
    // idx + the rank tables (fp32 rows always get full n/2-rank tables: >= 4n bytes)
    char* tmp = reinterpret_cast<char*>(idx);
    if constexpr (ESZ == 2 && MAXN <= kZoneMax) {
      constexpr int MAXV = (MAXN / 8 + NT - 1) / NT;
      bool idx_done = false;
      with_dt<KC>(dt, [&](auto D) {
        idx_done = snapkv_keys16<D.value, NT, MAXV>(nrow, trow, n, ly->pool_kernel, desc,
                                                    reinterpret_cast<uint16_t*>(key), idx,
                                                    reinterpret_cast<uint16_t*>(tmp), sc, stamps);
      });
      if (!idx_done) {
        __syncthreads();  // the scores (in the idx region) are dead
        for (int v = tid; v < (n + 7) / 8; v += NT) {
          const uint32_t b = (uint32_t)v * 8;
          reinterpret_cast<uint4*>(idx)[v] =
              make_uint4(b | (b + 1) << 16, (b + 2) | (b + 3) << 16, (b + 4) | (b + 5) << 16,
                         (b + 6) | (b + 7) << 16);
        }
      }
    } else {
      with_dt<KC>(dt, [&](auto D) {
        snapkv_keys<D.value, KeyT, NT>(nrow, n, ly->pool_kernel, desc, key, tmp, sc);
      });
      __syncthreads();
      for (int i = tid; i < n; i += NT) idx[i] = (uint16_t)i;
    }
  } else {
    // 16-B loads, all issued before the first use (norm rows are padded to 64 elements, so a
    // whole vector past n stays inside the row); keys/indices written as 16-B LDS stores
    constexpr int VEC = 16 / ESZ;
    constexpr int MAXV = ((MAXN < kZoneMax ? MAXN : kZoneMax) / VEC + NT - 1) / NT;  // per batch
    const int nvec = (n + VEC - 1) / VEC;
    for (int v0 = 0; v0 < nvec; v0 += MAXV * NT) {  // one batch for n <= kZoneMax
    uint4 buf[MAXV];
#pragma unroll
    for (int q = 0; q < MAXV; ++q) {
      const int v = v0 + tid + q * NT;
      if (v < nvec) buf[q] = reinterpret_cast<const uint4*>(nrow)[v];
    }
#pragma unroll
    for (int q = 0; q < MAXV; ++q) {
      const int v = v0 + tid + q * NT;
      if (v < nvec) {
        const uint32_t w[4] = {buf[q].x, buf[q].y, buf[q].z, buf[q].w};
        uint32_t kw[4], iw[4];
        if constexpr (KC != KVC_F32) {
          // packed key map (key_h16x2): key_h16's order and ties, other codes -- every key of
          // the row is made here, and the selection only compares keys with each other
          const uint32_t inf = inf_bits16(dt);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            kw[e] = key_h16x2(w[e], desc, inf);
            iw[e] = (uint32_t)(v * 8 + 2 * e) | ((uint32_t)(v * 8 + 2 * e + 1) << 16);
          }
          *reinterpret_cast<uint4*>(key + v * 8) = make_uint4(kw[0], kw[1], kw[2], kw[3]);
          *reinterpret_cast<uint4*>(idx + v * 8) = make_uint4(iw[0], iw[1], iw[2], iw[3]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) kw[e] = key_f32(w[e], desc);
          *reinterpret_cast<uint4*>(key + v * 4) = make_uint4(kw[0], kw[1], kw[2], kw[3]);
          *reinterpret_cast<uint2*>(idx + v * 4) =
              make_uint2((uint32_t)(v * 4) | ((uint32_t)(v * 4 + 1) << 16),
                         (uint32_t)(v * 4 + 2) | ((uint32_t)(v * 4 + 3) << 16));
        }
      }
    }
    }
  }
  __syncthreads();
  KVC_STAMP(1);

  // ---- KVC_ALGO_STABLE: the first k of a stable sort (ties in position order) ----
  if constexpr (STABLE) {
    static_assert(MAXJ <= 64, "stable selection: positions per lane (flag words)");
    if constexpr (MAXN > kZoneMax) {
      // the global-scratch variant (zones up to kZoneMaxGlobal): the histograms in LDS
      __shared__ int stable_hist[512];
      stable_select<NT, MAXJ, KeyT, TO_LDS>(key, n, k, sc, out, sel, stable_hist, true, stamps);
    } else {
      // the radix histograms (512 ints) over the idx region and the rank tables, unused here
      // (sel, when in LDS, is the idx region too: written only after the last histogram read);
      // shorter rows bisect over the key range instead
      const bool radix = (size_t)n_cap * 2 + (size_t)(cap + 72) * 4 >= 2048;
      stable_select<NT, MAXJ, KeyT, TO_LDS>(key, n, k, sc, out, sel, reinterpret_cast<int*>(idx),
                                            radix, stamps);
    }
    KVC_STAMP(4);
    return true;
  }

  // ---- reference-exact k-selection ----
  if constexpr (sizeof(KeyT) == 4 && MAXJ <= 16) {  // fp32 keys: untied boundary -> values only
    // (`sel` may alias the key region: the keys are read into registers before any store)
    // the rank tables (>= 2 KiB from n_cap = 1024 on) hold the radix histograms
    const bool radix = (size_t)(cap + 72) * 4 >= 2048;
    if (select_fast_untied<NT, MAXJ, KeyT, TO_LDS>(key, n, k, sc, out, sel,
                                                   reinterpret_cast<int*>(idx + n_cap), radix)) {
      KVC_STAMP(31);  // diagnostic build: fast path taken
      return true;
    }
  }
  if (partial) {  // std::partial_sort's heap select
    bool done = false;
    if constexpr (HH && NT > 64) {  // heavy-hitter kernels only: see heap_candidates
      if (k <= 64 && n >= 4096) {
        // wave 0 builds the register heap while the other waves prefilter the scan's candidates
        // into the rank tables (unused by the heap select); then wave 0 scans only those
        constexpr bool PK = sizeof(KeyT) == 2;
        RegHeap<PK> h;
        if (wid == 0) reg_heap_make(h, key, idx, k);
        uint16_t* cand = idx + n_cap;
        const int nc = heap_candidates<NT>(key, k, n, cand, (cap + 72) * 2, sc.wa, sc.wb, 1);
        if (wid == 0) reg_heap_scan(h, key, idx, k, n, nc >= 0 ? cand : nullptr, nc);
        done = true;
      }
    }
    if (!done && wid == 0) wave_heap_select(key, idx, k, n);
  } else {
    int lo = 0, hi = n, depth = 2 * floor_log2(n), level = 0;
    uint64_t* accb = nullptr;
    uint64_t* accw = nullptr;
#ifdef KVC_STAMPS
    if (stamps) {
      accb = stamps + blockIdx.x * 32 + 5;
      accw = stamps + blockIdx.x * 32 + 10;
      if (tid == 0)
        for (int q = 0; q < 21; ++q) accb[q] = 0;
    }
#endif
    const int st = run_chain<KeyT, NT, MAXJ, L0T>(
        key, idx, spos, A.gpos, sc, k, topk, thr, cap, lo, hi, depth, level, wave_seg, accb, status,
        MAXJ <= 16 ? n_cap / 2 : 0);
    KVC_STAMP(2);
    if (st == 1 && wid == 0)
      run_chain<KeyT, 64, 16>(key, idx, spos, A.gpos, sc, k, topk, thr, cap, lo, hi, depth,
                              level, wave_seg, accw, status);
  }
  __syncthreads();
  KVC_STAMP(3);

  // ---- emit the kept set {idx[0..k)} as ascending zone-local indices: a bitmap of the kept
  // positions over the (dead) key region, one block scan of per-thread popcounts, and each
  // thread writing the positions of its words.  Every bitmap word is in registers before the
  // scan's barrier, so `sel` (which aliases the key region) is only written after it.
  uint32_t* bm = reinterpret_cast<uint32_t*>(key);
  const int nw = (n + 31) >> 5;
  for (int w = tid; w < nw; w += NT) bm[w] = 0u;
  __syncthreads();
  for (int i = tid; i < k; i += NT) {
    const int x = idx[i];
    atomicOr(&bm[x >> 5], 1u << (x & 31));
  }
  __syncthreads();
  constexpr int MAXW = (MAXN / 32 + NT - 1) / NT;  // bitmap words per thread
  uint32_t wv[MAXW];
  int cnt = 0;
#pragma unroll
  for (int q = 0; q < MAXW; ++q) {
    const int w = tid * MAXW + q;
    wv[q] = w < nw ? bm[w] : 0u;
    cnt += __popc(wv[q]);
  }
  int r = block_exclusive_scan<NT>(cnt, sc.wa, lane, wid);
#pragma unroll
  for (int q = 0; q < MAXW; ++q) {
    const int base = (tid * MAXW + q) * 32;
    for (uint32_t b = wv[q]; b; b &= b - 1u, ++r) {
      const int pos = base + (int)__builtin_ctz(b);
      if constexpr (TO_LDS) sel[r] = (uint16_t)pos;
      else out[r] = pos;
    }
  }
  KVC_STAMP(4);
  return true;
}


// One workgroup of NT threads per (layer, b, h) row.  NT = 256 for zones up to 4 096
// positions, arrays in dynamic LDS sized by the call's longest zone (n_cap): several rows per
// CU.  NT = 1 024 beyond, arrays in static LDS laid out for kZoneMax (compile-time addresses)
// with rank windows of kSelCapBig: two rows per CU for bf16.
template <typename KeyT>
constexpr int kSelCapBig = sel_cap(kZoneMax, (int)sizeof(KeyT), kBigBudget);
template <typename KeyT>
constexpr int kSelBytesBig = (int)sel_bytes(kZoneMax, (int)sizeof(KeyT), kSelCapBig<KeyT>);

// 8 waves per SIMD: two 1024-thread rows per CU (fp32 rows of the big kernel: one per CU, LDS).
// HH: the heavy-hitter instance (kvc_heavy_hitters), whose heap selects prefilter their scan.
template <int KC, int NT, bool HH = false, bool STABLE = false>
__global__ void __launch_bounds__(NT, sel_waves_per_eu(KC, NT, HH))
    select_kernel(const LayerChunk T, int BH, int dt, int order, int algo,
                  const char* __restrict__ norms, int64_t norm_stride,
                  int32_t* __restrict__ out_idx, int64_t idx_stride, int wave_seg, int n_cap,
                  int cap, uint64_t* stamps, uint32_t* status, const uint32_t* __restrict__ tmax) {
  typedef typename DTypeTraits<KC>::key_t KeyT;
  constexpr int ESZ = DTypeTraits<KC>::esz;
  constexpr int MAXN = NT == kSelThreads ? kZoneMax : NT * 16;
  __shared__ SelScalars<KeyT> sc;
  const kvc_layer_t* ly = T.l + blockIdx.x / BH;
  const int row = ly->row0 + (int)(blockIdx.x % BH);  // global workspace row
  const uint32_t* trow = tmax ? tmax + (int64_t)row * (norm_stride / kTile) : nullptr;
  if constexpr (NT == kSelThreads) {
    // LDS: key[kZoneMax] | idx[kZoneMax] (u16) | spos | gpos (u16 rank windows) -- SelArrays
    __shared__ __attribute__((aligned(16))) char smem[kSelBytesBig<KeyT>];
    select_body<KC, false, MAXN, NT, HH, STABLE>(ly, dt, order, algo,
                                     norms + (int64_t)row * norm_stride * ESZ,
                                     out_idx + (int64_t)row * idx_stride, nullptr, smem, kZoneMax,
                                     kSelCapBig<KeyT>, sc, wave_seg, stamps, status, trow);
  } else {
    extern __shared__ __attribute__((aligned(16))) char dsmem[];
    select_body<KC, false, MAXN, NT, HH, STABLE>(ly, dt, order, algo,
                                     norms + (int64_t)row * norm_stride * ESZ,
                                     out_idx + (int64_t)row * idx_stride, nullptr, dsmem, n_cap,
                                     cap, sc, wave_seg, stamps, status, trow);
  }
}

// Zones longer than kZoneMax (up to kZoneMaxGlobal): the same selection with its arrays in a
// per-row global scratch (L2 / Infinity-Cache resident; a workgroup barrier orders the
// workgroup's global accesses like LDS ones -- all its waves share one CU's L1).
template <int KC, bool STABLE = false>
__global__ void __launch_bounds__(kSelThreads)
    select_global_kernel(const LayerChunk T, int BH, int dt, int order, int algo,
                         const char* __restrict__ norms, int64_t norm_stride,
                         int32_t* __restrict__ out_idx, int64_t idx_stride, int wave_seg,
                         char* __restrict__ scratch, int64_t scratch_row_bytes, int n_cap,
                         uint32_t* status) {
  typedef typename DTypeTraits<KC>::key_t KeyT;
  constexpr int ESZ = DTypeTraits<KC>::esz;
  __shared__ SelScalars<KeyT> sc;
  const kvc_layer_t* ly = T.l + blockIdx.x / BH;
  const int row = ly->row0 + (int)(blockIdx.x % BH);
  select_body<KC, false, kZoneMaxGlobal, kSelThreads, false, STABLE>(
      ly, dt, order, algo, norms + (int64_t)row * norm_stride * ESZ,
      out_idx + (int64_t)row * idx_stride, nullptr, scratch + (int64_t)row * scratch_row_bytes,
      n_cap, n_cap / 2 + 1, sc, wave_seg, nullptr, status);
}

// Zones longer than kZoneMaxGlobal (up to kZoneMaxLong): the same partition chain with u32
// positions and full rank tables in a per-row global scratch
//   key[n_cap] | idx[n_cap] (u32) | spos[n_cap/2 + 2] (u32) | gpos[n_cap/2 + 2] (u32)
// Too many positions per lane to keep a level's flags in registers, so each pass re-derives
// them from the keys (the keys do not change between a level's passes: the median move and the
// swaps run after the last one); counts are plain ints.  Rare, long rows: simplicity over speed.
__host__ __device__ constexpr size_t sel_long_bytes(int n_cap, int key_size) {
  return (size_t)n_cap * key_size + (size_t)n_cap * 4 + 2 * (size_t)(n_cap / 2 + 2) * 4;
}

struct LongScalars {
  int ge[kSelWaves];
  int le[kSelWaves];
  int nsw[kSelWaves];
  int ff[kSelWaves];
};

// One level over [lo, hi) (see run_chain for the algorithm); returns cut.
template <typename KeyT>
__device__ int partition_long(KeyT* key, uint32_t* idx, uint32_t* spos, uint32_t* gpos,
                              LongScalars& sc, int lo, int hi) {
  const int tid = threadIdx.x, lane = tid & 63, wid = uni(tid >> 6);
  const int a = lo + 1, b = lo + (hi - lo) / 2, c = hi - 1;
  const uint32_t ka = (uint32_t)uni((int)key[a]), kb = (uint32_t)uni((int)key[b]);
  const uint32_t kc = (uint32_t)uni((int)key[c]), klo = (uint32_t)uni((int)key[lo]);
  int ch;  // std::__move_median_to_first(lo, a, b, c)
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
  const int J = (hi - lo - 1 + kSelThreads - 1) / kSelThreads;
  const int wbeg = lo + 1 + wid * J * 64;
  const int half = (hi - lo) / 2 + 1;  // swapped ranks m <= (n - 1) / 2
  // ---- P1: wave counts of ge / le positions ----
  int cge = 0, cle = 0;
  for (int j = 0; j < J; ++j) {
    const int pos = wbeg + j * 64 + lane;
    const bool inb = pos < hi;
    const uint32_t kk = inb ? (pos == ch ? klo : (uint32_t)key[pos]) : 0u;
    cge += __popcll(__builtin_amdgcn_ballot_w64(inb && kk >= p));
    cle += __popcll(__builtin_amdgcn_ballot_w64(inb && kk <= p));
  }
  if (lane == 0) {
    sc.ge[wid] = cge;
    sc.le[wid] = cle;
  }
  __syncthreads();
  int ge_before = 0, le_before = 0, tot_le = 0;
  for (int w = 0; w < kSelWaves; ++w) {
    const int g = sc.ge[w], l = sc.le[w];
    ge_before += w < wid ? g : 0;
    le_before += w < wid ? l : 0;
    tot_le += l;
  }
  // ---- P2: rank -> position tables, swap count, first unswapped ge ----
  int rge = ge_before, rle = le_before, nsw = 0, ff = kBig;
  for (int j = 0; j < J; ++j) {
    const int pos = wbeg + j * 64 + lane;
    const bool inb = pos < hi;
    const uint32_t kk = inb ? (pos == ch ? klo : (uint32_t)key[pos]) : 0u;
    const bool ge = inb && kk >= p, le = inb && kk <= p;
    const uint64_t bg = __builtin_amdgcn_ballot_w64(ge), bl = __builtin_amdgcn_ballot_w64(le);
    const int A = mbcnt(bg, rge);
    const int lin = mbcnt(bl, rle) + (le ? 1 : 0);
    const bool cond = A + lin < tot_le;
    const int sr = tot_le - lin + 1;
    if (le && sr <= half) spos[sr] = (uint32_t)pos;
    if (ge && cond) gpos[A + 1] = (uint32_t)pos;
    const uint64_t bc = __builtin_amdgcn_ballot_w64(cond);
    nsw += __popcll(bg & bc);
    const uint64_t bf = bg & ~bc;
    ff = min(ff, bf ? wbeg + j * 64 + (int)__builtin_ctzll(bf) : kBig);
    rge += __popcll(bg);
    rle += __popcll(bl);
  }
  if (lane == 0) {
    sc.nsw[wid] = nsw;
    sc.ff[wid] = ff;
  }
  __syncthreads();
  int msw = 0, gnext = kBig;
  for (int w = 0; w < kSelWaves; ++w) {
    msw += sc.nsw[w];
    gnext = min(gnext, sc.ff[w]);  // stripes ascend with the wave id
  }
  if (tid == 0) kv_swap(key, idx, lo, ch);  // the median move, made physical
  __syncthreads();
  // ---- P4: the m disjoint swaps g_t <-> s_t ----
  for (int t = tid + 1; t <= msw; t += kSelThreads) {
    const int g = (int)gpos[t], sv = (int)spos[t];
    const KeyT kg = key[g], ks = key[sv];
    const uint32_t ig = idx[g], is = idx[sv];
    key[g] = ks;
    key[sv] = kg;
    idx[g] = is;
    idx[sv] = ig;
  }
  const int cut = min(gnext, msw > 0 ? (int)spos[msw] : kBig);
  __syncthreads();  // tables and counters are reused by the next level
  return cut;
}

// The selection of workspace row `row`, whose zone_len, n_select, score_mode and pool_kernel are
// ly's (the layer's, or a ragged row's own: kvc_ragged.h); ssc / sc: the kernel's LDS scalars.
template <int KC>
__device__ __forceinline__ void select_long_body(
    const kvc_layer_t* ly, int row, int dt, int order, int algo, const char* __restrict__ norms,
    int64_t norm_stride, int32_t* __restrict__ out_idx, int64_t idx_stride,
    char* __restrict__ scratch, int64_t scratch_row_bytes, int n_cap, uint32_t* status,
    SelScalars<typename DTypeTraits<KC>::key_t>& ssc, LongScalars& sc) {
  typedef typename DTypeTraits<KC>::key_t KeyT;
  constexpr int ESZ = DTypeTraits<KC>::esz;
  const int n = ly->zone_len, k = ly->n_select;
  int32_t* out = out_idx + (int64_t)row * idx_stride;
  if (k > 0 && k >= n) {  // keeps its whole zone: no scratch, any length (as in select_body)
    for (int i = threadIdx.x; i < n; i += kSelThreads) out[i] = i;
    return;
  }
  if (n > n_cap || n > kZoneMaxLong) {
    if (threadIdx.x == 0 && status) atomicOr(status, (uint32_t)KVC_DEV_SELECT_BOUNDS);
    return;
  }
  if (k <= 0 || n <= 0) return;
  const char* nrow = norms + (int64_t)row * norm_stride * ESZ;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  char* base = scratch + (int64_t)row * scratch_row_bytes;
  KeyT* key = reinterpret_cast<KeyT*>(base);
  uint32_t* idx = reinterpret_cast<uint32_t*>(base + (size_t)n_cap * sizeof(KeyT));
  uint32_t* spos = idx + n_cap;
  uint32_t* gpos = spos + (n_cap / 2 + 2);
  const bool desc = order == KVC_DESC;
  if (ly->score_mode == KVC_SCORE_SNAPKV) {  // unpooled scores in the idx region first
    with_dt<KC>(dt, [&](auto D) {
      snapkv_keys<D.value, KeyT, kSelThreads>(nrow, n, ly->pool_kernel, desc, key,
                                              reinterpret_cast<char*>(idx), ssc);
    });
    __syncthreads();
  } else {
    for (int i = tid; i < n; i += kSelThreads) {
      if constexpr (KC == KVC_F32)
        key[i] = key_f32(reinterpret_cast<const uint32_t*>(nrow)[i], desc);
      else
        key[i] = key_h16(reinterpret_cast<const uint16_t*>(nrow)[i], desc, inf_bits16(dt));
    }
  }
  for (int i = tid; i < n; i += kSelThreads) idx[i] = (uint32_t)i;
  __syncthreads();
  const bool topk = algo == KVC_ALGO_TOPK;
  if (topk && (int64_t)k * 64 <= n) {  // std::partial_sort's heap select (one wave)
    if (wid == 0) wave_heap_select(key, idx, k, n);
  } else {
    const int thr = topk ? 3 : 16;
    int lo = 0, hi = n, depth = 2 * floor_log2(n);
    while (true) {
      if (lo == k || hi == k) break;
      if (hi - lo <= thr) {
        if (tid == 0) insertion_sort(key, idx, lo, hi);
        break;
      }
      if (depth == 0) {
        if (tid == 0) {
          if (topk) {
            heap_select(key + lo, idx + lo, k - lo, hi - lo);
            kv_swap(key, idx, lo, k - 1);
          } else {
            make_heap(key + lo, idx + lo, hi - lo);
            sort_heap(key + lo, idx + lo, hi - lo);
          }
        }
        break;
      }
      --depth;
      const int cut = partition_long<KeyT>(key, idx, spos, gpos, sc, lo, hi);
      if (topk) {
        if (cut <= k - 1) lo = cut; else hi = cut;
      } else {
        if (k <= cut) hi = cut; else lo = cut;
      }
    }
  }
  __syncthreads();
  // ---- emit {idx[0..k)} ascending: u16 flags over the (dead) key region, two counted passes
  uint16_t* flag = reinterpret_cast<uint16_t*>(key);
  for (int i = tid; i < n; i += kSelThreads) flag[i] = 0;
  __syncthreads();
  for (int i = tid; i < k; i += kSelThreads) flag[idx[i]] = 1;
  __syncthreads();
  const int J = (n + kSelThreads - 1) / kSelThreads;
  const int wbeg = wid * J * 64;
  int c = 0;
  for (int j = 0; j < J; ++j) {
    const int pos = wbeg + j * 64 + lane;
    c += __popcll(__builtin_amdgcn_ballot_w64(pos < n && flag[pos] != 0));
  }
  if (lane == 0) sc.ge[wid] = c;
  __syncthreads();
  int run = 0;
  for (int w = 0; w < wid; ++w) run += sc.ge[w];
  for (int j = 0; j < J; ++j) {
    const int pos = wbeg + j * 64 + lane;
    const bool f = pos < n && flag[pos] != 0;
    const uint64_t bf = __builtin_amdgcn_ballot_w64(f);
    if (f) out[run + __popcll(bf & lanemask_lt(lane))] = pos;
    run += __popcll(bf);
  }
}

template <int KC>
__global__ void __launch_bounds__(kSelThreads)
    select_long_kernel(const LayerChunk T, int BH, int dt, int order, int algo,
                       const char* __restrict__ norms, int64_t norm_stride,
                       int32_t* __restrict__ out_idx, int64_t idx_stride,
                       char* __restrict__ scratch, int64_t scratch_row_bytes, int n_cap,
                       uint32_t* status) {
  __shared__ SelScalars<typename DTypeTraits<KC>::key_t> ssc;
  __shared__ LongScalars sc;
  const kvc_layer_t* ly = T.l + blockIdx.x / BH;
  select_long_body<KC>(ly, ly->row0 + (int)(blockIdx.x % BH), dt, order, algo, norms, norm_stride,
                       out_idx, idx_stride, scratch, scratch_row_bytes, n_cap, status, ssc, sc);
}

}  // namespace kvc
