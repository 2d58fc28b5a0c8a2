// kvc_device_util.h -- what every kernel of kvc.hip shares: constants, dtype traits, wave-level
// helpers, and the layout of the selection's working set.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "kvc.h"
#include "kvc_common.h"

namespace kvc {

constexpr int kTile = 64;  // tokens per score tile (one per lane)
constexpr int kSelThreads = 1024;
constexpr int kSelWaves = kSelThreads / 64;
// Zones of up to kSmallZone positions select with 512-thread workgroups and LDS sized by the
// call's longest zone, at most kSmallBudget bytes: four rows per CU (all 1 024 rows of a
// 32-layer call resident at once), a row's copy phase with 8 waves of loads in flight
// (256-thread rows: SELECT_GATHER 0.129 ms at S = 4 096, 0.104 ms at S = 513; 512: 0.115 /
// 0.096).  Up to 8 192 positions the budget holds the bf16 / fp16 rows with rank windows
// (profiles/r03_d_small_path_rows_per_cu_ab.jsonl, S = 8 192: 0.137 ms with 1 024-thread rows
// two per CU, 0.148 ms with 512-thread rows three per CU and full tables, 0.1265 ms four per CU
// with windows).  Longer zones keep 1 024 threads.
constexpr int kSelThreadsSmall = 512;
constexpr int kSmallZone = 8192;
// occupancy the select kernels ask the compiler for (waves per SIMD)
// (the heavy-hitter select kernels run one row per CU: no occupancy target to spill for)
constexpr int sel_waves_per_eu(int kc, int nt, bool hh = false) {
  return hh || (kc == KVC_F32 && nt == kSelThreads) ? 4 : 8;
}
constexpr long kSmallBudget = 40448;  // 4 x (this + scalars) <= 160 KiB of LDS per CU
constexpr long kBigBudget = 81408;    // 2 x (this + scalars) <= 160 KiB
constexpr int kZoneMax = 16384;        // longest zone whose selection runs from LDS
constexpr int kZoneMaxGlobal = 65536;  // longest zone of the u16-position global variant
constexpr int kZoneMaxLong = 1 << 24;   // longest zone at all (u32 positions; global scratch)
constexpr int kWaveSeg = 256;  // segments this short are finished by one wave (64 / 128 / 512 / 1024 measured slower)
// the same for 512-thread rows (128 / 512 / 1 024 measured the same or slower at S = 4 096 and
// 8 192: profiles/r03_g_small_wave_threshold_ab.jsonl)
constexpr int kWaveSegSmall = 256;
constexpr int kGatherThreads = 256;
constexpr int kGatherTokens = 64;  // output tokens per gather block
constexpr int kBig = 0x7FFFFFFF;
// Layer tables travel to the score / select / gather kernels BY VALUE in the kernel arguments
// (chunks of kArgLayers, 8.7 KiB): no host->device table copy, whose completion would stand
// ~10 us between the copy and the first kernel of every call.
constexpr int kArgLayers = 64;
// SELECT_GATHER launches of at most this many rows (fewer than the 256 CUs: one row per CU)
// copy each row's sink / tail rows in a second workgroup beside the selecting one
constexpr int kSplitCopyRows = 255;
struct LayerChunk {
  kvc_layer_t l[kArgLayers];
};

template <int DT>
struct DTypeTraits;
template <>
struct DTypeTraits<KVC_BF16> {
  static constexpr int esz = 2;
  typedef uint16_t key_t;
};
template <>
struct DTypeTraits<KVC_F16> {
  static constexpr int esz = 2;
  typedef uint16_t key_t;
};
template <>
struct DTypeTraits<KVC_F32> {
  static constexpr int esz = 4;
  typedef uint32_t key_t;
};
// fp8 (OCP e4m3fn / e5m2) STORAGE: 1-byte elements that only SCORE decodes and GATHER moves as
// bytes.  Everything behind SCORE -- the norm region, the tile maxima, the sort keys -- is that of
// the exact bf16 upcast: the SCORE dtype below.
template <>
struct DTypeTraits<KVC_F8E4M3> {
  static constexpr int esz = 1;
  typedef uint16_t key_t;
};
template <>
struct DTypeTraits<KVC_F8E5M2> {
  static constexpr int esz = 1;
  typedef uint16_t key_t;
};
__host__ __device__ constexpr bool is_fp8(int dt) { return dt == KVC_F8E4M3 || dt == KVC_F8E5M2; }
// The dtype a storage dtype's keys are scored, stored in the norm region and selected in.
__host__ __device__ constexpr int score_dt(int dt) { return is_fp8(dt) ? KVC_BF16 : dt; }

template <int DT>
__device__ __forceinline__ float load_dt(const char* base, int i) {
  if constexpr (DT == KVC_BF16)
    return bf16_to_f32(reinterpret_cast<const uint16_t*>(base)[i]);
  else if constexpr (DT == KVC_F16)
    return f16_to_f32(reinterpret_cast<const uint16_t*>(base)[i]);
  else
    return reinterpret_cast<const float*>(base)[i];
}

// storage bits of an fp32 value rounded to a 16-bit dtype (c10 conversions)
template <int DT>
__device__ __forceinline__ uint32_t bits16_dt(float f) {
  if constexpr (DT == KVC_BF16)
    return f32_to_bf16_rne(f);
  else
    return f32_to_f16_rne(f);
}

template <int DT>
__device__ __forceinline__ float round_dt(float f) {
  if constexpr (DT == KVC_BF16)
    return bf16_to_f32(f32_to_bf16_rne(f));
  else if constexpr (DT == KVC_F16)
    return f16_to_f32(f32_to_f16_rne(f));
  else
    return f;
}

// sort key of a 16-bit storage pattern
template <int DT>
__device__ __forceinline__ uint16_t key16_dt(uint32_t bits, bool desc) {
  if constexpr (DT == KVC_BF16)
    return key_bf16(bits, desc);
  else
    return key_f16(bits, desc);
}

template <int DT>
__device__ __forceinline__ typename DTypeTraits<DT>::key_t key_of(float f, bool desc) {
  if constexpr (DT == KVC_F32)
    return key_f32(f32_to_bits(f), desc);
  else
    return key16_dt<DT>(bits16_dt<DT>(f), desc);
}

// Selection kernels are compiled per KEY CLASS (KC): KVC_BF16 stands for every 16-bit storage
// dtype (u16 keys), KVC_F32 for fp32 (u32 keys).  bf16 and fp16 rows run the same binary with the
// storage dtype as a runtime argument: the two differ only in the NaN threshold of the key map
// and in the float conversions of the snapkv scores.  (Two instantiations of identical source
// compiled ~2x apart in speed -- DESIGN.md "fp16 selection".)  f(integral_constant<int, DT>)
// runs with the row's storage dtype.
template <int KC, typename F>
__device__ __forceinline__ void with_dt(int dt, F&& f) {
  if constexpr (KC == KVC_F32)
    f(std::integral_constant<int, KVC_F32>());
  else if (dt == KVC_F16)
    f(std::integral_constant<int, KVC_F16>());
  else
    f(std::integral_constant<int, KVC_BF16>());
}
__device__ __forceinline__ uint32_t inf_bits16(int dt) { return dt == KVC_F16 ? 0x7C00u : 0x7F80u; }

// torch.gather's NaN rewrite on two 16-bit elements (kvc_common.h canon_nan_bf16x2 /
// canon_nan_f16x2) in five packed-u16 VALU ops instead of two compare/select chains:
// x = |w| per half; x + (0xFFFE - NANMIN) saturates to 0xFFFF exactly for x > NANMIN (a NaN);
// that - 0xFFFE (saturating) is 1 for a NaN half and 0 otherwise, scaled to the bits to set.
// Pinned on the device by the test_nan_payload_gpu suite (every NaN pattern of bf16 / fp16 in
// either half of a word, beside a NaN and a non-NaN half, through every copy kernel); the scalar
// forms are swept over all 65 536 values of each half in test_nan_payload.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
template <uint16_t NANMIN, uint16_t SET>
__device__ __forceinline__ uint32_t canon_nan_pk(uint32_t w) {
  const u16x2 x = __builtin_bit_cast(u16x2, w & 0x7FFF7FFFu);
  const u16x2 m = __builtin_elementwise_add_sat(
      x, (u16x2){(uint16_t)(0xFFFEu - NANMIN), (uint16_t)(0xFFFEu - NANMIN)});
  const u16x2 t = __builtin_elementwise_sub_sat(m, (u16x2){0xFFFE, 0xFFFE});
  return w | __builtin_bit_cast(uint32_t, t * (u16x2){SET, SET});
}
template <int DT>
__device__ __forceinline__ uint4 canon_nan_dt(uint4 a) {
  if constexpr (DT == KVC_BF16)  // NaN -> 0xFFFF
    return make_uint4(canon_nan_pk<0x7F80, 0xFFFF>(a.x), canon_nan_pk<0x7F80, 0xFFFF>(a.y),
                      canon_nan_pk<0x7F80, 0xFFFF>(a.z), canon_nan_pk<0x7F80, 0xFFFF>(a.w));
  else if constexpr (DT == KVC_F16)  // NaN |= 0x200 (quiet bit)
    return make_uint4(canon_nan_pk<0x7C00, 0x200>(a.x), canon_nan_pk<0x7C00, 0x200>(a.y),
                      canon_nan_pk<0x7C00, 0x200>(a.z), canon_nan_pk<0x7C00, 0x200>(a.w));
  else
    return a;
}

// Diagnostic build only (-DKVC_STAMPS): thread 0 of every select workgroup records s_memtime at
// phase boundaries into a per-row slot after the index region; the product build has no stamps.
#ifdef KVC_STAMPS
#define KVC_STAMP(i)                                                             \
  do {                                                                           \
    if (stamps && threadIdx.x == 0) stamps[blockIdx.x * 32 + (i)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define KVC_STAMP(i) \
  do {               \
  } while (0)
#endif

// Materialises x in a VGPR here: keeps the compiler from sinking the computation of a select
// operand into an exec-mask branch (s_and_saveexec / s_or_b64 exec: scalar instructions on the
// CU's one scalar unit, shared by all its waves) when only some lanes use it.
__device__ __forceinline__ int vreg(int x) {
  asm("" : "+v"(x));
  return x;
}

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}


#ifdef KVC_STAMPS
#define KVC_TICK(v) (v) = __builtin_amdgcn_s_memtime()
#else
#define KVC_TICK(v) (void)0
#endif

// Uniform (wave-invariant) value into an SGPR, so that the arithmetic on it runs on the scalar
// unit instead of costing a 4-cycle wave64 VALU slot in every wave.
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
// inclusive prefix sum within each 16-lane row (4 DPP adds); lanes 0..15 = the 16 waves
__device__ __forceinline__ int row_scan16(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);  // row_shr:8
  return v;
}
// lanes below this one with their bit set in `mask`, plus `base` (v_mbcnt_lo/hi: 2 VALU)
__device__ __forceinline__ int mbcnt(uint64_t mask, int base) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                        __builtin_amdgcn_mbcnt_lo((uint32_t)mask, (uint32_t)base));
}

// f(integral_constant<int, I>) for I in [B, E): a loop the compiler cannot leave rolled.
template <int B, int E, typename F>
__device__ __forceinline__ void unroll_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>());
    unroll_for<B + 1, E>(f);
  }
}


// ---- the selection's working set (LDS, or a global scratch row) ----
template <typename KeyT>
struct SelScalars {
  int wa[kSelWaves];  // per wave: ge count | le count << 16 (P1); snapkv scratch
  int wb[kSelWaves];  //           snapkv scratch
  int wm[kSelWaves];  //           swaps | first unswapped ge position << 16 (P2)
  float fmax[kSelWaves];
  int fnan[kSelWaves];
};

// Selection arrays for zones of up to n_cap positions:
//   key[n_cap] | idx[n_cap] (u16) | 64 sinks | spos[cap + 8] | 64 sinks | gpos[cap + 8]
// spos / gpos are the s / g rank -> position tables (1-based) of one window of `cap` swap ranks
// (m <= (n-1)/2 swapped pairs per level; a level with m > cap runs its swaps in windows); the 64
// entries before each are per-lane sinks for lanes with nothing to record (branch-free scatter).
// In LDS (dynamic, sized by the call's longest zone), or in a per-row global scratch for zones
// longer than kZoneMax.
__host__ __device__ constexpr size_t sel_bytes(int n_cap, int key_size, int cap) {
  return (size_t)n_cap * key_size + (size_t)n_cap * 2 + (size_t)(64 + cap + 8) * 2 * 2;
}
// Rank-window size for an n_cap-position LDS selection within `budget` bytes of arrays.  16-bit
// keys fit the budget when the tables hold fewer than the n_cap/2 ranks a level can need; levels
// with more swaps take further windows.  fp32 keys (whose snapkv scores use the tables as
// scratch) and short zones get full tables.
__host__ __device__ constexpr int sel_cap(int n_cap, int key_size, long budget) {
  const int full = n_cap / 2 + 1;
  const long tables = budget - (long)n_cap * (key_size + 2) - 4L * 72;  // bytes for the tables
  const int fit = tables > 0 ? (int)(tables / 4) : 0;
  return (key_size == 2 && fit < full && fit >= 1024) ? (fit & ~63) : full;
}
template <typename KeyT>
struct SelArrays {
  KeyT* key;
  uint16_t* idx;
  uint16_t* spos;
  uint16_t* gpos;
  __device__ SelArrays(char* base, int n_cap, int cap)
      : key(reinterpret_cast<KeyT*>(base)),
        idx(reinterpret_cast<uint16_t*>(base + (size_t)n_cap * sizeof(KeyT))),
        spos(idx + n_cap + 64),
        gpos(spos + cap + 8 + 64) {}
};

__device__ __forceinline__ uint64_t lanemask_lt(int lane) { return (1ull << lane) - 1ull; }
__device__ __forceinline__ uint64_t lanemask_le(int lane) {
  return lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
}

}  // namespace kvc
