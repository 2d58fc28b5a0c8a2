/*
 * kvc.h -- C ABI of the MI355X-native KV-cache compression engine.
 *
 * This library is the native half of the drop-in replacement for the reference's
 * kvcompress/methods hot path (od-liu/CS3602-LLM-Inference-Acceleration).  One call compresses a
 * batch of layers; each layer's output is built from three segments of its input sequence:
 *
 *     out = K[:, :, sink]  ++  K[:, :, zone][selected]  ++  K[:, :, tail]      (same for V)
 *
 * which covers every compressing branch of the eight in-scope methods.  Each entry below names the
 * reference lines (in /root/reference/kvcompress/methods/) whose norm -> argsort/topk -> sort ->
 * gather -> cat sequence one call replaces:
 *   fix_size_l2   fix_size_l2.py:99-150   zone [0,S-P), select keep, tail = last P
 *   l2_compress   l2_compress.py:62-90    zone [0,S),   select ceil(kr*S)
 *   h2o_l2        h2o_l2.py:99-151        sink start, zone middle, tail recent
 *   snapkv_lite   snapkv_lite.py:83-152   zone prefix (snapkv scoring, topk), tail obs window
 *   pyramid_kv    pyramid_kv.py:115-183   sink, zone middle, tail recent (per-layer size)
 *   adaptive_l2   adaptive_l2.py:81-145 (hard limit), :147-199 (gradual)
 *   streaming_llm streaming_llm.py:99-109 sink + tail, no selection (pure copy);
 *                 evict_for_space streaming_llm.py:154-168 likewise
 * recent_only (recent_only.py:65-66) returns views and never reaches the engine.
 *
 * The reference does this with torch CPU/GPU ops (torch.norm -> argsort/topk -> sort -> gather
 * -> cat); the engine reproduces their results bit-exactly, including libstdc++'s introsort /
 * introselect tie order, torch.norm's 8-lane FMA order, and torch.gather's bf16 NaN rewrite.
 *
 * Phases (stream-ordered on `stream`, one kernel each per chunk of <= 64 layers; SELECT and
 * GATHER run as one select_gather kernel unless params.flags has KVC_FLAG_SPLIT_SELECT_GATHER):
 *   SCORE  : key L2 norms of every zone token           -> workspace norm region
 *            (and per-64-token-tile statistics of those norms -> a workspace region behind the
 *            index region that kvc_plan() sizes and kvc_plan_info_t does not name)
 *   SELECT : per (layer,b,h) row: snapkv scoring (opt.), reference-exact k-selection,
 *            ascending zone-local indices                -> workspace index region (int32)
 *   GATHER : segment copy of K and V into k_out / v_out (caller-allocated, contiguous)
 * The phases of one call may be launched separately, in this order on one stream and one
 * workspace (SCORE, then SELECT | GATHER; or SCORE, SELECT, GATHER): the outputs are the bytes of
 * a KVC_PHASE_ALL launch.  A separate SELECT writes the index region (n_select ascending indices
 * per row) even without KVC_FLAG_SPLIT_SELECT_GATHER.  No phase reads workspace bytes that an
 * earlier phase of the call did not write, so the workspace needs no initialisation.
 *   - SELECT of KVC_SCORE_SNAPKV rows reads SCORE's tile statistics: SCORE must have run on the
 *     same workspace with the same table.
 *   - SELECT of plain-norm rows (KVC_SCORE_NORM) reads the norm region only, and only columns
 *     [0, zone_len) of a row decide its result: the caller may fill those itself (row
 *     layer.row0 + b*heads + h, norm_row_stride elements of the SCORE dtype apart, norms in that
 *     dtype: dtype itself, or bf16 for the fp8 dtypes) and launch SELECT without SCORE.
 *     Columns from zone_len up to norm_row_stride may hold anything.
 *
 * Ownership: the caller allocates outputs and the workspace; the library never allocates,
 * frees or synchronises.  Entry points are reentrant (no global mutable state, no environment
 * variables read) and may be used concurrently on different devices/streams.  All functions
 * return a kvc_status (0 = ok); a HIP launch failure is reported from that launch's own return
 * value, and a caller's pending HIP error is left untouched.
 */
#ifndef KVC_H
#define KVC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history:
 *   3  kvc_params_t.flags / reserved / device_status; the h2o_attention entries.
 *   4  KVC_ALGO_STABLE and KVC_ATTN_HH_STABLE (opt-in stable tie policy); KVC_FLAG_GATHER_FIXED /
 *      KVC_FLAG_GATHER_SELECTED are refused (KVC_E_ARG) without external_index, where a v3
 *      library accepted them; device status bit KVC_DEV_INTERNAL. */
#define KVC_ABI_VERSION 4

typedef struct ihipStream_t* kvc_stream_t; /* a hipStream_t; NULL = legacy default stream */

/* KVC_F16: IEEE half (what transformers >= 5 loads pythia checkpoints as: dtype="auto").  Its
 * norm follows torch's non-vectorised CPU reduction (one fp32 accumulator in dim order), not the
 * 8-lane order of bf16/fp32 -- see DESIGN.md. */
enum kvc_dtype {
  KVC_F32 = 0,
  KVC_BF16 = 1,
  KVC_F16 = 2,
  /* fp8 K/V caches, the OCP formats (torch.float8_e4m3fn / float8_e5m2; gfx950's native fp8), with
   * dequantisation scale 1 (per-token or uniform scales of paged caches compacted in place:
   * kvc_scales_t, "Per-token-scaled fp8 paged caches" below).  Elements are 1 byte: strides,
   * alignment, spans and GATHER units follow the D-byte rows.  Every fp8 pattern upcasts to bf16
   * exactly, and the SCORE dtype of an fp8 call is bf16: the kept positions, the norm region
   * (norm_row_stride counts 2-byte elements), the tile statistics, the index region and the
   * workspace layout are those of a bf16 call on K.to(bf16) -- torch.norm's 8-lane FMA order over
   * the D upcast elements, norms rounded to bf16, u16 keys, NaN patterns as the one NaN key, e5m2
   * +-inf giving an inf norm.  GATHER copies the kept rows' BYTES of K and V verbatim: no NaN
   * rewrite, V is never interpreted.  head_dim is 64, 128 or 256 (else KVC_E_HEADDIM).  The fnuz
   * formats and raw byte tensors have no code; scales of dense K/V calls and of paged calls with
   * dense outputs are out of scope (kvc_layer_t has no room for them in ABI 4, and a dense output
   * no channel for the moved scales).  The kvc_attn_* / kvc_heavy_hitters entries refuse them
   * (KVC_E_DTYPE): attention tensors are not fp8.  Additive within ABI 4: an older library answers
   * KVC_E_DTYPE. */
  KVC_F8E4M3 = 16,
  KVC_F8E5M2 = 17
};
/* KVC_ASC keeps the smallest keys (argsort ascending, "keep_low");
 * KVC_DESC keeps the largest (argsort descending / topk largest, "keep_high", snapkv). */
enum kvc_order { KVC_ASC = 0, KVC_DESC = 1 };
/* KVC_ALGO_SORT: set of argsort(stable=False)[:k] = libstdc++ std::sort (introsort)
 * KVC_ALGO_TOPK: set of torch.topk = std::nth_element (introselect), or std::partial_sort
 *                (heap select) when k*64 <= n, exactly as aten TopKImpl.h chooses.
 * KVC_ALGO_STABLE (opt-in, not the reference's tie order): set of argsort(stable=True)[:k] --
 *                every key strictly before the k-th one and the first of the tied keys in
 *                position order; the same set for sort and topk callers.  A radix select with
 *                no partition chain.  Zones of at most 65 536 positions (else KVC_E_TOO_LONG). */
enum kvc_algo { KVC_ALGO_SORT = 0, KVC_ALGO_TOPK = 1, KVC_ALGO_STABLE = 2 };
enum kvc_score { KVC_SCORE_NORM = 0, KVC_SCORE_SNAPKV = 1 };
enum kvc_phase {
  KVC_PHASE_SCORE = 1,
  KVC_PHASE_SELECT = 2,
  KVC_PHASE_GATHER = 4,
  KVC_PHASE_ALL = 7
};
enum kvc_flag {
  KVC_FLAG_SPLIT_SELECT_GATHER = 1, /* SELECT writes the index region, then a GATHER kernel    */
  KVC_FLAG_SHARED_INDEX = 2,        /* external_index: index row (layer*batch + b) serves every
                                       head of (layer, b) -- h2o_attention's heavy hitters, one
                                       index list per layer (h2o_attention.py:326-333)        */
  KVC_FLAG_GATHER_FIXED = 4,        /* GATHER copies only the sink and tail rows of each output
                                       (the rows no selection decides), layout unchanged      */
  KVC_FLAG_GATHER_SELECTED = 8      /* GATHER copies only the selected rows.  With the previous
                                       flag: one call's copy in two launches, e.g. the fixed rows
                                       on a second stream while the selection runs.  At most one
                                       of the two, and only with external_index (the parts
                                       read the caller's indices; KVC_E_ARG otherwise)         */
};
/* Bits the kernels OR into *params.device_status (when not NULL).  The word is sticky: the
 * library never clears it; the caller zeroes it and reads it after the stream has drained. */
enum kvc_device_status {
  KVC_DEV_SELECT_BOUNDS = 1, /* a selection row exceeded its kernel's zone capacity: nothing
                                is selected and the row's index entries are not written.  In
                                the fused select_gather kernel none of that row's output rows
                                is written either; a separate GATHER kernel (SPLIT flag, long
                                zones, separately launched phases) still copies the row's sink
                                and tail and gathers through whatever the index row held
                                (never expected: kvc_launch picks kernels by the planned zone
                                lengths)                                                       */
  KVC_DEV_INDEX_RANGE = 2,   /* an external index lay outside its zone and was clamped        */
  KVC_DEV_INTERNAL = 4       /* an internal invariant of a selection failed (e.g. the register
                                tail of the partition chain saw more swaps than a 64-lane
                                segment allows): that row's output is unspecified (never
                                expected; checked so a violation cannot pass silently)        */
};
enum kvc_status {
  KVC_OK = 0,
  KVC_E_ARG = -1,       /* malformed layer table / params                             */
  KVC_E_DTYPE = -2,     /* dtype is not bf16 / fp16 / fp32 / fp8 e4m3fn / fp8 e5m2 (the
                           attention entries: not bf16 / fp16 / fp32)                  */
  KVC_E_HEADDIM = -3,   /* head_dim*elem_size not in {64,128,160,256,320,512,1024} B;
                           fp8 dtypes: head_dim not in {64,128,256}                    */
  KVC_E_ALIGN = -4,     /* a base pointer or stride is not 16-byte aligned            */
  KVC_E_TOO_LONG = -5,  /* a scored zone is longer than kvc_max_zone_len() (2^24), or a
                           KVC_ALGO_STABLE selection zone longer than 65 536            */
  KVC_E_WORKSPACE = -6, /* workspace smaller than kvc_plan() reported                 */
  KVC_E_HIP = -7        /* a HIP launch failed                                        */
};

/* One layer.  Inputs K,V: [batch, heads, seq_len, head_dim], last dim contiguous, arbitrary
 * element strides for the other three dims, K's and V's independent of each other (16-byte
 * multiples for every dim larger than 1, else KVC_E_ALIGN; a stride of 0 -- an expanded batch --
 * and offsets beyond 2^32 bytes are fine).  Every kernel path is tested on such views: windows of
 * a static cache, the K / V thirds of a fused QKV projection, permuted, sliced and expanded
 * tensors (the test_strided_inputs suite).  Outputs: contiguous [batch, heads, n_out, head_dim]
 * with n_out = sink_len + n_select + tail_len. */
typedef struct kvc_layer {
  const void* k;
  const void* v;
  void* k_out;
  void* v_out;
  int64_t k_stride[3]; /* element strides of dims batch, heads, seq (fp8: 1-byte elements) */
  int64_t v_stride[3];
  int32_t seq_len;     /* S */
  int32_t zone_start;  /* scored zone [zone_start, zone_start + zone_len) */
  int32_t zone_len;
  int32_t n_select;    /* tokens kept from the zone: 0 <= n_select <= zone_len */
  int32_t sink_len;    /* segment A: source rows [0, sink_len)                   */
  int32_t tail_start;  /* segment C: source rows [tail_start, tail_start+tail_len) */
  int32_t tail_len;
  int32_t pool_kernel; /* KVC_SCORE_SNAPKV: avg_pool1d kernel; <= 1 means no pooling */
  int32_t score_mode;  /* enum kvc_score */
  /* ---- filled in by kvc_plan() ---- */
  int32_t n_out;
  int32_t row0;  /* first workspace row of this layer (rows = layer*batch*heads + b*heads + h) */
  int32_t tile0; /* first 64-token SCORE tile of this layer */
  int64_t unit0; /* first GATHER unit (one 16-byte chunk of one output row of K or V) */
} kvc_layer_t;

typedef struct kvc_params {
  int32_t dtype;
  int32_t batch;
  int32_t heads;
  int32_t head_dim;
  int32_t order;          /* enum kvc_order */
  int32_t algo;           /* enum kvc_algo  */
  int32_t phases;         /* OR of enum kvc_phase */
  int32_t external_index; /* 1: GATHER reads indices the caller wrote into the index region */
  int32_t flags;          /* OR of enum kvc_flag (other bits: KVC_E_ARG) */
  int32_t reserved;       /* must be 0 (else KVC_E_ARG) */
  uint32_t* device_status;/* optional device word for enum kvc_device_status bits (or NULL) */
} kvc_params_t;

typedef struct kvc_plan_info {
  size_t norm_offset;      /* workspace byte offset of the norm region                    */
  size_t index_offset;     /* workspace byte offset of the int32 index region             */
  size_t workspace_bytes;  /* total workspace the launch needs                              */
  int64_t norm_row_stride; /* elements (of the score dtype: dtype, bf16 for fp8) per norm row */
  int64_t index_row_stride;/* int32 entries per row in the index region                   */
  int64_t rows;            /* num_layers * batch * heads                                   */
  int64_t score_tiles;     /* SCORE work items                                             */
  int64_t gather_units;    /* GATHER work items                                            */
} kvc_plan_info_t;

/* ABI/library identification. */
int kvc_version(void);
size_t kvc_layer_struct_size(void);
int kvc_max_zone_len(void);
const char* kvc_status_string(int status);
/* SHA-256 (hex) of the sources this library was compiled from (csrc/kvc.hip, then the headers it
 * includes -- kvc_common.h, kvc_serial.h, kvc_device_util.h, kvc_score.h, kvc_snapkv_keys.h,
 * kvc_select_chain.h, kvc_select.h, kvc_gather.h, kvc_attn.h, kvc_gather_dest.h,
 * kvc_paged.h, kvc_ragged.h -- then include/kvc.h, in that order), or "unknown" for builds that
 * do not set it --
 * lets a caller (and tests/test_abi.py) check that a shipped binary matches its source tree. */
const char* kvc_source_digest(void);

/* Validates the table, fills the kvc_plan() fields of every layer (host memory) and the
 * workspace layout.  Pure host function. */
int kvc_plan(const kvc_params_t* params, kvc_layer_t* layers, int num_layers,
             kvc_plan_info_t* info);

/* Launches the requested phases.  `layers` is the host table filled by kvc_plan(); the kernels
 * receive it by value in their kernel arguments (no copy is enqueued). */
int kvc_launch(const kvc_params_t* params, const kvc_layer_t* layers, int num_layers,
               void* workspace, size_t workspace_bytes, kvc_stream_t stream);

/* Convenience: kvc_plan + kvc_launch.  `layers` is updated in place. */
int kvc_compress(const kvc_params_t* params, kvc_layer_t* layers, int num_layers,
                 void* workspace, size_t workspace_bytes, kvc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Caller-provided destinations (additive within ABI 4: kvc_layer_t and kvc_params_t are
 * unchanged; a library without these two entries does not export them).
 *
 * kvc_dest_t says where one layer's result goes.  Strided destination (in_place == 0): the
 * layer's k_out / v_out are the bases of views [batch, heads, S_d, head_dim] with S_d >= n_out,
 * last dim contiguous, the other three dims with the element strides given here (K's and V's
 * independent; the inputs' rules: 16-byte aligned pointers, strides of dims larger than 1
 * multiples of 16 bytes -- the seq dim counts as larger than 1 when n_out > 1 -- else
 * KVC_E_ALIGN).  The library writes rows [0, n_out) of every (b, h) row and no other byte.  The
 * byte span of the K destination and of the V destination must not intersect the byte span of
 * the same layer's K source or V source (KVC_E_ARG).  A span is [base, base + sum over the three
 * dims of (size - 1) * stride * element size + one row's bytes), sized with n_out for a
 * destination and seq_len for a source: the check is conservative (it refuses, e.g., a
 * destination interleaved with its own source inside one fused buffer).  Overlap between
 * DIFFERENT layers of a call -- a destination of one with a source or a destination of another
 * -- is not checked: that they are disjoint is the caller's promise.
 *
 * In place (in_place == 1): the destination is the layer's own input -- k_out == k, v_out == v
 * and the strides here equal the layer's k_stride / v_stride (KVC_E_ARG otherwise).  After the
 * call rows [0, n_out) of every (b, h) row of K and V hold the compressed sequence; rows
 * [n_out, S) and all bytes outside the written rows stay untouched.  Allowed only when the row
 * map is strictly increasing with source row >= output row: sink_len <= zone_start when
 * n_select > 0, and, when tail_len > 0, zone_start + zone_len <= tail_start and
 * sink_len <= tail_start (KVC_E_ARG otherwise); caller-provided indices must be ascending (as
 * the index region's contract says anyway).  Every stride of a dim larger than 1 must be
 * non-zero (an expanded batch would be written twice; KVC_E_ARG).  K and V of a layer, and the
 * layers of a call, must not share memory (the caller's promise).  Sink rows are already in
 * place and are not touched.
 *
 * Values are byte-identical to kvc_launch's.  A launch with destinations runs SCORE and SELECT
 * with the kernels of KVC_FLAG_SPLIT_SELECT_GATHER (SELECT writes the index region) and GATHER
 * with a copy kernel of its own, which orders an in-place row's loads before its stores; phases
 * may be launched separately as with kvc_launch.  KVC_FLAG_GATHER_FIXED / _SELECTED are refused
 * with destinations (KVC_E_ARG).  Layers with n_out == 0 are exempt from the destination checks.
 * ------------------------------------------------------------------------------------------- */
typedef struct kvc_dest {
  int64_t k_stride[3];  /* element strides of k_out's batch, heads, seq dims */
  int64_t v_stride[3];
  int32_t in_place;     /* 0 or 1 (else KVC_E_ARG) */
  int32_t reserved;     /* 0 (else KVC_E_ARG) */
} kvc_dest_t;           /* 56 bytes */

/* kvc_plan with destinations: dests[i] belongs to layers[i].  dests == NULL behaves exactly like
 * kvc_plan.  With dests it validates them as described above, and fills the same layer fields
 * and the same kvc_plan_info_t as kvc_plan (the workspace layout does not depend on
 * destinations).  Pure host function. */
int kvc_plan_dest(const kvc_params_t* params, kvc_layer_t* layers, const kvc_dest_t* dests,
                  int num_layers, kvc_plan_info_t* info);

/* kvc_launch with destinations (dests == NULL: exactly kvc_launch).  Re-validates table and
 * destinations as kvc_plan_dest does; the kernels receive both by value. */
int kvc_launch_dest(const kvc_params_t* params, const kvc_layer_t* layers,
                    const kvc_dest_t* dests, int num_layers, void* workspace,
                    size_t workspace_bytes, kvc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Paged caches (additive within ABI 4: kvc_layer_t, kvc_params_t and kvc_dest_t are unchanged; a
 * library without these two entries does not export them).
 *
 * kvc_pages_t says that one layer's K and V live in a page pool addressed through a block table,
 * as the paged-attention caches of serving stacks do.  The layer's k / v are the pool bases
 * (page 0), and logical row s of (b, h) is read at
 *     base + (block_table[b * table_stride + (s >> log2 P)] * page_stride + h * stride[1]
 *             + (s & (P - 1)) * stride[2]) * element size          (P = page_size)
 * so the layer's stride[1] / stride[2] step over the heads and the slots INSIDE a page and the
 * table replaces the batch stride: stride[0] must be 0 (KVC_E_ARG).  K's and V's strides and page
 * strides are independent: one description covers a pool stored [N, P, H, D] and one stored
 * [N, H, P, D].  The inputs' alignment rules hold (16-byte aligned pointers, strides of dims
 * larger than 1 multiples of 16 bytes, else KVC_E_ALIGN; the page stride counts as a dim larger
 * than 1 when num_pages > 1).  block_table NULL or not 4-byte aligned, table_stride smaller than
 * ceil(seq_len / page_size), a page_size that is not a power of two in [1, 65536], num_pages < 1,
 * in_place other than 0 / 1 or reserved != 0 give KVC_E_ARG.  All address arithmetic is 64-bit:
 * offsets beyond 2^32 bytes are fine.  With `pages`, every layer of the call is paged; pages[i]
 * belongs to layers[i].
 *
 * Output of a paged layer, one of three:
 *   (a) in_place == 0, dests == NULL: contiguous k_out / v_out, as with kvc_launch.
 *   (b) in_place == 0, dests[i]: a strided dense destination under kvc_dest_t's rules
 *       (dests[i].in_place must be 0).  Its byte span must not meet the K or V pool's span --
 *       [base, base + ((num_pages - 1) * page_stride + (heads - 1) * stride[1] + (P - 1) *
 *       stride[2]) * element size + one row's bytes) for non-negative strides; conservative as
 *       above (KVC_E_ARG).
 *   (c) in_place == 1: k_out == k and v_out == v (KVC_E_ARG otherwise); dests[i] is not read.
 *       Output row t is written to the slot of LOGICAL row t through the same table, so the
 *       compressed sequence ends up in the sequence's leading pages and the caller can free the
 *       pages from ceil(n_out / P) on.  The segment-order rules of kvc_dest_t's in-place contract
 *       apply unchanged; strides of dims larger than 1 must be non-zero.  Sink rows are not
 *       touched; rows [n_out, seq_len) and every pool byte that is not a written row keep their
 *       contents.  The caller promises that the page ids of one table row are distinct, that
 *       different batch rows, K and V, and different layers share no page that is written, and
 *       that the table is not modified while the call runs.  Pages that hold only sink rows are
 *       never written and so may be shared between sequences (a shared prefix).
 *
 * Values are byte-identical to kvc_launch on the dense tensor the table describes.  SCORE and
 * GATHER run kernels of their own that differ from the dense ones in address arithmetic only;
 * SELECT is the kernels of KVC_FLAG_SPLIT_SELECT_GATHER (it reads the workspace only).  Phases may
 * be launched separately under the contract above; external_index and KVC_FLAG_SHARED_INDEX work;
 * KVC_FLAG_GATHER_FIXED / _SELECTED are refused (KVC_E_ARG).  Plan info and workspace layout are
 * kvc_plan's for the same table.  Layers with n_out == 0 are exempt from the page checks.
 *
 * Device safety: a page id outside [0, num_pages) is clamped for loads and KVC_DEV_INDEX_RANGE is
 * ORed into the status word; an in-place store through such an id is dropped, not clamped.
 * The table is device data read when the kernels run: a replay of a captured launch follows the
 * table's contents at replay time.
 * ------------------------------------------------------------------------------------------- */
typedef struct kvc_pages {
  const int32_t* block_table; /* device memory: page id of logical page p of batch row b at
                                 block_table[b * table_stride + p]                          */
  int64_t table_stride;       /* int32 entries per batch row, >= ceil(seq_len / page_size)   */
  int64_t k_page_stride;      /* elements between consecutive pages of the K pool            */
  int64_t v_page_stride;
  int32_t page_size;          /* tokens per page: a power of two, 1 .. 65536                 */
  int32_t num_pages;          /* pages in the pool, >= 1                                     */
  int32_t in_place;           /* 0 or 1                                                      */
  int32_t reserved;           /* 0                                                           */
} kvc_pages_t;                /* 48 bytes */

/* kvc_plan_dest for paged layers.  pages == NULL behaves exactly like kvc_plan_dest.  Fills the
 * same layer fields and the same kvc_plan_info_t as kvc_plan.  Pure host function. */
int kvc_plan_paged(const kvc_params_t* params, kvc_layer_t* layers, const kvc_pages_t* pages,
                   const kvc_dest_t* dests, int num_layers, kvc_plan_info_t* info);

/* kvc_launch_dest for paged layers (pages == NULL: exactly kvc_launch_dest).  Re-validates as
 * kvc_plan_paged does; the kernels receive the three tables by value. */
int kvc_launch_paged(const kvc_params_t* params, const kvc_layer_t* layers,
                     const kvc_pages_t* pages, const kvc_dest_t* dests, int num_layers,
                     void* workspace, size_t workspace_bytes, kvc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Ragged paged batches (additive within ABI 4: no existing struct, size or entry changes; a
 * library without these two entries does not export them).
 *
 * A continuous-batching server's block table has a length per row.  With a kvc_ragged_t per layer,
 * every (layer, b) of a paged call has its own segments: the result is that of kvc_launch_paged on
 * each sequence alone (batch = 1, the table row of b, the segments of record b), in ONE launch set
 * whose kernel count does not depend on the batch.
 *
 * kvc_seq_t is the part of kvc_layer_t that the methods' size arithmetic decides, per sequence.
 * Every layer gives `batch` records twice: `host` (read by plan and launch, validated there) and
 * `dev` (device memory holding the same records, read by the kernels when they RUN).  The library
 * never allocates, copies or synchronises: the caller uploads the records.  A captured launch
 * follows the device records at replay time, as it follows the block table; rewritten records
 * must stay inside what was planned (below), which the library cannot check at replay.
 *
 * Rules (KVC_E_ARG otherwise): every layer is paged and in place (kvc_pages_t.in_place == 1,
 * k_out == k, v_out == v); external_index, KVC_FLAG_SHARED_INDEX and KVC_FLAG_GATHER_FIXED /
 * _SELECTED are refused; host and dev are non-NULL, host 4-byte and dev 16-byte aligned (the
 * kernels read a record as three 16-byte words); every record obeys the
 * rules of a layer -- segment bounds inside its own seq_len, 0 <= n_select <= zone_len, a known
 * score_mode, n_out == sink_len + n_select + tail_len, reserved 0, the in-place row-map rule of
 * kvc_dest_t's contract -- and table_stride >= ceil(max seq_len / page_size).  Zone-length limits
 * (KVC_E_TOO_LONG) apply to the envelope below.
 *
 * For a ragged layer the segment fields of kvc_layer_t are OUTPUTS of kvc_plan_ragged: it
 * overwrites them with the ENVELOPE of the layer's records,
 *     seq_len   = max seq_len          zone_start = 0        sink_len = 0    tail_start = 0
 *     zone_len  = max zone_len  (*)    n_select   = max n_select
 *     tail_len  = max n_out - max n_select   (so n_out = max n_out)
 *     score_mode = KVC_SCORE_SNAPKV if a selecting record has it, else KVC_SCORE_NORM
 *     pool_kernel = max pool_kernel
 *     (*) max n_select + 1 when some record selects (0 < n_select < zone_len) although
 *         max n_select == max zone_len: the envelope of a layer with a selecting record selects.
 * and then fills n_out, row0, tile0, unit0 and kvc_plan_info_t exactly as kvc_plan does for that
 * envelope layer: workspace layout, grids and the kernel choice are those of the longest
 * sequence.  kvc_launch_ragged expects the table as kvc_plan_ragged left it.  k, v, k_out, v_out
 * and the strides stay the caller's inputs.
 *
 * A NO-OP record is sink_len = n_out = seq_len, every other field 0: nothing is scored, selected
 * or copied (sink rows are never touched in place).  It stands for a sequence that passes through
 * or that this launch leaves to another one.
 *
 * Device safety: the kernels take a row's bounds from its device record.  A record whose zone is
 * longer than the launch's selection capacity sets KVC_DEV_SELECT_BOUNDS as on every path.
 * ------------------------------------------------------------------------------------------- */
typedef struct kvc_seq {
  int32_t seq_len;
  int32_t zone_start;
  int32_t zone_len;
  int32_t n_select;
  int32_t sink_len;
  int32_t tail_start;
  int32_t tail_len;
  int32_t score_mode;  /* enum kvc_score */
  int32_t pool_kernel;
  int32_t n_out;       /* sink_len + n_select + tail_len */
  int32_t reserved[2]; /* 0 */
} kvc_seq_t;           /* 48 bytes */

typedef struct kvc_ragged {
  const kvc_seq_t* host; /* `batch` records in host memory                        */
  const kvc_seq_t* dev;  /* the same `batch` records in device memory             */
} kvc_ragged_t;          /* 16 bytes */

/* kvc_plan_paged for ragged layers: ragged[i] belongs to layers[i] / pages[i].  ragged == NULL
 * behaves exactly like kvc_plan_paged(params, layers, pages, NULL, ...).  Pure host function. */
int kvc_plan_ragged(const kvc_params_t* params, kvc_layer_t* layers, const kvc_pages_t* pages,
                    const kvc_ragged_t* ragged, int num_layers, kvc_plan_info_t* info);

/* kvc_launch_paged for ragged layers (ragged == NULL: exactly kvc_launch_paged without dests).
 * Re-validates table, pages and host records as kvc_plan_ragged does.  The kernels receive the
 * layer and page tables and the device record pointers by value (chunks of 32 layers); SCORE,
 * SELECT and GATHER are kernels of their own that read each row's bounds from its record. */
int kvc_launch_ragged(const kvc_params_t* params, const kvc_layer_t* layers,
                      const kvc_pages_t* pages, const kvc_ragged_t* ragged, int num_layers,
                      void* workspace, size_t workspace_bytes, kvc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Per-token-scaled fp8 paged caches (additive within ABI 4: no existing struct, size or entry
 * changes; a library without these two entries does not export them).
 *
 * A per-token quantised fp8 cache keeps one fp32 dequantisation scale per (page, head, slot) in a
 * scale pool beside the K pool and one beside the V pool, addressed through the SAME block table:
 * the scale of logical row s of (b, h) is the float at
 *     scale + (block_table[b * table_stride + (s >> log2 P)] * page_stride + h * stride[0]
 *              + (s & (P - 1)) * stride[1]) * 4
 * (element strides of 4-byte floats; a pool stored [N, H, P] or [N, P, H] alike).  With a
 * kvc_scales_t per layer:
 *
 *   SCORE stores, for a key row with scale s,
 *       bf16( torch.norm(K8.to(float32), dim=-1) * |s| )
 *     -- the fp32 norm the unscaled fp8 call rounds (torch.norm's 8-lane FMA order over the D
 *     upcast elements, correctly rounded sqrt), ONE fp32 multiply by |s| (round to nearest even,
 *     denormal products kept), and one bf16 rounding in place of the unscaled call's.  NaN or inf
 *     in s or in the row give what those operations give (0 * inf is NaN); a negative scale
 *     counts by its magnitude.  The tile statistics, SELECT and everything behind them see these
 *     stored norms and are the bf16 call on them.  V scales are never read for scoring.
 *   GATHER moves, with output row t, the 4 BYTES of the K scale and of the V scale of its source
 *     row src(t) into the slots of logical row t, in the same pass of the same workgroup that
 *     moves the row (a row's scale is part of the row: the in-place ordering argument is
 *     unchanged).  No float is interpreted: a NaN scale keeps its payload.  Sink rows are not
 *     touched; rows [n_out, seq_len), spare pages and every other scale-pool byte keep their
 *     contents.  A row whose destination page id is out of range drops its scale stores with its
 *     row stores (KVC_DEV_INDEX_RANGE).
 *
 * A UNIFORM scale (KVC_SCALE_K_UNIFORM / _V_UNIFORM: vLLM's per-tensor k_scale) is ONE device
 * float that serves every token: the K one is read by SCORE, on the device, with the formula
 * above and never written; the V one is ignored.  It changes the result only through rounding
 * ties (every row of a sequence is scaled alike).  KVC_SCALE_K_NONE / _V_NONE: no scale on that
 * side (scale 1; the pointer is not read).
 *
 * Rules: every layer of the call is paged and in_place == 1 (KVC_E_ARG otherwise -- a dense
 * output has no channel for the moved scales); dtype is an fp8 format (KVC_E_DTYPE); flags has no
 * unknown bit, at most one of UNIFORM / NONE per side, reserved is 0 (KVC_E_ARG); a pointer that
 * is read is non-NULL (KVC_E_ARG) and 4-byte aligned (KVC_E_ALIGN); a per-token pool has a
 * non-zero stride on every dim larger than 1 -- pages when num_pages > 1, heads, slots
 * (KVC_E_ARG: a scale shared by the heads would be written by `heads` workgroups that keep
 * different rows).  The caller promises that the scale pools alias neither each other nor the
 * K / V pools, and that what the paged contract says of written pages holds for their scales.
 * Plan info and workspace layout are those of the unscaled call.  Phases may be launched
 * separately: SCORE alone writes the scaled norms, GATHER alone moves the scales.
 * external_index / KVC_FLAG_SHARED_INDEX work as for kvc_launch_paged when ragged == NULL.
 * ------------------------------------------------------------------------------------------- */
enum kvc_scale_flag {
  KVC_SCALE_K_UNIFORM = 1, /* k_scale points at one float                     */
  KVC_SCALE_V_UNIFORM = 2, /* v_scale points at one float (never read)        */
  KVC_SCALE_K_NONE = 4,    /* no K scale: keys scored as with scale 1          */
  KVC_SCALE_V_NONE = 8     /* no V scale: nothing moves beside the V rows      */
};

typedef struct kvc_scales {
  float* k_scale;         /* device: K scale pool base (page 0), or the one uniform float  */
  float* v_scale;
  int64_t k_page_stride;  /* floats between consecutive pages of the K scale pool          */
  int64_t v_page_stride;
  int64_t k_stride[2];    /* float strides of the heads and of the slots inside a page     */
  int64_t v_stride[2];
  int32_t flags;          /* OR of enum kvc_scale_flag                                     */
  int32_t reserved;       /* 0                                                             */
} kvc_scales_t;           /* 72 bytes */

/* kvc_plan_ragged for scaled layers: scales[i] belongs to layers[i] / pages[i].  scales == NULL
 * behaves exactly like kvc_plan_ragged; ragged == NULL plans the single-length paged call
 * (kvc_plan_paged without dests).  Pure host function. */
int kvc_plan_scaled(const kvc_params_t* params, kvc_layer_t* layers, const kvc_pages_t* pages,
                    const kvc_ragged_t* ragged, const kvc_scales_t* scales, int num_layers,
                    kvc_plan_info_t* info);

/* kvc_launch_ragged for scaled layers (scales == NULL: exactly kvc_launch_ragged).  Re-validates
 * as kvc_plan_scaled does; the kernels receive the scale descriptions by value. */
int kvc_launch_scaled(const kvc_params_t* params, const kvc_layer_t* layers,
                      const kvc_pages_t* pages, const kvc_ragged_t* ragged,
                      const kvc_scales_t* scales, int num_layers, void* workspace,
                      size_t workspace_bytes, kvc_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Paged destinations: pages to pages (additive within ABI 4: no existing struct, size or entry
 * changes; a library without these two entries does not export them).
 *
 * Compaction in place (mode (c) of "Paged caches") asks the caller to promise that no written page
 * is shared.  A server with prefix caching or forked sequences cannot: a shared prompt lies inside
 * every method's scored zone.  With a kvc_page_dest_t per layer the compressed sequence of a paged
 * layer is written through a SECOND block table into pages the caller chose -- fresh pages of the
 * same pool (k_out == k, v_out == v) or another pool -- and the source pool is only read.
 *
 * Row addressing.  The layer's k_out / v_out are the DESTINATION pool bases (page 0); they may
 * equal k / v.  Output row t in [0, n_out) of (b, h) is written at
 *     k_out + (block_table[b * table_stride + (t >> log2 Pd)] * k_page_stride + h * k_stride[0]
 *              + (t & (Pd - 1)) * k_stride[1]) * element size        (Pd = this page_size)
 * and V likewise, with the table, page size, pool size and strides of THIS struct: none of them
 * need equal the source's.  That includes the sink rows: nothing is "already in place".  Every
 * other byte of every pool keeps its contents, destination rows [n_out, ...) of a partly filled
 * page included.  Values are byte-identical to kvc_launch_paged into a dense destination for the
 * same source table (torch.gather's NaN rewrite on the gathered segment only, none on fp8 bytes).
 *
 * Rules.  Every layer of the call is paged and pages[i].in_place is 0 (KVC_E_ARG).  There is no
 * segment-order rule: out of place, any row map that is legal for a dense destination is legal
 * here (ragged records included).  The destination pointers and strides obey the source pool's
 * alignment rules (16-byte aligned k_out / v_out; head stride when heads > 1, slot stride when
 * Pd > 1 and n_out > 1, page stride when num_pages > 1 multiples of 16 bytes: KVC_E_ALIGN).
 * KVC_E_ARG: page_size not a power of two in [1, 65536]; num_pages < 1; table_stride smaller than
 * ceil(n_out / page_size) (ragged: of the envelope's n_out, the largest record's); a zero stride
 * on one of those dims larger than 1 (different rows would be one address); block_table NULL or
 * not 4-byte aligned.  Layers with n_out == 0 are exempt.
 *
 * The caller's promise (the tables are device data: the library cannot check it without reading
 * device memory, and it does not).  Within a call, a destination page that receives a row is
 * none of: a source page that any sequence of that layer reads; a destination page of another
 * (layer, b); a page of the other side (K / V).  The page ids of one destination table row are
 * distinct.  Neither table is modified while the call runs.
 *
 * Ragged (ragged != NULL): per-sequence bounds come from the device records, as with
 * kvc_launch_ragged; the records need not obey the in-place row-map rule.  On THIS path the old
 * no-op record no longer means "nothing moves": a record with sink_len = n_out = seq_len (a
 * sequence that passes through) is COPIED to its destination pages, because its destination table
 * must describe it afterwards.  A record with n_out == 0 writes nothing: it stands for a sequence
 * that belongs to another launch group.  A device record's n_out is capped at the planned
 * envelope's.
 *
 * Scales (scales != NULL; fp8): dscales[i] describes the DESTINATION scale pools, addressed by the
 * destination table and page size as the rows are.  For each side that is per-token in scales[i],
 * dscales[i] must be per-token too, with a non-NULL (KVC_E_ARG), 4-byte aligned (KVC_E_ALIGN)
 * pointer and non-zero strides on every dim larger than 1 (pages when the destination's
 * num_pages > 1, heads, slots when Pd > 1; KVC_E_ARG); the 4 bytes of source row src(t)'s scale
 * are stored at output row t's slot, uninterpreted (a NaN keeps its payload).  A side that is
 * uniform or absent in scales[i] moves nothing, and dscales[i] must carry the same flag on that
 * side (KVC_E_ARG); its pointer is not read.  dscales == NULL with scales != NULL is KVC_E_ARG.
 * SCORE reads the SOURCE scales as kvc_launch_scaled does.
 *
 * Device safety: a destination page id outside [0, num_pages) drops that row's stores, its scale
 * stores included, and sets KVC_DEV_INDEX_RANGE; a bad source id is clamped for loads, as on
 * every paged path.
 *
 * SCORE and SELECT are the kernels of kvc_launch_paged / _ragged / _scaled, unchanged; GATHER is a
 * copy kernel of its own on the out-of-place grid (rows, passes of the longest output), for
 * ragged layers too (a block past its sequence's n_out returns after the record load).  Phases
 * may be launched separately.  external_index and KVC_FLAG_SHARED_INDEX work when ragged == NULL;
 * KVC_FLAG_GATHER_FIXED / _SELECTED are refused (KVC_E_ARG).  Plan info and workspace layout are
 * those of the in-place call for the same tables.  Both tables (and the ragged records) are read
 * when the kernels run: a replay of a captured launch follows their contents at replay time.
 * Kernel arguments travel by value: chunks of 32 layers, of 16 when scales move (two scale
 * descriptions per layer would take 32 layers past 12 KiB of arguments).
 * ------------------------------------------------------------------------------------------- */
typedef struct kvc_page_dest {
  const int32_t* block_table; /* device: DESTINATION page id of logical page p of row b at
                                 block_table[b * table_stride + p]                            */
  int64_t table_stride;       /* >= ceil(n_out / page_size) (ragged: of the largest n_out)    */
  int64_t k_page_stride;      /* elements between consecutive pages of the destination K pool */
  int64_t v_page_stride;
  int64_t k_stride[2];        /* element strides of the heads and of the slots inside a page  */
  int64_t v_stride[2];
  int32_t page_size;          /* power of two in [1, 65536]; need not equal the source's      */
  int32_t num_pages;          /* pages in the destination pool, >= 1                          */
} kvc_page_dest_t;            /* 72 bytes */

/* kvc_plan_scaled with paged destinations: pdests[i] (and dscales[i]) belong to layers[i].
 * ragged, scales and dscales are nullable as in the entries above; pdests == NULL behaves exactly
 * like kvc_plan_scaled.  Fills the same layer fields and kvc_plan_info_t.  Pure host function. */
int kvc_plan_repage(const kvc_params_t* params, kvc_layer_t* layers, const kvc_pages_t* pages,
                    const kvc_ragged_t* ragged, const kvc_scales_t* scales,
                    const kvc_page_dest_t* pdests, const kvc_scales_t* dscales, int num_layers,
                    kvc_plan_info_t* info);

/* kvc_launch_scaled with paged destinations (pdests == NULL: exactly kvc_launch_scaled).
 * Re-validates as kvc_plan_repage does; the kernels receive every table by value. */
int kvc_launch_repage(const kvc_params_t* params, const kvc_layer_t* layers,
                      const kvc_pages_t* pages, const kvc_ragged_t* ragged,
                      const kvc_scales_t* scales, const kvc_page_dest_t* pdests,
                      const kvc_scales_t* dscales, int num_layers, void* workspace,
                      size_t workspace_bytes, kvc_stream_t stream);

/* Diagnostic entry (tests of the device status channel; no reference counterpart).  Runs the
 * 512-thread SELECT (params->phases == KVC_PHASE_SELECT) or SELECT_GATHER (KVC_PHASE_SELECT |
 * KVC_PHASE_GATHER) kernel of a planned table (at most 64 layers) as kvc_launch would, but with
 * the kernels' zone capacity set to `zone_cap` (a multiple of 64, <= 8192) instead of the
 * table's longest zone.  A row whose zone is longer than that capacity selects nothing, writes
 * no index and no K/V output row, and ORs KVC_DEV_SELECT_BOUNDS into params->device_status --
 * the path a dispatch bug would take.  kvc_launch itself always passes a sufficient capacity. */
int kvc_debug_select_capacity(const kvc_params_t* params, const kvc_layer_t* layers,
                              int num_layers, void* workspace, size_t workspace_bytes,
                              int zone_cap, kvc_stream_t stream);


/* ---------------------------------------------------------------------------------------------
 * h2o_attention heavy hitters (reference: kvcompress/methods/h2o_attention.py).  The reference's
 * H2OAttentionManager keeps per layer an accumulated attention tensor acc [B,H,len]:
 *   update_attention_scores (:84-153)  acc = (acc*decay, zero-extended | zeros) + attn.sum(dim=2)
 *   get_heavy_hitter_indices (:156-213) top-k of acc[:, :, m0:m1].sum(dim=1), sorted ascending
 * Both sums follow torch's CPU reduction order (aten cascade_sum: four-level cascade per column,
 * four interleaved lanes -- row_sum -- for the columns the SIMD loop leaves over, which depend on
 * the reference process's thread chunks: col_chunk below); the top-k is the reference-exact
 * std::nth_element / std::partial_sort set (KVC_ALGO_TOPK, descending).
 * ------------------------------------------------------------------------------------------- */
typedef struct kvc_attn_params {
  int32_t dtype;        /* enum kvc_dtype of attn / acc */
  int32_t batch;
  int32_t heads;
  int32_t vec_bytes;    /* SIMD width of the reference's CPU sum kernel: 32 on x86 (sum_stub has
                           no AVX512 variant) */
  float decay;          /* decay_factor as the fp32 value torch multiplies by (:136, :146) */
  int32_t flags;        /* kvc_heavy_hitters: 0 or KVC_ATTN_HH_STABLE.  kvc_attn_accumulate: 0, or
                           KVC_ATTN_OLD_DTYPE(d) when every layer's acc_old (old_len > 0 in every
                           layer) is of enum kvc_dtype d != dtype -- the reference then promotes
                           through `acc * decay`, torch.cat and `+` (:129-151): base is rounded to
                           d, and acc_new is FLOAT32 = fp32(base) + fp32(attn.sum), unrounded --
                           and/or KVC_ATTN_HH_STABLE, which it ignores (one struct per step),
                           and/or KVC_ATTN_SCALAR_SUM */
  uint32_t* device_status; /* optional, as kvc_params_t */
} kvc_attn_params_t;

#define KVC_ATTN_OLD_DTYPE(d) ((int32_t)(d) + 1) /* kvc_attn_params.flags, bits 0-1 */
/* kvc_attn_params.flags bit 2 (opt-in): kvc_heavy_hitters selects the first n_select of a STABLE
 * descending sort of the head sums (KVC_ALGO_STABLE's tie order) instead of torch.topk's; zones
 * of at most 65 536 positions (else KVC_E_TOO_LONG). */
#define KVC_ATTN_HH_STABLE 4
/* kvc_attn_params.flags bit 3, kvc_attn_accumulate only (kvc_heavy_hitters refuses it): the
 * reference summed attention tensors whose LAST dim has a step (a [..., ::2] view), and `attn`
 * is a last-dim-contiguous copy of each.  torch's CPU sum then runs aten's
 * scalar outer loop instead of the SIMD one: in every loop call the cascade takes whole groups of
 * FOUR columns and row_sum the rest, and the thread chunks of col_chunk columns keep their
 * bounds (no rounding to 128 bytes).  vec_bytes is ignored.  (Additive within ABI 4: a library
 * without the flag refuses it with KVC_E_ARG like every unknown bit.) */
#define KVC_ATTN_SCALAR_SUM 8

/* One layer of update_attention_scores (:100-154). */
typedef struct kvc_attn_layer {
  const void* attn;       /* [batch, heads, q_len, key_len], last dim contiguous */
  int64_t attn_stride[3]; /* element strides of batch, heads, q */
  const void* acc_old;    /* [batch, heads, old_len] contiguous (NULL when old_len == 0) */
  void* acc_new;          /* [batch, heads, key_len] contiguous, written */
  int32_t q_len;          /* >= 1 */
  int32_t key_len;        /* >= 1 */
  int32_t old_len;        /* 0: first update or reset (:118-123, :138-144); else <= key_len:
                             columns [0, old_len) carry acc_old * decay (:129-137, :145-146) */
  int32_t col_chunk;      /* columns per reference thread chunk of the q-sum; 0 = one chunk */
} kvc_attn_layer_t;

/* One layer of get_heavy_hitter_indices (:183-213). */
typedef struct kvc_hh_layer {
  const void* acc;        /* [batch, heads, acc_len] contiguous */
  int32_t acc_len;
  int32_t zone_start;     /* middle_start (:187) */
  int32_t zone_len;       /* middle_end - middle_start >= 1 (:188, :205) */
  int32_t n_select;       /* min(heavy_hitter_size, zone_len) (:206) */
  int32_t col_chunk;      /* columns per reference thread chunk of the head sum; 0 = one */
  int32_t reserved;       /* 0 */
} kvc_hh_layer_t;

/* acc_new of every layer (one kernel per chunk of layers). */
int kvc_attn_accumulate(const kvc_attn_params_t* params, const kvc_attn_layer_t* layers,
                        int num_layers, kvc_stream_t stream);

/* Workspace kvc_heavy_hitters needs for this table. */
int kvc_hh_workspace(const kvc_attn_params_t* params, const kvc_hh_layer_t* layers,
                     int num_layers, size_t* bytes);

/* Heavy hitters of every layer: row (layer*batch + b) of out_idx (int32, row stride
 * out_row_stride >= max n_select) receives the n_select ascending zone-local indices of
 * torch.topk(head_sum, n_select) (:198-211).  With out_idx = the index region of a
 * KVC_FLAG_SHARED_INDEX gather plan, kvc_launch then compacts K/V (:305-361). */
int kvc_heavy_hitters(const kvc_attn_params_t* params, const kvc_hh_layer_t* layers,
                      int num_layers, int32_t* out_idx, int64_t out_row_stride, void* workspace,
                      size_t workspace_bytes, kvc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* KVC_H */
