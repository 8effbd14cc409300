/*
 * arrowhip.h — C ABI of libarrowhip.so: MI355X (gfx950) kernels for the hot path of
 * arrow-go's arrow/compute + arrow/math kernel registry.
 *
 * This is the drop-in boundary.  Each entry point replaces one leaf the Go code
 * reaches today through c2goasm Plan9 assembly (or a pure-Go loop); the citation on
 * each declaration is the reference interface it replaces (paths relative to the
 * arrow-go tree).  A Go maintainer binds these with cgo (INTEGRATION.md shows the
 * stubs); nothing here mentions torch, C++ or HIP types.
 *
 * Conventions
 *   - every function returns an int status: AH_OK or an error class; the message is
 *     available from ah_last_error(ctx) until the next call on that ctx.
 *   - pointers named *_host are host memory, read or written before the call
 *     returns (the library never retains a host pointer — the cgo pointer rule);
 *     all other data pointers are DEVICE pointers (from ah_buf_alloc, or any
 *     hipMalloc'd / torch-allocated memory on the ctx's device).
 *   - bitmaps are Arrow validity/boolean bitmaps: LSB-first, bit i of the logical
 *     array is bit ((off + i) & 7) of byte ((off + i) >> 3).  A NULL validity
 *     pointer means "all valid" (ArraySpan.Buffers[0].Buf == nil).
 *   - kernels are enqueued on the ctx's compute stream and the call returns without
 *     waiting, EXCEPT when the signature has a *_host output: those calls
 *     synchronise the stream before returning.  ah_sync() waits for everything (and returns
 *     AH_EHIP if a kernel reported since the last synchronisation that it gave up waiting for
 *     another workgroup — the one-pass cumulative sums' bounded look-back; that call's output is invalid).
 *   - an ah_ctx may be used from any OS thread (every entry point selects the
 *     ctx's device first — Go's executor goroutine may migrate between threads,
 *     compute/exec.go:165) but serves one call at a time.
 *   - buffers must not alias unless stated; sizes are in ELEMENTS unless named
 *     nbytes / nbits.
 *   - a call writes nothing outside the bytes its declaration gives an output — for a
 *     bitmap, nothing outside the bits the declaration gives — whether it succeeds or
 *     returns an error; data pointers need the alignment of their element type and no
 *     more (an output may be an interior slice of a larger buffer).
 */
#ifndef ARROWHIP_H
#define ARROWHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status classes ------------------------------------------------------ */
#define AH_OK 0
#define AH_EINVALID 1   /* arrow.ErrInvalid */
#define AH_EINDEX 2     /* arrow.ErrIndex ("<v> out of bounds") */
#define AH_EOVERFLOW 3  /* arrow.ErrInvalid: "overflow" (kernels/base_arithmetic.go errOverflow) */
#define AH_EHIP 4       /* HIP runtime failure */
#define AH_ENOTIMPL 5   /* arrow.ErrNotImplemented */

/* arrow.Type ids passed verbatim — arrow/datatype.go:36-72 == kernels/_lib/types.h:20-34 */
#define AH_BOOL 1                /* a bitmap column, where an entry says it takes one (ah_format_int_*) */
#define AH_UINT8 2
#define AH_INT8 3
#define AH_UINT16 4
#define AH_INT16 5
#define AH_UINT32 6
#define AH_INT32 7
#define AH_UINT64 8
#define AH_INT64 9
#define AH_FLOAT32 11
#define AH_FLOAT64 12
#define AH_BINARY 14             /* also String: same bytes, same order */
#define AH_FIXED_SIZE_BINARY 15
#define AH_DECIMAL128 23
#define AH_DECIMAL256 24
#define AH_LARGE_BINARY 35       /* also LargeString */

/* ArithmeticOp — kernels/base_arithmetic.go:37-82 == kernels/_lib/base_arithmetic.cc:31-74 */
#define AH_OP_ADD 0
#define AH_OP_SUB 1
#define AH_OP_MUL 2
#define AH_OP_ABS 4
#define AH_OP_NEGATE 5
#define AH_OP_SIGN 20
#define AH_OP_DIV 3               /* ah_arithmetic_ext ops: the reference's ArithmeticOp numbering where it has one … */
#define AH_OP_SQRT 6
#define AH_OP_DIV_CHECKED 24
#define AH_OP_ABS_CHECKED 25
#define AH_OP_NEGATE_CHECKED 26
#define AH_OP_SQRT_CHECKED 27
#define AH_OP_POWER 7             /* OpPower / OpPowerChecked (base_arithmetic.go:46,71) */
#define AH_OP_POWER_CHECKED 28
#define AH_OP_SHIFT_LEFT 64       /* … and private numbers for the shift / bit-wise kernels (scalar_arithmetic.go) */
#define AH_OP_SHIFT_LEFT_CHECKED 65
#define AH_OP_SHIFT_RIGHT 66
#define AH_OP_SHIFT_RIGHT_CHECKED 67
#define AH_OP_BIT_AND 68
#define AH_OP_BIT_OR 69
#define AH_OP_BIT_XOR 70
#define AH_OP_BIT_NOT 71
#define AH_OP_FLOOR 72             /* floor / ceil / trunc (kernels/rounding.go:180-187, 748-775) */
#define AH_OP_CEIL 73
#define AH_OP_TRUNC 74
#define AH_OP_ADD_CHECKED 21
#define AH_OP_SUB_CHECKED 22
#define AH_OP_MUL_CHECKED 23

/* cmpop — kernels/_lib/scalar_comparison.cc:172-178; LESS/LESS_EQUAL are the
 * caller's operand swap, exactly as compute/scalar_compare.go:73-99 does it. */
#define AH_CMP_EQ 0
#define AH_CMP_NE 1
#define AH_CMP_GT 2
#define AH_CMP_GE 3
/* operand shapes: array∘array, array∘scalar, scalar∘array (kernels/helpers.go:193-236) */
#define AH_SHAPE_AA 0
#define AH_SHAPE_AS 1
#define AH_SHAPE_SA 2
/* bitOp — arrow/bitutil/bitmaps.go:494-521 */
#define AH_BIT_AND 0
#define AH_BIT_OR 1
#define AH_BIT_XOR 2
#define AH_BIT_AND_NOT 3
#define AH_BIT_XNOR 4
/* Kleene ops — compute/scalar_bool.go:94-110 */
#define AH_KLEENE_AND 0
#define AH_KLEENE_OR 1
#define AH_KLEENE_AND_NOT 2
/* NullSelectionBehavior — kernels/vector_selection.go:34-39 */
#define AH_DROP_NULLS 0
#define AH_EMIT_NULLS 1

/* ---- context ------------------------------------------------------------- */
typedef struct ah_ctx ah_ctx; /* device id, compute stream, copy stream, scratch arena */

/* Own streams (compute + copy). */
int ah_ctx_create(int device_id, ah_ctx** out);
/* Borrow an existing hipStream_t as the compute stream (e.g. torch's current
 * stream, so torch.distributed collectives order naturally after our kernels). */
int ah_ctx_create_on_stream(int device_id, void* hip_stream, ah_ctx** out);
void ah_ctx_destroy(ah_ctx* ctx);
const char* ah_last_error(ah_ctx* ctx); /* never NULL; owned by ctx */
/* measurement / test switches of one context; none changes a result.  "nt" (nontemporal streaming accesses 0|1),
 * "blocks_per_cu" (grid cap of grid-stride kernels, 0 = each kernel's default), "take_binned" (0 never, 1 auto, 2 whenever
 * legal), "take_window_log2" (bytes of values per bin), "take_hint_cache" (1, the default of ah_ctx_create: the neighbour sample that picks a Take's path is kept for the
 * Take that directly follows with the same index vector — one vector gathers all columns of a record batch —, dropped like the filter cache by every other
 * compute entry point and by uploads / copies / memsets into the vector, sampled again on every 32nd use; every path returns the same bytes, so an entry
 * gone stale behind the library's back costs speed, never results; 0, the default of ah_ctx_create_on_stream: sample on every call), "take_gather_wg_per_cu", "take_gather_load", "scan_segment_log2",
 * "hash_direct" (unique / dictionary_encode: 0 ids in a separate pass … 2 default, 3 without the re-packed table),
 * "hash_sum_partition" (id-based hash + sum above 4096 groups: 1 default, 0 plain device atomics),
 * "groupby_partition" (hash + sum: 0 id-based path only, 1 auto, k >= 5 always 2^(k-2) partitions, 2 sort-based, 3 / 4 two levels,
 * -2 no cut), "groupby_keys" (expected keys per partition the auto choice aims at, default 1280), "sort_msd" (sort_indices:
 * 0 LSD passes only, 1 auto), "groupby_seed" (hash + sum with few groups: 1 the workgroups' LDS tables start from the keys a quick look
 * found and are added up slot by slot, 0 empty tables merged with atomics), "groupby_lean" (same path: 0 keep a pending group per lane,
 * 1 leave it out when neighbouring rows rarely share a key, 2 always leave it out), "groupby_reserve" (partitioned hash + sum: 1 the
 * scatter reserves its runs in per-(partition, XCD) regions sized from the key sample — no histogram pass —, 0 histogram first), "scan_onepass" (cumulative_sum of 4- /
 * 8-byte integers, and of unchecked 2-byte ones without nulls: 1 one pass with decoupled look-back, the output's validity and null count written by the same kernel, 0 reduce-then-scan, 2 one pass with
 * a separate bitmap copy + popcount, 3 one pass for unchecked columns without nulls only — 2 and 3 are measurement switches), "filter_cache" (1: ah_filter_count leaves its tile prefixes for the ah_filter_primitive that
 * follows, dropped by every entry point of THIS context that may write device memory — the default of ah_ctx_create; 0: the fill
 * always recounts — the default of ah_ctx_create_on_stream, where another producer on the shared stream may rewrite the mask
 * between the two calls; set it to 1 there only if nothing else writes the mask in between), "string_tile_bytes" (the string searches:
 * bytes of the value buffer a workgroup stages per LDS tile, 0 = 16384, else 64 … 32768 — so that a test can put tile borders where
 * it wants them).  Defaults come from the ARROWHIP_*
 * environment variables of the same names at context creation. */
int ah_ctx_set_option(ah_ctx* ctx, const char* name, int64_t value);
const char* ah_version(void);
int ah_device_count(int* n_host);

/* ---- buffers (back a Go memory.Allocator: arrow/memory/allocator.go:23-27) - */
int ah_buf_alloc(ah_ctx* ctx, size_t nbytes, void** dptr_host);      /* 256-B aligned, NOT zeroed */
int ah_buf_free(ah_ctx* ctx, void* dptr);
int ah_host_alloc_pinned(ah_ctx* ctx, size_t nbytes, void** hptr_host);
int ah_host_free_pinned(ah_ctx* ctx, void* hptr);
/* copies run on the copy stream; the compute stream is made to wait for an upload,
 * a download waits for the compute work enqueued so far.  hptr should be pinned
 * (pageable memory works but the runtime stages it). */
int ah_upload_async(ah_ctx* ctx, void* dptr, const void* hptr, size_t nbytes);
int ah_download_async(ah_ctx* ctx, void* hptr, const void* dptr, size_t nbytes);
int ah_memset_async(ah_ctx* ctx, void* dptr, int byte_value, size_t nbytes); /* arrow/memory/_lib/memory.c:20-27 */
/* device → device, ordered on the compute stream: the value-range copies of array.Concatenate
 * (arrow/array/concat.go:159-180 concatBuffers) when chunked inputs are laid end to end in HBM */
int ah_copy_async(ah_ctx* ctx, void* dst, const void* src, size_t nbytes);
int ah_sync(ah_ctx* ctx);
/* ---- hipGraph capture: many launch-bound calls, one submission ----------------------------------------------------------------
 * No reference analogue.  Between ah_graph_begin and ah_graph_end the calls on this context are RECORDED, not run; ah_graph_launch
 * replays the sequence (same pointers, same lengths — new contents) with one submission to the compute stream.  Capturable: the
 * calls that neither wait for the device nor allocate — element-wise arithmetic, comparisons, bitmap / Kleene ops, copies and
 * memsets, the *_dev flavours (ah_sum_*_dev, ah_cmp_filter_sum_*_dev, ah_filter_primitive_dev, ah_take_primitive_dev),
 * ah_cumulative_sum without a null count — after ONE eager call of the same sequence (the scratch arenas get their size there).
 * A call with a *_host result invalidates the capture; ah_graph_end then fails and nothing was run.  The recorded launches point into
 * the context's work areas: if a later, larger call grows one of them, ah_graph_launch refuses the stale graph (AH_EINVALID) — record again. */
typedef struct ah_graph ah_graph;
int ah_graph_begin(ah_ctx* ctx);
int ah_graph_end(ah_ctx* ctx, ah_graph** out);
int ah_graph_launch(ah_ctx* ctx, ah_graph* graph);
int ah_graph_destroy(ah_graph* graph);
/* pin / unpin memory the host already owns (hipHostRegister) — e.g. a Go []byte for the duration of one cgo call; copies from
 * pageable memory are staged by the runtime and overlap nothing */
int ah_host_register(ah_ctx* ctx, void* hptr, size_t nbytes);
int ah_host_unregister(ah_ctx* ctx, void* hptr);

/* ---- overlapped host -> HBM ingest (csrc/ah_ingest.hip) ----------------------------------------------------------------------
 * Replaces, for host-resident inputs, the executor's span loop: ExecCtx.ChunkSize / NumParallel (arrow/compute/executor.go:46-64)
 * and the per-span kernel call (:658-702), over buffers from a memory.Allocator (arrow/memory/allocator.go:20-27 — here
 * ah_host_alloc_pinned).  An ah_ingest owns `depth` slots of three `chunk_bytes` device buffers, an upload stream and a download
 * stream; chunk k + 1 uploads while chunk k computes and chunk k - 1 downloads, ordered by per-slot events (not by the
 * stream-wide fences of ah_upload_async).  chunk_bytes = 0 -> 32 MiB, depth = 0 -> 3.  Host buffers must be pinned
 * (ah_host_alloc_pinned / ah_host_register) for the copies to overlap; pageable memory still gives correct results.
 * One call at a time per ah_ingest; it shares its context's compute stream. */
typedef struct ah_ingest ah_ingest;
int ah_ingest_create(ah_ctx* ctx, size_t chunk_bytes, int depth, ah_ingest** out);
int ah_ingest_destroy(ah_ingest* ing);
/* arrow/math Sum of a HOST column (float64.go:34-47 / int64.go:34-47; validity ignored): every chunk's double-double workgroup
 * partials are kept and reduced ONCE, so the result has the rounding of ah_sum_float64 over the whole column */
int ah_ingest_sum_float64(ah_ingest* ing, const double* buf_host, size_t len, double* res_host);
int ah_ingest_sum_int64(ah_ingest* ing, const int64_t* buf_host, size_t len, int64_t* res_host);
/* ah_arithmetic_binary with all three buffers on the host (base_arithmetic.cc:441-475) */
int ah_ingest_arithmetic_binary(ah_ingest* ing, int type, int8_t op, const void* l_host, const void* r_host, void* out_host, int64_t len);
/* PrimitiveFilter (vector_selection.go:449-520) on host buffers, two-phase like ah_filter_count / ah_filter_primitive: the count
 * call uploads the selection vector (n/8 bytes) and KEEPS it on the device; the host allocates the outputs; the fill call
 * streams the values through (chunks with no survivor never cross PCIe) and returns values, validity (out_valid_host nullable:
 * pass NULL when no input has nulls) and null count.  Same payload rules as ah_filter_primitive. */
int ah_ingest_filter_count(ah_ingest* ing, const uint8_t* fdata_host, const uint8_t* fvalid_host, int64_t foff, int64_t n, int null_sel,
                           int64_t* n_out_host);
int ah_ingest_filter_primitive(ah_ingest* ing, int byte_width, const void* values_host, const uint8_t* vvalid_host, int64_t voff, int64_t n,
                               int64_t n_out, void* out_values_host, uint8_t* out_valid_host, int64_t* out_null_count_host);
/* The slot protocol itself, for a host that runs other kernels over its own chunking (go/arrowhip/register.go stage()):
 *   upload(slot, which, …, first_of_chunk=1 for the chunk's first copy)   h2d stream; waits only for the slot's last release
 *   ready(slot, writes_output)                                            compute stream waits for the slot's uploads
 *                                                                          (and, if the kernel writes buffer 2, for its last download)
 *   … any ah_* kernels on ah_ingest_slot_buffer(slot, 0..2) …
 *   release(slot)                                                          marks the kernels done
 *   download(slot, which, …)                                               d2h stream; waits for the release
 *   wait()                                                                 host waits for all three streams */
int ah_ingest_depth(ah_ingest* ing);
size_t ah_ingest_chunk_bytes(ah_ingest* ing);
void* ah_ingest_slot_buffer(ah_ingest* ing, int slot, int which);
int ah_ingest_slot_upload(ah_ingest* ing, int slot, int which, size_t dst_offset, const void* hptr, size_t nbytes, int first_of_chunk);
int ah_ingest_slot_ready(ah_ingest* ing, int slot, int writes_output);
int ah_ingest_slot_release(ah_ingest* ing, int slot);
int ah_ingest_slot_download(ah_ingest* ing, int slot, int which, size_t src_offset, void* hptr, size_t nbytes);
int ah_ingest_wait(ah_ingest* ing);
/* hipEvent pair on the compute stream (what bench.py times kernels with). */
int ah_timer_start(ah_ctx* ctx);
int ah_timer_stop(ah_ctx* ctx, float* ms_host); /* synchronises */
/* numbered event slots (0..65535): bracket single kernels inside a longer timed region
 * without synchronising in between; elapsed_ms waits for slot_b only. */
int ah_event_record(ah_ctx* ctx, int slot);
int ah_event_elapsed_ms(ah_ctx* ctx, int slot_a, int slot_b, float* ms_host);

/* ---- arrow/math Sum -------------------------------------------------------
 * replaces _sum_float64_avx2 / sum_float64_go (arrow/math/float64_avx2_amd64.go:33-42,
 * arrow/math/float64.go:41-47; C truth arrow/math/_lib/float64.c:20-26) and the
 * int64/uint64 twins (arrow/math/_lib/int64.c:21-27, uint64.c).  Validity is
 * ignored exactly as the reference ignores it.  len == 0 → 0.
 * float64: every lane accumulates in double-double (TwoSum), so the result is the
 * exact sum rounded once (≤ 1 ULP), independent of launch geometry; see DESIGN.md
 * for why this — not either of the reference's two mutually inconsistent orders —
 * is the parity rule.  int64/uint64: wrapping, bit-exact. */
int ah_sum_float64(ah_ctx* ctx, const double* buf, size_t len, double* res_host);
int ah_sum_int64(ah_ctx* ctx, const int64_t* buf, size_t len, int64_t* res_host);
int ah_sum_uint64(ah_ctx* ctx, const uint64_t* buf, size_t len, uint64_t* res_host);
/* same, result left in device memory (8 bytes), no synchronisation */
int ah_sum_float64_dev(ah_ctx* ctx, const double* buf, size_t len, double* res_dev);
int ah_sum_int64_dev(ah_ctx* ctx, const int64_t* buf, size_t len, int64_t* res_dev);

/* ---- element-wise arithmetic ------------------------------------------------
 * replace _arithmetic_binary_avx2 / _arithmetic_arr_scalar_avx2 /
 * _arithmetic_scalar_arr_avx2 / _arithmetic_unary_same_types_avx2
 * (kernels/base_arithmetic_avx2_amd64.go:27-60; C truth
 * kernels/_lib/base_arithmetic.cc:465-483).  op ∈ {ADD, SUB, MUL} (the *_CHECKED
 * ids alias the unchecked op, as in the C source :54-57); every slot is computed,
 * null payloads included.  Scalars are read from host memory (one element). */
int ah_arithmetic_binary(ah_ctx* ctx, int type, int8_t op, const void* l, const void* r, void* out, int64_t len);
int ah_arithmetic_arr_scalar(ah_ctx* ctx, int type, int8_t op, const void* l, const void* r_host, void* out, int64_t len);
int ah_arithmetic_scalar_arr(ah_ctx* ctx, int type, int8_t op, const void* l_host, const void* r, void* out, int64_t len);
int ah_arithmetic_unary(ah_ctx* ctx, int type, int8_t op, const void* in, void* out, int64_t len); /* ABS, NEGATE, SIGN */
/* checked integer ADD/SUB/MUL — replaces the pure-Go ScalarBinaryNotNull path
 * (kernels/base_arithmetic.go:249-286, kernels/helpers.go:284-380): ADD/SUB write 0
 * under null slots and test only valid slots; MUL evaluates every slot
 * (mulWithOverflow :84-106).  Returns AH_EOVERFLOW ("overflow") if any tested slot
 * overflowed by the reference's own carry test; `out` is then unspecified, as the
 * reference discards it.  For AS/SA shapes the scalar operand pointer is host
 * memory and scalar_valid says whether the scalar is non-null.  Synchronises. */
int ah_arithmetic_checked(ah_ctx* ctx, int type, int8_t op, int shape,
                          const void* l, const uint8_t* lvalid, int64_t loff,
                          const void* r, const uint8_t* rvalid, int64_t roff,
                          int scalar_valid, void* out, int64_t len);

/* The exact rest of the arithmetic registry — no assembly leaf in the reference (base_arithmetic_amd64.go:67-105
 * keeps these in Go), signature derived from the Go closures.  Same argument meaning as ah_arithmetic_checked;
 * unary ops ignore r / shape.
 *   DIV, DIV_CHECKED (divide_unchecked, divide; base_arithmetic.go:154-160,287-294,386-396): integers refuse a zero
 *       divisor in a valid slot under BOTH names (AH_EINVALID "divide by zero"), truncated quotient, MinInt / −1
 *       wraps; floats: IEEE a / b, the checked name refuses b == 0.  Null slots hold 0 (ScalarBinaryNotNull).
 *   ABS_CHECKED, NEGATE_CHECKED (abs, negate; :295-340,398-411): MinInt in ANY slot, null or not, is
 *       AH_EOVERFLOW "overflow" (ScalarUnary walks the whole value buffer); unsigned abs copies; no unsigned negate.
 *   BIT_AND / OR / XOR (bit_wise_*; scalar_arithmetic.go:170-245): every slot.  BIT_NOT (:253-268): null slots hold 0.
 *   SHIFT_LEFT / RIGHT [_CHECKED] (:293-378): a count outside [0, bits − 2] (signed) / [0, bits − 1] (unsigned)
 *       returns the left operand; the checked names make it AH_EINVALID "shift amount must be >= 0 and less than
 *       precision of type".  Null slots hold 0.
 *   SQRT (every slot), SQRT_CHECKED (null slots 0; a negative valid value is AH_EINVALID "square root of negative
 *       number"; :412-426): correctly rounded IEEE sqrt, floats only.
 *   FLOOR, CEIL, TRUNC (floor, ceil, trunc; rounding.go:180-187,748-775): every slot, floats only.
 *   POWER (power_unchecked; base_arithmetic.go:226-248): integers right-to-left in uint64, narrowed (wraps), EVERY slot;
 *       POWER_CHECKED (power; :342-373): left-to-right with mulWithOverflow → AH_EOVERFLOW "overflow", valid slots only,
 *       null slots 0.  A negative integer exponent is AH_EINVALID "integers to negative integer powers are not allowed"
 *       under both.  Floats (:443-446): pow in double under both names, every slot, never fails. */
int ah_arithmetic_ext(ah_ctx* ctx, int type, int op, int shape, const void* l, const uint8_t* lvalid, int64_t loff, const void* r,
                      const uint8_t* rvalid, int64_t roff, int scalar_valid, void* out, int64_t len);

/* round / round_to_multiple on Float32 / Float64 (kernels/rounding.go:321-370 round[T].call, :562-598
 * roundToMultiple[T].call; ScalarUnaryNotNull → null slots hold 0).  mode = RoundMode (rounding.go:40-59: 0 Down, 1 Up,
 * 2 TowardsZero, 3 AwayFromZero, 4 HalfDown, 5 HalfUp, 6 HalfTowardsZero, 7 HalfAwayFromZero, 8 HalfToEven, 9 HalfToOdd).
 * multiple_host == NULL: round to ndigits, pow10 = math.Pow10(|ndigits|) computed by the caller exactly as
 * InitRoundState does (:72-91); else *multiple_host (one element of `type`, positive) is the rounding multiple and
 * ndigits / pow10 are ignored.  A non-finite result in a valid slot is AH_EOVERFLOW "overflow". */
int ah_round(ah_ctx* ctx, int type, const void* values, const uint8_t* valid, int64_t off, int64_t n, int64_t ndigits, int mode,
             const void* multiple_host, double pow10, void* out);

/* ---- comparisons → packed bitmap ----------------------------------------------
 * replaces the 12 _comparison_<op>_<shape>_avx2 symbols
 * (kernels/scalar_comparison_avx2_amd64.go; C truth
 * kernels/_lib/scalar_comparison.cc:210-256).  out_bits points at the byte holding
 * the first output bit, out_bit_offset % 8 is the bit prefix inside it (the
 * reference passes out.Offset; kernels/scalar_comparisons.go:199-218).  Only bits
 * [prefix, prefix+length) are written. */
int ah_comparison(ah_ctx* ctx, int cmpop, int shape, int type, const void* l, const void* r,
                  uint8_t* out_bits, int64_t length, int out_bit_offset);
/* One operand of ah_compare_binary.  Base-binary (String / Binary / LargeString / LargeBinary): offset_width 4 or 8,
 * `offsets` the offsets buffer, `data` the value bytes; row i is data[offsets[off + i] … offsets[off + i + 1]).  Fixed
 * slots (FixedSizeBinary): offset_width 0, row i is the byte_width bytes at data + (off + i)·byte_width.  broadcast = 1:
 * a scalar, every row reads element `off`.  Buffers are DEVICE memory; the descriptor itself is host memory. */
typedef struct ah_cmp_operand {
  int offset_width;
  int byte_width;
  const void* offsets;
  const uint8_t* data;
  int64_t off;
  int broadcast;
} ah_cmp_operand;
/* equal / not_equal / greater / greater_equal of byte strings (getBinaryCmp, kernels/scalar_comparisons.go:520-540, in
 * the base-binary and FixedSizeBinary kernels of CompareKernels, :694-713): bytes.Equal / bytes.Compare — unsigned
 * bytewise, a proper prefix first.  The two operands may have different layouts (String ∘ LargeBinary, FixedSizeBinary[3]
 * ∘ FixedSizeBinary[1], FixedSizeBinary ∘ String) and need no cast.  Every row is computed, null slots included (the
 * caller owns the validity).  Writes bits [out_bit_offset, out_bit_offset + n) of out_bits, every other bit kept.  No host
 * synchronisation. */
int ah_compare_binary(ah_ctx* ctx, int cmpop, const ah_cmp_operand* l, const ah_cmp_operand* r, int64_t n, uint8_t* out_bits,
                      int64_t out_bit_offset);
/* the same comparisons of Decimal128 / Decimal256 values (genDecimalCompareKernel, kernels/scalar_comparisons.go:370-392)
 * by signed value.  Each side: width 16 or 32 (two's complement, little-endian; a 16-byte side is sign-extended),
 * element offset, broadcast flag (a scalar: every row reads element off) and scale-up exponent k (0 … 76): the side is
 * compared as value · 10^k, the rescale castBinaryDecimalArgs asks for (compute/utils.go:261-326) — exact for every
 * value within the promoted precision (≤ 76 digits).  Output as ah_compare_binary.  No host synchronisation. */
int ah_compare_decimal(ah_ctx* ctx, int cmpop, int l_width, const uint8_t* l, int64_t l_off, int l_broadcast, int l_scaleup,
                       int r_width, const uint8_t* r, int64_t r_off, int r_broadcast, int r_scaleup, int64_t n,
                       uint8_t* out_bits, int64_t out_bit_offset);

/* ---- null-bitmap utilities -----------------------------------------------------
 * replace bitutil.BitmapAnd/Or/Xor/AndNot/Xnor (arrow/bitutil/bitmaps.go:592-637 →
 * _bitmap_aligned_*_avx2, arrow/bitutil/bitmap_ops_avx2_amd64.go:26-52, plus the Go
 * unaligned path :568-582), CountSetBits (arrow/bitutil/bitutil.go:89-130),
 * CopyBitmap/InvertBitmap (bitmaps.go:483-493), SetBitsTo (bitutil.go:158-204) and
 * the Kleene word kernels (kernels/scalar_boolean.go:29-65).  Arbitrary,
 * independent bit offsets; only bits [ooff, ooff+nbits) of the output change. */
int ah_bitmap_op(ah_ctx* ctx, int op, const uint8_t* l, int64_t loff, const uint8_t* r, int64_t roff,
                 uint8_t* out, int64_t ooff, int64_t nbits);
int ah_count_set_bits(ah_ctx* ctx, const uint8_t* bits, int64_t off, int64_t nbits, int64_t* out_host);
int ah_copy_bitmap(ah_ctx* ctx, const uint8_t* src, int64_t soff, int64_t nbits, uint8_t* dst, int64_t doff, int invert);
int ah_set_bits_to(ah_ctx* ctx, uint8_t* bits, int64_t off, int64_t nbits, int value);
int ah_kleene(ah_ctx* ctx, int op, const uint8_t* lvalid, const uint8_t* ldata, int64_t loff,
              const uint8_t* rvalid, const uint8_t* rdata, int64_t roff,
              uint8_t* ovalid, uint8_t* odata, int64_t ooff, int64_t nbits);

/* ---- selection -------------------------------------------------------------------
 * Filter: data-dependent output size and Go owns allocation, so the protocol is the
 * reference's own two steps: ah_filter_count == getFilterOutputSize
 * (kernels/vector_selection.go:57-81), caller allocates n_out*byte_width bytes (+
 * ceil(n_out/8) validity bytes iff either input has nulls — preallocateData :83-93,
 * PrimitiveFilter :486-488), then ah_filter_primitive == primitiveFilterImpl
 * (:267-395).  n_out is the value ah_filter_count returned (the library zero-fills
 * the ceil(n_out/8) bytes of out_valid itself and cross-checks n_out when it
 * synchronises; pass -1 only when out_valid is NULL).  Payload rules in DESIGN.md.
 * byte_width ∈ {1,2,4,8}.  out_null_count_host may be NULL (then no sync).
 * The count call leaves the per-tile survivor prefixes of ITS mask in the context, and an ah_filter_primitive with the same
 * (fdata, fvalid, foff, n, null_sel) uses them instead of counting again — as long as nothing that can change device memory was
 * called on this context in between: allocation, synchronisation, timers, and a memset / upload / copy whose destination
 * does not overlap the mask's bytes keep them; every other entry point drops them.  Writing the mask from OUTSIDE this
 * context between the two calls (another context, another library on another stream) breaks the two-phase contract itself —
 * n_out would no longer be the mask's count either. */
int ah_filter_count(ah_ctx* ctx, const uint8_t* fdata, const uint8_t* fvalid, int64_t foff, int64_t n,
                    int null_sel, int64_t* n_out_host);
int ah_filter_primitive(ah_ctx* ctx, int byte_width, const void* values, const uint8_t* vvalid, int64_t voff,
                        const uint8_t* fdata, const uint8_t* fvalid, int64_t foff, int64_t n, int null_sel,
                        int64_t n_out, void* out_values, uint8_t* out_valid, int64_t* out_null_count_host);
/* The same compaction without the count call and without a host round trip, for pipelines that
 * keep going on the stream: out_values holds n·byte_width bytes and out_valid (iff either input has
 * nulls) ceil(n/8) — the worst case — and status_dev[0] = rows selected, status_dev[1] = output
 * null count are left in DEVICE memory (16 bytes, readable after ah_sync or by the next kernel). */
int ah_filter_primitive_dev(ah_ctx* ctx, int byte_width, const void* values, const uint8_t* vvalid, int64_t voff,
                            const uint8_t* fdata, const uint8_t* fvalid, int64_t foff, int64_t n, int null_sel,
                            void* out_values, uint8_t* out_valid, int64_t* status_dev /* [2] */);
/* … and the same in ONE synchronous call: outputs sized for n rows as above, the rows selected and the output null count returned to
 * the host through the polled mailbox — for callers that can afford the worst-case allocation (vector_selection.go:459-475 sizes
 * exactly, at the price of a count call and a second launch after the host has heard back). */
int ah_filter_primitive_once(ah_ctx* ctx, int byte_width, const void* values, const uint8_t* vvalid, int64_t voff,
                             const uint8_t* fdata, const uint8_t* fvalid, int64_t foff, int64_t n, int null_sel,
                             void* out_values, uint8_t* out_valid, int64_t* n_out_host, int64_t* out_null_count_host);
/* GetTakeIndices (kernels/vector_selection.go:102-236), uint32 flavour: the mask as
 * an index vector so FilterRecordBatch can gather N columns with one scan. */
int ah_filter_to_indices(ah_ctx* ctx, const uint8_t* fdata, const uint8_t* fvalid, int64_t foff, int64_t n,
                         int null_sel, int64_t n_out, uint32_t* out_idx, uint8_t* out_valid,
                         int64_t* out_null_count_host);
/* Take == PrimitiveTake (kernels/vector_selection.go:1162-1192 → primitiveTakeImpl
 * :878-988): out[i] = values[idx[i]]; null index or null value → payload 0, validity
 * 0.  byte_width ∈ {1,2,4,8} and, for FSBImpl's slots (:1997-2031: Decimal128/256, 16- and 32-byte binaries), {16,32}; any other
 * width up to 4096 is copied byte by byte (a plain kernel: the reference's own test column is binary(3)).
 * idx_byte_width ∈ {1,2,4,8}; idx_signed selects the bounds rule of
 * checkIndexBounds (kernels/helpers.go:929-957; only valid index slots are checked).
 * An out-of-range valid index returns AH_EINDEX with the first offender (in index
 * order) in *bad_index_host and "<v> out of bounds" as the message; the check is
 * fused into the gather and also runs when bounds_check == 0 (where the reference
 * would panic).  out_valid may be NULL when neither input has nulls.  Synchronises. */
int ah_take_primitive(ah_ctx* ctx, int byte_width, const void* values, const uint8_t* vvalid, int64_t voff,
                      int64_t nvalues, int idx_byte_width, int idx_signed, const void* idx,
                      const uint8_t* ivalid, int64_t ioff, int64_t nidx, int bounds_check,
                      void* out_values, uint8_t* out_valid, int64_t* out_null_count_host,
                      int64_t* bad_index_host);
/* Take without the host round trip: status_dev[0] = POSITION (not value) of the first valid index
 * that is out of range, UINT64_MAX when there is none — the output is then unspecified at the
 * offending rows (payload 0, validity 0) and the caller raises checkIndexBounds' error itself;
 * status_dev[1] = output null count (0 without out_valid).  Device memory, 16 bytes.  The one wait
 * left is the path choice for columns ≥ 64 MiB gathered by ≥ 2^20 indices (a 64 × 255-neighbour sample). */
int ah_take_primitive_dev(ah_ctx* ctx, int byte_width, const void* values, const uint8_t* vvalid, int64_t voff,
                          int64_t nvalues, int idx_byte_width, int idx_signed, const void* idx,
                          const uint8_t* ivalid, int64_t ioff, int64_t nidx,
                          void* out_values, uint8_t* out_valid, uint64_t* status_dev /* [2] */);

/* ---- hashing ------------------------------------------------------------------------
 * unique / dictionary_encode over 8-byte keys == doAppendNumeric[uint64] over
 * hashing.Table[uint64] (kernels/vector_hash.go:359-385,
 * internal/hashing/xxh3_memo_table_types.go:189-294; Int64 and Float64 columns both
 * hash their raw bit patterns, vector_hash.go:604-607).  Dense ids are in
 * FIRST-SEEN ORDER, bit-identical to the sequential memo table.  encode_nulls = 1
 * (unique, NullEncodingEncode): null owns the id at which it was first seen;
 * = 0 (NullEncodingMask): null → id 0 + cleared validity bit.  out_dict must hold
 * min(n, distinct)+1 keys — call with out_dict = NULL first to learn the size if
 * unknown, or size it n+1.  out_ids / out_ids_valid may be NULL.  Synchronises.  ≤ 2^30 rows per call
 * (slot numbers travel through the int32 id column; every reference config is ≤ 2^30 rows). */
int ah_hash_u64_encode(ah_ctx* ctx, const uint64_t* keys, const uint8_t* valid, int64_t off, int64_t n,
                       int encode_nulls, int32_t* out_ids, uint8_t* out_ids_valid, uint64_t* out_dict,
                       int64_t* out_ndict_host, int32_t* out_null_id_host);
/* The same for Binary / String (offset_width 4) and LargeBinary / LargeString (8) values ==
 * doAppendBinary (kernels/vector_hash.go:288-325) over hashing.BinaryMemoTable
 * (internal/hashing/xxh3_memo_table.go:248-341: lookup by hash + bytes.Equal, memo index = position
 * in the builder = order of first occurrence; null via GetOrInsertNull :333-341).  `offsets`: the
 * values' offsets buffer (elements off + i, off + i + 1 delimit row i; validity bit off + i).
 * The memo table's hash (hash_funcs.go:86-124, xxh3 for > 16 bytes) only places entries inside the
 * reference's table and cannot influence ids or dictionary order, so the device uses its own 64-bit
 * hash and compares bytes on tag match.  The dictionary is not copied here: out_first_rows[id]
 * (int64, relative to off, n + 1 entries of room) is the row that first held dictionary entry id —
 * dictionary = ah_take_binary_offsets / _data with those rows as indices (the null entry, if any,
 * points at a null row: zero length, as BinaryBuilder.AppendNull leaves it).  ≤ 2^30 rows per call. */
int ah_hash_binary_encode(ah_ctx* ctx, int offset_width, const void* offsets, const uint8_t* data, const uint8_t* valid, int64_t off,
                          int64_t n, int encode_nulls, int32_t* out_ids, uint8_t* out_ids_valid, int64_t* out_first_rows,
                          int64_t* out_ndict_host, int32_t* out_null_id_host);
/* FixedSizeBinary / Decimal128 / Decimal256 keys of unique / dictionary_encode (kernels/vector_hash.go:608-609, 698: the same
 * BinaryMemoTable, every value byte_width bytes; row i of the call = data + (off + i)·byte_width, validity bit off + i).  ids, index
 * validity, first rows, null id as ah_hash_binary_encode; out_dict (nullable, ndict·byte_width bytes) receives the dictionary —
 * the value at each entry's first row, zeros for the null entry.  Synchronises. */
int ah_hash_fixed_encode(ah_ctx* ctx, int byte_width, const uint8_t* data, const uint8_t* valid, int64_t off, int64_t n, int encode_nulls,
                         int32_t* out_ids, uint8_t* out_ids_valid, int64_t* out_first_rows, uint8_t* out_dict, int64_t* out_ndict_host,
                         int32_t* out_null_id_host);
/* group-by sum (NEW — arrow-go has no hash aggregate; definition in DESIGN.md): groups
 * = dictionary_encode(keys, encode_nulls=1) ids; out_sums[g] = Σ valid vals of group
 * g, out_counts[g] = number of valid vals.  i64 sums wrap and are exact; f64 sums are
 * accumulated in 128-bit fixed point with integer atomics (csrc/ah_hashing.h): the same bytes
 * run after run; a column spanning <= 42 binades gives every group its CORRECTLY ROUNDED exact
 * sum, a wider one (an outlier such as 1e300 next to ordinary values) one scale per group and
 * |err| <= ulp/2 + n_g·2^-94·max_g|x| — inside the sequential definition's n_g·ε·Σ_g|x|.
 * out_first_rows (nullable) receives each group's first
 * row index — what a cross-GPU merge needs to restore the global first-seen order.
 * Outputs sized like out_dict above. */
int ah_hash_sum_f64(ah_ctx* ctx, const uint64_t* keys, const uint8_t* kvalid, int64_t koff,
                    const double* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                    uint64_t* out_keys, double* out_sums, int64_t* out_counts, int64_t* out_first_rows,
                    int64_t* out_ngroups_host, int32_t* out_null_group_host);
int ah_hash_sum_i64(ah_ctx* ctx, const uint64_t* keys, const uint8_t* kvalid, int64_t koff,
                    const int64_t* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                    uint64_t* out_keys, int64_t* out_sums, int64_t* out_counts, int64_t* out_first_rows,
                    int64_t* out_ngroups_host, int32_t* out_null_group_host);
/* group-by min / max (NEW — no reference analogue; definition in DESIGN.md): the groups, their order, out_keys, out_first_rows, the
 * null group and *out_ngroups_host are those of ah_hash_sum_* on the same keys.  out_counts[g] = number of valid vals of group g
 * (Float64: NaNs included), out_mins[g] / out_maxs[g] = the smallest / largest valid value; a group with out_counts[g] == 0 has 8 zero
 * bytes in both.  i64: signed order, u64: unsigned order.  f64: NaNs are ignored, the rest is ordered numerically with -0 < +0
 * (+-inf take part); a group whose valid values are all NaN gives the quiet NaN 0x7FF8000000000000 in both.  The result is a function
 * of the inputs alone: the same bytes run after run and on every path.  Outputs sized like out_dict above (n + 1 entries of room);
 * <= 2^30 rows per call; n == 0: no groups, nothing touched. */
int ah_hash_min_max_i64(ah_ctx* ctx, const uint64_t* keys, const uint8_t* kvalid, int64_t koff,
                        const int64_t* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                        uint64_t* out_keys, int64_t* out_mins, int64_t* out_maxs, int64_t* out_counts,
                        int64_t* out_first_rows, int64_t* out_ngroups_host, int32_t* out_null_group_host);
int ah_hash_min_max_u64(ah_ctx* ctx, const uint64_t* keys, const uint8_t* kvalid, int64_t koff,
                        const uint64_t* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                        uint64_t* out_keys, uint64_t* out_mins, uint64_t* out_maxs, int64_t* out_counts,
                        int64_t* out_first_rows, int64_t* out_ngroups_host, int32_t* out_null_group_host);
int ah_hash_min_max_f64(ah_ctx* ctx, const uint64_t* keys, const uint8_t* kvalid, int64_t koff,
                        const double* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                        uint64_t* out_keys, double* out_mins, double* out_maxs, int64_t* out_counts,
                        int64_t* out_first_rows, int64_t* out_ngroups_host, int32_t* out_null_group_host);

/* One key column of ah_group_ids; row i of the call is element off + i of every buffer and bit off + i of `valid` (nullable).
 * offset_width 4 / 8: String / Binary / LargeString / LargeBinary (offsets = the offsets buffer, data = the data buffer, which
 * may be null when every value is empty); offset_width 0 and byte_width 1 ... 4096: fixed slots of that many bytes in `data`
 * (numeric columns, FixedSizeBinary, Decimal128 / 256); bits = 1 (offset_width and byte_width 0): Boolean, bit off + i of `data`. */
typedef struct ah_group_key {
  int offset_width;
  int byte_width;
  int bits;
  const void* offsets;
  const uint8_t* data;
  const uint8_t* valid;
  int64_t off;
} ah_group_key;
/* Dense group ids of a TUPLE of key columns (NEW — no reference analogue; definition in DESIGN.md §3.2).  Rows i and j are in one
 * group iff, for every column, both are null or both are valid with equal bytes (var-length columns: equal length and equal
 * bytes).  The payload under a null is never looked at.  Keys are bytes: -0.0 and +0.0 are two keys, NaNs with different payloads
 * are different keys — as the 8-byte entry points treat their words.  A null is one more value of its column, so (null, "a"),
 * (null, "b"), (1, null) and (null, null) are four groups; there is no "null group" output.  out_ids[i] (n int32) = the group of
 * row i, dense, in first-seen order; out_first_rows[g] (int64, n + 1 entries of room) = the first row of group g — the groups' key
 * values are each key column gathered at these rows (ah_take_*).  *out_ngroups_host = the number of groups.
 * 1 <= nkeys <= 8; n <= 2^30.  The descriptor array is host memory, the buffers are device memory.  Synchronises.  n == 0: no
 * groups, nothing touched.  With nkeys == 1 ids, first rows and count are those of ah_hash_u64_encode / ah_hash_binary_encode /
 * ah_hash_fixed_encode with encode_nulls = 1 on that column (for 8-byte, var-length and other fixed columns the call IS that
 * encoder).  Tuples of fixed-width and Boolean columns whose value bits plus one bit per column with a validity buffer are <= 64
 * are packed into one 8-byte word per row and take the 8-byte encoder with all of its routes; every other tuple is hashed and
 * compared column by column where it lies. */
int ah_group_ids(ah_ctx* ctx, int nkeys, const ah_group_key* keys, int64_t n, int32_t* out_ids, int64_t* out_first_rows,
                 int64_t* out_ngroups_host);
/* The aggregates of ah_hash_sum_* / ah_hash_min_max_* over CALLER-SUPPLIED dense group ids (ah_group_ids, or one of the encoders
 * with encode_nulls = 1).  PRECONDITION: 0 <= ids[i] < ngroups for every row i; the ids are not checked, and the behaviour with an
 * id outside that range is undefined.  Sum, count,
 * minimum, maximum, the NaN rules and the count-0 rule are exactly those of ah_hash_sum_* / ah_hash_min_max_*, and so are the bytes:
 * out_sums / out_mins / out_maxs / out_counts hold ngroups entries each, all of them written (a group without valid values: zeros).
 * ngroups < 2^31, n <= 2^30; ngroups == 0: nothing touched. */
int ah_group_sum_i64(ah_ctx* ctx, const int32_t* ids, int64_t ngroups, const int64_t* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                     int64_t* out_sums, int64_t* out_counts);
int ah_group_sum_f64(ah_ctx* ctx, const int32_t* ids, int64_t ngroups, const double* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                     double* out_sums, int64_t* out_counts);
int ah_group_min_max_i64(ah_ctx* ctx, const int32_t* ids, int64_t ngroups, const int64_t* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                         int64_t* out_mins, int64_t* out_maxs, int64_t* out_counts);
int ah_group_min_max_u64(ah_ctx* ctx, const int32_t* ids, int64_t ngroups, const uint64_t* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                         uint64_t* out_mins, uint64_t* out_maxs, int64_t* out_counts);
int ah_group_min_max_f64(ah_ctx* ctx, const int32_t* ids, int64_t ngroups, const double* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                         double* out_mins, double* out_maxs, int64_t* out_counts);
/* The same aggregates for a value column of ANY numeric width (NEW — DESIGN.md §3.2), over the same caller-supplied ids with the same
 * precondition and limits (a row whose id is outside [0, ngroups) touches nothing).  `type`: AH_INT8 ... AH_INT64, AH_UINT8 ...
 * AH_UINT64, AH_FLOAT32, AH_FLOAT64.  Values are loaded at their own width from `vals` (element-aligned) and widened in registers:
 * no 8-byte copy of the column is written.  THE BYTES are those of the 64-bit call on the column cast to Int64 (signed), to UInt64
 * bit patterns (unsigned) or to Float64 (floats):
 *   ah_group_sum_typed      out_sums (ngroups x 8 bytes): wrapping Int64 / wrapping UInt64 / the reproducible, correctly rounded
 *                           Float64 sum with its wide-column route and its non-finite rules (ah_group_sum_i64 / _f64).
 *   ah_group_min_max_typed  out_mins / out_maxs (ngroups entries of the INPUT type): the 64-bit result narrowed back, which is exact;
 *                           NaNs counted but ignored, -0 < +0, an all-NaN group = the type's canonical quiet NaN, count 0 = zero bytes.
 *   ah_group_count          out_counts[g] (int64) = rows of group g whose validity bit is set (vvalid == NULL: every row).  Reads
 *                           the ids and the validity bits only.
 *   ah_group_mean           out_means[g] = (double)sums[g] / (double)counts[g] (IEEE), 0.0 where counts[g] == 0 — the caller derives
 *                           the validity from the counts.  sum_type: AH_INT64, AH_UINT64 or AH_FLOAT64, how `sums` is read.
 * out_counts is int64, ngroups entries.  n == 0: every group is empty.  ngroups == 0: nothing touched. */
int ah_group_count(ah_ctx* ctx, const int32_t* ids, int64_t ngroups, const uint8_t* vvalid, int64_t voff, int64_t n, int64_t* out_counts);
int ah_group_sum_typed(ah_ctx* ctx, int type, const int32_t* ids, int64_t ngroups, const void* vals, const uint8_t* vvalid, int64_t voff,
                       int64_t n, void* out_sums, int64_t* out_counts);
int ah_group_min_max_typed(ah_ctx* ctx, int type, const int32_t* ids, int64_t ngroups, const void* vals, const uint8_t* vvalid,
                           int64_t voff, int64_t n, void* out_mins, void* out_maxs, int64_t* out_counts);
int ah_group_mean(ah_ctx* ctx, int sum_type, const void* sums, const int64_t* counts, int64_t ngroups, double* out_means);
/* Variance and standard deviation over the same ids (NEW — definition in DESIGN.md §3.2), same preconditions and limits; `type` is any
 * numeric type, read at its own width and taken as cast to Float64 (8-byte integers beyond 2^53 round to nearest even).
 *   ah_group_m2        out_counts[g] = valid rows of group g; out_means[g] = S_g / (double)counts[g], S_g the reproducible Float64 group
 *                      sum — the bytes of ah_group_sum_typed + ah_group_mean on the column cast to Float64, never a wrapped integer sum;
 *                      out_m2[g] = the sum over the group's valid rows of fl(d * d), d = fl(x - out_means[g]), through the 128-bit
 *                      fixed-point accumulator at the group's own scale: within 1 ULP of the exact sum of those terms, and the same
 *                      bytes on every run and launch geometry.  NaN where a valid value or the mean is not finite by the IEEE rules,
 *                      +inf where a square overflows.  A group without valid values: zeros.  Three passes over the column for an
 *                      integer narrower than 8 bytes, four for the other types; temporaries are O(ngroups).  Up to 4096 groups the
 *                      passes accumulate in LDS; above, every pass is device atomics, with no partitioned route: at 2^26 rows and
 *                      2^16 groups a Float64 column takes about 17 ms, 12 x ah_group_sum_typed on it.
 *   ah_group_variance  out[g] = m2[g] / (double)(counts[g] - ddof) (IEEE), its correctly rounded square root with take_sqrt != 0;
 *                      0.0 where counts[g] <= ddof — the caller derives the validity from the counts.  ddof >= 0.
 * n == 0: every group is empty.  ngroups == 0: nothing touched. */
int ah_group_m2(ah_ctx* ctx, int type, const int32_t* ids, int64_t ngroups, const void* vals, const uint8_t* vvalid, int64_t voff,
                int64_t n, double* out_means, double* out_m2, int64_t* out_counts);
int ah_group_variance(ah_ctx* ctx, const double* m2, const int64_t* counts, int64_t ngroups, int ddof, int take_sqrt, double* out);

/* ---- hash join over CALLER-SUPPLIED dense group ids (NEW — no reference analogue: arrow-go has no join; definition in DESIGN.md
 * §3.2a) -------------------------------------------------------------------------------------------------------------------
 * Both sides carry ids from ONE id space (one ah_group_ids call over the left rows followed by the right rows), so equal keys are
 * equal ids.  PRECONDITION, as for the ah_group_* aggregates: 0 <= id < ngroups for every row; the ids are not checked.  Each side
 * has an optional row-validity bitmap (row i = bit off + i); a cleared bit means "a key column is null here": the row matches nothing.
 * Row numbers, starts and offsets are int64.  <= 2^30 rows per side and call.
 *
 * ah_join_build   the build side as a CSR.  out_starts (ngroups + 1 entries): out_starts[g] .. out_starts[g + 1] delimit, in
 *                 out_rows (n_build entries of room), the VALID build rows of group g in ASCENDING row order; out_starts[0] = 0 and
 *                 out_starts[ngroups] = the number of valid rows.  The entries of out_rows behind that are unspecified.  n_build == 0:
 *                 ngroups + 1 zeros, out_rows untouched.  ngroups < 2^31 - 1.  Synchronises (the sort's read-backs).
 * ah_join_count   m[i] = out_starts[id + 1] - out_starts[id] of probe row i, 0 under a cleared validity bit; with emit_unmatched
 *                 (left outer join) max(m[i], 1).  out_offsets (n_probe + 1 entries) = the exclusive scan of m;
 *                 *out_total_host = out_offsets[n_probe], the rows of the result.  Synchronises once.
 * ah_join_expand  the two index vectors of the result, `total` entries each.  Output slot j belongs to the probe row i with
 *                 offsets[i] <= j < offsets[i + 1]: out_probe_rows[j] = i, out_build_rows[j] = rows[starts[id_i] + (j - offsets[i])].
 *                 emit_unmatched: the one slot of a probe row without a match gets build row 0 and a CLEAR bit j in out_build_valid
 *                 (ceil(total / 8) bytes, bit 0 = slot 0; every other slot's bit is set, the bits at and above `total` in the last
 *                 byte are 0) and *out_null_count_host (nullable) = the clear bits below `total`, which takes a synchronisation.
 *                 Without emit_unmatched out_build_valid and out_null_count_host are not touched (the count is set to 0).  starts /
 *                 rows: ah_join_build's; offsets / total: ah_join_count's for the same probe arguments and the same emit_unmatched.
 *                 Nothing behind `total` entries of either vector is written; total == 0 touches nothing.  Work is split by OUTPUT
 *                 SLOT, 2048 per workgroup: a probe row with a million matches costs what a million rows with one match cost.
 * ah_join_match_bits  bit i of out_bits (ceil(n_probe / 8) bytes, written whole, tail bits 0) = probe row i is valid and its
 *                 group holds a valid build row: the mask of a semi join; inverted, of an anti join.  No host synchronisation. */
int ah_join_build(ah_ctx* ctx, const int32_t* build_ids, const uint8_t* build_valid, int64_t voff, int64_t n_build, int64_t ngroups,
                  int64_t* out_starts, int64_t* out_rows);
int ah_join_count(ah_ctx* ctx, const int32_t* probe_ids, const uint8_t* probe_valid, int64_t poff, int64_t n_probe, const int64_t* starts,
                  int emit_unmatched, int64_t* out_offsets, int64_t* out_total_host);
int ah_join_expand(ah_ctx* ctx, const int32_t* probe_ids, const uint8_t* probe_valid, int64_t poff, int64_t n_probe, const int64_t* starts,
                   const int64_t* rows, const int64_t* offsets, int64_t total, int emit_unmatched, int64_t* out_probe_rows,
                   int64_t* out_build_rows, uint8_t* out_build_valid, int64_t* out_null_count_host);
int ah_join_match_bits(ah_ctx* ctx, const int32_t* probe_ids, const uint8_t* probe_valid, int64_t poff, int64_t n_probe,
                       const int64_t* starts, uint8_t* out_bits);

/* ---- LZ4 blocks inflated in HBM (NEW — no reference analogue: the reference inflates IPC bodies on the host, arrow/ipc/
 * compression.go:25-72; definition in DESIGN.md §3.8) ----------------------------------------------------------------
 * src / dst: device memory.  blocks_host: 4 int64 per block {src_off, src_len, dst_off, dst_len}; src_len bit 62 set = stored block
 * (copy).  dst_len <= 65536.  Blocks are independent: a match never reaches in front of its own block's output.
 * out_status_host (nullable, nblocks bytes): 0 ok, 1 corrupt, 2 produced != dst_len; *out_nbad_host (nullable): blocks with a status.
 * A failed block leaves unspecified bytes inside its own dst range and touches nothing else; it is not an error of the call.
 * AH_EINVALID before anything runs if a range lies outside src_bytes / dst_bytes, a dst_len is beyond 65536, or dst_off does not
 * ascend without overlap.  Synchronises once. */
int ah_lz4_decompress_blocks(ah_ctx* ctx, const uint8_t* src, int64_t src_bytes, uint8_t* dst, int64_t dst_bytes,
                             const int64_t* blocks_host, int64_t nblocks, uint8_t* out_status_host, int64_t* out_nbad_host);

/* ---- LZ4 blocks compressed in HBM, and an IPC body put together from them (NEW — no reference analogue: the reference compresses
 * IPC bodies on the host, arrow/ipc/writer.go:430-470, compression.go:66-72; definition in DESIGN.md §3.8) ---------------------
 * ah_lz4_compress_blocks: src / dst: device memory.  blocks_host: 3 int64 per block {src_off, src_len, dst_off}, src_len <= 65536.
 * Block i is compressed on its own (a match never reaches in front of its block) into its slot dst[dst_off, dst_off + src_len);
 * the bytes are a function of the block's bytes alone — not of where the block or its slot lie, and the same on every run.
 * out_sizes_host[i]: bytes written to the slot; out_stored_host[i]: 1 = the block would not have come out smaller than src_len, and
 * its slot holds the src_len input bytes instead (what an LZ4 frame marks with bit 31 of the block size).  src_len == 0: size 0,
 * stored.  Nothing outside the first out_sizes_host[i] bytes of a slot is written.  dst must not overlap src: a block's compressed
 * bytes reach its slot while other blocks are still being read.
 * AH_EINVALID before anything runs if a source range lies outside src_bytes, a src_len is beyond 65536, a slot lies outside
 * dst_bytes, or the slots do not ascend without overlap.  One launch; synchronises once.
 *
 * ah_ipc_pack_body: dst[0, dst_bytes) := the concatenation of nrows pieces.  rows_host: 4 int64 per row {src_off, len, dst_off,
 * word}; word & 3 selects the source — 0: comp (device), 1: plain (device), 2: lits_host (host bytes, uploaded with the rows) —
 * and word bit 8 asks for the 32 bits above bit 32 of word to be written, little-endian, in the 4 bytes BEFORE dst_off (the block
 * size word of an LZ4 frame); every other bit of word must be 0.  The rows must tile the output: row 0 (with its 4 leading bytes,
 * if any) starts at 0, every row starts where the one before it ended, the last ends at dst_bytes — so every byte of dst is
 * written, and written once.  AH_EINVALID before anything runs otherwise, or if a source range lies outside its source.
 * dst must not overlap comp or plain.  One launch; synchronises once. */
int ah_lz4_compress_blocks(ah_ctx* ctx, const uint8_t* src, int64_t src_bytes, uint8_t* dst, int64_t dst_bytes,
                           const int64_t* blocks_host, int64_t nblocks, int32_t* out_sizes_host, uint8_t* out_stored_host);
int ah_ipc_pack_body(ah_ctx* ctx, const uint8_t* comp, int64_t comp_bytes, const uint8_t* plain, int64_t plain_bytes,
                     const uint8_t* lits_host, int64_t lits_bytes, const int64_t* rows_host, int64_t nrows, uint8_t* dst, int64_t dst_bytes);

/* ---- fused Compare(op scalar) → Filter(DropNulls) → Sum ------------------------------
 * NEW entry point (no reference analogue) computing in ONE pass what the reference
 * computes with "greater" → "array_filter" → math.Sum: Σ x[i] over valid slots with
 * x[i] OP threshold, and the survivor count.  8 B/row of HBM traffic instead of
 * 16.25 + 16·s.  *_dev variants leave {sum, count} (16 bytes) in device memory for a
 * following RCCL all-reduce. */
int ah_cmp_filter_sum_i64(ah_ctx* ctx, int cmpop, const int64_t* x, const uint8_t* valid, int64_t off, int64_t n,
                          int64_t threshold, int64_t* out_sum_host, int64_t* out_count_host);
int ah_cmp_filter_sum_f64(ah_ctx* ctx, int cmpop, const double* x, const uint8_t* valid, int64_t off, int64_t n,
                          double threshold, double* out_sum_host, int64_t* out_count_host);
int ah_cmp_filter_sum_i64_dev(ah_ctx* ctx, int cmpop, const int64_t* x, const uint8_t* valid, int64_t off,
                              int64_t n, int64_t threshold, int64_t* out_sum_count_dev /* [2] */);
int ah_cmp_filter_sum_f64_dev(ah_ctx* ctx, int cmpop, const double* x, const uint8_t* valid, int64_t off,
                              int64_t n, double threshold, double* out_sum_dev, int64_t* out_count_dev);

/* ---- cumulative_sum (row §8(f)-2) -----------------------------------------------------------
 * replaces cumulativeSumExec → cumulativeSum{NoNulls,WithNulls}[Checked]
 * (kernels/vector_cumulative.go:228-360) behind "cumulative_sum" / "cumulative_sum_checked"
 * (compute/vector_cumulative.go:76-96): out[i] = start + Σ_{j≤i, valid} in[j]; a null row gives a
 * null output (payload 0) and, unless skip_nulls, turns every later row null as well; checked →
 * AH_EOVERFLOW ("overflow") as soon as a running sum leaves the type's range.  One pass over HBM
 * (decoupled look-back scan).  start_host: one element of `type` or NULL (= 0).  out_valid must be
 * given iff `valid` is (ceil(n/8) bytes, offset 0).  Integers bit-exact; floats are summed in a
 * parallel order (tolerance in DESIGN.md).  Synchronises if checked or out_null_count_host. */
int ah_cumulative_sum(ah_ctx* ctx, int type, const void* values, const uint8_t* valid, int64_t off, int64_t n,
                      const void* start_host, int skip_nulls, int checked, void* out_values, uint8_t* out_valid,
                      int64_t* out_null_count_host);

/* ---- device interchange (row §8(f)-3) ---------------------------------------------------------------
 * ArrowDeviceArray.sync_event (arrow/cdata/abi.h:104-128; for ARROW_DEVICE_ROCM a hipEvent_t*): make
 * the context's compute stream wait for the producer's event before touching imported buffers.
 * NULL = already synchronised.  No host synchronisation. */
int ah_wait_event(ah_ctx* ctx, void* hip_event_ptr);
int ah_device_id(ah_ctx* ctx);

/* ---- min_max (row §8(f)-2) -----------------------------------------------------------------------
 * replaces utils.GetMinMax{Int8…Uint64} (internal/utils/min_max.go:161-215; AVX2 leaves
 * _int64_max_min_avx2(values, len, &min, &max) …, internal/utils/min_max_avx2_amd64.go; C:
 * internal/utils/_lib/min_max.c:23-126).  Integer types; validity is not consulted (as in the
 * reference); an empty input returns (MaxOf, MinOf).  One pass, w bytes per row; synchronises. */
int ah_min_max(ah_ctx* ctx, int type, const void* values, int64_t n, void* out_min_host, void* out_max_host);

/* ---- multi-GPU group merge helper: owner of a key = (hashInt(key) >> 40) mod nparts,
 * hashInt = internal/hashing/hash_funcs.go:60-67.  No reference analogue (the reference is single-process). */
int ah_hash_partition_u64(ah_ctx* ctx, const uint64_t* keys, int64_t n, int nparts, int32_t* out_part);

/* ---- multi-GPU exchange — RCCL over xGMI on the context's compute stream -------------------------------
 * No reference analogue (arrow-go is single-process).  One process per GPU.  Rank 0 calls ah_comm_unique_id and the
 * host distributes the 128 bytes (file, socket, launcher); every rank then calls ah_comm_init on its own ah_ctx.
 * Collectives are enqueued behind the kernels already on the compute stream and return without waiting (ah_sync to
 * wait); buffers are device pointers, counts / offsets host arrays of `world` entries.  The path needs exactly these:
 *   C4  ah_comm_allreduce_sum(AH_INT64, partial, partial, 2) after ah_cmp_filter_sum_i64_dev — 16 bytes;
 *       float64: ah_comm_allgather of the 8-byte partials, added in rank order by the caller (bit-reproducible)
 *   C5  owner merge of group tuples: ah_comm_alltoallv (direct send / recv pairs — all xGMI links at once) of
 *       O(groups) bytes, then ah_comm_allgather of the owners' results
 * RCCL is bound with dlopen at first use (the copy already in the process, e.g. torch's, else the system's;
 * ARROWHIP_RCCL overrides); a machine without it gets AH_EHIP from these calls and loses nothing else. */
typedef struct ah_comm ah_comm;
int ah_comm_unique_id(void* id_host128);
int ah_comm_init(ah_ctx* ctx, int rank, int world, const void* unique_id_host128, ah_comm** out);
int ah_comm_destroy(ah_comm* comm);
int ah_comm_rank(ah_comm* comm);
int ah_comm_world(ah_comm* comm);
/* type: AH_INT32 / UINT32 / INT64 / UINT64 / FLOAT32 / FLOAT64; send may equal recv (in place) */
int ah_comm_allreduce_sum(ah_comm* comm, int type, const void* send, void* recv, int64_t count);
/* recv holds world × nbytes_per_rank bytes, rank r's block at r × nbytes_per_rank */
int ah_comm_allgather(ah_comm* comm, const void* send, void* recv, int64_t nbytes_per_rank);
/* block for rank r: send + send_offs_host[r], send_bytes_host[r] bytes; arrives at recv + recv_offs_host[r] of rank r;
 * recv_bytes_host[r] must be what rank r sends here (exchange the sizes first: an allgather of 8·world bytes) */
int ah_comm_alltoallv(ah_comm* comm, const void* send, const int64_t* send_bytes_host, const int64_t* send_offs_host, void* recv,
                      const int64_t* recv_bytes_host, const int64_t* recv_offs_host);
/* A communicator whose bytes are carried by the HOST's own transport (its launcher's sockets, MPI, a gloo group in the tests)
 * instead of RCCL: the two callbacks work on host memory, return 0 on success, and are called by every rank in the same order.
 * Device blocks are staged through pinned memory.  For hosts without RCCL between their processes — and for several ranks on
 * ONE GPU, which RCCL refuses.  All ah_comm_* entry points work on either flavour. */
typedef struct ah_transport {
  void* user;
  /* every rank contributes nbytes_per_rank bytes; recv_host gets world x nbytes_per_rank, rank order */
  int (*allgather)(void* user, const void* send_host, void* recv_host, int64_t nbytes_per_rank);
  /* block for rank r: send_host + send_offs[r], send_bytes[r] bytes -> recv_host + recv_offs[r] on rank r (the own block included) */
  int (*alltoallv)(void* user, const void* send_host, const int64_t* send_bytes, const int64_t* send_offs, void* recv_host,
                   const int64_t* recv_bytes, const int64_t* recv_offs);
} ah_transport;
int ah_comm_init_transport(ah_ctx* ctx, int rank, int world, const ah_transport* transport, ah_comm** out);
/* ---- configs C4 / C5 as single calls — what a host runs per record-batch shard, nothing in between -------------
 * C4: the fused Compare(op, scalar) -> Filter(DropNulls) -> Sum over THIS rank's shard (ah_cmp_filter_sum_*) and the one exchange
 * step of the path: Int64 — an all-reduce of the 16-byte {sum, count} (wrapping sums are exact in any order); Float64 — an
 * all-gather of the partials, added in RANK order on every rank (the same bytes on every rank and in every run of a given world
 * size; an all-reduce's order is the ring's).  Every rank receives the global result.  Synchronises. */
int ah_comm_cmp_filter_sum_i64(ah_comm* comm, int cmpop, const int64_t* x, const uint8_t* valid, int64_t off, int64_t n_local,
                               int64_t threshold, int64_t* out_sum_host, int64_t* out_count_host);
int ah_comm_cmp_filter_sum_f64(ah_comm* comm, int cmpop, const double* x, const uint8_t* valid, int64_t off, int64_t n_local,
                               double threshold, double* out_sum_host, int64_t* out_count_host);
/* C5: merge of the ranks' LOCAL aggregates (the outputs of ah_hash_sum_* over each rank's row shard; first_rows local, row_offset =
 * the shard's first global row) by key-hash owner: groups bucketed by (hashInt(key) >> 40) mod world on the device -> ragged
 * all-to-all of {key, sum, count, global first row} tuples (O(groups) bytes, never O(rows)) -> the owner re-aggregates (Float64:
 * the reproducible sums of ah_hash_sum_f64) -> ragged all-gather -> ordered by global first row: the groups, in the order, that
 * unique / dictionary_encode over the undivided column gives (kernels/vector_hash.go:359-385, 721-741).  Every rank receives all
 * groups.  Device buffers; out_* hold `capacity` groups; *out_ngroups_host = the global group count — AH_EINVALID with that
 * count set (and nothing written) when capacity is too small.  Synchronises.
 * The NULL group: null_group_local = what ah_hash_sum_* reported in *out_null_group_host for this rank's shard (−1: none).  A null
 * key has no hash owner — its group (key slot 0, like the local aggregate's) is merged on every rank from the ranks' null tuples
 * in rank order, takes its place in the first-seen order, and *out_null_group_host (nullable) = its position, −1 if no rank had
 * one.  A column holding both null keys and the key 0 therefore yields two groups, as over the undivided column. */
int ah_comm_merge_groups(ah_comm* comm, int is_f64, const uint64_t* keys, const void* sums, const int64_t* counts, const int64_t* first_rows,
                         int64_t ngroups_local, int32_t null_group_local, int64_t row_offset, int64_t capacity, uint64_t* out_keys,
                         void* out_sums, int64_t* out_counts, int64_t* out_first_rows, int64_t* out_ngroups_host,
                         int32_t* out_null_group_host);

/* ---- numeric cast (row §8(f)-2) ----------------------------------------------------------------
 * replaces castNumberToNumberUnsafe → castNumericUnsafe (kernels/cast_numeric.go:28-131; AVX2 leaf
 * cast_type_numeric_avx2(itype, otype, in, out, len), kernels/_lib/cast_numeric.cc:62) together with
 * the safe-cast checks the reference runs as separate passes: intsCanFit / intsInRange
 * (helpers.go:496-652), checkIntToFloatTrunc (numeric_cast.go:698-729), checkFloatTrunc (:613-660) —
 * behind compute's "cast" with CastOptions{ToType, AllowIntOverflow, AllowFloatTruncate}
 * (kernels/cast.go:27-35).  Every slot is converted (valid or not); only VALID slots can fail a check
 * (valid = NULL: all valid).  Failure → AH_EINVALID with the reference's text for the first offending
 * row: "integer value %d not in range: %d to %d" / "float value %f was truncated converting to %s".
 * Synchronises only when a check is active.  in_type == out_type is a device copy. */
int ah_cast_numeric(ah_ctx* ctx, int in_type, int out_type, const void* values, const uint8_t* valid, int64_t off, int64_t n,
                    int allow_int_overflow, int allow_float_truncate, void* out_values);
/* ---- decimal casts (row §8(f)-2) ------------------------------------------------------------------------
 * The decimal kernels behind compute's "cast": all arithmetic on the unscaled integer (16 bytes: Decimal128, 32 bytes: Decimal256,
 * little-endian two's complement).  `values` points at the first row; `off` is the bit offset of that row in `valid` (NULL: all
 * valid).  ScalarUnaryNotNull: a null slot is not looked at and its output is zero bytes; only VALID rows can fail, and the error is
 * that of the FIRST offending row.  One pass; synchronises only when a check is active.
 *
 * ah_cast_decimal_rescale replaces CastDecimalToDecimal (kernels/numeric_cast.go:377-429).  scale_delta = out_scale − in_scale,
 * −76 … 76.  allow_truncate == 0 (safeRescaleDecimal128Out / 256Out, :310-375): × 10^k, or ÷ 10^k where a non-zero remainder is
 * AH_EINVALID "rescale data loss"; then |v| < 10^out_precision, else AH_EINVALID "decimal value does not fit in precision" (also
 * when the product leaves the width); a 32 → 16 byte cast narrows after the check.  allow_truncate != 0 (unsafeUpscale* /
 * unsafeDownscale*, :264-308): × 10^k modulo 2^128 / 2^256, or ÷ 10^k truncated toward zero; no precision check; 32 → 16 keeps
 * the low 16 bytes. */
int ah_cast_decimal_rescale(ah_ctx* ctx, int in_width, int out_width, int scale_delta, int out_precision, int allow_truncate,
                            const void* values, const uint8_t* valid, int64_t off, int64_t n, void* out_values);
/* replaces CastIntegerToDecimal → integerToDecimal128 / 256 (kernels/numeric_cast.go:173-239): value · 10^scale, sign- or
 * zero-extended by in_type (AH_UINT8 … AH_INT64).  scale < 0 → AH_EINVALID "scale must be non-negative".  The precision check is
 * the caller's, from the types (precision ≥ MaxDecimalDigitsForInt(in_type) + scale); this entry refuses a scale with which that
 * bound exceeds the width's 38 / 76 digits, so the product never leaves the width.  Never synchronises. */
int ah_cast_int_to_decimal(ah_ctx* ctx, int in_type, int out_width, int scale, const void* values, const uint8_t* valid, int64_t off,
                           int64_t n, void* out_values);
/* replaces CastDecimal128ToInteger / CastDecimal256ToInteger → decimalToIntImpl (kernels/numeric_cast.go:79-171).
 * allow_truncate == 0: Rescale(in_scale, 0) — a non-zero remainder is AH_EINVALID "rescale data loss"; != 0:
 * ReduceScaleBy(in_scale, round = true), half away from zero.  A negative in_scale multiplies by 10^−in_scale.  allow_overflow == 0: a
 * value outside out_type's inclusive range is AH_EINVALID "integer value out of bounds".  The result is the low 64 bits narrowed to
 * out_type (AH_UINT8 … AH_INT64). */
int ah_cast_decimal_to_int(ah_ctx* ctx, int in_width, int in_scale, int out_type, int allow_truncate, int allow_overflow,
                           const void* values, const uint8_t* valid, int64_t off, int64_t n, void* out_values);
/* ---- string casts (row §8(f)-2) --------------------------------------------------------------------------
 * The kernels behind compute's "cast" between String / Binary / LargeString / LargeBinary / FixedSizeBinary columns and the
 * integer and boolean types.  A byte-string column is (offset_width 4 | 8, offsets, data): `offsets` is the offsets BUFFER and
 * `off` the array's offset into it and into `valid` (NULL: all valid).  A fixed-width column is `values` pointing at its first row
 * with `off` the bit offset of that row in `valid`; in_type AH_BOOL: `values` is the data bitmap, read at bit `off` as well.  A
 * null row is never looked at.
 *
 * ah_parse_int replaces getParseStringExec under ScalarUnaryNotNullBinaryArg (kernels/numeric_cast.go:742-781,
 * helpers.go:130-154): strconv.ParseInt(s, 0, bits) / ParseUint(s, 0, bits) of every valid row into out_type (AH_UINT8 … AH_INT64),
 * 0 for a null row.  The reference keeps the error of the LAST offending valid row: AH_EINVALID with that row (relative to `off`) in
 * *bad_row_host and 1 (strconv.ErrSyntax) or 2 (strconv.ErrRange) in *bad_kind_host, for the caller to quote the row's bytes.
 * Synchronises once (the offender word). */
int ah_parse_int(ah_ctx* ctx, int offset_width, const void* offsets, const uint8_t* data, const uint8_t* valid, int64_t off, int64_t n,
                 int out_type, void* out_values, int64_t* bad_row_host, int* bad_kind_host);
/* replaces the strconv.ParseBool kernels under ScalarUnaryNotNullBinaryArgBoolOut (kernels/boolean_cast.go:77-95): 1 t T TRUE true
 * True / 0 f F FALSE false False into the bitmap out_bits from bit 0 (ceil(n / 8) bytes, every one written; a null row gives 0).
 * Error as ah_parse_int (always a syntax error). */
int ah_parse_bool(ah_ctx* ctx, int offset_width, const void* offsets, const uint8_t* data, const uint8_t* valid, int64_t off, int64_t n,
                  uint8_t* out_bits, int64_t* bad_row_host);
/* replace the integer / boolean → string formatters of addNumericAndTemporalToStringCasts (kernels/string_casts.go:444-579):
 * strconv.FormatInt(v, 10) / FormatUint(v, 10) / "true" | "false" of every valid row, nothing for a null row.  Two calls with the
 * caller's allocation in between, like ah_take_binary_offsets / _data: _offsets writes out_offsets[0 … n] (starting at 0) and
 * returns the byte total to the host (one synchronisation; 4-byte offsets and a total above INT32_MAX: AH_EINVALID); _data, given
 * the same column and those offsets, writes the characters (never synchronises). */
int ah_format_int_offsets(ah_ctx* ctx, int in_type, const void* values, const uint8_t* valid, int64_t off, int64_t n, int offset_width,
                          void* out_offsets, int64_t* out_total_bytes_host);
int ah_format_int_data(ah_ctx* ctx, int in_type, const void* values, const uint8_t* valid, int64_t off, int64_t n, int offset_width,
                       const void* out_offsets, uint8_t* out_data);
/* replaces validateUTF8Sequence / validateUtf8 / validateUtf8Fsb (kernels/string_casts.go:39-87): utf8.Valid of every valid row,
 * rows independent of each other.  offset_width 0: fixed-size rows of byte_width bytes, `data` the values buffer, row `off` the
 * first.  The FIRST offending valid row: AH_EINVALID with the row (relative to `off`) in *bad_row_host.  Synchronises once. */
int ah_validate_utf8(ah_ctx* ctx, int offset_width, const void* offsets, const uint8_t* data, int byte_width, const uint8_t* valid,
                     int64_t off, int64_t n, int64_t* bad_row_host);
/* replaces the offsets loop of CastFsbToBinary (kernels/string_casts.go:154-193): out_offsets[i] = (off + i) · byte_width for
 * i = 0 … n, the offsets under which a FixedSizeBinary column's values buffer is a Binary column's data.  4-byte offsets that
 * cannot hold (off + n) · byte_width: AH_EINVALID.  Never synchronises. */
int ah_fixed_binary_offsets(ah_ctx* ctx, int offset_width, int byte_width, int64_t off, int64_t n, void* out_offsets);
/* ---- temporal unit change (the casts either side of the temporal kernels) ----------------------------
 * replaces ShiftTime[InT, OutT](ctx, op, factor, input, output) (kernels/cast_temporal.go:35-104), the leaf of the
 * timestamp / duration / time32↔time64 / date32↔date64 casts (cast_temporal.go:240-420) and of the implicit unit
 * casts DispatchBest inserts between temporal operands (arithmetic.go:130-131).  in_bits / out_bits: 32 or 64
 * (the storage integers).  op: AH_SHIFT_MULTIPLY out = OutT(v)·OutT(factor) (wrapping), AH_SHIFT_DIVIDE
 * out = OutT(v / InT(factor)) (truncating); factor == 1 only converts the width.  Every slot is converted.
 * check != 0 (CastOptions.AllowTimeOverflow / AllowTimeTruncate false): a VALID value (valid = NULL: all) outside
 * [MinInt64/factor, MaxInt64/factor] (multiply) or not a multiple of factor (divide) → AH_EINVALID, *bad_value =
 * that value of the FIRST such row ("would result in out of bounds timestamp: %d" / "would lose data: %d");
 * the type names of the reference's message are the host's to add.  Synchronises only when checking. */
#define AH_SHIFT_MULTIPLY 0
#define AH_SHIFT_DIVIDE 1
int ah_shift_time(ah_ctx* ctx, int in_bits, int out_bits, int op, int64_t factor, int check, const void* values, const uint8_t* valid,
                  int64_t off, int64_t n, void* out_values, int64_t* bad_value);
/* boolToNum (numeric_cast.go:555-569): out[i] = bit(off + i) ? 1 : 0.  (numeric → bool is
 * isNonZero, boolean_cast.go:30-36 = ah_comparison(AH_CMP_NE, AH_SHAPE_AS, type, values, &zero).) */
int ah_cast_bool_to_numeric(ah_ctx* ctx, int out_type, const uint8_t* bits, int64_t off, int64_t n, void* out_values);

/* ---- is_in (row §8(f)-2) -----------------------------------------------------------------------
 * replaces SetLookupState.Init + isInKernelExec (kernels/scalar_set_lookup.go:192-244, 374-413)
 * behind compute's "is_in" with SetOptions{ValueSet, NullBehavior} (compute/scalar_set_lookup.go:
 * 62-65, 175-200).  Keys are the raw bits of a 1/2/4/8-byte value.  Writes the result's data AND
 * validity bits [out_bit_offset, out_bit_offset + n) (NullComputedPrealloc) and preserves every other
 * bit.  No host synchronisation. */
#define AH_NULL_MATCH 0        /* NullMatchingBehavior, kernels/scalar_set_lookup.go:31-38 */
#define AH_NULL_SKIP 1
#define AH_NULL_EMIT_NULL 2
#define AH_NULL_INCONCLUSIVE 3
int ah_is_in(ah_ctx* ctx, int byte_width, const void* values, const uint8_t* valid, int64_t off, int64_t n,
             const void* set_values, const uint8_t* set_valid, int64_t set_off, int64_t set_n, int null_behavior,
             uint8_t* out_data, uint8_t* out_valid, int64_t out_bit_offset);
/* One piece of a value set for ah_is_in_binary / ah_is_in_fixed (a plain array is one piece; a chunked value set, one piece per
 * chunk: SetLookupOptions.ValueSet, kernels/scalar_set_lookup.go:40-45, filled per chunk by initSetLookup, compute/
 * scalar_set_lookup.go:118-131).  Row i of the piece is element off + i of `offsets` / `data` and bit off + i of `valid`
 * (nullable).  Base-binary pieces: offset_width 4 or 8, `offsets` the offsets buffer, `data` the value bytes.  Fixed-width
 * pieces: offset_width 0, `offsets` unused, `data` the slots (byte_width each).  The table of pieces is HOST memory. */
typedef struct ah_set_chunk {
  int offset_width;
  const void* offsets;
  const uint8_t* data;
  const uint8_t* valid;
  int64_t off, n;
} ah_set_chunk;
/* is_in of String / Binary / LargeString / LargeBinary rows (SetLookupState[[]byte].Init + visitBinary + isInKernelExec,
 * kernels/scalar_set_lookup.go:192-244, 270-300, 374-413, behind compute's "is_in", compute/scalar_set_lookup.go:207-214):
 * values compare bytewise, so "" is a value.  Row i of the input is offsets[off + i] … offsets[off + i + 1] (offset_width 4
 * or 8) of `data`, validity bit off + i.  Every piece of the value set is inserted into ONE table (pieces may have either
 * offset width: String ↔ LargeString and Binary ↔ LargeBinary compare as bytes).  Null behaviours and the output contract
 * as ah_is_in.  No host synchronisation. */
int ah_is_in_binary(ah_ctx* ctx, int offset_width, const void* offsets, const uint8_t* data, const uint8_t* valid, int64_t off, int64_t n,
                    int set_nchunks, const ah_set_chunk* set, int null_behavior, uint8_t* out_data, uint8_t* out_valid,
                    int64_t out_bit_offset);
/* is_in of fixed-width rows of byte_width bytes — FixedSizeBinary, Decimal128 (16), Decimal256 (32) and every numeric type
 * (visitBinary / visitNumeric, kernels/scalar_set_lookup.go:106-133, 270-300): raw bytes compare.  Widths 1, 2, 4 and 8 take
 * ah_is_in's kernels (the reference's FixedSizeBinary fast path, SetLookupState[uintN]); other widths the byte-string table of
 * ah_is_in_binary.  Row i of the input is data + (off + i)·byte_width, validity bit off + i; value-set pieces have
 * offset_width 0 and the same byte_width.  Null behaviours and output as ah_is_in.  No host synchronisation. */
int ah_is_in_fixed(ah_ctx* ctx, int byte_width, const uint8_t* data, const uint8_t* valid, int64_t off, int64_t n, int set_nchunks,
                   const ah_set_chunk* set, int null_behavior, uint8_t* out_data, uint8_t* out_valid, int64_t out_bit_offset);
/* is_in of a dictionary array from is_in of its dictionary (what ensureDictionaryDecoded + execIsIn compute, compute/
 * scalar_set_lookup.go:56-61, without decoding the column): lut_data / lut_valid (bits 0 … lut_n − 1) hold is_in of the
 * dictionary's entries, bit lut_n the result for a NULL value.  Row i (index_width 1, 2, 4 or 8, signed; element off + i of
 * `indices`, validity bit off + i) gets bit indices[off + i] of the table, a null index gets bit lut_n; an index outside
 * [0, lut_n) gives a null row.  Writes data and validity bits [out_bit_offset, out_bit_offset + n).  No host synchronisation. */
int ah_is_in_dict_gather(ah_ctx* ctx, int index_width, const void* indices, const uint8_t* valid, int64_t off, int64_t n,
                         const uint8_t* lut_data, const uint8_t* lut_valid, int64_t lut_n, uint8_t* out_data, uint8_t* out_valid,
                         int64_t out_bit_offset);

/* ---- sort_indices (row §8(f)-2) ----------------------------------------------------------------
 * replaces kernels.SortIndices for one key over one array (kernels/vector_sort.go:388-481 →
 * arraySortOneColumnRange, vector_sort_internal.go:252-273) behind compute's "sort_indices"
 * (compute/vector_sort.go:42-52): a STABLE permutation of [0, n) as uint64 row numbers; nulls at the
 * end (default) or the start, NaNs next to them, the rest ascending or descending with ties in
 * input order.  Stable LSD radix sort; synchronises (two small read-backs). */
int ah_sort_indices(ah_ctx* ctx, int type, const void* values, const uint8_t* valid, int64_t off, int64_t n,
                    int descending, int nulls_at_start, uint64_t* out_indices);
/* several sort keys over equal-length columns (record batch / table: radixRecordBatchSortRange,
 * kernels/vector_sort_internal.go, and multiColumnComparator, vector_sort.go:103-120): lexicographic
 * by key 0, then key 1, …, each with its own order and null placement; stable.  Arrays of nkeys entries. */
int ah_sort_indices_multi(ah_ctx* ctx, int nkeys, const int* types, const void* const* values, const uint8_t* const* valids,
                          const int64_t* offs, int64_t n, const int* descending, const int* nulls_at_start, uint64_t* out_indices);
/* one sort key of ah_sort_indices_keys; row i of the call is element off + i of every buffer and bit off + i of `valid`
 * (nullable).  type: a numeric id (values = the values), AH_BINARY / AH_LARGE_BINARY (values = the DATA buffer, offsets = the
 * 4- / 8-byte offsets buffer; values may be null when every value is empty), AH_FIXED_SIZE_BINARY (values = the slots,
 * byte_width = the width) or AH_DECIMAL128 / AH_DECIMAL256 (values = the slots, byte_width = 16 / 32). */
typedef struct ah_sort_key {
  int type;
  const void* values;
  const void* offsets;
  int byte_width;
  const uint8_t* valid;
  int64_t off;
  int descending;
  int nulls_at_start;
} ah_sort_key;
/* sort_indices over keys of any sortable kind (kernels.SortIndices, kernels/vector_sort.go:388-481, with the binary, fixed-size
 * binary and decimal comparators of vector_sort.go:195-245; record batches as ah_sort_indices_multi): lexicographic by key 0,
 * 1, …; stable.  Binary and fixed-size binary values order bytewise, unsigned, a proper prefix first ("ab" < "ab\0" < "abc");
 * decimals by signed value.  Nulls of every key go to its end or start in input order; no NaN category outside the floats.
 * Binary keys are sorted in rounds of 7 bytes: a round re-sorts only the rows still tied.  Data buffers of
 * the 64-bit-offset types may exceed 4 GiB.  Synchronises. */
int ah_sort_indices_keys(ah_ctx* ctx, int nkeys, const ah_sort_key* keys, int64_t n, uint64_t* out_indices);
/* select_k: exactly the first min(k, n) entries ah_sort_indices_keys returns for the same keys (kernels.SortIndices,
 * kernels/vector_sort.go:388-481, cut at k: ORDER BY … LIMIT k) without sorting the column — stable, ties in input order,
 * −0.0 ties +0.0, NaNs next to the nulls.  AH_SELECT_RADIX: a first key of an integer or float type; the threshold key by MSD
 * histogram levels over key 0, one collecting pass, a sort of the k survivors; AH_ENOTIMPL for any other
 * first key.  AH_SELECT_SORT: the sort with its final widening cut at k entries, for every key the sort takes.
 * AH_SELECT_AUTO chooses on the host from n, k and the key types.  The result does not depend on the route.  k < 0:
 * AH_EINVALID; k = 0 or n = 0 write nothing. */
#define AH_SELECT_AUTO 0
#define AH_SELECT_RADIX 1
#define AH_SELECT_SORT 2
int ah_select_k(ah_ctx* ctx, int nkeys, const ah_sort_key* keys, int64_t n, int64_t k, int route, uint64_t* out_indices);
/* route: AH_SELECT_AUTO 0 | AH_SELECT_RADIX 1 | AH_SELECT_SORT 2.  out_indices holds min(k, n) entries.  Synchronises. */

/* ---- window functions: ranks and running aggregates over the partitions of a sort order (NEW — no reference analogue: arrow-go
 * has no window operator; definition in DESIGN.md §3.7.3) ---------------------------------------------------------------------
 * The caller brings dense partition ids (ah_group_ids) and `order`, the n uint64 row numbers ah_sort_indices_keys wrote for the
 * keys (partition id ascending, then the ORDER BY keys): sorted position p holds row order[p].  order == NULL is the identity
 * (position p holds row p).  PRECONDITION: `order` is a permutation of [0, n); an entry outside [0, n) is never used as an
 * address (its position reads and writes nothing), any other violation gives unspecified values inside the outputs.  n <= 2^30
 * (AH_EINVALID above).  n == 0: nothing touched.  All three calls are enqueued on the compute stream and do not synchronise;
 * temporaries: O(n / 2048) words of the scratch arena.
 *
 * ah_window_flags: out_flags[p] (n bytes, one per SORTED position): bit 0 = a partition starts at p, bit 1 = a peer group starts
 * at p; position 0 starts both, and a partition start is a peer start.  p > 0 compares row order[p - 1] with row order[p]:
 * bit 0 iff part_ids differs (part_ids: n int32 indexed by ROW, or NULL = one partition); bit 1 iff bit 0, or the rows do not
 * tie on some key.  Rows tie on a key as the comparator of ah_sort_indices_keys ties them: both null; both NaN (any payload);
 * equal values with -0.0 = +0.0; binary and fixed-size binary values of equal length and equal bytes; decimals of equal value
 * (= equal bytes).  order_keys: 0 <= nkeys <= 8 entries of host memory laid out as for ah_sort_indices_keys (row i = element
 * off + i of every buffer); descending and nulls_at_start are not looked at.  nkeys == 0: every row is its own peer group. */
int ah_window_flags(ah_ctx* ctx, const int32_t* part_ids, int nkeys, const ah_sort_key* order_keys, const uint64_t* order, int64_t n,
                    uint8_t* out_flags);
/* ah_window_rank: out[order[p]] (n uint64, 1-based, every row written once) = AH_WINDOW_ROW_NUMBER: p - s + 1, s the last
 * partition start at or before p; AH_WINDOW_RANK: g - s + 1, g the last peer-group start at or before p (the row number of the
 * first row of p's peer group); AH_WINDOW_DENSE_RANK: the number of peer-group starts in [s, p].  `flags`: what ah_window_flags
 * wrote for the same order. */
#define AH_WINDOW_ROW_NUMBER 0
#define AH_WINDOW_RANK 1
#define AH_WINDOW_DENSE_RANK 2
int ah_window_rank(ah_ctx* ctx, int kind, const uint8_t* flags, const uint64_t* order, int64_t n, uint64_t* out);
/* ah_window_scan: the running aggregate of a value column over ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW of the row's
 * partition in the given order — a segmented inclusive scan over the sorted positions restarting where bit 0 of `flags` is set,
 * the column gathered through `order` and the result scattered back: out_values[order[p]], one store per row, EVERY row written.
 * `values` points at row 0 of the call (element-aligned), `valid` (nullable) is read at bit off + row; `type`: any of the ten
 * numeric ids.  A row whose value is null gets payload 0 and does not contribute; the output's validity is the input's, which
 * the caller copies (ah_copy_bitmap): no validity bit is written here.
 *   AH_WINDOW_SUM    out: 8 bytes per row — wrapping Int64 (signed types), wrapping UInt64 (unsigned types), Float64 (floats, added
 *                    in double in a tree that depends on n and the flags only: the same bytes on every run; no float atomics).
 *   AH_WINDOW_MIN / AH_WINDOW_MAX   out: the input type.  The rules of ah_group_min_max_typed on the prefix: NaNs are ignored
 *                    unless every valid value so far is a NaN, then the canonical quiet NaN; -0 < +0.
 *   AH_WINDOW_COUNT  out: int64, the valid values so far (valid == NULL: the row number); never null; `type` and `values` are
 *                    not looked at. */
#define AH_WINDOW_SUM 0
#define AH_WINDOW_MIN 1
#define AH_WINDOW_MAX 2
#define AH_WINDOW_COUNT 3
int ah_window_scan(ah_ctx* ctx, int op, int type, const void* values, const uint8_t* valid, int64_t off, const uint8_t* flags,
                   const uint64_t* order, int64_t n, void* out_values);

/* Boolean VALUES (booleanTakeImpl, kernels/vector_selection.go:990-1074): data and validity are bitmaps
 * indexed at voff + idx; a null output keeps data bit 0.  Output bitmaps start at bit 0.  Filter of a
 * boolean column = ah_filter_to_indices + this (the reference's own boolFilterWriter never advances its
 * output position, :433-436 — SURVEY.md quirk 8 — and is not replicated). */
int ah_take_boolean(ah_ctx* ctx, const uint8_t* data, const uint8_t* vvalid, int64_t voff, int64_t nvalues, int idx_byte_width,
                    int idx_signed, const void* idx, const uint8_t* ivalid, int64_t ioff, int64_t nidx, int bounds_check,
                    uint8_t* out_data, uint8_t* out_valid, int64_t* out_null_count_host, int64_t* bad_index_host);

/* ---- var-length Take / Filter (row §8(f)-4) ------------------------------------------------------
 * replaces VarBinaryImpl (kernels/vector_selection.go:1925-1992) under takeExec / filterExec
 * (:1460-1598, 1821-1923) for Binary / String (offset_width 4) and LargeBinary / LargeString (8).
 * `offsets`: the values' offsets buffer (element voff + i and voff + i + 1 delimit value i; vvalid
 * bit voff + i).  Two calls with the caller's allocation in between:
 *   _offsets: out_offsets[0..nidx] (offset_width each, starting at 0), out_valid (nullable), the null
 *             count, the number of data bytes, AH_EINDEX "<v> out of bounds" for the first offending
 *             valid index, AH_EINVALID "binary output offset overflow" (:1245) — synchronises;
 *   _data:    the bytes, into a buffer of that many bytes.
 * A null output (null value or null index) has zero length.  Filter of a binary column =
 * ah_filter_count → ah_filter_to_indices → these two (GetTakeIndices, as compute/selection.go:687 does
 * for record batches); uint32 indices, so < 2^32 rows. */
int ah_take_binary_offsets(ah_ctx* ctx, int offset_width, const void* offsets, const uint8_t* vvalid, int64_t voff, int64_t nvalues,
                           int idx_byte_width, int idx_signed, const void* idx, const uint8_t* ivalid, int64_t ioff, int64_t nidx,
                           int bounds_check, void* out_offsets, uint8_t* out_valid, int64_t* out_null_count_host,
                           int64_t* out_total_bytes_host, int64_t* bad_index_host);
int ah_take_binary_data(ah_ctx* ctx, int offset_width, const void* offsets, const uint8_t* data, int64_t voff, int idx_byte_width,
                        const void* idx, int64_t nidx, const void* out_offsets, uint8_t* out_data);

/* ---- conditionals: if_else and the directed null fills (NEW — no reference analogue: arrow-go has neither; the semantics are
 * Arrow C++'s) ----------------------------------------------------------------------------------------------------
 * if_else(cond, l, r): row i is null where cond[i] is null; otherwise it is l[i] (cond true) or r[i] with that side's validity.
 * The condition is a Boolean column: cond_data and cond_valid (nullable) are bitmaps read at bit cond_off + i.  coalesce(x, y) is
 * if_else with cond_data = x's validity bitmap and cond_valid = NULL.  Where Arrow leaves bytes unspecified: the payload under a
 * null slot of a fixed-width output is zero bytes, a null data bit is 0, a null var-length row has length 0.
 *
 * One side.  Fixed width: offset_width 0, row i is the byte_width bytes at data + (off + i) * byte_width.  Boolean
 * (ah_if_else_boolean): `data` is a bitmap read at bit off + i.  Var-length: offset_width 4 or 8, `offsets` the offsets buffer,
 * row i is data[offsets[off + i] ... offsets[off + i + 1]).  `valid` (nullable) is read at bit off + i.  broadcast != 0: a scalar
 * as a one-row device column, every row reads element `off`.  Buffers are DEVICE memory; the descriptor itself is host memory. */
typedef struct ah_cond_side {
  int offset_width;
  int byte_width;
  const void* offsets;
  const void* data;
  const uint8_t* valid;
  int64_t off;
  int broadcast;
} ah_cond_side;
/* Fixed-width sides of the same byte_width (1 ... 4096; 1 / 2 / 4 / 8 / 16 / 32 move as vectors when the buffers are aligned to
 * min(byte_width, 8), any other width or alignment row by row).  One streaming pass, no host synchronisation.  out_values: n
 * slots; out_valid: a bitmap that starts at bit 0 — exactly ceil(n / 8) bytes are written, the unused bits of the last one 0.
 * The three input offsets are independent.  out_valid may be NULL only when cond_valid, l->valid and r->valid all are. */
int ah_if_else(ah_ctx* ctx, const uint8_t* cond_data, const uint8_t* cond_valid, int64_t cond_off, const ah_cond_side* l,
               const ah_cond_side* r, int64_t n, void* out_values, uint8_t* out_valid);
/* Boolean sides: (c & l) | (~c & r) word by word on data and validity.  out_data and out_valid start at bit 0, ceil(n / 8) bytes
 * each.  No host synchronisation. */
int ah_if_else_boolean(ah_ctx* ctx, const uint8_t* cond_data, const uint8_t* cond_valid, int64_t cond_off, const ah_cond_side* l,
                       const ah_cond_side* r, int64_t n, uint8_t* out_data, uint8_t* out_valid);
/* Var-length sides (either may have 4- or 8-byte offsets), two calls with the caller's allocation in between, like
 * ah_take_binary_offsets / _data:
 *   _offsets: out_offsets[0 ... n] (out_offset_width bytes each, starting at 0), out_valid (as above), the number of data bytes;
 *             AH_EINVALID "binary output offset overflow" when they do not fit 4-byte offsets — synchronises;
 *   _data:    the bytes, into a buffer of that many bytes; out_offsets is what _offsets wrote.  No host synchronisation. */
int ah_if_else_binary_offsets(ah_ctx* ctx, const uint8_t* cond_data, const uint8_t* cond_valid, int64_t cond_off, const ah_cond_side* l,
                              const ah_cond_side* r, int64_t n, int out_offset_width, void* out_offsets, uint8_t* out_valid,
                              int64_t* out_total_bytes_host);
int ah_if_else_binary_data(ah_ctx* ctx, const uint8_t* cond_data, const uint8_t* cond_valid, int64_t cond_off, const ah_cond_side* l,
                           const ah_cond_side* r, int64_t n, int out_offset_width, const void* out_offsets, uint8_t* out_data);
/* fill_null_forward (direction 0) / fill_null_backward (direction 1): a null row takes the nearest valid row at or before / at
 * or after it and stays null when there is none.  `valid` (nullable) is read at bit off + i.  n <= 2^32 - 1 (AH_ENOTIMPL
 * above).  The walk is over the bitmap's 64-bit words: a count-leading / -trailing-zeros inside a word, a reduce-then-scan
 * running maximum across them (three launches, no workgroup waits for another).  Outputs start at bit 0 / row 0; a validity
 * output is needed whenever `valid` is given.  out_null_count_host nullable: when given, the call synchronises.
 *   _indices:  out_idx[i] (uint32) = the row number of row i's source, 0 where there is none, and out_idx_valid its bit: the
 *              (idx, ivalid) pair of the Take family, for the columns _directed does not take (Boolean, var-length, odd widths);
 *   _directed: the same walk with the gather fused in: out_values[i] = values[off + source] (payload 0 where there is none) for
 *              byte_width 1 / 2 / 4 / 8 / 16 / 32 (AH_ENOTIMPL otherwise); `values` is the buffer's element 0. */
int ah_fill_null_indices(ah_ctx* ctx, const uint8_t* valid, int64_t off, int64_t n, int direction, uint32_t* out_idx,
                         uint8_t* out_idx_valid, int64_t* out_null_count_host);
int ah_fill_null_directed(ah_ctx* ctx, int byte_width, const void* values, const uint8_t* valid, int64_t off, int64_t n, int direction,
                          void* out_values, uint8_t* out_valid, int64_t* out_null_count_host);

/* ---- fused scalar-expression evaluation (row §8(f)-1: the expression executor) ---------
 * What compute.Expression trees — NewCall / NewFieldRef / NewLiteral, arrow/compute/
 * expression.go:596-620 — evaluate to through executeScalarBatch (arrow/compute/exprs/
 * exec.go:542-700: one scalar kernel per call node, every intermediate materialised),
 * computed in ONE kernel generated for the tree and JIT-compiled with hiprtc.  The tree is a
 * postfix program; results are bit-identical to executing the calls one by one through the
 * entry points above (same wraparound / IEEE / checked-overflow / null-intersection rules;
 * operand types of a call must match — the caller inserts AH_X_CAST nodes where the reference's
 * DispatchBest would cast — else AH_ENOTIMPL). */
typedef struct { int32_t op; int32_t arg; } ah_expr_node;
typedef struct ah_expr ah_expr;
#define AH_X_FIELD 1        /* push input column `arg` */
#define AH_X_LITERAL 2      /* push literal `arg` (value given at execute time) */
#define AH_X_ADD 10         /* add_unchecked / subtract_unchecked / multiply_unchecked */
#define AH_X_SUB 11
#define AH_X_MUL 12
#define AH_X_ADD_CHECKED 13 /* add / subtract / multiply (checked on integers) */
#define AH_X_SUB_CHECKED 14
#define AH_X_MUL_CHECKED 15
#define AH_X_NEGATE 20      /* negate_unchecked, abs_unchecked, sign */
#define AH_X_ABS 21
#define AH_X_SIGN 22
#define AH_X_EQ 30          /* equal, not_equal, greater, greater_equal, less, less_equal */
#define AH_X_NE 31
#define AH_X_GT 32
#define AH_X_GE 33
#define AH_X_LT 34
#define AH_X_LE 35
#define AH_X_AND 40         /* and, or, xor, and_not, invert (plain, non-Kleene) */
#define AH_X_OR 41
#define AH_X_XOR 42
#define AH_X_AND_NOT 43
#define AH_X_INVERT 44
#define AH_X_CAST 50        /* value-preserving numeric conversion of the top of the stack to type `arg`: integer → wider integer
                             * (unsigned → signed only when wider), ≤ 32-bit integer → double, ≤ 16-bit integer → float, float →
                             * double — the implicit casts DispatchBest inserts (commonNumeric, compute/internal/kernels/
                             * helpers.go) that can never fail a safe-cast check; any other pair is AH_ENOTIMPL */
/* column / literal types are arrow.Type ids (1 = BOOL: bitmap column).  Compiled programs are
 * cached per context by (program, types); the returned handle is owned by the context. */
int ah_expr_compile(ah_ctx* ctx, const ah_expr_node* nodes, int n_nodes, const int* col_types, int n_cols,
                    const int* lit_types, int n_lits, ah_expr** out, int* out_type_host);
/* col_values[i]: element 0 of column i (offset applied) — for BOOL columns the bitmap base;
 * col_valid[i] (nullable) and BOOL data are addressed with bit offset col_offsets[i].
 * lit_values_host: n_lits × 8 bytes (little-endian payload), lit_valid_host: n_lits flags.
 * out_values: len elements (BOOL: ceil(len/8) bytes, 8-byte aligned); out_valid (nullable:
 * pass NULL when no input can be null) receives the AND of all referenced validities.
 * Returns AH_EOVERFLOW ("overflow") like ah_arithmetic_checked when a checked node overflows
 * in a valid slot (synchronises only if the program has checked integer nodes). */
int ah_expr_execute(ah_ctx* ctx, ah_expr* expr, const void* const* col_values, const uint8_t* const* col_valid,
                    const int64_t* col_offsets, const void* lit_values_host, const int* lit_valid_host, int64_t len,
                    void* out_values, uint8_t* out_valid);
const char* ah_expr_source(ah_expr* expr); /* generated HIP source, for inspection */
/* stateless: generate (and optionally hiprtc-compile for gfx950) without a GPU or a context;
 * src_buf/err_buf may be NULL.  Used by the CPU test-suite. */
int ah_expr_codegen(const ah_expr_node* nodes, int n_nodes, const int* col_types, int n_cols, const int* lit_types, int n_lits,
                    int do_compile, char* src_buf, size_t src_cap, char* err_buf, size_t err_cap, int* out_type_host);

#ifdef __cplusplus
}
#endif
#endif /* ARROWHIP_H */
