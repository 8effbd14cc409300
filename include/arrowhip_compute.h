/*
 * arrowhip_compute.h — C ABI of libarrowhip_compute.so: the ARRAY-LEVEL face of the MI355X execution layer.
 *
 * libarrowhip.so (arrowhip.h) replaces the reference's leaves (pointers + lengths).  This library sits one level up:
 * it carries the part of arrow-go's arrow/compute that a Go host would otherwise keep — function registry, scalar /
 * vector executors (null propagation, preallocation, chunked arguments, DispatchBest casts), the Arrow IPC stream
 * reader — next to the device, so that a chain of calls never leaves HBM.  Whole arrays enter and leave through the
 * Arrow C Data Interface and the Arrow C Device Data Interface, i.e. the structs arrow-go's own arrow/cdata package
 * speaks (arrow/cdata/abi.h:50-128, cdata.go:69-72, interface.go:73-153).
 *
 *   ahc_call(session, "add", "", 2, args, &out)   ≙   compute.CallFunction(ctx, "add", nil, a, b)   compute/exec.go:191
 *
 * A Go binding (INTEGRATION.md §"array-level route") is `#include "arrowhip_compute.h"` + cdata.ExportArrowArray /
 * cdata.ImportCArrayWithType on either side of ahc_import / ahc_export.
 *
 * Conventions
 *   - every int-returning function returns 0 or a status class (AHC_*); the message is ahc_last_error(session) until
 *     the next call on that session.  Functions returning a count return -1 for "not that kind of datum".
 *   - an ahc_datum is an opaque, reference-counted handle (compute.Datum, compute/datum.go:52-60: scalar, array,
 *     chunked array, record batch) whose buffers live in HBM; release every handle you were given with
 *     ahc_datum_release.  A datum may outlive its session handle: device memory is returned when the last datum goes.
 *   - one call at a time per session (it owns one ah_ctx: one compute stream, one copy stream); sessions are
 *     independent and may be used from different threads.
 *   - nothing here retains a host pointer after the call returns.
 */
#ifndef ARROWHIP_COMPUTE_C_H
#define ARROWHIP_COMPUTE_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Arrow C Data Interface / C Device Data Interface (verbatim ABI: arrow/cdata/abi.h:50-79, 95-128) ------------- */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
#define ARROW_FLAG_DICTIONARY_ORDERED 1
#define ARROW_FLAG_NULLABLE 2
#define ARROW_FLAG_MAP_KEYS_SORTED 4
struct ArrowSchema {
  const char* format;
  const char* name;
  const char* metadata;
  int64_t flags;
  int64_t n_children;
  struct ArrowSchema** children;
  struct ArrowSchema* dictionary;
  void (*release)(struct ArrowSchema*);
  void* private_data;
};
struct ArrowArray {
  int64_t length;
  int64_t null_count;
  int64_t offset;
  int64_t n_buffers;
  int64_t n_children;
  const void** buffers;
  struct ArrowArray** children;
  struct ArrowArray* dictionary;
  void (*release)(struct ArrowArray*);
  void* private_data;
};
#endif /* ARROW_C_DATA_INTERFACE */

#ifndef ARROW_C_DEVICE_DATA_INTERFACE
#define ARROW_C_DEVICE_DATA_INTERFACE
typedef int32_t ArrowDeviceType;
#define ARROW_DEVICE_CPU 1
#define ARROW_DEVICE_ROCM 10
#define ARROW_DEVICE_ROCM_HOST 11
struct ArrowDeviceArray {
  struct ArrowArray array;
  int64_t device_id;
  ArrowDeviceType device_type;
  void* sync_event; /* ARROW_DEVICE_ROCM: hipEvent_t* or NULL */
  int64_t reserved[3];
};
#endif /* ARROW_C_DEVICE_DATA_INTERFACE */

/* ---- status classes: the sentinel errors of arrow/errors.go the Go side wraps with fmt.Errorf("%w: …") ------------ */
#define AHC_OK 0
#define AHC_EINVALID 1  /* arrow.ErrInvalid (also "overflow") */
#define AHC_EINDEX 2    /* arrow.ErrIndex */
#define AHC_ENOTIMPL 3  /* arrow.ErrNotImplemented */
#define AHC_ETYPE 4     /* arrow.ErrType — no kernel matching input types */
#define AHC_EKEY 5      /* arrow.ErrKey — unknown function / already registered (compute/registry.go:106-135) */
#define AHC_EHIP 6      /* HIP runtime failure; there is no CPU fallback */

/* datum kinds (ahc_datum_info) — compute.DatumKind, compute/datum.go:35-49 */
#define AHC_KIND_NONE 0
#define AHC_KIND_SCALAR 1
#define AHC_KIND_ARRAY 2
#define AHC_KIND_CHUNKED 3
#define AHC_KIND_RECORD 4

typedef struct ahc_session ahc_session;       /* ah_ctx + compute.ExecCtx with its own child registry (compute/executor.go:46-112) */
typedef struct ahc_datum ahc_datum;           /* compute.Datum */
typedef struct ahc_ipc_writer ahc_ipc_writer; /* ipc.Writer (arrow/ipc/writer.go:85-110) */
typedef struct ahc_ipc_reader ahc_ipc_reader; /* ipc.Reader (arrow/ipc/reader.go:45-70) */

/* ---- session / registry ------------------------------------------------------------------------------------------ */
int ahc_session_create(int device_id, ahc_session** out);
void ahc_session_destroy(ahc_session* s);
const char* ahc_last_error(ahc_session* s); /* never NULL; owned by the session */
/* compute.GetFunctionRegistry(): NumFunctions / GetFunction(name) != nil / len(fn.Kernels()) (registry.go:30-40) */
int ahc_num_functions(void);
int ahc_has_function(const char* name);
int ahc_function_num_kernels(const char* name);
/* fn.DispatchBest(types...) of a scalar function (functions.go:199-218; arithmeticFunction / compareFunction.DispatchBest:
 * arithmetic.go:112-142, scalar_compare.go:37-63) or DispatchExact of a vector function, without executing: out_type_ids receives
 * the argument types of the chosen kernel (type ids as in ahc_datum_type_id), i.e. the implicit casts the executor would insert.
 * Needs no session and no GPU.  Error text into err. */
int ahc_dispatch_best(const char* function, int nargs, const int* type_ids, int* out_type_ids, char* err, int64_t cap);
/* the type id of what the kernel chosen as above returns (0 where the call's options decide it); no session, no GPU */
int ahc_output_type(const char* function, int nargs, const int* type_ids, int* out_type_id, char* err, int64_t cap);
/* what `function` answers to an options string ("key=value;…") before anything runs: the string predicates (match_substring,
 * starts_with, ends_with, find_substring, match_like) check pattern_hex / ignore_case here, the string transforms start / stop / step (the slices) and
 * characters_hex (the trims that take characters), every other function accepts.  Returns
 * the status code (0 = fine), the text into err; no session, no GPU */
int ahc_validate_options(const char* function, const char* options, char* err, int64_t cap);
/* a SQL LIKE pattern compiled into the segment program ah_string_like takes (include/arrowhip.h; `%`, `_`, `\` as in Arrow C++'s
 * match_like) → the program's length in bytes, -1 when it does not fit `cap`.  A plain host function */
int64_t ahc_like_compile(const uint8_t* pattern, int64_t pattern_len, uint8_t* out, int64_t cap);
/* AddAlias / AddFunction(allowOverwrite) on the session's child registry (registry.go:69-73, 97-135) */
int ahc_registry_add_alias(ahc_session* s, const char* alias, const char* existing, int allow_overwrite);

/* ---- datums ------------------------------------------------------------------------------------------------------- */
/* cdata.ImportCArrayWithType on a HOST array: buffers are uploaded (pinned staging → hipMemcpyAsync on the copy
 * stream); the producer's structs are released before returning, success or not.  Formats: the ten numeric types,
 * bool, u / z / U / Z (string / binary), tdD tdm tt* ts* tD* (temporal: stored as integers + label), and
 * dictionary-encoded arrays of those. */
int ahc_import(ahc_session* s, struct ArrowArray* arr, struct ArrowSchema* schema, ahc_datum** out);
/* cdata.ExportArrowArray: device → host copy; the caller owns (and must release) arr and schema */
int ahc_export(ahc_session* s, ahc_datum* d, struct ArrowArray* arr, struct ArrowSchema* schema);
/* HOST-RESIDENT arguments — chunked, overlapped execution (arrow_go_amd/host/hoststream.cc).  The reference's executor cuts a call
 * into spans of at most ExecCtx.ChunkSize rows (arrow/compute/executor.go:47-50, :499 iterateExecSpans); for a column that lives in
 * host memory that span loop is what hides the PCIe link.  ahc_import_host is ahc_import WITHOUT the upload for flat fixed-width
 * columns of at least "host_threshold_bytes" (64 MiB) value bytes: the producer's buffers stay where they are (pin them for the copies
 * to overlap) and are released with the datum.  ahc_call then streams such arguments span by span — upload k + 1, kernel k, download
 * k − 1 on three streams — for add / sub / subtract / multiply [+ _unchecked], equal … less_equal (array ∘ array, array ∘ scalar,
 * scalar ∘ array of one numeric type; a null scalar is handled as the whole-array kernels handle it: only checked integer add / sub
 * leave the payload untouched), filter / array_filter, cast (numeric → numeric, safe or not) and cumulative_sum[_checked] of integer
 * columns with nulls skipped or none (the running sum is carried from span to span); ahc_math_sum sums them chunk by chunk with one
 * final reduction.  The bytes of a streamed result — payload under nulls, validity, its last byte's tail bits — are those of the
 * whole-array call.  Results of streamed calls are host-resident too (pinned memory of the session's; ahc_export hands the buffers out
 * without a copy, ahc_datum_buffers returns HOST pointers for them).  Every other function uploads a host-resident argument whole the
 * first time it meets it; the copy stays with the datum, which counts as device-resident from then on (ahc_datum_on_host → 0,
 * ahc_datum_buffers → the device pointers, later calls use the copy instead of streaming).  A column larger than the free HBM can be
 * added, compared, filtered, cast and summed this way: only three spans of it are on the device at any time.
 * ahc_session_set_option: "select_k_route" (select_k: 0 the library chooses, 1 the radix route, 2 the sort cut at k entries),
 * "chunk_bytes" (bytes of the widest column per span: ExecCtx.ChunkSize's role; 0 = 32 MiB),
 * "host_threshold_bytes". */
int ahc_import_host(ahc_session* s, struct ArrowArray* arr, struct ArrowSchema* schema, ahc_datum** out);
int ahc_datum_on_host(ahc_datum* d);
int ahc_session_set_option(ahc_session* s, const char* name, int64_t value);
/* Arrow C Device Data Interface.  ARROW_DEVICE_ROCM on the session's device: ZERO COPY both ways — import wraps the
 * producer's buffers (its release callback runs when the last datum referencing them is gone; the compute stream
 * waits for sync_event), export hands the datum's HBM buffers out (stream synchronised, sync_event = NULL; the export
 * keeps them alive until the consumer calls release).  ARROW_DEVICE_CPU / ROCM_HOST imports take the upload path.
 * Layouts: fixed-width (2 buffers) and string / binary (3 buffers: validity, offsets, data). */
int ahc_import_device(ahc_session* s, struct ArrowDeviceArray* darr, struct ArrowSchema* schema, ahc_datum** out);
int ahc_export_device(ahc_session* s, ahc_datum* d, struct ArrowDeviceArray* out, struct ArrowSchema* schema);
/* scalar.Scalar of arrow.Type `type_id` (ids as in arrowhip.h; 1 = BOOL); value8: little-endian payload, 8 bytes */
int ahc_scalar(ahc_session* s, int type_id, int valid, const void* value8, ahc_datum** out);
/* a String / Binary / LargeString / LargeBinary / FixedSizeBinary / Decimal scalar: `format` its Arrow C Data format ("u", "z",
 * "U", "Z", "w:16", "d:10,2", "d:40,5,256"), data / len the value's bytes (a decimal: little-endian two's complement of the
 * unscaled value, 16 or 32 bytes; a FixedSizeBinary: exactly its width).  Copied; ignored when valid = 0. */
int ahc_scalar_bytes(ahc_session* s, const char* format, int valid, const void* data, int64_t len, ahc_datum** out);
/* temporal label of a datum as its C Data format ("tsu:UTC", "tdD", …; "" = plain); valid until the next call on
 * this thread.  ahc_scalar_set_logical labels a scalar made by ahc_scalar (AHC_ETYPE if the storage width differs). */
const char* ahc_datum_logical(ahc_datum* d);
int ahc_scalar_set_logical(ahc_session* s, ahc_datum* d, const char* format);
/* kind, arrow.Type id, Len(), null count (arrays; -1 = unknown), and for scalars validity + payload */
int ahc_datum_info(ahc_datum* d, int* kind, int* type_id, int64_t* length, int64_t* null_count, int* scalar_valid,
                   void* scalar_value8);
/* the device pointers behind an array datum (validity may be NULL; for binary types `data` is the offsets buffer) */
int ahc_datum_buffers(ahc_datum* d, void** validity, void** data);
void ahc_datum_release(ahc_datum* d);
/* compute.ChunkedDatum from array datums of one type (datum.go:186-230); the arrays stay the caller's */
int ahc_chunked_from_arrays(ahc_session* s, int type_id, int n, ahc_datum** arrays, ahc_datum** out);
int ahc_datum_num_chunks(ahc_datum* d);
int ahc_datum_chunk(ahc_session* s, ahc_datum* d, int i, ahc_datum** out);
/* compute.RecordDatum from equal-length array datums (datum.go:232-262) */
int ahc_record_from_arrays(ahc_session* s, int n, const char* const* names, ahc_datum** arrays, ahc_datum** out);
int ahc_record_num_columns(ahc_datum* d);
int ahc_record_column(ahc_session* s, ahc_datum* d, int i, const char** name, ahc_datum** out);

/* ---- calls -------------------------------------------------------------------------------------------------------- */
/* compute.CallFunction(ctx, name, opts, args...) (compute/exec.go:191-199).  `options` is "key=value;key=value" (NULL
 * or "" = the function's defaults) for the option structs of the registered functions:
 *   FilterOptions  null_selection_behavior=drop|emit_null; output_sizing=exact|worst_case (worst_case: the output is allocated
 *                  for the input's length and the kernel runs in ONE call — ah_filter_primitive_once — instead of count → allocate → fill)
 *   TakeOptions    bounds_check=0|1
 *   CastOptions    to_type=<type name>, string | large_string | binary | large_binary, or a parametric type by its C Data format
 *                  (d:22,2 = Decimal128, d:22,2,256 = Decimal256, w:16 = FixedSizeBinary of 16 bytes);
 *                  to_logical=<C Data format>; safe=0; allow_int_overflow= allow_float_truncate= allow_decimal_truncate=
 *                  allow_invalid_utf8= allow_time_truncate= allow_time_overflow=0|1
 *   SetOptions     value_set=@<hex address of an array ahc_datum>; null_matching_behavior=match|skip|emit_null|inconclusive
 *   SortOptions    sort_keys=<col>:<asc|desc>:<at_end|at_start>,…    ArraySortOptions  order= null_placement=
 *   CumulativeSumOptions  start=<number>; skip_nulls=0|1           RoundOptions  ndigits= round_mode= multiple=
 *   DictionaryEncodeOptions  null_encoding_behavior=mask|encode
 * Errors carry the reference's texts ("overflow", "%d out of bounds", "no kernel matching input types (…)", …). */
int ahc_call(ahc_session* s, const char* name, const char* options, int nargs, ahc_datum** args, ahc_datum** out);
/* math.Float64.Sum / Int64.Sum / Uint64.Sum (arrow/math/float64.go:34-39 …): the pointer matching the array's type
 * receives the result, validity ignored as in the reference */
int ahc_math_sum(ahc_session* s, ahc_datum* d, double* f64, int64_t* i64, uint64_t* u64);
/* exprs.ExecuteScalarExpression over a batch of columns (compute/exprs/exec.go:542-700).  text: call := name '(' arg
 * {',' arg} ')'; arg := call | '$'N (column N) | '#'N (literal N, a scalar datum).  fuse != 0: one generated kernel for
 * the whole tree where the generator covers it (*fused_out says whether), else call by call — same bytes either way. */
int ahc_expr_eval(ahc_session* s, const char* text, int ncols, ahc_datum** cols, int nlits, ahc_datum** lits, int fuse,
                  ahc_datum** out, int* fused_out);
/* The same executor fed with the reference's own tree shape instead of text: compute.Expression is Literal{datum} |
 * Parameter{field reference} | Call{funcName, args, options} (arrow/compute/expression.go:52-78, 278-290, NewLiteral :596,
 * NewFieldRef / NewRef :610, NewCall :617).  nodes[] holds the tree in post-order — a call's arguments come before it, the root is
 * the LAST node; a field reference is a column position, or index = -1 and a name resolved against col_names (FieldRef.FindOne:
 * "no match for field reference"); a literal is a position in lits[] (scalar datums); a call carries the options text of
 * ahc_call.  Same fusion rule and same bytes as ahc_expr_eval. */
#define AHC_EXPR_LITERAL 0
#define AHC_EXPR_FIELD_REF 1
#define AHC_EXPR_CALL 2
typedef struct ahc_expr_node {
  int32_t kind;
  int32_t index;          /* LITERAL: position in lits[]; FIELD_REF: column position or -1 (by name) */
  const char* name;       /* CALL: function name; FIELD_REF by name */
  const char* options;    /* CALL: options text (nullable) */
  int32_t nargs;          /* CALL */
  const int32_t* args;    /* CALL: positions in nodes[] of the arguments, each smaller than this node's */
} ahc_expr_node;
int ahc_expr_eval_tree(ahc_session* s, const ahc_expr_node* nodes, int n_nodes, int ncols, ahc_datum** cols, const char* const* col_names,
                       int nlits, ahc_datum** lits, int fuse, ahc_datum** out, int* fused_out);
/* exprs.ExecuteScalarSubstrait (arrow/compute/exprs/exec.go:465-488): `bytes` is a serialized substrait.ExtendedExpression with ONE
 * referred expression — scalar functions of the default extension set (add / subtract / multiply / divide / power / sqrt / abs with
 * their `overflow` option, equal / not_equal / lt / lte / gt / gte / is_null / is_not_null / is_nan, and / or / not), root field
 * references, primitive literals (unsigned ones as arrow-go's type variations or Arrow C++'s user-defined types), casts.  cols: the
 * input's columns in the order of the base schema, or — with col_names — matched by name, missing fields being null scalars
 * (makeExecBatch, exec.go:384-438); a column whose type differs from the schema's is arrow.ErrInvalid "referenced field … was …,
 * but should have been …"; what the reference's executor refuses is refused with its error class (ErrNotImplemented: measures,
 * several referred expressions, if-then, nested references, unknown functions, SATURATE, RETURN_NULL casts; ErrInvalid: no
 * expression, unspecified cast behaviour).  All-scalar input gives a scalar datum. */
int ahc_expr_eval_substrait(ahc_session* s, const uint8_t* bytes, int64_t len, int ncols, ahc_datum** cols, const char* const* col_names,
                            int fuse, ahc_datum** out, int* fused_out);

/* The same reader without a device: parses `bytes` and renders what it understood into out (NUL-terminated, truncated to cap) as
 * "name:type,…|output_name=expression|…" — literals as type(hex payload) or type(null), field references as $index, casts as cast(x -> type unsafe), an
 * expression the executor would refuse as "!" + its error text.  A malformed message returns the status code with the error text in out.
 * Needs no session and no GPU: the CPU tests of the wire-format reader (truncated and random bytes included) go through it. */
int ahc_substrait_inspect(const uint8_t* bytes, int64_t len, char* out, int64_t cap);

/* ---- Arrow IPC → HBM (ipc.NewReader / Reader.Next, arrow/ipc/reader.go:97-300) ------------------------------------ */
/* stream or file format, uncompressed bodies; each RecordBatch body goes to the device in one copy and the columns are
 * slices of it.  `bytes` must stay valid until ahc_ipc_close. */
int ahc_ipc_open(ahc_session* s, const uint8_t* bytes, int64_t len, ahc_ipc_reader** out);
void ahc_ipc_close(ahc_ipc_reader* r);
int ahc_ipc_num_fields(ahc_ipc_reader* r);
int ahc_ipc_field(ahc_ipc_reader* r, int i, const char** name, int* type_id, int* nullable);
/* next record batch: `columns` receives ahc_ipc_num_fields() array datums; *rows = -1 at end of stream */
int ahc_ipc_next(ahc_ipc_reader* r, ahc_datum** columns, int64_t* rows);
int64_t ahc_ipc_bytes_uploaded(ahc_ipc_reader* r);
/* A body compressed with LZ4_FRAME whose frames are made of independent 64 KiB blocks without checksums (what arrow-go's writer
 * produces) is uploaded compressed and inflated in HBM; every other compressed buffer (ZSTD, linked blocks — Arrow C++ / pyarrow —,
 * checksums, other block sizes), and any frame the device decoder reports a status for, is inflated on the host as before.
 * ahc_session_set_option, read when a reader is opened: "ipc_device_lz4" (1; 0 = always the host), "ipc_device_lz4_min_bytes"
 * (bodies of fewer compressed bytes stay on the host).
 * One outcome depends on the path: liblz4 up to 1.9 inflates a match offset of 0, which the LZ4 block format forbids, to zero bytes.
 * A frame with such a match is an error ("corrupt LZ4 frame") where the device path examined it, and reads as those zeros on the
 * host path (option 0, a body below the minimum, a frame that does not qualify).  Every valid stream reads the same on both.
 * out: {body bytes uploaded, compressed buffers inflated on the device, on the host, on the host after a device status} so far */
void ahc_ipc_stats(ahc_ipc_reader* r, int64_t out[4]);
/* ---- HBM → Arrow IPC (ipc.NewWriter / Writer.Write / Close, arrow/ipc/writer.go:85-260) ------------------------------ */
/* A stream of record batches whose columns live in HBM.  options: "compression=lz4" (the default for NULL / "") or
 * "compression=none".  With lz4 every buffer of a body is compressed IN HBM — an LZ4 frame of independent 64 KiB blocks without
 * checksums, the kind ahc_ipc_open inflates in HBM — or written raw behind a -1 length where the frame would not be smaller, and only
 * the compressed body crosses the link: per batch one compress launch, one launch that assembles the messages, one download.
 * ahc_ipc_write_batch: array datums only, all of one length; types: what ahc_ipc_open reads (ErrNotImplemented names the column
 * otherwise).  The first batch fixes the schema and writes the Schema message; a later batch that differs in a name, type, temporal
 * type or dictionary index type is ErrInvalid naming the column, as is a chunked or scalar datum (write chunk by chunk).  A
 * dictionary-encoded column gets its DictionaryBatch before the first record batch, and a replacement before a batch whose
 * dictionary is not the identical device buffers.  A sliced column is written as the offset-0 array of its rows.  Every byte of the
 * stream is defined: the same batches give the same bytes.  After an error the writer (and the session) stay usable.
 * ahc_ipc_writer_finish writes the end-of-stream marker; *bytes belongs to the writer and is valid until ahc_ipc_writer_close.
 * ahc_ipc_writer_stats: {plain bytes of all buffers, body bytes written, buffers written as frames, buffers written raw} so far. */
int ahc_ipc_writer_open(ahc_session* s, const char* options, ahc_ipc_writer** out);
int ahc_ipc_write_batch(ahc_ipc_writer* w, int ncols, const char* const* names, ahc_datum** columns);
int ahc_ipc_writer_finish(ahc_ipc_writer* w, const uint8_t** bytes, int64_t* len);
void ahc_ipc_writer_stats(ahc_ipc_writer* w, int64_t out[4]);
void ahc_ipc_writer_close(ahc_ipc_writer* w);

/* walks a stream WITHOUT a device: "hex(name):type_id:nullable:hex(logical),…|rows,rows,…" into out (NUL-terminated),
 * or the error text with the status returned */
int ahc_ipc_inspect(const uint8_t* bytes, int64_t len, char* out, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* ARROWHIP_COMPUTE_C_H */
