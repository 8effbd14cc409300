//go:build hip

package arrowhip

/*
#include <stdlib.h>
#include "arrowhip.h"
*/
import "C"

import (
	"fmt"
	"unsafe"

	"github.com/apache/arrow-go/v18/arrow"
)

// EXPERIMENTAL — never compiled (no Go toolchain in the build image; tests/test_go_shim_static.py checks the declarations and
// every C call against include/arrowhip.h).  The rest of the header's entry points, one thin method each: all pointers are
// DEVICE memory unless the name says Host.

// ---- context plumbing ------------------------------------------------------------------------------------------------------

func Version() string { return C.GoString(C.ah_version()) }

func DeviceCount() (int, error) {
	var n C.int
	if st := C.ah_device_count(&n); st != C.AH_OK {
		return 0, fmt.Errorf("arrowhip: ah_device_count failed (status %d)", int(st))
	}
	return int(n), nil
}

// NewContextOnStream shares an existing hipStream_t (another library's compute stream) instead of creating one: calls of
// both are ordered by the stream.
func NewContextOnStream(device int, hipStream unsafe.Pointer) (*Context, error) {
	var c *C.ah_ctx
	if st := C.ah_ctx_create_on_stream(C.int(device), hipStream, &c); st != C.AH_OK {
		return nil, fmt.Errorf("arrowhip: ah_ctx_create_on_stream(%d) failed (status %d)", device, int(st))
	}
	return &Context{c: c}, nil
}

func (x *Context) DeviceID() int { return int(C.ah_device_id(x.c)) }

// SetOption: the measurement switches of DESIGN.md §8 ("take_binned", "groupby_partition", …).
func (x *Context) SetOption(name string, value int64) error {
	cs := C.CString(name)
	defer C.free(unsafe.Pointer(cs))
	return x.err(C.ah_ctx_set_option(x.c, cs, C.int64_t(value)))
}

// WaitEvent makes the compute stream wait for a hipEvent_t recorded by another library.
func (x *Context) WaitEvent(hipEvent unsafe.Pointer) error { return x.err(C.ah_wait_event(x.c, hipEvent)) }

func (x *Context) Memset(dst unsafe.Pointer, byteValue int, nbytes int) error {
	return x.err(C.ah_memset_async(x.c, dst, C.int(byteValue), C.size_t(nbytes)))
}

func (x *Context) TimerStart() error { return x.err(C.ah_timer_start(x.c)) }

func (x *Context) TimerStop() (ms float32, err error) {
	var v C.float
	err = x.err(C.ah_timer_stop(x.c, &v))
	return float32(v), err
}

func (x *Context) EventRecord(slot int) error { return x.err(C.ah_event_record(x.c, C.int(slot))) }

func (x *Context) EventElapsedMs(slotA, slotB int) (ms float32, err error) {
	var v C.float
	err = x.err(C.ah_event_elapsed_ms(x.c, C.int(slotA), C.int(slotB), &v))
	return float32(v), err
}

// ---- element-wise ----------------------------------------------------------------------------------------------------------

// ArithmeticChecked is the kernel behind the DEFAULT compute.Add / Subtract / Multiply ("add", "subtract", "multiply" are
// OpAddChecked …: compute/arithmetic.go:635-636, kernels/base_arithmetic.go:249-286): op = opAdd / opSub / opMul, shape
// = shapeAA / AS / SA; for AS / SA the scalar operand is HOST memory and scalarValid says whether it is non-null.  An
// overflow in a valid slot comes back as arrow.ErrInvalid "overflow" (AH_EOVERFLOW), like the reference's errOverflow.
func (x *Context) ArithmeticChecked(typ arrow.Type, op int8, shape int, l, lvalid unsafe.Pointer, loff int64, r, rvalid unsafe.Pointer, roff int64,
	scalarValid bool, out unsafe.Pointer, n int64) error {
	return x.err(C.ah_arithmetic_checked(x.c, C.int(typ), C.int8_t(op), C.int(shape), l, (*C.uint8_t)(lvalid), C.int64_t(loff),
		r, (*C.uint8_t)(rvalid), C.int64_t(roff), boolInt(scalarValid), out, C.int64_t(n)))
}

// ArithmeticUnary: abs_unchecked / negate_unchecked / sign over the _arithmetic_unary_*_avx2 leaves
// (kernels/base_arithmetic_avx2_amd64.go:55-77): op = AH_OP_ABS / AH_OP_NEGATE / AH_OP_SIGN.
func (x *Context) ArithmeticUnary(typ arrow.Type, op int8, in, out unsafe.Pointer, n int64) error {
	return x.err(C.ah_arithmetic_unary(x.c, C.int(typ), C.int8_t(op), in, out, C.int64_t(n)))
}

// Round mirrors round / round_to_multiple (kernels/rounding.go:38-178): mode = compute.RoundMode; multipleHost: one element of
// the column's type in HOST memory for round_to_multiple, nil for round; pow10 = 10^|ndigits| as the reference computes it.
func (x *Context) Round(typ arrow.Type, values, valid unsafe.Pointer, off, n, ndigits int64, mode int, multipleHost unsafe.Pointer, pow10 float64, out unsafe.Pointer) error {
	return x.err(C.ah_round(x.c, C.int(typ), values, (*C.uint8_t)(valid), C.int64_t(off), C.int64_t(n), C.int64_t(ndigits), C.int(mode), multipleHost, C.double(pow10), out))
}

// MinMax mirrors the _int*_max_min_avx2 leaves (internal/utils/min_max_avx2_amd64.go): outMinHost / outMaxHost receive one
// element of the column's type each.
func (x *Context) MinMax(typ arrow.Type, values unsafe.Pointer, n int64, outMinHost, outMaxHost unsafe.Pointer) error {
	return x.err(C.ah_min_max(x.c, C.int(typ), values, C.int64_t(n), outMinHost, outMaxHost))
}

// CastBoolToNumeric: boolean → number (kernels/numeric_cast.go:614-640), 1 for a set bit.
func (x *Context) CastBoolToNumeric(out arrow.Type, bits unsafe.Pointer, off, n int64, outValues unsafe.Pointer) error {
	return x.err(C.ah_cast_bool_to_numeric(x.c, C.int(out), (*C.uint8_t)(bits), C.int64_t(off), C.int64_t(n), outValues))
}

// CopyBitmap == bitutil.CopyBitmap / InvertBitmap (arrow/bitutil/bitmaps.go:523-560): bits outside [doff, doff+n) keep their value.
func (x *Context) CopyBitmap(src unsafe.Pointer, soff, n int64, dst unsafe.Pointer, doff int64, invert bool) error {
	return x.err(C.ah_copy_bitmap(x.c, (*C.uint8_t)(src), C.int64_t(soff), C.int64_t(n), (*C.uint8_t)(dst), C.int64_t(doff), boolInt(invert)))
}

// SetBitsTo == bitutil.SetBitsTo (arrow/bitutil/bitutil.go:106-143).
func (x *Context) SetBitsTo(bits unsafe.Pointer, off, n int64, value bool) error {
	return x.err(C.ah_set_bits_to(x.c, (*C.uint8_t)(bits), C.int64_t(off), C.int64_t(n), boolInt(value)))
}

// ---- selection -------------------------------------------------------------------------------------------------------------

// TakeBoolean == the boolean flavour of Take (kernels/vector_selection.go:1194-1271): `data` is a bitmap column.
func (x *Context) TakeBoolean(data, vvalid unsafe.Pointer, voff, nvalues int64, idxWidth int, idxSigned bool, idx, ivalid unsafe.Pointer, ioff, nidx int64,
	outData, outValid unsafe.Pointer) (nulls int64, err error) {
	var r, bad C.int64_t
	err = x.err(C.ah_take_boolean(x.c, (*C.uint8_t)(data), (*C.uint8_t)(vvalid), C.int64_t(voff), C.int64_t(nvalues), C.int(idxWidth), boolInt(idxSigned),
		idx, (*C.uint8_t)(ivalid), C.int64_t(ioff), C.int64_t(nidx), 1, (*C.uint8_t)(outData), (*C.uint8_t)(outValid), &r, &bad))
	return int64(r), err
}

// TakeBinaryOffsets / TakeBinaryData == the two passes of the var-length Take (kernels/vector_selection.go:1273-1440 VarBinaryImpl):
// first the output offsets, validity and total byte count; the caller allocates the data buffer; then the bytes.
func (x *Context) TakeBinaryOffsets(offsetWidth int, offsets, vvalid unsafe.Pointer, voff, nvalues int64, idxWidth int, idxSigned bool,
	idx, ivalid unsafe.Pointer, ioff, nidx int64, outOffsets, outValid unsafe.Pointer) (nulls, totalBytes int64, err error) {
	var r, tot, bad C.int64_t
	err = x.err(C.ah_take_binary_offsets(x.c, C.int(offsetWidth), offsets, (*C.uint8_t)(vvalid), C.int64_t(voff), C.int64_t(nvalues), C.int(idxWidth), boolInt(idxSigned),
		idx, (*C.uint8_t)(ivalid), C.int64_t(ioff), C.int64_t(nidx), 1, outOffsets, (*C.uint8_t)(outValid), &r, &tot, &bad))
	return int64(r), int64(tot), err
}

func (x *Context) TakeBinaryData(offsetWidth int, offsets, data unsafe.Pointer, voff int64, idxWidth int, idx unsafe.Pointer, nidx int64, outOffsets, outData unsafe.Pointer) error {
	return x.err(C.ah_take_binary_data(x.c, C.int(offsetWidth), offsets, (*C.uint8_t)(data), C.int64_t(voff), C.int(idxWidth), idx, C.int64_t(nidx), outOffsets, (*C.uint8_t)(outData)))
}

// ---- hashing ---------------------------------------------------------------------------------------------------------------

// HashFixedEncode: unique / dictionary_encode over FixedSizeBinary / Decimal128 / Decimal256 keys (kernels/vector_hash.go:608-609,
// 698: byteWidth-byte keys through BinaryMemoTable); ids in first-seen order, first rows, the dictionary's bytes.
func (x *Context) HashFixedEncode(byteWidth int, data, valid unsafe.Pointer, off, n int64, encodeNulls bool, outIDs, outIDsValid, outFirstRows, outDict unsafe.Pointer) (ndict int64, nullID int32, err error) {
	var nd C.int64_t
	var nid C.int32_t
	st := C.ah_hash_fixed_encode(x.c, C.int(byteWidth), (*C.uint8_t)(data), (*C.uint8_t)(valid), C.int64_t(off), C.int64_t(n), boolInt(encodeNulls), (*C.int32_t)(outIDs),
		(*C.uint8_t)(outIDsValid), (*C.int64_t)(outFirstRows), (*C.uint8_t)(outDict), &nd, &nid)
	return int64(nd), int32(nid), x.err(st)
}

// HashSumInt64: the group-by sum with Int64 values (wrapping, exact in any order).
func (x *Context) HashSumInt64(keys, kvalid unsafe.Pointer, koff int64, vals, vvalid unsafe.Pointer, voff, n int64,
	outKeys, outSums, outCounts, outFirstRows unsafe.Pointer) (ngroups int64, nullGroup int32, err error) {
	var ng C.int64_t
	var nid C.int32_t
	st := C.ah_hash_sum_i64(x.c, (*C.uint64_t)(keys), (*C.uint8_t)(kvalid), C.int64_t(koff), (*C.int64_t)(vals), (*C.uint8_t)(vvalid), C.int64_t(voff), C.int64_t(n),
		(*C.uint64_t)(outKeys), (*C.int64_t)(outSums), (*C.int64_t)(outCounts), (*C.int64_t)(outFirstRows), &ng, &nid)
	return int64(ng), int32(nid), x.err(st)
}

// HashMinMaxInt64: the group-by minimum / maximum / count with Int64 values (signed order) over the groups of HashSumInt64;
// a group without valid values has count 0 and zero bytes in both.
func (x *Context) HashMinMaxInt64(keys, kvalid unsafe.Pointer, koff int64, vals, vvalid unsafe.Pointer, voff, n int64,
	outKeys, outMins, outMaxs, outCounts, outFirstRows unsafe.Pointer) (ngroups int64, nullGroup int32, err error) {
	var ng C.int64_t
	var nid C.int32_t
	st := C.ah_hash_min_max_i64(x.c, (*C.uint64_t)(keys), (*C.uint8_t)(kvalid), C.int64_t(koff), (*C.int64_t)(vals), (*C.uint8_t)(vvalid), C.int64_t(voff), C.int64_t(n),
		(*C.uint64_t)(outKeys), (*C.int64_t)(outMins), (*C.int64_t)(outMaxs), (*C.int64_t)(outCounts), (*C.int64_t)(outFirstRows), &ng, &nid)
	return int64(ng), int32(nid), x.err(st)
}

// HashMinMaxUint64: the same in unsigned order.
func (x *Context) HashMinMaxUint64(keys, kvalid unsafe.Pointer, koff int64, vals, vvalid unsafe.Pointer, voff, n int64,
	outKeys, outMins, outMaxs, outCounts, outFirstRows unsafe.Pointer) (ngroups int64, nullGroup int32, err error) {
	var ng C.int64_t
	var nid C.int32_t
	st := C.ah_hash_min_max_u64(x.c, (*C.uint64_t)(keys), (*C.uint8_t)(kvalid), C.int64_t(koff), (*C.uint64_t)(vals), (*C.uint8_t)(vvalid), C.int64_t(voff), C.int64_t(n),
		(*C.uint64_t)(outKeys), (*C.uint64_t)(outMins), (*C.uint64_t)(outMaxs), (*C.int64_t)(outCounts), (*C.int64_t)(outFirstRows), &ng, &nid)
	return int64(ng), int32(nid), x.err(st)
}

// HashMinMaxFloat64: the same for Float64: NaNs are counted and otherwise ignored, -0 < +0, a group of NaNs only gives the quiet NaN.
func (x *Context) HashMinMaxFloat64(keys, kvalid unsafe.Pointer, koff int64, vals, vvalid unsafe.Pointer, voff, n int64,
	outKeys, outMins, outMaxs, outCounts, outFirstRows unsafe.Pointer) (ngroups int64, nullGroup int32, err error) {
	var ng C.int64_t
	var nid C.int32_t
	st := C.ah_hash_min_max_f64(x.c, (*C.uint64_t)(keys), (*C.uint8_t)(kvalid), C.int64_t(koff), (*C.double)(vals), (*C.uint8_t)(vvalid), C.int64_t(voff), C.int64_t(n),
		(*C.uint64_t)(outKeys), (*C.double)(outMins), (*C.double)(outMaxs), (*C.int64_t)(outCounts), (*C.int64_t)(outFirstRows), &ng, &nid)
	return int64(ng), int32(nid), x.err(st)
}

// GroupKey is one key column of GroupIDs (ah_group_key): a String / Binary / LargeString / LargeBinary column (OffsetWidth 4 or 8,
// Offsets the offsets buffer, Data the data buffer), a fixed-width column (ByteWidth 1 … 4096 bytes per slot of Data: numeric,
// FixedSizeBinary, Decimal128 / 256) or a Boolean column (Bits, Data the bitmap).  Row i of the call is element Off + i of every
// buffer and bit Off + i of Valid.
type GroupKey struct {
	OffsetWidth int
	ByteWidth   int
	Bits        bool
	Offsets     unsafe.Pointer
	Data        unsafe.Pointer
	Valid       unsafe.Pointer
	Off         int64
}

// GroupIDs: the dense first-seen group ids of a tuple of 1 … 8 key columns, and the first row of every group (ah_group_ids).  Rows
// are in one group when every column is null in both or valid with equal bytes in both; a null is one more value of its column.
// The key table is built in C memory, as in SortIndicesMulti.
func (x *Context) GroupIDs(keys []GroupKey, n int64, outIDs, outFirstRows unsafe.Pointer) (ngroups int64, err error) {
	k := len(keys)
	if k == 0 {
		return 0, fmt.Errorf("%w: arrowhip: GroupIDs wants at least one key", arrow.ErrInvalid)
	}
	var one C.ah_group_key
	tbl := C.malloc(C.size_t(k) * C.size_t(unsafe.Sizeof(one)))
	defer C.free(tbl)
	ks := unsafe.Slice((*C.ah_group_key)(tbl), k)
	for i, key := range keys {
		ks[i].offset_width, ks[i].byte_width, ks[i].bits = C.int(key.OffsetWidth), C.int(key.ByteWidth), boolInt(key.Bits)
		ks[i].offsets, ks[i].data, ks[i].valid, ks[i].off = key.Offsets, (*C.uint8_t)(key.Data), (*C.uint8_t)(key.Valid), C.int64_t(key.Off)
	}
	var ng C.int64_t
	st := C.ah_group_ids(x.c, C.int(k), (*C.ah_group_key)(tbl), C.int64_t(n), (*C.int32_t)(outIDs), (*C.int64_t)(outFirstRows), &ng)
	return int64(ng), x.err(st)
}

// GroupSumInt64 / GroupSumFloat64: the sums and counts of HashSumInt64 / HashSumFloat64 over caller-supplied dense group ids
// (GroupIDs or an encoder with nulls encoded): 0 <= ids[i] < ngroups, which is not checked.
func (x *Context) GroupSumInt64(ids unsafe.Pointer, ngroups int64, vals, vvalid unsafe.Pointer, voff, n int64, outSums, outCounts unsafe.Pointer) error {
	return x.err(C.ah_group_sum_i64(x.c, (*C.int32_t)(ids), C.int64_t(ngroups), (*C.int64_t)(vals), (*C.uint8_t)(vvalid), C.int64_t(voff), C.int64_t(n),
		(*C.int64_t)(outSums), (*C.int64_t)(outCounts)))
}

func (x *Context) GroupSumFloat64(ids unsafe.Pointer, ngroups int64, vals, vvalid unsafe.Pointer, voff, n int64, outSums, outCounts unsafe.Pointer) error {
	return x.err(C.ah_group_sum_f64(x.c, (*C.int32_t)(ids), C.int64_t(ngroups), (*C.double)(vals), (*C.uint8_t)(vvalid), C.int64_t(voff), C.int64_t(n),
		(*C.double)(outSums), (*C.int64_t)(outCounts)))
}

// GroupMinMaxInt64 / Uint64 / Float64: the minima, maxima and counts of HashMinMax* over caller-supplied dense group ids.
func (x *Context) GroupMinMaxInt64(ids unsafe.Pointer, ngroups int64, vals, vvalid unsafe.Pointer, voff, n int64, outMins, outMaxs, outCounts unsafe.Pointer) error {
	return x.err(C.ah_group_min_max_i64(x.c, (*C.int32_t)(ids), C.int64_t(ngroups), (*C.int64_t)(vals), (*C.uint8_t)(vvalid), C.int64_t(voff), C.int64_t(n),
		(*C.int64_t)(outMins), (*C.int64_t)(outMaxs), (*C.int64_t)(outCounts)))
}

func (x *Context) GroupMinMaxUint64(ids unsafe.Pointer, ngroups int64, vals, vvalid unsafe.Pointer, voff, n int64, outMins, outMaxs, outCounts unsafe.Pointer) error {
	return x.err(C.ah_group_min_max_u64(x.c, (*C.int32_t)(ids), C.int64_t(ngroups), (*C.uint64_t)(vals), (*C.uint8_t)(vvalid), C.int64_t(voff), C.int64_t(n),
		(*C.uint64_t)(outMins), (*C.uint64_t)(outMaxs), (*C.int64_t)(outCounts)))
}

func (x *Context) GroupMinMaxFloat64(ids unsafe.Pointer, ngroups int64, vals, vvalid unsafe.Pointer, voff, n int64, outMins, outMaxs, outCounts unsafe.Pointer) error {
	return x.err(C.ah_group_min_max_f64(x.c, (*C.int32_t)(ids), C.int64_t(ngroups), (*C.double)(vals), (*C.uint8_t)(vvalid), C.int64_t(voff), C.int64_t(n),
		(*C.double)(outMins), (*C.double)(outMaxs), (*C.int64_t)(outCounts)))
}

// GroupCount: the number of rows of every group whose validity bit is set (vvalid nil: every row) over caller-supplied dense group
// ids (ah_group_count).  Reads the ids and the validity bits only; outCounts holds ngroups int64.
func (x *Context) GroupCount(ids unsafe.Pointer, ngroups int64, vvalid unsafe.Pointer, voff, n int64, outCounts unsafe.Pointer) error {
	return x.err(C.ah_group_count(x.c, (*C.int32_t)(ids), C.int64_t(ngroups), (*C.uint8_t)(vvalid), C.int64_t(voff), C.int64_t(n), (*C.int64_t)(outCounts)))
}

// GroupSumTyped: GroupSumInt64 / GroupSumFloat64 for a value column of any numeric type id, read at its own width (ah_group_sum_typed).
// outSums holds ngroups 8-byte sums: wrapping Int64 for signed, wrapping Uint64 for unsigned, Float64 for floating-point values.
func (x *Context) GroupSumTyped(typeID arrow.Type, ids unsafe.Pointer, ngroups int64, vals, vvalid unsafe.Pointer, voff, n int64, outSums, outCounts unsafe.Pointer) error {
	return x.err(C.ah_group_sum_typed(x.c, C.int(typeID), (*C.int32_t)(ids), C.int64_t(ngroups), vals, (*C.uint8_t)(vvalid), C.int64_t(voff), C.int64_t(n),
		outSums, (*C.int64_t)(outCounts)))
}

// GroupMinMaxTyped: GroupMinMax* for a value column of any numeric type id (ah_group_min_max_typed); outMins / outMaxs hold ngroups
// values of the input type.
func (x *Context) GroupMinMaxTyped(typeID arrow.Type, ids unsafe.Pointer, ngroups int64, vals, vvalid unsafe.Pointer, voff, n int64, outMins, outMaxs, outCounts unsafe.Pointer) error {
	return x.err(C.ah_group_min_max_typed(x.c, C.int(typeID), (*C.int32_t)(ids), C.int64_t(ngroups), vals, (*C.uint8_t)(vvalid), C.int64_t(voff), C.int64_t(n),
		outMins, outMaxs, (*C.int64_t)(outCounts)))
}

// GroupMean: outMeans[g] = float64(sums[g]) / float64(counts[g]), 0 where the count is 0 (ah_group_mean); sumType says how the sums
// are read: arrow.INT64, arrow.UINT64 or arrow.FLOAT64.
func (x *Context) GroupMean(sumType arrow.Type, sums, counts unsafe.Pointer, ngroups int64, outMeans unsafe.Pointer) error {
	return x.err(C.ah_group_mean(x.c, C.int(sumType), sums, (*C.int64_t)(counts), C.int64_t(ngroups), (*C.double)(outMeans)))
}

// GroupM2: the means, the sums of squared deviations from the mean and the valid counts of every group (ah_group_m2) for a value
// column of any numeric type id, read at its own width and taken as cast to Float64.  outMeans / outM2 hold ngroups float64,
// outCounts ngroups int64; the bytes are the same on every run.
func (x *Context) GroupM2(typeID arrow.Type, ids unsafe.Pointer, ngroups int64, vals, vvalid unsafe.Pointer, voff, n int64, outMeans, outM2, outCounts unsafe.Pointer) error {
	return x.err(C.ah_group_m2(x.c, C.int(typeID), (*C.int32_t)(ids), C.int64_t(ngroups), vals, (*C.uint8_t)(vvalid), C.int64_t(voff), C.int64_t(n),
		(*C.double)(outMeans), (*C.double)(outM2), (*C.int64_t)(outCounts)))
}

// GroupVariance: out[g] = m2[g] / float64(counts[g] - ddof), its square root with takeSqrt, 0 where counts[g] <= ddof
// (ah_group_variance).
func (x *Context) GroupVariance(m2, counts unsafe.Pointer, ngroups int64, ddof int, takeSqrt bool, out unsafe.Pointer) error {
	s := 0
	if takeSqrt {
		s = 1
	}
	return x.err(C.ah_group_variance(x.c, (*C.double)(m2), (*C.int64_t)(counts), C.int64_t(ngroups), C.int(ddof), C.int(s), (*C.double)(out)))
}

// JoinBuild: the build side of a hash join over caller-supplied dense group ids as a CSR (ah_join_build): outStarts[g] .. outStarts[g+1]
// (ngroups + 1 int64) delimit, in outRows (nBuild int64 of room), the valid build rows of group g in ascending row order.
func (x *Context) JoinBuild(buildIDs, buildValid unsafe.Pointer, voff, nBuild, ngroups int64, outStarts, outRows unsafe.Pointer) error {
	return x.err(C.ah_join_build(x.c, (*C.int32_t)(buildIDs), (*C.uint8_t)(buildValid), C.int64_t(voff), C.int64_t(nBuild), C.int64_t(ngroups),
		(*C.int64_t)(outStarts), (*C.int64_t)(outRows)))
}

// JoinCount: outOffsets (nProbe + 1 int64) = the exclusive scan of every probe row's match count, at least 1 with emitUnmatched
// (ah_join_count); total is the number of rows of the join's result.
func (x *Context) JoinCount(probeIDs, probeValid unsafe.Pointer, poff, nProbe int64, starts unsafe.Pointer, emitUnmatched bool, outOffsets unsafe.Pointer) (total int64, err error) {
	var t C.int64_t
	err = x.err(C.ah_join_count(x.c, (*C.int32_t)(probeIDs), (*C.uint8_t)(probeValid), C.int64_t(poff), C.int64_t(nProbe), (*C.int64_t)(starts),
		boolInt(emitUnmatched), (*C.int64_t)(outOffsets), &t))
	return int64(t), err
}

// JoinExpand: the probe row and the build row of every output slot, total int64 each (ah_join_expand); with emitUnmatched also the
// validity bitmap of the build rows (outBuildValid), whose clear bits are counted in nulls.
func (x *Context) JoinExpand(probeIDs, probeValid unsafe.Pointer, poff, nProbe int64, starts, rows, offsets unsafe.Pointer, total int64, emitUnmatched bool,
	outProbeRows, outBuildRows, outBuildValid unsafe.Pointer) (nulls int64, err error) {
	var nc C.int64_t
	err = x.err(C.ah_join_expand(x.c, (*C.int32_t)(probeIDs), (*C.uint8_t)(probeValid), C.int64_t(poff), C.int64_t(nProbe), (*C.int64_t)(starts),
		(*C.int64_t)(rows), (*C.int64_t)(offsets), C.int64_t(total), boolInt(emitUnmatched), (*C.int64_t)(outProbeRows), (*C.int64_t)(outBuildRows),
		(*C.uint8_t)(outBuildValid), &nc))
	return int64(nc), err
}

// JoinMatchBits: bit i of outBits = probe row i is valid and its group holds a build row (ah_join_match_bits): the mask of a semi join.
func (x *Context) JoinMatchBits(probeIDs, probeValid unsafe.Pointer, poff, nProbe int64, starts, outBits unsafe.Pointer) error {
	return x.err(C.ah_join_match_bits(x.c, (*C.int32_t)(probeIDs), (*C.uint8_t)(probeValid), C.int64_t(poff), C.int64_t(nProbe), (*C.int64_t)(starts),
		(*C.uint8_t)(outBits)))
}

// Lz4DecompressBlocks: independent LZ4 blocks of the device bytes src inflated into the device bytes dst (ah_lz4_decompress_blocks).
// blocks holds 4 values per block {srcOff, srcLen (bit 62: stored), dstOff, dstLen ≤ 65536}, dstOff ascending; status receives one
// byte per block (0 ok, 1 corrupt, 2 produced != dstLen) and nbad is the number of blocks with a status — those leave unspecified
// bytes in their own output range only and are not an error of the call.
func (x *Context) Lz4DecompressBlocks(src unsafe.Pointer, srcBytes int64, dst unsafe.Pointer, dstBytes int64, blocks []int64, status []byte) (nbad int64, err error) {
	if len(blocks)%4 != 0 || len(status) < len(blocks)/4 {
		return 0, fmt.Errorf("%w: lz4 block table of %d values with %d status bytes", arrow.ErrInvalid, len(blocks), len(status))
	}
	if len(blocks) == 0 {
		return 0, nil
	}
	tb := (*C.int64_t)(unsafe.Pointer(&blocks[0]))
	sb := (*C.uint8_t)(unsafe.Pointer(&status[0]))
	var bad C.int64_t
	st := C.ah_lz4_decompress_blocks(x.c, (*C.uint8_t)(src), C.int64_t(srcBytes), (*C.uint8_t)(dst), C.int64_t(dstBytes), tb, C.int64_t(len(blocks)/4), sb, &bad)
	return int64(bad), x.err(st)
}

// Lz4CompressBlocks: blocks of at most 65536 bytes of the device bytes src, each compressed on its own as one LZ4 block into its slot
// of the device bytes dst (ah_lz4_compress_blocks).  blocks holds 3 values per block {srcOff, srcLen, dstOff}; the slots
// dst[dstOff, dstOff+srcLen) ascend without overlap.  sizes receives the bytes written to every slot, stored 1 where the block did
// not shrink and its slot holds the input bytes.
func (x *Context) Lz4CompressBlocks(src unsafe.Pointer, srcBytes int64, dst unsafe.Pointer, dstBytes int64, blocks []int64, sizes []int32, stored []byte) error {
	n := len(blocks) / 3
	if len(blocks)%3 != 0 || len(sizes) < n || len(stored) < n {
		return fmt.Errorf("%w: lz4 block table of %d values with %d sizes and %d flags", arrow.ErrInvalid, len(blocks), len(sizes), len(stored))
	}
	if n == 0 {
		return nil
	}
	return x.err(C.ah_lz4_compress_blocks(x.c, (*C.uint8_t)(src), C.int64_t(srcBytes), (*C.uint8_t)(dst), C.int64_t(dstBytes),
		(*C.int64_t)(unsafe.Pointer(&blocks[0])), C.int64_t(n), (*C.int32_t)(unsafe.Pointer(&sizes[0])), (*C.uint8_t)(unsafe.Pointer(&stored[0]))))
}

// IpcPackBody: the device bytes dst[0, dstBytes) put together from the pieces of rows, 4 values per row {srcOff, len, dstOff, word}
// (ah_ipc_pack_body): word&3 selects the device bytes comp (0), the device bytes plain (1) or the host bytes lits (2); word bit 8
// writes the 32 bits above bit 32 of word, little-endian, in the 4 bytes before dstOff.  The rows must tile the output exactly.
func (x *Context) IpcPackBody(comp unsafe.Pointer, compBytes int64, plain unsafe.Pointer, plainBytes int64, lits []byte, rows []int64, dst unsafe.Pointer, dstBytes int64) error {
	if len(rows)%4 != 0 {
		return fmt.Errorf("%w: pack table of %d values", arrow.ErrInvalid, len(rows))
	}
	var lp *C.uint8_t
	if len(lits) > 0 {
		lp = (*C.uint8_t)(unsafe.Pointer(&lits[0]))
	}
	var rp *C.int64_t
	if len(rows) > 0 {
		rp = (*C.int64_t)(unsafe.Pointer(&rows[0]))
	}
	return x.err(C.ah_ipc_pack_body(x.c, (*C.uint8_t)(comp), C.int64_t(compBytes), (*C.uint8_t)(plain), C.int64_t(plainBytes), lp, C.int64_t(len(lits)),
		rp, C.int64_t(len(rows)/4), (*C.uint8_t)(dst), C.int64_t(dstBytes)))
}

// HashPartition: partition id of every key by the reference's integer hash (internal/hashing/hash_funcs.go:60-67) — the owner
// function of the C5 merge.
func (x *Context) HashPartition(keys unsafe.Pointer, n int64, nparts int, outPart unsafe.Pointer) error {
	return x.err(C.ah_hash_partition_u64(x.c, (*C.uint64_t)(keys), C.int64_t(n), C.int(nparts), (*C.int32_t)(outPart)))
}

// ---- fused / sort ----------------------------------------------------------------------------------------------------------

// CmpFilterSumFloat64 is the fused Compare→Filter→Sum over Float64 (the sum as math.Float64.Sum would give it, DESIGN.md §4).
func (x *Context) CmpFilterSumFloat64(cmpop int, values, valid unsafe.Pointer, off, n int64, threshold float64) (sum float64, count int64, err error) {
	var s C.double
	var c C.int64_t
	err = x.err(C.ah_cmp_filter_sum_f64(x.c, C.int(cmpop), (*C.double)(values), (*C.uint8_t)(valid), C.int64_t(off), C.int64_t(n), C.double(threshold), &s, &c))
	return float64(s), int64(c), err
}

// CmpFilterSumInt64Dev / CmpFilterSumFloat64Dev leave {sum, count} in device memory (no host round trip).
func (x *Context) CmpFilterSumInt64Dev(cmpop int, values, valid unsafe.Pointer, off, n, threshold int64, outSumCountDev unsafe.Pointer) error {
	return x.err(C.ah_cmp_filter_sum_i64_dev(x.c, C.int(cmpop), (*C.int64_t)(values), (*C.uint8_t)(valid), C.int64_t(off), C.int64_t(n), C.int64_t(threshold), (*C.int64_t)(outSumCountDev)))
}

func (x *Context) CmpFilterSumFloat64Dev(cmpop int, values, valid unsafe.Pointer, off, n int64, threshold float64, outSumDev, outCountDev unsafe.Pointer) error {
	return x.err(C.ah_cmp_filter_sum_f64_dev(x.c, C.int(cmpop), (*C.double)(values), (*C.uint8_t)(valid), C.int64_t(off), C.int64_t(n), C.double(threshold),
		(*C.double)(outSumDev), (*C.int64_t)(outCountDev)))
}

// SortKey is one column of a multi-key sort (compute.SortKey, compute/vector_sort.go:40-60).
type SortKey struct {
	Type         arrow.Type
	Values       unsafe.Pointer
	Valid        unsafe.Pointer
	Off          int64
	Descending   bool
	NullsAtStart bool
}

// SortIndicesMulti mirrors the multi-column path of sort_indices (compute/vector_sort.go:217-330): a stable lexicographic order.
// The pointer tables are built in C memory: cgo forbids passing Go memory that itself holds pointers.
func (x *Context) SortIndicesMulti(keys []SortKey, n int64, outIndices unsafe.Pointer) error {
	k := len(keys)
	if k == 0 {
		return fmt.Errorf("%w: arrowhip: SortIndicesMulti wants at least one key", arrow.ErrInvalid)
	}
	ptrSize := C.size_t(unsafe.Sizeof(unsafe.Pointer(nil)))
	vals := C.malloc(C.size_t(k) * ptrSize)
	defer C.free(vals)
	valids := C.malloc(C.size_t(k) * ptrSize)
	defer C.free(valids)
	vslice := unsafe.Slice((*unsafe.Pointer)(vals), k)
	mslice := unsafe.Slice((*unsafe.Pointer)(valids), k)
	types := make([]C.int, k)
	desc := make([]C.int, k)
	nulls := make([]C.int, k)
	offs := make([]C.int64_t, k)
	for i, key := range keys {
		vslice[i], mslice[i] = key.Values, key.Valid
		types[i], desc[i], nulls[i], offs[i] = C.int(key.Type), boolInt(key.Descending), boolInt(key.NullsAtStart), C.int64_t(key.Off)
	}
	return x.err(C.ah_sort_indices_multi(x.c, C.int(k), &types[0], (*unsafe.Pointer)(vals), (**C.uint8_t)(valids), &offs[0], C.int64_t(n), &desc[0], &nulls[0], (*C.uint64_t)(outIndices)))
}

// SortColumn is one key of SortIndicesKeys: a numeric column (Values), a String / Binary / LargeString / LargeBinary column
// (Values = the data buffer, Offsets = the offsets buffer) or a FixedSizeBinary / Decimal128 / Decimal256 column (Values = the
// slots, ByteWidth = their width).  Row i of the call is element Off + i of every buffer and bit Off + i of Valid.
type SortColumn struct {
	Type         arrow.Type
	Values       unsafe.Pointer
	Offsets      unsafe.Pointer
	ByteWidth    int
	Valid        unsafe.Pointer
	Off          int64
	Descending   bool
	NullsAtStart bool
}

// SortIndicesKeys mirrors sort_indices over keys of every sortable kind (kernels/vector_sort.go:195-245): stable, lexicographic
// by key 0, 1, …; binary values bytewise, decimals by value.  The key table is built in C memory, as in SortIndicesMulti.
func (x *Context) SortIndicesKeys(keys []SortColumn, n int64, outIndices unsafe.Pointer) error {
	if len(keys) == 0 {
		return fmt.Errorf("%w: arrowhip: SortIndicesKeys wants at least one key", arrow.ErrInvalid)
	}
	tbl := sortKeyTable(keys)
	defer C.free(tbl)
	return x.err(C.ah_sort_indices_keys(x.c, C.int(len(keys)), (*C.ah_sort_key)(tbl), C.int64_t(n), (*C.uint64_t)(outIndices)))
}

// sortKeyTable is the ah_sort_key table of the keys, in C memory: the caller frees it.
func sortKeyTable(keys []SortColumn) unsafe.Pointer {
	k := len(keys)
	var one C.ah_sort_key
	tbl := C.malloc(C.size_t(k) * C.size_t(unsafe.Sizeof(one)))
	ks := unsafe.Slice((*C.ah_sort_key)(tbl), k)
	for i, key := range keys {
		typ := C.int(key.Type)
		switch key.Type {
		case arrow.STRING:
			typ = C.AH_BINARY
		case arrow.LARGE_STRING:
			typ = C.AH_LARGE_BINARY
		}
		ks[i]._type, ks[i].values, ks[i].offsets, ks[i].byte_width = typ, key.Values, key.Offsets, C.int(key.ByteWidth)
		ks[i].valid, ks[i].off = (*C.uint8_t)(key.Valid), C.int64_t(key.Off)
		ks[i].descending, ks[i].nulls_at_start = boolInt(key.Descending), boolInt(key.NullsAtStart)
	}
	return tbl
}

// SelectKRoute is the route of SelectK: the library's choice, the radix route (a numeric first key), or the sort and its head.
type SelectKRoute int

const (
	SelectKAuto  SelectKRoute = C.AH_SELECT_AUTO
	SelectKRadix SelectKRoute = C.AH_SELECT_RADIX
	SelectKSort  SelectKRoute = C.AH_SELECT_SORT
)

// SelectK writes the first min(k, n) entries SortIndicesKeys would write for the same keys (ORDER BY … LIMIT k), without sorting
// the column where the first key is numeric.  outIndices holds min(k, n) uint64 row numbers.
func (x *Context) SelectK(keys []SortColumn, n, k int64, route SelectKRoute, outIndices unsafe.Pointer) error {
	if len(keys) == 0 {
		return fmt.Errorf("%w: arrowhip: SelectK wants at least one key", arrow.ErrInvalid)
	}
	tbl := sortKeyTable(keys)
	defer C.free(tbl)
	return x.err(C.ah_select_k(x.c, C.int(len(keys)), (*C.ah_sort_key)(tbl), C.int64_t(n), C.int64_t(k), C.int(route), (*C.uint64_t)(outIndices)))
}

// ---- window functions: ranks and running aggregates over the partitions of a sort order ---------------------------------------
// The caller brings dense partition ids (GroupIds) and the order SortIndicesKeys wrote for (partition id, order keys); the three
// calls are enqueued on the compute stream and do not synchronise.  order nil: the identity.

// WindowRankKind selects what WindowRank writes.
type WindowRankKind int

const (
	WindowRowNumber WindowRankKind = C.AH_WINDOW_ROW_NUMBER
	WindowRank      WindowRankKind = C.AH_WINDOW_RANK
	WindowDenseRank WindowRankKind = C.AH_WINDOW_DENSE_RANK
)

// WindowScanOp selects the running aggregate of WindowScan.
type WindowScanOp int

const (
	WindowSum   WindowScanOp = C.AH_WINDOW_SUM
	WindowMin   WindowScanOp = C.AH_WINDOW_MIN
	WindowMax   WindowScanOp = C.AH_WINDOW_MAX
	WindowCount WindowScanOp = C.AH_WINDOW_COUNT
)

// WindowFlags writes one byte per sorted position p (row order[p]): bit 0 a partition starts there (partIds: int32 by row, nil =
// one partition), bit 1 a peer group starts there (the rows at p-1 and p do not tie on every key).  No keys: every row is its own
// peer group.
func (x *Context) WindowFlags(partIds unsafe.Pointer, keys []SortColumn, order unsafe.Pointer, n int64, outFlags unsafe.Pointer) error {
	var tbl unsafe.Pointer
	if len(keys) > 0 {
		tbl = sortKeyTable(keys)
		defer C.free(tbl)
	}
	return x.err(C.ah_window_flags(x.c, (*C.int32_t)(partIds), C.int(len(keys)), (*C.ah_sort_key)(tbl), (*C.uint64_t)(order), C.int64_t(n), (*C.uint8_t)(outFlags)))
}

// WindowRank writes out[order[p]] (uint64, 1-based) = the row number, rank or dense rank at sorted position p.
func (x *Context) WindowRank(kind WindowRankKind, flags, order unsafe.Pointer, n int64, out unsafe.Pointer) error {
	return x.err(C.ah_window_rank(x.c, C.int(kind), (*C.uint8_t)(flags), (*C.uint64_t)(order), C.int64_t(n), (*C.uint64_t)(out)))
}

// WindowScan writes outValues[order[p]] = the running aggregate of the column over the row's partition up to sorted position p.
// Sums are 8 bytes per row (Int64, Uint64 or Float64), minima and maxima have the input type, counts are Int64.  A null row gets
// payload 0; the output's validity is the input's, which the caller copies (CopyBitmap).
func (x *Context) WindowScan(op WindowScanOp, typeID arrow.Type, values, valid unsafe.Pointer, off int64, flags, order unsafe.Pointer, n int64, outValues unsafe.Pointer) error {
	return x.err(C.ah_window_scan(x.c, C.int(op), C.int(typeID), values, (*C.uint8_t)(valid), C.int64_t(off), (*C.uint8_t)(flags), (*C.uint64_t)(order), C.int64_t(n), outValues))
}

// ---- conditionals: if_else and the directed null fills (no reference analogue; Arrow C++'s semantics) ---------------------------

// CondSide is one side of the IfElse calls (ah_cond_side).  Fixed width: OffsetWidth 0, Data the slots of ByteWidth bytes; Boolean
// (IfElseBoolean): Data a bitmap; var-length: OffsetWidth 4 or 8, Offsets the offsets buffer, Data the value bytes.  Valid (nil: no
// nulls) and, for Boolean sides, Data are read at bit Off + i; row i is element Off + i.  Broadcast: a scalar as a one-row device
// column, every row reads element Off.
type CondSide struct {
	OffsetWidth, ByteWidth int
	Offsets, Data, Valid   unsafe.Pointer
	Off                    int64
	Broadcast              bool
}

func (o CondSide) c() C.ah_cond_side {
	var r C.ah_cond_side
	r.offset_width, r.byte_width, r.offsets, r.data, r.valid, r.off = C.int(o.OffsetWidth), C.int(o.ByteWidth), o.Offsets, o.Data, (*C.uint8_t)(o.Valid), C.int64_t(o.Off)
	if o.Broadcast {
		r.broadcast = 1
	}
	return r
}

// IfElse writes row i = l[i] where the condition's bit condOff + i is set, else r[i]; the row is null where the condition or the
// chosen side is (payload 0).  Fixed-width sides of one byte width.  outValid (from bit 0) may be nil only when condValid and both
// sides' Valid are.  Enqueued; no synchronisation.
func (x *Context) IfElse(condData, condValid unsafe.Pointer, condOff int64, l, r CondSide, n int64, outValues, outValid unsafe.Pointer) error {
	lc, rc := l.c(), r.c()
	return x.err(C.ah_if_else(x.c, (*C.uint8_t)(condData), (*C.uint8_t)(condValid), C.int64_t(condOff), &lc, &rc, C.int64_t(n), outValues, (*C.uint8_t)(outValid)))
}

// IfElseBoolean is IfElse for Boolean sides: outData and outValid are bitmaps from bit 0, a null row's data bit is 0.
func (x *Context) IfElseBoolean(condData, condValid unsafe.Pointer, condOff int64, l, r CondSide, n int64, outData, outValid unsafe.Pointer) error {
	lc, rc := l.c(), r.c()
	return x.err(C.ah_if_else_boolean(x.c, (*C.uint8_t)(condData), (*C.uint8_t)(condValid), C.int64_t(condOff), &lc, &rc, C.int64_t(n), (*C.uint8_t)(outData), (*C.uint8_t)(outValid)))
}

// IfElseBinaryOffsets is the first call for var-length sides: outOffsets[0 … n] (outOffsetWidth bytes each, from 0), the validity, and
// the number of value bytes to allocate for IfElseBinaryData.  Bytes that do not fit 4-byte offsets are arrow.ErrInvalid.
func (x *Context) IfElseBinaryOffsets(condData, condValid unsafe.Pointer, condOff int64, l, r CondSide, n int64, outOffsetWidth int, outOffsets, outValid unsafe.Pointer) (totalBytes int64, err error) {
	lc, rc := l.c(), r.c()
	var tot C.int64_t
	err = x.err(C.ah_if_else_binary_offsets(x.c, (*C.uint8_t)(condData), (*C.uint8_t)(condValid), C.int64_t(condOff), &lc, &rc, C.int64_t(n), C.int(outOffsetWidth), outOffsets, (*C.uint8_t)(outValid), &tot))
	return int64(tot), err
}

// IfElseBinaryData copies the chosen rows' bytes behind the offsets IfElseBinaryOffsets wrote.
func (x *Context) IfElseBinaryData(condData, condValid unsafe.Pointer, condOff int64, l, r CondSide, n int64, outOffsetWidth int, outOffsets, outData unsafe.Pointer) error {
	lc, rc := l.c(), r.c()
	return x.err(C.ah_if_else_binary_data(x.c, (*C.uint8_t)(condData), (*C.uint8_t)(condValid), C.int64_t(condOff), &lc, &rc, C.int64_t(n), C.int(outOffsetWidth), outOffsets, (*C.uint8_t)(outData)))
}

// FillDirection of the directed null fills: a null row takes the nearest valid row before (forward) or after (backward) it.
type FillDirection int

const (
	FillForward  FillDirection = 0
	FillBackward FillDirection = 1
)

// FillNullIndices writes per row the number of the row it takes its value from (uint32, 0 where there is none) and that slot's
// validity bit: the (indices, validity) pair the Take calls read.  Returns the number of rows that stay null.
func (x *Context) FillNullIndices(valid unsafe.Pointer, off, n int64, direction FillDirection, outIdx, outIdxValid unsafe.Pointer) (nulls int64, err error) {
	var r C.int64_t
	err = x.err(C.ah_fill_null_indices(x.c, (*C.uint8_t)(valid), C.int64_t(off), C.int64_t(n), C.int(direction), (*C.uint32_t)(outIdx), (*C.uint8_t)(outIdxValid), &r))
	return int64(r), err
}

// FillNullDirected is the same walk with the gather fused in, for values of 1, 2, 4, 8, 16 or 32 bytes: outValues[i] =
// values[off + source of row i], payload 0 where a row stays null.  Returns the number of rows that stay null.
func (x *Context) FillNullDirected(byteWidth int, values, valid unsafe.Pointer, off, n int64, direction FillDirection, outValues, outValid unsafe.Pointer) (nulls int64, err error) {
	var r C.int64_t
	err = x.err(C.ah_fill_null_directed(x.c, C.int(byteWidth), values, (*C.uint8_t)(valid), C.int64_t(off), C.int64_t(n), C.int(direction), outValues, (*C.uint8_t)(outValid), &r))
	return int64(r), err
}

// ---- ingest slots: the building blocks of Ingest for callers that run their own kernels on the chunks ------------------------

func (i *Ingest) Depth() int      { return int(C.ah_ingest_depth(i.g)) }
func (i *Ingest) ChunkBytes() int { return int(C.ah_ingest_chunk_bytes(i.g)) }

// SlotBuffer: device buffer `which` (0, 1 inputs; 2 output) of a slot.
func (i *Ingest) SlotBuffer(slot, which int) unsafe.Pointer {
	return C.ah_ingest_slot_buffer(i.g, C.int(slot), C.int(which))
}

func (i *Ingest) SlotUpload(slot, which int, dstOffset int, host []byte, firstOfChunk bool) error {
	if len(host) == 0 {
		return nil
	}
	return i.ctx.err(C.ah_ingest_slot_upload(i.g, C.int(slot), C.int(which), C.size_t(dstOffset), unsafe.Pointer(&host[0]), C.size_t(len(host)), boolInt(firstOfChunk)))
}

func (i *Ingest) SlotReady(slot int, writesOutput bool) error {
	return i.ctx.err(C.ah_ingest_slot_ready(i.g, C.int(slot), boolInt(writesOutput)))
}

func (i *Ingest) SlotRelease(slot int) error { return i.ctx.err(C.ah_ingest_slot_release(i.g, C.int(slot))) }

func (i *Ingest) SlotDownload(slot, which int, srcOffset int, host []byte) error {
	if len(host) == 0 {
		return nil
	}
	return i.ctx.err(C.ah_ingest_slot_download(i.g, C.int(slot), C.int(which), C.size_t(srcOffset), unsafe.Pointer(&host[0]), C.size_t(len(host))))
}

func (i *Ingest) Wait() error { return i.ctx.err(C.ah_ingest_wait(i.g)) }

// SetPiece is one piece of an is_in value set (ah_set_chunk): a plain array is one piece, a chunked value set one piece per
// chunk.  Base-binary pieces: OffsetWidth 4 or 8, Offsets the offsets buffer, Data the value bytes.  Fixed-width pieces:
// OffsetWidth 0, Data the slots.  Row i of the piece is element Off + i of every buffer and bit Off + i of Valid.
type SetPiece struct {
	OffsetWidth int
	Offsets     unsafe.Pointer
	Data        unsafe.Pointer
	Valid       unsafe.Pointer
	Off, N      int64
}

func setPieces(set []SetPiece) (unsafe.Pointer, func()) {
	if len(set) == 0 {
		return nil, func() {}
	}
	var one C.ah_set_chunk
	tbl := C.malloc(C.size_t(len(set)) * C.size_t(unsafe.Sizeof(one)))
	ps := unsafe.Slice((*C.ah_set_chunk)(tbl), len(set))
	for i, p := range set {
		ps[i].offset_width, ps[i].offsets, ps[i].data = C.int(p.OffsetWidth), p.Offsets, (*C.uint8_t)(p.Data)
		ps[i].valid, ps[i].off, ps[i].n = (*C.uint8_t)(p.Valid), C.int64_t(p.Off), C.int64_t(p.N)
	}
	return tbl, func() { C.free(tbl) }
}

// IsInBinary mirrors SetLookupState[[]byte] + isInKernelExec for String / Binary / LargeString / LargeBinary rows
// (kernels/scalar_set_lookup.go:192-244, 270-300, 374-413): bytewise membership, every piece of the value set in one table.
func (x *Context) IsInBinary(offsetWidth int, offsets, data, valid unsafe.Pointer, off, n int64, set []SetPiece, nullBehavior int,
	outData, outValid unsafe.Pointer, outBitOffset int64) error {
	tbl, free := setPieces(set)
	defer free()
	return x.err(C.ah_is_in_binary(x.c, C.int(offsetWidth), offsets, (*C.uint8_t)(data), (*C.uint8_t)(valid), C.int64_t(off), C.int64_t(n),
		C.int(len(set)), (*C.ah_set_chunk)(tbl), C.int(nullBehavior), (*C.uint8_t)(outData), (*C.uint8_t)(outValid), C.int64_t(outBitOffset)))
}

// IsInFixed mirrors is_in of fixed-width rows — FixedSizeBinary, Decimal128 / Decimal256 and the numeric types
// (visitBinary / visitNumeric, kernels/scalar_set_lookup.go:106-133, 270-300): raw-byte membership.
func (x *Context) IsInFixed(byteWidth int, data, valid unsafe.Pointer, off, n int64, set []SetPiece, nullBehavior int,
	outData, outValid unsafe.Pointer, outBitOffset int64) error {
	tbl, free := setPieces(set)
	defer free()
	return x.err(C.ah_is_in_fixed(x.c, C.int(byteWidth), (*C.uint8_t)(data), (*C.uint8_t)(valid), C.int64_t(off), C.int64_t(n), C.int(len(set)),
		(*C.ah_set_chunk)(tbl), C.int(nullBehavior), (*C.uint8_t)(outData), (*C.uint8_t)(outValid), C.int64_t(outBitOffset)))
}

// IsInDictGather finishes is_in of a dictionary column (ensureDictionaryDecoded + execIsIn, compute/scalar_set_lookup.go:56-61)
// without decoding it: bits 0 … lutN − 1 of lutData / lutValid are is_in of the dictionary's entries, bit lutN that of a null.
func (x *Context) IsInDictGather(indexWidth int, indices, valid unsafe.Pointer, off, n int64, lutData, lutValid unsafe.Pointer, lutN int64,
	outData, outValid unsafe.Pointer, outBitOffset int64) error {
	return x.err(C.ah_is_in_dict_gather(x.c, C.int(indexWidth), indices, (*C.uint8_t)(valid), C.int64_t(off), C.int64_t(n), (*C.uint8_t)(lutData),
		(*C.uint8_t)(lutValid), C.int64_t(lutN), (*C.uint8_t)(outData), (*C.uint8_t)(outValid), C.int64_t(outBitOffset)))
}

// CmpOperand is one side of CompareBinary (ah_cmp_operand).  Base-binary: OffsetWidth 4 or 8, Offsets the offsets buffer, Data the
// value bytes.  FixedSizeBinary: OffsetWidth 0, Data the slots of ByteWidth bytes.  Row i is element Off + i; Broadcast: a scalar,
// every row reads element Off.
type CmpOperand struct {
	OffsetWidth, ByteWidth int
	Offsets, Data          unsafe.Pointer
	Off                    int64
	Broadcast              bool
}

func (o CmpOperand) c() C.ah_cmp_operand {
	var r C.ah_cmp_operand
	r.offset_width, r.byte_width, r.offsets, r.data, r.off = C.int(o.OffsetWidth), C.int(o.ByteWidth), o.Offsets, (*C.uint8_t)(o.Data), C.int64_t(o.Off)
	if o.Broadcast {
		r.broadcast = 1
	}
	return r
}

// CompareBinary mirrors getBinaryCmp over the base-binary and FixedSizeBinary kernels of CompareKernels
// (kernels/scalar_comparisons.go:520-540, 694-713): bytes.Equal / bytes.Compare of every row, null slots included, into bits
// [outBitOffset, outBitOffset + n) of outBits.  The two sides may have different layouts.
func (x *Context) CompareBinary(cmpOp int, l, r CmpOperand, n int64, outBits unsafe.Pointer, outBitOffset int64) error {
	lc, rc := l.c(), r.c()
	return x.err(C.ah_compare_binary(x.c, C.int(cmpOp), &lc, &rc, C.int64_t(n), (*C.uint8_t)(outBits), C.int64_t(outBitOffset)))
}

// CompareDecimal mirrors genDecimalCompareKernel (kernels/scalar_comparisons.go:370-392) after castBinaryDecimalArgs: each side
// 16 or 32 bytes wide, compared as value · 10^scaleUp by signed value.  lBroadcast / rBroadcast 1: that side is a scalar.
func (x *Context) CompareDecimal(cmpOp int, lWidth int, l unsafe.Pointer, lOff int64, lBroadcast int, lScaleUp int,
	rWidth int, r unsafe.Pointer, rOff int64, rBroadcast int, rScaleUp int, n int64, outBits unsafe.Pointer, outBitOffset int64) error {
	return x.err(C.ah_compare_decimal(x.c, C.int(cmpOp), C.int(lWidth), (*C.uint8_t)(l), C.int64_t(lOff), C.int(lBroadcast), C.int(lScaleUp),
		C.int(rWidth), (*C.uint8_t)(r), C.int64_t(rOff), C.int(rBroadcast), C.int(rScaleUp), C.int64_t(n), (*C.uint8_t)(outBits), C.int64_t(outBitOffset)))
}

// CastDecimalRescale mirrors CastDecimalToDecimal (kernels/numeric_cast.go:377-429): inWidth / outWidth 16 or 32 bytes, scaleDelta the
// output's scale minus the input's.  allowTruncate false: data loss and a value beyond outPrecision are arrow.ErrInvalid for the first
// offending valid row; true: truncate toward zero / wrap, no precision check.  values points at the first row, off is its bit in valid.
func (x *Context) CastDecimalRescale(inWidth, outWidth, scaleDelta, outPrecision int, allowTruncate bool, values, valid unsafe.Pointer,
	off, n int64, dst unsafe.Pointer) error {
	return x.err(C.ah_cast_decimal_rescale(x.c, C.int(inWidth), C.int(outWidth), C.int(scaleDelta), C.int(outPrecision), boolInt(allowTruncate),
		values, (*C.uint8_t)(valid), C.int64_t(off), C.int64_t(n), dst))
}

// CastIntToDecimal mirrors CastIntegerToDecimal (kernels/numeric_cast.go:173-239): value · 10^scale into 16- or 32-byte slots; the
// precision check against MaxDecimalDigitsForInt is the caller's.
func (x *Context) CastIntToDecimal(in arrow.Type, outWidth, scale int, values, valid unsafe.Pointer, off, n int64, dst unsafe.Pointer) error {
	return x.err(C.ah_cast_int_to_decimal(x.c, C.int(in), C.int(outWidth), C.int(scale), values, (*C.uint8_t)(valid), C.int64_t(off), C.int64_t(n), dst))
}

// CastDecimalToInt mirrors CastDecimal128ToInteger / CastDecimal256ToInteger (kernels/numeric_cast.go:79-171); allowTruncate is
// CastOptions.AllowDecimalTruncate (round half away from zero instead of the data-loss error), allowOverflow is AllowIntOverflow.
func (x *Context) CastDecimalToInt(inWidth, inScale int, out arrow.Type, allowTruncate, allowOverflow bool, values, valid unsafe.Pointer, off, n int64,
	dst unsafe.Pointer) error {
	return x.err(C.ah_cast_decimal_to_int(x.c, C.int(inWidth), C.int(inScale), C.int(out), boolInt(allowTruncate), boolInt(allowOverflow),
		values, (*C.uint8_t)(valid), C.int64_t(off), C.int64_t(n), dst))
}

// ParseInt mirrors getParseStringExec under ScalarUnaryNotNullBinaryArg (kernels/numeric_cast.go:742-781): strconv.ParseInt /
// ParseUint(s, 0, bits) of every valid row of a String / Binary column (offsetWidth 4) or LargeString / LargeBinary column (8) into
// out's slots, 0 for a null row.  offsets is the offsets buffer, off the array's offset.  On arrow.ErrInvalid badRow is the LAST
// offending valid row (relative to off), as the reference reports it, and badKind 1 (strconv.ErrSyntax) or 2 (strconv.ErrRange).
func (x *Context) ParseInt(offsetWidth int, offsets, data, valid unsafe.Pointer, off, n int64, out arrow.Type, dst unsafe.Pointer) (badRow int64, badKind int, err error) {
	var row C.int64_t
	var kind C.int
	err = x.err(C.ah_parse_int(x.c, C.int(offsetWidth), offsets, (*C.uint8_t)(data), (*C.uint8_t)(valid), C.int64_t(off), C.int64_t(n), C.int(out), dst, &row, &kind))
	return int64(row), int(kind), err
}

// ParseBool mirrors the strconv.ParseBool kernels (kernels/boolean_cast.go:77-95): the result bitmap from bit 0.
func (x *Context) ParseBool(offsetWidth int, offsets, data, valid unsafe.Pointer, off, n int64, dstBits unsafe.Pointer) (badRow int64, err error) {
	var row C.int64_t
	err = x.err(C.ah_parse_bool(x.c, C.int(offsetWidth), offsets, (*C.uint8_t)(data), (*C.uint8_t)(valid), C.int64_t(off), C.int64_t(n), (*C.uint8_t)(dstBits), &row))
	return int64(row), err
}

// FormatIntOffsets is the first half of the integer / boolean → String / LargeString cast (kernels/string_casts.go:444-579): the
// output's offsets (from 0) and the number of bytes the caller allocates for FormatIntData.  in arrow.BOOL: values is the data bitmap.
func (x *Context) FormatIntOffsets(in arrow.Type, values, valid unsafe.Pointer, off, n int64, offsetWidth int, dstOffsets unsafe.Pointer) (totalBytes int64, err error) {
	var total C.int64_t
	err = x.err(C.ah_format_int_offsets(x.c, C.int(in), values, (*C.uint8_t)(valid), C.int64_t(off), C.int64_t(n), C.int(offsetWidth), dstOffsets, &total))
	return int64(total), err
}

// FormatIntData writes the characters (strconv.FormatInt / FormatUint in base 10, "true" / "false") under FormatIntOffsets' offsets.
func (x *Context) FormatIntData(in arrow.Type, values, valid unsafe.Pointer, off, n int64, offsetWidth int, dstOffsets, dstData unsafe.Pointer) error {
	return x.err(C.ah_format_int_data(x.c, C.int(in), values, (*C.uint8_t)(valid), C.int64_t(off), C.int64_t(n), C.int(offsetWidth), dstOffsets, (*C.uint8_t)(dstData)))
}

// ValidateUTF8 mirrors validateUTF8Sequence (kernels/string_casts.go:39-87): utf8.Valid of every valid row; offsetWidth 0 is a
// FixedSizeBinary column of byteWidth bytes whose values buffer is data.  On arrow.ErrInvalid badRow is the FIRST offending valid row.
func (x *Context) ValidateUTF8(offsetWidth int, offsets, data unsafe.Pointer, byteWidth int, valid unsafe.Pointer, off, n int64) (badRow int64, err error) {
	var row C.int64_t
	err = x.err(C.ah_validate_utf8(x.c, C.int(offsetWidth), offsets, (*C.uint8_t)(data), C.int(byteWidth), (*C.uint8_t)(valid), C.int64_t(off), C.int64_t(n), &row))
	return int64(row), err
}

// FixedBinaryOffsets mirrors the offsets loop of CastFsbToBinary (kernels/string_casts.go:154-193): (off + i) · byteWidth.
func (x *Context) FixedBinaryOffsets(offsetWidth, byteWidth int, off, n int64, dstOffsets unsafe.Pointer) error {
	return x.err(C.ah_fixed_binary_offsets(x.c, C.int(offsetWidth), C.int(byteWidth), C.int64_t(off), C.int64_t(n), dstOffsets))
}
