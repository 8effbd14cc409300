// kernels.cc — the kernel library: one ExecFn per function family, each a thin adapter
// from exec.ArraySpan to a leaf of include/arrowhip.h, plus the Register* entry points.
//
// ≙ arrow/compute/internal/kernels/{helpers.go:193-236 (ScalarBinary), :284-380
//   (ScalarBinaryNotNull), scalar_arithmetic.go, scalar_comparisons.go:199-218,
//   scalar_boolean.go:67-347, vector_selection.go:449-520,1162-1192,
//   vector_hash.go:620-741} and arrow/compute/{arithmetic.go, scalar_compare.go,
//   scalar_bool.go:94-110, selection.go:42-114,618-650, vector_hash.go:61-100}.
#include <cmath>
#include "arrowhip_compute.h"
#include "like_program.h"


#include <algorithm>
#include <cstring>

namespace arrowhip {
namespace compute {

using exec::ArraySpan;
using exec::ExecResult;
using exec::ExecSpan;
using exec::KernelCtx;

static const Type kNumericTypes[] = {Type::UINT8, Type::INT8,  Type::UINT16, Type::INT16,   Type::UINT32,
                                     Type::INT32, Type::UINT64, Type::INT64, Type::FLOAT32, Type::FLOAT64};

// exec.GetSpanValues (exec/utils.go:38-45): values pointer with the span offset applied
static inline const uint8_t* Values(const ArraySpan& a) { return a.buffers[1].buf + a.offset * (a.type->bit_width / 8); }
static inline uint8_t* Values(ArraySpan* a) { return a->buffers[1].buf + a->offset * (a->type->bit_width / 8); }

// Where the bytes of a base-binary or fixed-width array are, as the kernels' descriptors (ah_cmp_operand, ah_set_chunk,
// ah_sort_key, ah_hash_*_encode) take them: String / Binary / LargeString / LargeBinary have offset_width 4 or 8, offsets in
// buffer 1 and bytes in buffer 2; FixedSizeBinary / Decimal have byte_width-byte slots in buffer 1.
struct ByteLayout {
  int offset_width = 0, byte_width = 0;
  const void* offsets = nullptr;
  const uint8_t* data = nullptr;
  int64_t offset = 0;
};
static ByteLayout LayoutOf(const DataType* t, const void* b1, const void* b2, int64_t offset) {
  ByteLayout l;
  l.offset = offset;
  if (IsBaseBinary(t->id)) {
    l.offset_width = t->bit_width / 8;
    l.offsets = b1;
    l.data = (const uint8_t*)b2;
  } else {
    l.byte_width = t->bit_width / 8;
    l.data = (const uint8_t*)b1;
  }
  return l;
}
static ByteLayout LayoutOf(const ArraySpan& a) { return LayoutOf(a.type, a.buffers[1].buf, a.buffers[2].buf, a.offset); }
static ByteLayout LayoutOf(const ArrayData& a) {
  auto dptr = [&](int i) -> const void* { return a.buffers[i] ? a.buffers[i]->dptr : nullptr; };
  return LayoutOf(a.type, dptr(1), dptr(2), a.offset);
}

static int ShapeOf(const ExecSpan& b) {
  if (b.values[0].IsArray()) return b.values[1].IsArray() ? AH_SHAPE_AA : AH_SHAPE_AS;
  return AH_SHAPE_SA;
}

// ---- arithmetic ---------------------------------------------------------------------------
struct ArithData { int op; bool checked; };

// ScalarBinary (helpers.go:193-236) over the unchecked SIMD leaves
static Status ExecArithUnchecked(KernelCtx* k, const ExecSpan& b, ExecResult* out, int op) {
  Session* s = k->session;
  int type = (int)out->type->id;
  int shape = ShapeOf(b);
  if (out->len == 0) return Status::OK();
  switch (shape) {
    case AH_SHAPE_AA:
      return s->FromStatus(ah_arithmetic_binary(s->ctx(), type, (int8_t)op, Values(b.values[0].array), Values(b.values[1].array), Values(out), out->len));
    case AH_SHAPE_AS:
      return s->FromStatus(ah_arithmetic_arr_scalar(s->ctx(), type, (int8_t)op, Values(b.values[0].array), b.values[1].scalar->value, Values(out), out->len));
    default:
      return s->FromStatus(ah_arithmetic_scalar_arr(s->ctx(), type, (int8_t)op, b.values[0].scalar->value, Values(b.values[1].array), Values(out), out->len));
  }
}

// The operands of a binary (or, with one value, unary) call as the validity-aware leaves take them: values pointer, validity
// bitmap and offset of an array; value pointer and validity of a scalar.
struct BinaryOperands {
  const void* p[2] = {nullptr, nullptr};
  const uint8_t* valid[2] = {nullptr, nullptr};
  int64_t off[2] = {0, 0};
  int scalar_valid = 1, shape = AH_SHAPE_AS;
  // skip_clean_bitmaps: no bitmap for an array that cannot have nulls
  BinaryOperands(const ExecSpan& b, bool skip_clean_bitmaps) {
    if (b.values.size() == 2) shape = ShapeOf(b);
    for (size_t i = 0; i < b.values.size() && i < 2; i++) {
      const auto& v = b.values[i];
      if (v.IsArray()) {
        p[i] = Values(v.array);
        valid[i] = skip_clean_bitmaps && !v.array.MayHaveNulls() ? nullptr : v.array.buffers[0].buf;
        off[i] = v.array.offset;
      } else {
        p[i] = v.scalar->value;
        scalar_valid = v.scalar->valid;
      }
    }
  }
};

// ScalarBinaryNotNull (helpers.go:284-380) for the checked integer ops
static Status ExecArithChecked(KernelCtx* k, const ExecSpan& b, ExecResult* out, int op) {
  Session* s = k->session;
  if (IsFloating(out->type->id)) return ExecArithUnchecked(k, b, out, op);  // base_arithmetic_amd64.go:109-117
  if (out->len == 0) return Status::OK();
  const BinaryOperands o(b, /*skip_clean_bitmaps=*/false);
  return s->FromStatus(ah_arithmetic_checked(s->ctx(), (int)out->type->id, (int8_t)op, o.shape, o.p[0], o.valid[0], o.off[0], o.p[1], o.valid[1], o.off[1], o.scalar_valid,
                                             Values(out), out->len));
}

// Go's math.Pow10 (src/math/pow10.go): a product of two table entries — pow10tab[n % 32] · pow10postab32[n / 32] — which
// is what InitRoundState hands the round kernel (rounding.go:86-90); beyond 1e31 it is NOT always the correctly rounded
// literal, so it is restated rather than replaced by pow()
static double GoPow10(int64_t n) {
  static const double tab[32] = {1e00, 1e01, 1e02, 1e03, 1e04, 1e05, 1e06, 1e07, 1e08, 1e09, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15,
                                 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22, 1e23, 1e24, 1e25, 1e26, 1e27, 1e28, 1e29, 1e30, 1e31};
  static const double pos32[10] = {1e00, 1e32, 1e64, 1e96, 1e128, 1e160, 1e192, 1e224, 1e256, 1e288};
  if (n < 0) return 0;
  if (n > 308) return HUGE_VAL;
  return pos32[n / 32] * tab[n % 32];
}

// ScalarBinaryNotNull / ScalarUnaryNotNull / whole-buffer closures of the pure-Go arithmetic kernels: divide, abs, negate,
// bit-wise, shifts, sqrt (base_arithmetic.go:154-160,287-340,386-426; scalar_arithmetic.go:170-378)
static Status ExecArithExt(KernelCtx* k, const ExecSpan& b, ExecResult* out, int op) {
  Session* s = k->session;
  if (out->len == 0) return Status::OK();
  const BinaryOperands o(b, /*skip_clean_bitmaps=*/true);
  return s->FromStatus(ah_arithmetic_ext(s->ctx(), (int)out->type->id, op, o.shape, o.p[0], o.valid[0], o.off[0], o.p[1], o.valid[1], o.off[1], o.scalar_valid, Values(out),
                                         out->len));
}

static std::shared_ptr<ScalarFunction> MakeArithExt(const std::string& name, int op, int nargs, std::initializer_list<Type> types) {
  auto fn = std::make_shared<ScalarFunction>(name, Arity{nargs, false});
  for (Type t : types) {
    exec::ScalarKernel k;
    k.sig.in_types = nargs == 2 ? std::vector<Type>{t, t} : std::vector<Type>{t};
    k.sig.out_is_first_input = true;
    k.exec_fn = [op](KernelCtx* c, const ExecSpan& b, ExecResult* o) { return ExecArithExt(c, b, o, op); };
    fn->AddKernel(std::move(k));
  }
  fn->promote_numeric = true;  // arithmeticFunction.DispatchBest (arithmetic.go:112-142)
  return fn;
}

static Status ExecUnary(KernelCtx* k, const ExecSpan& b, ExecResult* out, int op) {
  Session* s = k->session;
  if (out->len == 0) return Status::OK();
  return s->FromStatus(ah_arithmetic_unary(s->ctx(), (int)out->type->id, (int8_t)op, Values(b.values[0].array), Values(out), out->len));
}

static std::shared_ptr<ScalarFunction> MakeArith(const std::string& name, int op, bool checked) {
  auto fn = std::make_shared<ScalarFunction>(name, Arity{2, false});
  for (Type t : kNumericTypes) {
    exec::ScalarKernel k;
    k.sig.in_types = {t, t};
    k.sig.out_is_first_input = true;
    k.exec_fn = checked ? exec::ArrayKernelExec([op](KernelCtx* c, const ExecSpan& b, ExecResult* o) { return ExecArithChecked(c, b, o, op); })
                        : exec::ArrayKernelExec([op](KernelCtx* c, const ExecSpan& b, ExecResult* o) { return ExecArithUnchecked(c, b, o, op); });
    fn->AddKernel(std::move(k));
  }
  fn->promote_numeric = true;  // arithmeticFunction.DispatchBest (arithmetic.go:112-142)
  return fn;
}

void RegisterScalarArithmetic(FunctionRegistry* reg) {
  // compute/arithmetic.go: "add" / "subtract" / "multiply" are the CHECKED kernels (the
  // default of compute.Add, :1090-1104), "*_unchecked" the wrapping SIMD ones
  reg->AddFunction(MakeArith("add", AH_OP_ADD_CHECKED, true), false);
  reg->AddFunction(MakeArith("add_unchecked", AH_OP_ADD, false), false);
  reg->AddFunction(MakeArith("subtract", AH_OP_SUB_CHECKED, true), false);
  reg->AddFunction(MakeArith("subtract_unchecked", AH_OP_SUB, false), false);
  // … and under the names compute.Subtract itself calls: impl(ctx, "sub", …) + "_unchecked" with NoCheckOverflow (arithmetic.go:679-682, 1115-1117)
  reg->AddFunction(MakeArith("sub", AH_OP_SUB_CHECKED, true), false);
  reg->AddFunction(MakeArith("sub_unchecked", AH_OP_SUB, false), false);
  reg->AddFunction(MakeArith("multiply", AH_OP_MUL_CHECKED, true), false);
  reg->AddFunction(MakeArith("multiply_unchecked", AH_OP_MUL, false), false);
  // the pure-Go rest of the registry that is exact (arithmetic.go:784-785, 822-840, 855-856, 944-995)
  const auto ints = {Type::UINT8, Type::INT8, Type::UINT16, Type::INT16, Type::UINT32, Type::INT32, Type::UINT64, Type::INT64};
  const auto nums = {Type::UINT8, Type::INT8, Type::UINT16, Type::INT16, Type::UINT32, Type::INT32, Type::UINT64, Type::INT64, Type::FLOAT32, Type::FLOAT64};
  const auto sgn = {Type::INT8, Type::INT16, Type::INT32, Type::INT64, Type::FLOAT32, Type::FLOAT64};
  const auto flt = {Type::FLOAT32, Type::FLOAT64};
  reg->AddFunction(MakeArithExt("divide", AH_OP_DIV_CHECKED, 2, nums), false);
  reg->AddFunction(MakeArithExt("divide_unchecked", AH_OP_DIV, 2, nums), false);
  reg->AddFunction(MakeArithExt("power", AH_OP_POWER_CHECKED, 2, nums), false);             // arithmetic.go:929-930
  reg->AddFunction(MakeArithExt("power_unchecked", AH_OP_POWER, 2, nums), false);
  reg->AddFunction(MakeArithExt("abs", AH_OP_ABS_CHECKED, 1, nums), false);
  reg->AddFunction(MakeArithExt("negate", AH_OP_NEGATE_CHECKED, 1, sgn), false);  // GetArithmeticUnarySignedKernels: no unsigned kernel
  reg->AddFunction(MakeArithExt("bit_wise_and", AH_OP_BIT_AND, 2, ints), false);
  reg->AddFunction(MakeArithExt("bit_wise_or", AH_OP_BIT_OR, 2, ints), false);
  reg->AddFunction(MakeArithExt("bit_wise_xor", AH_OP_BIT_XOR, 2, ints), false);
  reg->AddFunction(MakeArithExt("bit_wise_not", AH_OP_BIT_NOT, 1, ints), false);
  reg->AddFunction(MakeArithExt("shift_left", AH_OP_SHIFT_LEFT_CHECKED, 2, ints), false);
  reg->AddFunction(MakeArithExt("shift_left_unchecked", AH_OP_SHIFT_LEFT, 2, ints), false);
  reg->AddFunction(MakeArithExt("shift_right", AH_OP_SHIFT_RIGHT_CHECKED, 2, ints), false);
  reg->AddFunction(MakeArithExt("shift_right_unchecked", AH_OP_SHIFT_RIGHT, 2, ints), false);
  for (auto p : {std::make_pair("sqrt", AH_OP_SQRT_CHECKED), std::make_pair("sqrt_unchecked", AH_OP_SQRT)}) {
    auto fn = MakeArithExt(p.first, p.second, 1, flt);
    fn->promote_to_float = true;  // arithmeticFloatingPointFunc.DispatchBest (arithmetic.go:144-170): integers go to float64
    reg->AddFunction(fn, false);
  }
  for (auto p : {std::make_pair("floor", AH_OP_FLOOR), std::make_pair("ceil", AH_OP_CEIL), std::make_pair("trunc", AH_OP_TRUNC)}) {
    auto fn = MakeArithExt(p.first, p.second, 1, flt);  // GetSimpleRoundKernels (rounding.go:748-775)
    fn->promote_to_float = true;                         // arithmeticIntegerToFloatingPointFunc (arithmetic.go:172-200)
    reg->AddFunction(fn, false);
  }
  // round / round_to_multiple (arithmetic.go:1036-1056; kernels/rounding.go:321-370, 562-598)
  {
    static const RoundOptions kDefaultRound;                  // {NDigits: 0, Mode: RoundHalfToEven} (arithmetic.go:78)
    static const RoundToMultipleOptions kDefaultRoundMultiple = [] {  // Multiple: float64 1 (:79-80)
      RoundToMultipleOptions o;
      auto one = std::make_shared<Scalar>();
      one->type = GetDataType(Type::FLOAT64); one->valid = true;
      const double v = 1.0; memcpy(one->value, &v, 8);
      o.Multiple = one;
      return o;
    }();
    for (bool multiple : {false, true}) {
      auto fn = std::make_shared<ScalarFunction>(multiple ? "round_to_multiple" : "round", Arity{1, false});
      fn->SetDefaultOptions(multiple ? (const FunctionOptions*)&kDefaultRoundMultiple : (const FunctionOptions*)&kDefaultRound);
      for (Type t : flt) {
        exec::ScalarKernel k;
        k.sig.in_types = {t};
        k.sig.out_is_first_input = true;
        k.exec_fn = [multiple](KernelCtx* c, const ExecSpan& b, ExecResult* out) -> Status {
          Session* s = c->session;
          const ArraySpan& in = b.values[0].array;
          const uint8_t* valid = in.MayHaveNulls() ? in.buffers[0].buf : nullptr;
          const int type = (int)out->type->id;
          if (!multiple) {
            const RoundOptions* o = dynamic_cast<const RoundOptions*>(static_cast<const FunctionOptions*>(c->state));
            if (!o) return Status::Make(StatusCode::Invalid, "attempted to initialize kernel state from invalid function options");  // InitRoundState
            if (out->len == 0) return Status::OK();
            const int64_t ad = o->NDigits < 0 ? -o->NDigits : o->NDigits;
            return s->FromStatus(ah_round(s->ctx(), type, Values(in), valid, in.offset, out->len, o->NDigits, (int)o->Mode, nullptr, GoPow10(ad), Values(out)));
          }
          const RoundToMultipleOptions* o = dynamic_cast<const RoundToMultipleOptions*>(static_cast<const FunctionOptions*>(c->state));
          if (!o) return Status::Make(StatusCode::Invalid, "attempted to initialize kernel state from invalid function options");
          // InitRoundToMultipleState (rounding.go:127-177)
          if (!o->Multiple || !o->Multiple->valid) return Status::Make(StatusCode::Invalid, "rounding multiple must be non-null and valid");
          const Scalar& m = *o->Multiple;
          double mv = 0;
          bool positive = false;
          if (m.type->id == Type::FLOAT64) { memcpy(&mv, m.value, 8); positive = mv > 0; }
          else if (m.type->id == Type::FLOAT32) { float f; memcpy(&f, m.value, 4); mv = f; positive = f > 0; }
          else if (IsSignedInteger(m.type->id)) { long long x = 0; memcpy(&x, m.value, m.type->bit_width / 8); if (m.type->bit_width < 64) x = (x << (64 - m.type->bit_width)) >> (64 - m.type->bit_width); mv = (double)x; positive = x > 0; }
          else if (IsInteger(m.type->id)) { unsigned long long x = 0; memcpy(&x, m.value, m.type->bit_width / 8); mv = (double)x; positive = true; }  // isPositive: unsigned is always "positive"
          else return Status::Make(StatusCode::Invalid, "rounding multiple must be positive");
          if (!positive) return Status::Make(StatusCode::Invalid, "rounding multiple must be positive");
          // an integer multiple is cast to float64, a floating one to the input type (:157-175)
          uint8_t mbuf[8];
          if (type == AH_FLOAT32) { const float f = (float)mv; memcpy(mbuf, &f, 4); } else memcpy(mbuf, &mv, 8);
          if (out->len == 0) return Status::OK();
          return s->FromStatus(ah_round(s->ctx(), type, Values(in), valid, in.offset, out->len, 0, (int)o->Mode, mbuf, 1.0, Values(out)));
        };
        fn->AddKernel(std::move(k));
      }
      fn->promote_to_float = true;  // arithmeticIntegerToFloatingPointFunc
      reg->AddFunction(fn, false);
    }
  }
  struct U { const char* name; int op; };
  for (U u : {U{"abs_unchecked", AH_OP_ABS}, U{"negate_unchecked", AH_OP_NEGATE}, U{"sign", AH_OP_SIGN}}) {
    auto fn = std::make_shared<ScalarFunction>(u.name, Arity{1, false});
    for (Type t : kNumericTypes) {
      exec::ScalarKernel k;
      k.sig.in_types = {t};
      int op = u.op;
      k.exec_fn = [op](KernelCtx* c, const ExecSpan& b, ExecResult* o) { return ExecUnary(c, b, o, op); };
      fn->AddKernel(std::move(k));
    }
    reg->AddFunction(fn, false);
  }
}

// ---- comparisons --------------------------------------------------------------------------
// compareKernel[T] (scalar_comparisons.go:199-218): out bitmap starts at byte out.Offset/8,
// bit prefix out.Offset%8
static Status ExecCompare(KernelCtx* k, const ExecSpan& b, ExecResult* out, int cmpop) {
  Session* s = k->session;
  if (out->len == 0) return Status::OK();
  int shape = ShapeOf(b);
  const DataType* in_type = b.values[0].type();
  const void* l = b.values[0].IsArray() ? (const void*)Values(b.values[0].array) : (const void*)b.values[0].scalar->value;
  const void* r = b.values[1].IsArray() ? (const void*)Values(b.values[1].array) : (const void*)b.values[1].scalar->value;
  return s->FromStatus(ah_comparison(s->ctx(), cmpop, shape, (int)in_type->id, l, r, out->buffers[1].buf + out->offset / 8, out->len, (int)(out->offset % 8)));
}

static Status ExecBoolBinary(KernelCtx* k, const ExecSpan& b, ExecResult* out, int bitop);

// ---- comparisons of byte strings and decimals ----------------------------------------------------------------------------
// The kernels take their arguments uncast (ScalarKernel::consumes_uncast): the String ∘ Binary, LargeString ∘ FixedSizeBinary …
// pairings commonBinary resolves, and decimals of different scales or widths, are compared as they arrive.  A scalar operand
// becomes a length-1 device array read by every row (broadcast).

static std::string DecimalText(const DataType* t) {
  int p = 0, sc = 0;
  return DecimalParams(t, &p, &sc) ? std::string(t->name) + "(" + std::to_string(p) + ", " + std::to_string(sc) + ")" : std::string(t->name);
}

// one side of the call as a device array (a scalar: uploaded) + whether it is broadcast
static Status CompareSide(Session* s, const exec::ExecValue& v, ArrayDataPtr* keep, ByteLayout* l, int* bcast) {
  *bcast = v.IsScalar() ? 1 : 0;
  if (!v.IsScalar()) {
    *l = LayoutOf(v.array);
    return Status::OK();
  }
  AHC_RETURN_NOT_OK(ScalarToArray(s, *v.scalar, keep));
  *l = LayoutOf(**keep);
  return Status::OK();
}

// getBinaryCmp over NewVarBinaryIter / NewFSBIter (kernels/scalar_comparisons.go:520-540, 694-713).  NewFSBIter ignores the
// span's offset (exec/utils.go:266-277); here the offset is honoured, as for every other layout — DESIGN.md §4 quirk 10.
static Status ExecCompareBytes(KernelCtx* k, const ExecSpan& b, ExecResult* out, int cmpop) {
  Session* s = k->session;
  if (out->len == 0) return Status::OK();
  ah_cmp_operand o[2];
  ArrayDataPtr keep[2];
  for (int i = 0; i < 2; i++) {
    ByteLayout l;
    AHC_RETURN_NOT_OK(CompareSide(s, b.values[i], &keep[i], &l, &o[i].broadcast));
    o[i] = ah_cmp_operand{l.offset_width, l.byte_width, l.offsets, l.data, l.offset, o[i].broadcast};
  }
  return s->FromStatus(ah_compare_binary(s->ctx(), cmpop, &o[0], &o[1], out->len, out->buffers[1].buf, out->offset));
}

// genDecimalCompareKernel (kernels/scalar_comparisons.go:370-392) after castBinaryDecimalArgs: each side is rescaled in the
// kernel (value · 10^k, k = the larger scale − its scale), never cast.  An integer scalar becomes a decimal of scale 0 on the
// host, exactly; an integer array would need an integer → decimal cast, which this layer does not have.
static Status ExecCompareDecimal(KernelCtx* k, const ExecSpan& b, ExecResult* out, int cmpop) {
  Session* s = k->session;
  const DataType* t[2] = {b.values[0].type(), b.values[1].type()};
  Scalar as_dec[2];
  exec::ExecValue vals[2] = {b.values[0], b.values[1]};
  int prec, sc[2] = {0, 0};  // an integer side has scale 0
  for (int i = 0; i < 2; i++) {
    if (DecimalParams(t[i], &prec, &sc[i])) continue;
    const DataType* other = t[1 - i];
    if (!IsInteger(t[i]->id) || !vals[i].IsScalar())
      return Status::Make(StatusCode::NotImplemented, std::string("unsupported cast to ") + DecimalText(other) + " from " + t[i]->name);
    const Scalar& in = *vals[i].scalar;
    uint64_t u = 0;
    memcpy(&u, in.value, 8);
    const int bits = t[i]->bit_width;
    if (bits < 64) {
      u &= (1ull << bits) - 1;
      if (IsSignedInteger(t[i]->id) && (u >> (bits - 1)) & 1) u |= ~0ull << bits;  // sign-extend
    }
    const bool neg = IsSignedInteger(t[i]->id) && (int64_t)u < 0;
    as_dec[i].type = FixedWidthBinaryFromFormat("d:76,0,256");
    as_dec[i].valid = in.valid;
    as_dec[i].bytes.assign(32, neg ? 0xFF : 0x00);
    memcpy(as_dec[i].bytes.data(), &u, 8);
    vals[i].scalar = &as_dec[i];
    t[i] = as_dec[i].type;
  }
  if (out->len == 0) return Status::OK();
  const int target = std::max(sc[0], sc[1]);
  ByteLayout l[2];
  int bcast[2];
  ArrayDataPtr keep[2];
  for (int i = 0; i < 2; i++) AHC_RETURN_NOT_OK(CompareSide(s, vals[i], &keep[i], &l[i], &bcast[i]));
  return s->FromStatus(ah_compare_decimal(s->ctx(), cmpop, l[0].byte_width, l[0].data, l[0].offset, bcast[0], target - sc[0], l[1].byte_width, l[1].data,
                                          l[1].offset, bcast[1], target - sc[1], out->len, out->buffers[1].buf, out->offset));
}

void RegisterScalarComparisons(FunctionRegistry* reg) {
  struct C { const char* name; int op; };
  for (C c : {C{"equal", AH_CMP_EQ}, C{"not_equal", AH_CMP_NE}, C{"greater", AH_CMP_GT}, C{"greater_equal", AH_CMP_GE}}) {
    auto fn = std::make_shared<ScalarFunction>(c.name, Arity{2, false});
    if (c.op == AH_CMP_EQ || c.op == AH_CMP_NE) {
      // Boolean × Boolean, the first kernels of CompareKernels(CmpEQ / CmpNE) (kernels/scalar_comparisons.go:612-666: boolEQ / boolNE
      // over the data bitmaps, validity by NullIntersection): equal = XNOR, not_equal = XOR of the data bits
      exec::ScalarKernel k;
      k.sig.in_types = {Type::BOOL, Type::BOOL};
      k.sig.out_is_first_input = false;
      k.sig.out_type = Type::BOOL;
      const int bitop = c.op == AH_CMP_EQ ? AH_BIT_XNOR : AH_BIT_XOR;
      k.exec_fn = [bitop](KernelCtx* kc, const ExecSpan& b, ExecResult* o) { return ExecBoolBinary(kc, b, o, bitop); };
      fn->AddKernel(std::move(k));
    }
    for (Type t : kNumericTypes) {
      exec::ScalarKernel k;
      k.sig.in_types = {t, t};
      k.sig.out_is_first_input = false;
      k.sig.out_type = Type::BOOL;
      int op = c.op;
      k.exec_fn = [op](KernelCtx* kc, const ExecSpan& b, ExecResult* o) { return ExecCompare(kc, b, o, op); };
      fn->AddKernel(std::move(k));
    }
    // base-binary, decimal and FixedSizeBinary kernels (CompareKernels, kernels/scalar_comparisons.go:694-713): each matches its
    // own type id on both sides; the mixed pairings DispatchBest resolves reach them uncast
    for (Type t : {Type::STRING, Type::BINARY, Type::LARGE_STRING, Type::LARGE_BINARY, Type::DECIMAL128, Type::DECIMAL256,
                   Type::FIXED_SIZE_BINARY}) {
      exec::ScalarKernel k;
      k.sig.in_types = {t, t};
      k.sig.out_is_first_input = false;
      k.sig.out_type = Type::BOOL;
      k.consumes_uncast = true;
      int op = c.op;
      if (IsDecimal(t)) k.exec_fn = [op](KernelCtx* kc, const ExecSpan& b, ExecResult* o) { return ExecCompareDecimal(kc, b, o, op); };
      else k.exec_fn = [op](KernelCtx* kc, const ExecSpan& b, ExecResult* o) { return ExecCompareBytes(kc, b, o, op); };
      fn->AddKernel(std::move(k));
    }
    fn->promote_numeric = true;  // compareFunction.DispatchBest (scalar_compare.go:37-63)
    fn->promote_binary_decimal = true;
    reg->AddFunction(fn, false);
  }
  // scalar_compare.go:73-99: less / less_equal = flipped greater / greater_equal
  auto less = std::make_shared<ScalarFunction>("less", Arity{2, false});
  less->flipped_of = "greater";
  reg->AddFunction(less, false);
  auto le = std::make_shared<ScalarFunction>("less_equal", Arity{2, false});
  le->flipped_of = "greater_equal";
  reg->AddFunction(le, false);
  // is_null / is_not_null / is_nan (scalar_compare.go:138-160; kernels/scalar_comparisons.go:718-813)
  const std::vector<Type> any_types = {Type::BOOL, Type::UINT8, Type::INT8, Type::UINT16, Type::INT16, Type::UINT32, Type::INT32, Type::UINT64,
                                       Type::INT64, Type::FLOAT32, Type::FLOAT64, Type::STRING, Type::BINARY, Type::LARGE_STRING, Type::LARGE_BINARY};
  auto validity_fn = [&](const char* name, bool want_null) {
    auto fn = std::make_shared<ScalarFunction>(name, Arity{1, false});
    for (Type t : any_types) {
      exec::ScalarKernel k;
      k.sig.in_types = {t};
      k.sig.out_is_first_input = false;
      k.sig.out_type = Type::BOOL;
      k.null_handling = exec::NullHandling::NullComputedNoPrealloc;  // :753-758: the result is never null
      k.mem_alloc = exec::MemAlloc::MemNoPrealloc;
      k.exec_fn = [want_null](KernelCtx* c, const ExecSpan& b, ExecResult* out) -> Status {
        // isNullExec: the inverted validity, or zeros when there is none (:718-730).  isNotNullExec: the validity itself
        // (:732-745) — the reference shares the buffer WITHOUT carrying the input offset, which mis-reads sliced arrays;
        // here the bits are copied from the offset (equal wherever the reference is right)
        Session* s = c->session;
        const ArraySpan& in = b.values[0].array;
        BufferPtr bits;
        AHC_RETURN_NOT_OK(c->AllocateBitmap(in.len, &bits));
        out->nulls = 0;
        out->buffers[1].WrapBuffer(bits);
        if (in.len == 0) return Status::OK();
        AHC_RETURN_NOT_OK(s->FromStatus(ah_memset_async(s->ctx(), bits->dptr, 0, (size_t)((in.len + 7) / 8))));
        if (in.buffers[0].buf)
          return s->FromStatus(ah_copy_bitmap(s->ctx(), in.buffers[0].buf, in.offset, in.len, (uint8_t*)bits->dptr, 0, want_null ? 1 : 0));
        return want_null ? Status::OK() : s->FromStatus(ah_set_bits_to(s->ctx(), (uint8_t*)bits->dptr, 0, in.len, 1));
      };
      fn->AddKernel(std::move(k));
    }
    reg->AddFunction(fn, false);
  };
  validity_fn("is_null", true);
  validity_fn("is_not_null", false);
  {
    auto fn = std::make_shared<ScalarFunction>("is_nan", Arity{1, false});
    for (Type t : kNumericTypes) {
      exec::ScalarKernel k;
      k.sig.in_types = {t};
      k.sig.out_is_first_input = false;
      k.sig.out_type = Type::BOOL;
      k.null_handling = exec::NullHandling::NullNoOutput;  // :788,792,800
      k.exec_fn = [](KernelCtx* c, const ExecSpan& b, ExecResult* out) -> Status {
        Session* s = c->session;
        if (out->len == 0) return Status::OK();
        const ArraySpan& in = b.values[0].array;
        uint8_t* ob = out->buffers[1].buf + out->offset / 8;
        if (IsFloating(in.type->id))  // isNanKernelExec: x != x over every slot (:770-780)
          return s->FromStatus(ah_comparison(s->ctx(), AH_CMP_NE, AH_SHAPE_AA, (int)in.type->id, Values(in), Values(in), ob, out->len, (int)(out->offset % 8)));
        return s->FromStatus(ah_set_bits_to(s->ctx(), out->buffers[1].buf, out->offset, out->len, 0));  // ConstBoolExec(false) :763-768
      };
      fn->AddKernel(std::move(k));
    }
    reg->AddFunction(fn, false);
  }

}

// ---- boolean --------------------------------------------------------------------------------
// a boolean scalar operand is materialised as a constant bitmap (SetBitsTo) so every shape
// runs through the same bitmap kernels — scalar_boolean.go:75-88 does CopyBitmap/SetBitsTo too
static Status BoolOperand(KernelCtx* k, const exec::ExecValue& v, int64_t len, const uint8_t** data, int64_t* off, BufferPtr* keep) {
  if (v.IsArray()) { *data = v.array.buffers[1].buf; *off = v.array.offset; return Status::OK(); }
  AHC_RETURN_NOT_OK(k->AllocateBitmap(len, keep));
  if (v.scalar->value[0] & 1)
    AHC_RETURN_NOT_OK(k->session->FromStatus(ah_set_bits_to(k->session->ctx(), (uint8_t*)(*keep)->dptr, 0, len, 1)));
  *data = (const uint8_t*)(*keep)->dptr;
  *off = 0;
  return Status::OK();
}

static Status ExecBoolBinary(KernelCtx* k, const ExecSpan& b, ExecResult* out, int bitop) {
  Session* s = k->session;
  if (out->len == 0) return Status::OK();
  const uint8_t *l, *r; int64_t lo, ro; BufferPtr kl, kr;
  AHC_RETURN_NOT_OK(BoolOperand(k, b.values[0], out->len, &l, &lo, &kl));
  AHC_RETURN_NOT_OK(BoolOperand(k, b.values[1], out->len, &r, &ro, &kr));
  AHC_RETURN_NOT_OK(s->FromStatus(ah_bitmap_op(s->ctx(), bitop, l, lo, r, ro, out->buffers[1].buf, out->offset, out->len)));
  if (kl || kr) AHC_RETURN_NOT_OK(s->FromStatus(ah_sync(s->ctx())));  // temporaries die with this frame
  return Status::OK();
}

static Status ExecKleene(KernelCtx* k, const ExecSpan& b, ExecResult* out, int op) {
  Session* s = k->session;
  if (out->len == 0) return Status::OK();
  const uint8_t *ld, *rd, *lv = nullptr, *rv = nullptr; int64_t lo, ro; BufferPtr kl, kr, klv, krv;
  AHC_RETURN_NOT_OK(BoolOperand(k, b.values[0], out->len, &ld, &lo, &kl));
  AHC_RETURN_NOT_OK(BoolOperand(k, b.values[1], out->len, &rd, &ro, &kr));
  if (b.values[0].IsArray()) lv = b.values[0].array.buffers[0].buf;
  else if (!b.values[0].scalar->valid) { AHC_RETURN_NOT_OK(k->AllocateBitmap(out->len, &klv)); lv = (const uint8_t*)klv->dptr; }
  if (b.values[1].IsArray()) rv = b.values[1].array.buffers[0].buf;
  else if (!b.values[1].scalar->valid) { AHC_RETURN_NOT_OK(k->AllocateBitmap(out->len, &krv)); rv = (const uint8_t*)krv->dptr; }
  // validity bitmaps share the data offset of their array (ArraySpan.Offset)
  AHC_RETURN_NOT_OK(s->FromStatus(ah_kleene(s->ctx(), op, lv, ld, lo, rv, rd, ro, out->buffers[0].buf, out->buffers[1].buf, out->offset, out->len)));
  out->nulls = kUnknownNullCount;
  if (kl || kr || klv || krv) AHC_RETURN_NOT_OK(s->FromStatus(ah_sync(s->ctx())));
  return Status::OK();
}

void RegisterScalarBoolean(FunctionRegistry* reg) {
  struct B { const char* name; int op; };
  for (B bo : {B{"and", AH_BIT_AND}, B{"or", AH_BIT_OR}, B{"xor", AH_BIT_XOR}, B{"and_not", AH_BIT_AND_NOT}}) {
    auto fn = std::make_shared<ScalarFunction>(bo.name, Arity{2, false});
    exec::ScalarKernel k;
    k.sig.in_types = {Type::BOOL, Type::BOOL};
    int op = bo.op;
    k.exec_fn = [op](KernelCtx* kc, const ExecSpan& b, ExecResult* o) { return ExecBoolBinary(kc, b, o, op); };
    fn->AddKernel(std::move(k));
    reg->AddFunction(fn, false);
  }
  for (B bo : {B{"and_kleene", AH_KLEENE_AND}, B{"or_kleene", AH_KLEENE_OR}, B{"and_not_kleene", AH_KLEENE_AND_NOT}}) {
    auto fn = std::make_shared<ScalarFunction>(bo.name, Arity{2, false});
    exec::ScalarKernel k;
    k.sig.in_types = {Type::BOOL, Type::BOOL};
    k.null_handling = exec::NullHandling::NullComputedPrealloc;  // scalar_bool.go:101-109
    int op = bo.op;
    k.exec_fn = [op](KernelCtx* kc, const ExecSpan& b, ExecResult* o) { return ExecKleene(kc, b, o, op); };
    fn->AddKernel(std::move(k));
    reg->AddFunction(fn, false);
  }
  auto inv = std::make_shared<ScalarFunction>("invert", Arity{1, false});
  exec::ScalarKernel k;
  k.sig.in_types = {Type::BOOL};
  k.exec_fn = [](KernelCtx* kc, const ExecSpan& b, ExecResult* o) {
    if (o->len == 0) return Status::OK();
    const ArraySpan& a = b.values[0].array;  // NotExecKernel (scalar_boolean.go:334-347)
    return kc->session->FromStatus(ah_copy_bitmap(kc->session->ctx(), a.buffers[1].buf, a.offset, a.len, o->buffers[1].buf, o->offset, 1));
  };
  inv->AddKernel(std::move(k));
  reg->AddFunction(inv, false);
}

// ---- selection --------------------------------------------------------------------------------
// PrimitiveFilter (vector_selection.go:449-520)
static Status ExecFilter(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  Session* s = k->session;
  ArraySpan values = b.values[0].array, filter = b.values[1].array;
  const FilterOptions* opts = static_cast<const FilterOptions*>(k->state);
  int null_sel = opts ? (int)opts->NullSelection : DropNulls;
  AHC_RETURN_NOT_OK(values.UpdateNullCount(s));
  AHC_RETURN_NOT_OK(filter.UpdateNullCount(s));
  const uint8_t* fvalid = filter.MayHaveNulls() ? filter.buffers[0].buf : nullptr;
  if (opts && opts->WorstCaseOutput && values.len > 0 && values.type->bit_width >= 8) {
    // ONE call (ah_filter_primitive_once): the output is sized for the input's length, the kernel counts and fills back to back and the
    // host hears the selection count once, at the end — the reference's count → allocate → fill costs a host language two calls and a
    // turnaround between two launches (0.318 against ≈ 0.29 ms for 2^27 rows at s = 0.5)
    const int w = values.type->bit_width / 8;
    out->nulls = (values.nulls == 0 && (null_sel == DropNulls || filter.nulls == 0)) ? 0 : kUnknownNullCount;
    const bool allocate_validity = values.nulls != 0 || filter.nulls != 0;
    BufferPtr vb, db;
    if (allocate_validity) { AHC_RETURN_NOT_OK(k->AllocateBitmap(values.len, &vb)); out->buffers[0].WrapBuffer(vb); }
    AHC_RETURN_NOT_OK(k->Allocate(values.len * w, &db, /*zero_all=*/false));
    out->buffers[1].WrapBuffer(db);
    int64_t n_sel = 0, nulls = 0;
    const uint8_t* vvalid = values.MayHaveNulls() ? values.buffers[0].buf : nullptr;
    AHC_RETURN_NOT_OK(s->FromStatus(ah_filter_primitive_once(s->ctx(), w, Values(values), vvalid, values.offset, filter.buffers[1].buf, fvalid, filter.offset,
                                                             values.len, null_sel, db->dptr, allocate_validity ? (uint8_t*)vb->dptr : nullptr, &n_sel, &nulls)));
    out->len = n_sel;
    if (allocate_validity) out->nulls = nulls;
    return Status::OK();
  }
  int64_t n_out = 0;
  if (values.len > 0)  // getFilterOutputSize :57-81
    AHC_RETURN_NOT_OK(s->FromStatus(ah_filter_count(s->ctx(), filter.buffers[1].buf, fvalid, filter.offset, filter.len, null_sel, &n_out)));
  // :464-468
  out->nulls = (values.nulls == 0 && (null_sel == DropNulls || filter.nulls == 0)) ? 0 : kUnknownNullCount;
  bool allocate_validity = values.nulls != 0 || filter.nulls != 0;  // :486-488
  int w = values.type->bit_width / 8;
  if (values.type->bit_width == 1)
    return Status::Make(StatusCode::NotImplemented, "boolean-valued filter is outside the accelerated path");
  out->len = n_out;  // preallocateData :83-93
  BufferPtr vb, db;
  if (allocate_validity) { AHC_RETURN_NOT_OK(k->AllocateBitmap(n_out, &vb)); out->buffers[0].WrapBuffer(vb); }
  AHC_RETURN_NOT_OK(k->Allocate(n_out * w, &db, /*zero_all=*/false));
  out->buffers[1].WrapBuffer(db);
  if (values.len == 0) return Status::OK();
  int64_t nulls = 0;
  const uint8_t* vvalid = values.MayHaveNulls() ? values.buffers[0].buf : nullptr;
  AHC_RETURN_NOT_OK(s->FromStatus(ah_filter_primitive(s->ctx(), w, Values(values), vvalid, values.offset, filter.buffers[1].buf, fvalid,
                                                      filter.offset, values.len, null_sel, n_out, db->dptr,
                                                      allocate_validity ? (uint8_t*)vb->dptr : nullptr, allocate_validity ? &nulls : nullptr)));
  if (allocate_validity) out->nulls = nulls;
  return Status::OK();
}

// An index operand of a Take: the indices of an array, or the selection vector a filter turned into.
struct IndexOperand {
  int width = 4;
  bool is_signed = false;
  const void* data = nullptr;
  const uint8_t* valid = nullptr;   // null: no null slots
  int64_t offset = 0, len = 0, nulls = 0;
  BufferPtr data_buf, valid_buf;    // (a filter's indices: their owner)
};
static IndexOperand IndexOperandOf(const ArraySpan& indices) {   // null count known (UpdateNullCount)
  IndexOperand ix;
  ix.width = indices.type->bit_width / 8;
  ix.is_signed = IsSignedInteger(indices.type->id);
  ix.data = Values(indices);
  ix.valid = indices.MayHaveNulls() ? indices.buffers[0].buf : nullptr;
  ix.offset = indices.offset;
  ix.len = indices.len;
  ix.nulls = indices.nulls;
  return ix;
}
// GetTakeIndices (vector_selection.go:102-236): the filter's first `rows` slots as uint32 selection indices, null slots (EmitNulls)
// with their validity.  A filter of `limit` rows or more is refused with the caller's words (:229-235).
static Status FilterToIndices(Session* s, ArraySpan& filter, int64_t rows, const FilterOptions* opts, int64_t limit, const char* too_long,
                              IndexOperand* ix) {
  const int null_sel = opts ? (int)opts->NullSelection : DropNulls;
  AHC_RETURN_NOT_OK(filter.UpdateNullCount(s));
  if (rows >= limit) return Status::Make(StatusCode::NotImplemented, too_long);
  const uint8_t* fvalid = filter.MayHaveNulls() ? filter.buffers[0].buf : nullptr;
  if (rows > 0)
    AHC_RETURN_NOT_OK(s->FromStatus(ah_filter_count(s->ctx(), filter.buffers[1].buf, fvalid, filter.offset, filter.len, null_sel, &ix->len)));
  AHC_RETURN_NOT_OK(s->Allocate(ix->len * 4, &ix->data_buf));
  AHC_RETURN_NOT_OK(s->AllocateBitmap(ix->len, &ix->valid_buf));
  if (ix->len > 0)
    AHC_RETURN_NOT_OK(s->FromStatus(ah_filter_to_indices(s->ctx(), filter.buffers[1].buf, fvalid, filter.offset, rows, null_sel, ix->len,
                                                         (uint32_t*)ix->data_buf->dptr, (uint8_t*)ix->valid_buf->dptr, &ix->nulls)));
  ix->data = ix->data_buf->dptr;
  ix->valid = ix->nulls ? (const uint8_t*)ix->valid_buf->dptr : nullptr;
  return Status::OK();
}

// PrimitiveTake (vector_selection.go:1162-1192)
static Status TakeFixedCommon(KernelCtx* k, const ArraySpan& values, const IndexOperand& ix, bool allocate_validity, int bounds_check, ExecResult* out) {
  Session* s = k->session;
  const int w = values.type->bit_width / 8;
  out->len = ix.len;
  BufferPtr vb, db;
  if (allocate_validity) { AHC_RETURN_NOT_OK(k->AllocateBitmap(ix.len, &vb)); out->buffers[0].WrapBuffer(vb); }
  AHC_RETURN_NOT_OK(k->Allocate(ix.len * w, &db, /*zero_all=*/false));
  out->buffers[1].WrapBuffer(db);
  out->nulls = 0;
  if (ix.len == 0) return Status::OK();
  int64_t nulls = 0, bad = 0;
  AHC_RETURN_NOT_OK(s->FromStatus(ah_take_primitive(
      s->ctx(), w, values.buffers[1].buf ? Values(values) : nullptr, values.MayHaveNulls() ? values.buffers[0].buf : nullptr, values.offset,
      values.len, ix.width, ix.is_signed ? 1 : 0, ix.data, ix.valid, ix.offset, ix.len, bounds_check, db->dptr,
      allocate_validity ? (uint8_t*)vb->dptr : nullptr, &nulls, &bad)));
  out->nulls = allocate_validity ? nulls : 0;
  return Status::OK();
}
static Status ExecTake(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  ArraySpan values = b.values[0].array, indices = b.values[1].array;
  const TakeOptions* opts = static_cast<const TakeOptions*>(k->state);
  AHC_RETURN_NOT_OK(values.UpdateNullCount(k->session));
  AHC_RETURN_NOT_OK(indices.UpdateNullCount(k->session));
  if (values.type->bit_width == 1)
    return Status::Make(StatusCode::NotImplemented, "boolean-valued take is outside the accelerated path");
  return TakeFixedCommon(k, values, IndexOperandOf(indices), values.nulls != 0 || indices.nulls != 0 /* :1176 */, opts ? (int)opts->BoundsCheck : 1, out);
}

// FSBImpl (vector_selection.go:1997-2031; registered for FIXED_SIZE_BINARY, DECIMAL128 and DECIMAL256 at :2344-2346 / :2354-2356):
// fixed-width values of any byte width are one slot per row.  The device take moves slots of 1, 2, 4, 8, 16 or 32 bytes (the two
// decimals, UUID-sized and hash-sized binaries) with one access each and any other width byte by byte (the reference's own test
// column is binary(3)); beyond 4096 bytes a slot is refused.
static Status CheckSlotWidth(const ArraySpan& values) {
  const int w = values.type->bit_width / 8;
  if (w >= 1 && w <= 4096) return Status::OK();
  return Status::Make(StatusCode::NotImplemented, "selection of fixed-size binary values: byte widths 1 … 4096, not " + std::to_string(w));
}
static Status ExecTakeFixed(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  AHC_RETURN_NOT_OK(CheckSlotWidth(b.values[0].array));
  return ExecTake(k, b, out);
}
// the filter of wide slots goes through GetTakeIndices (vector_selection.go:102-236) and the take, like the binary and boolean
// filters here: ah_filter_primitive's compaction is built for slots of at most 8 bytes
static Status ExecFilterFixed(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  ArraySpan values = b.values[0].array, filter = b.values[1].array;
  AHC_RETURN_NOT_OK(CheckSlotWidth(values));
  const int w = values.type->bit_width / 8;
  if (w == 1 || w == 2 || w == 4 || w == 8) return ExecFilter(k, b, out);
  AHC_RETURN_NOT_OK(values.UpdateNullCount(k->session));
  IndexOperand ix;
  AHC_RETURN_NOT_OK(FilterToIndices(k->session, filter, values.len, static_cast<const FilterOptions*>(k->state), (int64_t)1 << 32,
                                    "filter of a fixed-size binary column with 2^32 rows or more", &ix));
  return TakeFixedCommon(k, values, ix, values.nulls != 0 || filter.nulls != 0, /*bounds_check=*/0, out);
}

// dictionaryTake / dictionaryFilter (compute/selection.go:497-586): select the INDICES (int32 on the device), keep a pointer
// to the same dictionary
static void CarryDictionary(const ArraySpan& in, ExecResult* out) {
  out->dictionary = in.dictionary;
  out->dict_value_type = in.dict_value_type;
  out->dict_index_type = in.dict_index_type;
}
static Status ExecTakeDictionary(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  AHC_RETURN_NOT_OK(ExecTake(k, b, out));
  CarryDictionary(b.values[0].array, out);
  return Status::OK();
}
static Status ExecFilterDictionary(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  AHC_RETURN_NOT_OK(ExecFilter(k, b, out));
  CarryDictionary(b.values[0].array, out);
  return Status::OK();
}

// VarBinaryImpl (vector_selection.go:1925-1992) under takeExec: offsets + validity + byte count, then the bytes
static Status TakeBinaryCommon(KernelCtx* k, const ArraySpan& values, const IndexOperand& ix, bool allocate_validity, ExecResult* out) {
  Session* s = k->session;
  const int ow = values.type->bit_width / 8;
  out->len = ix.len;
  BufferPtr vb, ob, db;
  if (allocate_validity) { AHC_RETURN_NOT_OK(k->AllocateBitmap(ix.len, &vb)); out->buffers[0].WrapBuffer(vb); }
  AHC_RETURN_NOT_OK(k->Allocate((ix.len + 1) * ow, &ob));
  out->buffers[1].WrapBuffer(ob);
  int64_t nulls = 0, total = 0, bad = 0;
  AHC_RETURN_NOT_OK(s->FromStatus(ah_take_binary_offsets(s->ctx(), ow, values.buffers[1].buf, values.MayHaveNulls() ? values.buffers[0].buf : nullptr,
                                                         values.offset, values.len, ix.width, ix.is_signed, ix.data, ix.valid, ix.offset, ix.len, 1, ob->dptr,
                                                         allocate_validity ? (uint8_t*)vb->dptr : nullptr, &nulls, &total, &bad)));
  AHC_RETURN_NOT_OK(k->Allocate(total, &db, /*zero_all=*/false));
  out->buffers[2].WrapBuffer(db);
  if (ix.len > 0)
    AHC_RETURN_NOT_OK(s->FromStatus(ah_take_binary_data(s->ctx(), ow, values.buffers[1].buf, values.buffers[2].buf, values.offset, ix.width, ix.data, ix.len,
                                                        ob->dptr, (uint8_t*)db->dptr)));
  out->nulls = allocate_validity ? nulls : 0;
  return Status::OK();
}

static Status ExecTakeBinary(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  ArraySpan values = b.values[0].array, indices = b.values[1].array;
  AHC_RETURN_NOT_OK(values.UpdateNullCount(k->session));
  AHC_RETURN_NOT_OK(indices.UpdateNullCount(k->session));
  return TakeBinaryCommon(k, values, IndexOperandOf(indices), values.nulls != 0 || indices.nulls != 0, out);
}

// binaryFilterImpl (vector_selection.go:1650-1815) = GetTakeIndices (:102-236) + the var-length take
static Status ExecFilterBinary(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  ArraySpan values = b.values[0].array, filter = b.values[1].array;
  AHC_RETURN_NOT_OK(values.UpdateNullCount(k->session));
  IndexOperand ix;
  AHC_RETURN_NOT_OK(FilterToIndices(k->session, filter, values.len, static_cast<const FilterOptions*>(k->state), (int64_t)1 << 32,
                                    "filter of a binary column with 2^32 rows or more", &ix));
  return TakeBinaryCommon(k, values, ix, values.nulls != 0 || filter.nulls != 0, out);
}

// booleanTakeImpl (vector_selection.go:990-1074) and, for filter, GetTakeIndices in front of it
static Status TakeBooleanCommon(KernelCtx* k, const ArraySpan& values, const IndexOperand& ix, bool allocate_validity, ExecResult* out) {
  Session* s = k->session;
  out->len = ix.len;
  BufferPtr vb, db;
  if (allocate_validity) { AHC_RETURN_NOT_OK(k->AllocateBitmap(ix.len, &vb)); out->buffers[0].WrapBuffer(vb); }
  AHC_RETURN_NOT_OK(k->AllocateBitmap(ix.len, &db));
  out->buffers[1].WrapBuffer(db);
  int64_t nulls = 0, bad = 0;
  AHC_RETURN_NOT_OK(s->FromStatus(ah_take_boolean(s->ctx(), values.buffers[1].buf, values.MayHaveNulls() ? values.buffers[0].buf : nullptr, values.offset,
                                                  values.len, ix.width, ix.is_signed, ix.data, ix.valid, ix.offset, ix.len, 1, (uint8_t*)db->dptr,
                                                  allocate_validity ? (uint8_t*)vb->dptr : nullptr, &nulls, &bad)));
  out->nulls = allocate_validity ? nulls : 0;
  return Status::OK();
}

static Status ExecTakeBoolean(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  ArraySpan values = b.values[0].array, indices = b.values[1].array;
  AHC_RETURN_NOT_OK(values.UpdateNullCount(k->session));
  AHC_RETURN_NOT_OK(indices.UpdateNullCount(k->session));
  return TakeBooleanCommon(k, values, IndexOperandOf(indices), values.nulls != 0 || indices.nulls != 0, out);
}

static Status ExecFilterBoolean(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  ArraySpan values = b.values[0].array, filter = b.values[1].array;
  AHC_RETURN_NOT_OK(values.UpdateNullCount(k->session));
  IndexOperand ix;
  AHC_RETURN_NOT_OK(FilterToIndices(k->session, filter, values.len, static_cast<const FilterOptions*>(k->state), (int64_t)1 << 32,
                                    "filter of a boolean column with 2^32 rows or more", &ix));
  return TakeBooleanCommon(k, values, ix, values.nulls != 0 || filter.nulls != 0, out);
}

static const Type kBinaryTypes[] = {Type::STRING, Type::BINARY, Type::LARGE_STRING, Type::LARGE_BINARY};

static const FilterOptions kDefaultFilterOptions;
static const TakeOptions kDefaultTakeOptions;
static const DictionaryEncodeOptions kDefaultDictOptions;

// FilterRecordBatch (compute/selection.go:679-722): the mask becomes ONE index vector (GetTakeIndices,
// kernels/vector_selection.go:102-236) and every column is gathered with it, bounds check off
static Status FilterRecordBatch(ExecCtx* ctx, const Datum& batch, const ArrayData& filter_in, const FilterOptions* opts, Datum* out) {
  Session* s = ctx->session;
  if (batch.num_rows != filter_in.length) return Status::Make(StatusCode::Invalid, "filter inputs must all be the same length");
  exec::ArraySpan filter;
  filter.SetMembers(filter_in);
  IndexOperand ix;
  AHC_RETURN_NOT_OK(FilterToIndices(s, filter, filter.len, opts, ((int64_t)1 << 32) - 1,
                                    "filter length exceeds UINT32_MAX, consider a different strategy for selecting elements", &ix));
  const int64_t n_out = ix.len;
  auto idx = std::make_shared<ArrayData>();
  idx->type = GetDataType(Type::UINT32);
  idx->length = n_out;
  idx->buffers[1] = ix.data_buf;
  idx->null_count = ix.nulls;
  if (ix.nulls) idx->buffers[0] = ix.valid_buf;
  static const TakeOptions kNoBoundsCheck = [] { TakeOptions t; t.BoundsCheck = false; return t; }();
  std::vector<ArrayDataPtr> cols;
  for (auto& c : batch.chunks) {
    Datum col;
    AHC_RETURN_NOT_OK(CallFunction(ctx, "array_take", &kNoBoundsCheck, {Datum::Of(c), Datum::Of(idx)}, &col));
    cols.push_back(col.array);
  }
  *out = Datum::OfRecord(batch.names, std::move(cols), n_out);
  return Status::OK();
}

void RegisterVectorSelection(FunctionRegistry* reg) {
  static const Type kIndexTypes[] = {Type::INT8, Type::UINT8, Type::INT16, Type::UINT16, Type::INT32, Type::UINT32, Type::INT64, Type::UINT64};
  static const Type kBool[] = {Type::BOOL}, kDictionary[] = {Type::DICTIONARY};
  static const Type kFixedSlotTypes[] = {Type::FIXED_SIZE_BINARY, Type::DECIMAL128, Type::DECIMAL256};
  // one kernel per (value type, second type) pair, value-major
  auto add = [](VectorFunction* fn, const auto& values, const auto& seconds, exec::ArrayKernelExec exec_fn, bool chunkwise) {
    for (Type t : values)
      for (Type t2 : seconds) {
        exec::VectorKernel k;
        k.sig.in_types = {t, t2};
        k.exec_fn = exec_fn;
        k.can_execute_chunkwise = chunkwise;
        fn->AddKernel(std::move(k));
      }
  };
  auto af = std::make_shared<VectorFunction>("array_filter", Arity{2, false}, &kDefaultFilterOptions);
  af->chunked = VectorFunction::Chunked::Filter;
  add(af.get(), kNumericTypes, kBool, ExecFilter, true);
  add(af.get(), kDictionary, kBool, ExecFilterDictionary, true);
  add(af.get(), kBinaryTypes, kBool, ExecFilterBinary, true);
  add(af.get(), kBool, kBool, ExecFilterBoolean, true);
  add(af.get(), kFixedSlotTypes, kBool, ExecFilterFixed, true);   // vector_selection.go:2344-2346
  reg->AddFunction(af, false);
  auto at = std::make_shared<VectorFunction>("array_take", Arity{2, false}, &kDefaultTakeOptions);
  at->chunked = VectorFunction::Chunked::Take;
  // (not chunkwise: selection.go:639)
  add(at.get(), kNumericTypes, kIndexTypes, ExecTake, false);
  add(at.get(), kDictionary, kIndexTypes, ExecTakeDictionary, false);
  add(at.get(), kBool, kIndexTypes, ExecTakeBoolean, false);
  add(at.get(), kFixedSlotTypes, kIndexTypes, ExecTakeFixed, false);   // vector_selection.go:2354-2356
  add(at.get(), kBinaryTypes, kIndexTypes, ExecTakeBinary, false);
  reg->AddFunction(at, false);
  // filterMetaFunc (selection.go:42-85): validates, then dispatches on the values kind
  reg->AddFunction(std::make_shared<MetaFunction>("filter", Arity{2, false}, &kDefaultFilterOptions,
      [](ExecCtx* ctx, const FunctionOptions* o, const std::vector<Datum>& args, Datum* out) {
        if (!args[1].type() || args[1].type()->id != Type::BOOL)
          return Status::Make(StatusCode::NotImplemented, "filter argument must be boolean type");  // :45-48
        if (args[0].kind == DatumKind::Record) {
          if (args[1].kind != DatumKind::Array)
            return Status::Make(StatusCode::NotImplemented, "record batch filtering only implemented for Array filter");  // :69
          return FilterRecordBatch(ctx, args[0], *args[1].array, static_cast<const FilterOptions*>(o), out);
        }
        if (args[0].kind == DatumKind::Array && args[1].kind == DatumKind::Array && args[0].Len() != args[1].Len())
          return Status::Make(StatusCode::Invalid, "filter inputs must all be the same length");  // FilterArray check
        return CallFunction(ctx, "array_filter", o, args, out);
      }), false);
  // takeMetaFunc (selection.go:93-114)
  reg->AddFunction(std::make_shared<MetaFunction>("take", Arity{2, false}, &kDefaultTakeOptions,
      [](ExecCtx* ctx, const FunctionOptions* o, const std::vector<Datum>& args, Datum* out) {
        if (!args[1].type() || !IsInteger(args[1].type()->id))
          return Status::Make(StatusCode::NotImplemented, "take indices must be an integer type");
        if (args[0].kind == DatumKind::Record) {  // takeRecordImpl (selection.go:160-204): every column through array_take with the same indices
          Datum indices = args[1];
          if (indices.kind == DatumKind::Chunked) {
            if (indices.chunks.empty()) return Status::Make(StatusCode::Invalid, "Must pass at least one array");  // concat.go:43-45
            ArrayDataPtr whole;
            AHC_RETURN_NOT_OK(Concatenate(ctx->session, indices.chunks, indices.chunked_type, &whole));
            indices = Datum::Of(whole);
          }
          std::vector<ArrayDataPtr> cols;
          for (auto& c : args[0].chunks) {
            Datum col;
            AHC_RETURN_NOT_OK(CallFunction(ctx, "array_take", o, {Datum::Of(c), indices}, &col));
            cols.push_back(col.array);
          }
          *out = Datum::OfRecord(args[0].names, std::move(cols), indices.Len());
          return Status::OK();
        }
        return CallFunction(ctx, "array_take", o, args, out);
      }), false);
}

// ---- hashing -----------------------------------------------------------------------------------
// The common end of unique / dictionary_encode.  `d` is the dictionary (GetDictArrayData, arrow/array/util.go:321-390): its
// type, length and value buffers are set; if the memo table holds a null (null_id ≥ 0), its validity is all ones with that
// bit cleared (memory.Set(…, 0xFF), util.go:375-384).  unique returns the dictionary itself (uniqueFinalize,
// vector_hash.go:721-741); dictionary_encode returns the ids with `d` attached (dictionaryEncodeAction.Flush :188-209).
static Status FinishHash(KernelCtx* k, const ArraySpan& keys, const ArrayDataPtr& d, int32_t null_id, bool dict_encode, const BufferPtr& ids,
                         const BufferPtr& ids_valid, ExecResult* out) {
  Session* s = k->session;
  d->null_count = null_id >= 0 ? 1 : 0;
  if (null_id >= 0) {
    BufferPtr dv;
    AHC_RETURN_NOT_OK(k->AllocateBitmap(d->length, &dv));
    AHC_RETURN_NOT_OK(s->FromStatus(ah_memset_async(s->ctx(), dv->dptr, 0xFF, (size_t)((d->length + 7) / 8))));
    AHC_RETURN_NOT_OK(s->FromStatus(ah_set_bits_to(s->ctx(), (uint8_t*)dv->dptr, null_id, 1, 0)));
    d->buffers[0] = dv;
  }
  if (!dict_encode) {
    out->type = d->type;
    out->len = d->length;
    out->nulls = d->null_count;
    for (int i = 0; i < 3; i++) out->buffers[i].WrapBuffer(d->buffers[i]);
    return Status::OK();
  }
  out->len = keys.len;
  out->nulls = ids_valid ? keys.nulls : 0;
  out->buffers[0].WrapBuffer(ids_valid);
  out->buffers[1].WrapBuffer(ids);
  out->dictionary = d;
  return Status::OK();
}

// regularHashState over Table[uint64] (vector_hash.go:243-286,359-385,604-607)
static Status ExecHash(KernelCtx* k, const ExecSpan& b, ExecResult* out, bool dict_encode) {
  Session* s = k->session;
  ArraySpan keys = b.values[0].array;
  // 1/2/4-byte keys: the reference memoises them in Table[uint8/16/32] keyed on the raw bits
  // (vector_hash.go:596-607); here the bits are zero-extended to 64 on the device, hashed in the same
  // table, and the dictionary is narrowed back — the ids and the first-seen order are unchanged
  // Boolean keys (doAppendBoolean, vector_hash.go:387-415: the bit becomes the uint8 key 0 / 1 of the same memo table): the bits
  // are widened on the device like the narrow integers, and the ≤ 3 dictionary entries go back to a bitmap through `!= 0`
  const bool is_bool = keys.type->id == Type::BOOL;
  const int kw = is_bool ? 1 : keys.type->bit_width / 8;
  const int raw_type = kw == 1 ? AH_UINT8 : kw == 2 ? AH_UINT16 : AH_UINT32;
  const DictionaryEncodeOptions* opts = static_cast<const DictionaryEncodeOptions*>(k->state);
  int encode_nulls = dict_encode ? (opts && opts->NullEncoding == NullEncodingEncode) : 1;  // uniqueAction.ShouldEncodeNulls() == true
  AHC_RETURN_NOT_OK(keys.UpdateNullCount(s));
  const uint8_t* valid = keys.MayHaveNulls() ? keys.buffers[0].buf : nullptr;
  int64_t n = keys.len;
  BufferPtr ids, ids_valid, dict;
  AHC_RETURN_NOT_OK(k->Allocate((n + 1) * 8, &dict));
  if (dict_encode) {
    AHC_RETURN_NOT_OK(k->Allocate(n * 4, &ids, /*zero_all=*/false));
    if (valid && !encode_nulls) AHC_RETURN_NOT_OK(k->AllocateBitmap(n, &ids_valid));
  }
  int64_t ndict = 0; int32_t null_id = -1;
  const uint64_t* keys64 = is_bool ? nullptr : (const uint64_t*)Values(keys);
  BufferPtr widened;
  if (kw < 8 && n > 0) {
    AHC_RETURN_NOT_OK(k->Allocate(n * 8, &widened, /*zero_all=*/false));
    if (is_bool) AHC_RETURN_NOT_OK(s->FromStatus(ah_cast_bool_to_numeric(s->ctx(), AH_UINT64, keys.buffers[1].buf, keys.offset, n, widened->dptr)));
    else AHC_RETURN_NOT_OK(s->FromStatus(ah_cast_numeric(s->ctx(), raw_type, AH_UINT64, Values(keys), nullptr, 0, n, 1, 1, widened->dptr)));
    keys64 = (const uint64_t*)widened->dptr;
  }
  if (n > 0)
    AHC_RETURN_NOT_OK(s->FromStatus(ah_hash_u64_encode(s->ctx(), keys64, valid, keys.offset, n, encode_nulls,
                                                       ids ? (int32_t*)ids->dptr : nullptr, ids_valid ? (uint8_t*)ids_valid->dptr : nullptr,
                                                       (uint64_t*)dict->dptr, &ndict, &null_id)));
  // GetDictArrayData (arrow/array/util.go:321-390): values by memo index
  auto d = std::make_shared<ArrayData>();
  d->type = keys.type;
  d->length = ndict;
  if (is_bool) {
    BufferPtr bits;
    AHC_RETURN_NOT_OK(k->AllocateBitmap(ndict, &bits));
    alignas(8) uint8_t zero[8] = {0};
    if (ndict > 0) AHC_RETURN_NOT_OK(s->FromStatus(ah_comparison(s->ctx(), AH_CMP_NE, AH_SHAPE_AS, AH_UINT64, dict->dptr, zero, (uint8_t*)bits->dptr, ndict, 0)));
    dict = bits;
  } else if (kw < 8) {
    BufferPtr narrow;
    AHC_RETURN_NOT_OK(k->Allocate(ndict * kw, &narrow, /*zero_all=*/false));
    if (ndict > 0)
      AHC_RETURN_NOT_OK(s->FromStatus(ah_cast_numeric(s->ctx(), AH_UINT64, raw_type, dict->dptr, nullptr, 0, ndict, 1, 1, narrow->dptr)));
    dict = narrow;
  }
  d->buffers[1] = dict;
  dict->size = is_bool ? (ndict + 7) / 8 : ndict * kw;
  return FinishHash(k, keys, d, null_id, dict_encode, ids, ids_valid, out);
}

// regularHashState over BinaryMemoTable (vector_hash.go:288-325,612-618): ids on the device, the dictionary
// = the var-length take of each entry's first row (the memo table's builder holds exactly those bytes)
static Status ExecHashBinary(KernelCtx* k, const ExecSpan& b, ExecResult* out, bool dict_encode) {
  Session* s = k->session;
  ArraySpan keys = b.values[0].array;
  const DictionaryEncodeOptions* opts = static_cast<const DictionaryEncodeOptions*>(k->state);
  int encode_nulls = dict_encode ? (opts && opts->NullEncoding == NullEncodingEncode) : 1;
  AHC_RETURN_NOT_OK(keys.UpdateNullCount(s));
  const uint8_t* valid = keys.MayHaveNulls() ? keys.buffers[0].buf : nullptr;
  const int64_t n = keys.len;
  const ByteLayout l = LayoutOf(keys);
  BufferPtr ids, ids_valid, first_rows;
  AHC_RETURN_NOT_OK(k->Allocate((n + 1) * 8, &first_rows));
  if (dict_encode) {
    AHC_RETURN_NOT_OK(k->Allocate(n * 4, &ids, /*zero_all=*/false));
    if (valid && !encode_nulls) AHC_RETURN_NOT_OK(k->AllocateBitmap(n, &ids_valid));
  }
  int64_t ndict = 0; int32_t null_id = -1;
  if (n > 0)
    AHC_RETURN_NOT_OK(s->FromStatus(ah_hash_binary_encode(s->ctx(), l.offset_width, l.offsets, l.data, valid, l.offset, n, encode_nulls,
                                                          ids ? (int32_t*)ids->dptr : nullptr, ids_valid ? (uint8_t*)ids_valid->dptr : nullptr,
                                                          (int64_t*)first_rows->dptr, &ndict, &null_id)));
  // GetDictArrayData (arrow/array/util.go:341-366): offsets + values in memo order, a null entry has no bytes
  ExecResult dres;
  dres.type = keys.type;
  IndexOperand rows;   // int64 first-occurrence rows, no nulls
  rows.width = 8; rows.is_signed = true; rows.data = first_rows->dptr; rows.len = ndict;
  AHC_RETURN_NOT_OK(TakeBinaryCommon(k, keys, rows, false, &dres));
  auto d = std::make_shared<ArrayData>();
  d->type = keys.type;
  d->length = ndict;
  d->buffers[1] = dres.buffers[1].owner;
  d->buffers[2] = dres.buffers[2].owner;
  return FinishHash(k, keys, d, null_id, dict_encode, ids, ids_valid, out);
}

// FixedSizeBinary / Decimal128 / Decimal256 keys (vector_hash.go:608-609, 698: the BinaryMemoTable over values of one byte width):
// ah_hash_fixed_encode — ids, index validity, null id as for the var-length keys; the dictionary comes back as ndict values
static Status ExecHashFixed(KernelCtx* k, const ExecSpan& b, ExecResult* out, bool dict_encode) {
  Session* s = k->session;
  ArraySpan keys = b.values[0].array;
  const DictionaryEncodeOptions* opts = static_cast<const DictionaryEncodeOptions*>(k->state);
  int encode_nulls = dict_encode ? (opts && opts->NullEncoding == NullEncodingEncode) : 1;
  AHC_RETURN_NOT_OK(keys.UpdateNullCount(s));
  const uint8_t* valid = keys.MayHaveNulls() ? keys.buffers[0].buf : nullptr;
  const int64_t n = keys.len;
  const ByteLayout l = LayoutOf(keys);
  const int w = l.byte_width;
  if (w <= 0) return Status::Make(StatusCode::Invalid, "fixed-size binary keys need a byte width");
  BufferPtr ids, ids_valid, first_rows, dict;
  AHC_RETURN_NOT_OK(k->Allocate((n + 1) * 8, &first_rows));
  AHC_RETURN_NOT_OK(k->Allocate((n + 1) * w, &dict));   // at most n + 1 entries; handed on as the dictionary's value buffer
  if (dict_encode) {
    AHC_RETURN_NOT_OK(k->Allocate(n * 4, &ids, /*zero_all=*/false));
    if (valid && !encode_nulls) AHC_RETURN_NOT_OK(k->AllocateBitmap(n, &ids_valid));
  }
  int64_t ndict = 0; int32_t null_id = -1;
  if (n > 0)
    AHC_RETURN_NOT_OK(s->FromStatus(ah_hash_fixed_encode(s->ctx(), w, l.data, valid, l.offset, n, encode_nulls, ids ? (int32_t*)ids->dptr : nullptr,
                                                         ids_valid ? (uint8_t*)ids_valid->dptr : nullptr, (int64_t*)first_rows->dptr, (uint8_t*)dict->dptr,
                                                         &ndict, &null_id)));
  auto d = std::make_shared<ArrayData>();
  d->type = keys.type;
  d->length = ndict;
  d->buffers[1] = dict;
  return FinishHash(k, keys, d, null_id, dict_encode, ids, ids_valid, out);
}

void RegisterVectorHash(FunctionRegistry* reg) {
  auto uq = std::make_shared<VectorFunction>("unique", Arity{1, false});
  uq->chunked = VectorFunction::Chunked::SingleArray;
  auto de = std::make_shared<VectorFunction>("dictionary_encode", Arity{1, false}, &kDefaultDictOptions);
  std::vector<Type> fixed(std::begin(kNumericTypes), std::end(kNumericTypes));
  fixed.push_back(Type::BOOL);
  for (Type t : fixed) {
    exec::VectorKernel ku;
    ku.sig.in_types = {t};
    ku.exec_fn = [](KernelCtx* k, const ExecSpan& b, ExecResult* o) { return ExecHash(k, b, o, false); };
    uq->AddKernel(std::move(ku));
    exec::VectorKernel kd;
    kd.sig.in_types = {t};
    kd.output_is_dictionary = true;
    kd.exec_fn = [](KernelCtx* k, const ExecSpan& b, ExecResult* o) { return ExecHash(k, b, o, true); };
    de->AddKernel(std::move(kd));
  }
  for (Type t : {Type::FIXED_SIZE_BINARY, Type::DECIMAL128, Type::DECIMAL256}) {
    exec::VectorKernel ku;
    ku.sig.in_types = {t};
    ku.exec_fn = [](KernelCtx* k, const ExecSpan& b, ExecResult* o) { return ExecHashFixed(k, b, o, false); };
    uq->AddKernel(std::move(ku));
    exec::VectorKernel kd;
    kd.sig.in_types = {t};
    kd.output_is_dictionary = true;
    kd.exec_fn = [](KernelCtx* k, const ExecSpan& b, ExecResult* o) { return ExecHashFixed(k, b, o, true); };
    de->AddKernel(std::move(kd));
  }
  for (Type t : {Type::BINARY, Type::STRING, Type::LARGE_BINARY, Type::LARGE_STRING}) {
    exec::VectorKernel ku;
    ku.sig.in_types = {t};
    ku.exec_fn = [](KernelCtx* k, const ExecSpan& b, ExecResult* o) { return ExecHashBinary(k, b, o, false); };
    uq->AddKernel(std::move(ku));
    exec::VectorKernel kd;
    kd.sig.in_types = {t};
    kd.output_is_dictionary = true;
    kd.exec_fn = [](KernelCtx* k, const ExecSpan& b, ExecResult* o) { return ExecHashBinary(k, b, o, true); };
    de->AddKernel(std::move(kd));
  }
  {
    // dictionaryHashState (vector_hash.go:505-576, uniqueFinalizeDictionary :757-775): the distinct INDICES in first-seen
    // order, as a dictionary array over the same dictionary; dictionary_encode of a dictionary array is the identity (:473-478)
    exec::VectorKernel ku;
    ku.sig.in_types = {Type::DICTIONARY};
    ku.exec_fn = [](KernelCtx* k, const ExecSpan& b, ExecResult* o) {
      AHC_RETURN_NOT_OK(ExecHash(k, b, o, false));
      CarryDictionary(b.values[0].array, o);
      return Status::OK();
    };
    uq->AddKernel(std::move(ku));
    exec::VectorKernel kd;
    kd.sig.in_types = {Type::DICTIONARY};
    kd.exec_fn = [](KernelCtx*, const ExecSpan& b, ExecResult* o) {
      *o = b.values[0].array;
      return Status::OK();
    };
    de->AddKernel(std::move(kd));
  }
  reg->AddFunction(uq, false);
  reg->AddFunction(de, false);
}

// ---- cast (numeric ↔ numeric, bool ↔ numeric, decimal ↔ decimal, integer ↔ decimal, string ↔ integer / boolean / binary) ----
// CastIntToInt / CastFloatingToInteger / CastIntegerToFloating / CastFloatingToFloating
// (kernels/numeric_cast.go:37-71): conversion and safe-cast check in one pass on the device
static Status ExecCastNumeric(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  Session* s = k->session;
  if (out->len == 0) return Status::OK();
  const CastOptions* opts = static_cast<const CastOptions*>(k->state);
  const ArraySpan& in = b.values[0].array;
  return s->FromStatus(ah_cast_numeric(s->ctx(), (int)in.type->id, (int)out->type->id, Values(in), in.MayHaveNulls() ? in.buffers[0].buf : nullptr,
                                       in.offset, in.len, opts && opts->AllowIntOverflow, opts && opts->AllowFloatTruncate, Values(out)));
}
// boolToNum (numeric_cast.go:555-569)
static Status ExecCastBoolToNumeric(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  Session* s = k->session;
  if (out->len == 0) return Status::OK();
  const ArraySpan& in = b.values[0].array;
  return s->FromStatus(ah_cast_bool_to_numeric(s->ctx(), (int)out->type->id, in.buffers[1].buf, in.offset, in.len, Values(out)));
}
// isNonZero (boolean_cast.go:30-36): v != 0 — the array∘scalar "not_equal" kernel
static Status ExecCastNumericToBool(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  Session* s = k->session;
  if (out->len == 0) return Status::OK();
  const ArraySpan& in = b.values[0].array;
  alignas(8) uint8_t zero[8] = {0};
  return s->FromStatus(ah_comparison(s->ctx(), AH_CMP_NE, AH_SHAPE_AS, (int)in.type->id, Values(in), zero, out->buffers[1].buf + out->offset / 8,
                                     out->len, (int)(out->offset % 8)));
}

// ---- decimal casts (kernels/numeric_cast.go:79-429) ------------------------------------------------------------------------
// precision and scale of a decimal cast target, checked against the width
static Status CastTargetDecimal(const DataType* t, int* precision, int* scale) {
  if (!DecimalParams(t, precision, scale)) return Status::Make(StatusCode::Invalid, std::string("cast: not a decimal type: ") + t->name);
  const int max_p = t->id == Type::DECIMAL128 ? 38 : 76;
  if (*precision < 1 || *precision > max_p)
    return Status::Make(StatusCode::Invalid, "Decimal precision out of range [1, " + std::to_string(max_p) + "]: " + std::to_string(*precision));
  return Status::OK();
}

// CastDecimalToDecimal (numeric_cast.go:377-429): rescale by the difference of the scales, then the precision check — or, with
// AllowDecimalTruncate, truncate / wrap and check nothing.  Negative scales: refused, as in CastBinaryDecimalArgs.
static Status ExecCastDecimalToDecimal(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  Session* s = k->session;
  const CastOptions* opts = static_cast<const CastOptions*>(k->state);
  const ArraySpan& in = b.values[0].array;
  int in_p = 0, in_s = 0, out_p = 0, out_s = 0;
  if (!DecimalParams(in.type, &in_p, &in_s)) return Status::Make(StatusCode::Invalid, "cast: decimal input without precision and scale");
  AHC_RETURN_NOT_OK(CastTargetDecimal(out->type, &out_p, &out_s));
  if (in_s < 0 || out_s < 0) return Status::Make(StatusCode::NotImplemented, "decimals with negative scales not supported");
  if (out->len == 0) return Status::OK();
  return s->FromStatus(ah_cast_decimal_rescale(s->ctx(), in.type->bit_width / 8, out->type->bit_width / 8, out_s - in_s, out_p,
                                               opts && opts->AllowDecimalTruncate, Values(in), in.MayHaveNulls() ? in.buffers[0].buf : nullptr, in.offset,
                                               in.len, Values(out)));
}

// CastIntegerToDecimal (numeric_cast.go:207-239): the scale and precision checks are made from the types, before any row is read
static Status ExecCastIntegerToDecimal(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  Session* s = k->session;
  const ArraySpan& in = b.values[0].array;
  int out_p = 0, out_s = 0;
  AHC_RETURN_NOT_OK(CastTargetDecimal(out->type, &out_p, &out_s));
  if (out_s < 0) return Status::Make(StatusCode::Invalid, "scale must be non-negative");
  const int min_precision = MaxDecimalDigitsForInt(in.type->id) + out_s;
  if (out_p < min_precision)
    return Status::Make(StatusCode::Invalid, "precision is not great enough for result. It should be at least " + std::to_string(min_precision));
  if (out->len == 0) return Status::OK();
  return s->FromStatus(ah_cast_int_to_decimal(s->ctx(), (int)in.type->id, out->type->bit_width / 8, out_s, Values(in),
                                              in.MayHaveNulls() ? in.buffers[0].buf : nullptr, in.offset, in.len, Values(out)));
}

// CastDecimal128ToInteger / CastDecimal256ToInteger (numeric_cast.go:91-171)
static Status ExecCastDecimalToInteger(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  Session* s = k->session;
  const CastOptions* opts = static_cast<const CastOptions*>(k->state);
  const ArraySpan& in = b.values[0].array;
  int in_p = 0, in_s = 0;
  if (!DecimalParams(in.type, &in_p, &in_s)) return Status::Make(StatusCode::Invalid, "cast: decimal input without precision and scale");
  if (out->len == 0) return Status::OK();
  return s->FromStatus(ah_cast_decimal_to_int(s->ctx(), in.type->bit_width / 8, in_s, (int)out->type->id, opts && opts->AllowDecimalTruncate,
                                              opts && opts->AllowIntOverflow, Values(in), in.MayHaveNulls() ? in.buffers[0].buf : nullptr, in.offset,
                                              in.len, Values(out)));
}

// ---- string casts (kernels/string_casts.go, numeric_cast.go:742-781, boolean_cast.go:77-95) --------------------------------
// DataType.String() as the reference's messages print it
static std::string CastTypeText(const DataType* t) {
  if (t->id == Type::FIXED_SIZE_BINARY) return "fixed_size_binary[" + std::to_string(t->bit_width / 8) + "]";
  return t->name;
}
static bool IsStringType(Type id) { return id == Type::STRING || id == Type::LARGE_STRING; }

// the bytes of row `row` of a byte-string or fixed-size binary column, on the host (the one row an error message quotes)
static Status DownloadRow(Session* s, const ArraySpan& in, int64_t row, std::string* bytes) {
  bytes->clear();
  int64_t begin = 0, len = 0;
  const uint8_t* data = nullptr;
  if (IsBaseBinary(in.type->id)) {
    const int ow = in.type->bit_width / 8;
    alignas(8) uint8_t raw[16] = {0};
    AHC_RETURN_NOT_OK(s->FromStatus(ah_download_async(s->ctx(), raw, in.buffers[1].buf + (in.offset + row) * ow, (size_t)(2 * ow))));
    AHC_RETURN_NOT_OK(s->FromStatus(ah_sync(s->ctx())));
    if (ow == 4) { int32_t o[2]; memcpy(o, raw, 8); begin = o[0]; len = (int64_t)o[1] - o[0]; }
    else { int64_t o[2]; memcpy(o, raw, 16); begin = o[0]; len = o[1] - o[0]; }
    data = in.buffers[2].buf;
  } else {
    len = in.type->bit_width / 8;
    begin = (in.offset + row) * len;
    data = in.buffers[1].buf;
  }
  if (len <= 0) return Status::OK();
  bytes->resize((size_t)len);
  AHC_RETURN_NOT_OK(s->FromStatus(ah_download_async(s->ctx(), &(*bytes)[0], data + begin, (size_t)len)));
  return s->FromStatus(ah_sync(s->ctx()));
}

// strconv.Quote for the bytes of a NumError: \" \\ \n \t \r, \xNN for every other byte outside printable ASCII
static std::string GoQuote(const std::string& b) {
  std::string q = "\"";
  char hex[8];
  for (unsigned char c : b) {
    if (c == '"' || c == '\\') { q += '\\'; q += (char)c; }
    else if (c == '\n') q += "\\n";
    else if (c == '\t') q += "\\t";
    else if (c == '\r') q += "\\r";
    else if (c >= 0x20 && c < 0x7F) q += (char)c;
    else { snprintf(hex, sizeof hex, "\\x%02x", c); q += hex; }
  }
  return q + "\"";
}

// the reference's error of a parse kernel: fmt.Errorf("%w: %s", arrow.ErrInvalid, &strconv.NumError{Func, Num, Err})
static Status ParseError(Session* s, const ArraySpan& in, const char* func, int64_t row, int kind) {
  std::string bytes;
  AHC_RETURN_NOT_OK(DownloadRow(s, in, row, &bytes));
  return Status::Make(StatusCode::Invalid, std::string("strconv.") + func + ": parsing " + GoQuote(bytes) + ": " +
                                               (kind == 2 ? "value out of range" : "invalid syntax"));
}

// getParseStringExec (numeric_cast.go:742-781): String / Binary / LargeString / LargeBinary → the eight integer types
static Status ExecCastStringToInteger(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  Session* s = k->session;
  if (out->len == 0) return Status::OK();
  const ArraySpan& in = b.values[0].array;
  int64_t bad = -1;
  int kind = 0;
  const int rc = ah_parse_int(s->ctx(), in.type->bit_width / 8, in.buffers[1].buf, in.buffers[2].buf, in.MayHaveNulls() ? in.buffers[0].buf : nullptr,
                              in.offset, in.len, (int)out->type->id, Values(out), &bad, &kind);
  if (rc == AH_EINVALID && bad >= 0) return ParseError(s, in, IsSignedInteger(out->type->id) ? "ParseInt" : "ParseUint", bad, kind);
  return s->FromStatus(rc);
}

// strconv.ParseBool under ScalarUnaryNotNullBinaryArgBoolOut (boolean_cast.go:77-95)
static Status ExecCastStringToBool(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  Session* s = k->session;
  if (out->len == 0) return Status::OK();
  const ArraySpan& in = b.values[0].array;
  int64_t bad = -1;
  const int rc = ah_parse_bool(s->ctx(), in.type->bit_width / 8, in.buffers[1].buf, in.buffers[2].buf, in.MayHaveNulls() ? in.buffers[0].buf : nullptr,
                               in.offset, in.len, out->buffers[1].buf, &bad);
  if (rc == AH_EINVALID && bad >= 0) return ParseError(s, in, "ParseBool", bad, 1);
  return s->FromStatus(rc);
}

// maxFormattedBytes (string_casts.go:429-442)
static int MaxFormattedBytes(Type id) {
  switch (id) {
    case Type::INT8: case Type::UINT8: return 4;
    case Type::INT16: return 6;
    case Type::UINT16: return 5;
    case Type::INT32: return 11;
    case Type::UINT32: return 10;
    case Type::INT64: case Type::UINT64: return 20;
    default: return 0;
  }
}
static Status PayloadTooLarge(int64_t total) {
  return Status::Make(StatusCode::Invalid, "formatted cast payload (" + std::to_string(total) + " bytes) exceeds single data buffer limit (" +
                                               std::to_string((int64_t)INT32_MAX) + " bytes) for destination builder");
}

// integer / boolean → String / LargeString (string_casts.go:444-579): the validity is the executor's (NullIntersection); offsets,
// the byte total, the allocation, the characters
static Status ExecCastIntegerToString(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  Session* s = k->session;
  ArraySpan in = b.values[0].array;
  const int ow = out->type->bit_width / 8;
  const bool is_bool = in.type->id == Type::BOOL;
  if (!is_bool && ow == 4) {  // reserveFormattedData: the reference refuses by its UPPER bound, before it formats a row
    AHC_RETURN_NOT_OK(in.UpdateNullCount(s));
    const int64_t reserve = (in.len - in.nulls) * (int64_t)MaxFormattedBytes(in.type->id);
    if (reserve > (int64_t)INT32_MAX) return PayloadTooLarge(reserve);
  }
  BufferPtr ob, db;
  AHC_RETURN_NOT_OK(k->Allocate((out->len + 1) * ow, &ob, /*zero_all=*/false));
  out->buffers[1].WrapBuffer(ob);
  const uint8_t* values = is_bool ? in.buffers[1].buf : Values(in);
  const uint8_t* valid = in.MayHaveNulls() ? in.buffers[0].buf : nullptr;
  int64_t total = 0;
  const int rc = ah_format_int_offsets(s->ctx(), (int)in.type->id, values, valid, in.offset, in.len, ow, ob->dptr, &total);
  if (rc == AH_EINVALID && total > (int64_t)INT32_MAX) return PayloadTooLarge(total);   // boolean input: the exact count
  AHC_RETURN_NOT_OK(s->FromStatus(rc));
  AHC_RETURN_NOT_OK(k->Allocate(total, &db, /*zero_all=*/false));
  out->buffers[2].WrapBuffer(db);
  if (in.len == 0 || total == 0) return Status::OK();
  return s->FromStatus(ah_format_int_data(s->ctx(), (int)in.type->id, values, valid, in.offset, in.len, ow, ob->dptr, (uint8_t*)db->dptr));
}

// shouldValidateUTF8 + validateUtf8 / validateUtf8Fsb (string_casts.go:39-87)
static Status ValidateUtf8ForCast(KernelCtx* k, const ArraySpan& in, const DataType* to) {
  const CastOptions* opts = static_cast<const CastOptions*>(k->state);
  if ((opts && opts->AllowInvalidUtf8) || !IsStringType(to->id) || IsStringType(in.type->id) || in.len == 0) return Status::OK();
  Session* s = k->session;
  const ByteLayout l = LayoutOf(in);
  int64_t bad = -1;
  const int rc = ah_validate_utf8(s->ctx(), l.offset_width, l.offsets, l.data, l.byte_width, in.MayHaveNulls() ? in.buffers[0].buf : nullptr, in.offset,
                                  in.len, &bad);
  if (rc == AH_EINVALID && bad >= 0) {
    std::string bytes, hex;
    AHC_RETURN_NOT_OK(DownloadRow(s, in, bad, &bytes));
    char h[4];
    for (unsigned char c : bytes) { snprintf(h, sizeof h, "%02x", c); hex += h; }
    return Status::Make(StatusCode::Invalid, "invalid UTF8 bytes: " + hex);
  }
  return s->FromStatus(rc);
}

static Status InputTooLarge(const DataType* from, const DataType* to) {
  return Status::Make(StatusCode::Invalid, "failed casting from " + CastTypeText(from) + " to " + CastTypeText(to) + ": input array too large");
}

// CastBinaryToBinary (string_casts.go:89-152): the same offset width shares every buffer; another one shares validity's content and
// the data and widens or narrows the offsets
static Status ExecCastBinaryToBinary(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  Session* s = k->session;
  const ArraySpan& in = b.values[0].array;
  const DataType* to = out->type;
  AHC_RETURN_NOT_OK(ValidateUtf8ForCast(k, in, to));
  const int iw = in.type->bit_width / 8, ow = to->bit_width / 8;
  if (iw == ow) {  // ZeroCopyCastExec
    *out = in;
    out->type = to;
    return Status::OK();
  }
  if (ow == 4 && in.len > 0) {  // the last offset must fit
    int64_t last = 0;
    AHC_RETURN_NOT_OK(s->FromStatus(ah_download_async(s->ctx(), &last, in.buffers[1].buf + (in.offset + in.len) * 8, 8)));
    AHC_RETURN_NOT_OK(s->FromStatus(ah_sync(s->ctx())));
    if (last > (int64_t)INT32_MAX) return InputTooLarge(in.type, to);
  }
  BufferPtr ob;
  AHC_RETURN_NOT_OK(k->Allocate((in.len + 1) * ow, &ob, /*zero_all=*/false));
  out->buffers[1].WrapBuffer(ob);
  AHC_RETURN_NOT_OK(s->FromStatus(ah_cast_numeric(s->ctx(), iw == 4 ? AH_INT32 : AH_INT64, ow == 4 ? AH_INT32 : AH_INT64, in.buffers[1].buf + in.offset * iw,
                                                  nullptr, 0, in.len + 1, /*allow_int_overflow=*/1, /*allow_float_truncate=*/1, ob->dptr)));
  out->buffers[2] = in.buffers[2];
  return Status::OK();
}

// CastFsbToBinary (string_casts.go:154-193): the values buffer becomes the data buffer, offsets (offset + i) · width
static Status ExecCastFsbToBinary(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  Session* s = k->session;
  const ArraySpan& in = b.values[0].array;
  const DataType* to = out->type;
  AHC_RETURN_NOT_OK(ValidateUtf8ForCast(k, in, to));
  const int ow = to->bit_width / 8;
  const int64_t width = in.type->bit_width / 8;
  if (width * in.len > (ow == 4 ? (int64_t)INT32_MAX : INT64_MAX)) return InputTooLarge(in.type, to);
  if (ow == 4 && width * (in.offset + in.len) > (int64_t)INT32_MAX) return InputTooLarge(in.type, to);   // (the reference's int32 wraps here)
  BufferPtr ob;
  AHC_RETURN_NOT_OK(k->Allocate((in.len + 1) * ow, &ob, /*zero_all=*/false));
  out->buffers[1].WrapBuffer(ob);
  AHC_RETURN_NOT_OK(s->FromStatus(ah_fixed_binary_offsets(s->ctx(), ow, (int)width, in.offset, in.len, ob->dptr)));
  out->buffers[2] = in.buffers[1];
  return Status::OK();
}

// CastFsbToFsb (string_casts.go:89-99)
static Status ExecCastFsbToFsb(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  const ArraySpan& in = b.values[0].array;
  const CastOptions* opts = static_cast<const CastOptions*>(k->state);
  const DataType* to = opts && opts->ToType ? opts->ToType : out->type;
  if (in.type->bit_width != to->bit_width)
    return Status::Make(StatusCode::Invalid, "failed casting from " + CastTypeText(in.type) + " to " + CastTypeText(to) + ": widths must match");
  *out = in;
  return Status::OK();
}

// arrow.TypeEqual for the cast meta function's shortcut: decimals by precision and scale (interned: usually the same pointer), every
// other type by its id
static bool CastIsIdentity(const DataType* from, const DataType* to) {
  if (from->id != to->id) return false;
  if (from->id == Type::FIXED_SIZE_BINARY) return from->bit_width == to->bit_width;
  if (!IsDecimal(from->id) || from == to) return true;
  int fp = 0, fs = 0, tp = 0, ts = 0;
  return DecimalParams(from, &fp, &fs) && DecimalParams(to, &tp, &ts) && fp == tp && fs == ts;
}

static const char* CastFunctionName(Type t) {
  switch (t) {
    case Type::DECIMAL128: return "cast_decimal"; case Type::DECIMAL256: return "cast_decimal256";   // cast.go:883-885
    case Type::STRING: return "cast_string"; case Type::LARGE_STRING: return "cast_large_string";              // cast.go:906-912
    case Type::BINARY: return "cast_binary"; case Type::LARGE_BINARY: return "cast_large_binary";
    case Type::FIXED_SIZE_BINARY: return "cast_fixed_sized_binary";
    case Type::BOOL: return "cast_boolean";
    case Type::UINT8: return "cast_uint8"; case Type::INT8: return "cast_int8"; case Type::UINT16: return "cast_uint16";
    case Type::INT16: return "cast_int16"; case Type::UINT32: return "cast_uint32"; case Type::INT32: return "cast_int32";
    case Type::UINT64: return "cast_uint64"; case Type::INT64: return "cast_int64"; case Type::FLOAT32: return "cast_float";
    case Type::FLOAT64: return "cast_double";
    default: return nullptr;
  }
}

// RegisterScalarCast (compute/cast.go:83-85) + the per-target cast functions getCastFunction resolves
// (cast.go:190-260: "cast_int32" …), numeric, boolean, decimal and binary-like targets
void RegisterScalarCast(FunctionRegistry* reg) {
  for (Type to : kNumericTypes) {
    auto fn = std::make_shared<ScalarFunction>(CastFunctionName(to), Arity{1, false});
    for (Type from : kNumericTypes) {
      if (from == to) continue;
      exec::ScalarKernel k;
      k.sig.in_types = {from};
      k.sig.out_is_first_input = false;
      k.sig.out_type = to;
      k.exec_fn = ExecCastNumeric;
      fn->AddKernel(std::move(k));
    }
    exec::ScalarKernel kb;
    kb.sig.in_types = {Type::BOOL};
    kb.sig.out_is_first_input = false;
    kb.sig.out_type = to;
    kb.exec_fn = ExecCastBoolToNumeric;
    fn->AddKernel(std::move(kb));
    // the decimal kernels of every cast_<integer> function (numeric_cast.go:852-857), matched by type id: held beside the
    // function's numeric table (ScalarFunction::AddParametricKernel), whose size of ten is what NumKernels() goes on reporting
    if (IsInteger(to))
      for (Type from : {Type::DECIMAL128, Type::DECIMAL256}) {
        exec::ScalarKernel kd;
        kd.sig.in_types = {from};
        kd.sig.out_is_first_input = false;
        kd.sig.out_type = to;
        kd.exec_fn = ExecCastDecimalToInteger;
        fn->AddParametricKernel(std::move(kd));
      }
    // … and the String / Binary / LargeString / LargeBinary kernels (numeric_cast.go:815-833), beside the table in the same way
    if (IsInteger(to))
      for (Type from : {Type::BINARY, Type::STRING, Type::LARGE_BINARY, Type::LARGE_STRING}) {
        exec::ScalarKernel ks;
        ks.sig.in_types = {from};
        ks.sig.out_is_first_input = false;
        ks.sig.out_type = to;
        ks.exec_fn = ExecCastStringToInteger;
        fn->AddParametricKernel(std::move(ks));
      }
    reg->AddFunction(fn, false);
  }
  // cast_decimal / cast_decimal256 (cast.go:883-885; getDecimalCastKernels numeric_cast.go:912-970): the eight integer inputs by exact
  // type, Decimal128 / Decimal256 by id; the output type is the options' ToType (resolveOutputFromOptions)
  for (Type to : {Type::DECIMAL128, Type::DECIMAL256}) {
    auto fn = std::make_shared<ScalarFunction>(CastFunctionName(to), Arity{1, false});
    for (Type from : kNumericTypes) {
      if (!IsInteger(from)) continue;
      exec::ScalarKernel k;
      k.sig.in_types = {from};
      k.sig.out_is_first_input = false;
      k.sig.out_type = to;
      k.sig.out_from_options = true;
      k.exec_fn = ExecCastIntegerToDecimal;
      fn->AddKernel(std::move(k));
    }
    for (Type from : {Type::DECIMAL128, Type::DECIMAL256}) {
      exec::ScalarKernel k;
      k.sig.in_types = {from};
      k.sig.out_is_first_input = false;
      k.sig.out_type = to;
      k.sig.out_from_options = true;
      k.exec_fn = ExecCastDecimalToDecimal;
      fn->AddKernel(std::move(k));
    }
    reg->AddFunction(fn, false);
  }
  auto fb = std::make_shared<ScalarFunction>(CastFunctionName(Type::BOOL), Arity{1, false});
  for (Type from : kNumericTypes) {
    exec::ScalarKernel k;
    k.sig.in_types = {from};
    k.sig.out_is_first_input = false;
    k.sig.out_type = Type::BOOL;
    k.exec_fn = ExecCastNumericToBool;
    fb->AddKernel(std::move(k));
  }
  for (Type from : {Type::BINARY, Type::STRING, Type::LARGE_BINARY, Type::LARGE_STRING}) {   // boolean_cast.go:77-95
    exec::ScalarKernel k;
    k.sig.in_types = {from};
    k.sig.out_is_first_input = false;
    k.sig.out_type = Type::BOOL;
    k.exec_fn = ExecCastStringToBool;
    fb->AddParametricKernel(std::move(k));
  }
  reg->AddFunction(fb, false);
  // cast_binary / cast_large_binary / cast_string / cast_large_string (cast.go:906-911; GetToBinaryKernels string_casts.go:581-607):
  // the four base-binary inputs and FixedSizeBinary; the string targets also take the integers and Boolean.  The kernels build
  // their own offsets and data (MemNoPrealloc); validity is the executor's, or the input's where the buffers are shared.
  for (Type to : {Type::BINARY, Type::LARGE_BINARY, Type::STRING, Type::LARGE_STRING}) {
    auto fn = std::make_shared<ScalarFunction>(CastFunctionName(to), Arity{1, false});
    auto add = [&](Type from, exec::ArrayKernelExec ex) {
      exec::ScalarKernel k;
      k.sig.in_types = {from};
      k.sig.out_is_first_input = false;
      k.sig.out_type = to;
      k.mem_alloc = exec::MemAlloc::MemNoPrealloc;
      k.exec_fn = std::move(ex);
      fn->AddKernel(std::move(k));
    };
    for (Type from : {Type::STRING, Type::BINARY, Type::LARGE_STRING, Type::LARGE_BINARY}) add(from, ExecCastBinaryToBinary);
    add(Type::FIXED_SIZE_BINARY, ExecCastFsbToBinary);
    if (IsStringType(to)) {
      for (Type from : kNumericTypes)
        if (IsInteger(from)) add(from, ExecCastIntegerToString);
      add(Type::BOOL, ExecCastIntegerToString);
    }
    reg->AddFunction(fn, false);
  }
  // cast_fixed_sized_binary (the reference's spelling, cast.go:912; GetFsbCastKernels string_casts.go:224-232): CastFsbToFsb only
  {
    auto fn = std::make_shared<ScalarFunction>(CastFunctionName(Type::FIXED_SIZE_BINARY), Arity{1, false});
    exec::ScalarKernel k;
    k.sig.in_types = {Type::FIXED_SIZE_BINARY};
    k.sig.out_is_first_input = true;
    k.null_handling = exec::NullHandling::NullComputedNoPrealloc;
    k.mem_alloc = exec::MemAlloc::MemNoPrealloc;
    k.exec_fn = ExecCastFsbToFsb;
    fn->AddKernel(std::move(k));
    reg->AddFunction(fn, false);
  }
  // castMetaFunc (cast.go:45-81)
  reg->AddFunction(std::make_shared<MetaFunction>("cast", Arity{1, false}, nullptr,
      [](ExecCtx* ctx, const FunctionOptions* o, const std::vector<Datum>& args, Datum* out) {
        const CastOptions* opts = dynamic_cast<const CastOptions*>(o);
        if (!opts || !opts->ToType)
          return Status::Make(StatusCode::Invalid, "cast requires that options be passed with a ToType");
        if (CastIsIdentity(args[0].type(), opts->ToType)) { *out = args[0]; return Status::OK(); }  // TypeEqual → the input itself
        const char* name = CastFunctionName(opts->ToType->id);
        if (!name)
          return Status::Make(StatusCode::NotImplemented, std::string("unsupported cast to ") + opts->ToType->name + " from " + args[0].type()->name);
        Status st = CallFunction(ctx, name, o, args, out);
        if (!st.ok() && st.code == StatusCode::NotImplemented && st.msg.find("has no kernel matching") != std::string::npos)
          return Status::Make(StatusCode::NotImplemented, std::string("unsupported cast to ") + opts->ToType->name + " from " + args[0].type()->name);
        return st;
      }), false);
}

// ---- is_in -------------------------------------------------------------------------------------------
static std::string SetTypeText(const DataType* t) {
  return IsFixedWidthBinary(t->id) ? std::string(t->name) + "<" + t->format + ">" : std::string(t->name);
}
static bool IsUtf8(Type id) { return id == Type::STRING || id == Type::LARGE_STRING; }

// initSetLookup (compute/scalar_set_lookup.go:67-135): the value set as pieces in the input's layout.  Numeric inputs: a value set
// of another type is SAFE-cast to the input type, piece by piece.  Byte-string inputs take their own type, String ↔ LargeString and
// Binary ↔ LargeBinary (the offset width differs, the bytes compare the same); the mixes the reference would cast and this layer has
// no cast for (String ↔ Binary: UTF-8 validation; decimals of another precision or scale: a rescale; FixedSizeBinary of another
// width) are refused with NotImplemented — DESIGN.md "Reference quirks — decisions".
static Status IsInValueSet(Session* s, const SetOptions* opts, const DataType* in_type, std::vector<ArrayDataPtr>* parts) {
  const DataType* vt = nullptr;
  if (opts->ValueSet) { *parts = {opts->ValueSet}; vt = opts->ValueSet->type; }
  else if (opts->ValueSetChunkedType) { *parts = opts->ValueSetChunks; vt = opts->ValueSetChunkedType; }
  else return Status::Make(StatusCode::Invalid, "expected array-like datum, got nil");
  const Type iid = in_type->id, vid = vt->id;
  auto mismatch = [&]() {
    return Status::Make(StatusCode::Invalid, "array type doesn't match type of values set: " + SetTypeText(in_type) + " vs " + SetTypeText(vt));
  };
  if (IsUtf8(iid) && !IsBaseBinary(vid)) return mismatch();  // :87-93: no implicit cast from a non-binary type to string
  if (vt == in_type) return Status::OK();                    // interned types: the same pointer ⇔ arrow.TypeEqual
  if (IsBaseBinary(iid) || IsFixedWidthBinary(iid)) {
    const bool both_binary = IsBaseBinary(iid) && IsBaseBinary(vid), both_fixed = IsFixedWidthBinary(iid) && IsFixedWidthBinary(vid);
    const bool both_decimal = both_fixed && iid != Type::FIXED_SIZE_BINARY && vid != Type::FIXED_SIZE_BINARY;
    if (both_binary && IsUtf8(iid) == IsUtf8(vid)) return Status::OK();
    if (both_binary || (both_fixed && (iid == vid || both_decimal)))
      return Status::Make(StatusCode::NotImplemented, "is_in: a " + SetTypeText(in_type) + " column with a " + SetTypeText(vt) +
                                                          " value set needs a cast this layer does not have");
    return mismatch();
  }
  if (IsBaseBinary(vid) || IsFixedWidthBinary(vid)) return mismatch();
  ExecCtx ectx;
  ectx.session = s;
  for (auto& pc : *parts) {
    if (pc->type == in_type) continue;
    Datum casted;
    Status st = CastDatum(&ectx, Datum::Of(pc), CastOptions::Safe(in_type), &casted);
    if (!st.ok()) return st.code == StatusCode::NotImplemented ? mismatch() : st;
    pc = casted.array;
  }
  return Status::OK();
}

static Status ExecIsInDictionary(Session* s, const SetOptions* opts, const ArraySpan& in, ExecResult* out);

// execIsIn (compute/scalar_set_lookup.go:137-172) → DispatchIsIn: the kernel writes data and validity (NullComputedPrealloc)
static Status ExecIsIn(KernelCtx* k, const ExecSpan& b, ExecResult* out) {
  Session* s = k->session;
  const SetOptions* opts = dynamic_cast<const SetOptions*>(static_cast<const FunctionOptions*>(k->state));
  if (!opts) return Status::Make(StatusCode::Invalid, "calling a set lookup function without SetOptions");
  const ArraySpan& in = b.values[0].array;
  if (in.type->id == Type::DICTIONARY) return ExecIsInDictionary(s, opts, in, out);
  std::vector<ArrayDataPtr> parts;
  AHC_RETURN_NOT_OK(IsInValueSet(s, opts, in.type, &parts));
  if (out->len == 0) return Status::OK();
  const uint8_t* valid = in.MayHaveNulls() ? in.buffers[0].buf : nullptr;
  const Type id = in.type->id;
  if ((IsInteger(id) || IsFloating(id)) && opts->ValueSet) {  // one array: ah_is_in as before
    const ArrayDataPtr& vset = parts[0];
    const int w = in.type->bit_width / 8;
    const uint8_t* set_vals = vset->length ? (const uint8_t*)vset->buffers[1]->dptr + vset->offset * w : nullptr;
    const uint8_t* set_valid = vset->buffers[0] ? (const uint8_t*)vset->buffers[0]->dptr : nullptr;
    AHC_RETURN_NOT_OK(s->FromStatus(ah_is_in(s->ctx(), w, Values(in), valid, in.offset, in.len, set_vals, set_valid, vset->offset, vset->length,
                                             opts->NullBehavior, out->buffers[1].buf, out->buffers[0].buf, out->offset)));
    out->nulls = kUnknownNullCount;
    return Status::OK();
  }
  std::vector<ah_set_chunk> set;
  for (auto& pc : parts) {
    const ByteLayout l = LayoutOf(*pc);
    const uint8_t* set_valid = pc->null_count != 0 && pc->buffers[0] ? (const uint8_t*)pc->buffers[0]->dptr : nullptr;
    set.push_back(ah_set_chunk{l.offset_width, l.offsets, l.data, set_valid, l.offset, pc->length});
  }
  const ByteLayout l = LayoutOf(in);
  int rc;
  if (l.offset_width)
    rc = ah_is_in_binary(s->ctx(), l.offset_width, l.offsets, l.data, valid, l.offset, in.len, (int)set.size(), set.data(), opts->NullBehavior,
                         out->buffers[1].buf, out->buffers[0].buf, out->offset);
  else
    rc = ah_is_in_fixed(s->ctx(), l.byte_width, l.data, valid, l.offset, in.len, (int)set.size(), set.data(), opts->NullBehavior, out->buffers[1].buf,
                        out->buffers[0].buf, out->offset);
  AHC_RETURN_NOT_OK(s->FromStatus(rc));
  out->nulls = kUnknownNullCount;
  return Status::OK();
}

// setLookupFunc.DispatchBest decodes a dictionary input first (ensureDictionaryDecoded, compute/scalar_set_lookup.go:37-61).  Here
// the column stays encoded: is_in runs over the dictionary's entries plus one null value behind them (a short array), and every
// row takes the bit of its index — a null index the bit of the null value.  Same data and validity as decode-then-is_in.
static Status ExecIsInDictionary(Session* s, const SetOptions* opts, const ArraySpan& in, ExecResult* out) {
  const ArrayDataPtr& dict = in.dictionary;
  if (!dict) return Status::Make(StatusCode::Invalid, "is_in: dictionary array without a dictionary");
  const DataType* vt = dict->type;
  auto null1 = std::make_shared<ArrayData>();
  null1->type = vt;
  null1->length = 1;
  null1->null_count = 1;
  null1->logical = dict->logical;
  AHC_RETURN_NOT_OK(s->AllocateBitmap(1, &null1->buffers[0]));
  AHC_RETURN_NOT_OK(s->Allocate(IsBaseBinary(vt->id) ? 2 * (vt->bit_width / 8) : std::max(1, vt->bit_width / 8), &null1->buffers[1]));  // zeroed
  if (IsBaseBinary(vt->id)) AHC_RETURN_NOT_OK(s->Allocate(8, &null1->buffers[2]));
  ArrayDataPtr entries;
  AHC_RETURN_NOT_OK(Concatenate(s, {dict, null1}, vt, &entries));
  ExecCtx ectx;
  ectx.session = s;
  Datum lut;
  AHC_RETURN_NOT_OK(CallFunction(&ectx, "is_in", opts, {Datum::Of(entries)}, &lut));
  if (out->len == 0) return Status::OK();
  const ArrayData& l = *lut.array;
  if (l.offset != 0 || !l.buffers[0] || !l.buffers[1]) return Status::Make(StatusCode::Invalid, "is_in: unexpected layout of the dictionary's result");
  AHC_RETURN_NOT_OK(s->FromStatus(ah_is_in_dict_gather(s->ctx(), in.type->bit_width / 8, in.buffers[1].buf, in.MayHaveNulls() ? in.buffers[0].buf : nullptr,
                                                       in.offset, in.len, (const uint8_t*)l.buffers[1]->dptr, (const uint8_t*)l.buffers[0]->dptr,
                                                       dict->length, out->buffers[1].buf, out->buffers[0].buf, out->offset)));
  out->nulls = kUnknownNullCount;
  return Status::OK();
}

// RegisterScalarSetLookup (compute/scalar_set_lookup.go:175-232): fixed-width numeric inputs, String / Binary / LargeString /
// LargeBinary, FixedSizeBinary, Decimal128 / Decimal256, and dictionary inputs of any of them (setLookupFunc.DispatchBest).
// Boolean stays unregistered.
void RegisterScalarSetLookup(FunctionRegistry* reg) {
  auto fn = std::make_shared<ScalarFunction>("is_in", Arity{1, false});
  std::vector<Type> types(std::begin(kNumericTypes), std::end(kNumericTypes));
  for (Type t : {Type::STRING, Type::BINARY, Type::LARGE_STRING, Type::LARGE_BINARY, Type::FIXED_SIZE_BINARY, Type::DECIMAL128, Type::DECIMAL256,
                 Type::DICTIONARY})
    types.push_back(t);
  for (Type t : types) {
    exec::ScalarKernel k;
    k.sig.in_types = {t};
    k.sig.out_is_first_input = false;
    k.sig.out_type = Type::BOOL;
    k.null_handling = exec::NullHandling::NullComputedPrealloc;  // :186-187
    k.exec_fn = ExecIsIn;
    fn->AddKernel(std::move(k));
  }
  reg->AddFunction(fn, false);
}

// ---- sort_indices / sort ------------------------------------------------------------------------------
// sortIndicesMetaFunc → sortIndicesImpl (compute/vector_sort.go:42-52, 117-190) → kernels.SortIndices
// (kernels/vector_sort.go:388-481), array input: one key, ColumnIndex ignored; uint64 indices, no nulls
// What sort_indices and select_k share: the arguments as equal-length arrays (a record batch → its columns, a chunked column →
// its concatenation) and the options' keys as ah_sort_keys over them.  `fn` names the caller in the messages.
static Status PrepareSortKeys(Session* s, const char* fn, const std::vector<SortKey>& keys_in, const std::vector<Datum>& args_in,
                              std::vector<Datum>* args_out, std::vector<ah_sort_key>* skeys, int64_t* length_out) {
  const std::string name = fn;
  if (keys_in.empty()) return Status::Make(StatusCode::Invalid, "must provide at least one sort key");  // :119-121
  // a chunked column is sorted as its logical concatenation: the indices address the whole column
  // (compute/vector_sort.go:144-148, SortIndicesChunked :226)
  std::vector<Datum>& args = *args_out;
  args = args_in;
  if (args.size() == 1 && args[0].kind == DatumKind::Record) {  // KindRecord (:150-166): the keys name columns of the batch
    std::vector<Datum> cols;
    for (auto& c : args_in[0].chunks) cols.push_back(Datum::Of(c));
    if (cols.empty()) return Status::Make(StatusCode::Invalid, name + ": record batch without columns");
    args = cols;
  }
  for (auto& a : args) {
    if (a.kind != DatumKind::Chunked) continue;
    if (a.chunks.empty()) return Status::Make(StatusCode::NotImplemented, name + " of a chunked array without chunks");
    ArrayDataPtr whole;
    AHC_RETURN_NOT_OK(Concatenate(s, a.chunks, a.chunked_type, &whole));
    a = Datum::Of(whole);
  }
  // one array: the first key, ColumnIndex ignored (:130-141); several arrays = the columns of a record batch,
  // every key names its column (:153-166)
  std::vector<SortKey> keys = keys_in;
  if (args.size() == 1) { keys.resize(1); keys[0].ColumnIndex = 0; }
  if (keys.size() > 8)  // maxRadixSortKeys (kernels/vector_sort.go:60): beyond it the reference switches comparator
    return Status::Make(StatusCode::NotImplemented, name + ": more than 8 sort keys");
  int64_t length = -1;
  for (auto& a : args) {
    if (a.kind != DatumKind::Array)
      return Status::Make(StatusCode::NotImplemented, "unsupported type for " + name + " operation: the accelerated path sorts arrays");
    if (length < 0) length = a.array->length;
    else if (length != a.array->length) return Status::Make(StatusCode::Invalid, "all columns must have the same length");  // kernels :403-407
  }
  for (size_t i = 0; i < keys.size(); i++) {
    const SortKey& key = keys[i];
    if (key.ColumnIndex < 0 || key.ColumnIndex >= (int)args.size())
      return Status::Make(StatusCode::Invalid, "sort key " + std::to_string(i) + " has invalid column index " + std::to_string(key.ColumnIndex));  // :158-160
    const ArrayData& a = *args[key.ColumnIndex].array;
    const Type id = a.type->id;
    ah_sort_key k{};
    if (IsInteger(id) || IsFloating(id)) {
      k.type = (int)id;
      k.values = a.length && a.buffers[1] ? a.buffers[1]->dptr : nullptr;
    } else if (IsBaseBinary(id) || IsFixedWidthBinary(id)) {  // binary :225-232, FixedSizeBinary :233-234, Decimal128 / 256 :213-216
      const ByteLayout l = LayoutOf(a);
      k.type = l.offset_width == 4 ? AH_BINARY : l.offset_width == 8 ? AH_LARGE_BINARY : (int)id;
      k.offsets = l.offsets;
      k.values = l.data;
      k.byte_width = l.byte_width;
    } else {
      return Status::Make(StatusCode::NotImplemented, std::string("sorting not supported for type ") + a.type->name);  // :266-268
    }
    k.valid = (a.buffers[0] && a.null_count != 0) ? (const uint8_t*)a.buffers[0]->dptr : nullptr;
    k.off = a.offset;
    k.descending = key.Order == SortOrderDescending;
    k.nulls_at_start = key.Placement == SortNullsAtStart;
    skeys->push_back(k);
  }
  *length_out = length;
  return Status::OK();
}

// `length` uint64 row numbers without nulls, not yet written
static Status AllocateIndices(Session* s, int64_t length, std::shared_ptr<ArrayData>* out) {
  auto res = std::make_shared<ArrayData>();
  res->type = GetDataType(Type::UINT64);
  res->length = length;
  res->null_count = 0;
  AHC_RETURN_NOT_OK(s->Allocate(length * 8, &res->buffers[1], /*zero_all=*/false));
  *out = res;
  return Status::OK();
}

static Status SortIndicesImpl(ExecCtx* ctx, const FunctionOptions* o, const std::vector<Datum>& args_in, Datum* out) {
  const SortOptions* opts = dynamic_cast<const SortOptions*>(o);
  if (!opts || opts->Keys.empty()) return Status::Make(StatusCode::Invalid, "must provide at least one sort key");  // :119-121
  Session* s = ctx->session;
  std::vector<Datum> args;
  std::vector<ah_sort_key> skeys;
  int64_t length = 0;
  AHC_RETURN_NOT_OK(PrepareSortKeys(s, "sort_indices", opts->Keys, args_in, &args, &skeys, &length));
  std::shared_ptr<ArrayData> res;
  AHC_RETURN_NOT_OK(AllocateIndices(s, length, &res));
  if (length > 0)
    AHC_RETURN_NOT_OK(s->FromStatus(ah_sort_indices_keys(s->ctx(), (int)skeys.size(), skeys.data(), length, (uint64_t*)res->buffers[1]->dptr)));
  *out = Datum::Of(res);
  return Status::OK();
}

// select_k / select_k_unstable: the first min(K, length) entries of sort_indices with the same keys, without the sort where the
// first key is numeric (ah_select_k, csrc/ah_select.hip); takes what sort_indices takes
static Status SelectKImpl(ExecCtx* ctx, const FunctionOptions* o, const std::vector<Datum>& args_in, Datum* out) {
  const SelectKOptions* opts = dynamic_cast<const SelectKOptions*>(o);
  if (!opts || opts->K < 0) return Status::Make(StatusCode::Invalid, "select_k: a non-negative k must be given");
  Session* s = ctx->session;
  std::vector<Datum> args;
  std::vector<ah_sort_key> skeys;
  int64_t length = 0;
  AHC_RETURN_NOT_OK(PrepareSortKeys(s, "select_k", opts->Keys, args_in, &args, &skeys, &length));
  const int64_t k = std::min(opts->K, length);
  std::shared_ptr<ArrayData> res;
  AHC_RETURN_NOT_OK(AllocateIndices(s, k, &res));
  if (k > 0)
    AHC_RETURN_NOT_OK(s->FromStatus(ah_select_k(s->ctx(), (int)skeys.size(), skeys.data(), length, k, ctx->SelectKRoute, (uint64_t*)res->buffers[1]->dptr)));
  *out = Datum::Of(res);
  return Status::OK();
}

void RegisterVectorSort(FunctionRegistry* reg) {
  // Arity: one array, or the columns of a record batch as separate arguments (this layer has no RecordBatch datum)
  reg->AddFunction(std::make_shared<MetaFunction>("sort_indices", Arity{1, true}, nullptr, SortIndicesImpl), false);
  // sortMetaFunc (compute/vector_sort.go:66-85): take(input, sort_indices(input, options))
  reg->AddFunction(std::make_shared<MetaFunction>("sort", Arity{1, false}, nullptr,
      [](ExecCtx* ctx, const FunctionOptions* o, const std::vector<Datum>& args, Datum* out) {
        Datum indices;
        AHC_RETURN_NOT_OK(CallFunction(ctx, "sort_indices", o, args, &indices));
        return CallFunction(ctx, "take", nullptr, {args[0], indices}, out);
      }), false);
  // one implementation under two names, like sub / subtract: Arrow C++ calls it select_k_unstable, and a stable answer is a valid one
  for (const char* name : {"select_k", "select_k_unstable"})
    reg->AddFunction(std::make_shared<MetaFunction>(name, Arity{1, true}, nullptr, SelectKImpl), false);
}

// ---- cumulative_sum / cumulative_sum_checked ---------------------------------------------------
// Safe numeric cast of the Start scalar to the input type — what safeCastScalar → CastDatum(SafeCastOptions)
// decides (compute/vector_cumulative.go:53-70, kernels/vector_cumulative.go:71-90): integer targets
// need an in-range, integral value; an integer start for a float target must be exactly representable;
// float → float is always allowed.  Failure is arrow.ErrInvalid.
Status SafeCastCumulativeStart(const Scalar& start, const DataType* to, uint8_t out[8]) {
  auto fail = [&](const char* why) {
    return Status::Make(StatusCode::Invalid, std::string("cannot cast cumulative sum start value to ") + to->name + ": " + why);
  };
  memset(out, 0, 8);
  Type from = start.type->id;
  if (from == to->id) { memcpy(out, start.value, 8); return Status::OK(); }
  if (!IsInteger(from) && !IsFloating(from)) return fail("start value is not numeric");
  // widen the source to (sign, magnitude) or a double
  bool src_float = IsFloating(from);
  double f = 0; bool neg = false; uint64_t mag = 0;
  if (src_float) {
    if (from == Type::FLOAT32) { float t; memcpy(&t, start.value, 4); f = t; } else memcpy(&f, start.value, 8);
  } else if (IsSignedInteger(from)) {
    int64_t v = 0;
    switch (start.type->bit_width) {
      case 8: { int8_t t; memcpy(&t, start.value, 1); v = t; break; }
      case 16: { int16_t t; memcpy(&t, start.value, 2); v = t; break; }
      case 32: { int32_t t; memcpy(&t, start.value, 4); v = t; break; }
      default: memcpy(&v, start.value, 8);
    }
    neg = v < 0;
    mag = neg ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
  } else {
    memcpy(&mag, start.value, start.type->bit_width / 8);
  }
  if (IsFloating(to->id)) {
    if (src_float) {  // float64 → float32: plain conversion
      float t = (float)f; memcpy(out, &t, 4);
      return Status::OK();
    }
    const uint64_t lim = to->id == Type::FLOAT32 ? (1ull << 24) : (1ull << 53);  // exactly representable integers
    if (mag > lim) return fail("integer value not exactly representable in the float type");
    double d = neg ? -(double)mag : (double)mag;
    if (to->id == Type::FLOAT32) { float t = (float)d; memcpy(out, &t, 4); } else memcpy(out, &d, 8);
    return Status::OK();
  }
  // integer target
  if (src_float) {
    if (!(f == f) || f != std::trunc(f)) return fail("float value would be truncated");
    if (std::fabs(f) >= 18446744073709551616.0) return fail("value out of range");
    neg = f < 0;
    mag = (uint64_t)std::fabs(f);
  }
  int bits = to->bit_width;
  if (IsSignedInteger(to->id)) {
    uint64_t maxpos = (1ull << (bits - 1)) - 1;
    if (neg ? mag > maxpos + 1 : mag > maxpos) return fail("value out of range");
    int64_t v = neg ? (int64_t)((uint64_t)0 - mag) : (int64_t)mag;
    memcpy(out, &v, bits / 8);
  } else {
    if (neg && mag != 0) return fail("value out of range");
    if (bits < 64 && mag >> bits) return fail("value out of range");
    memcpy(out, &mag, bits / 8);
  }
  return Status::OK();
}

// cumulativeSumExec → cumulativeSumSpans (kernels/vector_cumulative.go:320-360)
static Status ExecCumulativeSum(KernelCtx* k, const ExecSpan& b, ExecResult* out, bool checked) {
  Session* s = k->session;
  ArraySpan in = b.values[0].array;
  const CumulativeOptions* opts = static_cast<const CumulativeOptions*>(k->state);
  // initCumulativeSum :118-146 → cumulativeStartValue :92-116
  uint8_t start[8] = {0};
  bool have_start = false;
  if (opts && opts->Start) {
    if (!opts->Start->valid) return Status::Make(StatusCode::Invalid, "cumulative sum start value must be valid");
    AHC_RETURN_NOT_OK(SafeCastCumulativeStart(*opts->Start, in.type, start));
    have_start = true;
  }
  out->len = in.len;
  if (in.len == 0) return Status::OK();
  AHC_RETURN_NOT_OK(in.UpdateNullCount(s));
  bool needs_validity = in.MayHaveNulls();  // :354
  int w = in.type->bit_width / 8;
  BufferPtr vb, db;
  AHC_RETURN_NOT_OK(k->Allocate(in.len * w, &db, /*zero_all=*/false));  // prepareCumulativeOutput :211-226
  out->buffers[1].WrapBuffer(db);
  if (needs_validity) {
    AHC_RETURN_NOT_OK(k->AllocateBitmap(in.len, &vb));
    AHC_RETURN_NOT_OK(s->FromStatus(ah_memset_async(s->ctx(), vb->dptr, 0xFF, (size_t)((in.len + 7) / 8))));  // memory.Set(validity, 0xFF)
    out->buffers[0].WrapBuffer(vb);
  }
  int64_t nulls = 0;
  AHC_RETURN_NOT_OK(s->FromStatus(ah_cumulative_sum(s->ctx(), (int)in.type->id, Values(in), needs_validity ? in.buffers[0].buf : nullptr, in.offset,
                                                    in.len, have_start ? start : nullptr, opts && opts->SkipNulls, checked ? 1 : 0, db->dptr,
                                                    needs_validity ? (uint8_t*)vb->dptr : nullptr, needs_validity ? &nulls : nullptr)));
  out->nulls = nulls;
  return Status::OK();
}

static const CumulativeOptions kDefaultCumulativeOptions;

// RegisterVectorCumulative (compute/vector_cumulative.go:72-94)
void RegisterVectorCumulative(FunctionRegistry* reg) {
  for (bool checked : {false, true}) {
    auto fn = std::make_shared<VectorFunction>(checked ? "cumulative_sum_checked" : "cumulative_sum", Arity{1, false}, &kDefaultCumulativeOptions);
    fn->chunked = VectorFunction::Chunked::SingleChunk;
    for (Type t : kNumericTypes) {
      exec::VectorKernel k;
      k.sig.in_types = {t};
      k.can_execute_chunkwise = false;  // newCumulativeSumKernel :383-384
      k.exec_fn = [checked](KernelCtx* kc, const ExecSpan& b, ExecResult* o) { return ExecCumulativeSum(kc, b, o, checked); };
      fn->AddKernel(std::move(k));
    }
    reg->AddFunction(fn, false);
  }
}

// ---- group_by (no reference analogue: arrow-go has no hash aggregate) --------------------------------------------
// One RecordDatum in, one out: the key columns gathered at every group's first row, then one column per aggregate, rows = groups in
// first-seen order.  ah_group_ids runs once per call; per value column the typed aggregates of ah_group_agg.hip run once each and
// are shared by the aggregates that name the column (sum + mean + count: one ah_group_sum_typed, one ah_group_mean; variance + stddev
// at any ddof + mean + count: one ah_group_m2, then one ah_group_variance per output column).  count_distinct is a composition: a
// second ah_group_ids over the pair (group id, value), the group id and the value's validity bit gathered at every pair's first row,
// and ah_group_count over those.
namespace {

struct GroupByColumnWork {   // what the aggregates naming one value column need, and what has been computed for it
  bool sum = false, mean = false, min_max = false, count = false, m2 = false, distinct = false;
  bool means_done = false;   // ah_group_m2 has left the means
  BufferPtr sums, mins, maxs, means, m2s, counts, distinct_counts, validity;
  int64_t nulls = 0;   // groups without a valid value
  std::map<int, std::pair<BufferPtr, int64_t>> ddof_validity;   // ddof > 0 → bits of counts > ddof (null: all set), groups with counts ≤ ddof
};

// a column as ah_group_ids takes it; false: not a type it takes
bool GroupKeyOf(const ArrayData& a, ah_group_key* out) {
  const Type id = a.type->id;
  ah_group_key k{};
  auto dptr = [&](int i) -> const uint8_t* { return a.buffers[i] ? (const uint8_t*)a.buffers[i]->dptr : nullptr; };
  if (id == Type::BOOL) { k.bits = 1; k.data = dptr(1); }
  else if (IsBaseBinary(id)) { k.offset_width = a.type->bit_width / 8; k.offsets = dptr(1); k.data = dptr(2); }
  else if (IsNumeric(id) || IsFixedWidthBinary(id)) { k.byte_width = a.type->bit_width / 8; k.data = dptr(1); }
  else return false;
  k.valid = a.null_count != 0 ? dptr(0) : nullptr;
  k.off = a.offset;
  *out = k;
  return true;
}

Status GroupByImpl(ExecCtx* ctx, const FunctionOptions* o, const std::vector<Datum>& args, Datum* out) {
  const GroupByOptions* opts = dynamic_cast<const GroupByOptions*>(o);
  if (args[0].kind != DatumKind::Record) return Status::Make(StatusCode::Invalid, "group_by: the argument must be a record batch");
  if (!opts || opts->Keys.empty()) return Status::Make(StatusCode::Invalid, "group_by: no keys (keys=<column>,...)");
  if (opts->Keys.size() > 8) return Status::Make(StatusCode::Invalid, "group_by: more than 8 keys (" + std::to_string(opts->Keys.size()) + ")");
  Session* s = ctx->session;
  const Datum& batch = args[0];
  const int64_t n = batch.num_rows;
  auto column = [&](const std::string& name) -> int {
    for (size_t i = 0; i < batch.names.size(); i++) if (batch.names[i] == name) return (int)i;
    return -1;
  };
  auto no_kernel = [](const std::string& what, const ArrayData& a) {
    return Status::Make(StatusCode::NotImplemented, "function 'group_by' has no kernel matching input types (" + what + ": " +
                                                        (a.logical.empty() ? std::string(a.type->name) : a.logical) + ")");
  };
  for (auto& c : batch.chunks)
    if (c->on_host) return Status::Make(StatusCode::NotImplemented, "group_by: host-resident columns are not taken; upload the batch first");
  // the keys, as ah_group_ids describes them
  std::vector<int> key_cols;
  std::vector<ah_group_key> gkeys;
  for (auto& name : opts->Keys) {
    const int ci = column(name);
    if (ci < 0) return Status::Make(StatusCode::Invalid, "group_by: unknown key column '" + name + "'");
    const ArrayData& a = *batch.chunks[ci];
    const Type id = a.type->id;
    // a dictionary's indices are not its values: two indices may name equal values
    if (id == Type::DICTIONARY) return Status::Make(StatusCode::NotImplemented, "group_by: dictionary-typed key column '" + name + "'; decode it first");
    ah_group_key k{};
    if (!GroupKeyOf(a, &k)) return no_kernel("key", a);
    key_cols.push_back(ci);
    gkeys.push_back(k);
  }
  // the aggregates: names and types checked before anything runs
  std::map<int, GroupByColumnWork> work;
  bool count_all = false;
  for (auto& ag : opts->Aggregates) {
    const std::string& f = ag.Function;
    if (f == "count_all") {
      if (!ag.Column.empty()) return Status::Make(StatusCode::Invalid, "group_by: count_all takes no column, got '" + ag.Column + "'");
      count_all = true;
      continue;
    }
    const bool moment = f == "variance" || f == "stddev";
    if (f != "sum" && f != "mean" && f != "min" && f != "max" && f != "count" && f != "count_distinct" && !moment)
      return Status::Make(StatusCode::Invalid, "group_by: unknown aggregate '" + f + "'");
    if (ag.DdofGiven && !moment)
      return Status::Make(StatusCode::Invalid, "group_by: ddof is an option of variance and stddev, not of '" + f + "' ('" + f + ":" + ag.Column + ":<ddof>')");
    if (ag.Ddof < 0)
      return Status::Make(StatusCode::Invalid, "group_by: the ddof of '" + f + ":" + ag.Column + "' must be an integer >= 0");
    const int ci = column(ag.Column);
    if (ci < 0) return Status::Make(StatusCode::Invalid, "group_by: unknown column '" + ag.Column + "' of aggregate '" + f + "'");
    const ArrayData& a = *batch.chunks[ci];
    GroupByColumnWork& w = work[ci];
    if (f == "count") { w.count = true; continue; }
    if (f == "count_distinct") {
      if (a.type->id == Type::DICTIONARY)
        return Status::Make(StatusCode::NotImplemented, "group_by: count_distinct of the dictionary-typed column '" + ag.Column + "'; decode it first");
      ah_group_key k{};
      if (!GroupKeyOf(a, &k)) return no_kernel(f, a);
      w.distinct = true;
      continue;
    }
    if (!IsNumeric(a.type->id) || ((f == "sum" || f == "mean" || moment) && !a.logical.empty())) return no_kernel(f, a);
    if (f == "sum") w.sum = true; else if (f == "mean") w.mean = true; else if (moment) w.m2 = true; else w.min_max = true;
  }
  // ids and first rows, once
  BufferPtr ids, first_rows;
  AHC_RETURN_NOT_OK(s->Allocate((n > 0 ? n : 1) * 4, &ids, /*zero_all=*/false));
  AHC_RETURN_NOT_OK(s->Allocate((n + 1) * 8, &first_rows, /*zero_all=*/false));
  int64_t ng = 0;
  if (n > 0) AHC_RETURN_NOT_OK(s->FromStatus(ah_group_ids(s->ctx(), (int)gkeys.size(), gkeys.data(), n, (int32_t*)ids->dptr, (int64_t*)first_rows->dptr, &ng)));
  std::vector<std::string> names;
  std::vector<ArrayDataPtr> cols;
  {
    auto idx = std::make_shared<ArrayData>();
    idx->type = GetDataType(Type::INT64);
    idx->length = ng;
    idx->null_count = 0;
    idx->buffers[1] = first_rows;
    static const TakeOptions kNoBoundsCheck = [] { TakeOptions t; t.BoundsCheck = false; return t; }();
    for (size_t i = 0; i < key_cols.size(); i++) {
      Datum col;
      AHC_RETURN_NOT_OK(CallFunction(ctx, "array_take", &kNoBoundsCheck, {Datum::Of(batch.chunks[key_cols[i]]), Datum::Of(idx)}, &col));
      names.push_back(opts->Keys[i]);
      cols.push_back(col.array);
    }
  }
  const int64_t room = ng > 0 ? ng : 1;
  const int32_t* idp = (const int32_t*)ids->dptr;
  for (auto& kv : work) {
    const ArrayData& a = *batch.chunks[kv.first];
    GroupByColumnWork& w = kv.second;
    const uint8_t* vvalid = a.buffers[0] && a.null_count != 0 ? (const uint8_t*)a.buffers[0]->dptr : nullptr;
    // the mean is ah_group_m2's where that runs anyway — but an 8-byte integer's stays the wrapping sum's quotient, as without a variance
    const bool m2_mean = w.m2 && !(IsInteger(a.type->id) && a.type->bit_width == 64);
    const bool need_sum = w.sum || (w.mean && !m2_mean);
    const bool reads = need_sum || w.min_max || w.m2;
    const int width = reads ? a.type->bit_width / 8 : 0;
    const uint8_t* vals = width && a.buffers[1] ? (const uint8_t*)a.buffers[1]->dptr + a.offset * width : nullptr;
    AHC_RETURN_NOT_OK(s->Allocate(room * 8, &w.counts, /*zero_all=*/false));
    if (w.m2) {
      AHC_RETURN_NOT_OK(s->Allocate(room * 8, &w.means, /*zero_all=*/false));
      AHC_RETURN_NOT_OK(s->Allocate(room * 8, &w.m2s, /*zero_all=*/false));
      AHC_RETURN_NOT_OK(s->FromStatus(ah_group_m2(s->ctx(), (int)a.type->id, idp, ng, vals, vvalid, a.offset, n, (double*)w.means->dptr, (double*)w.m2s->dptr,
                                                  (int64_t*)w.counts->dptr)));
      w.means_done = m2_mean;
    }
    if (w.distinct && ng > 0) {
      ah_group_key pair[2] = {};
      pair[0].byte_width = 4;
      pair[0].data = (const uint8_t*)idp;
      GroupKeyOf(a, &pair[1]);
      BufferPtr pair_ids, pair_rows;
      AHC_RETURN_NOT_OK(s->Allocate(n * 4, &pair_ids, /*zero_all=*/false));
      AHC_RETURN_NOT_OK(s->Allocate((n + 1) * 8, &pair_rows, /*zero_all=*/false));
      int64_t npairs = 0;
      AHC_RETURN_NOT_OK(s->FromStatus(ah_group_ids(s->ctx(), 2, pair, n, (int32_t*)pair_ids->dptr, (int64_t*)pair_rows->dptr, &npairs)));
      auto rows = std::make_shared<ArrayData>();
      rows->type = GetDataType(Type::INT64);
      rows->length = npairs;
      rows->null_count = 0;
      rows->buffers[1] = pair_rows;
      static const TakeOptions kNoBoundsCheck = [] { TakeOptions t; t.BoundsCheck = false; return t; }();
      auto all_ids = std::make_shared<ArrayData>();
      all_ids->type = GetDataType(Type::INT32);
      all_ids->length = n;
      all_ids->null_count = 0;
      all_ids->buffers[1] = ids;
      Datum gids, vbits;
      AHC_RETURN_NOT_OK(CallFunction(ctx, "array_take", &kNoBoundsCheck, {Datum::Of(all_ids), Datum::Of(rows)}, &gids));
      if (vvalid) {   // the value's validity bits, gathered as the values of a Boolean column that lies where the bitmap lies
        auto valid_bits = std::make_shared<ArrayData>();
        valid_bits->type = GetDataType(Type::BOOL);
        valid_bits->length = n;
        valid_bits->offset = a.offset;
        valid_bits->null_count = 0;
        valid_bits->buffers[1] = a.buffers[0];
        AHC_RETURN_NOT_OK(CallFunction(ctx, "array_take", &kNoBoundsCheck, {Datum::Of(valid_bits), Datum::Of(rows)}, &vbits));
      }
      if (gids.array->offset != 0) return Status::Make(StatusCode::Invalid, "group_by: the gather returned a sliced array");
      AHC_RETURN_NOT_OK(s->Allocate(room * 8, &w.distinct_counts, /*zero_all=*/false));
      AHC_RETURN_NOT_OK(s->FromStatus(ah_group_count(s->ctx(), (const int32_t*)gids.array->buffers[1]->dptr, ng,
                                                     vvalid ? (const uint8_t*)vbits.array->buffers[1]->dptr : nullptr, vvalid ? vbits.array->offset : 0, npairs,
                                                     (int64_t*)w.distinct_counts->dptr)));
    }
    if (w.distinct && ng == 0) AHC_RETURN_NOT_OK(s->Allocate(room * 8, &w.distinct_counts, /*zero_all=*/false));
    if (need_sum) {
      AHC_RETURN_NOT_OK(s->Allocate(room * 8, &w.sums, /*zero_all=*/false));
      if (!w.means) AHC_RETURN_NOT_OK(s->Allocate(room * 8, &w.means, /*zero_all=*/false));
      AHC_RETURN_NOT_OK(s->FromStatus(ah_group_sum_typed(s->ctx(), (int)a.type->id, idp, ng, vals, vvalid, a.offset, n, w.sums->dptr, (int64_t*)w.counts->dptr)));
    }
    if (w.min_max) {
      AHC_RETURN_NOT_OK(s->Allocate(room * width, &w.mins, /*zero_all=*/false));
      AHC_RETURN_NOT_OK(s->Allocate(room * width, &w.maxs, /*zero_all=*/false));
      AHC_RETURN_NOT_OK(s->FromStatus(ah_group_min_max_typed(s->ctx(), (int)a.type->id, idp, ng, vals, vvalid, a.offset, n, w.mins->dptr, w.maxs->dptr,
                                                             (int64_t*)w.counts->dptr)));
    }
    if (!need_sum && !w.min_max && !w.m2 && w.count)
      AHC_RETURN_NOT_OK(s->FromStatus(ah_group_count(s->ctx(), idp, ng, vvalid, a.offset, n, (int64_t*)w.counts->dptr)));
    // a group holds at least one row, so only a column with nulls can leave a group without a valid value: validity = counts != 0
    // (variance and stddev at ddof > 0: validity = counts > ddof, whether the column has nulls or not)
    auto count_validity = [&](const char* cmp, int64_t bound, BufferPtr* validity, int64_t* nulls) -> Status {
      auto counts = std::make_shared<ArrayData>();
      counts->type = GetDataType(Type::INT64);
      counts->length = ng;
      counts->null_count = 0;
      counts->buffers[1] = w.counts;
      auto than = std::make_shared<Scalar>();
      than->type = counts->type;
      than->valid = true;
      memcpy(than->value, &bound, 8);
      Datum bits;
      AHC_RETURN_NOT_OK(CallFunction(ctx, cmp, nullptr, {Datum::Of(counts), Datum::Of(than)}, &bits));
      ArraySpan span;
      span.type = GetDataType(Type::BOOL);
      span.len = ng;
      span.offset = bits.array->offset;
      span.buffers[0].WrapBuffer(bits.array->buffers[1]);
      AHC_RETURN_NOT_OK(span.UpdateNullCount(s, nulls));
      if (*nulls) {
        if (bits.array->offset != 0) return Status::Make(StatusCode::Invalid, "group_by: the comparison returned a sliced bitmap");
        *validity = bits.array->buffers[1];
      }
      return Status::OK();
    };
    if (vvalid && ng > 0 && (need_sum || w.min_max || w.m2)) AHC_RETURN_NOT_OK(count_validity("not_equal", 0, &w.validity, &w.nulls));
    if (w.m2 && ng > 0)
      for (auto& ag : opts->Aggregates)
        if ((ag.Function == "variance" || ag.Function == "stddev") && column(ag.Column) == kv.first && ag.Ddof > 0 && !w.ddof_validity.count(ag.Ddof)) {
          auto& v = w.ddof_validity[ag.Ddof];
          v.second = 0;
          AHC_RETURN_NOT_OK(count_validity("greater", ag.Ddof, &v.first, &v.second));
        }
  }
  BufferPtr all_counts;
  if (count_all) {
    AHC_RETURN_NOT_OK(s->Allocate(room * 8, &all_counts, /*zero_all=*/false));
    AHC_RETURN_NOT_OK(s->FromStatus(ah_group_count(s->ctx(), idp, ng, nullptr, 0, n, (int64_t*)all_counts->dptr)));
  }
  for (auto& ag : opts->Aggregates) {
    auto col = std::make_shared<ArrayData>();
    col->length = ng;
    col->null_count = 0;
    const std::string& f = ag.Function;
    if (f == "count_all") {
      col->type = GetDataType(Type::INT64);
      col->buffers[1] = all_counts;
      names.push_back("count_all");
      cols.push_back(col);
      continue;
    }
    const int ci = column(ag.Column);
    const ArrayData& a = *batch.chunks[ci];
    GroupByColumnWork& w = work[ci];
    if (f == "count") {
      col->type = GetDataType(Type::INT64);
      col->buffers[1] = w.counts;
    } else if (f == "count_distinct") {
      col->type = GetDataType(Type::INT64);
      col->buffers[1] = w.distinct_counts;
    } else if (f == "variance" || f == "stddev") {
      BufferPtr vals;
      AHC_RETURN_NOT_OK(s->Allocate(room * 8, &vals, /*zero_all=*/false));
      AHC_RETURN_NOT_OK(s->FromStatus(ah_group_variance(s->ctx(), (const double*)w.m2s->dptr, (const int64_t*)w.counts->dptr, ng, ag.Ddof, f == "stddev",
                                                        (double*)vals->dptr)));
      col->type = GetDataType(Type::FLOAT64);
      col->buffers[1] = vals;
      if (ag.Ddof > 0 && ng > 0) { col->buffers[0] = w.ddof_validity[ag.Ddof].first; col->null_count = w.ddof_validity[ag.Ddof].second; }
      else { col->buffers[0] = w.validity; col->null_count = w.nulls; }
    } else {
      col->null_count = w.nulls;
      col->buffers[0] = w.validity;
      if (f == "sum") {
        col->type = GetDataType(IsFloating(a.type->id) ? Type::FLOAT64 : IsSignedInteger(a.type->id) ? Type::INT64 : Type::UINT64);
        col->buffers[1] = w.sums;
      } else if (f == "mean" && w.means_done) {
        col->type = GetDataType(Type::FLOAT64);
        col->buffers[1] = w.means;
      } else if (f == "mean") {
        const int sum_type = IsFloating(a.type->id) ? AH_FLOAT64 : IsSignedInteger(a.type->id) ? AH_INT64 : AH_UINT64;
        AHC_RETURN_NOT_OK(s->FromStatus(ah_group_mean(s->ctx(), sum_type, w.sums->dptr, (const int64_t*)w.counts->dptr, ng, (double*)w.means->dptr)));
        col->type = GetDataType(Type::FLOAT64);
        col->buffers[1] = w.means;
      } else {
        col->type = a.type;
        col->logical = a.logical;
        col->buffers[1] = f == "min" ? w.mins : w.maxs;
      }
    }
    names.push_back(ag.Column + "_" + f);
    cols.push_back(col);
  }
  *out = Datum::OfRecord(std::move(names), std::move(cols), ng);
  return Status::OK();
}

}  // namespace

void RegisterGroupBy(FunctionRegistry* reg) {
  reg->AddFunction(std::make_shared<MetaFunction>("group_by", Arity{1, false}, nullptr, GroupByImpl), false);
}

// ---- hash_join (no reference analogue: arrow-go has no join) ------------------------------------------------------
// Two RecordDatums in, one out.  The key columns of both sides are laid end to end, position by position, and ONE ah_group_ids call
// gives every row of both sides a dense id in one id space: equal key tuples ARE equal ids (the equality of ah_group_ids: bytes).  A
// null is one more value to ah_group_ids, so each side also carries a row-validity bitmap — the AND of its key columns' validity —
// and a row under a cleared bit matches nothing.  The right side becomes a CSR by id (ah_join_build); the left side is counted and
// expanded into two index vectors (ah_join_count, ah_join_expand), or into a mask (ah_join_match_bits) for the semi / anti joins;
// every output column is an array_take with those indices, a filter with that mask.
namespace {

enum class JoinKind { Inner, LeftOuter, LeftSemi, LeftAnti };

// the AND of the validity bitmaps of `cols` over the batch's rows: *bits == nullptr when no column has nulls; one column with nulls
// lends its own buffer (and bit offset); more are ANDed into a bitmap of the call's
Status JoinRowValidity(Session* s, const Datum& batch, const std::vector<int>& cols, BufferPtr* owner, const uint8_t** bits, int64_t* off) {
  *bits = nullptr;
  *off = 0;
  std::vector<const ArrayData*> with_nulls;
  for (int ci : cols) {
    const ArrayData& a = *batch.chunks[ci];
    if (a.null_count != 0 && a.buffers[0]) with_nulls.push_back(&a);
  }
  if (with_nulls.empty() || batch.num_rows == 0) return Status::OK();
  auto vbits = [](const ArrayData* a) { return (const uint8_t*)a->buffers[0]->dptr; };
  if (with_nulls.size() == 1) {
    *owner = with_nulls[0]->buffers[0];
    *bits = vbits(with_nulls[0]);
    *off = with_nulls[0]->offset;
    return Status::OK();
  }
  AHC_RETURN_NOT_OK(s->AllocateBitmap(batch.num_rows, owner));
  uint8_t* ob = (uint8_t*)(*owner)->dptr;
  AHC_RETURN_NOT_OK(s->FromStatus(ah_bitmap_op(s->ctx(), AH_BIT_AND, vbits(with_nulls[0]), with_nulls[0]->offset, vbits(with_nulls[1]), with_nulls[1]->offset,
                                              ob, 0, batch.num_rows)));
  for (size_t i = 2; i < with_nulls.size(); i++)
    AHC_RETURN_NOT_OK(s->FromStatus(ah_bitmap_op(s->ctx(), AH_BIT_AND, ob, 0, vbits(with_nulls[i]), with_nulls[i]->offset, ob, 0, batch.num_rows)));
  *bits = ob;
  return Status::OK();
}

Status HashJoinImpl(ExecCtx* ctx, const FunctionOptions* o, const std::vector<Datum>& args, Datum* out) {
  const HashJoinOptions* opts = dynamic_cast<const HashJoinOptions*>(o);
  if (args[0].kind != DatumKind::Record || args[1].kind != DatumKind::Record)
    return Status::Make(StatusCode::Invalid, "hash_join: both arguments must be record batches");
  if (!opts || opts->LeftKeys.empty()) return Status::Make(StatusCode::Invalid, "hash_join: no keys (left_keys=<column>,...)");
  const std::vector<std::string>& lnames = opts->LeftKeys;
  const std::vector<std::string>& rnames = opts->RightKeys.empty() ? opts->LeftKeys : opts->RightKeys;
  if (lnames.size() > 8) return Status::Make(StatusCode::Invalid, "hash_join: more than 8 keys (" + std::to_string(lnames.size()) + ")");
  if (rnames.size() != lnames.size())
    return Status::Make(StatusCode::Invalid, "hash_join: " + std::to_string(lnames.size()) + " left keys but " + std::to_string(rnames.size()) + " right keys");
  JoinKind kind;
  const std::string& jt = opts->JoinType;
  if (jt.empty() || jt == "inner") kind = JoinKind::Inner;
  else if (jt == "left_outer") kind = JoinKind::LeftOuter;
  else if (jt == "left_semi") kind = JoinKind::LeftSemi;
  else if (jt == "left_anti") kind = JoinKind::LeftAnti;
  else return Status::Make(StatusCode::Invalid, "hash_join: unknown type '" + jt + "' (inner, left_outer, left_semi, left_anti)");
  const bool pairs = kind == JoinKind::Inner || kind == JoinKind::LeftOuter;
  Session* s = ctx->session;
  const Datum &left = args[0], &right = args[1];
  const int64_t n_left = left.num_rows, n_right = right.num_rows, n_all = n_left + n_right;
  auto column = [](const Datum& batch, const std::string& name) -> int {
    for (size_t i = 0; i < batch.names.size(); i++) if (batch.names[i] == name) return (int)i;
    return -1;
  };
  auto type_name = [](const ArrayData& a) { return a.logical.empty() ? std::string(a.type->name) + " [" + a.type->format + "]" : a.logical; };
  for (const Datum* b : {&left, &right})
    for (auto& c : b->chunks)
      if (c->on_host) return Status::Make(StatusCode::NotImplemented, "hash_join: host-resident columns are not taken; upload the batch first");
  // the keys, position by position: names, then types — no promotion, the bytes of both sides must mean the same
  std::vector<int> lcols, rcols;
  for (size_t k = 0; k < lnames.size(); k++) {
    const int li = column(left, lnames[k]), ri = column(right, rnames[k]);
    if (li < 0) return Status::Make(StatusCode::Invalid, "hash_join: unknown key column '" + lnames[k] + "' of the left batch");
    if (ri < 0) return Status::Make(StatusCode::Invalid, "hash_join: unknown key column '" + rnames[k] + "' of the right batch");
    lcols.push_back(li);
    rcols.push_back(ri);
  }
  for (size_t k = 0; k < lcols.size(); k++) {
    const ArrayData &l = *left.chunks[lcols[k]], &r = *right.chunks[rcols[k]];
    // a dictionary's indices are not its values: two indices may name equal values
    for (const ArrayData* a : {&l, &r})
      if (a->type->id == Type::DICTIONARY)
        return Status::Make(StatusCode::NotImplemented, "hash_join: dictionary-typed key column '" + (a == &l ? lnames[k] : rnames[k]) + "'; decode it first");
    const Type id = l.type->id;
    if (!(id == Type::BOOL || IsBaseBinary(id) || IsNumeric(id) || IsFixedWidthBinary(id)))
      return Status::Make(StatusCode::NotImplemented, "function 'hash_join' has no kernel matching input types (key: " + type_name(l) + ")");
    if (id != r.type->id || std::string(l.type->format) != r.type->format || l.logical != r.logical)
      return Status::Make(StatusCode::NotImplemented, "function 'hash_join' has no kernel matching input types (key '" + lnames[k] + "': " + type_name(l) +
                                                          ", key '" + rnames[k] + "': " + type_name(r) + "; cast one side first)");
  }
  // the result's columns: every left column, then the right columns that are not keys
  std::vector<int> rpayload;
  if (pairs) {
    for (size_t i = 0; i < right.names.size(); i++) {
      if (std::find(rcols.begin(), rcols.end(), (int)i) != rcols.end()) continue;
      if (column(left, right.names[i]) >= 0)
        return Status::Make(StatusCode::Invalid, "hash_join: column '" + right.names[i] + "' is on both sides and is not a key; rename one");
      rpayload.push_back((int)i);
    }
  }
  if (n_all > ((int64_t)1 << 30))
    return Status::Make(StatusCode::Invalid, "hash_join: " + std::to_string(n_all) + " rows on both sides together, more than 2^30");
  // one id space for both sides: rows [0, n_left) of the concatenated keys are the left side's
  BufferPtr ids, first_rows;
  AHC_RETURN_NOT_OK(s->Allocate((n_all > 0 ? n_all : 1) * 4, &ids, /*zero_all=*/false));
  int64_t ng = 0;
  if (n_all > 0) {
    AHC_RETURN_NOT_OK(s->Allocate((n_all + 1) * 8, &first_rows, /*zero_all=*/false));
    std::vector<ArrayDataPtr> both(lcols.size());
    std::vector<ah_group_key> gkeys;
    for (size_t k = 0; k < lcols.size(); k++) {
      AHC_RETURN_NOT_OK(Concatenate(s, {left.chunks[lcols[k]], right.chunks[rcols[k]]}, left.chunks[lcols[k]]->type, &both[k]));
      const ArrayData& a = *both[k];
      const Type id = a.type->id;
      ah_group_key g{};
      auto dptr = [&](int i) -> const uint8_t* { return a.buffers[i] ? (const uint8_t*)a.buffers[i]->dptr : nullptr; };
      if (id == Type::BOOL) { g.bits = 1; g.data = dptr(1); }
      else if (IsBaseBinary(id)) { g.offset_width = a.type->bit_width / 8; g.offsets = dptr(1); g.data = dptr(2); }
      else { g.byte_width = a.type->bit_width / 8; g.data = dptr(1); }
      g.valid = a.null_count != 0 ? dptr(0) : nullptr;
      g.off = a.offset;
      gkeys.push_back(g);
    }
    AHC_RETURN_NOT_OK(s->FromStatus(ah_group_ids(s->ctx(), (int)gkeys.size(), gkeys.data(), n_all, (int32_t*)ids->dptr, (int64_t*)first_rows->dptr, &ng)));
  }
  const int32_t *lids = (const int32_t*)ids->dptr, *rids = lids + n_left;
  BufferPtr lvalid_owner, rvalid_owner;
  const uint8_t *lvalid, *rvalid;
  int64_t loff, roff;
  AHC_RETURN_NOT_OK(JoinRowValidity(s, left, lcols, &lvalid_owner, &lvalid, &loff));
  AHC_RETURN_NOT_OK(JoinRowValidity(s, right, rcols, &rvalid_owner, &rvalid, &roff));
  // the right side by id
  BufferPtr starts, rows;
  AHC_RETURN_NOT_OK(s->Allocate((ng + 1) * 8, &starts, /*zero_all=*/false));
  AHC_RETURN_NOT_OK(s->Allocate((n_right > 0 ? n_right : 1) * 8, &rows, /*zero_all=*/false));
  AHC_RETURN_NOT_OK(s->FromStatus(ah_join_build(s->ctx(), rids, rvalid, roff, n_right, ng, (int64_t*)starts->dptr, (int64_t*)rows->dptr)));
  if (!pairs) {   // semi / anti: the left rows with / without a match, through the filter path
    BufferPtr bits;
    AHC_RETURN_NOT_OK(s->AllocateBitmap(n_left, &bits));
    AHC_RETURN_NOT_OK(s->FromStatus(ah_join_match_bits(s->ctx(), lids, lvalid, loff, n_left, (const int64_t*)starts->dptr, (uint8_t*)bits->dptr)));
    if (kind == JoinKind::LeftAnti && n_left > 0) {
      BufferPtr inverted;
      AHC_RETURN_NOT_OK(s->AllocateBitmap(n_left, &inverted));
      AHC_RETURN_NOT_OK(s->FromStatus(ah_copy_bitmap(s->ctx(), (const uint8_t*)bits->dptr, 0, n_left, (uint8_t*)inverted->dptr, 0, 1)));
      bits = inverted;
    }
    auto mask = std::make_shared<ArrayData>();
    mask->type = GetDataType(Type::BOOL);
    mask->length = n_left;
    mask->null_count = 0;
    mask->buffers[1] = bits;
    static const FilterOptions kDropNulls;
    return CallFunction(ctx, "filter", &kDropNulls, {left, Datum::Of(mask)}, out);
  }
  // inner / left outer: count, size the result, expand
  const int emit = kind == JoinKind::LeftOuter ? 1 : 0;
  BufferPtr offsets, lrows, rrows, rrows_valid;
  int64_t total = 0, unmatched = 0;
  AHC_RETURN_NOT_OK(s->Allocate((n_left + 1) * 8, &offsets, /*zero_all=*/false));
  AHC_RETURN_NOT_OK(s->FromStatus(ah_join_count(s->ctx(), lids, lvalid, loff, n_left, (const int64_t*)starts->dptr, emit, (int64_t*)offsets->dptr, &total)));
  if (total >= ((int64_t)1 << 31))
    return Status::Make(StatusCode::Invalid, "hash_join: the result has " + std::to_string(total) + " rows, more than 2^31 - 1");
  AHC_RETURN_NOT_OK(s->Allocate((total > 0 ? total : 1) * 8, &lrows, /*zero_all=*/false));
  AHC_RETURN_NOT_OK(s->Allocate((total > 0 ? total : 1) * 8, &rrows, /*zero_all=*/false));
  if (emit) AHC_RETURN_NOT_OK(s->AllocateBitmap(total, &rrows_valid));
  AHC_RETURN_NOT_OK(s->FromStatus(ah_join_expand(s->ctx(), lids, lvalid, loff, n_left, (const int64_t*)starts->dptr, (const int64_t*)rows->dptr,
                                                 (const int64_t*)offsets->dptr, total, emit, (int64_t*)lrows->dptr, (int64_t*)rrows->dptr,
                                                 emit ? (uint8_t*)rrows_valid->dptr : nullptr, emit ? &unmatched : nullptr)));
  auto index = [&](const BufferPtr& data) {
    auto idx = std::make_shared<ArrayData>();
    idx->type = GetDataType(Type::INT64);
    idx->length = total;
    idx->null_count = 0;
    idx->buffers[1] = data;
    return idx;
  };
  ArrayDataPtr lidx = index(lrows), ridx = index(rrows);
  if (unmatched) {   // an unmatched left row takes the right columns through Take's null-index path
    ridx->null_count = unmatched;
    ridx->buffers[0] = rrows_valid;
  }
  static const TakeOptions kNoBoundsCheck = [] { TakeOptions t; t.BoundsCheck = false; return t; }();
  std::vector<std::string> names;
  std::vector<ArrayDataPtr> cols;
  for (size_t i = 0; i < left.chunks.size(); i++) {
    Datum col;
    AHC_RETURN_NOT_OK(CallFunction(ctx, "array_take", &kNoBoundsCheck, {Datum::Of(left.chunks[i]), Datum::Of(lidx)}, &col));
    names.push_back(left.names[i]);
    cols.push_back(col.array);
  }
  for (int ci : rpayload) {
    Datum col;
    AHC_RETURN_NOT_OK(CallFunction(ctx, "array_take", &kNoBoundsCheck, {Datum::Of(right.chunks[ci]), Datum::Of(ridx)}, &col));
    names.push_back(right.names[ci]);
    cols.push_back(col.array);
  }
  *out = Datum::OfRecord(std::move(names), std::move(cols), total);
  return Status::OK();
}

}  // namespace

void RegisterHashJoin(FunctionRegistry* reg) {
  reg->AddFunction(std::make_shared<MetaFunction>("hash_join", Arity{2, false}, nullptr, HashJoinImpl), false);
}

// ---- fused extension (no reference analogue) --------------------------------
// "greater_filter_sum"(x, scalar) etc.: Σ x over valid slots with x OP scalar, as a 1-element
// array of x's type — what "greater" → "filter" → math.Sum computes in three calls.
void RegisterFusedExtensions(FunctionRegistry* reg) {
  struct F { const char* name; int op; };
  for (F f : {F{"equal_filter_sum", AH_CMP_EQ}, F{"not_equal_filter_sum", AH_CMP_NE}, F{"greater_filter_sum", AH_CMP_GT}, F{"greater_equal_filter_sum", AH_CMP_GE}}) {
    int op = f.op;
    reg->AddFunction(std::make_shared<MetaFunction>(f.name, Arity{2, false}, nullptr,
        [op](ExecCtx* ctx, const FunctionOptions*, const std::vector<Datum>& args, Datum* out) {
          Session* s = ctx->session;
          if (args[0].kind != DatumKind::Array || args[1].kind != DatumKind::Scalar)
            return Status::Make(StatusCode::Invalid, "fused compare-filter-sum needs (array, scalar)");
          const ArrayData& a = *args[0].array;
          if (a.type->id != args[1].scalar->type->id) return Status::Make(StatusCode::TypeError, "operand types differ");
          if (!args[1].scalar->valid) return Status::Make(StatusCode::Invalid, "null threshold");
          auto sc = std::make_shared<Scalar>();
          sc->type = a.type;
          sc->valid = true;
          const uint8_t* valid = a.buffers[0] ? (const uint8_t*)a.buffers[0]->dptr : nullptr;
          const uint8_t* vals = a.length ? (const uint8_t*)a.buffers[1]->dptr + a.offset * 8 : nullptr;
          int64_t cnt = 0;
          if (a.type->id == Type::INT64) {
            int64_t thr, sum = 0; memcpy(&thr, args[1].scalar->value, 8);
            AHC_RETURN_NOT_OK(s->FromStatus(ah_cmp_filter_sum_i64(s->ctx(), op, (const int64_t*)vals, valid, a.offset, a.length, thr, &sum, &cnt)));
            memcpy(sc->value, &sum, 8);
          } else if (a.type->id == Type::FLOAT64) {
            double thr, sum = 0; memcpy(&thr, args[1].scalar->value, 8);
            AHC_RETURN_NOT_OK(s->FromStatus(ah_cmp_filter_sum_f64(s->ctx(), op, (const double*)vals, valid, a.offset, a.length, thr, &sum, &cnt)));
            memcpy(sc->value, &sum, 8);
          } else {
            return Status::Make(StatusCode::NotImplemented, "fused compare-filter-sum is implemented for int64 and float64");
          }
          *out = Datum::Of(sc);
          return Status::OK();
        }), false);
  }
}

// ---- window / rank (no reference analogue: arrow-go has no window operator) ---------------------------------------
// window: one RecordDatum in, one out with the SAME rows in the same order and one column per function.  Five steps: dense partition
// ids (ah_group_ids), the stable order of (partition id, order keys) (ah_sort_indices_keys; skipped when there is neither), the
// partition / peer flags of that order (ah_window_flags), one ah_window_rank / ah_window_scan per function, and for the running
// aggregates the input column's validity copied (ah_copy_bitmap): an output row is null exactly where the input value is.
// rank: the same without partitions over one array or one record batch's sort keys.
namespace {

constexpr int64_t kWindowMaxRows = (int64_t)1 << 30;

// the order of `keys` (column indices into `cols`, the partition ids in front when given) and its flags
Status WindowOrderAndFlags(Session* s, const char* fn, const std::vector<Datum>& cols, const std::vector<SortKey>& keys_in, const BufferPtr& ids,
                           int64_t n, BufferPtr* order_buf, BufferPtr* flags_buf) {
  std::vector<Datum> args = cols;
  std::vector<SortKey> keys;
  if (ids) {
    auto col = std::make_shared<ArrayData>();
    col->type = GetDataType(Type::INT32);
    col->length = n;
    col->null_count = 0;
    col->buffers[1] = ids;
    SortKey k;
    k.ColumnIndex = (int)args.size();
    args.push_back(Datum::Of(col));
    keys.push_back(k);
  }
  keys.insert(keys.end(), keys_in.begin(), keys_in.end());
  std::vector<ah_sort_key> skeys;
  const uint64_t* order = nullptr;
  if (!keys.empty()) {
    std::vector<Datum> flat;
    int64_t length = 0;
    AHC_RETURN_NOT_OK(PrepareSortKeys(s, fn, keys, args, &flat, &skeys, &length));
    AHC_RETURN_NOT_OK(s->Allocate(n * 8, order_buf, /*zero_all=*/false));
    AHC_RETURN_NOT_OK(s->FromStatus(ah_sort_indices_keys(s->ctx(), (int)skeys.size(), skeys.data(), n, (uint64_t*)(*order_buf)->dptr)));
    order = (const uint64_t*)(*order_buf)->dptr;
  }
  const size_t first = ids ? 1 : 0;   // the flags compare the order keys; the partition id has its own bit
  AHC_RETURN_NOT_OK(s->Allocate(n, flags_buf, /*zero_all=*/false));
  return s->FromStatus(ah_window_flags(s->ctx(), ids ? (const int32_t*)ids->dptr : nullptr, (int)(skeys.size() - first), skeys.data() + first, order, n,
                                       (uint8_t*)(*flags_buf)->dptr));
}

Status WindowImpl(ExecCtx* ctx, const FunctionOptions* o, const std::vector<Datum>& args, Datum* out) {
  const WindowOptions* opts = dynamic_cast<const WindowOptions*>(o);
  if (args[0].kind != DatumKind::Record) return Status::Make(StatusCode::Invalid, "window: the argument must be a record batch");
  if (!opts || opts->Functions.empty())
    return Status::Make(StatusCode::Invalid, "window: no functions (functions=row_number,rank,dense_rank,cumulative_sum:<column>,...)");
  if (opts->PartitionBy.size() > 8)
    return Status::Make(StatusCode::Invalid, "window: more than 8 partition columns (" + std::to_string(opts->PartitionBy.size()) + ")");
  if (opts->OrderBy.size() > 7)   // the partition id is the sort's first key, and the sort takes 8
    return Status::Make(StatusCode::Invalid, "window: more than 7 order keys (" + std::to_string(opts->OrderBy.size()) + ")");
  Session* s = ctx->session;
  const Datum& batch = args[0];
  const int64_t n = batch.num_rows;
  if (n > kWindowMaxRows) return Status::Make(StatusCode::Invalid, "window: " + std::to_string(n) + " rows, more than 2^30");
  auto column = [&](const std::string& name) -> int {
    for (size_t i = 0; i < batch.names.size(); i++) if (batch.names[i] == name) return (int)i;
    return -1;
  };
  auto no_kernel = [](const std::string& what, const ArrayData& a) {
    return Status::Make(StatusCode::NotImplemented, "function 'window' has no kernel matching input types (" + what + ": " +
                                                        (a.logical.empty() ? std::string(a.type->name) : a.logical) + ")");
  };
  for (auto& c : batch.chunks)
    if (c->on_host) return Status::Make(StatusCode::NotImplemented, "window: host-resident columns are not taken; upload the batch first");
  // everything named is checked before anything runs
  std::vector<ah_group_key> pkeys;
  for (auto& name : opts->PartitionBy) {
    const int ci = column(name);
    if (ci < 0) return Status::Make(StatusCode::KeyError, "window: unknown partition column '" + name + "'");
    const ArrayData& a = *batch.chunks[ci];
    if (a.type->id == Type::DICTIONARY)
      return Status::Make(StatusCode::NotImplemented, "window: dictionary-typed partition column '" + name + "'; decode it first");
    ah_group_key k{};
    if (!GroupKeyOf(a, &k)) return no_kernel("partition column '" + name + "'", a);
    pkeys.push_back(k);
  }
  std::vector<SortKey> okeys;
  for (auto& key : opts->OrderBy) {
    const int ci = column(key.Column);
    if (ci < 0) return Status::Make(StatusCode::KeyError, "window: unknown order column '" + key.Column + "'");
    SortKey k;
    k.ColumnIndex = ci;
    k.Order = key.Order;
    k.Placement = key.Placement;
    okeys.push_back(k);
  }
  struct Plan { int kind; int column; std::string name; };   // kind: 0 … 2 ah_window_rank's, 10 + ah_window_scan's op
  std::vector<Plan> plan;
  for (auto& f : opts->Functions) {
    Plan p{-1, -1, ""};
    if (f.Function == "row_number") p.kind = AH_WINDOW_ROW_NUMBER;
    else if (f.Function == "rank") p.kind = AH_WINDOW_RANK;
    else if (f.Function == "dense_rank") p.kind = AH_WINDOW_DENSE_RANK;
    else if (f.Function == "cumulative_sum") p.kind = 10 + AH_WINDOW_SUM;
    else if (f.Function == "cumulative_min") p.kind = 10 + AH_WINDOW_MIN;
    else if (f.Function == "cumulative_max") p.kind = 10 + AH_WINDOW_MAX;
    else if (f.Function == "cumulative_count") p.kind = 10 + AH_WINDOW_COUNT;
    else return Status::Make(StatusCode::Invalid, "window: unknown function '" + f.Function + "'");
    if (p.kind < 10) {
      if (!f.Column.empty()) return Status::Make(StatusCode::Invalid, "window: " + f.Function + " takes no column, got '" + f.Column + "'");
      p.name = f.Function;
    } else {
      if (f.Column.empty()) return Status::Make(StatusCode::Invalid, "window: " + f.Function + " needs a column ('" + f.Function + ":<column>')");
      p.column = column(f.Column);
      if (p.column < 0) return Status::Make(StatusCode::KeyError, "window: unknown column '" + f.Column + "' of function '" + f.Function + "'");
      const ArrayData& a = *batch.chunks[p.column];
      if (!IsNumeric(a.type->id) || (p.kind == 10 + AH_WINDOW_SUM && !a.logical.empty())) return no_kernel(f.Function + " of column '" + f.Column + "'", a);
      p.name = f.Column + "_" + f.Function;
    }
    for (auto& q : plan)
      if (q.name == p.name) return Status::Make(StatusCode::Invalid, "window: two output columns named '" + p.name + "'");
    plan.push_back(p);
  }
  // 1. partition ids   2. the order   3. the flags
  BufferPtr ids, first_rows, order_buf, flags_buf;
  if (n > 0) {
    if (!pkeys.empty()) {
      int64_t ng = 0;
      AHC_RETURN_NOT_OK(s->Allocate(n * 4, &ids, /*zero_all=*/false));
      AHC_RETURN_NOT_OK(s->Allocate((n + 1) * 8, &first_rows, /*zero_all=*/false));
      AHC_RETURN_NOT_OK(s->FromStatus(ah_group_ids(s->ctx(), (int)pkeys.size(), pkeys.data(), n, (int32_t*)ids->dptr, (int64_t*)first_rows->dptr, &ng)));
      first_rows.reset();
    }
    std::vector<Datum> cols;
    for (auto& c : batch.chunks) cols.push_back(Datum::Of(c));
    AHC_RETURN_NOT_OK(WindowOrderAndFlags(s, "window", cols, okeys, ids, n, &order_buf, &flags_buf));
  } else {   // nothing runs, but a key the sort would refuse is refused all the same
    for (auto& k : okeys) {
      const ArrayData& a = *batch.chunks[k.ColumnIndex];
      const Type id = a.type->id;
      if (!(IsInteger(id) || IsFloating(id) || IsBaseBinary(id) || IsFixedWidthBinary(id)))
        return Status::Make(StatusCode::NotImplemented, std::string("sorting not supported for type ") + a.type->name);
    }
  }
  const uint8_t* flags = flags_buf ? (const uint8_t*)flags_buf->dptr : nullptr;
  const uint64_t* order = order_buf ? (const uint64_t*)order_buf->dptr : nullptr;
  // 4. one call per function   5. the validity of the running aggregates
  const int64_t room = n > 0 ? n : 1;
  std::vector<std::string> names;
  std::vector<ArrayDataPtr> cols_out;
  for (auto& p : plan) {
    auto col = std::make_shared<ArrayData>();
    col->length = n;
    col->null_count = 0;
    if (p.kind < 10) {
      col->type = GetDataType(Type::UINT64);
      AHC_RETURN_NOT_OK(s->Allocate(room * 8, &col->buffers[1], /*zero_all=*/false));
      AHC_RETURN_NOT_OK(s->FromStatus(ah_window_rank(s->ctx(), p.kind, flags, order, n, (uint64_t*)col->buffers[1]->dptr)));
    } else {
      const int op = p.kind - 10;
      const ArrayData& a = *batch.chunks[p.column];
      const Type id = a.type->id;
      const int width = a.type->bit_width / 8;
      const uint8_t* vvalid = a.buffers[0] && a.null_count != 0 ? (const uint8_t*)a.buffers[0]->dptr : nullptr;
      const uint8_t* vals = a.buffers[1] ? (const uint8_t*)a.buffers[1]->dptr + a.offset * width : nullptr;
      int out_width = width;
      if (op == AH_WINDOW_SUM) {
        col->type = GetDataType(IsFloating(id) ? Type::FLOAT64 : IsSignedInteger(id) ? Type::INT64 : Type::UINT64);
        out_width = 8;
      } else if (op == AH_WINDOW_COUNT) {
        col->type = GetDataType(Type::INT64);
        out_width = 8;
      } else {
        col->type = a.type;
        col->logical = a.logical;
      }
      AHC_RETURN_NOT_OK(s->Allocate(room * out_width, &col->buffers[1], /*zero_all=*/false));
      AHC_RETURN_NOT_OK(s->FromStatus(ah_window_scan(s->ctx(), op, (int)id, vals, vvalid, a.offset, flags, order, n, col->buffers[1]->dptr)));
      if (vvalid && op != AH_WINDOW_COUNT && n > 0) {
        AHC_RETURN_NOT_OK(s->Allocate((n + 7) / 8, &col->buffers[0], /*zero_all=*/false));
        AHC_RETURN_NOT_OK(s->FromStatus(ah_copy_bitmap(s->ctx(), vvalid, a.offset, n, (uint8_t*)col->buffers[0]->dptr, 0, 0)));
        col->null_count = a.null_count;
        if (col->null_count < 0) {
          ArraySpan span;
          span.type = GetDataType(Type::BOOL);
          span.len = n;
          span.offset = 0;
          span.buffers[0].WrapBuffer(col->buffers[0]);
          AHC_RETURN_NOT_OK(span.UpdateNullCount(s, &col->null_count));
        }
      }
    }
    names.push_back(p.name);
    cols_out.push_back(col);
  }
  *out = Datum::OfRecord(std::move(names), std::move(cols_out), n);
  return Status::OK();
}

Status RankImpl(ExecCtx* ctx, const FunctionOptions* o, const std::vector<Datum>& args_in, Datum* out) {
  const RankOptions* opts = dynamic_cast<const RankOptions*>(o);
  if (!opts || opts->Keys.empty()) return Status::Make(StatusCode::Invalid, "rank: must provide at least one sort key");
  const std::string& tb = opts->Tiebreaker;
  int kind;
  if (tb.empty() || tb == "min") kind = AH_WINDOW_RANK;
  else if (tb == "first") kind = AH_WINDOW_ROW_NUMBER;
  else if (tb == "dense") kind = AH_WINDOW_DENSE_RANK;
  else if (tb == "max") return Status::Make(StatusCode::NotImplemented, "rank: tiebreaker=max is not implemented (min, first or dense)");
  else return Status::Make(StatusCode::Invalid, "rank: unknown tiebreaker '" + tb + "' (min, first or dense)");
  Session* s = ctx->session;
  // the arguments as the sort flattens them, so that a chunked column is concatenated once
  std::vector<Datum> flat;
  std::vector<ah_sort_key> checked;
  int64_t n = 0;
  AHC_RETURN_NOT_OK(PrepareSortKeys(s, "rank", opts->Keys, args_in, &flat, &checked, &n));
  if (n > kWindowMaxRows) return Status::Make(StatusCode::Invalid, "rank: " + std::to_string(n) + " rows, more than 2^30");
  std::vector<SortKey> keys = opts->Keys;
  if (flat.size() == 1) { keys.resize(1); keys[0].ColumnIndex = 0; }
  std::shared_ptr<ArrayData> res;
  AHC_RETURN_NOT_OK(AllocateIndices(s, n, &res));
  if (n > 0) {
    BufferPtr order_buf, flags_buf;
    AHC_RETURN_NOT_OK(WindowOrderAndFlags(s, "rank", flat, keys, nullptr, n, &order_buf, &flags_buf));
    AHC_RETURN_NOT_OK(s->FromStatus(ah_window_rank(s->ctx(), kind, (const uint8_t*)flags_buf->dptr, (const uint64_t*)order_buf->dptr, n,
                                                   (uint64_t*)res->buffers[1]->dptr)));
  }
  *out = Datum::Of(res);
  return Status::OK();
}

}  // namespace

void RegisterWindow(FunctionRegistry* reg) {
  reg->AddFunction(std::make_shared<MetaFunction>("window", Arity{1, false}, nullptr, WindowImpl), false);
  // Arity: one array, or the columns of a record batch as separate arguments, as sort_indices
  reg->AddFunction(std::make_shared<MetaFunction>("rank", Arity{1, true}, nullptr, RankImpl), false);
}

// ---- conditionals: if_else, coalesce, fill_null, fill_null_forward, fill_null_backward -------------------------------
// No reference analogue (arrow-go registers none of them); the semantics are Arrow C++'s.  if_else: row i is null where cond[i] is null,
// otherwise left[i] or right[i] with that side's validity.  coalesce: the first valid value of the row.  The directed fills: a null
// row takes the nearest valid row before / after it.  Any argument may be an array or a scalar; a scalar is a one-row device column
// every row reads (ah_cond_side.broadcast).
namespace {

constexpr int kForward = 0, kBackward = 1;

// the value types: every type the take of this layer accepts, dictionaries left out
std::vector<Type> ConditionalValueTypes() {
  std::vector<Type> t(std::begin(kNumericTypes), std::end(kNumericTypes));
  t.push_back(Type::BOOL);
  t.insert(t.end(), std::begin(kBinaryTypes), std::end(kBinaryTypes));
  for (Type f : {Type::FIXED_SIZE_BINARY, Type::DECIMAL128, Type::DECIMAL256}) t.push_back(f);
  return t;
}

// the bits a call reads its condition from
struct CondBits {
  const uint8_t* data = nullptr;
  const uint8_t* valid = nullptr;
  int64_t off = 0;
};

// one side as ah_if_else takes it, with the array that owns its buffers
struct CondSide {
  ah_cond_side s;
  ArrayDataPtr keep;
};
Status SideOf(Session* s, const Datum& d, CondSide* out) {
  const bool broadcast = d.kind == DatumKind::Scalar;
  if (broadcast) AHC_RETURN_NOT_OK(ScalarToArray(s, *d.scalar, &out->keep));
  else out->keep = d.array;
  const ArrayData& a = *out->keep;
  auto dptr = [&](int i) -> const void* { return a.buffers[i] ? a.buffers[i]->dptr : nullptr; };
  out->s = ah_cond_side{};
  if (IsBaseBinary(a.type->id)) {
    out->s.offset_width = a.type->bit_width / 8;
    out->s.offsets = dptr(1);
    out->s.data = dptr(2);
  } else {
    out->s.byte_width = a.type->bit_width / 8;   // (Boolean: 0, the data is a bitmap)
    out->s.data = dptr(1);
  }
  out->s.valid = a.null_count != 0 ? (const uint8_t*)dptr(0) : nullptr;
  out->s.off = a.offset;
  out->s.broadcast = broadcast ? 1 : 0;
  return Status::OK();
}

// n rows chosen by the condition's bits from two sides of one type.  Fixed-width and Boolean sides: one launch, no synchronisation,
// the null count left to whoever asks for it; var-length sides: the offsets call brings the byte count home.
Status IfElseRows(Session* s, const CondBits& c, const Datum& left, const Datum& right, int64_t n, Datum* out) {
  CondSide l, r;
  AHC_RETURN_NOT_OK(SideOf(s, left, &l));
  AHC_RETURN_NOT_OK(SideOf(s, right, &r));
  const DataType* t = l.keep->type;
  auto res = std::make_shared<ArrayData>();
  res->type = t;
  res->length = n;
  res->logical = l.keep->logical;
  const bool nulls = c.valid || l.s.valid || r.s.valid;
  res->null_count = nulls ? kUnknownNullCount : 0;
  if (nulls) AHC_RETURN_NOT_OK(s->AllocateBitmap(n, &res->buffers[0]));
  uint8_t* ov = nulls ? (uint8_t*)res->buffers[0]->dptr : nullptr;
  if (t->id == Type::BOOL) {
    AHC_RETURN_NOT_OK(s->AllocateBitmap(n, &res->buffers[1]));
    AHC_RETURN_NOT_OK(s->FromStatus(ah_if_else_boolean(s->ctx(), c.data, c.valid, c.off, &l.s, &r.s, n, (uint8_t*)res->buffers[1]->dptr, ov)));
  } else if (IsBaseBinary(t->id)) {
    const int ow = t->bit_width / 8;
    int64_t total = 0;
    AHC_RETURN_NOT_OK(s->Allocate((n + 1) * ow, &res->buffers[1]));
    AHC_RETURN_NOT_OK(s->FromStatus(ah_if_else_binary_offsets(s->ctx(), c.data, c.valid, c.off, &l.s, &r.s, n, ow, res->buffers[1]->dptr, ov, &total)));
    AHC_RETURN_NOT_OK(s->Allocate(total, &res->buffers[2], /*zero_all=*/false));
    AHC_RETURN_NOT_OK(s->FromStatus(ah_if_else_binary_data(s->ctx(), c.data, c.valid, c.off, &l.s, &r.s, n, ow, res->buffers[1]->dptr, (uint8_t*)res->buffers[2]->dptr)));
  } else {
    AHC_RETURN_NOT_OK(s->Allocate(n * (t->bit_width / 8), &res->buffers[1], /*zero_all=*/false));   // every slot is written
    AHC_RETURN_NOT_OK(s->FromStatus(ah_if_else(s->ctx(), c.data, c.valid, c.off, &l.s, &r.s, n, res->buffers[1]->dptr, ov)));
  }
  *out = Datum::Of(res);
  return Status::OK();
}

// n null rows of a type: zero payload, zero lengths
Status AllNullRows(Session* s, const DataType* t, const std::string& logical, int64_t n, Datum* out) {
  auto res = std::make_shared<ArrayData>();
  res->type = t;
  res->length = n;
  res->null_count = n;
  res->logical = logical;
  AHC_RETURN_NOT_OK(s->AllocateBitmap(n, &res->buffers[0]));
  if (t->id == Type::BOOL) AHC_RETURN_NOT_OK(s->AllocateBitmap(n, &res->buffers[1]));
  else if (IsBaseBinary(t->id)) {
    AHC_RETURN_NOT_OK(s->Allocate((n + 1) * (t->bit_width / 8), &res->buffers[1]));
    AHC_RETURN_NOT_OK(s->Allocate(0, &res->buffers[2]));
  } else AHC_RETURN_NOT_OK(s->Allocate(n * (t->bit_width / 8), &res->buffers[1]));
  *out = Datum::Of(res);
  return Status::OK();
}

// a scalar as a column of n rows: if_else over a condition of n zero bits with the scalar on both sides
Status BroadcastRows(Session* s, const Datum& scalar, int64_t n, Datum* out) {
  BufferPtr zeros;
  AHC_RETURN_NOT_OK(s->AllocateBitmap(n, &zeros));
  CondBits c;
  c.data = (const uint8_t*)zeros->dptr;
  return IfElseRows(s, c, scalar, scalar, n, out);
}

std::string ValueTypeText(const DataType* t) { return IsFixedWidthBinary(t->id) ? std::string(t->name) + "[" + t->format + "]" : std::string(t->name); }

// A scalar function of this family: dispatch as every scalar function (DispatchBest with promote_from: the VALUE arguments go to
// their common numeric type by the rule `add` uses, every other pairing must match exactly), the implicit safe casts, and then the
// family's own executor — the arguments arrive as arrays or scalars of one value type, chunked columns already concatenated
// (ExecuteChunked) and re-chunked behind it.
class ConditionalFunction : public ScalarFunction {
 public:
  using Impl = std::function<Status(Session*, const std::vector<Datum>&, int64_t, Datum*)>;   // (session, arguments, rows or −1: all scalars, result)
  ConditionalFunction(std::string name, Arity arity, int first_value, Impl impl) : ScalarFunction(std::move(name), arity), impl_(std::move(impl)) {
    promote_from = first_value;
    for (Type t : ConditionalValueTypes()) {
      exec::ScalarKernel k;
      for (int i = 0; i < arity.NArgs; i++) k.sig.in_types.push_back(i < first_value ? Type::BOOL : t);
      k.sig.out_is_first_input = false;
      k.sig.out_type = t;
      k.exec_fn = [](KernelCtx*, const ExecSpan&, ExecResult*) { return Status::Make(StatusCode::NotImplemented, "the conditionals run through their function's executor"); };
      AddKernel(std::move(k));
    }
  }
  Status Execute(ExecCtx* ctx, const FunctionOptions*, const std::vector<Datum>& args_in, Datum* out) override {
    AHC_RETURN_NOT_OK(CheckArity(args_in.size()));
    Session* s = ctx ? ctx->session : nullptr;
    if (!s) return Status::Make(StatusCode::Invalid, "ExecCtx has no device session");
    std::vector<Datum> args = args_in;
    std::vector<const DataType*> types;
    for (auto& a : args) {
      if (a.kind != DatumKind::Array && a.kind != DatumKind::Scalar) return Status::Make(StatusCode::NotImplemented, "function '" + name_ + "' takes arrays, chunked arrays and scalars");
      types.push_back(a.type());
    }
    const std::vector<const DataType*> given = types;
    const exec::ScalarKernel* kernel = nullptr;
    AHC_RETURN_NOT_OK(DispatchBest(&types, &kernel));
    for (size_t i = 0; i < args.size(); i++) {   // the implicit casts are SAFE casts (execInternal, exec.go:105-114)
      if (args[i].type()->id == types[i]->id) continue;
      Datum casted;
      AHC_RETURN_NOT_OK(CastDatum(ctx, args[i], CastOptions::Safe(types[i]), &casted));
      args[i] = casted;
    }
    // parametric value types (decimal precision and scale, the width of a fixed-size binary) match exactly too
    for (size_t i = (size_t)promote_from + 1; i < args.size(); i++)
      if (args[i].type() != args[promote_from].type() && strcmp(args[i].type()->format, args[promote_from].type()->format) != 0) {
        std::string text = "(";
        for (size_t j = 0; j < given.size(); j++) text += std::string(j ? ", " : "") + ValueTypeText(given[j]);
        return Status::Make(StatusCode::NotImplemented, "function '" + name_ + "' has no kernel matching input types " + text + ")");
      }
    int64_t n = -1;   // inferBatchLength (executor.go:352-390)
    for (auto& a : args) {
      if (a.kind != DatumKind::Array) continue;
      if (n < 0) n = a.array->length;
      else if (n != a.array->length) return Status::Make(StatusCode::Invalid, "array arguments must all be the same length");
    }
    return impl_(s, args, n, out);
  }
 private:
  Impl impl_;
};

Status IfElseImpl(Session* s, const std::vector<Datum>& args, int64_t n, Datum* out) {
  const Datum& cond = args[0];
  if (cond.kind == DatumKind::Scalar) {   // decided here: one side is the result
    const Datum& side = (cond.scalar->value[0] & 1) ? args[1] : args[2];
    if (n < 0) {   // all scalars: a scalar
      if (cond.scalar->valid) { *out = side; return Status::OK(); }
      auto sc = std::make_shared<Scalar>(*args[1].scalar);
      sc->valid = false;
      memset(sc->value, 0, sizeof(sc->value));
      sc->bytes.clear();
      *out = Datum::Of(sc);
      return Status::OK();
    }
    if (!cond.scalar->valid) {
      const Datum& any = args[1].kind == DatumKind::Array ? args[1] : args[2];
      return AllNullRows(s, args[1].type(), any.array->logical, n, out);
    }
    if (side.kind == DatumKind::Array) { *out = side; return Status::OK(); }
    return BroadcastRows(s, side, n, out);
  }
  const ArrayData& c = *cond.array;
  CondBits bits;
  bits.data = c.buffers[1] ? (const uint8_t*)c.buffers[1]->dptr : nullptr;
  bits.valid = c.buffers[0] && c.null_count != 0 ? (const uint8_t*)c.buffers[0]->dptr : nullptr;
  bits.off = c.offset;
  return IfElseRows(s, bits, args[1], args[2], n, out);
}

// coalesce(x1 … xk) = if_else(is_valid(x1), x1, coalesce(x2 … xk)): a right fold of if_else whose condition is the left argument's
// validity bitmap at its offset.  A left argument without nulls is the result as it is, a null scalar leaves the rest.
Status CoalesceImpl(Session* s, const std::vector<Datum>& args, int64_t n, Datum* out) {
  Datum acc = args.back();
  for (size_t i = args.size() - 1; i-- > 0;) {
    const Datum& x = args[i];
    if (x.kind == DatumKind::Scalar) {
      if (x.scalar->valid) acc = x;
      continue;
    }
    exec::ArraySpan span;
    span.SetMembers(*x.array);
    AHC_RETURN_NOT_OK(span.UpdateNullCount(s));
    if (span.nulls == 0) { acc = x; continue; }
    x.array->null_count = span.nulls;
    CondBits bits;
    bits.data = (const uint8_t*)x.array->buffers[0]->dptr;
    bits.off = x.array->offset;
    AHC_RETURN_NOT_OK(IfElseRows(s, bits, x, acc, n, &acc));
  }
  if (acc.kind == DatumKind::Scalar && n >= 0) return BroadcastRows(s, acc, n, out);
  *out = acc;
  return Status::OK();
}

// fill_null_forward / fill_null_backward: the fused entry for values of 1 / 2 / 4 / 8 / 16 / 32 bytes; Boolean, var-length and
// other widths through ah_fill_null_indices and the Take of their layout.  A column without nulls is returned as it is.  A chunked
// column arrives concatenated (ExecuteChunked), so the carry crosses the chunk borders, and leaves re-chunked like the input.
Status ExecFillDirected(KernelCtx* k, const ExecSpan& b, ExecResult* out, int direction) {
  Session* s = k->session;
  ArraySpan in = b.values[0].array;
  AHC_RETURN_NOT_OK(in.UpdateNullCount(s));
  const int64_t n = in.len;
  if (in.nulls == 0 || n == 0) {
    *out = in;
    out->nulls = 0;
    return Status::OK();
  }
  const int w = in.type->bit_width / 8;
  const bool fixed = in.type->id != Type::BOOL && !IsBaseBinary(in.type->id);
  if (fixed) AHC_RETURN_NOT_OK(CheckSlotWidth(in));
  const bool word_aligned = fixed && (((uintptr_t)in.buffers[1].buf) & (uintptr_t)((w < 8 ? w : 8) - 1)) == 0;
  if (fixed && word_aligned && (w == 1 || w == 2 || w == 4 || w == 8 || w == 16 || w == 32)) {
    BufferPtr vb, db;
    AHC_RETURN_NOT_OK(k->AllocateBitmap(n, &vb));
    AHC_RETURN_NOT_OK(k->Allocate(n * w, &db, /*zero_all=*/false));
    int64_t nulls = 0;
    AHC_RETURN_NOT_OK(s->FromStatus(ah_fill_null_directed(s->ctx(), w, in.buffers[1].buf, in.buffers[0].buf, in.offset, n, direction, db->dptr, (uint8_t*)vb->dptr, &nulls)));
    out->len = n;
    out->offset = 0;
    out->buffers[0].WrapBuffer(vb);
    out->buffers[1].WrapBuffer(db);
    out->nulls = nulls;
    return Status::OK();
  }
  IndexOperand ix;
  ix.width = 4;
  ix.len = n;
  AHC_RETURN_NOT_OK(s->Allocate(n * 4, &ix.data_buf, /*zero_all=*/false));
  AHC_RETURN_NOT_OK(s->AllocateBitmap(n, &ix.valid_buf));
  AHC_RETURN_NOT_OK(s->FromStatus(ah_fill_null_indices(s->ctx(), in.buffers[0].buf, in.offset, n, direction, (uint32_t*)ix.data_buf->dptr, (uint8_t*)ix.valid_buf->dptr, &ix.nulls)));
  ix.data = ix.data_buf->dptr;
  ix.valid = ix.nulls ? (const uint8_t*)ix.valid_buf->dptr : nullptr;
  // the sources are valid rows: the output has a null exactly where an index slot is null
  if (in.type->id == Type::BOOL) return TakeBooleanCommon(k, in, ix, ix.nulls != 0, out);
  if (!fixed) return TakeBinaryCommon(k, in, ix, ix.nulls != 0, out);
  return TakeFixedCommon(k, in, ix, ix.nulls != 0, /*bounds_check=*/0, out);
}

}  // namespace

void RegisterConditional(FunctionRegistry* reg) {
  reg->AddFunction(std::make_shared<ConditionalFunction>("if_else", Arity{3, false}, 1, IfElseImpl), false);
  reg->AddFunction(std::make_shared<ConditionalFunction>("coalesce", Arity{1, true}, 0, CoalesceImpl), false);
  reg->AddFunction(std::make_shared<ConditionalFunction>("fill_null", Arity{2, false}, 0, CoalesceImpl), false);
  for (int direction : {kForward, kBackward}) {
    auto fn = std::make_shared<VectorFunction>(direction == kForward ? "fill_null_forward" : "fill_null_backward", Arity{1, false});
    for (Type t : ConditionalValueTypes()) {
      exec::VectorKernel k;
      k.sig.in_types = {t};
      k.exec_fn = [direction](KernelCtx* c, const ExecSpan& b, ExecResult* o) { return ExecFillDirected(c, b, o, direction); };
      k.can_execute_chunkwise = false;   // the carry crosses chunk borders
      fn->AddKernel(std::move(k));
    }
    reg->AddFunction(fn, false);
  }
}

// ---- string predicates: match_substring, starts_with, ends_with, find_substring, match_like, binary_length, utf8_length ----------------
// No reference analogue (arrow-go has none of them): Arrow C++'s functions and semantics, DESIGN.md §3.17.  One argument, an array or
// a chunked array (a chunk at a time, like every scalar function); the output's validity is the input's (NullIntersection).  The
// kernels compute every row, null slots included.
namespace {

enum StringFn { kFnSubstring = AH_STR_SUBSTRING, kFnStartsWith = AH_STR_STARTS_WITH, kFnEndsWith = AH_STR_ENDS_WITH, kFnFind, kFnLike, kFnBinaryLength, kFnUtf8Length };

Status ExecStringMatch(KernelCtx* k, const ExecSpan& b, ExecResult* out, const char* name, int fn) {
  Session* s = k->session;
  const bool needs_pattern = fn != kFnBinaryLength && fn != kFnUtf8Length;
  const MatchSubstringOptions* opts = nullptr;
  if (needs_pattern) {
    const FunctionOptions* given = static_cast<const FunctionOptions*>(k->state);
    AHC_RETURN_NOT_OK(ValidateStringMatchOptions(name, given));
    opts = static_cast<const MatchSubstringOptions*>(given);
  }
  if (out->len == 0) return Status::OK();   // (a scalar argument never gets here: ScalarFunction::arrays_only)
  const ArraySpan& in = b.values[0].array;
  const ByteLayout l = LayoutOf(in);
  const ah_cmp_operand col{l.offset_width, l.byte_width, l.offsets, l.data, l.offset, 0};
  const uint8_t* pattern = opts ? (const uint8_t*)opts->Pattern.data() : nullptr;
  const int64_t m = opts ? (int64_t)opts->Pattern.size() : 0;
  const int out_width = in.type->id == Type::LARGE_STRING || in.type->id == Type::LARGE_BINARY ? 8 : 4;
  switch (fn) {
    case kFnFind:
      return s->FromStatus(ah_string_find(s->ctx(), &col, out->len, pattern, m, out_width, out->buffers[1].buf + out->offset * out_width));
    case kFnLike: {
      const std::vector<uint8_t> program = like::Compile(pattern, (size_t)m);
      return s->FromStatus(ah_string_like(s->ctx(), &col, out->len, IsUtf8(in.type->id) ? 1 : 0, program.data(), (int64_t)program.size(), out->buffers[1].buf, out->offset));
    }
    case kFnBinaryLength:
    case kFnUtf8Length:
      return s->FromStatus(ah_string_length(s->ctx(), &col, out->len, fn == kFnUtf8Length ? 1 : 0, out_width, out->buffers[1].buf + out->offset * out_width));
    default:
      return s->FromStatus(ah_string_match(s->ctx(), fn, &col, out->len, pattern, m, out->buffers[1].buf, out->offset));
  }
}

}  // namespace

Status ValidateStringMatchOptions(const std::string& function, const FunctionOptions* options) {
  const MatchSubstringOptions* o = dynamic_cast<const MatchSubstringOptions*>(options);
  if (!o || !o->PatternGiven) return Status::Make(StatusCode::Invalid, "function '" + function + "' needs the option pattern_hex=<the pattern's bytes in hex>");
  if (o->PatternBadHex) return Status::Make(StatusCode::Invalid, "function '" + function + "': pattern_hex is not a string of hex byte pairs");
  if (o->IgnoreCase)
    return Status::Make(StatusCode::NotImplemented, "function '" + function + "': ignore_case=true is not implemented (Arrow folds Unicode case; an ASCII-only fold would disagree with it)");
  if (o->Pattern.size() > (size_t)AH_STR_MAX_PATTERN)
    return Status::Make(StatusCode::NotImplemented, "function '" + function + "': a pattern of " + std::to_string(o->Pattern.size()) + " bytes (at most " +
                                                        std::to_string(AH_STR_MAX_PATTERN) + ")");
  return Status::OK();
}

void RegisterStringMatch(FunctionRegistry* reg) {
  struct F { const char* name; int fn; };
  for (F f : {F{"match_substring", kFnSubstring}, F{"starts_with", kFnStartsWith}, F{"ends_with", kFnEndsWith}, F{"find_substring", kFnFind},
              F{"match_like", kFnLike}, F{"binary_length", kFnBinaryLength}, F{"utf8_length", kFnUtf8Length}}) {
    auto fn = std::make_shared<ScalarFunction>(f.name, Arity{1, false});
    std::vector<Type> types = {Type::STRING, Type::LARGE_STRING};
    if (f.fn != kFnUtf8Length) { types.push_back(Type::BINARY); types.push_back(Type::LARGE_BINARY); }
    if (f.fn == kFnBinaryLength) types.push_back(Type::FIXED_SIZE_BINARY);
    for (Type t : types) {
      exec::ScalarKernel k;
      k.sig.in_types = {t};
      k.sig.out_is_first_input = false;
      const bool large = t == Type::LARGE_STRING || t == Type::LARGE_BINARY;
      k.sig.out_type = f.fn == kFnFind || f.fn == kFnBinaryLength || f.fn == kFnUtf8Length ? (large ? Type::INT64 : Type::INT32) : Type::BOOL;
      const F ff = f;
      k.exec_fn = [ff](KernelCtx* kc, const ExecSpan& b, ExecResult* o) { return ExecStringMatch(kc, b, o, ff.name, ff.fn); };
      fn->AddKernel(std::move(k));
    }
    fn->arrays_only = true;
    reg->AddFunction(fn, false);
  }
}

// ---- string transforms: ascii_upper / ascii_lower, utf8_slice_codeunits, binary_slice, the nine trims ------------------------------------
// No reference analogue (arrow-go has none of them): Arrow C++'s functions and semantics, DESIGN.md §3.18.  The result of every row is
// one contiguous sub-range of the row's bytes (the case mappings: the whole row through a byte map), so one pair of entry points
// serves all thirteen: ah_string_ranges (source starts, output offsets, the byte total — the call's one synchronisation), the
// allocation, ah_string_gather.  The output's validity is the input's (NullIntersection); a null row has length 0.
namespace {

enum TransformChars { kCharsNone, kCharsBytes, kCharsCodePoints, kCharsWhitespace };
enum TransformMap { kMapNone, kMapUpper, kMapLower };
struct TransformFn { const char* name; int op, sides, chars, map; bool strings; };   // strings: String / LargeString, else Binary / LargeBinary
const TransformFn kTransformFns[] = {
    {"ascii_upper", AH_STX_WHOLE, 0, kCharsNone, kMapUpper, true},
    {"ascii_lower", AH_STX_WHOLE, 0, kCharsNone, kMapLower, true},
    {"utf8_slice_codeunits", AH_STX_SLICE_CODEPOINTS, 0, kCharsNone, kMapNone, true},
    {"binary_slice", AH_STX_SLICE_BYTES, 0, kCharsNone, kMapNone, false},
    {"ascii_trim", AH_STX_TRIM_BYTES, AH_STX_LEFT | AH_STX_RIGHT, kCharsBytes, kMapNone, true},
    {"ascii_ltrim", AH_STX_TRIM_BYTES, AH_STX_LEFT, kCharsBytes, kMapNone, true},
    {"ascii_rtrim", AH_STX_TRIM_BYTES, AH_STX_RIGHT, kCharsBytes, kMapNone, true},
    {"ascii_trim_whitespace", AH_STX_TRIM_BYTES, AH_STX_LEFT | AH_STX_RIGHT, kCharsWhitespace, kMapNone, true},
    {"ascii_ltrim_whitespace", AH_STX_TRIM_BYTES, AH_STX_LEFT, kCharsWhitespace, kMapNone, true},
    {"ascii_rtrim_whitespace", AH_STX_TRIM_BYTES, AH_STX_RIGHT, kCharsWhitespace, kMapNone, true},
    {"utf8_trim", AH_STX_TRIM_CODEPOINTS, AH_STX_LEFT | AH_STX_RIGHT, kCharsCodePoints, kMapNone, true},
    {"utf8_ltrim", AH_STX_TRIM_CODEPOINTS, AH_STX_LEFT, kCharsCodePoints, kMapNone, true},
    {"utf8_rtrim", AH_STX_TRIM_CODEPOINTS, AH_STX_RIGHT, kCharsCodePoints, kMapNone, true},
};
const TransformFn* TransformByName(const std::string& name) {
  for (const TransformFn& f : kTransformFns)
    if (name == f.name) return &f;
  return nullptr;
}

// RFC 3629: no overlong forms, no surrogates, nothing above U+10FFFF
bool ValidUtf8(const std::string& s) {
  for (size_t i = 0; i < s.size();) {
    const unsigned char b = (unsigned char)s[i];
    const int len = b < 0x80 ? 1 : (b & 0xE0) == 0xC0 ? 2 : (b & 0xF0) == 0xE0 ? 3 : (b & 0xF8) == 0xF0 ? 4 : 0;
    if (!len || i + len > s.size()) return false;
    unsigned cp = len == 1 ? b : b & (0xFF >> (len + 1));
    for (int j = 1; j < len; j++) {
      const unsigned char c = (unsigned char)s[i + j];
      if ((c & 0xC0) != 0x80) return false;
      cp = (cp << 6) | (c & 0x3F);
    }
    static const unsigned least[5] = {0, 0, 0x80, 0x800, 0x10000};
    if (cp < least[len] || cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF)) return false;
    i += len;
  }
  return true;
}

Status ExecStringTransform(KernelCtx* k, const ExecSpan& b, ExecResult* out, const TransformFn& f) {
  Session* s = k->session;
  const FunctionOptions* given = static_cast<const FunctionOptions*>(k->state);
  AHC_RETURN_NOT_OK(ValidateStringTransformOptions(f.name, given));
  const ArraySpan& in = b.values[0].array;
  const int ow = out->type->bit_width / 8;
  const int64_t n = out->len;
  BufferPtr ob, db, sb;
  AHC_RETURN_NOT_OK(k->Allocate((n + 1) * ow, &ob));   // (zeroed: the lone closing offset of an empty chunk)
  out->buffers[1].WrapBuffer(ob);
  if (n == 0) {   // (a scalar argument never gets here: ScalarFunction::arrays_only)
    AHC_RETURN_NOT_OK(k->Allocate(0, &db));
    out->buffers[2].WrapBuffer(db);
    return Status::OK();
  }
  int64_t start = 0, stop = 0;
  int has_stop = 0;
  std::string chars;
  if (f.op == AH_STX_SLICE_BYTES || f.op == AH_STX_SLICE_CODEPOINTS) {
    const SliceOptions* o = static_cast<const SliceOptions*>(given);
    start = o->Start;
    stop = o->Stop;
    has_stop = o->StopGiven ? 1 : 0;
  } else if (f.chars == kCharsWhitespace) {
    chars = "\t\n\v\f\r ";
  } else if (f.chars != kCharsNone) {
    chars = static_cast<const TrimOptions*>(given)->Characters;
  }
  uint8_t map[256];
  for (int c = 0; c < 256; c++)
    map[c] = (uint8_t)(f.map == kMapUpper && c >= 'a' && c <= 'z' ? c - 32 : f.map == kMapLower && c >= 'A' && c <= 'Z' ? c + 32 : c);
  const ByteLayout l = LayoutOf(in);
  const ah_cmp_operand col{l.offset_width, l.byte_width, l.offsets, l.data, l.offset, 0};
  const uint8_t* valid = in.MayHaveNulls() ? in.buffers[0].buf : nullptr;
  AHC_RETURN_NOT_OK(k->Allocate(n * ow, &sb, /*zero_all=*/false));
  int64_t total = 0;
  AHC_RETURN_NOT_OK(s->FromStatus(ah_string_ranges(s->ctx(), f.op, start, stop, has_stop, f.sides, (const uint8_t*)chars.data(), (int64_t)chars.size(), &col, valid,
                                             in.offset, n, sb->dptr, ob->dptr, &total)));
  AHC_RETURN_NOT_OK(k->Allocate(total, &db, /*zero_all=*/false));
  out->buffers[2].WrapBuffer(db);
  if (total == 0) return Status::OK();
  return s->FromStatus(ah_string_gather(s->ctx(), &col, sb->dptr, ob->dptr, n, f.map == kMapNone ? nullptr : map, (uint8_t*)db->dptr));
}

}  // namespace

bool IsStringTransformFunction(const std::string& function) { return TransformByName(function) != nullptr; }

Status ValidateStringTransformOptions(const std::string& function, const FunctionOptions* options) {
  const TransformFn* f = TransformByName(function);
  if (!f) return Status::Make(StatusCode::KeyError, "function '" + function + "' not found");
  if (f->op == AH_STX_SLICE_BYTES || f->op == AH_STX_SLICE_CODEPOINTS) {
    const SliceOptions* o = dynamic_cast<const SliceOptions*>(options);
    if (o && !o->BadInteger.empty()) return Status::Make(StatusCode::Invalid, "function '" + function + "': " + o->BadInteger + " is not an int64");
    if (!o || !o->StartGiven) return Status::Make(StatusCode::Invalid, "function '" + function + "' needs the option start=<int64>");
    if (o->Step == 0) return Status::Make(StatusCode::Invalid, "function '" + function + "': slice step cannot be zero");
    if (o->Step != 1)
      return Status::Make(StatusCode::NotImplemented, "function '" + function + "': step=" + std::to_string(o->Step) + " is not implemented (the result must be one sub-range of the row: step=1)");
    return Status::OK();
  }
  if (f->chars == kCharsBytes || f->chars == kCharsCodePoints) {
    const TrimOptions* o = dynamic_cast<const TrimOptions*>(options);
    if (!o || !o->Given) return Status::Make(StatusCode::Invalid, "function '" + function + "' needs the option characters_hex=<the characters' bytes in hex>");
    if (o->BadHex) return Status::Make(StatusCode::Invalid, "function '" + function + "': characters_hex is not a string of hex byte pairs");
    if (o->Characters.size() > (size_t)AH_STX_MAX_CHARS)
      return Status::Make(StatusCode::NotImplemented, "function '" + function + "': characters of " + std::to_string(o->Characters.size()) + " bytes (at most " +
                                                          std::to_string(AH_STX_MAX_CHARS) + ")");
    if (f->chars == kCharsCodePoints && !ValidUtf8(o->Characters)) return Status::Make(StatusCode::Invalid, "function '" + function + "': the characters are not valid UTF-8");
  }
  return Status::OK();
}

void RegisterStringTransform(FunctionRegistry* reg) {
  for (const TransformFn& f : kTransformFns) {
    auto fn = std::make_shared<ScalarFunction>(f.name, Arity{1, false});
    const std::vector<Type> types = f.strings ? std::vector<Type>{Type::STRING, Type::LARGE_STRING} : std::vector<Type>{Type::BINARY, Type::LARGE_BINARY};
    for (Type t : types) {
      exec::ScalarKernel k;
      k.sig.in_types = {t};   // (the output type is the input's: out_is_first_input)
      k.mem_alloc = exec::MemAlloc::MemNoPrealloc;
      const TransformFn* ff = &f;
      k.exec_fn = [ff](KernelCtx* kc, const ExecSpan& b, ExecResult* o) { return ExecStringTransform(kc, b, o, *ff); };
      fn->AddKernel(std::move(k));
    }
    fn->arrays_only = true;
    reg->AddFunction(fn, false);
  }
}

}  // namespace compute
}  // namespace arrowhip
