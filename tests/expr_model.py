"""An independent model of eval_expression: a parser for its prefix text and an evaluator over numpy arrays.

TEST INFRASTRUCTURE.  It calls neither libarrowhip nor liboracle: numpy for the element-wise IEEE and wrapping operations, Python
integers wherever a result must be decided exactly (the checked ops).  tests/test_expr_model_host.py holds it against the CPU oracle
op by op; tests/test_expressions_ranges.py holds both routes of eval_expression (one JIT-compiled kernel, one kernel per call) against
it.

    evaluate(text, columns, literals) -> (values, validity, status)

columns   one (values, valid) per `$i`: values a 1-D numpy array (dtype bool for a Boolean column), valid a bool array or None (no nulls)
literals  one (dtype, value) per `#k`; value None is a null literal (its payload is 0, as the library's null scalar has it)
values    the result payload of EVERY slot, null slots included; dtype bool for a Boolean result
validity  bool array
status    "ok" or "overflow" (then `values` is what the last call node would have written, and says nothing about the routes)

The rules (header of ah_expr.hip, ah_elementwise.h; the reference's kernels behind them):
  validity            AND of the operands' validity; a null literal makes every slot null
  unchecked int ops   wrap in the type's width, computed in every slot; abs_unchecked(min) = min; negate_unchecked wraps, unsigned too
  add / subtract      NotNull ops: a null slot holds 0 and reports nothing.  A valid slot reports by the reference's carry test
                      (base_arithmetic.go:249-278), which is one-sided: add reports iff the exact sum is ABOVE the type's maximum,
                      subtract iff the exact difference is BELOW its minimum (for unsigned types those are the only ways out of
                      range; for signed ones min + (−1) and max − (−1) wrap silently).  Decided here on exact Python integers.
  multiply            every slot, null payloads included: reports iff the exact product is outside the type; such a slot holds 0
  float ops           one IEEE operation in the operand's own dtype, no contraction; checked == unchecked
  sign                sign(±0) = +0, sign(NaN) = NaN; an integer's sign keeps the integer's type
  comparisons         IEEE: NaN compares false, != true
  boolean ops         plain bit-wise ops on the data bits of every slot (non-Kleene)
  promotion           operands of different types go to commonNumeric (compute/utils.go:178-240) with astype
"""
import numpy as np

ARITH = {"add": ("add", True), "add_unchecked": ("add", False), "subtract": ("sub", True), "sub": ("sub", True),
         "subtract_unchecked": ("sub", False), "sub_unchecked": ("sub", False), "multiply": ("mul", True), "multiply_unchecked": ("mul", False)}
UNARY = ("negate_unchecked", "abs_unchecked", "sign")
COMPARE = ("equal", "not_equal", "greater", "greater_equal", "less", "less_equal")
BOOLEAN = ("and", "or", "xor", "and_not")

BOOL = np.dtype(bool)


# ---- the text ------------------------------------------------------------------------------------------
def parse(text):
    """call := name '(' arg {',' arg} ')' ; arg := call | '$'N | '#'N   →   ("col", N) | ("lit", N) | ("call", name, [args])"""
    pos = 0

    def ws():
        nonlocal pos
        while pos < len(text) and text[pos] == " ":
            pos += 1

    def node():
        nonlocal pos
        ws()
        if pos < len(text) and text[pos] in "$#":
            kind = "col" if text[pos] == "$" else "lit"
            end = pos + 1
            while end < len(text) and text[end].isdigit():
                end += 1
            if end == pos + 1:
                raise ValueError(f"expected an index at {pos} of {text!r}")
            out = (kind, int(text[pos + 1:end]))
            pos = end
            return out
        end = pos
        while end < len(text) and (text[end].islower() or text[end].isdigit() or text[end] == "_"):
            end += 1
        name = text[pos:end]
        pos = end
        ws()
        if not name or pos >= len(text) or text[pos] != "(":
            raise ValueError(f"expected name( at {pos} of {text!r}")
        pos += 1
        args = []
        while True:
            args.append(node())
            ws()
            if pos < len(text) and text[pos] == ",":
                pos += 1
            elif pos < len(text) and text[pos] == ")":
                pos += 1
                return ("call", name, args)
            else:
                raise ValueError(f"expected , or ) at {pos} of {text!r}")

    tree = node()
    ws()
    if pos != len(text):
        raise ValueError(f"trailing text at {pos} of {text!r}")
    return tree


# ---- types ---------------------------------------------------------------------------------------------
def common_numeric(a, b):
    """commonNumeric of two numeric dtypes"""
    a, b = np.dtype(a), np.dtype(b)
    for f in (np.float64, np.float32):
        if a == f or b == f:
            return np.dtype(f)
    signed = max([d.itemsize * 8 for d in (a, b) if d.kind == "i"], default=0)
    unsigned = max([d.itemsize * 8 for d in (a, b) if d.kind == "u"], default=0)
    if signed == 0:
        return np.dtype(f"u{unsigned // 8}")
    if signed <= unsigned:   # the next power of two above the unsigned width, at most 64
        signed = min(unsigned * 2, 64)
    return np.dtype(f"i{signed // 8}")


def value_preserving(frm, to):
    """the casts that cannot lose a value: the only ones a column takes inside the fused kernel"""
    frm, to = np.dtype(frm), np.dtype(to)
    if frm == to:
        return True
    fb, tb = frm.itemsize * 8, to.itemsize * 8
    if frm.kind in "iu" and to.kind in "iu":
        return tb >= fb if frm.kind == to.kind else (frm.kind == "u" and tb > fb)
    if frm.kind in "iu":
        return fb <= 32 if to == np.float64 else fb <= 16
    return frm == np.float32 and to == np.float64


def limits(dt):
    info = np.iinfo(dt)
    return int(info.min), int(info.max)


def _exact(a):
    """the values as Python integers (an object array: its arithmetic is exact)"""
    return a.astype(object)


def _wrapped(exact, dt):
    """exact Python integers → the type's two's-complement value of the same low bits"""
    u = np.dtype(f"u{dt.itemsize}")
    mask = (1 << (dt.itemsize * 8)) - 1
    return np.array([int(x) & mask for x in exact], dtype=u).view(dt) if len(exact) else np.zeros(0, dt)


def boundary(dtype):
    """the values the tests plant: a type's {min, min+1, −1, 0, 1, max−1, max} (−1 is max for an unsigned type); for floats NaN,
    ±inf, ±0, the largest finite values, the smallest normal and denormals, and a few ordinary numbers"""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        fi = np.finfo(dt)
        return np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, fi.max, -fi.max, fi.tiny, -fi.tiny, fi.smallest_subnormal, -fi.smallest_subnormal,
                         fi.tiny / 4, 1.0, -1.0, 0.5, 3.0], dtype=dt)
    info = np.iinfo(dt)
    minus_one = info.max if dt.kind == "u" else -1
    return np.array([info.min, info.min + 1, minus_one, 0, 1, info.max - 1, info.max], dtype=dt)


# ---- evaluation ----------------------------------------------------------------------------------------
class _Eval:
    def __init__(self, columns, literals, n):
        self.columns, self.literals, self.n = columns, literals, n
        self.status = "ok"

    def promote(self, a, b):
        """both operands in the common type; a is (values, valid, is_literal)"""
        (av, ak, al), (bv, bk, bl) = a, b
        if av.dtype == bv.dtype:
            return av, ak, bv, bk
        if av.dtype == BOOL or bv.dtype == BOOL:
            raise TypeError("no common type of a Boolean and a number")
        common = common_numeric(av.dtype, bv.dtype)
        out = []
        for v, is_lit in ((av, al), (bv, bl)):
            if v.dtype != common:
                with np.errstate(all="ignore"):
                    c = v.astype(common)
                if is_lit:   # a scalar is safe-cast once, on the host: it must survive the trip
                    if len(v) and not (c[0] == v[0] and c.astype(v.dtype)[0] == v[0]):
                        raise ValueError(f"literal {v[0]!r} does not fit {common}")
                elif not value_preserving(v.dtype, common):
                    raise TypeError(f"a column cast {v.dtype} → {common} can fail: such a tree is not fused")
                v = c
            out.append(v)
        return out[0], ak, out[1], bk

    def arith(self, base, checked, a, ak, b, bk):
        dt = a.dtype
        ok = ak & bk
        if dt.kind == "f":
            with np.errstate(all="ignore"):
                return (a + b if base == "add" else a - b if base == "sub" else a * b), ok
        u = np.dtype(f"u{dt.itemsize}")
        if not checked:
            ua, ub = a.view(u), b.view(u)
            return (ua + ub if base == "add" else ua - ub if base == "sub" else ua * ub).view(dt), ok
        lo, hi = limits(dt)
        ea, eb = _exact(a), _exact(b)
        exact = ea + eb if base == "add" else ea - eb if base == "sub" else ea * eb
        if base == "mul":     # every slot
            over = np.array([x < lo or x > hi for x in exact], dtype=bool)
            if over.any():
                self.status = "overflow"
            return np.where(over, np.zeros(1, dt), _wrapped(exact, dt)), ok
        over = np.array([(x > hi) if base == "add" else (x < lo) for x in exact], dtype=bool)
        if (over & ok).any():  # a null slot reports nothing …
            self.status = "overflow"
        return np.where(ok, _wrapped(exact, dt), np.zeros(1, dt)), ok   # … and holds 0

    def unary(self, name, a):
        dt = a.dtype
        if dt.kind == "f":
            if name == "negate_unchecked":
                return -a
            if name == "abs_unchecked":
                return np.abs(a)
            one = np.ones(1, dt)
            return np.where(np.isnan(a), a, np.where(a == 0, np.zeros(1, dt), np.where(np.signbit(a), -one, one)))
        u = np.dtype(f"u{dt.itemsize}")
        ua = a.view(u)
        neg = (~ua + np.ones(1, u)).view(dt)   # two's complement: wraps, unsigned included
        if name == "negate_unchecked":
            return neg
        if name == "abs_unchecked":
            return a.copy() if dt.kind == "u" else np.where(a < 0, neg, a)
        if dt.kind == "u":
            return (a > 0).astype(dt)
        return (a > 0).astype(dt) - (a < 0).astype(dt)

    def run(self, t):
        """→ (values, valid, is_literal)"""
        n = self.n
        if t[0] == "col":
            v, k = self.columns[t[1]]
            v = np.asarray(v)
            return v, (np.ones(n, bool) if k is None else np.asarray(k, bool)), False
        if t[0] == "lit":
            dt, val = self.literals[t[1]]
            dt = np.dtype(dt)
            return np.full(n, 0 if val is None else val, dtype=dt), np.full(n, val is not None), True
        _, name, args = t
        if name in ARITH or name in COMPARE:
            a, ak, b, bk = self.promote(self.run(args[0]), self.run(args[1]))
            if a.dtype == BOOL:
                raise TypeError(f"{name} needs numeric operands")
            if name in ARITH:
                v, k = self.arith(*ARITH[name], a, ak, b, bk)
                return v, k, False
            with np.errstate(all="ignore"):
                v = {"equal": a == b, "not_equal": a != b, "greater": a > b, "greater_equal": a >= b, "less": a < b, "less_equal": a <= b}[name]
            return v, ak & bk, False
        if name in UNARY:
            a, ak, _ = self.run(args[0])
            if a.dtype == BOOL:
                raise TypeError(f"{name} needs a numeric operand")
            return self.unary(name, a), ak, False
        if name in BOOLEAN or name == "invert":
            ops = [self.run(x) for x in args]
            if any(o[0].dtype != BOOL for o in ops):
                raise TypeError(f"{name} needs Boolean operands")
            if name == "invert":
                return ~ops[0][0], ops[0][1], False
            (a, ak, _), (b, bk, _) = ops
            return {"and": a & b, "or": a | b, "xor": a ^ b, "and_not": a & ~b}[name], ak & bk, False
        raise KeyError(f"function {name!r} is not one the fused kernel covers")


def evaluate(text, columns, literals=()):
    if not columns:
        raise ValueError("the model needs at least one column")
    n = len(columns[0][0])
    ev = _Eval(list(columns), list(literals), n)
    values, valid, _ = ev.run(parse(text))
    return np.ascontiguousarray(values), valid, ev.status
