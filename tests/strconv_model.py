"""Go's strconv.ParseInt / ParseUint (base 0), ParseBool and Quote restated in Python, step by step as strconv/atoi.go and atob.go
do them — the expected values of tests/test_strconv_host.py and tests/test_cast_string.py.  Python's int(s, 0) is not this: it
refuses "012", skips white space and treats underscores differently.  Strings are `bytes`."""

SYNTAX, RANGE = "invalid syntax", "value out of range"
INT_BITS = {"int8": 8, "int16": 16, "int32": 32, "int64": 64, "uint8": 8, "uint16": 16, "uint32": 32, "uint64": 64}


def _lower(c):
    return c | 0x20


def underscore_ok(s):
    """atoi.go underscoreOK: underscores only between digits or directly after the base prefix"""
    saw = "^"
    i = 0
    if len(s) >= 1 and s[0] in b"+-":
        s = s[1:]
    hexa = False
    if len(s) >= 2 and s[0] == ord("0") and _lower(s[1]) in b"box":
        i = 2
        saw = "0"
        hexa = _lower(s[1]) == ord("x")
    while i < len(s):
        c = s[i]
        i += 1
        if ord("0") <= c <= ord("9") or (hexa and ord("a") <= _lower(c) <= ord("f")):
            saw = "0"
            continue
        if c == ord("_"):
            if saw != "0":
                return False
            saw = "_"
            continue
        if saw == "_":
            return False
        saw = "!"
    return saw != "_"


def go_parse_uint(s, bits):
    """(value, None) or (None, SYNTAX | RANGE): strconv.ParseUint(s, 0, bits)"""
    if len(s) == 0:
        return None, SYNTAX
    s0 = s
    base = 10
    if s[0] == ord("0"):
        if len(s) >= 3 and _lower(s[1]) == ord("b"):
            base, s = 2, s[2:]
        elif len(s) >= 3 and _lower(s[1]) == ord("o"):
            base, s = 8, s[2:]
        elif len(s) >= 3 and _lower(s[1]) == ord("x"):
            base, s = 16, s[2:]
        else:
            base, s = 8, s[1:]
    max64 = (1 << 64) - 1
    cutoff = max64 // base + 1
    max_val = (1 << bits) - 1
    underscores = False
    n = 0
    for c in s:
        if c == ord("_"):
            underscores = True
            continue
        if ord("0") <= c <= ord("9"):
            d = c - ord("0")
        elif ord("a") <= _lower(c) <= ord("z"):
            d = _lower(c) - ord("a") + 10
        else:
            return None, SYNTAX
        if d >= base:
            return None, SYNTAX
        if n >= cutoff:
            return None, RANGE
        n *= base
        n1 = n + d
        if n1 > max64 or n1 > max_val:
            return None, RANGE
        n = n1
    if underscores and not underscore_ok(s0):
        return None, SYNTAX
    return n, None


def go_parse_int(s, bits):
    """strconv.ParseInt(s, 0, bits)"""
    if len(s) == 0:
        return None, SYNTAX
    neg = False
    if s[0] == ord("+"):
        s = s[1:]
    elif s[0] == ord("-"):
        neg = True
        s = s[1:]
    un, err = go_parse_uint(s, bits)
    if err == SYNTAX:
        return None, SYNTAX
    cutoff = 1 << (bits - 1)
    if err == RANGE:
        un = (1 << bits) - 1
    if not neg and un >= cutoff:
        return None, RANGE
    if neg and un > cutoff:
        return None, RANGE
    return (-un if neg else un), None


def go_parse(type_name, s):
    bits = INT_BITS[type_name]
    return go_parse_uint(s, bits) if type_name.startswith("u") else go_parse_int(s, bits)


TRUE_SPELLINGS = [b"1", b"t", b"T", b"TRUE", b"true", b"True"]
FALSE_SPELLINGS = [b"0", b"f", b"F", b"FALSE", b"false", b"False"]


def go_parse_bool(s):
    if s in TRUE_SPELLINGS:
        return True, None
    if s in FALSE_SPELLINGS:
        return False, None
    return None, SYNTAX


def go_quote_ascii(s):
    """strconv.Quote of a byte string without bytes ≥ 0x80 (those depend on UTF-8 decoding; the tests pin printable ASCII)"""
    out = '"'
    for c in s:
        ch = chr(c)
        if ch in '"\\':
            out += "\\" + ch
        elif ch == "\n":
            out += "\\n"
        elif ch == "\t":
            out += "\\t"
        elif ch == "\r":
            out += "\\r"
        elif 0x20 <= c < 0x7F:
            out += ch
        else:
            out += "\\x%02x" % c
    return out + '"'


def parse_error_text(type_name, s, kind):
    """the NumError of the reference's cast: strconv.ParseInt: parsing "12 z": invalid syntax"""
    fn = "ParseBool" if type_name == "bool" else "ParseUint" if type_name.startswith("u") else "ParseInt"
    return "strconv.%s: parsing %s: %s" % (fn, go_quote_ascii(s), kind)


# TestStringToInt (arrow/compute/cast_test.go:2542-2579)
GOLDEN_ACCEPTED = (
    [(t, s, v) for t in ("int8", "int16", "int32", "int64")
     for s, v in zip([b"0", b"127", b"-1", b"0", b"0x0", b"0x7F"], [0, 127, -1, 0, 0, 127])]
    + [("int32", s, v) for s, v in zip([b"2147483647", b"-2147483648", b"0", b"0X0", b"0x7FFFFFFF", b"-0X1", b"-0x10000000"],
                                       [2147483647, -2147483648, 0, 0, 2147483647, -1, -268435456])]
    + [("int64", s, v) for s, v in zip([b"9223372036854775807", b"-9223372036854775808", b"0", b"0x0", b"0x7FFFFFFFFFFFFFFf", b"-0x0FFFFFFFFFFFFFFF"],
                                       [9223372036854775807, -9223372036854775808, 0, 0, 9223372036854775807, -1152921504606846975])]
    + [(t, s, v) for t in ("uint8", "uint16", "uint32", "uint64")
       for s, v in zip([b"0", b"127", b"255", b"0", b"0x0", b"0xff", b"0X7f"], [0, 127, 255, 0, 0, 255, 127])]
    + [("uint32", s, v) for s, v in zip([b"2147483647", b"4294967295", b"0", b"0x0", b"0x7FFFFFFf", b"0xFFFFFFFF"],
                                        [2147483647, 4294967295, 0, 0, 2147483647, 4294967295])]
    + [("uint64", s, v) for s, v in zip([b"9223372036854775807", b"18446744073709551615", b"0", b"0x0", b"0x7FFFFFFFFFFFFFFf", b"0xfFFFFFFFFFFFFFFf"],
                                        [9223372036854775807, 18446744073709551615, 0, 0, 9223372036854775807, 18446744073709551615])]
)
GOLDEN_NOT_INT8 = [b"z", b"12 z", b"128", b"-129", b"0.5", b"0x", b"0xfff", b"-0xf0"]
GOLDEN_NOT_UINT8 = [b"256", b"-1", b"0.5", b"0x", b"0x3wa", b"0x123"]
