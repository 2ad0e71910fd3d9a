"""CPU tests of speechless_amd/_cdecl.py, which derives the ctypes tables of _lib.py and _host_lib.py from the two headers:
every mapping rule on literal snippets, every refusal with the offending text, and the two real headers consumed whole."""
import ctypes
import re
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint64, c_void_p
from pathlib import Path

import pytest

from speechless_amd import _cdecl
from speechless_amd._cdecl import CDeclError, parse

ROOT = Path(__file__).resolve().parent.parent

SNIPPET = """
#ifndef SNIPPET_H
#define SNIPPET_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define SL_LIMIT 16   /* a comment with sl_hidden( in it */
#define SL_MASK 0x1f
typedef enum sl_kind { SL_A = 0, SL_B = 1,
                       SL_NEG = -3 } sl_kind;
typedef struct sl_inner {
    int32_t a, b;      /* a comma list */
    int64_t stride;
    const float* data; // a device address
    float scale;
} sl_inner;
typedef struct {
    void* x;
    sl_inner inner;    /* embedded by value */
    int n;
} sl_outer;
int sl_scalars(int a, int32_t b, int64_t c, uint64_t d, size_t e, float f, double g);
size_t sl_structs(const sl_inner* one, sl_outer* many, int n);
int sl_tables(void* const* ys, const void* const* ws, const float* const* biases);
const char* sl_text(const char* path, char* err, int err_len);
int sl_out_params(int* segs, int64_t* nodes, const int* lengths, const int64_t* offsets);
void* sl_addresses(const void* x, float* y, int32_t* labels, const uint32_t* alphabet, double* sum, void* stream);
double sl_score(void* handle);
void sl_free(void* handle);
int sl_nothing(void);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_every_mapping_rule():
    h = parse(SNIPPET)
    f = h.functions
    assert list(f) == ["sl_scalars", "sl_structs", "sl_tables", "sl_text", "sl_out_params", "sl_addresses", "sl_score", "sl_free",
                       "sl_nothing"]
    assert f["sl_scalars"] == (c_int, [c_int, c_int32, c_int64, c_uint64, c_size_t, c_float, c_double])
    assert f["sl_tables"] == (c_int, [POINTER(c_void_p)] * 3)
    assert f["sl_text"] == (c_char_p, [c_char_p, c_char_p, c_int])
    # a non-const pointer to int / int64_t is a host out-parameter; const ones and every other scalar pointer are addresses
    assert f["sl_out_params"] == (c_int, [POINTER(c_int), POINTER(c_int64), c_void_p, c_void_p])
    assert f["sl_addresses"] == (c_void_p, [c_void_p] * 6)
    assert f["sl_score"] == (c_double, [c_void_p])
    assert f["sl_free"] == (None, [c_void_p])
    assert f["sl_nothing"] == (c_int, [])
    restype, (one, many, n) = f["sl_structs"]
    assert (restype, n) == (c_size_t, c_int)
    inner, outer = one._type_, many._type_
    assert (inner.__name__, outer.__name__) == ("sl_inner", "sl_outer")
    assert h.structs == {
        "sl_inner": [("a", c_int32), ("b", c_int32), ("stride", c_int64), ("data", c_void_p), ("scale", c_float)],
        "sl_outer": [("x", c_void_p), ("inner", inner), ("n", c_int)]}
    assert inner._fields_ == h.structs["sl_inner"] and outer._fields_ == h.structs["sl_outer"]
    assert (ctypes.sizeof(inner), ctypes.sizeof(outer), outer.inner.offset) == (32, 48, 8)
    assert h.constants == {"SL_LIMIT": 16, "SL_MASK": 31, "SL_A": 0, "SL_B": 1, "SL_NEG": -3}
    assert not re.sub(r'(?m)^\s*#.*$|extern\s+"C"\s*\{|\}', "", h.leftover).strip()


def test_named_classes_receive_the_fields():
    class Inner(ctypes.Structure):
        """keeps its name, docstring and methods"""

        def total(self):
            return self.a + self.b

    h = parse(SNIPPET, {"sl_inner": Inner})
    assert Inner._fields_ == h.structs["sl_inner"] and Inner(a=2, b=3).total() == 5
    assert h.functions["sl_structs"][1][0] is POINTER(Inner)
    assert dict(h.structs["sl_outer"])["inner"] is Inner  # the embedded struct is the named class, not a twin
    with pytest.raises(CDeclError, match="sl_missing"):
        parse(SNIPPET, {"sl_missing": type("Missing", (ctypes.Structure,), {})})


@pytest.mark.parametrize("text, offending", [
    ("int sl_f(unsigned x);", "unsigned x"),                                  # an unknown type name
    ("int sl_f(const sl_later* p);", "sl_later"),                             # a struct this header does not typedef
    ("sl_handle sl_f(void);", "sl_handle"),                                   # an unknown return type
    ("int sl_f(void (*done)(int), void* stream);", "int sl_f(void (*done)(int), void* stream);"),  # a function pointer
    ("typedef struct { float taps[4]; } sl_s;", "float taps[4]"),             # an array in a struct
    ("typedef struct { int a, b[2]; } sl_s;", "int a, b[2]"),
    ("typedef struct { int flag : 1; } sl_s;", "int flag : 1"),               # a bit field
    ("typedef struct { int a; struct { int b; } in; } sl_s;", "struct { int b; } in;"),  # a nested definition
    ("int sl_f(const char* fmt, ...);", "int sl_f(const char* fmt, ...);"),   # a variadic function
    ("#define SL_RATE 0.5f", "#define SL_RATE 0.5f"),                         # a non-integer #define
    ("#define SL_TWICE(x) 2 * (x)", "#define SL_TWICE(x) 2 * (x)"),
    ("typedef enum { SL_A, SL_B } sl_e;", "SL_A"),                            # an enumerator without its value
    ("int sl_f(int a) __attribute__((cold));", "int sl_f(int a) __attribute__((cold));"),  # an sl_...( no pattern consumed
    ("static inline int sl_f(int a) { return a; }", "sl_f(int a)"),
    ("struct sl_s;\nint sl_f(int a);", "struct sl_s;"),                       # anything else that is left over
    ("#if SL_WIDE\nint sl_f(int64_t a);\n#else\nint sl_f(int a);\n#endif", "#if SL_WIDE #else"),  # declarations under a condition
])
def test_refusals_name_the_offending_text(text, offending):
    with pytest.raises(CDeclError, match=re.escape(offending)):
        parse(text)


@pytest.mark.parametrize("header, pattern, not_functions", [
    # the name patterns of tests/test_codec_and_host.py's two header tests
    ("speechless_hip.h", r"\b(sl_[a-z0-9_]+)\s*\(", {"sl_status", "sl_dtype", "sl_epilogue", "sl_conv_geom"}),
    ("speechless_host.h", r"\b(sl_host_[a-z0-9_]+)\s*\(", set()),
])
def test_real_headers_are_consumed_whole(header, pattern, not_functions):
    text = (ROOT / "include" / header).read_text()
    h = _cdecl.load(header)
    declared = set(re.findall(pattern, re.sub(r"/\*.*?\*/", "", text, flags=re.S))) - not_functions
    assert declared == set(h.functions), declared ^ set(h.functions)
    assert set(re.findall(pattern, text)) - not_functions == declared  # the hip test reads the comments too
    rest = re.sub(r'(?m)^[ \t]*#[ \t]*(ifndef|ifdef|define|include|endif)\b.*$|extern\s+"C"\s*\{|\}', "", h.leftover)
    assert not rest.strip(), rest.strip()
    assert all(isinstance(v, int) for v in h.constants.values())
