"""Derives ctypes bindings from a C header of ours (include/speechless_hip.h, include/speechless_host.h), so that an entry
point, a struct or a constant is declared in the header and nowhere else.  The headers are regular: `#define NAME <integer>`,
`typedef enum`, `typedef struct` and prototypes over a handful of types.  The mapping is by C type alone (`_ctype`); whatever
does not fit raises CDeclError with the declaration's text -- a guessed argtype would hand a kernel a truncated pointer."""
import ctypes
import re
from ctypes import POINTER, c_char_p, c_void_p
from pathlib import Path
from typing import NamedTuple

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
           "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}
INCLUDE_DIR = Path(__file__).resolve().parent.parent / "include"
# a non-const pointer to one of these is a host out-parameter (`int* segs`, `int64_t* n_trie_nodes`); any other scalar pointer
# is an address the library only forwards to kernels or reads as an array: c_void_p
OUT_SCALARS = ("int", "int64_t")

_DECL = re.compile(r"(const\s+)?(\w+)\s*((?:\*\s*(?:const\b\s*)?)*)(\w*)$")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(\w+)(\S*)[ \t]+(\S.*?)[ \t]*$", re.M)
_TYPEDEF = re.compile(r"\btypedef\s+(enum|struct)\b\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;")
_FUNCTION = re.compile(r"(?<![^;{}\s])([\w \t*]+?[ \t*])(\w+)\s*\(([^(){};]*)\)\s*;")
# what may remain of a header: its include guard, #include lines, the __cplusplus guards and extern "C" { }.  Not #if / #else:
# a declaration under a condition has no one signature
_FRAME = re.compile(r'^[ \t]*(#[ \t]*((ifndef|ifdef|endif|include)\b.*|define[ \t]+\w+[ \t]*)|extern\s+"C"\s*\{[ \t]*|\}[ \t]*)$',
                    re.M)


class CDeclError(ValueError):
    pass


class Header(NamedTuple):
    functions: dict  # name -> (restype, [argtypes])
    structs: dict    # typedef name -> ordered _fields_
    constants: dict  # name -> int: `#define NAME <integer>` and enumerators
    leftover: str    # the text no rule consumed


def _int(text):
    try:
        return int(text, 0)
    except ValueError:
        return None


def _ctype(decl, classes):
    """(ctypes type, declared name) of one parameter, field or return type; None is `void`."""
    m = _DECL.match(decl.strip())
    if not m:
        raise CDeclError("cannot parse `{}`".format(decl.strip()))
    const, base, stars, name = m.group(1), m.group(2), m.group(3).count("*"), m.group(4)
    if base not in SCALARS and base not in classes and base not in ("void", "char"):
        raise CDeclError("unknown type `{}` in `{}`".format(base, decl.strip()))
    if stars == 0:
        if base == "char":
            raise CDeclError("char by value in `{}`".format(decl.strip()))
        return (None if base == "void" else SCALARS.get(base) or classes[base]), name
    if stars > 1:
        return POINTER(c_void_p), name
    if base in classes:
        return POINTER(classes[base]), name
    if base == "char":
        return c_char_p, name
    if not const and base in OUT_SCALARS:
        return POINTER(SCALARS[base]), name  # a host out-parameter: passed with ctypes.byref
    return c_void_p, name  # device addresses, streams, opaque handles


def _fields(body, classes):
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = (d.strip() for d in decl.split(","))
        if any(not re.fullmatch(r"[A-Za-z_]\w*", n) for n in more):  # `int a[4], *b, c : 3`
            raise CDeclError("cannot parse struct field `{}`".format(decl))
        ctype, name = _ctype(first, classes)
        if ctype is None or not name:
            raise CDeclError("cannot parse struct field `{}`".format(decl))
        fields += [(n, ctype) for n in [name] + more]
    return fields


def parse(text, classes=None):
    """Header of C header `text`.  classes: typedef name -> the ctypes.Structure subclass that receives the struct's _fields_
    (any other struct of the header gets a class of the typedef's name)."""
    given = dict(classes or {})
    classes, structs, constants, functions = {}, {}, {}, {}
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)

    def define(m):
        value = _int(m.group(3))
        if m.group(2) or value is None:
            raise CDeclError("#define is not an integer constant: `{}`".format(m.group(0).strip()))
        constants[m.group(1)] = value
        return ""

    def typedef(m):
        kind, body, name = m.groups()
        if kind == "enum":
            for item in filter(None, (i.strip() for i in body.split(","))):
                key, _, value = (s.strip() for s in item.partition("="))
                if not re.fullmatch(r"[A-Za-z_]\w*", key) or _int(value) is None:
                    raise CDeclError("enumerator without an integer value: `{}` in enum {}".format(item, name))
                constants[key] = _int(value)
        else:
            cls = given.pop(name, None) or type(name, (ctypes.Structure,), {})
            structs[name] = _fields(body, classes)
            cls._fields_ = structs[name]
            classes[name] = cls
        return ""

    def function(m):
        params = [p.strip() for p in m.group(3).split(",")]
        if "..." in params:
            raise CDeclError("variadic function: `{}`".format(m.group(0).strip()))
        restype, _ = _ctype(m.group(1), classes)
        argtypes = [] if params in ([""], ["void"]) else [_ctype(p, classes)[0] for p in params]
        if None in argtypes:
            raise CDeclError("void parameter: `{}`".format(m.group(0).strip()))
        functions[m.group(2)] = (restype, argtypes)
        return ""

    for pattern, consume in ((_DEFINE, define), (_TYPEDEF, typedef), (_FUNCTION, function)):
        text = pattern.sub(consume, text)
    if given:
        raise CDeclError("the header has no struct {}".format(sorted(given)))
    rest = _FRAME.sub("", text).strip()
    if rest:  # e.g. a function-pointer parameter, or an sl_...( declaration no pattern matched: it would stay unbound
        raise CDeclError("cannot parse `{}`".format(" ".join(rest.split())))
    return Header(functions, structs, constants, text)


def load(name, classes=None):
    """parse() of include/<name>."""
    return parse((INCLUDE_DIR / name).read_text(), classes)
