"""The C ABI as include/*.h declares it: ctypes signatures, descriptor layouts and integer constants, read from the header text.

The headers are the one place where an entry point's argument list, a descriptor's fields and a literal `#define` are written;
dspnet_amd/_lib.py binds what parse() finds.  The vocabulary is closed: a declaration this module does not understand raises,
naming the header and the declaration (no torch import, no guess, no skip)."""
import ctypes
import glob
import os
import re

import numpy as np

INCLUDE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")

_SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong, "float": ctypes.c_float,
            "double": ctypes.c_double, "size_t": ctypes.c_size_t, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint,
            "unsigned char": ctypes.c_ubyte, "short": ctypes.c_short, "unsigned short": ctypes.c_ushort}
_RETURNS = ("int", "long long", "size_t", "const char *")
_PARAMS = ("int", "long long", "float", "double", "size_t", "unsigned", "unsigned int")
_FIELDS = ("int", "long long", "unsigned long long", "float", "double", "unsigned char", "short", "unsigned short", "unsigned")

_PROTOTYPE = re.compile(r"([\w\s\*]+?)\b(dspn_\w+)\s*\(([^()]*)\)\s*;")
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(0[xX][0-9a-fA-F]+|\d+)[ \t]*$", re.M)


def _strip_comments(text):
    """a comment becomes a space, so it cannot glue two tokens"""
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def _strip_preprocessor(text):
    return re.sub(r"^[ \t]*#(?:\\\n|[^\n])*", "", text, flags=re.M)        # a line ending in a backslash goes on


def _words(decl):
    """'const  float *x' -> 'const float * x': one space between tokens, `*` a token of its own"""
    return " ".join(decl.replace("*", " * ").split())


def _param(decl, where):
    """one parameter declaration -> its ctypes class; pointers and arrays are c_void_p"""
    decl = _words(decl)
    if "*" in decl or decl.endswith("]"):
        return ctypes.c_void_p
    for ctype in sorted(_PARAMS, key=len, reverse=True):        # `unsigned int n` before `unsigned n`
        if re.fullmatch(r"(const )?%s( \w+)?" % ctype, decl):
            return _SCALARS[ctype]
    raise ValueError(f"{where}: parameter type of `{decl}` is not in the C ABI's vocabulary")


def _struct(tag, body, where):
    """the body of `typedef struct tag { ... } tag;` -> a ctypes.Structure subclass (the platform lays it out)"""
    fields = []
    for decl in filter(None, (_words(re.sub(r"\bconst\b", "", d)) for d in body.split(";"))):
        # <type> <declarator>, <declarator> ...; a declarator is `name`, `*name`, `name[3]` or `name[3][64]`
        m = re.fullmatch(r"([\w ]+?) ((?:\* ?)*\w+(?: ?\[\d+\])*(?: ?, ?(?:\* ?)*\w+(?: ?\[\d+\])*)*)", decl)
        for declarator in m.group(2).split(",") if m else [None]:
            if not m or ("*" not in declarator and m.group(1) not in _FIELDS):
                raise ValueError(f"{where}: field type of `{decl}` in struct {tag} is not in the C ABI's vocabulary")
            name, *dims = re.findall(r"\w+", declarator)
            ctype = ctypes.c_void_p if "*" in declarator else _SCALARS[m.group(1)]
            for n in reversed(dims):                            # quant[3][64] is three arrays of 64
                ctype = ctype * int(n)
            fields.append((name, ctype))
    return type(tag, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"{where} {tag}"})


def parse_text(text, where="<header>"):
    """-> (signatures {name: (restype, [argtypes])}, structs {name: ctypes.Structure subclass}, defines {name: int})"""
    text = _strip_comments(text)
    defines = {name: int(value, 0) for name, value in _DEFINE.findall(text)}
    text = _strip_preprocessor(text)
    structs = {}
    for tag, body, name in _STRUCT.findall(text):
        if tag != name:
            raise ValueError(f"{where}: typedef struct {tag} is named {name}")
        structs[name] = _struct(name, body, where)
    if len(structs) != len(re.findall(r"\bstruct\s*\w*\s*\{", text)):
        raise ValueError(f"{where}: a struct that is not of the form `typedef struct X {{ fields }} X;`")
    signatures = {}
    for ret, name, params in _PROTOTYPE.findall(text):
        what = f"{where}: `{_words(ret)} {name}({_words(params)})`"
        if _words(ret) not in _RETURNS:
            raise ValueError(f"{what}: return type is not in the C ABI's vocabulary")
        restype = ctypes.c_char_p if "*" in ret else _SCALARS[_words(ret)]
        params = [] if _words(params) in ("", "void") else params.split(",")
        signatures[name] = (restype, [_param(p, what) for p in params])
    near = set(re.findall(r"\b(dspn_\w+)\s*\(", text)) - set(signatures)
    if near:
        raise ValueError(f"{where}: {sorted(near)} look like prototypes and do not parse as `<ret> dspn_name(<params>);`")
    return signatures, structs, defines


def parse(include_dir=INCLUDE_DIR):
    """every header of include_dir, merged; a name declared twice raises"""
    merged = {}, {}, {}
    for path in sorted(glob.glob(os.path.join(include_dir, "*.h"))):
        with open(path) as f:
            parts = parse_text(f.read(), os.path.basename(path))
        for into, part in zip(merged, parts):
            twice = set(into) & set(part)
            if twice:
                raise ValueError(f"{os.path.basename(path)}: {sorted(twice)} declared in an earlier header too")
            into.update(part)
    return merged


def dtype_of(struct):
    """the numpy dtype of a ctypes.Structure from the headers: its names, offsets and size; an array field is (base, shape)"""
    formats = []
    for _, ctype in struct._fields_:
        shape = ()
        while issubclass(ctype, ctypes.Array):
            shape, ctype = shape + (ctype._length_,), ctype._type_
        base = np.dtype("<u8" if ctype is ctypes.c_void_p else ctype)
        formats.append((base, shape) if shape else base)
    names = [name for name, _ in struct._fields_]
    return np.dtype({"names": names, "formats": formats, "offsets": [getattr(struct, n).offset for n in names],
                     "itemsize": ctypes.sizeof(struct)})


def fields_of(struct):
    """the same layout as a numpy field list [(name, format) | (name, format, shape)], for a struct without padding"""
    dt = dtype_of(struct)
    fields = [(n,) + ((dt[n].base.str, dt[n].shape) if dt[n].shape else (dt[n].str,)) for n in dt.names]
    assert np.dtype(fields) == dt, f"{struct.__name__} has padding: no field list describes it"
    return fields
