"""dspnet_amd/_abi.py on synthetic header text: the closed vocabulary of the C ABI, the layouts ctypes gives the structs, and the
declarations that must raise instead of being guessed or skipped (no library, no GPU)."""
import ctypes as c

import numpy as np
import pytest

from dspnet_amd import _abi

VP = c.c_void_p

HEADER = """
/* a header like include/dspn_*.h */
#ifndef DSPN_T_H_
#define DSPN_T_H_
#include <stddef.h>
#define DSPN_T_SLOTS 64
#define DSPN_T_FLAG 0x200   /* OR-ed into math */
#define DSPN_T_EXPR ((1 << 27) - 1)
#define DSPN_T_MACRO(x) \\
  dspn_t_not_a_prototype(x)
#ifdef __cplusplus
extern "C" {
#endif
typedef unsigned short dspn_bf16;
const char *dspn_t_last_error(void);
int dspn_t_version();
long long dspn_t_tiles(int Cout, const int taps);
size_t dspn_t_bytes(long long rows, size_t have, unsigned n, unsigned int m);
int dspn_t_scalars(int, long long, float eps, double, size_t, unsigned, unsigned int);
int dspn_t_pointers(const float *x, float*y, const dspn_bf16 *const *rows, void *stream, const double mean[3],
                    unsigned char lum[64], const char *text, const struct dspn_t_padded *p);
int dspn_t_split(const float *x,   /* the input, (rows, C) */
                 long long rows,   // a line comment, with a comma
                 int C,
                 void *stream
                );
typedef struct dspn_t_padded {
  int first;
  long long second;            /* 4 bytes of padding in front */
} dspn_t_padded;
typedef struct dspn_t_fields {
  long long coef_offset[3];
  unsigned long long base;
  int src_h, src_w;
  float gain; double sum;
  unsigned char quant[3][64], tab[4];
  short lo; unsigned short hi;
  unsigned n;
  float *moving_mean;
  const void *const *rows;
} dspn_t_fields;
#ifdef __cplusplus
}
#endif
#endif
"""


def test_vocabulary():
    sigs, structs, defines = _abi.parse_text(HEADER, "t.h")
    assert sigs == {
        "dspn_t_last_error": (c.c_char_p, []),
        "dspn_t_version": (c.c_int, []),
        "dspn_t_tiles": (c.c_longlong, [c.c_int, c.c_int]),
        "dspn_t_bytes": (c.c_size_t, [c.c_longlong, c.c_size_t, c.c_uint, c.c_uint]),
        "dspn_t_scalars": (c.c_int, [c.c_int, c.c_longlong, c.c_float, c.c_double, c.c_size_t, c.c_uint, c.c_uint]),
        "dspn_t_pointers": (c.c_int, [VP] * 8),
        "dspn_t_split": (c.c_int, [VP, c.c_longlong, c.c_int, VP]),
    }
    assert defines == {"DSPN_T_SLOTS": 64, "DSPN_T_FLAG": 0x200}, "integer literals only: no guard, no expression, no macro"
    assert sorted(structs) == ["dspn_t_fields", "dspn_t_padded"]


def test_struct_layouts():
    _, structs, _ = _abi.parse_text(HEADER, "t.h")
    padded, fields = structs["dspn_t_padded"], structs["dspn_t_fields"]
    assert issubclass(padded, c.Structure) and padded.second.offset == 8 and c.sizeof(padded) == 16
    dt = _abi.dtype_of(padded)
    assert dt.names == ("first", "second") and dt.fields["second"][1] == 8 and dt.itemsize == 16
    assert (dt["first"], dt["second"]) == (np.dtype("<i4"), np.dtype("<i8"))
    with pytest.raises(AssertionError):
        _abi.fields_of(padded)                   # a field list cannot say where the padding is

    dt = _abi.dtype_of(fields)
    assert dt.names == ("coef_offset", "base", "src_h", "src_w", "gain", "sum", "quant", "tab", "lo", "hi", "n", "moving_mean", "rows")
    assert [(dt[n].base.str, dt[n].shape) for n in dt.names] == [
        ("<i8", (3,)), ("<u8", ()), ("<i4", ()), ("<i4", ()), ("<f4", ()), ("<f8", ()), ("|u1", (3, 64)), ("|u1", (4,)), ("<i2", ()),
        ("<u2", ()), ("<u4", ()), ("<u8", ()), ("<u8", ())]
    assert [dt.fields[n][1] for n in dt.names] == [0, 24, 32, 36, 40, 48, 56, 248, 252, 254, 256, 264, 272] and dt.itemsize == 280
    assert dt.itemsize == c.sizeof(fields) and all(dt.fields[n][1] == getattr(fields, n).offset for n in dt.names)
    # an unpadded struct as a field list, the form np.zeros(n, FIELDS) takes: the same dtype
    _, structs, _ = _abi.parse_text("typedef struct s { long long offset, length; float lr[2]; } s;")
    assert _abi.fields_of(structs["s"]) == [("offset", "<i8"), ("length", "<i8"), ("lr", "<f4", (2,))]
    assert np.dtype(_abi.fields_of(structs["s"])) == _abi.dtype_of(structs["s"])


def test_the_types_are_read():
    """one parameter from int to long long changes that signature and no other"""
    a, _, _ = _abi.parse_text(HEADER, "t.h")
    b, _, _ = _abi.parse_text(HEADER.replace("long long rows,   //", "int rows,   //"), "t.h")
    assert a["dspn_t_split"][1][1] is c.c_longlong and b["dspn_t_split"][1][1] is c.c_int
    assert {n for n in a if a[n] != b[n]} == {"dspn_t_split"}


@pytest.mark.parametrize("text, names", [
    ("int dspn_t_f(const float *x, long rows);", ["t.h", "dspn_t_f", "long rows"]),                 # unknown parameter type
    ("int dspn_t_f(hipStream_t stream);", ["t.h", "dspn_t_f", "hipStream_t stream"]),
    ("int dspn_t_f(unsigned long long n);", ["t.h", "dspn_t_f", "unsigned long long n"]),
    ("void dspn_t_f(int n);", ["t.h", "dspn_t_f", "void"]),                                          # unknown return type
    ("float *dspn_t_f(int n);", ["t.h", "dspn_t_f"]),
    ("typedef struct s { int a; long b; } s;", ["t.h", "struct s", "long b"]),                      # unknown field type
    ("typedef struct s { int a; dspn_bf16 b[4]; } s;", ["t.h", "struct s", "dspn_bf16 b[4]"]),
    ("typedef struct s { int a : 3; } s;", ["t.h", "struct s"]),
    ("typedef struct s { int a; } t;", ["t.h", "struct s"]),
    ("struct s { int a; };", ["t.h", "struct"]),
    ("int dspn_t_f(int n, void (*callback)(int));", ["t.h", "dspn_t_f"]),                            # near-prototypes
    ("int dspn_t_f(int n)\nint dspn_t_g(int n);", ["t.h", "dspn_t_f"]),
    ("static inline int dspn_t_f(int n) { return n; }", ["t.h", "dspn_t_f"]),
    ("int dspn_t_f(int n, ...);", ["t.h", "dspn_t_f"]),
])
def test_what_is_not_understood_raises(text, names):
    with pytest.raises(ValueError) as e:
        _abi.parse_text(text, "t.h")
    assert all(n in str(e.value) for n in names), str(e.value)


def test_a_name_declared_in_two_headers_raises(tmp_path):
    (tmp_path / "a.h").write_text("int dspn_t_f(int n);\n")
    (tmp_path / "b.h").write_text("int dspn_t_g(int n);\n")
    assert sorted(_abi.parse(str(tmp_path))[0]) == ["dspn_t_f", "dspn_t_g"]
    (tmp_path / "c.h").write_text("long long dspn_t_f(int n);\n")
    with pytest.raises(ValueError, match="c.h.*dspn_t_f"):
        _abi.parse(str(tmp_path))
