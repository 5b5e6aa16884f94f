"""ctypes binding of libdspn_hip.so (the C ABI declared in include/*.h).

The HIP library is the product: there is no CPU or PyTorch fallback.  If the
shared object is missing or a symbol cannot be resolved, importing an operator
raises immediately.
"""
import ctypes
import os

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# DSPN_LIB: another build of the SAME library (A/B timing of two builds on one box); never a fallback
LIB_PATH = os.environ.get("DSPN_LIB") or os.path.join(_HERE, "libdspn_hip.so")

# include/*.h is the one place the C ABI is written: name -> (restype, [argtypes]) of every entry point (a pointer or array
# argument is c_void_p), name -> ctypes.Structure of every descriptor struct, name -> value of every integer-literal #define
SIGNATURES, STRUCTS, DEFINES = _abi.parse()


def layout(struct_name):
    """the numpy dtype of a descriptor struct of include/*.h"""
    return _abi.dtype_of(STRUCTS[struct_name])


def field_list(struct_name):
    """the same as a numpy field list (a struct without padding)"""
    return _abi.fields_of(STRUCTS[struct_name])


class DspnError(RuntimeError):
    """Raised when a C-ABI call returns a non-zero status (the MXNetError analogue)."""


_lib = None


def _bind(lib, signatures):
    for name, (res, args) in signatures.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise ImportError(f"{LIB_PATH} does not export {name}; rebuild with "
                              f"`make -C dspnet_amd/csrc`") from e
        fn.restype = res
        fn.argtypes = args


def lib():
    """Load (once) and return the ctypes handle.  Fails loudly if the .so is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
                f"Build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
                f"`make -C dspnet_amd/csrc`.")
        handle = ctypes.CDLL(LIB_PATH)
        _bind(handle, SIGNATURES)
        _lib = handle
    return _lib


def check(status, what=""):
    if status != 0:
        msg = lib().dspn_last_error().decode("utf-8", "replace")
        raise DspnError(f"{what}: {msg} (status {status})" if what else f"{msg} (status {status})")


def floats(values):
    arr = (ctypes.c_float * len(values))(*[float(v) for v in values])
    return arr
