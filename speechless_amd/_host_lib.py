"""ctypes binding of include/speechless_host.h (libspeechless_host.so: batch packer, n-gram model, CTC beam search), derived
from the header (_cdecl.py).  No torch here: these are plain host helpers.  Missing library or symbol -> raises."""
import ctypes
from pathlib import Path

from . import _cdecl

LIB_PATH = Path(__file__).resolve().parent / "libspeechless_host.so"

HEADER = _cdecl.load("speechless_host.h")
# name -> (restype, argtypes); every symbol include/speechless_host.h declares
HOST_SIGNATURES = HEADER.functions

_HOST_LIB = None


def host_lib():
    """The loaded library with typed entry points.  CDLL: ctypes releases the GIL while a call runs, so packing and
    beam search do not compete with the training thread."""
    global _HOST_LIB
    if _HOST_LIB is None:
        if not LIB_PATH.exists():
            raise RuntimeError("{} is missing: run `python -m speechless_amd.build`".format(LIB_PATH))
        lib = ctypes.CDLL(str(LIB_PATH))
        for name, (restype, argtypes) in HOST_SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is missing -> loud
            fn.restype = restype
            fn.argtypes = argtypes
        if lib.sl_host_version() != HEADER.constants["SL_HOST_VERSION"]:
            raise RuntimeError("libspeechless_host.so version mismatch")
        _HOST_LIB = lib
    return _HOST_LIB
