"""ctypes binding of include/speechless_hip.h, derived from the header itself (_cdecl.py): a new entry point, struct field or
constant is declared in the header and nowhere else.  There is NO fallback: if the HIP library is missing or a call fails, this
raises -- the product path never computes on the CPU."""
import ctypes
from pathlib import Path

# torch FIRST: its wheel bundles its own libamdhip64.so.7 / libhsa-runtime64.  libspeechless_hip.so needs the same
# SONAME, and a process must hold exactly ONE HIP runtime -- the one that owns the tensors' memory and streams.
# Loading ours first would pull /opt/rocm's runtime in and torch would then find "no ROCm-capable device".
import torch  # noqa: F401  (plumbing: device memory, streams, torch.distributed)

import os

from . import _cdecl
from .launch_list import HipLibraryError, raise_status  # noqa: F401  (the error every failing library call raises)

# SL_LIB_PATH: experiments only (a probe build of the library next to the real one)
LIB_PATH = Path(os.environ.get("SL_LIB_PATH") or Path(__file__).resolve().parent / "libspeechless_hip.so")


class AdamLayer(ctypes.Structure):
    """Mirror of sl_adam_layer (include/speechless_hip.h)."""


class OptRule(ctypes.Structure):
    """Mirror of sl_opt_rule (include/speechless_hip.h)."""


class BgwLayer(ctypes.Structure):
    """Mirror of sl_bgw_layer (include/speechless_hip.h)."""


class NormRange(ctypes.Structure):
    """Mirror of sl_norm_range (include/speechless_hip.h)."""


class ConvGeom(ctypes.Structure):
    """Mirror of sl_conv_geom (include/speechless_hip.h)."""

    def copy_from(self, src):
        for name, _ in ConvGeom._fields_:
            setattr(self, name, getattr(src, name))

    def copy(self):
        g = ConvGeom()
        g.copy_from(self)
        return g


class BeamLm(ctypes.Structure):
    """Mirror of sl_beam_lm (include/speechless_hip.h): device pointers of the flat scorer tables."""


class WgradJob(ctypes.Structure):
    """Mirror of sl_wgrad_job (include/speechless_hip.h)."""


# The classes above take their _fields_ from the header's typedefs; WgradJob.geom is ConvGeom itself
HEADER = _cdecl.load("speechless_hip.h", {"sl_adam_layer": AdamLayer, "sl_opt_rule": OptRule, "sl_bgw_layer": BgwLayer,
                                          "sl_norm_range": NormRange, "sl_conv_geom": ConvGeom, "sl_beam_lm": BeamLm,
                                          "sl_wgrad_job": WgradJob})
# name -> (restype, argtypes); every symbol include/speechless_hip.h declares
SIGNATURES = HEADER.functions


def _constants(prefix, *names):
    return [HEADER.constants[prefix + name] for name in names]


SL_VERSION, SL_TIME_TILE, SL_BF16, SL_F32, SL_F16 = _constants("SL_", "VERSION", "TIME_TILE", "BF16", "F32", "F16")
SL_RESAMPLE_TILE, SL_RESAMPLE_MAX_PHASES, SL_RESAMPLE_MAX_TAPS = _constants("SL_RESAMPLE_", "TILE", "MAX_PHASES", "MAX_TAPS")
# sl_stft `mode`
STFT_POWER, STFT_AMPLITUDE, STFT_COMPLEX, STFT_POWER_LEVEL = _constants(
    "SL_STFT_", "POWER", "AMPLITUDE", "COMPLEX", "POWER_LEVEL")
EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_RELU_MASK, EPI_BIAS_ELU, EPI_ELU_MASK = _constants(
    "SL_EPI_", "NONE", "BIAS", "BIAS_RELU", "RELU_MASK", "BIAS_ELU", "ELU_MASK")
# the number of fp32 state slots per parameter of each rule (in the header's prose only), and its SL_OPT_* number
OPT_SLOTS = {"adam": 2, "sgd": 1, "rmsprop": 1, "adagrad": 1, "adadelta": 2, "adamax": 2}
OPT_RULES = {name: HEADER.constants["SL_OPT_" + name.upper()] for name in OPT_SLOTS}

# The header gives the values of these three arguments in prose only.
# sl_conv1d_nt's out_f32: the output in the element type, as fp32 rows, or as hi + lo planes out of the epilogue
NT_OUT_ELEM, NT_OUT_F32, NT_OUT_PLANES = 0, 1, 2
# sl_split3 / sl_splitf16 `mode`: fp32 rows into planes as they are, through ReLU / ELU, or times the ReLU / ELU derivative
# taken from the stored activation (`mask`)
SPLIT_COPY, SPLIT_RELU, SPLIT_ELU, SPLIT_RELU_MASK, SPLIT_ELU_MASK = 0, 1, 2, 3, 4
# sl_split3_dropout / sl_splitf16_dropout `mode`: forward; the 1 / (1 - rate) left behind a ReLU mask; keep * elu' behind an ELU
DROP_FORWARD, DROP_SCALE, DROP_ELU_BACKWARD = 0, 1, 2


class HipLibrary:
    """Loaded libspeechless_hip.so with typed entry points.  `call(name, *args)` raises on a non-zero status."""

    def __init__(self, path=LIB_PATH):
        path = Path(path)
        if not path.exists():
            raise HipLibraryError(
                "{} not found: build it with `python -m speechless_amd.build` (or __graft_entry__.build()). "
                "The speechless_amd hot path has no CPU fallback.".format(path))
        self.path = path
        # PyDLL: the GIL is NOT released around a call.  Every entry point only enqueues work (microseconds); with CDLL
        # each of the ~60 launches of a step hands the GIL to the input pipeline's worker threads and has to win it back
        # (up to the interpreter's 5 ms switch interval) before the next launch can be issued.
        self._dll = ctypes.PyDLL(str(path)) if os.environ.get("SL_RELEASE_GIL", "0") != "1" else ctypes.CDLL(str(path))
        self._fn = {}
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(self._dll, name)  # AttributeError if the symbol is missing -> loud
            fn.restype = restype
            fn.argtypes = argtypes
            self._fn[name] = fn
        if self._fn["sl_version"]() != SL_VERSION:
            raise HipLibraryError("libspeechless_hip.so version mismatch")

    def raw(self, name):
        return self._fn[name]

    def last_error(self):
        msg = self._fn["sl_last_error"]()
        return msg.decode("utf8", "replace") if msg else ""

    def call(self, name, *args):
        rc = self._fn[name](*args)
        if rc != 0:
            raise_status(name, rc, self.last_error)


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = HipLibrary()
    return _LIB
