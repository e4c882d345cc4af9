"""ctypes loader of the in-tree HIP shared library (fhestring_amd/libfhestring_hip.so).

There is no CPU fallback: if the library is missing this raises, and every
entry point fails loudly when no MI355X is visible (fhs_ctx_create returns an
error that FhsError carries).
"""
import ctypes as C
import importlib
import importlib.util
import os
import sys

from . import cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
# FHS_LIB_PATH: load another build of the same library (kernel experiments: tools/ablate_fft.py); never a fallback
LIB_PATH = os.environ.get("FHS_LIB_PATH") or os.path.join(_HERE, "libfhestring_hip.so")

_lib = None


class FhsError(RuntimeError):
    code = None   # the FHS_ERR_* value where the error came from a library call that returned one


def hip_runtimes():
    """Paths of the HIP runtimes (libamdhip64) mapped into this process."""
    seen = []
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.rsplit(None, 1)[-1]
                if os.path.basename(path).startswith("libamdhip64") and path not in seen:
                    seen.append(path)
    except OSError:
        pass
    return seen


def check_single_hip_runtime():
    """Raise FhsError when two HIP runtimes are mapped into the process.

    PyTorch ships its own libamdhip64 / libhsa-runtime64 next to /opt/rocm's.  The dynamic loader shares ONE copy only
    when torch's is already there (this library's DT_NEEDED then resolves to it by SONAME); loaded in the other order,
    torch's RPATH maps a second runtime beside /opt/rocm's and the first GPU call of either side can crash the process
    (the segmentation faults of round 2's `call_b.log`: two pytest processes that loaded this library, then torch).
    """
    rts = hip_runtimes()
    if len(rts) > 1:
        raise FhsError(
            "two HIP runtimes are mapped into this process (%s): `import torch` BEFORE fhestring_amd "
            "(or not at all) so that both sides share one; refusing to touch the GPU" % ", ".join(rts))


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FhsError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
        # Load order (see check_single_hip_runtime): if torch is installed but not imported yet, import it first so
        # that a later `import torch` of the host program cannot map a second runtime.  FHS_SKIP_TORCH_PRELOAD=1
        # opts out (hosts that never use torch); the check below and in Context() still guards the process.
        if (not hip_runtimes() and "torch" not in sys.modules and not os.environ.get("FHS_SKIP_TORCH_PRELOAD")
                and importlib.util.find_spec("torch") is not None):
            importlib.import_module("torch")
        _lib = C.CDLL(LIB_PATH)
        check_single_hip_runtime()
        _declare(_lib)
    return _lib


_SCALARS = {"int": C.c_int, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "uint8_t": C.c_uint8,
            "int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}


def _fields(struct):
    return [(f, _SCALARS[t.base]) for f, t in dict(cabi.parse_header()["structs"])[struct]]


class CaptureRec(C.Structure):
    _fields_ = _fields("fhs_capture_rec")


class Stats(C.Structure):
    _fields_ = _fields("fhs_stats")


def _declare(L):
    """argtypes / restype of every function the header declares.  Scalars map exactly and `char *` is c_char_p; every
    other pointer, array parameter and function-pointer typedef is c_void_p, which takes ctypes arrays, byref(),
    ndarray.ctypes.data_as(), bytes, None and ints but not a bare ndarray.  Only a returned `T *` keeps its pointee."""
    h = cabi.parse_header()
    scalars = dict(_SCALARS)
    scalars.update((name, scalars[t.base]) for name, t in h["aliases"])
    scalars.update((name, C.c_void_p) for name, _, _ in h["fnptrs"])

    def ctype(t, ret=False):
        if t is None:
            return None
        if t.ptr == 0:
            return scalars[t.base]
        if t.ptr == 1 and t.base == "char":
            return C.c_char_p
        if ret and t.ptr == 1 and t.base in scalars:
            return C.POINTER(scalars[t.base])
        return C.c_void_p

    for name, ret, args in h["funcs"]:
        f = getattr(L, name)          # AttributeError: the header declares a symbol the library lacks
        f.argtypes = [ctype(t) for _, t in args]
        f.restype = ctype(ret, ret=True)


def live_resources():
    """fhs_debug_live_resources: [device bytes, pinned bytes, events, streams] this library holds now, acquisitions so far."""
    out = (C.c_uint64 * 5)()
    if lib().fhs_debug_live_resources(out):
        raise FhsError("fhs_debug_live_resources failed")
    return list(out)


def fft_tables():
    """Host-derived twiddle tables of the F64_FFT arithmetic (diagnostic)."""
    import numpy as np
    w_re, w_im = np.zeros(1024), np.zeros(1024)
    u_re, u_im = np.zeros(16), np.zeros(16)
    dp = C.POINTER(C.c_double)
    lib().fhs_fft_tables(*(a.ctypes.data_as(dp) for a in (w_re, w_im, u_re, u_im)))
    return w_re, w_im, u_re, u_im
