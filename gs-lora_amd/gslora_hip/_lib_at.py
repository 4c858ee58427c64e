"""ctypes binding of libgslora_at.so (C ABI declared in include/gslora_at.h): the attention-transfer term of the LIRF baseline on the
[B, T, D] stream between the two half networks — its value, the table that carries its gradient, and the in-place gradient at the boundary.
The library is opened on first use: a process that takes no LIRF step never loads it. As for every library here there is NO fallback:
a missing library or a refused call raises RuntimeError.
"""
import ctypes as C
import os

import torch

from ._cdll import LazyLib, _ld, _stream

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgslora_at.so")

DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}      # gsl_dtype of include/gslora_hip.h
MAX_T, MAX_D = 1025, 1024

_vp, _i, _l = C.c_void_p, C.c_int, C.c_long
_lp, _ip = C.POINTER(C.c_long), C.POINTER(C.c_int)

# name -> argtypes (restype is int unless listed in _RESTYPES)
SIGNATURES = {
    "gsa_last_error": [],
    "gsa_at_plan": [_i, _i, _i, _ip, _ip, _lp],
    "gsa_at_ws_elems": [_i, _i, _i],
    "gsa_at_fwd": [_vp, _l, _vp, _l, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    "gsa_at_bwd": [_vp, _l, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _l, _i, _vp],
}
_RESTYPES = {"gsa_last_error": C.c_char_p, "gsa_at_ws_elems": C.c_long}

_L = LazyLib(lambda: LIB_PATH, SIGNATURES, _RESTYPES, "gsa_last_error", "The LIRF baseline has no fallback.")
load, loaded, check = _L.load, _L.loaded, _L.check


def at_plan(B, T, D):
    """-> (nsplit, chunk, ws_elems): how gsa_at_fwd cuts the token axis over workgroups. A host function."""
    n, c, w = C.c_int(), C.c_int(), C.c_long()
    check(load().gsa_at_plan(B, T, D, C.byref(n), C.byref(c), C.byref(w)), "gsa_at_plan")
    return n.value, c.value, w.value


def at_ws_elems(B, T, D):
    return _L.nonneg(load().gsa_at_ws_elems(B, T, D), f"gsa_at_ws_elems({B}, {T}, {D})")


def _rows(t, what, dtypes=tuple(DTYPES)):
    """`t` as the [rows, D] view the library reads: a [rows, D] tensor or a [B, T, D] one whose images follow each other (stride(0) ==
    T * stride(1))."""
    ok = torch.is_tensor(t) and t.is_cuda and t.dtype in dtypes and t.dim() in (2, 3) and t.numel() > 0 and t.stride(-1) == 1
    if ok and t.dim() == 3:
        ok = t.shape[0] == 1 or t.stride(0) == t.shape[1] * t.stride(1)
        if ok:
            t = t.as_strided((t.shape[0] * t.shape[1], t.shape[2]), (t.stride(1), 1), t.storage_offset())
    if not ok or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        names = " / ".join(str(d).replace("torch.", "") for d in dtypes)
        raise RuntimeError(f"gslora_hip.at: {what} must be a [rows, D] or [B, T, D] {names} tensor on a ROCm GPU with unit column stride and "
                           "evenly spaced rows (the HIP path has no CPU fallback)")
    return t


def _f32(t, what, n):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n):
        raise RuntimeError(f"gslora_hip.at: {what} must be a contiguous f32 tensor of {n} element(s) on a ROCm GPU (the HIP path has no CPU "
                           "fallback)")
    return t


def at_fwd(xs, xt, B, T, loss, G, ws, at_s=None, at_t=None):
    """loss[0], G[B, D] (and the optional tables at_s, at_t [B, D]) of images 0 .. B-1 of the [rows, D] streams xs, xt (one dtype)."""
    D = xs.shape[1]
    check(load().gsa_at_fwd(xs.data_ptr(), _ld(xs), xt.data_ptr(), _ld(xt), DTYPES[xs.dtype], B, T, D, loss.data_ptr(), G.data_ptr(),
                            None if at_s is None else at_s.data_ptr(), None if at_t is None else at_t.data_ptr(), ws.data_ptr(), _stream()),
          "gsa_at_fwd")
    return loss, G


def at_bwd(xs, G, coef, scale, B, T, dmid):
    """dmid[b, t, :] += coef[0] * scale[0] * G[b, :] * xs[b, t, :] over images 0 .. B-1; coef, scale: device floats."""
    D = xs.shape[1]
    check(load().gsa_at_bwd(xs.data_ptr(), _ld(xs), DTYPES[xs.dtype], G.data_ptr(), coef.data_ptr(), scale.data_ptr(), B, T, D, dmid.data_ptr(),
                            _ld(dmid), DTYPES[dmid.dtype], _stream()), "gsa_at_bwd")
    return dmid
