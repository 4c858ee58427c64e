"""ctypes binding of libgslora_fd.so (C ABI declared in include/gslora_fd.h): the row distance between a student's and a frozen teacher's
outputs — the regulariser of the DER / DER++ and FDR baselines — with its tensor-level wrappers. The library is opened on first use: a process
that takes no DER or FDR step never loads it. As for every library here there is NO fallback: a missing library or a refused call
raises RuntimeError.
"""
import ctypes as C
import os

import torch

from ._cdll import LazyLib, _ld, _stream

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgslora_fd.so")

FD_WAVE, FD_BLOCK = 0, 1
FD_SQ, FD_ROWNORM = 0, 1
MODES = {"sq": FD_SQ, "rownorm": FD_ROWNORM}

_vp, _i, _l, _f = C.c_void_p, C.c_int, C.c_long, C.c_float
_lp, _ip = C.POINTER(C.c_long), C.POINTER(C.c_int)

# name -> argtypes (restype is int unless listed in _RESTYPES)
SIGNATURES = {
    "gsf_last_error": [],
    "gsf_rowdist_plan": [_i, _i, _ip, _ip, _lp],
    "gsf_rowdist_ws_elems": [_i, _i],
    "gsf_rowdist_fwd": [_vp, _l, _vp, _l, _i, _i, _i, _vp, _vp, _vp],
    "gsf_rowdist_bwd": [_vp, _l, _vp, _l, _vp, _vp, _i, _i, _i, _f, _vp, _l, _i, _vp],
}
_RESTYPES = {"gsf_last_error": C.c_char_p, "gsf_rowdist_ws_elems": C.c_long}

_L = LazyLib(lambda: LIB_PATH, SIGNATURES, _RESTYPES, "gsf_last_error", "The DER / FDR baselines have no fallback.")
load, loaded, check = _L.load, _L.loaded, _L.check


def rowdist_plan(B, W):
    """-> (kernel: FD_WAVE or FD_BLOCK, grid, ws_elems): the rule gsf_rowdist_fwd / gsf_rowdist_bwd launch by. A host function."""
    k, g, w = C.c_int(), C.c_int(), C.c_long()
    check(load().gsf_rowdist_plan(B, W, C.byref(k), C.byref(g), C.byref(w)), "gsf_rowdist_plan")
    return k.value, g.value, w.value


def rowdist_ws_elems(B, W):
    return _L.nonneg(load().gsf_rowdist_ws_elems(B, W), f"gsf_rowdist_ws_elems({B}, {W})")


def _rows(t, what):
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise RuntimeError(f"gslora_hip.fd: {what} must be a [B, W] f32 tensor on a ROCm GPU with unit column stride (the HIP path has no CPU "
                           "fallback)")


def rowdist_fwd(a, t, mode, out1, ws):
    """out1[0] = the distance of the [B, W] f32 rows a and t in `mode` (FD_SQ / FD_ROWNORM); ws: rowdist_ws_elems(B, W) floats, kept for
    rowdist_bwd."""
    _rows(a, "the student's rows")
    _rows(t, "the teacher's rows")
    B, W = a.shape
    check(load().gsf_rowdist_fwd(a.data_ptr(), _ld(a), t.data_ptr(), _ld(t), B, W, int(mode), out1.data_ptr(), ws.data_ptr(), _stream()),
          "gsf_rowdist_fwd")
    return out1


def rowdist_bwd(a, t, ws, gout, mode, coef, d, accumulate=False):
    """d (+)= gout[0] * coef * d(distance) / d a; gout: a device float; ws: what rowdist_fwd left."""
    B, W = a.shape
    check(load().gsf_rowdist_bwd(a.data_ptr(), _ld(a), t.data_ptr(), _ld(t), ws.data_ptr(), gout.data_ptr(), B, W, int(mode), float(coef),
                                 d.data_ptr(), _ld(d), 1 if accumulate else 0, _stream()), "gsf_rowdist_bwd")
    return d
