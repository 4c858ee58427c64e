"""ctypes binding of libgslora_kd.so (C ABI declared in include/gslora_kd.h): the distillation + cross-entropy row loss and the batched
parameter distance of the SCRUB baseline, with their tensor-level wrappers. The library is opened on first use: a process that runs no SCRUB
step never loads it. As for every library here there is NO fallback: a missing library or a refused call raises RuntimeError.
"""
import ctypes as C
import os

import torch

from ._cdll import LazyLib, _ld, _ptr, _stream, columns, table_to_device      # (table_to_device: tests reach it through this binding)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgslora_kd.so")

KD_WAVE, KD_BLOCK = 0, 1


class DistEntry(C.Structure):
    """gsk_dist_entry of include/gslora_kd.h, field for field."""
    _fields_ = [("p", C.c_void_p), ("q", C.c_void_p), ("n", C.c_long), ("chunk", C.c_long), ("goff", C.c_long), ("blk0", C.c_int),
                ("nblk", C.c_int), ("bblk0", C.c_int), ("pad_", C.c_int)]


_vp, _i, _l, _f = C.c_void_p, C.c_int, C.c_long, C.c_float
_lp, _ip = C.POINTER(C.c_long), C.POINTER(C.c_int)

# name -> argtypes (restype is int unless listed in _RESTYPES)
SIGNATURES = {
    "gsk_last_error": [],
    "gsk_kd_plan": [_i, _i, _ip, _ip, _lp],
    "gsk_kd_ws_elems": [_i, _i],
    "gsk_kd_ce_fwd": [_vp, _l, _vp, _l, _vp, _i, _i, _f, _f, _f, _vp, _vp, _vp],
    "gsk_kd_ce_bwd": [_vp, _l, _vp, _l, _vp, _vp, _vp, _i, _i, _f, _f, _f, _vp, _l, _i, _vp],
    "gsk_param_dist_layout": [C.POINTER(_vp), C.POINTER(_vp), _lp, _ip, _i, C.POINTER(DistEntry), _lp, _lp, _lp],
    "gsk_param_dist_fwd": [_vp, _i, _l, _f, _vp, _vp, _vp, _vp],
    "gsk_param_dist_bwd": [_vp, _i, _l, _f, _vp, _vp, _vp, _vp],
}
_RESTYPES = {"gsk_last_error": C.c_char_p, "gsk_kd_ws_elems": C.c_long}

_L = LazyLib(lambda: LIB_PATH, SIGNATURES, _RESTYPES, "gsk_last_error", "The SCRUB baseline has no fallback.")
load, loaded, check = _L.load, _L.loaded, _L.check


def kd_plan(B, C_):
    """-> (kernel: KD_WAVE or KD_BLOCK, grid, ws_elems): the rule gsk_kd_ce_fwd / gsk_kd_ce_bwd launch by. A host function."""
    k, g, w = C.c_int(), C.c_int(), C.c_long()
    check(load().gsk_kd_plan(B, C_, C.byref(k), C.byref(g), C.byref(w)), "gsk_kd_plan")
    return k.value, g.value, w.value


def kd_ws_elems(B, C_):
    return _L.nonneg(load().gsk_kd_ws_elems(B, C_), f"gsk_kd_ws_elems({B}, {C_})")


def _logits(t, what):
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise RuntimeError(f"gslora_hip.kd: {what} must be a [B, C] f32 tensor on a ROCm GPU with unit column stride (the HIP path has no CPU "
                           "fallback)")


def kd_ce_fwd(ys, yt, labels, T, c_kd, c_ce, out3, ws):
    """out3 = [KD, CE, c_kd * KD + c_ce * CE] of [B, C] f32 student / teacher logits; ws: kd_ws_elems(B, C) floats, kept for kd_ce_bwd."""
    _logits(ys, "the student's logits")
    _logits(yt, "the teacher's logits")
    B, C_ = ys.shape
    check(load().gsk_kd_ce_fwd(ys.data_ptr(), _ld(ys), yt.data_ptr(), _ld(yt), _ptr(labels), B, C_, float(T), float(c_kd), float(c_ce),
                               out3.data_ptr(), ws.data_ptr(), _stream()), "gsk_kd_ce_fwd")
    return out3


def kd_ce_bwd(ys, yt, labels, ws, gout, T, c_kd, c_ce, d, accumulate=False):
    """d (+)= gout[0] * d(c_kd * KD + c_ce * CE) / d ys; gout: a device float; ws: what kd_ce_fwd left."""
    B, C_ = ys.shape
    check(load().gsk_kd_ce_bwd(ys.data_ptr(), _ld(ys), yt.data_ptr(), _ld(yt), _ptr(labels), ws.data_ptr(), gout.data_ptr(), B, C_, float(T),
                               float(c_kd), float(c_ce), d.data_ptr(), _ld(d), 1 if accumulate else 0, _stream()), "gsk_kd_ce_bwd")
    return d


def param_dist_layout(entries):
    """entries: (p_ptr, q_ptr, n, trainable) per tensor, in parameter order. -> (table: a ctypes array of DistEntry, total_blocks, bwd_blocks,
    g_elems). A host function: nothing is launched."""
    ne = len(entries)
    P, Q, N, TR = columns(entries, _vp, _vp, _l, _i)      # (a bool is a ctypes int of 0 or 1)
    table = (DistEntry * max(ne, 1))()
    tot, bwd, ge = C.c_long(), C.c_long(), C.c_long()
    check(load().gsk_param_dist_layout(P, Q, N, TR, ne, table, C.byref(tot), C.byref(bwd), C.byref(ge)), "gsk_param_dist_layout")
    return table, tot.value, bwd.value, ge.value


def param_dist_fwd(table_dev, n_entries, total_blocks, p, out, norms, ws):
    check(load().gsk_param_dist_fwd(table_dev.data_ptr(), n_entries, total_blocks, float(p), out.data_ptr(), norms.data_ptr(), ws.data_ptr(),
                                    _stream()), "gsk_param_dist_fwd")
    return out


def param_dist_bwd(table_dev, n_entries, bwd_blocks, p, gout, norms, g):
    check(load().gsk_param_dist_bwd(table_dev.data_ptr(), n_entries, bwd_blocks, float(p), gout.data_ptr(), norms.data_ptr(), g.data_ptr(),
                                    _stream()), "gsk_param_dist_bwd")
    return g
