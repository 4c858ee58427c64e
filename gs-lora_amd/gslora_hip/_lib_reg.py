"""ctypes binding of libgslora_reg.so (C ABI declared in include/gslora_reg.h): importance accumulation, MAS's mean-of-squares objective and
the batched quadratic regulariser of the L2 / EWC / MAS baselines, with their tensor-level wrappers. The library is opened on first use: a
process that trains LoRA only, or the head only, never loads it. As for every library here there is NO fallback: a missing library or
a refused call raises RuntimeError.
"""
import ctypes as C
import os

import torch

from ._cdll import LazyLib, _ptr, _stream, columns

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgslora_reg.so")

EWC, MAS = 0, 1


class RegEntry(C.Structure):
    """gsr_reg_entry of include/gslora_reg.h, field for field."""
    _fields_ = [("p", C.c_void_p), ("p0", C.c_void_p), ("omega", C.c_void_p), ("n", C.c_long), ("chunk", C.c_long), ("goff", C.c_long),
                ("blk0", C.c_int), ("nblk", C.c_int)]


_vp, _i, _l, _f = C.c_void_p, C.c_int, C.c_long, C.c_float
_lp = C.POINTER(C.c_long)

# name -> argtypes (restype is int unless listed in _RESTYPES)
SIGNATURES = {
    "gsr_last_error": [],
    "gsr_importance_acc": [_vp, _vp, _l, _i, _f, _f, _vp, _vp, _vp],
    "gsr_sq_mean_ws_elems": [_i, _i],
    "gsr_sq_mean_fwd": [_vp, _l, _i, _i, _vp, _vp, _vp],
    "gsr_sq_mean_bwd": [_vp, _l, _vp, _vp, _l, _i, _i, _vp],
    "gsr_reg_multi_layout": [C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _lp, _i, _i, C.POINTER(RegEntry), _lp, _lp, _lp],
    "gsr_reg_multi_fwd": [_vp, _i, _l, _vp, _vp, _vp],
    "gsr_reg_multi_bwd": [_vp, _i, _i, _l, _vp, _vp, _vp],
}
_RESTYPES = {"gsr_last_error": C.c_char_p, "gsr_sq_mean_ws_elems": C.c_long}

_L = LazyLib(lambda: LIB_PATH, SIGNATURES, _RESTYPES, "gsr_last_error", "The regularisation baselines have no fallback.")
load, loaded, check = _L.load, _L.loaded, _L.check


def _flat_f32(t, what):
    if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
        raise RuntimeError(f"gslora_hip: {what} must be a contiguous f32 tensor on a ROCm GPU (the HIP path has no CPU fallback)")


def importance_acc(omega, g, kind, a, b, guard=None, skipped=None):
    """omega += (g * g) * a / b (kind EWC) or |g| / b (kind MAS), in place; every operation rounded on its own. guard: the device float of a
    loss-scaled fp16 backward (the update is skipped when it reads >= 65504 or is not finite); skipped: a device int32 counted up then."""
    _flat_f32(omega, "omega")
    _flat_f32(g, "the gradient")
    if omega.numel() != g.numel():
        raise ValueError(f"importance_acc: omega has {omega.numel()} elements, the gradient {g.numel()}")
    check(load().gsr_importance_acc(omega.data_ptr(), g.data_ptr(), omega.numel(), int(kind), float(a), float(b), _ptr(guard), _ptr(skipped),
                                    _stream()), "gsr_importance_acc")
    return omega


def sq_mean_ws_elems(B, C_):
    return _L.nonneg(load().gsr_sq_mean_ws_elems(B, C_), f"gsr_sq_mean_ws_elems({B}, {C_})")


def sq_mean_fwd(x, out, ws=None):
    """out[0] = mean(x ** 2) of a 2-D f32 view with unit column stride."""
    B, C_ = x.shape
    if ws is None:
        ws = torch.empty(sq_mean_ws_elems(B, C_), device=x.device, dtype=torch.float32)
    check(load().gsr_sq_mean_fwd(x.data_ptr(), max(x.stride(0), C_), B, C_, out.data_ptr(), ws.data_ptr(), _stream()), "gsr_sq_mean_fwd")
    return out


def sq_mean_bwd(x, gout, dx):
    """dx = (gout[0] / (B * C)) * (2 * x); gout: a device float; x, dx: 2-D f32 views with unit column stride."""
    B, C_ = x.shape
    check(load().gsr_sq_mean_bwd(x.data_ptr(), max(x.stride(0), C_), gout.data_ptr(), dx.data_ptr(), max(dx.stride(0), C_), B, C_, _stream()),
          "gsr_sq_mean_bwd")
    return dx


def reg_multi_layout(entries, n_terms, n_tensors):
    """entries: (p_ptr, p0_ptr, omega_ptr or None, n) per (term, tensor), term-major. -> (table: a ctypes array of RegEntry, total_blocks,
    bwd_blocks, g_elems). A host function: nothing is launched."""
    ne = n_terms * n_tensors
    if len(entries) != ne:
        raise ValueError(f"reg_multi_layout: {len(entries)} entries for {n_terms} terms of {n_tensors} tensors")
    P, P0, OM, N = columns(entries, _vp, _vp, _vp, _l)
    table = (RegEntry * ne)()
    tot, bwd, ge = C.c_long(), C.c_long(), C.c_long()
    check(load().gsr_reg_multi_layout(P, P0, OM, N, n_terms, n_tensors, table, C.byref(tot), C.byref(bwd), C.byref(ge)), "gsr_reg_multi_layout")
    return table, tot.value, bwd.value, ge.value


def reg_multi_fwd(table_dev, n_entries, total_blocks, out, ws):
    check(load().gsr_reg_multi_fwd(table_dev.data_ptr(), n_entries, total_blocks, out.data_ptr(), ws.data_ptr(), _stream()), "gsr_reg_multi_fwd")
    return out


def reg_multi_bwd(table_dev, n_terms, n_tensors, bwd_blocks, coef, g):
    check(load().gsr_reg_multi_bwd(table_dev.data_ptr(), n_terms, n_tensors, bwd_blocks, coef.data_ptr(), g.data_ptr(), _stream()), "gsr_reg_multi_bwd")
    return g
