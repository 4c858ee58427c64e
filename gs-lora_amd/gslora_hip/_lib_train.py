"""ctypes binding of libgslora_train.so (C ABI declared in include/gslora_train.h): the weight-gradient GEMM and the quadratic regulariser
of the FFN-training step, with their tensor-level wrappers. The library is opened on first use: a process that trains LoRA only never
loads it. As for libgslora_hip.so there is NO fallback: a missing library or a refused call raises RuntimeError.
"""
import ctypes as C
import os

import torch

from ._cdll import LazyLib, _ptr, _stream
from ._lib import BF16, F16, F32

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgslora_train.so")

_vp, _i, _l = C.c_void_p, C.c_int, C.c_long
_ip = C.POINTER(C.c_int)

# name -> argtypes (restype is int unless listed in _RESTYPES)
SIGNATURES = {
    "gst_last_error": [],
    "gst_wgrad_ws_elems": [_i, _i, _i, _i],
    "gst_wgrad_plan": [_i, _i, _i, _i, _ip, _ip, _ip, _ip],
    "gst_wgrad": [_vp, _l, _vp, _l, _vp, _l, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp],
    "gst_reg_quad_ws_elems": [_l],
    "gst_reg_quad_fwd": [_vp, _vp, _vp, _l, _vp, _i, _vp, _vp],
    "gst_reg_quad_bwd": [_vp, _vp, _vp, _l, _vp, _vp, _vp],
}
_RESTYPES = {"gst_last_error": C.c_char_p, "gst_wgrad_ws_elems": C.c_long, "gst_reg_quad_ws_elems": C.c_long}

_L = LazyLib(lambda: LIB_PATH, SIGNATURES, _RESTYPES, "gst_last_error", "Training FFN weights has no fallback.")
load, loaded, check = _L.load, _L.loaded, _L.check

_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}


def wgrad_ws_elems(M, N, K, dtype):
    return _L.nonneg(load().gst_wgrad_ws_elems(M, N, K, _DT[dtype]), f"gst_wgrad_ws_elems({M}, {N}, {K})")


def wgrad_plan(M, N, K, dtype):
    """-> (tile_n, tile_k, nsplit, rows_per_split): what a gst_wgrad launch of this shape uses."""
    v = [C.c_int() for _ in range(4)]
    check(load().gst_wgrad_plan(M, N, K, _DT[dtype], *(C.byref(x) for x in v)), "gst_wgrad_plan")
    return tuple(x.value for x in v)


def wgrad(Y, X, dW, db=None, accumulate=False, ws=None, gscale=None):
    """dW [N, K] (+)= c Y^T X, db [N] (+)= c colsum(Y). Y [M, N], X [M, K]: 2-D views with unit column stride in one of f32 / bf16 / fp16;
    dW, db f32 (dW a 2-D view with unit column stride). ws: f32 workspace of at least wgrad_ws_elems (allocated here when None)."""
    M, N = Y.shape
    K = X.shape[1]
    if X.shape[0] != M or X.dtype != Y.dtype or Y.stride(1) != 1 or X.stride(1) != 1 or dW.stride(1) != 1 or tuple(dW.shape) != (N, K):
        raise ValueError(f"wgrad: Y {tuple(Y.shape)} {Y.dtype}, X {tuple(X.shape)} {X.dtype}, dW {tuple(dW.shape)}: shapes, dtypes or column strides disagree")
    if dW.dtype != torch.float32 or (db is not None and (db.dtype != torch.float32 or db.numel() != N or not db.is_contiguous())):
        raise ValueError("wgrad: dW and db are f32, db contiguous [N]")
    if ws is None:
        ws = torch.empty(wgrad_ws_elems(M, N, K, Y.dtype), device=Y.device, dtype=torch.float32)
    elif ws.dtype != torch.float32 or ws.numel() < wgrad_ws_elems(M, N, K, Y.dtype):
        raise ValueError("wgrad: the workspace is smaller than gst_wgrad_ws_elems asks for")
    ldy = Y.stride(0) if M > 1 else max(Y.stride(0), N)
    ldx = X.stride(0) if M > 1 else max(X.stride(0), K)
    check(load().gst_wgrad(Y.data_ptr(), ldy, X.data_ptr(), ldx, dW.data_ptr(), dW.stride(0) if N > 1 else max(dW.stride(0), K), _ptr(db),
                           M, N, K, _DT[Y.dtype], int(bool(accumulate)), ws.data_ptr(), _ptr(gscale), _stream()), "gst_wgrad")
    return dW, db


def reg_quad_fwd(p, p0, omega, out, accumulate=False, ws=None):
    """out[0] (+)= sum omega (p - p0)^2 over flat f32 tensors (omega None: 1)."""
    n = p.numel()
    if ws is None:
        ws = torch.empty(load().gst_reg_quad_ws_elems(n), device=p.device, dtype=torch.float32)
    check(load().gst_reg_quad_fwd(p.data_ptr(), p0.data_ptr(), _ptr(omega), n, out.data_ptr(), int(bool(accumulate)), ws.data_ptr(), _stream()),
          "gst_reg_quad_fwd")
    return out


def reg_quad_bwd(p, p0, omega, coef, g):
    """g += ((coef * 2) * omega) * (p - p0); coef: a device float."""
    check(load().gst_reg_quad_bwd(p.data_ptr(), p0.data_ptr(), _ptr(omega), p.numel(), coef.data_ptr(), g.data_ptr(), _stream()), "gst_reg_quad_bwd")
    return g
