"""CPU tests of the host side of csrc/head.hip, csrc/norm.hip and gsl_lora_grad (csrc/lora.hip): the two things host code can change
without any kernel changing.

Refusals: every argument check of the nine entry points, reached by a call that is valid except in one argument, with its return code and
the full gsl_last_error() text. Every pointer is the address 16, never dereferenced because the check fails first; a check that went
missing would turn such a call into a launch on that address, so the module skips where a device is visible (without one such a launch
returns -2, "no ROCm-capable device is detected": a clean failure of the assertion).

Workspace sizes: gsl_lora_grad_ws_elems over an (M, N, r) grid and gsl_lora_grad_batch_ws_elems for a few descriptor lists, equal to
tests/golden/lora_grad_ws_parent.npz — what the library built from the commit before the host-side refactor returned
(`python tests/test_row_host_side_host.py OUT.npz` records the table from the library in the tree)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="build-machine test: a dropped check would launch on the address 16")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 16            # a non-null, 16-byte-aligned address
F32, BF16, F16 = 0, 1, 2
ARG, UNSUPPORTED = -1, -3

X_MSG = "x dtype (a 16-bit stream only in a 16-bit mode; bf16 stream only with bf16 operands)"
S_MSG = "stream dtype (f32, or the operand format of a 16-bit mode)"
RANGE_MSG = "C out of range: above 1024 classes B*C and C*D must stay below 2^31 elements"
ALIGN_MSG = "above 1024 classes Wn and emb must be 16-byte aligned (the tiled kernels load float4)"
KIND_MSG = "head_kind: 0 (CosFace) or 1 (ArcFace)"
ARC_LIN_MSG = "ArcFace is a cosine head (linear_head = 0)"
D_MSG = "D <= 1024, D%4==0"

# name -> (argument names in ABI order, a valid call)
HEAD_FWD = dict(x=P, x_dtype=F32, T=5, gamma=P, beta=P, eps=1e-5, Wn=P, label=P, emb=P, mean=P, rstd=P, logits=P, B=3, D=64, C=100, cos_s=64.0,
                cos_m=0.35, head_bias=None, linear_head=0, pool_mean=0)
HEAD_BWD = dict(dlogits=P, demb=None, x=P, x_dtype=F32, T=5, gamma=P, mean=P, rstd=P, emb=P, Wn=P, dx=P, dxb=None, B=3, D=64, C=100, cos_s=64.0,
                dtype=F32, stream_dtype=F32, p_drop=0.0, seed=0, site=0, linear_head=0, pool_mean=0, compact=0, gscale=None, amax_ws=None,
                target_exp=0)
CALLS = {
    "gsl_head_fwd": dict(HEAD_FWD, stream=None),
    "gsl_head_fwd_margin": dict(HEAD_FWD, head_kind=0, m=0.5, easy_margin=0, cos_y=P, stream=None),
    "gsl_head_bwd": dict(HEAD_BWD, stream=None),
    "gsl_head_bwd_margin": dict(HEAD_BWD, head_kind=0, m=0.5, easy_margin=0, cos_y=P, label=P, stream=None),
    "gsl_head_wgrad": dict(dlogits=P, emb=P, W=P, label=P, cos_y=P, dW=P, dbias=None, B=4, C=100, D=64, head_kind=0, cos_s=64.0, m=0.5,
                           easy_margin=0, stream=None),
    "gsl_layernorm_fwd": dict(x=P, x_row_stride=128, gamma=P, beta=P, eps=1e-5, y=P, mean=P, rstd=P, M=5, D=128, dtype=F32, x_dtype=F32,
                              stream=None),
    "gsl_layernorm_bwd": dict(dy=P, x=P, x_row_stride=128, gamma=P, mean=P, rstd=P, dres=None, dx=P, io_row_stride=0, dxb=None, M=5, D=128,
                              dtype=F32, stream_dtype=F32, x_dtype=F32, p_drop=0.0, seed=0, site=0, drop_row_stride=0, dres_cls_T=0, gmax=None,
                              stream=None),
    "gsl_layernorm_fwd_lora": dict(x=P, x_row_stride=512, gamma=P, beta=P, eps=1e-5, y=P, mean=P, rstd=P, M=5, D=512, P=P, ldp=512, alpha=1.0,
                                   u=P, stream=None),
    "gsl_lora_grad": dict(Y=P, ldy=256, U=P, ldu=16, G=P, gsn=8, gsj=1, M=100, N=256, r=8, dtype=BF16, accumulate=0, ws=P, gscale=None,
                          stream=None),
}

def head_common(**ws):      # checks the forward and the backward entry points share (ws: the workspace the backward needs above 1024 classes)
    return [(dict(D=0), D_MSG), (dict(D=1028), D_MSG), (dict(D=66), D_MSG),
            (dict(C=2000, B=1100000, **ws), RANGE_MSG), (dict(C=2097152, D=1024, B=1, **ws), RANGE_MSG),
            (dict(C=2000, Wn=24, **ws), ALIGN_MSG), (dict(C=2000, emb=24, **ws), ALIGN_MSG)]


FWD = [(dict(x_dtype=3), "x dtype")] + [(dict([(k, None)]), "null/size") for k in ("x", "gamma", "beta", "emb", "mean", "rstd")] + [
    (dict(B=0), "null/size"), (dict(T=0), "null/size"), (dict(Wn=None), "Wn required for logits"), (dict(C=0), "Wn required for logits")]
FWD_MARGIN = [(dict(head_kind=2), KIND_MSG), (dict(head_kind=-1), KIND_MSG), (dict(head_kind=1, linear_head=1), ARC_LIN_MSG),
              (dict(head_kind=1, label=None), "ArcFace logits need label and cos_y [B]"),
              (dict(head_kind=1, cos_y=None), "ArcFace logits need label and cos_y [B]")]
BWD = [(dict([(k, None)]), "null/size") for k in ("x", "gamma", "mean", "rstd", "emb", "dx")] + [
    (dict(B=0), "null/size"), (dict(T=0), "null/size"),
    (dict(C=2000), "C > 1024 needs the workspace amax_ws [B*(D+1)] (d e-hat of the class-tiled backward), also without gscale"),
    (dict(Wn=None), "Wn required with dlogits"), (dict(compact=1, pool_mean=1), "compact cls-row gradients need pool = 'cls'"),
    (dict(gscale=P), "gscale (loss-scaled gradients) needs amax_ws [B]"),
    (dict(target_exp=3), "target_exp: 0 (default 11) or 4 .. 15"), (dict(target_exp=16), "target_exp: 0 (default 11) or 4 .. 15"),
    (dict(target_exp=-1), "target_exp: 0 (default 11) or 4 .. 15"),
    (dict(stream_dtype=BF16), S_MSG), (dict(dtype=BF16, stream_dtype=F16), S_MSG), (dict(dtype=F16, stream_dtype=BF16), S_MSG),
    (dict(stream_dtype=3), S_MSG),
    (dict(x_dtype=BF16), X_MSG), (dict(x_dtype=F16), X_MSG), (dict(dtype=F16, x_dtype=BF16), X_MSG), (dict(dtype=BF16, x_dtype=3), X_MSG)]
BWD_MARGIN = [(dict(head_kind=2), KIND_MSG), (dict(head_kind=-1), KIND_MSG), (dict(head_kind=1, linear_head=1), ARC_LIN_MSG),
              (dict(head_kind=1, label=None), "ArcFace dlogits need label and cos_y [B]"),
              (dict(head_kind=1, cos_y=None), "ArcFace dlogits need label and cos_y [B]")]
LN_DTYPES = [(dict(dtype=3), "dtype"), (dict(dtype=-1), "dtype"),
             (dict(x_dtype=BF16), X_MSG), (dict(x_dtype=F16), X_MSG), (dict(dtype=F16, x_dtype=BF16), X_MSG), (dict(dtype=BF16, x_dtype=3), X_MSG)]
LN_STRIDES = [(dict(x_row_stride=130), "row stride alignment"), (dict(x_row_stride=124), "x_row_stride below the row length D")]

REFUSALS = {      # name -> [(the one change, the text of the failed check)]
    "gsl_head_fwd": FWD + head_common(),
    "gsl_head_fwd_margin": FWD + head_common() + FWD_MARGIN,
    "gsl_head_bwd": BWD + head_common(amax_ws=P),
    "gsl_head_bwd_margin": BWD + head_common(amax_ws=P) + BWD_MARGIN,
    "gsl_head_wgrad": [(dict(head_kind=3), "head_kind: 0 (CosFace), 1 (ArcFace) or 2 (linear)"),
                       (dict(head_kind=-1), "head_kind: 0 (CosFace), 1 (ArcFace) or 2 (linear)")] +
                      [(ch, "null/size") for ch in (dict(dlogits=None), dict(emb=None), dict(dW=None), dict(B=0), dict(C=0))] +
                      [(dict(W=None), "the cosine heads read W"), (dict(D=0), "D <= 1024"), (dict(D=1025), "D <= 1024"),
                       (dict(head_kind=1, label=None), "ArcFace needs label and cos_y [B]"),
                       (dict(head_kind=1, cos_y=None), "ArcFace needs label and cos_y [B]"),
                       (dict(dbias=P), "dbias belongs to the linear head"), (dict(head_kind=1, dbias=P), "dbias belongs to the linear head")],
    "gsl_layernorm_fwd": [(dict([(k, None)]), "null/size") for k in ("x", "gamma", "beta", "mean", "rstd")] + [(dict(M=0), "null/size")] +
                         LN_DTYPES + LN_STRIDES,
    "gsl_layernorm_bwd": [(dict([(k, None)]), "null/size") for k in ("dy", "x", "gamma", "mean", "rstd", "dx")] + [(dict(M=0), "null/size")] +
                         LN_DTYPES + [(dict(stream_dtype=BF16), S_MSG), (dict(dtype=BF16, stream_dtype=F16), S_MSG),
                                      (dict(dtype=F16, stream_dtype=BF16), S_MSG), (dict(stream_dtype=3), S_MSG)] + LN_STRIDES +
                         [(dict(io_row_stride=64), "io_row_stride between 0 and the row length D (rows of dx would overlap)"),
                          (dict(dres_cls_T=-1), "dres_cls_T: compact dres, out of place"),
                          (dict(dres_cls_T=5), "dres_cls_T: compact dres, out of place"),
                          (dict(dres_cls_T=5, dres=P), "dres_cls_T: compact dres, out of place"),
                          (dict(io_row_stride=130), "io row stride alignment")],
    "gsl_layernorm_fwd_lora": [(dict([(k, None)]), "null/size") for k in ("x", "gamma", "beta", "y", "mean", "rstd", "P", "u")] +
                              [(dict(M=0), "null/size"), (dict(D=256, x_row_stride=256, ldp=256), "width (512 or 768)"),
                               (dict(D=1024, x_row_stride=1024, ldp=1024), "width (512 or 768)"),
                               (dict(x_row_stride=516), "row stride alignment"), (dict(ldp=516), "row stride alignment"),
                               (dict(ldp=504), "row stride alignment"), (dict(x_row_stride=504), "x_row_stride below the row length D")],
    "gsl_lora_grad": [(dict([(k, None)]), "null/size") for k in ("Y", "U", "G", "ws")] +
                     [(dict(M=0), "null/size"), (dict(N=0), "null/size"), (dict(ldy=248), "null/size")] +
                     [(ch, "r in [1,64], ldu >= max(16, r) (zero-padded), ldu % 8 == 0")
                      for ch in (dict(r=0), dict(r=65, ldu=72), dict(ldu=8), dict(r=32, ldu=24), dict(ldu=20))] +
                     [(dict(dtype=3), "dtype"), (dict(dtype=-1), "dtype"),
                      (dict(N=260, ldy=260), "N must be a multiple of the vector width"),
                      (dict(dtype=F32, N=258, ldy=258), "N must be a multiple of the vector width")],
}
WIDTHS = {"gsl_layernorm_fwd": dict(D=500, x_row_stride=500), "gsl_layernorm_bwd": dict(D=500, x_row_stride=500)}
BAD_DTYPE = ("gsl_head_bwd", "gsl_head_bwd_margin")      # the operand dtype is the last thing the head backward looks at


@pytest.fixture(scope="module")
def L():
    from gslora_hip import _lib
    return _lib.load()


def call(L, name, change):
    args = dict(CALLS[name])
    assert set(change) <= set(args), (name, change)
    args.update(change)
    rc = getattr(L, name)(*args.values())
    return rc, L.gsl_last_error().decode()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_every_argument_check_refuses_with_its_own_text(L, name):
    from gslora_hip import _lib
    assert len(CALLS[name]) == len(_lib.SIGNATURES[name])
    for change, msg in REFUSALS[name]:
        assert call(L, name, change) == (ARG, f"{name}: argument check failed: {msg} (0,0)"), change


@pytest.mark.parametrize("name", sorted(WIDTHS))
def test_layernorm_refuses_a_width_outside_its_list(L, name):
    assert call(L, name, WIDTHS[name]) == (UNSUPPORTED, f"{name}: unsupported LayerNorm width 500")
    assert call(L, name, dict(D=96, x_row_stride=96)) == (UNSUPPORTED, f"{name}: unsupported LayerNorm width 96")


@pytest.mark.parametrize("name", BAD_DTYPE)
def test_head_backward_refuses_an_unknown_operand_dtype(L, name):
    assert call(L, name, dict(dtype=3)) == (ARG, f"{name}: bad dtype 3")
    assert call(L, name, dict(dtype=-1)) == (ARG, f"{name}: bad dtype -1")


# ------------------------------------------------------------------ workspace sizes
GRID_M = (1, 64, 127, 128, 129, 1000, 24576, 201728)
GRID_N = (8, 64, 256, 260, 512, 768, 2048, 3072)
GRID_R = (1, 8, 9, 16, 17, 32, 33, 64)
ANCHORS = {(201728, 512, 8): 3244032, (201728, 2048, 16): 25952256, (96, 768, 32): 98304, (1, 8, 64): 1024, (130, 260, 5): 6240}
# descriptor lists (M, N, r) of gsl_lora_grad_batch_ws_elems: the few-shot backward of a 6-block ViT (24 entries), mixed ranks, one entry,
# more than one launch (LGB_MAX = 24 per launch), a single row
BATCHES = (
    [(788, 512, 8), (788, 2048, 8), (788, 512, 8), (788, 512, 8)] * 6,
    [(788, 768, 16), (788, 3072, 48), (197, 256, 64), (4, 512, 33)],
    [(201728, 512, 8)],
    [(1576, 512, 8), (1576, 2048, 32)] * 13,
    [(1, 256, 1)],
)


class LgradDesc(ctypes.Structure):      # struct gsl_lgrad_desc (include/gslora_hip.h)
    _fields_ = [("Y", ctypes.c_void_p), ("ldy", ctypes.c_long), ("U", ctypes.c_void_p), ("ldu", ctypes.c_int), ("M", ctypes.c_int),
                ("N", ctypes.c_int), ("r", ctypes.c_int), ("accumulate", ctypes.c_int), ("pad_", ctypes.c_int), ("G", ctypes.c_void_p),
                ("gsn", ctypes.c_long), ("gsj", ctypes.c_long)]


def ws_grid(L):
    return np.array([[[L.gsl_lora_grad_ws_elems(M, N, r) for r in GRID_R] for N in GRID_N] for M in GRID_M], dtype=np.int64)


def ws_batches(L):
    out = []
    for batch in BATCHES:
        descs = (LgradDesc * len(batch))(*[LgradDesc(P, N, P, 64, M, N, r, 0, 0, P, r, 1) for M, N, r in batch])
        out.append(L.gsl_lora_grad_batch_ws_elems(ctypes.cast(descs, ctypes.c_void_p), len(batch)))
    return np.array(out, dtype=np.int64)


def test_lora_grad_workspace_sizes_are_the_parents(L, golden_dir):
    g = np.load(os.path.join(golden_dir, "lora_grad_ws_parent.npz"), allow_pickle=False)
    assert (tuple(g["M"]), tuple(g["N"]), tuple(g["r"])) == (GRID_M, GRID_N, GRID_R)
    got = ws_grid(L)
    assert got.shape == (8, 8, 8) and (got > 0).all()
    assert np.array_equal(got, g["elems"]), np.argwhere(got != g["elems"])
    for (M, N, r), want in ANCHORS.items():      # computed from the sources by hand: the fixture itself can be checked
        assert L.gsl_lora_grad_ws_elems(M, N, r) == want, (M, N, r)
        if M in GRID_M and N in GRID_N and r in GRID_R:
            assert g["elems"][GRID_M.index(M), GRID_N.index(N), GRID_R.index(r)] == want


def test_lora_grad_batch_workspace_sizes_are_the_parents(L, golden_dir):
    g = np.load(os.path.join(golden_dir, "lora_grad_ws_parent.npz"), allow_pickle=False)
    got = ws_batches(L)
    assert (got > 0).all() and np.array_equal(got, g["batch_elems"]), (got, g["batch_elems"])


if __name__ == "__main__":      # record the table from the library of this tree (run at the commit whose values are the reference)
    for p in (ROOT, os.path.join(ROOT, "gs-lora_amd")):
        sys.path.insert(0, p)
    from gslora_hip import _lib
    lib = _lib.load()
    np.savez(sys.argv[1], M=np.array(GRID_M), N=np.array(GRID_N), r=np.array(GRID_R), elems=ws_grid(lib), batch_elems=ws_batches(lib))
