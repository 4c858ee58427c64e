"""The function-distance term of the DER / DER++ and FDR baselines on the HIP path (libgslora_fd.so, opened on first use through
gslora_hip._lib_fd): the distance between a row range of the student's fused output and the frozen teacher's output as one autograd node
(reference baselines/DERtrain.py, DER_regularzaion_loss; baselines/FDRtrain.py, regularization_loss). Scope is that of
gslora_hip.step.distill_step: one process, eager.
"""
import torch

MODES = ("sq", "rownorm")


class _RowDist(torch.autograd.Function):
    """(dist, coef * dist) of rows [row0, row0 + nrows) of `full` against `t` over gsf_rowdist_fwd / gsf_rowdist_bwd. Only the second output
    carries a gradient, and only `full` receives one: a [Btot, W] buffer whose rows outside the range are zero and whose rows inside are
    written once by the kernel."""

    @staticmethod
    def forward(ctx, full, row0, nrows, t, mode, coef):
        from . import _lib_fd as LF
        a = full[row0:row0 + nrows]      # (a view inside the node: autograd records no slice)
        out = torch.empty(1, device=full.device, dtype=torch.float32)
        ws = torch.empty(LF.rowdist_ws_elems(nrows, full.shape[1]), device=full.device, dtype=torch.float32)
        LF.rowdist_fwd(a, t, mode, out, ws)
        ctx.save_for_backward(full, t, ws)
        ctx.hyper = (row0, nrows, mode, coef)
        dist = out[0]
        part = dist * coef
        ctx.mark_non_differentiable(dist)
        return dist, part

    @staticmethod
    def backward(ctx, _gdist, gpart):
        from . import _lib_fd as LF
        full, t, ws = ctx.saved_tensors
        row0, nrows, mode, coef = ctx.hyper
        d = torch.empty(full.shape, device=full.device, dtype=torch.float32)
        if row0 > 0:
            d[:row0].zero_()
        if row0 + nrows < full.shape[0]:
            d[row0 + nrows:].zero_()
        LF.rowdist_bwd(full[row0:row0 + nrows], t, ws, gpart.detach().float().reshape(1).contiguous(), mode, coef, d[row0:row0 + nrows])
        return d, None, None, None, None, None


def row_dist(full, row0, nrows, t, mode, coef):
    """-> (dist, part), two 0-dim f32 device tensors, of rows [row0, row0 + nrows) of `full` ([Btot, W], the student's logits or embedding
    over a fused batch) against `t` ([nrows, W], the teacher's):

      mode "sq"       dist = torch.norm(a - t, p=2) ** 2 as DER_regularzaion_loss forms it (n = sqrt(sum), n * n)
      mode "rownorm"  dist = torch.norm(a - t, 2, 1).mean(), FDR's regularization_loss; a row that equals the teacher's has a zero gradient
      part            coef * dist — the one output with a gradient (dist is marked non-differentiable)

    The gradient for `full` is one [Btot, W] buffer: zero outside the row range, written once inside it; no torch slice or slice-backward
    sits on the path. `t` never receives a gradient. Two launches forward, one backward."""
    from . import _lib_fd as LF
    if mode not in MODES:
        raise ValueError(f"row_dist: mode must be one of {MODES}, got {mode!r}")
    LF._rows(full, "the student's rows")
    LF._rows(t, "the teacher's rows")
    row0, nrows = int(row0), int(nrows)
    if not (0 <= row0 and 1 <= nrows and row0 + nrows <= full.shape[0]):
        raise ValueError(f"row_dist: rows [{row0}, {row0 + nrows}) are not a non-empty range of the {full.shape[0]} rows of the student's tensor")
    if tuple(t.shape) != (nrows, full.shape[1]):
        raise ValueError(f"row_dist: the teacher's tensor {tuple(t.shape)} does not match rows [{row0}, {row0 + nrows}) of the student's "
                         f"{tuple(full.shape)}")
    if t.device != full.device:
        raise ValueError(f"row_dist: the student's rows are on {full.device}, the teacher's on {t.device}")
    return _RowDist.apply(full, row0, nrows, t.detach(), LF.MODES[mode], float(coef))
