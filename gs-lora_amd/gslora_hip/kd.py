"""The loss side of the SCRUB baseline on the HIP path (libgslora_kd.so, opened on first use through gslora_hip._lib_kd): the
temperature-softened KL between student and teacher logits fused with the student's mean cross-entropy (reference util/sgda_utils.py,
DistillKL; baselines/SCRUBtrain.py, the two loss lines) as one autograd node, and param_dist (util/sgda_utils.py) over every parameter of a
model as another. Scope is that of gslora_hip.step.scrub_step: one process, eager.
"""
import weakref

import torch
import torch.nn as nn

from ._cdll import DeviceTable


class _KdCe(torch.autograd.Function):
    """(kd, ce, c_kd * kd + c_ce * ce) of [B, C] f32 logits over gsk_kd_ce_fwd / gsk_kd_ce_bwd. Only the third output carries a gradient, and
    only the student's logits receive one."""

    @staticmethod
    def forward(ctx, ys, yt, labels, T, c_kd, c_ce):
        from . import _lib_kd as LK
        B, C = ys.shape
        out3 = torch.empty(3, device=ys.device, dtype=torch.float32)
        ws = torch.empty(LK.kd_ws_elems(B, C), device=ys.device, dtype=torch.float32)
        LK.kd_ce_fwd(ys, yt, labels, T, c_kd, c_ce, out3, ws)
        ctx.save_for_backward(ys, yt, ws, *(() if labels is None else (labels,)))
        ctx.hyper = (float(T), float(c_kd), float(c_ce))
        kd, ce, part = out3[0], out3[1], out3[2]
        ctx.mark_non_differentiable(kd, ce)
        return kd, ce, part

    @staticmethod
    def backward(ctx, _gkd, _gce, gpart):
        from . import _lib_kd as LK
        ys, yt, ws, *rest = ctx.saved_tensors
        T, c_kd, c_ce = ctx.hyper
        d = torch.empty(ys.shape, device=ys.device, dtype=torch.float32)
        LK.kd_ce_bwd(ys, yt, rest[0] if rest else None, ws, gpart.detach().float().reshape(1).contiguous(), T, c_kd, c_ce, d)
        return d, None, None, None, None, None


def kd_ce(ys, yt, labels, T, c_kd, c_ce):
    """-> (kd, ce, part), three 0-dim f32 device tensors:

      kd    F.kl_div(F.log_softmax(ys / T, 1), F.softmax(yt / T, 1), reduction="sum") * T ** 2 / B        (DistillKL.forward)
      ce    mean cross-entropy of ys against labels; 0 when c_ce == 0 (then it is not computed and labels may be None)
      part  c_kd * kd + c_ce * ce, formed on the device — the one output with a gradient (kd and ce are marked non-differentiable)

    ys, yt: [B, C] f32 on the GPU with unit column stride. The teacher's logits never receive a gradient. Two launches forward, one
    backward."""
    from . import _lib_kd as LK
    LK._logits(ys, "the student's logits")
    LK._logits(yt, "the teacher's logits")
    if ys.shape != yt.shape:
        raise ValueError(f"kd_ce: student logits {tuple(ys.shape)} and teacher logits {tuple(yt.shape)} differ in shape")
    if not float(T) > 0.0:
        raise ValueError(f"kd_ce: the temperature must be positive, got {T}")
    if labels is None:
        if float(c_ce) != 0.0:
            raise ValueError("kd_ce: labels are required unless c_ce == 0")
    else:
        if labels.shape != (ys.shape[0],):
            raise ValueError(f"kd_ce: {tuple(labels.shape)} labels for {ys.shape[0]} rows")
        labels = labels.to(device=ys.device, dtype=torch.int64).contiguous()
    return _KdCe.apply(ys, yt.detach(), labels, float(T), float(c_kd), float(c_ce))


class DistillKL(nn.Module):
    """The reference's DistillKL (util/sgda_utils.py): constructor DistillKL(T), forward(y_s, y_t) -> the temperature-softened KL, batch
    mean, times T ** 2. It is kd_ce with c_kd = 1 and c_ce = 0 and returns `part` (1 * kd + 0 * 0: the bits of kd), so a loop written by
    hand against the reference's names runs the same kernels. y_t receives no gradient."""

    def __init__(self, T):
        super().__init__()
        self.T = T

    def forward(self, y_s, y_t):
        return kd_ce(y_s, y_t, None, self.T, 1.0, 0.0)[2]


class _ParamDist(torch.autograd.Function):
    """p * sum_k ||p_k - q_k|| as ONE autograd node over gsk_param_dist_fwd / gsk_param_dist_bwd."""

    @staticmethod
    def forward(ctx, pd, *params):
        from . import _lib_kd as LK
        out = torch.empty((), device=pd.table_dev.device, dtype=torch.float32)
        norms = torch.empty(pd.n_entries, device=out.device, dtype=torch.float32)
        LK.param_dist_fwd(pd.table_dev, pd.n_entries, pd.total_blocks, pd.p, out, norms, pd.ws)
        ctx.pd, ctx.norms = pd, norms
        return out

    @staticmethod
    def backward(ctx, gout):
        from . import _lib_kd as LK
        pd = ctx.pd
        g = torch.zeros(pd.g_elems, device=pd.table_dev.device, dtype=torch.float32)
        LK.param_dist_bwd(pd.table_dev, pd.n_entries, pd.bwd_blocks, pd.p, gout.detach().float().reshape(1).contiguous(), ctx.norms, g)
        return (None,) + pd.grad_views(g, pd.trainable, ctx.needs_input_grad[1:])


class ParamDist(DeviceTable):
    """param_dist(model, swa_model, p) of the reference (util/sgda_utils.py) prepared once for the batched kernels: `.loss()` is
    p * sum over ALL of zip(model.parameters(), swa_model.parameters()) — the frozen ones included, as in the reference — of the Frobenius
    norm of the difference, in two launches forward and one backward whatever the number of tensors. The entry table
    (gsk_param_dist_layout) is built and uploaded at construction; every `.loss()` compares data_ptr() of every tensor of both models with
    the table's and rebuilds it when one moved (the rule of gslora_hip.reg.RegTerms). Gradients go to the model's parameters that require
    one (views of one flat zero-initialised buffer); the averaged copy receives none. The two models are held by weak reference (the
    cache of util.sgda_utils.param_dist is keyed on the model): the caller keeps them alive, as a training loop does.

    With p == 0.0 (the reference's default --sgda_smoothing) `.loss()` launches nothing and returns a 0-dim zero without a gradient:
    0.0 times a finite distance is 0, and the gradient the reference back-propagates through it is 0 for every parameter."""

    def __init__(self, model, swa_model, p):
        self._model, self._swa_model, self.p = weakref.ref(model), weakref.ref(swa_model), float(p)      # (a cache may key on the model)
        self.rebuilds = 0
        if self.p != 0.0:
            self._build()

    def _pairs(self):
        model, swa_model = self._model(), self._swa_model()
        if model is None or swa_model is None:
            raise RuntimeError("gslora_hip.kd.ParamDist: the model or its averaged copy no longer exists")
        ps, qs = list(model.parameters()), list(swa_model.parameters())
        if len(ps) != len(qs):
            raise ValueError(f"param_dist: the model has {len(ps)} parameters, the averaged copy {len(qs)}")
        return ps, qs

    def _build(self):
        from . import _lib_kd as LK
        ps, qs = self._pairs()
        if not ps:
            raise ValueError("param_dist: the model has no parameters")
        entries = []
        for k, (a, b) in enumerate(zip(ps, qs)):
            if a.shape != b.shape:
                raise ValueError(f"param_dist: parameter {k} has shape {tuple(a.shape)}, its averaged copy {tuple(b.shape)}")
            for t in (a, b):
                if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
                    raise RuntimeError(f"gslora_hip.kd.ParamDist: parameter {k} must be a contiguous f32 tensor on the GPU (no CPU fallback)")
            entries.append((a.data_ptr(), b.data_ptr(), a.numel(), a.requires_grad))
        table, self.total_blocks, self.bwd_blocks, self.g_elems = LK.param_dist_layout(entries)
        self.n_entries = len(entries)
        self.trainable = [a for a in ps if a.requires_grad]
        self.goffs = [table[k].goff for k, a in enumerate(ps) if a.requires_grad]
        self._req = [a.requires_grad for a in ps]
        self._upload(table, self.total_blocks, ps + qs, ps[0].device)

    def loss(self):
        if self.p == 0.0:
            dev = next(self._model().parameters()).device
            return torch.zeros((), device=dev, dtype=torch.float32)
        ps, qs = self._pairs()
        if self.table_dev is None or self._moved(ps + qs) or [a.requires_grad for a in ps] != self._req:
            self.rebuilds += self.table_dev is not None
            self._build()
        if not self.trainable:      # nothing trains: the value alone
            return _ParamDist.apply(self).detach()
        return _ParamDist.apply(self, *self.trainable)
