"""The regularisation baselines (L2 / EWC / MAS) on the HIP path: the importance matrices of the reference's
train/train_own_forget_cl.py:1425-1432 (L2), :1444-1512 (EWC) and :1524-1561 (MAS), MAS's objective as an autograd node, and the quadratic
regulariser of engine_cl.get_reg_loss over every term and tensor in two launches forward and one backward (libgslora_reg.so, opened on
first use through gslora_hip._lib_reg). Scope is that of gslora_hip.step.ffn_reg_step: a ViT_face / ViTs_face built with lora_rank = 0 whose
FFN linears (and, optionally, the `loss` head) require a gradient; one process, eager.
"""
import torch

from ._cdll import DeviceTable
from .step import _ce_mean_and_hits, _model_input, _overflow_guard_of, _unwrap

KINDS = ("l2", "ewc", "mas")


class _SqMean(torch.autograd.Function):
    """mean(x ** 2) of [B, C] f32 logits over gsr_sq_mean_fwd / gsr_sq_mean_bwd."""

    @staticmethod
    def forward(ctx, x):
        from . import _lib_reg as LR
        out = torch.empty((), device=x.device, dtype=torch.float32)
        LR.sq_mean_fwd(x, out)
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, gout):
        from . import _lib_reg as LR
        x, = ctx.saved_tensors
        dx = torch.empty(x.shape, device=x.device, dtype=torch.float32)
        LR.sq_mean_bwd(x, gout.detach().float().reshape(1).contiguous(), dx)
        return dx


def sq_mean(logits):
    """The objective MAS differentiates (train_own_forget_cl.py:1548-1549: outputs.pow_(2); loss = outputs.mean()) as one autograd node.
    logits: [B, C] f32 on the GPU with unit column stride. The gradient has the bits of torch autograd for x.pow(2).mean()."""
    if logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_cuda or (logits.shape[1] > 1 and logits.stride(1) != 1):
        raise RuntimeError("gslora_hip.reg.sq_mean: logits must be a [B, C] f32 tensor on a ROCm GPU with unit column stride "
                           "(the HIP path has no CPU fallback)")
    return _SqMean.apply(logits)


class Importance(dict):
    """{name: f32 tensor} as calculate_importance returns it, plus `skipped`: how many importance batches were left out because their fp16
    backward saturated (always 0 in the f32 and bf16 modes and for kind "l2")."""
    skipped = 0


def calculate_importance(model, dataloader, kind, criterion=None, prior=None, device=None):
    """The importance matrix of a regularisation baseline over the parameters that require a gradient: an Importance (a dict {name: f32
    tensor}; its attribute `skipped` counts the batches left out, read with the function's single host sync at the end).

      kind "l2"   ones (train_own_forget_cl.py:1425-1432); the loader is not read
      kind "ewc"  sum over the loader's batches of grad(criterion(logits, y)) ** 2 * len(batch) / len(loader)          (:1444-1512)
      kind "mas"  sum over the loader's batches of |grad(mean(logits ** 2))| / len(loader)                              (:1524-1561)

    The reference's loops: model.eval() (dropout off), logits, _ = model(x, y), the loss (plain cross-entropy: the mean through
    losses.ce_sum_top1; any other criterion as it is; MAS: sq_mean), model.zero_grad(), backward, one gsr_importance_acc launch per tensor
    that has a gradient, model.train() at the end. In fp16 mode the runner's overflow guard goes to the kernel: a batch whose 16-bit gradient
    stores saturated is not accumulated (no host sync in the loop). prior ({name: tensor}, the reference's --online, :1448-1449): accumulation
    starts from these tensors IN PLACE and they are what is returned; without it, from zeros. n_fisher_sample is the caller's business: a
    different loader over the same arithmetic."""
    if kind not in KINDS:
        raise ValueError(f"calculate_importance: kind {kind!r}; use one of {KINDS}")
    net = _unwrap(model)
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    if kind == "l2":
        return Importance((n, p.clone().detach().fill_(1)) for n, p in named)
    from . import _lib_reg as LR
    if kind == "ewc" and criterion is None:
        raise ValueError("calculate_importance: kind 'ewc' differentiates criterion(logits, labels); pass the training criterion")
    device = torch.device(device) if device is not None else (named[0][1].device if named else torch.device("cuda"))
    if prior is not None:
        missing = [n for n, _ in named if n not in prior]
        if missing:
            raise ValueError(f"calculate_importance: prior has no entry for {missing[:3]}")
        importance = Importance((n, prior[n]) for n, _ in named)
    else:
        importance = Importance((n, torch.zeros(p.shape, device=p.device, dtype=torch.float32)) for n, p in named)
    for (n, p), om in zip(named, importance.values()):
        if om.shape != p.shape:
            raise ValueError(f"calculate_importance: the importance of {n!r} does not have the parameter's shape")
        LR._flat_f32(om, f"the importance of {n!r}")
    n_batches = len(dataloader)
    skipped = torch.zeros(1, device=device, dtype=torch.int32)
    code = LR.EWC if kind == "ewc" else LR.MAS
    model.eval()
    try:
        for samples, targets in dataloader:
            samples, targets = samples.to(device), targets.to(device)
            logits, _ = model(_model_input(net, samples), targets)
            loss = sq_mean(logits) if kind == "mas" else _ce_mean_and_hits(criterion, logits, targets, samples.size(0), hits=False)[0]
            model.zero_grad()
            loss.backward()
            guard = _overflow_guard_of(net)
            count = skipped      # a skipped batch counts once: the first launch of the batch carries the counter
            for (n, p), om in zip(named, importance.values()):
                if p.grad is not None:      # (some parameters may not have a gradient, :1502-1504: their importance stays as it is)
                    LR.importance_acc(om, p.grad, code, samples.size(0), n_batches, guard, count)
                    count = None
    finally:
        model.train()
    importance.skipped = int(skipped.item())      # the single host sync
    return importance


def _term_entries(model, regularization_terms):
    """The walk of get_reg_loss (reference engine_cl.py:449-459), term-major: (p, task_param, importance or None) per term and trainable
    tensor, the terms' tensors as contiguous f32 on the parameter's device. Raises what get_reg_loss on the HIP path refuses."""
    named = [(n, p) for n, p in _unwrap(model).named_parameters() if p.requires_grad]
    for term in regularization_terms.values():
        imp, ref = term["importance"], term["task_param"]
        for n, p in named:
            om, p0 = imp[n], ref[n]
            if p.dtype != torch.float32 or not p.is_contiguous() or not p.is_cuda:
                raise RuntimeError(f"gs-lora_amd get_reg_loss: parameter {n!r} must be a contiguous f32 tensor on the GPU (no CPU fallback)")
            if p0.shape != p.shape or (om is not None and om.shape != p.shape):
                raise ValueError(f"get_reg_loss: importance / task_param of {n!r} do not have the parameter's shape")
            yield (p, p0.detach().to(device=p.device, dtype=torch.float32).contiguous(),
                   None if om is None else om.detach().to(device=p.device, dtype=torch.float32).contiguous())


class _RegQuad(torch.autograd.Function):
    """reg_lambda * sum over terms and tensors of sum(importance * (p - task_param) ** 2) (reference engine_cl.py:449-459) as ONE autograd
    node over gst_reg_quad_fwd / gst_reg_quad_bwd. entries: what _term_entries yields."""

    @staticmethod
    def forward(ctx, entries, reg_lambda, *params):
        from . import _lib_train as LT
        dev = params[0].device
        out = torch.zeros((), device=dev, dtype=torch.float32)
        ws = torch.empty(max(LT.load().gst_reg_quad_ws_elems(p.numel()) for p in params), device=dev, dtype=torch.float32)
        for k, (p, p0, om) in enumerate(entries):
            LT.reg_quad_fwd(p.detach(), p0, om, out, accumulate=k > 0, ws=ws)
        ctx.entries, ctx.reg_lambda, ctx.ids = entries, float(reg_lambda), [id(p) for p in params]
        return out * float(reg_lambda)

    @staticmethod
    def backward(ctx, gout):
        from . import _lib_train as LT
        coef = (gout.detach().float() * ctx.reg_lambda).reshape(1).contiguous()      # a device float: upstream gradient times lambda
        grads = {}
        for p, p0, om in ctx.entries:
            g = grads.get(id(p))
            if g is None:
                g = grads[id(p)] = torch.zeros(p.shape, device=p.device, dtype=torch.float32)
            LT.reg_quad_bwd(p.detach(), p0, om, coef, g)
        return (None, None) + tuple(grads.get(i) if need else None for i, need in zip(ctx.ids, ctx.needs_input_grad[2:]))


def reg_loss(model, regularization_terms, reg_lambda, device):
    """engine_cl.get_reg_loss (reference engine_cl.py:435-460): reg_lambda * sum_terms sum_{trainable p} sum(importance[n] * (p -
    task_param[n]) ** 2), a 0-dim f32 tensor; a 0-dim zero when the terms are None. importance[n] may be None for the identity (L2).
    Two launches forward and one backward per term and tensor (libgslora_train.so); RegTerms is the batched form."""
    zero = torch.tensor(0.0, device=device)
    if regularization_terms is None:
        return zero
    entries = list(_term_entries(model, regularization_terms))
    if not entries:
        return zero
    return _RegQuad.apply(entries, reg_lambda, *[p for p in _unwrap(model).parameters() if p.requires_grad])


class _RegMulti(torch.autograd.Function):
    """reg_lambda * sum over terms and tensors of sum(importance * (p - task_param) ** 2) as ONE autograd node over gsr_reg_multi_fwd /
    gsr_reg_multi_bwd: the value and the gradients of _RegQuad, bit for bit."""

    @staticmethod
    def forward(ctx, rt, *params):
        from . import _lib_reg as LR
        out = torch.empty((), device=rt.table_dev.device, dtype=torch.float32)
        LR.reg_multi_fwd(rt.table_dev, rt.n_terms * rt.n_tensors, rt.total_blocks, out, rt.ws)
        ctx.rt = rt
        return out * rt.reg_lambda

    @staticmethod
    def backward(ctx, gout):
        from . import _lib_reg as LR
        rt = ctx.rt
        coef = (gout.detach().float() * rt.reg_lambda).reshape(1).contiguous()      # a device float: upstream gradient times lambda
        g = torch.zeros(rt.g_elems, device=rt.table_dev.device, dtype=torch.float32)
        LR.reg_multi_bwd(rt.table_dev, rt.n_terms, rt.n_tensors, rt.bwd_blocks, coef, g)
        return (None,) + rt.grad_views(g, rt.params, ctx.needs_input_grad[1:])


class RegTerms(DeviceTable):
    """The regularisation terms of a run, prepared once for the batched kernels: `.loss()` has the meaning of
    engine_cl.get_reg_loss(model, regularization_terms, reg_lambda, device) and its bits, in two launches forward and one backward whatever
    the number of terms and tensors. The entry table (gsr_reg_multi_layout) is built and uploaded at construction: the parameters' device
    addresses are stable, FusedAdamW writes through raw pointers. Every `.loss()` compares the parameters' data_ptr() with the table's and
    rebuilds it when one moved. The terms' own tensors (task_param, importance) are converted once and held here: terms added or changed
    afterwards need a new RegTerms. The walk over the terms and its refusals are reg_loss's own (_term_entries)."""

    def __init__(self, model, regularization_terms, reg_lambda):
        self.model, self.terms, self.reg_lambda = model, regularization_terms, float(reg_lambda)
        self.rebuilds = 0
        self._build()

    def _build(self):
        from . import _lib_reg as LR
        self.params = [p for p in _unwrap(self.model).parameters() if p.requires_grad]
        self.n_terms = 0 if self.terms is None else len(self.terms)
        self.n_tensors = len(self.params)
        self.table_dev = None
        if not self.n_terms or not self.n_tensors:
            return
        self._keep = list(_term_entries(self.model, self.terms))      # (holds the converted tensors the table points at)
        entries = [(p.data_ptr(), p0.data_ptr(), None if om is None else om.data_ptr(), p.numel()) for p, p0, om in self._keep]
        table, self.total_blocks, self.bwd_blocks, self.g_elems = LR.reg_multi_layout(entries, self.n_terms, self.n_tensors)
        self.goffs = [table[t].goff for t in range(self.n_tensors)]
        self._upload(table, self.total_blocks, self.params, self.params[0].device)

    def loss(self, device=None):
        """reg_lambda * sum_terms sum_{trainable p} sum(importance[n] * (p - task_param[n]) ** 2): a 0-dim f32 tensor with a gradient; a 0-dim
        zero when there are no terms or no trainable parameters."""
        if self.table_dev is None:
            return torch.tensor(0.0, device=device if device is not None else (self.params[0].device if self.params else "cuda"))
        if self._moved(self.params):
            self.rebuilds += 1
            self._build()
        return _RegMulti.apply(self, *self.params)
