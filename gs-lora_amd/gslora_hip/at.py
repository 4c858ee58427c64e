"""The attention-transfer term of the LIRF baseline on the HIP path (libgslora_at.so, opened on first use through gslora_hip._lib_at):
at_loss of the student's and the teacher's [B, T, D] mid stream (reference baselines/LIRFtrain.py, at / at_loss), the table that carries
its gradient, and the in-place addition of that gradient to the stream gradient at the boundary between the two half networks.
"""
import torch


def _shape(xs, B, T, xt):
    """The [rows, D] views of the two streams, checked against B images of T tokens."""
    from . import _lib_at as LA
    xs = LA._rows(xs, "the student's stream")
    xt = LA._rows(xt, "the teacher's stream")
    B, T = int(B), int(T)
    D = xs.shape[1]
    if B < 1 or T < 1 or xs.shape[0] < B * T:
        raise ValueError(f"at: {B} images of {T} tokens are not a leading range of the student's {xs.shape[0]} rows")
    if tuple(xt.shape) != (B * T, D):
        raise ValueError(f"at: the teacher's stream {tuple(xt.shape)} does not match {B} images of {T} tokens and {D} channels")
    if xt.dtype != xs.dtype or xt.device != xs.device:
        raise ValueError(f"at: the student's stream is {xs.dtype} on {xs.device}, the teacher's {xt.dtype} on {xt.device}")
    if D % 64 or D > LA.MAX_D or T > LA.MAX_T:
        raise ValueError(f"at: D = {D} must be a multiple of 64 up to {LA.MAX_D} and T = {T} at most {LA.MAX_T}")
    return xs, xt, B, T, D


def _forward(xs, B, T, xt, tables):
    from . import _lib_at as LA
    xs, xt, B, T, D = _shape(xs, B, T, xt)
    dev = xs.device
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    G = torch.empty(B, D, device=dev, dtype=torch.float32)
    ws = torch.empty(LA.at_ws_elems(B, T, D), device=dev, dtype=torch.float32)
    a_s = torch.empty(B, D, device=dev, dtype=torch.float32) if tables else None
    a_t = torch.empty(B, D, device=dev, dtype=torch.float32) if tables else None
    LA.at_fwd(xs.detach(), xt.detach(), B, T, loss, G, ws, a_s, a_t)
    return loss[0], G, a_s, a_t


def at_loss_value_and_table(xs, B, T, xt):
    """-> (loss, G): at_loss of images 0 .. B-1 of the student's stream `xs` ([rows, D] or [Btot, T, D] with at least B * T rows: the forget
    rows of a fused forward) against the teacher's `xt` ([B * T, D] or [B, T, D]), a 0-dim f32 device tensor, and the [B, D] f32 table
    G[b, d] = d loss / d xs[b, t, d] / xs[b, t, d] that at_inject spends. Both streams in one of f32 / f16 / bf16. No autograd node: the
    runner adds the gradient at the boundary itself. Three launches, no host sync."""
    loss, G, _, _ = _forward(xs, B, T, xt, False)
    return loss, G


def at_inject(dmid, xs, G, coef, scale, T=None):
    """dmid[b, t, d] += coef * scale * G[b, d] * xs[b, t, d] over the B = G.shape[0] images the table covers, in place. dmid: the stream
    gradient at the boundary ([rows, D] or [Btot, T, D], f32 or a 16-bit type), rows behind image B-1 untouched; xs: the student's stream
    as given to at_loss_value_and_table; coef: a 1-element f32 device tensor (the upstream gradient times the term's weight); scale: a
    1-element f32 device tensor, the loss scale of the pass (None: 1); T: the tokens per image, needed only when both tensors are [rows, D].
    One launch."""
    from . import _lib_at as LA
    if not (torch.is_tensor(G) and G.dim() == 2):
        raise RuntimeError("gslora_hip.at: G must be the [B, D] f32 table of at_loss_value_and_table (the HIP path has no CPU fallback)")
    if T is None:
        if not (torch.is_tensor(xs) and torch.is_tensor(dmid)) or (xs.dim() != 3 and dmid.dim() != 3):
            raise ValueError("at_inject: the token count is read from a [B, T, D] tensor; give xs or dmid with three dimensions, or T")
        T = xs.shape[1] if xs.dim() == 3 else dmid.shape[1]
    T = int(T)
    x2 = LA._rows(xs, "the student's stream")
    d2 = LA._rows(dmid, "the stream gradient")
    B, D = G.shape
    LA._f32(G, "G", B * D)
    if x2.shape[1] != D or d2.shape[1] != D or x2.shape[0] < B * T or d2.shape[0] < B * T:
        raise ValueError(f"at_inject: the stream {tuple(x2.shape)} and its gradient {tuple(d2.shape)} do not hold {B} images of {T} tokens and "
                         f"{D} channels")
    if scale is None:
        scale = torch.ones(1, device=x2.device, dtype=torch.float32)
    LA.at_bwd(x2.detach(), G, LA._f32(coef, "coef", 1), LA._f32(scale, "scale", 1), B, T, d2)
    return dmid


def at(x):
    """The reference's at(x) for a [B, T, D] stream: F.normalize(x.pow(2).mean(1)) with entries below 0.005 set to 0, [B, D] f32. The
    forward value only: NOT differentiable (training takes the gradient through gslora_hip.step.lirf_step). The kernels work on a pair of
    streams, so the stream is read twice."""
    if not torch.is_tensor(x) or x.dim() != 3:
        raise RuntimeError("gslora_hip.at: at(x) takes a [B, T, D] stream on a ROCm GPU (the HIP path has no CPU fallback)")
    return _forward(x, x.shape[0], x.shape[1], x, True)[2]


def at_loss(x, y):
    """The reference's at_loss(x, y) = (at(x) - at(y)).pow(2).mean() for two [B, T, D] streams, a 0-dim f32 device tensor. The forward value
    only: NOT differentiable."""
    if not torch.is_tensor(x) or x.dim() != 3 or not torch.is_tensor(y):
        raise RuntimeError("gslora_hip.at: at_loss(x, y) takes two [B, T, D] streams on a ROCm GPU (the HIP path has no CPU fallback)")
    return _forward(x, x.shape[0], x.shape[1], y, False)[0]
