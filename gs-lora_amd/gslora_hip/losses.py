"""Loss terms of the GS-LoRA step as autograd nodes over the HIP kernels.

  ce_sum_top1      — nn.CrossEntropyLoss (sum form) + top-1 count     (engine_cl.py:65-78)
  proto_kl_sum     — get_prototype_loss 'kl' (sum form)                (engine_cl.py:571-603)
  proto_l2_sum     — get_prototype_loss 'l2' (sum of the row means)    (engine_cl.py:593-594)
  structure_loss   — group-lasso over LoRA groups                      (engine_cl.py:349-432)
Upstream gradients arrive as 0-dim device tensors and are handed to the kernels as device
pointers, so the whole loss graph runs without a host sync.
"""
import torch

from . import ops


class _RowSum(torch.autograd.Function):
    """Sum over the rows of a per-row loss: fwd(x, labels[, table]) -> the sums (the first is the loss, `nondiff` names the others, such as
    CE's hit count); backward is bwd(x, labels[, table], coef, 1.0) with the upstream gradient as a device scalar."""

    @staticmethod
    def forward(ctx, x, labels, table, fwd, bwd, nondiff):
        x = x.contiguous().float()
        labels = labels.to(device=x.device, dtype=torch.int64).contiguous()
        extra = () if table is None else (table,)
        ctx.save_for_backward(x, labels, *extra)
        ctx.bwd = bwd
        res = tuple(fwd(x, labels, *extra))
        ctx.mark_non_differentiable(*(res[i] for i in nondiff))
        return res

    @staticmethod
    def backward(ctx, g, *_):
        return (ctx.bwd(*ctx.saved_tensors, g.reshape(1).float().contiguous(), 1.0),) + (None,) * 5


class _RowSumSplit(torch.autograd.Function):
    """_RowSum of the remain rows [0, nr) and the forget rows [nr, N) of ONE tensor (the step runs both batches as one forward); `order`
    ("rf" or "fr") is the order of the two ranges in the outputs. Backward writes the two row ranges of a single gradient buffer — slicing
    the tensor in Python instead would make autograd build two zero-filled full-size gradients and add them (10 extra one-off kernels per
    step)."""

    @staticmethod
    def forward(ctx, x, labels, table, nr, fwd, bwd, nondiff, order):
        x = x.contiguous().float()
        labels = labels.to(device=x.device, dtype=torch.int64).contiguous()
        extra = () if table is None else (table,)
        ctx.save_for_backward(x, labels, *extra)
        ctx.bwd, ctx.order, ctx.ranges = bwd, order, {"r": slice(0, nr), "f": slice(nr, None)}
        res = tuple(v for k in order for v in fwd(x[ctx.ranges[k]], labels[ctx.ranges[k]], *extra))
        ctx.mark_non_differentiable(*(res[i] for i in nondiff))
        return res

    @staticmethod
    def backward(ctx, *gs):
        x, labels, *extra = ctx.saved_tensors
        dx = torch.empty_like(x)
        for k in "rf":
            g, sl = gs[ctx.order.index(k) * (len(gs) // 2)], ctx.ranges[k]
            if g is None:
                dx[sl].zero_()
            else:
                ctx.bwd(x[sl], labels[sl], *extra, g.reshape(1).float().contiguous(), 1.0, dx[sl], False)
        return (dx,) + (None,) * 7


def ce_sum_top1(logits, labels):
    """-> (sum_i CE_i, number of top-1 hits), both 0-dim f32 device tensors."""
    return _RowSum.apply(logits, labels, None, ops.ce_fwd, ops.ce_bwd, (1,))


def ce_sum_top1_split(logits, labels, nr):
    """-> (CE sum, top-1 hits) of rows [0, nr) and of rows [nr, N): four 0-dim f32 device tensors."""
    return _RowSumSplit.apply(logits, labels, None, int(nr), ops.ce_fwd, ops.ce_bwd, (1, 3), "rf")


class _CeSegments(torch.autograd.Function):
    """ce_sum_top1 of several consecutive row segments of ONE logit tensor (gslora_hip.step.distill_step runs the forget batch, the remain
    batch and DER++'s second remain batch as one forward). sizes: the segments' row counts, in order, covering the tensor. Outputs: (CE sum,
    top-1 hits) per segment, in order. Backward writes every segment's rows of a single gradient buffer, as _RowSumSplit does for two."""

    @staticmethod
    def forward(ctx, x, labels, sizes):
        x = x.contiguous().float()
        labels = labels.to(device=x.device, dtype=torch.int64).contiguous()
        ctx.save_for_backward(x, labels)
        ctx.ranges, r0 = [], 0
        for n in sizes:
            ctx.ranges.append(slice(r0, r0 + n))
            r0 += n
        res = tuple(v for sl in ctx.ranges for v in ops.ce_fwd(x[sl], labels[sl]))
        ctx.mark_non_differentiable(*res[1::2])
        return res

    @staticmethod
    def backward(ctx, *gs):
        x, labels = ctx.saved_tensors
        dx = torch.empty_like(x)
        for k, sl in enumerate(ctx.ranges):
            g = gs[2 * k]
            if g is None:
                dx[sl].zero_()
            else:
                ops.ce_bwd(x[sl], labels[sl], g.reshape(1).float().contiguous(), 1.0, dx[sl], False)
        return dx, None, None


def ce_sum_top1_segments(logits, labels, sizes):
    """-> (CE sum, top-1 hits) of each of the consecutive row segments of `sizes` rows: 2 * len(sizes) 0-dim f32 device tensors. A segment
    whose sum is not used gets a zero gradient."""
    sizes = tuple(int(n) for n in sizes)
    if not sizes or min(sizes) < 1 or sum(sizes) != logits.shape[0]:
        raise ValueError(f"ce_sum_top1_segments: segments of {sizes} rows do not cover the {logits.shape[0]} rows of the logits")
    return _CeSegments.apply(logits, labels, sizes)


def proto_kl_sum(emb, labels, table):
    return _RowSum.apply(emb, labels, table, ops.proto_kl_fwd, ops.proto_kl_bwd, ())[0]


def proto_kl_sum_split(emb, labels, table, nr):
    """-> (KL sum of the forget rows [nr, N), KL sum of the remain rows [0, nr))."""
    return _RowSumSplit.apply(emb, labels, table, int(nr), ops.proto_kl_fwd, ops.proto_kl_bwd, (), "fr")


def proto_l2_sum(emb, labels, table):
    """sum_i mean_d (emb[i] - table[labels[i]])^2: divided by the row count, the reference's torch.mean((output - prototype_tensor) ** 2)."""
    return _RowSum.apply(emb, labels, table, ops.proto_l2_fwd, ops.proto_l2_bwd, ())[0]


def proto_l2_sum_split(emb, labels, table, nr):
    """-> (l2 sum of the forget rows [nr, N), l2 sum of the remain rows [0, nr)); see proto_l2_sum."""
    return _RowSumSplit.apply(emb, labels, table, int(nr), ops.proto_l2_fwd, ops.proto_l2_bwd, (), "fr")


PROTO_DISTANCES = ("kl", "l2")


def check_proto_distance(distance):
    if distance not in PROTO_DISTANCES:
        raise ValueError(f"proto_distance must be one of {PROTO_DISTANCES}, got {distance!r}")
    return distance


class _Combine(torch.autograd.Function):
    """total loss of the step from the five batch sums; one kernel forward, one multiply backward (see gsl_loss_combine)."""

    @staticmethod
    def forward(ctx, ce_r_sum, ce_f_sum, kl_f_sum, kl_r_sum, structure, hit_r, hit_f, n_r, n_f, beta, BND, alpha, w_f, w_r, BND_pro):
        f = lambda t: None if t is None else t.detach().float().contiguous()
        total, meters, coefs = ops.loss_combine(f(ce_r_sum), f(ce_f_sum), f(kl_f_sum), f(kl_r_sum), f(structure), f(hit_r), f(hit_f),
                                                n_r, n_f, beta, BND, alpha, w_f, w_r, BND_pro)
        ctx.save_for_backward(coefs)
        ctx.has = (kl_f_sum is not None, kl_r_sum is not None, structure is not None)
        ctx.mark_non_differentiable(meters)
        return total, meters

    @staticmethod
    def backward(ctx, g, _gm):
        (coefs,) = ctx.saved_tensors
        gc = coefs * g                      # one 5-element kernel; the entries below are views
        has_f, has_r, has_s = ctx.has
        return (gc[0], gc[1], gc[2] if has_f else None, gc[3] if has_r else None, gc[4] if has_s else None) + (None,) * 10


def combine(ce_r_sum, ce_f_sum, kl_f_sum, kl_r_sum, structure, hit_r, hit_f, n_r, n_f, beta, BND, alpha, w_f, w_r, BND_pro):
    return _Combine.apply(ce_r_sum, ce_f_sum, kl_f_sum, kl_r_sum, structure, hit_r, hit_f, n_r, n_f, beta, BND, alpha, w_f, w_r,
                          BND_pro)


class _CombinePack(torch.autograd.Function):
    """Data-parallel scalar tail: value from the all-reduced pack (global batch sums and sizes), gradient with respect to this rank's
    local sums (d global sum / d local sum = 1): one kernel forward, one 5-element multiply backward (gsl_loss_combine_pack)."""

    @staticmethod
    def forward(ctx, pack, ce_r_sum, ce_f_sum, kl_f_sum, kl_r_sum, structure, beta, BND, alpha, w_f, w_r, BND_pro):
        has_proto = kl_f_sum is not None
        total, meters, coefs = ops.loss_combine_pack(pack.detach().float().contiguous(),
                                                     None if structure is None else structure.detach().float().contiguous(),
                                                     has_proto, beta, BND, alpha, w_f, w_r, BND_pro)
        ctx.save_for_backward(coefs)
        ctx.has = (has_proto, structure is not None)
        ctx.mark_non_differentiable(meters)
        return total, meters

    @staticmethod
    def backward(ctx, g, _gm):
        (coefs,) = ctx.saved_tensors
        gc = coefs * g
        has_p, has_s = ctx.has
        return (None, gc[0], gc[1], gc[2] if has_p else None, gc[3] if has_p else None, gc[4] if has_s else None) + (None,) * 6


def combine_pack(pack, ce_r_sum, ce_f_sum, kl_f_sum, kl_r_sum, structure, beta, BND, alpha, w_f, w_r, BND_pro):
    return _CombinePack.apply(pack, ce_r_sum, ce_f_sum, kl_f_sum, kl_r_sum, structure, beta, BND, alpha, w_f, w_r, BND_pro)


_table_cache = {}


def prototype_table(prototype_dict, device, dim=None):
    """dict{int -> [D] tensor} (util.utils.calculate_prototypes) -> dense [C, D] f32 device table."""
    key = (id(prototype_dict), str(device))
    ent = _table_cache.get(key)
    if ent is not None and ent[0] is prototype_dict:
        return ent[1]
    C = max(int(k) for k in prototype_dict) + 1
    any_v = next(iter(prototype_dict.values()))
    # a class without a prototype holds NaN: the reference raises KeyError when a batch label misses (engine_cl.py:587-589); here the
    # look-up happens on the device without a host sync, so the loss (and the meters) turn NaN instead of silently using zeros
    table = torch.full((C, any_v.numel()), float("nan"), dtype=torch.float32)
    for k, v in prototype_dict.items():
        table[int(k)] = v.detach().float().cpu().reshape(-1)
    table = table.to(device)
    _table_cache.clear()
    _table_cache[key] = (prototype_dict, table)
    return table


class _StructureLoss(torch.autograd.Function):
    """sum_g ||group g||_2 over the flat LoRA bucket; backward adds coef * t/||g|| straight into the
    flat gradient bucket (the parameters' .grad views)."""

    @staticmethod
    def forward(ctx, bucket, tgroup, ngroups, grad_scale, *params):
        out = ops.group_norms_fwd(bucket.flat, bucket.toff, bucket.tnumel, tgroup, ngroups)
        ctx.bucket, ctx.tgroup, ctx.norm, ctx.grad_scale, ctx.n = bucket, tgroup, out["group_norm"], grad_scale, len(params)
        return out["loss"][0]

    @staticmethod
    def backward(ctx, g):
        b = ctx.bucket
        b.attach_grads()
        ops.group_norms_bwd(b.flat, b.toff, b.tnumel, ctx.tgroup, ctx.norm, g.reshape(1).float().contiguous(),
                            ctx.grad_scale, b.grad)
        return (None, None, None, None) + (None,) * ctx.n


def structure_loss(model, group_type="block", grad_scale=1.0):
    """Differentiable group-lasso term. grad_scale lets a data-parallel engine pre-divide the
    (rank-identical) parameter-only gradient by the world size before the gradient all-reduce."""
    bucket = model.lora_bucket()
    if bucket is None:
        raise RuntimeError("structure loss needs a model with LoRA parameters (lora_rank > 0)")
    tgroup, ng = bucket.group_table(group_type)
    trainable = [p for p in bucket.params if p.requires_grad]
    if torch.is_grad_enabled() and trainable:
        return _StructureLoss.apply(bucket, tgroup, ng, grad_scale, *trainable)
    return ops.group_norms_fwd(bucket.flat, bucket.toff, bucket.tnumel, tgroup, ng)["loss"][0]


def group_report(model, group_type="block", tau=0.0):
    """All K12 observables in one launch: group-lasso norms, cal_norm (sum of Frobenius norms),
    the selection mask (norm > tau) and the loss."""
    bucket = model.lora_bucket()
    tgroup, ng = bucket.group_table(group_type)
    return ops.group_norms_fwd(bucket.flat, bucket.toff, bucket.tnumel, tgroup, ng, tau=tau)
