"""ViT-Face with rank-r LoRA on the two FFN linears — MI355X-native drop-in for the reference
`vit_pytorch_face/vit_face.py` (ViT_face :449-548, Transformer :382-446, Attention :341-379,
FeedForward :326-338, PreNorm :316-323, Residual :307-313, CosFace :146-223, ArcFace :72-143,
Softmax :14-69).

The module tree, parameter names and shapes are exactly the reference's (state_dict compatible:
`transformer.layers.{i}.1.fn.fn.net.{0,3}.lora_{A,B}` ...), the parameters are real
`nn.Parameter`s, `train()/eval()` keep loralib's merge semantics — but none of the sub-modules
computes anything in PyTorch. `ViT_face.forward` hands the whole network to
`gslora_hip.vit_runner.ViTRunner`, which runs the hand-written gfx950 kernels (forward) and, through
one `torch.autograd.Function`, the hand-derived backward that fills `lora_*.grad`.
There is no CPU fallback: calling the model on CPU tensors raises.
"""
import math
import os
import weakref

import torch
import torch.nn as nn

import loralib as lora
from gslora_hip.ops import check_lora_rank, check_num_tokens
from gslora_hip.vit_runner import BlockSpec, ModelSpec, ViTRunner

MIN_NUM_PATCHES = 16
_DTYPES = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp16": torch.float16, "f16": torch.float16, "float16": torch.float16, "half": torch.float16,
           "fp32": torch.float32, "f32": torch.float32, "float32": torch.float32}


# "fp32x3": float32 tensors and kernels like "fp32", with the GEMMs' products on the bf16 matrix cores (GSL_F32X3: three bf16 pieces per operand, six
# products, f32-accurate — include/gslora_hip.h). The torch dtype of the mode is float32; the GEMM mode travels beside it (gemm_mode_of / compute_mode).
_GEMM_MODES = {"fp32x3": "x3", "f32x3": "x3", "float32x3": "x3"}
_MODE_NAMES = {torch.float16: "fp16", torch.bfloat16: "bf16", torch.float32: "fp32"}


def compute_dtype_of(name):
    """'fp16' | 'bf16' | 'fp32' | 'fp32x3' (and their aliases) or a torch dtype -> torch dtype ('fp32x3' is torch.float32: gemm_mode_of has the
    rest); ValueError lists the allowed names."""
    if not isinstance(name, str):
        if name in (torch.float32, torch.bfloat16, torch.float16):
            return name
        raise ValueError(f"gs-lora_amd: compute dtype must be torch.float32 / bfloat16 / float16, not {name!r}")
    if name.lower() in _GEMM_MODES:
        return torch.float32
    try:
        return _DTYPES[name.lower()]
    except KeyError:
        raise ValueError(f"gs-lora_amd: unknown compute dtype {name!r}; allowed: {sorted(_DTYPES) + sorted(_GEMM_MODES)}") from None


def gemm_mode_of(name):
    """The f32_mode of gslora_hip.ops.gemm_nt that a compute-dtype name selects: "x3" for 'fp32x3', None for every other name or torch dtype."""
    return _GEMM_MODES.get(name.lower()) if isinstance(name, str) else None


def compute_mode_name(dtype, gemm_mode=None):
    """(torch dtype, f32_mode) -> 'fp16' | 'bf16' | 'fp32' | 'fp32x3': the name that set_compute_dtype takes back."""
    return "fp32x3" if (dtype == torch.float32 and gemm_mode == "x3") else _MODE_NAMES[dtype]


class CosFace(nn.Module):
    """Parameter holder for the CosFace head (s=64, m=0.35; reference :146-223). The margin is applied
    whenever a label is passed, in train and eval alike; the arithmetic lives in gsl_head_fwd/bwd."""

    def __init__(self, in_features, out_features, device_id, s=64.0, m=0.35):
        super().__init__()
        self.in_features, self.out_features, self.device_id, self.s, self.m = in_features, out_features, device_id, s, m
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        nn.init.xavier_uniform_(self.weight)

    def forward(self, emb, label):
        raise RuntimeError("CosFace is evaluated inside ViT_face.forward (fused HIP head kernel)")

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}, s={self.s}, m={self.m}"


class ArcFace(nn.Module):
    """Parameter holder for the ArcFace head (s=64, m=0.5, easy_margin=False; reference :72-143): the label column's logit is
    s * phi(cos), phi = cos(theta + m) above the threshold th = cos(pi - m), cos - mm below it (easy_margin: phi above 0, cos below).
    Same attributes as the reference; the arithmetic lives in gsl_head_fwd_margin / gsl_head_bwd_margin, which take s and m from here."""

    def __init__(self, in_features, out_features, device_id, s=64.0, m=0.50, easy_margin=False):
        super().__init__()
        self.in_features, self.out_features, self.device_id, self.s, self.m = in_features, out_features, device_id, s, m
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        nn.init.xavier_uniform_(self.weight)
        self.easy_margin = easy_margin
        self.cos_m = math.cos(m)
        self.sin_m = math.sin(m)
        self.th = math.cos(math.pi - m)
        self.mm = math.sin(math.pi - m) * m

    def forward(self, emb, label):
        raise RuntimeError("ArcFace is evaluated inside ViT_face.forward (fused HIP head kernel)")

    def extra_repr(self):
        return (f"in_features={self.in_features}, out_features={self.out_features}, s={self.s}, m={self.m}, "
                f"easy_margin={self.easy_margin}")


class Softmax(nn.Module):
    """Parameter holder for the plain classification head (reference :14-69): logits = emb W^T + b, computed when a label is passed
    (the label itself is ignored), by the linear path of gsl_head_fwd / gsl_head_bwd."""

    def __init__(self, in_features, out_features, device_id):
        super().__init__()
        self.in_features, self.out_features, self.device_id = in_features, out_features, device_id
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features))
        nn.init.xavier_uniform_(self.weight)
        nn.init.zeros_(self.bias)

    def forward(self, emb, label):
        raise RuntimeError("Softmax is evaluated inside ViT_face.forward (fused HIP head kernel)")

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}"


# loss_type -> (holder class, ModelSpec.head_kind)
_HEADS = {"CosFace": (CosFace, "cosface"), "ArcFace": (ArcFace, "arcface"), "Softmax": (Softmax, "softmax")}


class _Holder(nn.Module):
    def forward(self, *a, **k):
        raise RuntimeError(f"{type(self).__name__} is a parameter holder; call ViT_face.forward (fused HIP path)")


class Residual(_Holder):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn


class PreNorm(_Holder):
    def __init__(self, dim, fn):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.fn = fn


class FeedForward(_Holder):
    def __init__(self, dim, hidden_dim, dropout=0.0, lora_rank=8):
        super().__init__()
        self.net = nn.Sequential(lora.Linear(dim, hidden_dim, r=lora_rank), nn.GELU(), nn.Dropout(dropout),
                                 lora.Linear(hidden_dim, dim, r=lora_rank), nn.Dropout(dropout))

    def lora_params(self):
        a, b = self.net[0], self.net[3]
        return (a.lora_A, a.lora_B, b.lora_A, b.lora_B)


class Attention(_Holder):
    def __init__(self, dim, heads=8, dim_head=64, dropout=0.0, lora_rank=0):
        super().__init__()
        if dim_head != 64:
            raise NotImplementedError("gs-lora_amd attention kernels are specialised for dim_head = 64")
        inner = dim_head * heads
        self.heads = heads
        self.scale = dim ** -0.5        # reference quirk (:346): dim, not dim_head
        self.to_qkv = lora.MergedLinear(in_features=dim, out_features=inner * 3, r=lora_rank,
                                        enable_lora=[True, True, True], bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, dim), nn.Dropout(dropout))


class Transformer(_Holder):
    def __init__(self, dim, depth, heads, dim_head, mlp_dim, dropout, lora_rank, up=False, lora_pos="FFN"):
        super().__init__()
        if lora_pos not in ("FFN", "Attention"):
            raise ValueError("lora_pos must be 'FFN' (GS-LoRA) or 'Attention' (the reference's ablation)")
        # reference :400-425: the adapters sit either on the two FFN linears or on the QKV projection, never on both
        self.layers = nn.ModuleList([
            nn.ModuleList([Residual(PreNorm(dim, Attention(dim, heads=heads, dim_head=dim_head, dropout=dropout,
                                                           lora_rank=lora_rank if lora_pos == "Attention" else 0))),
                           Residual(PreNorm(dim, FeedForward(dim, mlp_dim, dropout=dropout,
                                                             lora_rank=lora_rank if lora_pos == "FFN" else 0)))])
            for _ in range(depth)])
        self.up = up
        self.depth = depth


class _ViTFaceFn(torch.autograd.Function):
    """One autograd node for the whole network. The trainable parameters are passed so that autograd sees the dependency: first the head's
    (loss.weight, loss.bias — those that require a gradient), then the LoRA ones. LoRA gradients are accumulated straight into the flat
    bucket whose views are the parameters' .grad (same observable result as autograd accumulation, no per-tensor copies); the head's are
    freshly written buffers (gsl_head_wgrad) that autograd accumulates into .grad.
    mode True: the whole backward chain runs (LoRA, plus the head's one launch when it trains). mode "head" (no trainable LoRA parameter):
    the forward keeps nothing of the blocks and the backward is that one launch. mode "ffn" (a model without LoRA whose FFN linears train,
    the reference's --only_ffn): the parameters behind the head's are the FFN weights and biases, the backward chain forms their gradients
    with gst_wgrad into fresh buffers that autograd accumulates into .grad, like the head's."""

    @staticmethod
    def forward(ctx, runner, img, label, mode, n_head, *params):
        logits, emb, saved = runner.forward(img, label, save=mode)
        ctx.runner, ctx.saved, ctx.mode, ctx.n_head, ctx.n = runner, saved, mode, n_head, len(params)
        ctx.ffn_ids = [id(p) for p in params[n_head:]] if mode == "ffn" else None
        if logits is None:
            return emb
        return logits, emb

    @staticmethod
    def backward(ctx, *grads):
        if ctx.saved is None:
            raise RuntimeError("ViT_face backward called twice (activations are released after the first pass)")
        if len(grads) == 2:
            dlogits, demb = grads
        else:
            dlogits, demb = None, grads[0]
        head_grads = (None,) * ctx.n_head
        if ctx.n_head:      # d loss / d (loss.weight, loss.bias): demb (the prototype term) reaches the head's parameters through nothing
            head_grads = ctx.runner.head_param_grads(ctx.saved, dlogits, ctx.needs_input_grad[5:5 + ctx.n_head])
        rest = (None,) * (ctx.n - ctx.n_head)
        if ctx.mode is True:
            ctx.runner.backward(ctx.saved, dlogits, demb)
        elif ctx.mode == "ffn":
            wg = ctx.runner.backward(ctx.saved, dlogits, demb)
            rest = tuple(wg[i] if need else None for i, need in zip(ctx.ffn_ids, ctx.needs_input_grad[5 + ctx.n_head:]))
        ctx.saved = None
        return (None,) * 5 + tuple(head_grads) + rest


# the speed mode a model starts in (GSLORA_DTYPE overrides): IEEE fp16 operands since round 5 — same kernels, bytes and MFMA rate as bf16,
# 3 more significand bits on every matrix-core operand; DESIGN.md section 7 has what that buys in trajectory fidelity
DEFAULT_DTYPE = "fp16"


class HipModelMixin:
    """Shared by the model families that run on ViTRunner (ViT_face, ModifiedViT): compute-dtype switch, the lazily built
    runner / flat LoRA bucket, and the one-autograd-node call."""
    _runner = None
    gemm_mode = None                # f32_mode of the GEMMs (gslora_hip.ops.gemm_nt): "x3" in the 'fp32x3' mode, None otherwise
    input_norm = None               # (mean, std) once set_input_norm() was called: uint8 batches are raw bytes normalised in the patch gather
    accepts_batch_tuple = True      # forward(img) also takes a tuple of image batches, processed as one batch (gslora_hip.step)

    def set_compute_dtype(self, name):
        """'fp16' / 'bf16' (speed: 16-bit MFMA operands of that format, f32 accumulate; fp16 runs its backward on loss-scaled gradients)
        or 'fp32' (parity: exact-f32 kernels), or 'fp32x3' (float32 tensors and kernels as 'fp32', the GEMMs on the bf16 matrix cores at f32
        accuracy: compute_dtype is torch.float32, gemm_mode "x3"). A torch dtype selects its plain mode."""
        self.compute_dtype, self.gemm_mode = compute_dtype_of(name), gemm_mode_of(name)
        return self

    @property
    def compute_mode(self):
        """'fp16' | 'bf16' | 'fp32' | 'fp32x3': the name of the current mode. Code that switches the mode for a while (the evaluations) saves
        THIS and hands it back to set_compute_dtype — compute_dtype alone would turn an 'fp32x3' model into 'fp32'."""
        return compute_mode_name(self.compute_dtype, self.gemm_mode)

    def set_input_norm(self, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
        """Declare that uint8 batches are raw image bytes, to be normalised as the dataset transform ToTensor() + Normalize(mean, std)
        would: x = ((u / 255) - mean[c]) / std[c], evaluated inside the patch gather (gsl_patchify_u8 / gsl_unfold_patches_u8), so the
        batch crosses the host boundary in one byte per sub-pixel. mean / std: one value per channel, or a name — "totensor" (mean 0,
        std 1: the face drivers) or "imagenet" (the ImageNet constants: the ImageNet-100 driver). set_input_norm(None) withdraws it.
        float batches are untouched either way; without this call a uint8 batch is a value cast, as the reference's inputs.float()."""
        from gslora_hip import ops
        if mean is None:
            self.input_norm = None
            return self
        if isinstance(mean, str):
            if mean.lower() not in ops.INPUT_NORMS:
                raise ValueError(f"set_input_norm: unknown name {mean!r}; use one of {sorted(ops.INPUT_NORMS)} or per-channel values")
            mean, std = ops.INPUT_NORMS[mean.lower()]
        norm = (tuple(float(v) for v in mean), tuple(float(v) for v in std))
        ops.u8_norm_table(*norm)      # validates (one entry per channel, non-zero std)
        self.input_norm = norm
        return self

    def runner(self):
        if self._runner is None:
            self._runner = ViTRunner(self)
        return self._runner

    def lora_bucket(self):
        """Flat f32 storage behind the LoRA parameters (created on first use on the GPU)."""
        return self.runner().ensure_bucket()

    def invalidate_operand_caches(self):
        """Drop the runner's operand-format copies of the frozen weights (16-bit [N,K] / [K,N] forms, the gamma-folded QKV weight with its c / d
        vectors, the normalised CosFace weight). They are keyed on (data_ptr, _version) of their parameters, which in-place autograd-visible
        updates (loralib merge / un-merge, load_state_dict's copy_) bump — writes through `.data` do not: call this after one."""
        if self._runner is not None:
            self._runner.invalidate_operand_caches()

    def load_state_dict(self, state_dict, strict=True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self.invalidate_operand_caches()      # (copy_ bumps the versions anyway; explicit so that a custom loader writing through .data is covered too)
        return out

    # names of the non-LoRA parameters that may train on the HIP path: the classifier head of ViT_face / ViTs_face (the linear probe of
    # train/backbone_forget_main.py:596-600, the baselines' --ffn_open), whose gradient is gsl_head_wgrad
    trainable_head = ()
    # name fragment of the backbone weights that may train: the two FFN linears of every block, weight and bias — the reference's --only_ffn
    # rule (train/train_own_forget_cl.py:432-439) — in a model built WITHOUT LoRA (lora_rank = 0); their gradients are gst_wgrad's
    trainable_ffn = ""
    _frozen_note = ""

    def _hip_call(self, img, label):
        runner = self.runner()
        spec = self.hip_spec()
        lora_params = [p for blk in spec.blocks for p in blk.lora_params()] if spec.lora_rank > 0 else []
        grad_on = torch.is_grad_enabled()
        head_params, ffn_params = [], []
        if grad_on:
            for n, p in self.named_parameters():
                if not p.requires_grad or "lora_" in n:
                    continue
                if self.trainable_ffn and self.trainable_ffn in n:
                    if spec.lora_rank > 0:
                        raise RuntimeError(f"gs-lora_amd {type(self).__name__}: parameter {n!r} requires a gradient, but this model holds LoRA adapters "
                                           f"(lora_rank = {spec.lora_rank}): the FFN weights train only in a model built with lora_rank = 0 (the "
                                           "reference's --only_ffn baselines); LoRA and FFN weights training together is not implemented")
                    ffn_params.append(p)
                    continue
                if n not in self.trainable_head:
                    raise RuntimeError(f"gs-lora_amd {type(self).__name__}: parameter {n!r} requires a gradient, but the HIP path trains the LoRA "
                                       f"parameters{' and the classifier head (loss.weight, loss.bias)' if self.trainable_head else ''} only"
                                       f"{' (and, in a model built with lora_rank = 0, the FFN linears: names containing fn.fn.net)' if self.trainable_ffn else ''}"
                                       f"{self._frozen_note}: call loralib.mark_only_lora_as_trainable(model) first, set requires_grad by name "
                                       "as train/backbone_forget_main.py:596-600 does, or run under torch.no_grad()")
                head_params.append(p)
        if ffn_params:      # the third backward configuration (ViTRunner.backward): needs logits or an embedding gradient like the LoRA one
            out = _ViTFaceFn.apply(runner, img, label, "ffn", len(head_params), *head_params, *ffn_params)
            return out if isinstance(out, tuple) else (None, out)
        lora_live = grad_on and any(p.requires_grad for p in lora_params)
        if lora_live or (head_params and label is not None):
            # (without a label there are no logits: the head's parameters take no part in the forward)
            out = _ViTFaceFn.apply(runner, img, label, True if lora_live else "head", len(head_params), *head_params, *lora_params)
            return out if isinstance(out, tuple) else (None, out)
        logits, emb, _ = runner.forward(img, label, save=False)
        return logits, emb


class ViT_face(HipModelMixin, nn.Module):
    trainable_head = ("loss.weight", "loss.bias")
    trainable_ffn = "fn.fn.net"
    _transformer_up = False                              # Transformer(up=...): True in ViT_face_up
    _transformer_depth = staticmethod(lambda depth: depth)      # blocks the module owns: depth // 2 in ViT_face_low

    def __init__(self, *, loss_type, GPU_ID, num_class, image_size, patch_size, dim, depth, heads, mlp_dim, pool="cls",
                 channels=3, dim_head=64, dropout=0.0, emb_dropout=0.0, lora_rank=8, lora_pos: str = "FFN"):
        super().__init__()
        assert image_size % patch_size == 0, "Image dimensions must be divisible by the patch size."
        num_patches = (image_size // patch_size) ** 2
        patch_dim = channels * patch_size ** 2
        assert num_patches > MIN_NUM_PATCHES, (
            f"your number of patches ({num_patches}) is way too small for attention to be effective (at least 16). "
            "Try decreasing your patch size")
        assert pool in {"cls", "mean"}, "pool type must be either cls (cls token) or mean (mean pooling)"
        if patch_dim % 64 or dim % 64 or mlp_dim % 64:
            raise NotImplementedError("gs-lora_amd GEMM tiles need patch_dim, dim and mlp_dim to be multiples of 64")
        check_num_tokens("ViT_face", num_patches + 1)
        check_lora_rank("ViT_face", lora_rank, attention_site=(lora_pos == "Attention"))
        self.patch_size = patch_size
        self.pos_embedding = nn.Parameter(torch.randn(1, num_patches + 1, dim))
        self.patch_to_embedding = nn.Linear(patch_dim, dim)
        self.cls_token = nn.Parameter(torch.randn(1, 1, dim))
        self.dropout = nn.Dropout(emb_dropout)
        self.transformer = Transformer(dim, self._transformer_depth(depth), heads, dim_head, mlp_dim, dropout, lora_rank, up=self._transformer_up,
                                       lora_pos=lora_pos)
        self.pool = pool
        self.to_latent = nn.Identity()
        self.mlp_head = nn.Sequential(nn.LayerNorm(dim))
        self.loss_type = loss_type
        self.GPU_ID = GPU_ID
        if loss_type == "None":
            print("no loss for vit_face")
        elif loss_type in _HEADS:
            self.loss = _HEADS[loss_type][0](in_features=dim, out_features=num_class, device_id=GPU_ID)
        elif loss_type == "SFace":
            raise NotImplementedError(
                "gs-lora_amd does not implement the SFace head: the reference's training CLI cannot build it (config.py accepts "
                "'SFaceLoss' while ViT_face checks 'SFace'), and its forward returns a 6-tuple that the GS-LoRA engines cannot consume")
        else:
            raise NotImplementedError(f"gs-lora_amd implements the heads {sorted(_HEADS)}, not {loss_type}")
        # geometry consumed by the runner
        self.dim, self.depth, self.heads, self.mlp_dim = dim, depth, heads, mlp_dim
        self.num_tokens = num_patches + 1
        self.lora_rank = lora_rank
        self.lora_pos = lora_pos
        self.attn_scale = dim ** -0.5
        self.dropout_p, self.emb_dropout_p = float(dropout), float(emb_dropout)
        self.set_compute_dtype(os.environ.get("GSLORA_DTYPE", DEFAULT_DTYPE))
        self._runner = None

    # ---- helpers for the runner -------------------------------------------------------------
    def blocks(self):
        for attn, ff in self.transformer.layers:
            yield attn.fn, ff.fn          # the two PreNorm modules of a block

    def ffn_blocks(self):
        for _, ff in self.transformer.layers:
            yield ff.fn.fn

    def hip_spec(self):
        """What the kernels need to know about this family (see gslora_hip.vit_runner.ModelSpec)."""
        blocks = []
        for attn, ff in self.transformer.layers:
            a, f = attn.fn, ff.fn
            blocks.append(BlockSpec(a.norm, a.fn.to_qkv.weight, None, a.fn.to_out[0], f.norm, f.fn.net[0], f.fn.net[3],
                                    qkv_lora=a.fn.to_qkv if self.lora_pos == "Attention" and self.lora_rank > 0 else None))
        has_loss = self.loss_type in _HEADS
        kind = _HEADS[self.loss_type][1] if has_loss else "cosface"
        return ModelSpec(patch_size=self.patch_size, num_tokens=self.num_tokens, dim=self.dim, heads=self.heads,
                         attn_scale=self.attn_scale, ln_eps=1e-5, dropout_p=self.dropout_p, emb_dropout_p=self.emb_dropout_p,
                         lora_rank=self.lora_rank, patch_w=self.patch_to_embedding.weight, patch_is_conv=False,
                         patch_b=self.patch_to_embedding.bias, cls=self.cls_token, pos=self.pos_embedding, blocks=blocks,
                         final_ln=self.mlp_head[0], head_kind=kind, head_w=self.loss.weight if has_loss else None,
                         head_b=self.loss.bias if kind == "softmax" else None,
                         cos_s=self.loss.s if has_loss and kind != "softmax" else 64.0,
                         cos_m=self.loss.m if has_loss and kind != "softmax" else 0.35,
                         easy_margin=bool(self.loss.easy_margin) if kind == "arcface" else False,
                         lora_site="attention" if self.lora_pos == "Attention" else "ffn", pool=self.pool)

    # ---- reference API ---------------------------------------------------------------------------
    def forward(self, img, label=None, mask=None):
        """:return: (logits, emb) if label is given else emb — as the reference (:523-548)."""
        if mask is not None:
            raise NotImplementedError("attention masks are never passed by the GS-LoRA engines")
        logits, emb = self._hip_call(img, label)
        return emb if label is None else (logits, emb)


_REQUIRED = object()      # default of the keywords the reference's half-network constructors require, see _check_required
_HALF_REQUIRED = ("loss_type", "GPU_ID", "num_class", "image_size", "patch_size", "dim", "depth", "heads", "mlp_dim")
# low -> {id(up): _LowUpPair}, up -> the pairs it serves: invalidate_operand_caches() of either half reaches the pair's runner. Weak keys: a
# pair lives as long as its student.
_PAIRS_OF_LOW = weakref.WeakKeyDictionary()
_PAIRS_OF_UP = weakref.WeakKeyDictionary()
_LIRF_HINT = ("the halves run standalone under torch.no_grad() only (evaluation, the teacher, the deposit network); a training pass runs "
              "both halves as one, through gslora_hip.step.lirf_step")


def _check_required(cls, given):
    """The reference's ViT_face_low / ViT_face_up constructors have nine required keyword arguments. Here they carry a sentinel default
    and are checked by hand, so that a call without them raises NotImplementedError — what the placeholder classes these replace raised
    for any call, and what callers that probe for the LIRF baseline (and tests/test_host_logic.py) still expect of `ViT_face_low()`."""
    missing = [k for k in _HALF_REQUIRED if given[k] is _REQUIRED]
    if missing:
        raise NotImplementedError(f"{cls.__name__} needs the keyword arguments of the reference's constructor (vit_face.py:551-781): missing "
                                  f"{', '.join(missing)}")


class _HalfMixin:
    """What ViT_face_low and ViT_face_up share: the refusals of a standalone call and the reach of invalidate_operand_caches()."""

    def _standalone(self, mask):
        if mask is not None:
            raise NotImplementedError("attention masks are never passed by the GS-LoRA engines")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError(f"gs-lora_amd {type(self).__name__}: called with gradients enabled and trainable parameters; {_LIRF_HINT}")

    def invalidate_operand_caches(self):
        super().invalidate_operand_caches()
        pairs = (_PAIRS_OF_LOW.get(self) or {}).values() if isinstance(self, ViT_face_low) else list(_PAIRS_OF_UP.get(self) or ())
        for pair in pairs:
            pair.invalidate_operand_caches()


class ViT_face_low(_HalfMixin, ViT_face):
    """The lower half of a ViT_face for the LIRF baseline (reference vit_face.py:551-666): the patch stage and blocks 0 .. depth // 2 - 1;
    forward(img) -> the stream [B, T, D] in the stream dtype of the compute mode (f32 in the fp32 modes). Parameter names are the
    reference's: `transformer.layers.{0 .. depth // 2 - 1}` plus, unused, the final LayerNorm `mlp_head` and the head `loss`, so
    load_state_dict(full_checkpoint, strict=False) fills it and reports the upper blocks alone as unexpected. img may be a tuple of
    batches or uint8 (set_input_norm), as for ViT_face."""

    _transformer_depth = staticmethod(lambda depth: depth // 2)

    def __init__(self, *, loss_type=_REQUIRED, GPU_ID=_REQUIRED, num_class=_REQUIRED, image_size=_REQUIRED, patch_size=_REQUIRED,
                 dim=_REQUIRED, depth=_REQUIRED, heads=_REQUIRED, mlp_dim=_REQUIRED, pool="cls", channels=3, dim_head=64, dropout=0.0,
                 emb_dropout=0.0, lora_rank=8, lora_pos: str = "FFN"):
        _check_required(type(self), locals())
        if depth < 2:
            raise NotImplementedError("gs-lora_amd ViT_face_low / ViT_face_up: depth must be at least 2 (depth // 2 lower blocks)")
        super().__init__(loss_type=loss_type, GPU_ID=GPU_ID, num_class=num_class, image_size=image_size, patch_size=patch_size, dim=dim,
                         depth=depth, heads=heads, mlp_dim=mlp_dim, pool=pool, channels=channels, dim_head=dim_head, dropout=dropout,
                         emb_dropout=emb_dropout, lora_rank=lora_rank, lora_pos=lora_pos)
        self.split = depth // 2

    def hip_spec(self):
        sp = super().hip_spec()
        sp.final_ln, sp.head_w, sp.head_b, sp.stream_out = None, None, None, True
        return sp

    def forward(self, img, label=None, mask=None):
        """:return: the stream behind block depth // 2 - 1, [B, T, D] — as the reference (:638-665); label is not used."""
        self._standalone(mask)
        return self.runner().forward(img, None, save=False)[1]


class ViT_face_up(_HalfMixin, ViT_face):
    """The upper half of a ViT_face for the LIRF baseline (reference vit_face.py:668-781): blocks depth // 2 .. depth - 1 of a full-depth
    Transformer(up=True), then pooling, the final LayerNorm and the head; forward(x, label) -> (logits, emb), or emb without a label, from
    the lower half's stream x [B, T, D] (f32 or the stream dtype of the compute mode). It owns, unused, the patch embedding, cls_token,
    pos_embedding and the lower blocks, as the reference does: load_state_dict(full_checkpoint, strict=False) reports nothing unexpected.
    The dropout sites keep the network-wide block indices."""

    _transformer_up = True
    stream_in = True

    def __init__(self, *, loss_type=_REQUIRED, GPU_ID=_REQUIRED, num_class=_REQUIRED, image_size=_REQUIRED, patch_size=_REQUIRED,
                 dim=_REQUIRED, depth=_REQUIRED, heads=_REQUIRED, mlp_dim=_REQUIRED, pool="cls", channels=3, dim_head=64, dropout=0.0,
                 emb_dropout=0.0, lora_rank=8, lora_pos: str = "FFN"):
        _check_required(type(self), locals())
        if depth < 2:
            raise NotImplementedError("gs-lora_amd ViT_face_low / ViT_face_up: depth must be at least 2 (depth // 2 lower blocks)")
        super().__init__(loss_type=loss_type, GPU_ID=GPU_ID, num_class=num_class, image_size=image_size, patch_size=patch_size, dim=dim,
                         depth=depth, heads=heads, mlp_dim=mlp_dim, pool=pool, channels=channels, dim_head=dim_head, dropout=dropout,
                         emb_dropout=emb_dropout, lora_rank=lora_rank, lora_pos=lora_pos)
        self.split = depth // 2

    def hip_spec(self):
        sp = super().hip_spec()
        sp.blocks, sp.block0, sp.stream_in = sp.blocks[self.split:], self.split, True
        return sp

    def forward(self, x, label=None, mask=None):
        """:return: (logits, emb) if label is given else emb — as the reference (:755-781)."""
        self._standalone(mask)
        logits, emb, _ = self.runner().forward(x, label, save=False)
        return emb if label is None else (logits, emb)


class _LowUpPair:
    """A student ViT_face_low and a ViT_face_up as ONE model in front of a ViTRunner of its own: the patch stage and blocks [0, k) are the
    student's, blocks [k, depth), the final LayerNorm and the head the upper module's. The runner's operand caches are keyed per site and
    tagged with their parameters' (data_ptr, _version), so they serve the two modules' tensors like one model's."""
    accepts_batch_tuple = True

    def __init__(self, low, up):
        for a in ("dim", "depth", "heads", "mlp_dim", "num_tokens", "patch_size", "attn_scale"):
            if getattr(low, a) != getattr(up, a):
                raise ValueError(f"ViT_face_low / ViT_face_up: the halves differ in {a} ({getattr(low, a)} against {getattr(up, a)})")
        self._low, self.up = weakref.ref(low), up
        self._runner = None

    @property
    def low(self):
        low = self._low()
        if low is None:
            raise RuntimeError("ViT_face_low / ViT_face_up: the student's lower half no longer exists")
        return low

    def runner(self):
        if self._runner is None:
            self._runner = ViTRunner(self)
        return self._runner

    def invalidate_operand_caches(self):
        if self._runner is not None:
            self._runner.invalidate_operand_caches()

    # ---- what ViTRunner reads of its model
    compute_dtype = property(lambda self: self.low.compute_dtype)
    gemm_mode = property(lambda self: self.low.gemm_mode)
    input_norm = property(lambda self: self.low.input_norm)
    training = property(lambda self: self.low.training)

    def check_modes(self):
        low, up = self.low, self.up
        if low.compute_mode != up.compute_mode:
            raise RuntimeError(f"ViT_face_low / ViT_face_up: one pass runs in one compute mode; the student's half is in {low.compute_mode!r}, "
                               f"the upper half in {up.compute_mode!r} (set_compute_dtype)")

    def hip_spec(self):
        low, up = self.low, self.up
        sp, su = ViT_face.hip_spec(low), ViT_face.hip_spec(up)
        k = low.split
        su.blocks = sp.blocks + su.blocks[k:]
        su.boundary = k
        su.patch_w, su.patch_b, su.cls, su.pos = sp.patch_w, sp.patch_b, sp.cls, sp.pos
        # dropout: the lower blocks and the embedding follow the student's rate and mode (the pass's), the upper blocks the upper module's
        # own — the reference's loop trains student_low.train() under teacher_up.eval()
        su.dropout_p, su.emb_dropout_p = sp.dropout_p, sp.emb_dropout_p
        su.dropout_p_up = up.dropout_p if up.training else 0.0
        return su


def low_up_pair(low, up):
    """The pair object (and through it the runner) that serves this student and this upper half; made once per couple."""
    pairs = _PAIRS_OF_LOW.setdefault(low, {})
    pair = pairs.get(id(up))
    if pair is None or pair.up is not up:
        pair = pairs[id(up)] = _LowUpPair(low, up)
        _PAIRS_OF_UP.setdefault(up, weakref.WeakSet()).add(pair)
    return pair


class _LowUpFn(torch.autograd.Function):
    """One autograd node for up(low(img), label) with the attention-transfer term of the mid stream as a third output. The parameters
    handed over are the student's trainable FFN tensors; their gradients come from ViTRunner.backward (gst_wgrad), where the gradient of
    the third output enters at the boundary between the halves."""

    @staticmethod
    def forward(ctx, runner, img, label, at_images, at_teacher, *params):
        from gslora_hip import at as AT
        logits, emb, saved = runner.forward(img, label, save="ffn")
        c = saved["ctx"]
        G = None
        if at_teacher is not None:
            mid = saved["layers"][c.sp.boundary]["x"]      # block k's saved input IS the student's mid stream: no copy
            at_value, G = AT.at_loss_value_and_table(mid, at_images, c.T, at_teacher.to(mid.dtype))
        else:
            at_value = torch.zeros((), device=c.dev, dtype=torch.float32)
        ctx.runner, ctx.saved, ctx.G, ctx.ids = runner, saved, G, [id(p) for p in params]
        return logits, emb, at_value

    @staticmethod
    def backward(ctx, dlogits, demb, dat):
        if ctx.saved is None:
            raise RuntimeError("ViT_face_low / ViT_face_up backward called twice (activations are released after the first pass)")
        at = None
        if ctx.G is not None and dat is not None:
            at = (ctx.G, dat.detach().float().reshape(1).contiguous())      # a device float: the upstream gradient times the term's weight
        wg = ctx.runner.backward(ctx.saved, dlogits, demb, at=at)
        ctx.saved = ctx.G = None
        return (None,) * 5 + tuple(wg.get(i) if need else None for i, need in zip(ctx.ids, ctx.needs_input_grad[5:]))


def low_up_forward(low, up, img, label, at_images=0, at_teacher=None):
    """up(low(img), label) as one pass with a backward: -> (logits, emb, at_value). img: a batch or a tuple of batches; at_teacher: the
    teacher's mid stream [at_images, T, D] for the first at_images images, or None (at_value is then a constant 0). The trainable set is
    the reference's --only_ffn rule on the student's half (names containing fn.fn.net) in models built with lora_rank = 0; every
    parameter of the upper half is frozen. Used by gslora_hip.step.lirf_step."""
    for m in (low, up):
        if m.lora_rank > 0:
            raise RuntimeError(f"gs-lora_amd {type(m).__name__}: a training pass over both halves trains the FFN linears of models built with "
                               f"lora_rank = 0 (the reference's --only_ffn rule); this {type(m).__name__} holds LoRA adapters (lora_rank = "
                               f"{m.lora_rank})")
    params = []
    for n, p in low.named_parameters():
        if p.requires_grad:
            if low.trainable_ffn not in n:
                raise RuntimeError(f"gs-lora_amd ViT_face_low: parameter {n!r} requires a gradient, but the HIP path trains the FFN linears "
                                   "(names containing fn.fn.net) of the student's half only; set requires_grad by that rule first")
            params.append(p)
    frozen = [n for n, p in up.named_parameters() if p.requires_grad]
    if frozen:
        raise RuntimeError(f"gs-lora_amd ViT_face_up: parameter {frozen[0]!r} requires a gradient, but the upper half is the frozen, shared "
                           "network of the LIRF step")
    if not params or not torch.is_grad_enabled():
        raise RuntimeError(f"gs-lora_amd ViT_face_low: a pass over both halves is a training pass (trainable FFN weights, gradients enabled); "
                           f"{_LIRF_HINT}")
    pair = low_up_pair(low, up)
    pair.check_modes()
    return _LowUpFn.apply(pair.runner(), img, label, int(at_images), at_teacher, *params)


def __getattr__(name):      # vit_face.ViTs_face keeps resolving: the overlapping-patch model lives in vits_face.py (as in the reference)
    if name == "ViTs_face":
        from .vits_face import ViTs_face
        return ViTs_face
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
