"""ViTs-Face: ViT_face with an overlapping patch stage — MI355X-native drop-in for the reference
`vit_pytorch_face/vits_face.py` (ViTs_face :414-509).

The patch stage cuts nn.Unfold(ac_patch_size, stride=patch_size, padding=pad) windows (the reference driver: 12 x 12 at stride 8,
pad 4) and embeds each with one Linear of patch_dim = channels * ac_patch_size^2 inputs. Everything behind it — the transformer with
its FFN LoRA, the pooling and the CosFace / ArcFace / Softmax heads — is ViT_face's module tree and math, so the parameter names
are ViT_face's (`patch_to_embedding.weight` is [dim, patch_dim]) and a reference ViTs checkpoint loads strict. On the HIP path the
windows are gathered by gsl_unfold_patches into a K-padded operand of the same fused patch GEMM (gslora_hip.vit_runner).
"""
import os

import torch
import torch.nn as nn

from gslora_hip.ops import check_lora_rank, check_num_tokens, unfold_geometry

from .vit_face import DEFAULT_DTYPE, MIN_NUM_PATCHES, _HEADS, HipModelMixin, Transformer, ViT_face, compute_dtype_of


class ViTs_face(HipModelMixin, nn.Module):
    trainable_head = ViT_face.trainable_head      # the same heads, the same gradient kernel
    trainable_ffn = ViT_face.trainable_ffn        # ... and the same FFN linears under the same names

    def __init__(self, *, loss_type, GPU_ID, num_class, image_size, patch_size, ac_patch_size, pad, dim, depth, heads, mlp_dim,
                 pool="cls", channels=3, dim_head=64, dropout=0.0, emb_dropout=0.0, lora_rank=8):
        super().__init__()
        assert image_size % patch_size == 0, "Image dimensions must be divisible by the patch size."
        num_patches = (image_size // patch_size) ** 2
        patch_dim = channels * ac_patch_size ** 2
        assert num_patches > MIN_NUM_PATCHES, (
            f"your number of patches ({num_patches}) is way too small for attention to be effective (at least 16). "
            "Try decreasing your patch size")
        assert pool in {"cls", "mean"}, "pool type must be either cls (cls token) or mean (mean pooling)"
        if dim % 64 or mlp_dim % 64:
            raise NotImplementedError("gs-lora_amd GEMM tiles need dim and mlp_dim to be multiples of 64")
        if not 0 <= pad < ac_patch_size:
            raise ValueError(f"ViTs_face: the unfold padding must satisfy 0 <= pad < ac_patch_size, got pad {pad}, ac_patch_size {ac_patch_size}")
        lh, lw = unfold_geometry(image_size, image_size, ac_patch_size, patch_size, pad)
        if lh < 1 or lw < 1:
            raise ValueError(f"ViTs_face: a {ac_patch_size} x {ac_patch_size} window with pad {pad} does not fit a {image_size} px image")
        if lh * lw > num_patches:      # the reference fails in forward: pos_embedding[:, :n+1] has fewer rows than tokens
            raise ValueError(f"ViTs_face: nn.Unfold({ac_patch_size}, stride={patch_size}, padding={pad}) cuts {lh * lw} windows from a "
                             f"{image_size} px image, more than the {num_patches} rows of pos_embedding after the cls row")
        check_num_tokens("ViTs_face", lh * lw + 1)
        check_lora_rank("ViTs_face", lora_rank)
        self.patch_size = patch_size
        self.soft_split = nn.Unfold(kernel_size=(ac_patch_size, ac_patch_size), stride=(patch_size, patch_size), padding=(pad, pad))
        self.pos_embedding = nn.Parameter(torch.randn(1, num_patches + 1, dim))
        self.patch_to_embedding = nn.Linear(patch_dim, dim)
        self.cls_token = nn.Parameter(torch.randn(1, 1, dim))
        self.dropout = nn.Dropout(emb_dropout)
        self.transformer = Transformer(dim, depth, heads, dim_head, mlp_dim, dropout, lora_rank, lora_pos="FFN")
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
                "'SFaceLoss' while ViTs_face checks 'SFace'), and its forward returns a 6-tuple that the GS-LoRA engines cannot consume")
        else:
            raise NotImplementedError(f"gs-lora_amd implements the heads {sorted(_HEADS)}, not {loss_type}")
        # geometry consumed by the runner
        self.image_size, self.ac_patch_size, self.pad = image_size, ac_patch_size, pad
        self.dim, self.depth, self.heads, self.mlp_dim = dim, depth, heads, mlp_dim
        self.num_tokens = lh * lw + 1
        self.lora_rank = lora_rank
        self.lora_pos = "FFN"      # the reference's ViTs attention has no lora_pos: FFN adapters only
        self.attn_scale = dim ** -0.5
        self.dropout_p, self.emb_dropout_p = float(dropout), float(emb_dropout)
        self.set_compute_dtype(os.environ.get("GSLORA_DTYPE", DEFAULT_DTYPE))
        self._runner = None

    # ---- helpers for the runner (ViT_face's: the module tree behind the patch stage is the same) ----------------------------------
    blocks = ViT_face.blocks
    ffn_blocks = ViT_face.ffn_blocks

    def hip_spec(self):
        """ViT_face's spec with the unfold patch stage (see gslora_hip.vit_runner.ModelSpec)."""
        sp = ViT_face.hip_spec(self)
        sp.patch_kernel, sp.patch_stride, sp.patch_pad, sp.image_size = self.ac_patch_size, self.patch_size, self.pad, self.image_size
        return sp

    # ---- reference API ---------------------------------------------------------------------------
    def forward(self, img, label=None, mask=None):
        """:return: (logits, emb) if label is given else emb — as the reference (:489-509)."""
        if mask is not None:
            raise NotImplementedError("attention masks are never passed by the GS-LoRA engines")
        logits, emb = self._hip_call(img, label)
        return emb if label is None else (logits, emb)
