"""Whole-network forward/backward schedule of the ViT-Face + LoRA-FFN model on the HIP kernels.

This is the host-side "engine" behind vit_pytorch_face.ViT_face.forward: it owns
  * the flat f32 LoRA bucket (parameters become views into it, ordered group-by-group so that a
    group-lasso group is one contiguous slice),
  * the frozen-weight operand caches (bf16 casts / transposes, refreshed when a weight's
    (data_ptr, _version) changes, e.g. after loralib merge/un-merge or load_state_dict),
  * the per-forward activation stash that the hand-written backward consumes.
Reference semantics: vit_pytorch_face/vit_face.py:523-548 (forward), autograd of the same.
"""
import os
from types import SimpleNamespace

import torch

from . import _lib as L
from . import ops

PADK = 64                                  # LoRA K-segment width fed to the GEMM (r zero-padded to 64)
OP16 = (torch.bfloat16, torch.float16)     # the two operand formats of the speed mode ("bf16" / "fp16")
SITE_EMB = 1_000_000
# ---- numeric form of the bf16 speed mode: the three PRODUCT knobs (read once from the environment; module attributes, so a caller /
# tools/precision_ablation.py / the tests can also set them in-process). The f32 parity mode ignores them. README.md documents them.
# Residual-GRADIENT stream (the [M, dim] tensor every LayerNorm backward re-reads and re-writes) in bf16: -25 % of the bytes of each
# LayerNorm backward. GSLORA_GRAD_STREAM=f32 keeps it in f32.
GRAD_STREAM_BF16 = os.environ.get("GSLORA_GRAD_STREAM", "bf16").lower() != "f32"
# FORWARD residual stream x (read by every LayerNorm forward, read + written by the out-proj / FFN2 epilogues, re-read by every LayerNorm
# backward) in 2 bytes per element: f32 accumulate in the producing epilogue, one rounding on store. "f16" (default, round 4): IEEE fp16 —
# the stream is never a matrix-core operand, so it can spend its 16 bits on significand instead of exponent range: 8x finer rounding than
# bf16 at the same bytes (values clamp at +-65504; ViT residual streams are O(1 .. 100)); "bf16": round 3's form; "f32": 4 bytes
# (+9.7 GB per step). GSLORA_FWD_STREAM selects. profiles/r04_acc_stat.md has what each buys in trajectory fidelity.
FWD_STREAM = os.environ.get("GSLORA_FWD_STREAM", "f16").lower()
if FWD_STREAM not in ("f16", "bf16", "f32"):
    raise ValueError(f"GSLORA_FWD_STREAM must be f16, bf16 or f32, not {FWD_STREAM!r}")
# g' = GELU'(.) * dropmask / (1 - p) — written by the fused FFN1 epilogue, read once by the FFN2-dX epilogue — as an 8-bit fixed-point
# code (include/gslora_hip.h, GSL_EPI_BIAS_GELU_G8): half the bytes of one of the two [M, mlp] tensors of the FFN. GSLORA_GP8=0: bf16.
GP8 = os.environ.get("GSLORA_GP8", "1") != "0"

# ---- decided schedule choices (A/B'd in rounds 2 - 3, profiles/r03_notes.md). Plain constants: no environment reads; the tests that pin a
# form against the one it replaced (tests/test_hip_graph.py, tests/test_hip_model.py) patch the module attribute.
# The two [M, mlp] LoRA-gradient reductions of a block ride in the FFN2-dX epilogue (False: separate gsl_lora_grad launches).
FUSE_LORA_GRAD = True
# pool='cls' (vit_face.py:540): the head reads token 0 only and everything after a block's attention is token-wise, so in the LAST block
# only the cls query's attention output, its out-proj / LayerNorm / FFN rows are ever consumed — forward and backward of that block's
# tail run on B rows instead of B*T (exact: the skipped rows influence no output of the model). False keeps the dense forward (the
# backward then still runs on the cls rows).
TAIL_CLS = True
# ... and of that block's QKV projection only K and V are needed for every token: Q is projected for the cls rows alone (kv [M, 2*inner]
# + q_cls [B, inner]; the backward's dX GEMM contracts over 2*inner and the cls rows get their dQ term from a [B, inner] GEMM).
QSPLIT = True
# rows from which the LoRA down-projections are computed inside the 256x256 GEMM kernels (below: a separate N = 64 GEMM + a K segment
# on the small-tile kernels). Measured: profiles/r03_c_small_m.md.
INK_MIN_ROWS = 8192
# LayerNorm 1 folded into the QKV projection (16-bit modes whose forward stream has the operand format, i.e. the fp16 default): the GEMM reads
# the stream x itself with gamma folded into the weight and finishes the normalisation in its epilogue (EPI_STORE_LN); LayerNorm 1 shrinks to
# its row statistics (one read of x, no LN(x) tensor). GSLORA_LN1_FOLD=0: the LayerNorm kernel + plain GEMM of rounds 1 - 4.
LN1_FOLD = os.environ.get("GSLORA_LN1_FOLD", "1") != "0"
# fp16 operands: exponent of the loss-scaled backward — gsl_head_bwd picks the power of two S with S * max|head gradient| in [2^(E-1), 2^E)
# (0 = the library default 11: 32x headroom below 65504 at the head; the overflow guard lowers E on the device when a store saturates)
GRAD_TARGET_EXP = int(os.environ.get("GSLORA_GRAD_TARGET_EXP", "0"))
if GRAD_TARGET_EXP and not 4 <= GRAD_TARGET_EXP <= 15:
    raise ValueError(f"GSLORA_GRAD_TARGET_EXP={GRAD_TARGET_EXP}: 0 (default) or 4 .. 15")
INK_SMALL = True      # the in-kernel form on the small-tile kernel (few rows)
# The LoRA-gradient reductions of a backward pass that do not ride in the FFN2-dX epilogue are collected and issued as ONE batched pair of
# launches (gsl_lora_grad_batch) instead of two to three launches each; their operands stay alive until the end of the backward (or until
# the data-parallel hook needs the slice). Measured: few-shot 4+4 1.355 -> 1.155 ms (24 reductions, 48 launches before), ViT-B/16 48+48
# 11.01 -> 10.64 ms, 512+512 24.83 -> 24.69 ms (+1.2 GB of operands held). Row count above which the reductions run where their operands
# are produced instead (0 = always):
LGRAD_BATCH_MAX_ROWS = 1 << 30
# bf16 stream: the LayerNorm in front of the FFN can also emit the FFN1 adapter's down-projection u1 = s * LN(x) A1^T
# (gsl_layernorm_fwd_lora) instead of a skinny GEMM that re-reads LN(x). Measured time-neutral (profiles/r03_notes.md): off.
LN_LORA = False
# layout of the stashed qkv tensor in bf16 mode: head-major [B][H][3][T][64] (the QKV GEMM's store permutes, the attention kernels
# read contiguous per-head panels); False = token-major [B*T, 3*H*64] as the reference's to_qkv output (always used in f32 mode)
QKV_HEAD_MAJOR = True
# ... from this many tokens per image on: the permuting copy-out of the head-major store walks 8 rows at a step and may cross one image
# boundary in it (check_epilogue refuses STORE_QKV_HM below T = 8, csrc/gemm.hip); a shorter sequence takes the token-major layout
QKV_HM_MIN_T = 8


class BlockSpec:
    """One pre-norm transformer block as the kernels see it: x1 = x + drop(Wo attn(LN1 x) + bo), x2 = x1 + drop(W2' drop(gelu(W1' LN2 x1)))."""
    __slots__ = ("ln1", "qkv_w", "qkv_b", "out", "ln2", "l1", "l2", "qkv_lora")

    def __init__(self, ln1, qkv_w, qkv_b, out, ln2, l1, l2, qkv_lora=None):
        self.ln1, self.qkv_w, self.qkv_b, self.out, self.ln2, self.l1, self.l2 = ln1, qkv_w, qkv_b, out, ln2, l1, l2
        self.qkv_lora = qkv_lora      # loralib.MergedLinear with r > 0 (--lora_pos Attention): adapters on q / k / v instead of the FFN

    def lora_params(self):
        if self.qkv_lora is not None:
            return (self.qkv_lora.lora_A, self.qkv_lora.lora_B)
        return (self.l1.lora_A, self.l1.lora_B, self.l2.lora_A, self.l2.lora_B)


# head kinds that run the plain linear classifier of gsl_head_fwd / gsl_head_bwd (no normalisation, no margin)
LINEAR_HEADS = ("linear", "softmax")
# the kernels of gsl_gemm_nt_lora that hold the in-kernel LoRA form at few rows (ViTRunner.lora_in_kernel), and what the library's tile
# rule answered per (rows, N, K, dtype): a launch-bound step asks once per shape, not once per site
RING64_TILES = (L.TILE_RING64, L.TILE_RING64_WIDE, L.TILE_RING64_KSPLIT)
_RING_LORA = {}


class ModelSpec:
    """Geometry + parameter handles of one model family. Built by the model's `hip_spec()` on every forward (attribute
    look-ups only), so module surgery between calls — replace_ffn_with_lora, modify_head, load_state_dict — is picked up.
      ViT_face      (vit_pytorch_face/vit_face.py:449-548): Linear patch embedding, bias-free QKV, LN eps 1e-5,
                    scale dim^-0.5, margin head chosen by loss_type: "cosface" (s 64, m 0.35), "arcface" (s 64, m 0.5,
                    easy_margin; reference :72-143) — cos_s / cos_m are the head's s and m — or "softmax" (nn.Linear with bias,
                    reference :14-52: logits only when a label is passed, the label itself is ignored).
      ModifiedViT   (vit_pytorch_face/modified_VIT.py:5-45 over torchvision vit_b_16): conv16 patch embedding, QKV bias,
                    LN eps 1e-6, scale head_dim^-0.5, nn.Linear head with bias, the label argument is ignored.
      ViTs_face     (vit_pytorch_face/vits_face.py, reference vits_face.py:414-509): ViT_face with an overlapping patch stage —
                    nn.Unfold(patch_kernel, patch_stride, patch_pad) windows (gsl_unfold_patches) into the same Linear embedding, whose
                    weight is zero-padded along K to a multiple of 64; num_tokens = 1 + the number of windows.
      ViT_face_low / ViT_face_up (vit_pytorch_face/vit_face.py, reference :551-781), the two halves of a ViT_face for the LIRF baseline:
                    the lower half ends in the stream (stream_out: no final LayerNorm, no head), the upper half starts from one
                    (stream_in: no patch stage; block0 = the network-wide index of its first block, which the dropout sites keep). A
                    training pass runs both as ONE spec — patch stage and lower blocks of the student, upper blocks and head of the
                    upper module — with boundary = the index of the first upper block, whose saved input is the mid stream."""
    __slots__ = ("patch_size", "num_tokens", "dim", "heads", "attn_scale", "ln_eps", "dropout_p", "emb_dropout_p", "lora_rank",
                 "patch_w", "patch_is_conv", "patch_b", "cls", "pos", "blocks", "final_ln", "head_kind", "head_w", "head_b",
                 "cos_s", "cos_m", "easy_margin", "lora_site", "pool", "patch_kernel", "patch_stride", "patch_pad", "image_size",
                 "block0", "stream_in", "stream_out", "boundary", "dropout_p_up")

    def __init__(self, **kw):
        kw.setdefault("easy_margin", False)    # ArcFace only
        kw.setdefault("patch_kernel", 0)       # > 0: overlapping unfold windows of this size (ViTs_face); 0: gsl_patchify's p x p tiles
        kw.setdefault("patch_stride", 0)       # (the unfold's stride and zero padding)
        kw.setdefault("patch_pad", 0)
        kw.setdefault("image_size", None)      # (checked against the input on the unfold path)
        kw.setdefault("lora_site", "ffn")      # "ffn" (GS-LoRA) or "attention" (--lora_pos Attention ablation)
        kw.setdefault("pool", "cls")           # "cls" (token 0) or "mean" (mean over the tokens, vit_face.py:540)
        kw.setdefault("block0", 0)             # network-wide index of blocks[0] (ViT_face_up: depth // 2)
        kw.setdefault("stream_in", False)      # the input is the [B, T, D] stream in front of blocks[0], not images
        kw.setdefault("stream_out", False)     # the output is the stream behind the last block: no final LayerNorm, no head
        kw.setdefault("boundary", None)        # a lower + upper pair: index of the first upper block
        kw.setdefault("dropout_p_up", None)    # .. and the dropout rate in force in the upper blocks (the upper module's own mode decides it)
        for k in self.__slots__:
            setattr(self, k, kw[k])


class LoraBucket:
    """Flat storage for the trainable LoRA tensors of one model."""

    def __init__(self, layers):
        # layers: list of (A1, B1, A2, B2) nn.Parameters per transformer block
        self.params = [p for grp in layers for p in grp]
        self.groups = [i for i, grp in enumerate(layers) for _ in grp]
        dev = self.params[0].device
        n = sum(p.numel() for p in self.params)
        self.flat = torch.empty(n, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(n, device=dev, dtype=torch.float32)
        self.offsets = []
        off = 0
        with torch.no_grad():
            for p in self.params:
                k = p.numel()
                self.flat[off:off + k].copy_(p.detach().reshape(-1))
                p.data = self.flat[off:off + k].view(p.shape)
                self.offsets.append(off)
                off += k
        self.grad_views = [self.grad[o:o + p.numel()].view(p.shape) for o, p in zip(self.offsets, self.params)]
        self.toff = torch.tensor(self.offsets, device=dev, dtype=torch.int64)
        self.tnumel = torch.tensor([p.numel() for p in self.params], device=dev, dtype=torch.int64)
        self.tgroup_block = torch.tensor(self.groups, device=dev, dtype=torch.int32)
        self.ngroups_block = len(layers)
        self.per_layer = len(layers[0])
        self._gtables = {}

    def valid(self):
        base = self.flat.data_ptr()
        return all(p.data_ptr() == base + 4 * o for p, o in zip(self.params, self.offsets))

    def group_table(self, group_type="block"):
        """tensor->group ids for engine.get_structure_loss groupings (engine.py:585-650)."""
        L_ = self.ngroups_block
        if group_type == "block" or self.per_layer != 4:      # attention adapters: always one (A, B) group per block (engine.py:651-656)
            return self.tgroup_block, L_
        if group_type in self._gtables:
            return self._gtables[group_type]
        ids = []
        for i in range(L_):
            if group_type == "lora":
                ids += [i, i, L_ + i, L_ + i]
            elif group_type == "matrix":
                ids += [i, L_ + i, 2 * L_ + i, 3 * L_ + i]
            else:
                raise ValueError(f"unknown group type {group_type}")
        n = 2 * L_ if group_type == "lora" else 4 * L_
        self._gtables[group_type] = (torch.tensor(ids, device=self.flat.device, dtype=torch.int32), n)
        return self._gtables[group_type]

    def attach_grads(self):
        """Give every LoRA parameter its view of the flat gradient bucket. Returns True when the
        bucket had to be (re)attached, i.e. this is the first backward since zero_grad()."""
        fresh = False
        for p, g in zip(self.params, self.grad_views):
            if p.grad is None or p.grad.data_ptr() != g.data_ptr():
                fresh = True
                break
        if fresh:
            self.grad.zero_()
            for p, g in zip(self.params, self.grad_views):
                p.grad = g
        return fresh


def _res_epilogue(dtype):
    """The GEMM epilogue out = res + drop(acc + bias), by the dtype of the stream that res and out share."""
    return {torch.bfloat16: L.EPI_BIAS_RES_BF16, torch.float16: L.EPI_BIAS_RES_F16}.get(dtype, L.EPI_BIAS_RES_F32)


class _Pass:
    """What every step of one pass reads, computed once by the forward; the backward of the same pass goes on with it (`saved["ctx"]`)
    and adds its own state: the loss scale and its overflow guard, the gradient views, the deferred LoRA-gradient reductions."""
    __slots__ = ("sp", "dt", "xdt", "epi_res", "epi_patch", "B", "T", "D", "H", "M", "dev", "seed", "sflag", "p_drop", "p_emb", "r",
                 "attn_site", "s_lora", "eps", "save", "gscale", "gmax", "gv", "pending", "f32_mode", "ffn_train", "wg_ws", "wgrads", "p_up", "kb")

    def __init__(self, sp, dt, B, dev, training, seed, sflag, save, f32_mode=None):
        self.sp, self.dt, self.dev, self.seed, self.sflag, self.save = sp, dt, dev, seed, sflag, save
        self.ffn_train = False      # the FFN weights train (save="ffn"): the backward forms their gradients with gst_wgrad, see ViTRunner.backward
        self.f32_mode = f32_mode if dt == torch.float32 else None      # "x3" (the 'fp32x3' mode): every GEMM of the pass multiplies on the bf16 matrix cores
        self.B, self.T, self.D, self.H, self.M = B, sp.num_tokens, sp.dim, sp.heads, B * sp.num_tokens
        self.p_drop = sp.dropout_p if training else 0.0
        self.p_emb = sp.emb_dropout_p if training else 0.0
        self.p_up, self.kb = sp.dropout_p_up, sp.boundary      # a lower + upper pair: blocks kb .. drop at the upper module's rate, see pd()
        self.r, self.eps = sp.lora_rank, sp.ln_eps
        self.attn_site = self.r > 0 and sp.lora_site == "attention"
        self.s_lora = (1.0 / self.r) if self.r > 0 else 0.0
        xbf = dt in OP16 and FWD_STREAM != "f32"        # the residual stream in 2 bytes per element
        xf16 = xbf and (FWD_STREAM == "f16" or dt == torch.float16)      # (fp16 operands: the 16-bit stream is fp16 too)
        self.xdt = (torch.float16 if xf16 else torch.bfloat16) if xbf else torch.float32            # dtype of the residual stream
        self.epi_res = _res_epilogue(self.xdt)
        self.epi_patch = (L.EPI_PATCH_F16 if xf16 else L.EPI_PATCH_BF16) if xbf else L.EPI_PATCH

    def pd(self, i):
        """The dropout rate of block i's three sites."""
        return self.p_drop if (self.p_up is None or i < self.kb) else self.p_up

    def gemm(self, *a, **kw):
        """ops.gemm_nt in the pass's GEMM mode: every GEMM of the forward and the backward goes through here. (Attention, LayerNorm, head, losses,
        LoRA-gradient reductions and AdamW have no such mode: in 'fp32x3' they are the f32 kernels of 'fp32'.)"""
        return ops.gemm_nt(*a, f32_mode=self.f32_mode, **kw)


def _ffn_requires_grad(blk):
    return any(p.requires_grad for lin in (blk.l1, blk.l2) for p in (lin.weight, lin.bias))


def _cls_rows(c, t, w):
    """Rows b*T of a [B*T, w] tensor."""
    return t.view(c.B, c.T, w)[:, 0].contiguous()


def _gp_rows(c, t, w):
    """The cls rows of g'. (The 8-bit GELU' code tensor is slab-major [w/64][rows][64]: its cls rows, again slab-major for B rows.)"""
    return t.view(w // 64, c.B, c.T, 64)[:, :, 0].contiguous().view(c.B, w) if t.dtype == torch.uint8 else _cls_rows(c, t, w)


class ViTRunner:
    def __init__(self, model):
        self.model = model
        self.bucket = None
        self._wcache = {}
        self._lcache = {}
        self._packs, self._pack_tables, self._retired = {}, {}, []
        self._u8tab = None        # ((mean, std), device) -> the [C, 256] value table of uint8 inputs (input_table)
        self._rank = 0
        self.seed_dev = None      # int64 [1] device tensor: dropout seed of a step that is being captured / replayed as a HIP graph
        # dropout stream: torch.manual_seed() selects it (like the reference's nn.Dropout), and every data-parallel rank draws its own
        self.drop_seed = self._initial_drop_seed()
        self.drop_calls = 0
        self.grad_hook = None     # callable(layer) invoked when the LoRA gradients of `layer` are complete (data-parallel overlap, step.py)
        # fp16 operands: {S, 1/S, largest scaled gradient the LayerNorm backwards of the last backward saw, exponent in use} — device-resident
        # state of the loss scale and its overflow guard (gsl_head_bwd); persists across steps and HIP-graph replays
        self.gscale = None
        self._guard_on = False

    def __deepcopy__(self, memo):   # copies of the model build their own runner lazily
        return None

    def _loss_scale_state(self, device):
        if self.gscale is None or self.gscale.device != device:
            self.gscale = torch.zeros(4, device=device, dtype=torch.float32)
        return self.gscale

    def overflow_guard(self):
        """The device float FusedAdamW checks before it updates (None unless the last backward ran on loss-scaled fp16 gradients)."""
        return self.gscale[2:] if (self._guard_on and self.gscale is not None) else None

    def loss_scale_report(self):
        """Host read (one sync) of the loss-scale state after a backward: S, the exponent in use, the largest scaled gradient the LayerNorm
        backwards saw and the headroom 65504 / that (< = 1: a 16-bit store saturated, the optimizer skipped the step)."""
        if self.gscale is None:
            return None
        S, _, seen, E = self.gscale.tolist()
        return {"S": S, "exponent": int(E), "seen_max": seen, "headroom": (65504.0 / seen) if seen > 0 else float("inf"), "saturated": not seen < 65504.0}

    @staticmethod
    def _initial_drop_seed():
        import torch.distributed as dist
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        z = (torch.initial_seed() * 0x9E3779B97F4A7C15 + (rank + 1) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z ^= z >> 31
        return int(z & 0x7FFFFFFFFFF)      # 43 bits: (seed << 20) + call counter stays below 2^63

    # ------------------------------------------------------------------ caches
    def _cached(self, cache, key, params, fn):
        """fn(*params, detached), rebuilt when the (data_ptr, _version, device) of one of them changes. params: a tensor or a tuple of them."""
        ps = params if isinstance(params, tuple) else (params,)
        ent = cache.get(key)
        tag = tuple((p.data_ptr(), p._version, p.device) for p in ps)
        if ent is None or ent[0] != tag:
            with torch.no_grad():
                ent = cache[key] = (tag, fn(*(p.detach() for p in ps)))
        return ent[1]

    def invalidate_operand_caches(self):
        """Forget every cached operand-format copy of a frozen weight (they are rebuilt on the next forward). Captured HIP graphs hold the old
        copies' addresses: the graph stepper re-captures when the parameter versions it recorded change; after a `.data` write bump them too
        or drop the graphs (GraphedStep.graphs.clear())."""
        self._wcache = {k: v for k, v in self._wcache.items() if k and k[0] == "zeros"}
        self._lcache.clear()

    def input_table(self, norm, channels, device):
        """Device copy of the [C, 256] value table of the model's input normalisation (ops.u8_norm_table), cached on (mean, std) and the
        device alone. A replaced table is retired, not freed: a captured HIP graph may still read it."""
        ent = self._u8tab
        if ent is None or ent[0] != (norm, device):
            if len(norm[0]) != channels:
                raise ValueError(f"{type(self.model).__name__}: set_input_norm() was given {len(norm[0])} channels, the images have {channels}")
            if ent is not None:
                self._retired.append(ent[1])
            ent = self._u8tab = ((norm, device), ops.u8_norm_table(*norm).to(device))
        if ent[1].shape[0] != channels:
            raise ValueError(f"{type(self.model).__name__}: set_input_norm() was given {ent[1].shape[0]} channels, the images have {channels}")
        return ent[1]

    def w(self, name, param, dtype):
        """[N,K] operand in compute dtype."""
        if dtype == torch.float32:
            return param.detach()
        return self._cached(self._wcache, (name, "n", dtype), param, lambda p: ops.cast(p.contiguous(), dtype))

    def w_ln(self, name, weight, gamma, beta, bias, dtype):
        """Operands of a GEMM with a consumer-side LayerNorm in front (EPI_STORE_LN): W' = W * gamma along K in the operand format,
        c = rowsum(W') of the ROUNDED W' (so that the mean term cancels against what the matrix cores actually multiply), d = W beta (+ bias).
        Cached on the four parameters' versions (all frozen in GS-LoRA: built once)."""
        def build(weight, gamma, beta, bias=None):
            w32 = weight.float()
            wf = ops.cast((w32 * gamma.float()[None, :]).contiguous(), dtype)
            c = wf.float().sum(1).contiguous()
            d = (w32 @ beta.float()) + (bias.float() if bias is not None else 0.0)
            return wf, c, d.contiguous()
        return self._cached(self._wcache, (name, "ln", dtype), (weight, gamma, beta) + (() if bias is None else (bias,)), build)

    def w_conv(self, name, param, dtype):
        """conv_proj weight [D, C, p, p] as the [D, p*p*C] operand matching gsl_patchify's (p1 p2 c) feature order."""
        def build(p):
            w2 = p.permute(0, 2, 3, 1).reshape(p.shape[0], -1).contiguous()
            return w2 if dtype == torch.float32 else ops.cast(w2, dtype)
        return self._cached(self._wcache, (name, "conv", dtype), param, build)

    def w_kpad(self, name, param, kpad, dtype):
        """[D, K] weight zero-padded to [D, kpad] (the patch GEMM of the unfold path: K = C*k*k need not be a multiple of 64)."""
        def build(p):
            w2 = torch.zeros(p.shape[0], kpad, device=p.device, dtype=torch.float32)
            w2[:, :p.shape[1]] = p
            return w2 if dtype == torch.float32 else ops.cast(w2, dtype)
        return self._cached(self._wcache, (name, "kpad", kpad, dtype), param, build)

    def wT(self, name, param, dtype):
        """[K,N] transposed operand (dX GEMMs)."""
        return self._cached(self._wcache, (name, "t", dtype), param, lambda p: ops.transpose_cast(p.contiguous(), dtype))

    PACK_GEOM = {   # kind -> (si, sj, rows, cols, rows_out, ld_out) of gsl_pack_pad as functions of the LoRA tensor's (rows, cols, r)
        "A_rows": lambda R, C, r: (C, 1, r, C, PADK, C),        # [64, K]  rows j<r = A[j,:]
        "B_cols": lambda R, C, r: (r, 1, R, r, R, PADK),        # [N, 64]  cols j<r = B[:,j]
        "BT_rows": lambda R, C, r: (1, r, r, R, PADK, R),       # [64, N]  out[j, n] = B[n, j]
        "AT_cols": lambda R, C, r: (1, C, C, r, C, PADK),       # [K, 64]  out[k, j] = A[j, k]
        # operands of the in-kernel LoRA GEMM (gsl_gemm_nt_lora): P [16, K], Q [N, 32]
        "A_rows16": lambda R, C, r: (C, 1, r, C, 16, C),
        "B_cols32": lambda R, C, r: (r, 1, R, r, R, 32),
        "BT_rows16": lambda R, C, r: (1, r, r, R, 16, R),
        "AT_cols32": lambda R, C, r: (1, C, C, r, C, 32),
    }

    def lora_pack(self, name, param, kind, dtype):
        """Padded / transposed compute-dtype copy of one LoRA tensor. The output buffers are persistent and registered in a device
        descriptor table: after the first step, refresh_lora_packs() rebuilds ALL of them with one launch per step."""
        key = (name, kind, dtype)
        ent = self._packs.get(key)
        if ent is None or ent["ptr"] != param.data_ptr() or ent["dev"] != param.device:
            rows, cols = param.shape
            rank = rows if kind.startswith("A") else cols      # lora_A is [r, in], lora_B is [out, r] (min(rows, cols) is wrong where r > dim)
            si, sj, pr, pc, ro, ld = self.PACK_GEOM[kind](rows, cols, rank)
            out = torch.empty(ro, ld, device=param.device, dtype=dtype)
            ent = dict(ptr=param.data_ptr(), dev=param.device, param=param, out=out, geom=(si, sj, pr, pc), version=None)
            self._packs[key] = ent
            self._pack_tables.pop(dtype, None)
        if ent["version"] != param._version:
            with torch.no_grad():
                ops.pack_pad(param, *ent["geom"], *ent["out"].shape, dtype, out=ent["out"])
            ent["version"] = param._version
        return ent["out"]

    def qkv_lora_ops(self, i, ml, dtype):
        """Operands of the three q / k / v adapters of one MergedLinear, as ONE LoRA K segment (r3 = 3r <= 64 live columns), under the
        K-segment kinds of LORA_KINDS:
          A_rows  [64, dim]      rows g*r+j = A_g[j, :]                       (u = s * xn A_all^T)
          B_cols  [3*inner, 64]  row g*inner+n, column g*r+j = B_g[n, j]      (qkv += u Bblk^T: block diagonal)
          BT_rows [64, 3*inner]                                                (v = s * dqkv Bblk)
          AT_cols [dim, 64]      column g*r+j = A_g[j, :]                      (dxn1 += v A_all)"""
        r, ng = ml.r, len(ml.enable_lora)
        if ng * r > PADK:
            raise NotImplementedError("gs-lora_amd: 3 * lora_rank must not exceed 64 for --lora_pos Attention")

        def build(A, B):
            inner = B.shape[0] // ng
            a_rows = torch.zeros(PADK, A.shape[1], device=A.device, dtype=torch.float32)
            a_rows[:ng * r] = A
            bblk = torch.zeros(B.shape[0], PADK, device=A.device, dtype=torch.float32)
            for g in range(ng):
                bblk[g * inner:(g + 1) * inner, g * r:(g + 1) * r] = B[g * inner:(g + 1) * inner]
            cast = (lambda t: t.contiguous()) if dtype == torch.float32 else (lambda t: ops.cast(t.contiguous(), dtype))
            return dict(A_rows=cast(a_rows), B_cols=cast(bblk), BT_rows=cast(bblk.t()), AT_cols=cast(a_rows.t()))
        return self._cached(self._lcache, (f"qkvlora{i}", dtype), (ml.lora_A, ml.lora_B), build)

    def refresh_lora_packs(self, dtype):
        """One launch for every registered pack whose source changed (the optimizer touches all LoRA tensors each step)."""
        ents = [e for k, e in self._packs.items() if k[2] == dtype]
        if len(ents) < 2 or all(e["version"] == e["param"]._version for e in ents):
            return
        tab = self._pack_tables.get(dtype)
        if tab is None or tab[2] != len(ents):
            if torch.cuda.is_current_stream_capturing():
                return      # no H2D copy inside a capture: lora_pack() refreshes tensor by tensor (build_pack_tables() avoids this)
            tab = self.build_pack_tables(dtype)
        ops.pack_pad_batch(tab[0], tab[2], tab[1], dtype)
        for e in ents:
            e["version"] = e["param"]._version

    def build_pack_tables(self, dtype):
        """Device descriptor table of every registered pack of `dtype` (called at the end of an eager backward, so that a following
        HIP-graph capture finds it ready)."""
        ents = [e for k, e in self._packs.items() if k[2] == dtype]
        tab = self._pack_tables.get(dtype)
        if ents and (tab is None or tab[2] != len(ents)):
            if tab is not None:
                self._retired.append(tab[0])      # a captured HIP graph may still launch with the old table: never free it
            t, mx = ops.pack_desc_table([(e["param"], *e["geom"], 1.0, e["out"]) for e in ents], ents[0]["dev"])
            tab = self._pack_tables[dtype] = (t, mx, len(ents))
        return tab

    def _zeros(self, n, dev):
        z = self._wcache.get(("zeros", n, dev))
        if z is None:
            z = self._wcache[("zeros", n, dev)] = torch.zeros(n, device=dev, dtype=torch.float32)
        return z

    def lora_in_kernel(self, dtype, rows, N, K):
        """The bf16 wide GEMMs compute the LoRA down-projection inside the kernel (no extra pass over the activation): on the 256x256
        8-phase kernel from INK_MIN_ROWS rows on, and on the 64x64 ring kernel wherever gsl_gemm_nt_lora picks it (few rows: the
        launch-bound regime, where the separate skinny GEMM is a 6 - 12 us launch per adapted layer and direction). In between, the
        N = 512 GEMMs would run the 8-phase kernel on a handful of workgroups and the two-launch K-segment form wins. Which kernel
        gsl_gemm_nt_lora picks is the library's tile rule (csrc/gemm.hip), asked once per shape."""
        if dtype not in OP16 or self._rank > 16:
            return False
        if rows >= INK_MIN_ROWS:
            return True
        if not INK_SMALL:
            return False
        key = (rows, N, K, dtype)
        if key not in _RING_LORA:
            _RING_LORA[key] = ops.gemm_tile_choice(rows, N, K, dtype, in_kernel_lora=True) in RING64_TILES
        return _RING_LORA[key]

    # ------------------------------------------------------------------ the adapted linear layer
    # out = epilogue(a W^T + s (a P^T) Q^T): PACK_GEOM kinds of (P, Q) by direction and form. Forward: P from lora_A, Q from lora_B; dX
    # (a = dY, W = the transposed weight): P from lora_B, Q from lora_A. "kseg": a skinny GEMM writes u = s a P^T [rows, 64] and the
    # wide GEMM takes (u, Q) as a second K segment; "ink": gsl_gemm_nt_lora forms u inside the wide GEMM (P [16, K], Q [N, 32]).
    LORA_KINDS = {("fwd", "kseg"): ("A_rows", "B_cols"), ("fwd", "ink"): ("A_rows16", "B_cols32"),
                  ("dx", "kseg"): ("BT_rows", "AT_cols"), ("dx", "ink"): ("BT_rows16", "AT_cols32")}

    def ffn_packs(self, i, n, layer, dtype):
        """kind -> the packed operand of the adapter of FFN layer n (1 / 2) of block i."""
        return lambda kind: self.lora_pack(f"{kind[0]}{n}_{i}", layer.lora_A if kind[0] == "A" else layer.lora_B, kind, dtype)

    def _lora_project(self, c, a, pack, direction, N, *, in_kernel_ok=True, u=None, compact=False):
        """First half of one adapted linear layer: the form, the [rows, 64] down-projection u and, in the K-segment form, the skinny
        GEMM that fills it. pack: kind -> operand (ffn_packs, the q / k / v adapters' table), None: no live adapter, a plain GEMM follows.
        in_kernel_ok=False keeps the K-segment form whatever lora_in_kernel says; u: the projection from another producer
        (gsl_layernorm_fwd_lora); compact: the skinny GEMM also writes u's first 16 columns as [rows, 16] (step.uc).
        -> the step for _lora_finish; step.u is the projection for the stash and the reductions (in-kernel form: filled by _lora_finish)."""
        st = SimpleNamespace(a=a, pack=pack, u=u, uc=None, ink=False, kinds=None)
        if pack is None:
            return st
        rows, K = a.shape
        st.ink = in_kernel_ok and u is None and self.lora_in_kernel(c.dt, rows, N, K)
        st.kinds = self.LORA_KINDS[direction, "ink" if st.ink else "kseg"]
        if u is None:
            st.u = torch.empty(rows, PADK, device=c.dev, dtype=c.dt)
            if not st.ink:
                if compact:
                    st.uc = torch.empty(rows, 16, device=c.dev, dtype=c.dt)
                c.gemm(a, pack(st.kinds[0]), st.u, alpha=c.s_lora, out2=st.uc)
        return st

    def _lora_finish(self, c, st, w, out, kw, mulgrad=None):
        """Second half: the wide GEMM into `out`; kw: its epilogue and the epilogue's operands (a dict, handed on once: this runs per adapted
        layer of a launch-bound step). mulgrad (in-kernel form only): the operands of the gradient-fused epilogue of
        gsl_gemm_nt_lora_mulgrad behind `out` (aux, U1, G1, g1s, Y2, G2, g2s, r). -> out"""
        if st.pack is None:
            return c.gemm(st.a, w, out, **kw)
        if st.ink:
            P, Q = st.pack(st.kinds[0]), st.pack(st.kinds[1])
            if mulgrad is not None:
                return ops.gemm_nt_lora_mulgrad(st.a, w, P, Q, c.s_lora, st.u, out, *mulgrad, **kw)
            return ops.gemm_nt_lora(st.a, w, P, Q, c.s_lora, st.u, out, **kw)
        return c.gemm(st.a, w, out, A2=st.u, W2=st.pack(st.kinds[1]), **kw)

    def ensure_bucket(self, spec=None):
        spec = spec or self.model.hip_spec()
        self._rank = spec.lora_rank
        if spec.lora_rank <= 0:
            return None
        layers = [blk.lora_params() for blk in spec.blocks]
        if self.bucket is None or not self.bucket.valid() or any(a is not b for a, b in zip(self.bucket.params, (p for g in layers for p in g))):
            self.bucket = LoraBucket(layers)
            self._lcache.clear()
            self._retired.extend(t[0] for t in self._pack_tables.values())
            self._retired.extend(e["out"] for e in self._packs.values())
            self._packs.clear()
            self._pack_tables.clear()
        return self.bucket

    # ------------------------------------------------------------------ forward
    def forward(self, img, label, save):
        """img: [B, C, H, W], or a tuple of such batches that are processed as ONE batch (gs_lora_step hands over the remain and the
        forget batch this way: each is patchified into its row range of the token matrix, no concatenated image copy is made)."""
        head_only = save == "head"      # only the head's parameters train: nothing of the blocks is kept (see head_param_grads)
        ffn_train = save == "ffn"       # the FFN weights (and possibly the head) train, no LoRA in the model: everything is kept
        save = save is True or ffn_train
        c, parts, u8tab, label = self._fwd_prepare(img, label, save)
        c.ffn_train = ffn_train
        sp = c.sp
        x = self._fwd_stream_in(c, parts[0]) if sp.stream_in else self._fwd_patch(c, parts, u8tab)
        stash = []
        for i, blk in enumerate(sp.blocks):
            # (a lower half hands every token on: its last block is never the cls-row-only one)
            tail = TAIL_CLS and i == len(sp.blocks) - 1 and sp.pool == "cls" and not sp.stream_out
            xn, mean1, rstd1 = self._fwd_ln1(c, blk, x)
            qkv, q_cls, uq, hm = self._fwd_qkv(c, i, blk, x, xn, mean1, rstd1, tail)
            xn_keep = xn if (c.attn_site and save) else None
            del xn
            o, lse, x1 = self._fwd_attention(c, i, blk, x, qkv, q_cls, hm, tail)
            x2, st = self._fwd_ffn(c, i, blk, x1)
            if save:
                st.update(x=x, mean1=mean1, rstd1=rstd1, qkv=qkv, qkv_hm=hm, o=o, lse=lse, x1=x1, xn=xn_keep, uq=uq, tail=tail, q_cls=q_cls)
                stash.append(st)
            x = x2
        if sp.stream_out:
            if save or head_only:
                raise RuntimeError(f"{type(self.model).__name__}: a lower half network keeps nothing for a backward of its own; a training pass "
                                   "runs it together with the upper half (gslora_hip.step.lirf_step)")
            return None, x.view(c.B, c.T, c.D), None
        logits, emb, head = self._fwd_head(c, x, label)
        if head_only:
            return logits, emb, dict(ctx=c, emb=emb, label=label, cos_y=head["cos_y"])
        return logits, emb, (dict(ctx=c, layers=stash, x_last=x, emb=emb, label=label, **head) if save else None)

    def _fwd_prepare(self, img, label, save):
        """Input validation, the uint8 / float decision with its value table, the dropout seed and the LoRA state of this pass.
        -> (pass context, image batches, value table or None, label as the head wants it)"""
        m = self.model
        if getattr(m, "stream_in", False):      # ViT_face_up
            return self._fwd_prepare_stream(img, label, save)
        raw = list(img) if isinstance(img, (tuple, list)) else [img]
        # uint8 batches of a model that was told how to normalise them (set_input_norm) stay bytes up to the patch gather, which looks
        # ToTensor() + Normalize() up in a [C, 256] table; any other input is a value cast, as the reference's inputs.float()
        norm = getattr(m, "input_norm", None)
        u8 = norm is not None and all(t.dtype == torch.uint8 for t in raw)
        if norm is not None and not u8 and any(t.dtype == torch.uint8 for t in raw):
            raise ValueError(f"{type(m).__name__}: the batches of one forward must be all uint8 or all float once set_input_norm() is in effect")
        parts = raw if u8 else [t.float().contiguous() for t in raw]
        img = parts[0]
        if not all(t.is_cuda for t in parts):
            raise RuntimeError(f"{type(m).__name__} (gs-lora_amd): the model runs only on a ROCm GPU through libgslora_hip.so; "
                               "there is no CPU fallback. Move the model and inputs to 'cuda'.")
        if any(t.shape[1:] != img.shape[1:] for t in parts):
            raise ValueError("the batches of one forward must share the image shape")
        L.load()
        sp = m.hip_spec()
        u8tab = self.input_table(norm, img.shape[1], img.device) if u8 else None
        if sp.head_kind == "linear":
            label = None                       # modified_VIT.py:23-24: "label is not used in this model"
        elif label is not None:
            label = label.to(device=img.device, dtype=torch.int64).contiguous()
        self.drop_calls += 1
        if self.seed_dev is not None:      # HIP-graph mode: the kernels read the seed from device memory; one captured increment per forward
            self.seed_dev.add_(1)
            seed, sflag = self.seed_dev.data_ptr(), L.SEED_ON_DEVICE
        else:
            seed, sflag = (self.drop_seed << 20) + self.drop_calls, 0
        c = _Pass(sp, m.compute_dtype, sum(t.shape[0] for t in parts), img.device, m.training, seed, sflag, save, getattr(m, "gemm_mode", None))
        self.ensure_bucket(sp)
        if c.r > 0 and not c.attn_site:
            self.refresh_lora_packs(c.dt)
        return c, parts, u8tab, label

    def _fwd_prepare_stream(self, x, label, save):
        """_fwd_prepare of an upper half network: the input is the [B, T, D] stream of the lower half."""
        m = self.model
        sp = m.hip_spec()
        if not (torch.is_tensor(x) and x.dim() == 3 and tuple(x.shape[1:]) == (sp.num_tokens, sp.dim)
                and x.dtype in (torch.float32, torch.float16, torch.bfloat16)):
            raise ValueError(f"{type(m).__name__}: the input is the lower half's stream [B, {sp.num_tokens}, {sp.dim}] (f32 or a 16-bit stream), got "
                             f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        if not x.is_cuda:
            raise RuntimeError(f"{type(m).__name__} (gs-lora_amd): the model runs only on a ROCm GPU through libgslora_hip.so; "
                               "there is no CPU fallback. Move the model and inputs to 'cuda'.")
        L.load()
        if label is not None:
            label = label.to(device=x.device, dtype=torch.int64).contiguous()
        self.drop_calls += 1
        seed, sflag = (self.drop_seed << 20) + self.drop_calls, 0
        c = _Pass(sp, m.compute_dtype, x.shape[0], x.device, m.training, seed, sflag, save, getattr(m, "gemm_mode", None))
        self.ensure_bucket(sp)
        return c, [x], None, label

    def _fwd_stream_in(self, c, x):
        """The stream an upper half starts from, [M, D] in the pass's stream dtype (a copy only where the dtype or the layout differs)."""
        return x.detach().to(c.xdt).contiguous().view(c.M, c.D)

    def _fwd_patch(self, c, parts, u8tab):
        """Patch stage: the patch gather (tiles, or ViTs_face's overlapping windows) and the embedding GEMM whose epilogue adds bias and
        position, writes the cls rows and applies the embedding dropout. -> the residual stream x [M, D]"""
        sp, dt, img = c.sp, c.dt, parts[0]
        if sp.patch_kernel:      # ViTs_face: overlapping zero-padded windows, K padded to a multiple of 64 (weight and patches alike)
            if sp.image_size is not None and tuple(img.shape[2:]) != (sp.image_size, sp.image_size):
                raise ValueError(f"{type(self.model).__name__}: input images are {tuple(img.shape[2:])}, the model was built for "
                                 f"{sp.image_size} x {sp.image_size}")
            patches = ops.unfold_patches(parts, sp.patch_kernel, sp.patch_stride, sp.patch_pad, dt, table=u8tab)
            if patches.shape[0] != c.M:
                raise ValueError(f"{type(self.model).__name__}: the unfold yields {patches.shape[0] // c.B} tokens per image, the model has {c.T}")
            pw = self.w_kpad("pe", sp.patch_w, patches.shape[1], dt)
        else:
            patches = ops.patchify(parts, sp.patch_size, dt, table=u8tab)
            pw = self.w_conv("pe", sp.patch_w, dt) if sp.patch_is_conv else self.w("pe", sp.patch_w, dt)
        x = torch.empty(c.M, c.D, device=c.dev, dtype=c.xdt)
        c.gemm(patches, pw, x, epilogue=c.epi_patch, bias=sp.patch_b.detach(), pos=sp.pos.detach()[0, :c.T].contiguous(),
                    cls=sp.cls.detach().reshape(-1), T=c.T, p_drop=c.p_emb, seed=c.seed, site=SITE_EMB | c.sflag)
        return x

    def _fwd_ln1(self, c, blk, x):
        """LayerNorm 1 -> (xn, mean, rstd); xn is None when the normalisation is folded into the QKV projection (LN1_FOLD)."""
        n1 = blk.ln1
        attn_lora_live = c.attn_site and not blk.qkv_lora.merged      # the q / k / v adapters read LN1's output: no fold
        if LN1_FOLD and c.dt in OP16 and x.dtype == c.dt and not attn_lora_live:
            return (None,) + ops.layernorm_stats(x, c.D, c.M, c.D, n1.weight.detach(), n1.bias.detach(), c.eps, c.dt)
        return ops.layernorm_fwd(x, c.D, c.M, c.D, n1.weight.detach(), n1.bias.detach(), c.eps, c.dt)

    def _fwd_qkv(self, c, i, blk, x, xn, mean1, rstd1, tail):
        """QKV projection -> (qkv, q_cls, uq, layout). layout 0 / 1: qkv [M, 3*inner] token-major / head-major; layout 2 (cls-query last
        block, QSPLIT): qkv is K | V [M, 2*inner] and q_cls [B, inner] the cls rows' Q. uq: the adapters' down-projection (attention site)."""
        dt, B, T, D, M, inner = c.dt, c.B, c.T, c.D, c.M, c.H * 64
        fold = xn is None
        qsplit = tail and QSPLIT and not c.attn_site
        qkv = torch.empty(M, (2 if qsplit else 3) * inner, device=c.dev, dtype=dt)
        a = x if fold else xn
        # live q / k / v adapters: one block-diagonal LoRA K segment, always in that form (no fold while they are live: a is xn)
        live = c.attn_site and not blk.qkv_lora.merged
        st = self._lora_project(c, a, self.qkv_lora_ops(i, blk.qkv_lora, dt).__getitem__ if live else None, "fwd", 3 * inner, in_kernel_ok=False)
        # operand, weight, bias and epilogue: the stream itself with W' = W * gamma, d = W beta (+ bias) and the row statistics finishing
        # the normalisation in the epilogue (aux = rowsum(W')), or LayerNorm 1's output with the weight as it is
        if fold:
            (w, cw, b), ln = self.w_ln(f"qkv{i}", blk.qkv_w, blk.ln1.weight, blk.ln1.bias, blk.qkv_b, dt), dict(pos=mean1, cls=rstd1)
        else:
            w, cw, b, ln = self.w(f"qkv{i}", blk.qkv_w, dt), None, (None if blk.qkv_b is None else blk.qkv_b.detach()), {}
        if not qsplit:
            hm = 1 if (QKV_HEAD_MAJOR and dt in OP16 and T >= QKV_HM_MIN_T) else 0
            epi = (L.EPI_STORE_QKV_HM_LN if hm else L.EPI_STORE_LN) if fold else (L.EPI_STORE_QKV_HM if hm else L.EPI_STORE)
            # (T is the head-major store's; the token-major STORE_LN would read it as the row stride of mean / rstd: 0 = one per row)
            self._lora_finish(c, st, w, qkv, dict(epilogue=epi, T=0 if (fold and not hm) else T, aux=cw, bias=b, **ln))
            return qkv, None, st.u, hm
        # K and V for every token, Q for the cls rows only: rows inner .. 3*inner of the fused weight (and of W', c, d) are K | V
        rows = lambda t, s: None if t is None else t[s]
        kv, q = slice(inner, None), slice(None, inner)
        epi = L.EPI_STORE_LN if fold else L.EPI_STORE
        c.gemm(a, w[kv], qkv, epilogue=epi, aux=rows(cw, kv), bias=rows(b, kv), **ln)
        q_cls = torch.empty(B, inner, device=c.dev, dtype=dt)
        c.gemm(a.view(B, T * D)[:, :D], w[q], q_cls, epilogue=epi, T=T if fold else 0,      # A = the cls rows, T*D apart (T: their statistics, T apart)
                    aux=rows(cw, q), bias=rows(b, q), **ln)
        return qkv, q_cls, None, 2

    def _fwd_attention(self, c, i, blk, x, qkv, q_cls, hm, tail):
        """Attention and the out-projection with its residual: x1 = x + drop(Wo attn + bo). -> (o, lse, x1)"""
        sp, B, T, D = c.sp, c.B, c.T, c.D
        if tail:      # only the cls query of the last block is ever consumed: B rows from here on
            o, lse = ops.attention_fwd_cls(qkv, B, T, c.H, sp.attn_scale, layout=hm, q_cls=q_cls)
            xres = x.view(B, T, D)[:, 0].contiguous()
        else:
            o, lse = ops.attention_fwd(qkv, B, T, c.H, sp.attn_scale, layout=hm)
            xres = x
        x1 = torch.empty(xres.shape[0], D, device=c.dev, dtype=c.xdt)
        c.gemm(o, self.w(f"wo{i}", blk.out.weight, c.dt), x1, epilogue=c.epi_res,
                    bias=blk.out.bias.detach(), res=xres, p_drop=c.pd(i), seed=c.seed, site=(4 * (i + c.sp.block0)) | c.sflag)
        return o, lse, x1

    def _fwd_ffn(self, c, i, blk, x1):
        """FFN sub-layer: x2 = x1 + drop(W2' drop(gelu(W1' LN2 x1))), W' = W + s B A while the FFN adapters are live.
        -> (x2, this sub-layer's part of the block's stash or None)"""
        dt, D, r, dev, save = c.dt, c.D, c.r, c.dev, c.save
        n2, l1, l2 = blk.ln2, blk.l1, blk.l2
        Mr, mlp = x1.shape[0], l1.weight.shape[0]
        lora_on = r > 0 and not c.attn_site and not l1.merged
        pk1, pk2 = (self.ffn_packs(i, 1, l1, dt), self.ffn_packs(i, 2, l2, dt)) if lora_on else (None, None)
        # bf16 stream: LayerNorm 2 also emits u1 = s * xn2 A1^T (the LoRA K segment of FFN1) instead of a skinny GEMM that re-reads xn2
        ln_u1 = LN_LORA and lora_on and r <= 16 and D in (512, 768) and x1.dtype == torch.bfloat16 and dt == torch.bfloat16      # (bf16 operands + bf16 stream only)
        u1_ln = None
        if ln_u1:
            xn2, mean2, rstd2, u1_ln = ops.layernorm_fwd_lora(x1, D, Mr, D, n2.weight.detach(), n2.bias.detach(), c.eps,
                                                               pk1(self.LORA_KINDS["fwd", "kseg"][0]), c.s_lora)
        else:
            xn2, mean2, rstd2 = ops.layernorm_fwd(x1, D, Mr, D, n2.weight.detach(), n2.bias.detach(), c.eps, dt)
        if lora_on and (abs(l1.scaling * r - 1.0) > 1e-9 or abs(l2.scaling * r - 1.0) > 1e-9):
            raise NotImplementedError("gs-lora_amd: the fused LoRA path uses scaling = 1 / r (lora_alpha = 1, the only value GS-LoRA "
                                      f"passes); got scaling {l1.scaling} / {l2.scaling} for r = {r}")
        h = torch.empty(Mr, mlp, device=dev, dtype=dt)
        gp8 = GP8 and dt in OP16 and save and mlp % 64 == 0
        gp = torch.empty(Mr, mlp, device=dev, dtype=torch.uint8 if gp8 else dt) if save else None
        # FFN1. In-kernel only at few rows: at full size the K-segment form is as fast (the 8 N-tiles of a row panel would each recompute
        # u1), and its skinny GEMM also writes u1's first 16 columns as a compact [M, 16] tensor — the operand form the gradient-fused
        # FFN2-dX epilogue reads 32 rows of with one contiguous 1 KB load (16-bit modes, rank <= 16)
        st1 = self._lora_project(c, xn2, pk1, "fwd", mlp, in_kernel_ok=Mr < INK_MIN_ROWS, u=u1_ln,
                                 compact=save and dt in OP16 and r <= 16 and Mr >= INK_MIN_ROWS)
        self._lora_finish(c, st1, self.w(f"w1_{i}", l1.weight, dt), h, dict(
            epilogue=L.EPI_BIAS_GELU_G8 if gp8 else L.EPI_BIAS_GELU, bias=l1.bias.detach(), out2=gp, p_drop=c.pd(i), seed=c.seed,
            site=(4 * (i + c.sp.block0) + 1) | c.sflag, tag="ffn1" if lora_on else None))
        st2 = self._lora_project(c, h, pk2, "fwd", D)
        x2 = torch.empty(Mr, D, device=dev, dtype=c.xdt)
        self._lora_finish(c, st2, self.w(f"w2_{i}", l2.weight, dt), x2, dict(
            epilogue=c.epi_res, bias=l2.bias.detach(), res=x1, p_drop=c.pd(i), seed=c.seed, site=(4 * (i + c.sp.block0) + 2) | c.sflag))
        return x2, (dict(mean2=mean2, rstd2=rstd2, xn2=xn2, u1=st1.u, u1c=st1.uc, h=h, gp=gp, u2=st2.u, lora_on=lora_on) if save else None)

    def _fwd_head(self, c, x, label):
        """Final LayerNorm, pooling and the head of the model's kind. -> (logits, emb, what the head backward needs)"""
        sp, B, D, hn = c.sp, c.B, c.D, c.sp.final_ln
        Th = x.shape[0] // B      # rows per image of the stream that reaches the head: T, or 1 after a cls-row-only last block
        cos_y = None
        ln = (x, B, Th, D, hn.weight.detach(), hn.bias.detach(), c.eps)
        if sp.head_kind in LINEAR_HEADS:      # plain classifier, no normalisation, no margin: logits for every call (ModifiedViT) / with a label (Softmax)
            Wn = sp.head_w.detach().contiguous() if (sp.head_kind == "linear" or label is not None) else None
            logits, emb, meanh, rstdh = ops.head_fwd(*ln, Wn, None, 1.0, 0.0, head_bias=sp.head_b.detach(), linear=Wn is not None,
                                                     pool_mean=(sp.pool == "mean"))
        else:
            if label is None:
                Wn = None
            elif sp.head_w.requires_grad:
                Wn = ops.cosface_prep(sp.head_w.detach().contiguous())
            else:      # frozen head (GS-LoRA trains the adapters only): the row-normalised weight is computed once per weight version
                Wn = self._cached(self._wcache, ("cosface_wn",), sp.head_w, lambda p: ops.cosface_prep(p.contiguous()))
            if sp.head_kind == "arcface":      # cos_y: the label column's cosine before the margin, for the backward's branch
                logits, emb, meanh, rstdh, cos_y = ops.head_fwd_margin(*ln, Wn, label, sp.cos_s, 0.0, "arcface", m=sp.cos_m,
                                                                       easy_margin=sp.easy_margin, pool_mean=(sp.pool == "mean"))
            else:
                logits, emb, meanh, rstdh = ops.head_fwd(*ln, Wn, label, sp.cos_s, sp.cos_m, pool_mean=(sp.pool == "mean"))
        return logits, emb, dict(Th=Th, meanh=meanh, rstdh=rstdh, Wn=Wn, cos_y=cos_y)

    # ------------------------------------------------------------------ backward
    def head_param_grads(self, saved, dlogits, want):
        """d loss / d (head weight[, head bias]) from the upstream dlogits: ONE gsl_head_wgrad launch into fresh buffers, for the head
        parameters that train (`want`: one flag per parameter handed to the autograd node — the weight, then the Softmax head's bias).
        Reads the forward's emb (and, ArcFace, its labels and label cosines) and the raw weight: no activation of the blocks, no
        gsl_head_bwd, no loss-scale state — the head's arithmetic is f32 in every compute mode."""
        sp = saved["ctx"].sp
        if dlogits is None or not any(want):
            return (None,) * len(want)
        params = [p for p in (sp.head_w, sp.head_b) if p is not None and p.requires_grad]
        linear = sp.head_kind in LINEAR_HEADS
        dW, db = ops.head_wgrad(dlogits.contiguous().float(), saved["emb"], sp.head_w.detach().contiguous(),
                                "linear" if linear else sp.head_kind, cos_s=sp.cos_s, m=sp.cos_m, easy_margin=sp.easy_margin,
                                label=saved["label"], cos_y=saved["cos_y"], bias=linear and sp.head_b is not None and sp.head_b.requires_grad)
        by_param = {id(sp.head_w): dW, id(sp.head_b): db}
        return tuple(by_param[id(p)] if w else None for p, w in zip(params, want))

    def backward(self, saved, dlogits, demb, at=None):
        """Accumulates d(loss)/d(LoRA) into the flat gradient bucket (views are the params' .grad). One chain for both LoRA sites: with
        the adapters on the FFN it stops after the LoRA gradients of block 0's FFN; with the adapters on the QKV projection
        (--lora_pos Attention; reference vit_face.py:349-355 with loralib.MergedLinear) the FFN is a plain frozen sub-layer (dX only),
        every block's attention needs its dqkv, and the chain stops after the LoRA gradients of block 0's projection.
        at = (G, coef) (a lower + upper pair, sp.boundary = k): the attention-transfer term's gradient coef * G[b, d] * x[b, t, d] enters
        at the boundary, see _inject_at."""
        c = saved["ctx"]
        sp, bucket = c.sp, self.bucket
        if c.ffn_train:      # third configuration (no LoRA in the model): see _bwd_ffn_train. -> {id(parameter): its gradient}
            bucket, c.wgrads, c.wg_ws = None, {}, self._wgrad_workspace(c, sp)
        elif bucket is None:
            return
        else:
            bucket.attach_grads()
        dx, dxb = self._bwd_head(c, saved, dlogits, demb)
        if bucket is not None:
            c.gv = {id(p): g for p, g in zip(bucket.params, bucket.grad_views)}
        c.pending = []      # deferred LoRA-gradient reductions (launch-bound regime): (Y, U, G, gsn, gsj, r, accumulate), operands kept alive
        nl = len(saved["layers"])
        for i in reversed(range(nl)):
            st, blk = saved["layers"][i], sp.blocks[i]
            # The network pools x[:, 0] (vit_face.py:540): the stream gradient entering the LAST block is exactly zero
            # outside the B cls rows, so its FFN backward, LoRA-gradient reductions, LN2 backward, out-proj dX and the
            # attention backward (a rank-1 cls-query form) run on B rows instead of B*T. Exact, not an approximation.
            sparse = (i == nl - 1) and sp.pool == "cls"      # (with pool='mean' every token carries gradient: dense last block)
            # tail: the forward of this block already ran on the cls rows, every saved tensor behind the attention is [B, .]; otherwise
            # dx / dxb arrive compact ([B, D]) from the head backward and the cls rows of the dense saved tensors are gathered
            gather = sparse and not st["tail"]
            # trainable FFN weights: a block whose FFN tensors all stay frozen (the upper half of a lower + upper pair) takes the dX-only form
            ffn_bwd = ((self._bwd_ffn_train if _ffn_requires_grad(blk) else self._bwd_ffn_frozen) if c.ffn_train
                       else (self._bwd_ffn_frozen if c.attn_site else self._bwd_ffn_lora))
            dxn2 = ffn_bwd(c, i, blk, st, dxb, gather)
            if dxn2 is None:
                break   # FFN site / trainable FFN weights: nothing below the layer-0 FFN input is trainable
            dx1, dx1b = self._bwd_ln2(c, i, blk, st, dxn2, dx, gather)
            del dxn2
            # ---- attention sub-layer: x1 = x + drop(Wo o + bo) -------------------------------------
            d_o = torch.empty(dx1b.shape[0], c.H * 64, device=c.dev, dtype=c.dt)
            c.gemm(dx1b, self.wT(f"wo{i}", blk.out.weight, c.dt), d_o)
            if c.attn_site:
                dqkv = self._bwd_attention(c, st, d_o, sparse)
                del d_o, dx1b
                dxn1 = self._bwd_qkv_lora(c, i, blk, st, dqkv)
                del dqkv
                if dxn1 is None:
                    break      # attention site: nothing below the block-0 QKV projection is trainable
            else:
                dxn1 = self._bwd_qkv_frozen(c, i, blk, st, d_o, sparse)
                del d_o, dx1b
            cls_T = c.T if sparse else 0      # after the cls-row-only block dx1 is compact [B, D]
            if at is not None and i == sp.boundary:
                dx1, cls_T = self._inject_at(c, st["x"], dx1, cls_T, at), 0
            dx, dxb = ops.layernorm_bwd(dxn1, st["x"], c.D, blk.ln1.weight.detach(), st["mean1"], st["rstd1"], dx1,
                                        p_drop=c.pd(i - 1), seed=c.seed, site=(4 * (i - 1) + 2) | c.sflag,
                                        dres_cls_T=cls_T, gmax=c.gmax)
            saved["layers"][i] = None   # free this layer's activations
        if c.ffn_train:
            return c.wgrads
        if not c.attn_site and not torch.cuda.is_current_stream_capturing():
            self.build_pack_tables(c.dt)    # every pack of the step is registered now: the next forward refreshes them in one launch

    def _inject_at(self, c, x, dx1, cls_T, at):
        """The boundary of a lower + upper pair, block k = sp.boundary. x (block k's saved input) IS the student's mid stream, and through
        the residual x1 = x + attn(LN1 x) the stream gradient dx1 reaches it unchanged: the attention-transfer term's gradient
        coef * S * G[b, d] * x[b, t, d] (gsa_at_bwd; S: the loss scale of an fp16 pass, else 1) is added IN PLACE to dx1 on the forget rows
        BEFORE LayerNorm 1's backward reads it as its residual input. That one kernel then writes dx = dx1 + LN1'(dxn1) and its
        operand-format copy dxb (with block k-1's FFN2 dropout mask) from the same sum, and raises the overflow guard to the largest |dx|
        it stores: both forms are consistent and the guard sees the gradient with the injected term. dx1's other reader (the out-proj dX
        GEMM, through dx1b) has run by now. When block k is the cls-row-only last block (an upper half of one block) dx1 is compact
        [B, D]: it is spread to the dense [M, D] rows first. -> the dense dx1"""
        from . import at as AT
        G, coef = at
        if cls_T:
            dense = torch.zeros(c.M, c.D, device=c.dev, dtype=dx1.dtype)
            dense.view(c.B, c.T, c.D)[:, 0] = dx1
            dx1 = dense
        one = c.gscale[0:1] if c.gscale is not None else self._ones(c.dev)
        AT.at_inject(dx1, x, G, coef, one, T=c.T)
        return dx1

    def _ones(self, dev):
        o = self._wcache.get(("zeros", "one", dev))      # (kept by invalidate_operand_caches like the zero vectors)
        if o is None:
            o = self._wcache[("zeros", "one", dev)] = torch.ones(1, device=dev, dtype=torch.float32)
        return o

    def _bwd_head(self, c, saved, dlogits, demb):
        """Head backward with the loss-scale / overflow-guard state of the pass. -> (dx, dxb): the stream gradient entering the last block,
        compact [B, D] cls rows under pool='cls' (nothing zero-filled)."""
        sp, dt = c.sp, c.dt
        if dlogits is not None:
            dlogits = dlogits.contiguous().float()
        if demb is not None:
            demb = demb.contiguous().float()
        if dlogits is not None and saved["Wn"] is None:
            raise RuntimeError("backward through logits requires a forward with labels")
        # fp16 operands: the backward runs on loss-scaled gradients — gsl_head_bwd picks the power of two S on the device and writes
        # {S, 1/S} here; every LoRA-gradient reduction below multiplies by 1/S on the way out (bf16 / f32: no scaling)
        c.gscale = self._loss_scale_state(saved["x_last"].device) if dt == torch.float16 else None
        self._guard_on = c.gscale is not None
        c.gmax = c.gscale[2:] if c.gscale is not None else None      # the overflow guard: raised by every LayerNorm backward below
        linear_head = sp.head_kind in LINEAR_HEADS
        # ArcFace: the margin form, with the label column's cosine and the labels the forward saved
        margin = {}
        if sp.head_kind == "arcface":
            margin = dict(head_kind="arcface", m=sp.cos_m, easy_margin=sp.easy_margin, cos_y=saved["cos_y"], label=saved["label"])
        return (ops.head_bwd_margin if margin else ops.head_bwd)(
            dlogits, demb, saved["x_last"], c.B, saved["Th"], c.D, sp.final_ln.weight.detach(), saved["meanh"], saved["rstdh"],
            saved["emb"], saved["Wn"], 1.0 if linear_head else sp.cos_s, dt, p_drop=c.pd(len(saved["layers"]) - 1), seed=c.seed,
            site=(4 * (len(saved["layers"]) - 1) + 2) | c.sflag, linear=linear_head, pool_mean=(sp.pool == "mean"),
            stream_dtype=dt if (dt in OP16 and GRAD_STREAM_BF16) else torch.float32,
            compact=(sp.pool == "cls"), gscale=c.gscale, target_exp=GRAD_TARGET_EXP, **margin)

    def _lgrad(self, c, Y, U, G, gsn, gsj, rr):
        """One LoRA-gradient reduction: deferred to the batched launch pair of _flush where it fits, issued now otherwise."""
        if Y.shape[0] < LGRAD_BATCH_MAX_ROWS and c.M < LGRAD_BATCH_MAX_ROWS and ops.lora_grad_batchable(Y, U, rr):
            c.pending.append((Y, U, G, gsn, gsj, rr, True))
        else:
            ops.lora_grad(Y, U, G, gsn, gsj, rr, gscale=c.gscale)

    def _flush(self, c):
        ops.lora_grad_batch(c.pending, gscale=c.gscale)
        c.pending.clear()

    def _grads_done(self, c, i):
        """The LoRA gradients of block i are complete: the hook hands finished gradient slices to the all-reduce."""
        if self.grad_hook is not None:
            self._flush(c)
            self.grad_hook(i)

    def _bwd_ffn_lora(self, c, i, blk, st, dyb, gather):
        """FFN sub-layer with live adapters: y = x1 + drop(W2' h + b2), h = drop(gelu(W1' xn2 + b1)). The four LoRA gradients, then
        -> dxn2 (None for block 0, where the chain ends)."""
        dt, D, r, dev, gv = c.dt, c.D, c.r, c.dev, c.gv
        l1, l2 = blk.l1, blk.l2
        mlp = l1.weight.shape[0]
        if not st["lora_on"]:
            raise RuntimeError("backward with merged LoRA weights is undefined (model.train() un-merges)")
        if gather:
            xn2, h, gp, u1, u2 = (_cls_rows(c, st["xn2"], D), _cls_rows(c, st["h"], mlp), _gp_rows(c, st["gp"], mlp),
                                  _cls_rows(c, st["u1"], PADK), _cls_rows(c, st["u2"], PADK))
        else:
            xn2, h, gp, u1, u2 = st["xn2"], st["h"], st["gp"], st["u1"], st["u2"]
        u1c = None if gather else st.get("u1c")      # the compact [M, 16] form of u1 (16-bit modes, full-size blocks)
        Mrows = dyb.shape[0]
        # FFN2-dX -> da = (dy W2' ) * g', with v2 = s*dy*B2 (g' possibly as the 8-bit code of the forward: decode scale from p_drop)
        s2 = self._lora_project(c, dyb, self.ffn_packs(i, 2, l2, dt), "dx", mlp)
        da = torch.empty(Mrows, mlp, device=dev, dtype=dt)
        w2t = self.wT(f"w2_{i}", l2.weight, dt)
        fused_grads = s2.ink and FUSE_LORA_GRAD and Mrows >= INK_MIN_ROWS      # the gradient-fused epilogue lives on the 8-phase kernel
        if fused_grads:
            # the two gradient reductions that contract over the rows of the [M, mlp] tiles (dB1 from the da the GEMM produces, dA2 from
            # h and the v2 it holds) ride in its epilogue
            self._lora_finish(c, s2, w2t, da, dict(tag="ffn2dx", p_drop=c.p_drop, gscale=c.gscale),
                              mulgrad=(gp, u1c if u1c is not None else u1, gv[id(l1.lora_B)], (r, 1), h, gv[id(l2.lora_A)], (1, mlp), r))
        else:
            self._lora_finish(c, s2, w2t, da, dict(epilogue=L.EPI_MUL_G8 if gp.dtype == torch.uint8 else L.EPI_MUL, aux=gp, p_drop=c.p_drop))
        self._lgrad(c, dyb, u2, gv[id(l2.lora_B)], r, 1, r)                        # dB2[c, j]
        if not fused_grads:
            self._lgrad(c, h, s2.u, gv[id(l2.lora_A)], 1, mlp, r)                  # dA2[j, hid]
        # FFN1-dX with v1 = s*da*B1. The in-kernel form makes v1 in the dX launch itself, so that launch goes in front of the reductions
        # that read v1; in the K-segment form they (and the hook) run between the two halves. Block 0 needs v1 alone: K-segment form.
        s1 = self._lora_project(c, da, self.ffn_packs(i, 1, l1, dt), "dx", D, in_kernel_ok=i > 0)
        finish = lambda: self._lora_finish(c, s1, self.wT(f"w1_{i}", l1.weight, dt), torch.empty(Mrows, D, device=dev, dtype=dt), {})
        dxn2 = finish() if s1.ink else None
        if not fused_grads:
            self._lgrad(c, da, u1, gv[id(l1.lora_B)], r, 1, r)                     # dB1[hid, j]
        self._lgrad(c, xn2, s1.u, gv[id(l1.lora_A)], 1, D, r)                      # dA1[j, c]
        self._grads_done(c, i)
        if i == 0:
            self._flush(c)
            return None
        return dxn2 if s1.ink else finish()

    def _bwd_ffn_frozen(self, c, i, blk, st, dyb, gather):
        """FFN sub-layer without live adapters (attention site), or a frozen one among trainable FFN weights: dX only. -> dxn2 (None for
        block 0 of a pass that trains FFN weights, where the chain ends)."""
        dt, l1, l2 = c.dt, blk.l1, blk.l2
        if c.ffn_train:
            if i == 0:
                return None
        elif st["uq"] is None:
            raise RuntimeError("backward with merged LoRA weights is undefined (model.train() un-merges)")
        mlp = l1.weight.shape[0]
        gp = _gp_rows(c, st["gp"], mlp) if gather else st["gp"]
        da = torch.empty(dyb.shape[0], mlp, device=c.dev, dtype=dt)
        c.gemm(dyb, self.wT(f"w2_{i}", l2.weight, dt), da, epilogue=L.EPI_MUL_G8 if gp.dtype == torch.uint8 else L.EPI_MUL, aux=gp,
                    p_drop=c.pd(i))
        dxn2 = torch.empty(dyb.shape[0], c.D, device=c.dev, dtype=dt)
        c.gemm(da, self.wT(f"w1_{i}", l1.weight, dt), dxn2)
        return dxn2

    def _wgrad_workspace(self, c, sp):
        """One f32 workspace for every gst_wgrad of a backward pass: the largest gst_wgrad_ws_elems of its shapes (both FFN products, on all
        M rows and on the B cls rows of the last block under pool='cls')."""
        from . import _lib_train as LT
        mlp = sp.blocks[0].l1.weight.shape[0]
        rows = {c.M, c.B} if sp.pool == "cls" else {c.M}
        n = max(LT.wgrad_ws_elems(m, a, b, c.dt) for m in rows for a, b in ((c.D, mlp), (mlp, c.D)))
        return torch.empty(n, device=c.dev, dtype=torch.float32)

    def _bwd_ffn_train(self, c, i, blk, st, dyb, gather):
        """FFN sub-layer whose two linears train (no adapters): FFN2-dX as _bwd_ffn_frozen forms it, then the weight and bias gradients
        dW2 = dyb^T h, db2 = colsum(dyb), dW1 = da^T xn2, db1 = colsum(da) (gst_wgrad, fresh f32 buffers in c.wgrads; fp16: the loss
        scale is divided out), then FFN1-dX -> dxn2 (None for block 0, where the chain ends)."""
        from . import _lib_train as LT
        dt, D, l1, l2 = c.dt, c.D, blk.l1, blk.l2
        mlp = l1.weight.shape[0]
        if gather:
            xn2, h, gp = _cls_rows(c, st["xn2"], D), _cls_rows(c, st["h"], mlp), _gp_rows(c, st["gp"], mlp)
        else:
            xn2, h, gp = st["xn2"], st["h"], st["gp"]
        da = torch.empty(dyb.shape[0], mlp, device=c.dev, dtype=dt)
        c.gemm(dyb, self.wT(f"w2_{i}", l2.weight, dt), da, epilogue=L.EPI_MUL_G8 if gp.dtype == torch.uint8 else L.EPI_MUL, aux=gp,
                    p_drop=c.pd(i))
        for layer, Y, X in ((l2, dyb, h), (l1, da, xn2)):
            dW = torch.empty(layer.weight.shape, device=c.dev, dtype=torch.float32)
            db = torch.empty(layer.bias.shape, device=c.dev, dtype=torch.float32)
            LT.wgrad(Y, X, dW, db, ws=c.wg_ws, gscale=c.gscale)
            c.wgrads[id(layer.weight)], c.wgrads[id(layer.bias)] = dW, db
        if i == 0:
            return None
        dxn2 = torch.empty(dyb.shape[0], D, device=c.dev, dtype=dt)
        c.gemm(da, self.wT(f"w1_{i}", l1.weight, dt), dxn2)
        return dxn2

    def _bwd_ln2(self, c, i, blk, st, dxn2, dx, gather):
        """LayerNorm 2 backward -> (dx1, dx1b): the stream gradient at x1 and its operand-format copy with the out-proj dropout mask."""
        gamma, kw = blk.ln2.weight.detach(), dict(p_drop=c.pd(i), seed=c.seed, site=(4 * i) | c.sflag, gmax=c.gmax)
        if gather:   # compact in, compact out: the cls rows of x1 are T*D apart, the dropout counters are those of the dense tensor
            return ops.layernorm_bwd(dxn2, st["x1"], c.T * c.D, gamma, _cls_rows(c, st["mean2"].view(-1, 1), 1).view(-1),
                                     _cls_rows(c, st["rstd2"].view(-1, 1), 1).view(-1), dx, drop_row_stride=c.T * c.D, **kw)
        return ops.layernorm_bwd(dxn2, st["x1"], c.D, gamma, st["mean2"], st["rstd2"], dx, **kw)

    def _bwd_attention(self, c, st, d_o, sparse):
        """Attention backward -> dqkv [B*T, 3*inner], or (dkv [B*T, 2*inner], dq_cls [B, inner]) where the forward projected Q for the
        cls rows only (layout 2). sparse: the cls-query form of the last block."""
        if sparse:
            return ops.attention_bwd_cls(st["qkv"], st["o"], d_o, st["lse"], c.B, c.T, c.H, c.sp.attn_scale, layout=st["qkv_hm"], q_cls=st["q_cls"])
        return ops.attention_bwd(st["qkv"], st["o"], d_o, st["lse"], c.B, c.T, c.H, c.sp.attn_scale, layout=st["qkv_hm"])

    def _bwd_qkv_frozen(self, c, i, blk, st, d_o, sparse):
        """Attention backward and the dX of the frozen QKV projection (FFN site). -> dxn1"""
        dt, D, inner = c.dt, c.D, c.H * 64
        dxn1 = torch.empty(c.M, D, device=c.dev, dtype=dt)
        dqkv = self._bwd_attention(c, st, d_o, sparse)
        wt = self.wT(f"qkv{i}", blk.qkv_w, dt)                         # [dim, 3*inner]
        if st["q_cls"] is None:
            c.gemm(dqkv, wt, dxn1)
        else:      # Q was projected for the cls rows only: dX contracts over K | V, the cls rows get dQ W_q on top
            dkv, dq_cls = dqkv
            c.gemm(dkv, wt[:, inner:], dxn1)
            rows = dxn1.view(c.B, c.T * D)[:, :D]                      # the cls rows of dxn1, T*D apart: updated in place
            c.gemm(dq_cls, wt[:, :inner], rows, epilogue=_res_epilogue(dt), bias=self._zeros(D, c.dev), res=rows)
        return dxn1

    def _bwd_qkv_lora(self, c, i, blk, st, dqkv):
        """QKV projection with the q / k / v adapters (attention site): their gradients, then -> dxn1 with the adapter segment (None for
        block 0, where the chain ends). Same kernels as the FFN-site path."""
        dt, D, r, ml = c.dt, c.D, c.r, blk.qkv_lora
        sq = self._lora_project(c, dqkv, self.qkv_lora_ops(i, ml, dt).__getitem__, "dx", D, in_kernel_ok=False)
        v = sq.u                                                                 # v[:, g*r+j] = s * dqkv_g . B_g[:, j]
        ng, inner = len(ml.enable_lora), c.H * 64
        gA, gB = c.gv[id(ml.lora_A)], c.gv[id(ml.lora_B)]
        for g in range(ng):
            ops.lora_grad(st["xn"], v[:, g * r:], gA[g * r:(g + 1) * r], 1, D, r, gscale=c.gscale)                       # dA_g[j, c]
            ops.lora_grad(dqkv[:, g * inner:(g + 1) * inner], st["uq"][:, g * r:], gB[g * inner:(g + 1) * inner], r, 1, r, gscale=c.gscale)   # dB_g[n, j]
        self._grads_done(c, i)
        if i == 0:
            return None
        return self._lora_finish(c, sq, self.wT(f"qkv{i}", blk.qkv_w, dt), torch.empty(c.M, D, device=c.dev, dtype=dt), {})
