"""The model geometries of the sweep (tests/test_geometry_sweep_host.py on the CPU, tests/test_hip_geometry_sweep.py on the GPU): a named
table of ViT_face configurations with their batch sizes, and what both files need of a row. No test lives here.

Every case has dim_head 64, heads = dim / 64, 8-pixel patches and 3 channels unless its row says otherwise; image sizes 8 / 16 / 24 give
T = 2 / 5 / 10 tokens. The table reaches every width of ln_for_width (csrc/norm.hip), depth 1 (the only block is block 0 and the
cls-row-only last block at once), T = 2, batch 1, ranks 1 2 3 5 7 16 21, mlp widths off a multiple of 256, one channel, patch dimensions 64
and 256. A later sweep of another family is a matter of adding rows.

The reference's constructor (vit_face.py:477) asserts more than 16 patches per image, and ViT_face keeps that assertion: `build` lowers
vit_face.MIN_NUM_PATCHES while it constructs, so that the runner and the kernels, which take any T > 1, are reached at token counts where
one forward and backward is a few hundred rows.

Helpers: `build` (the model on the GPU), `inputs` (seeded images, labels and upstream gradients), `reference` / `cpu32` (the float64
restatement of tests/large_row_reference.py and its float32 run, cached per case), `forward_with_fault` / `fault_gradients` (a copy of that
forward with one of six fault models applied; without a fault it is bit-identical to LR.forward, which the host file asserts)."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

import large_row_reference as LR
from oracle import gslora_oracle as O
from oracle import recipe

NUM_CLASS = 12


def _cfg(dim, depth, image_size, mlp_dim, lora_rank, patch_size=8, channels=3, **other):
    return dict(image_size=image_size, patch_size=patch_size, dim=dim, depth=depth, heads=dim // 64, dim_head=64, mlp_dim=mlp_dim,
                num_class=NUM_CLASS, lora_rank=lora_rank, channels=channels, **other)


# name -> (configuration, batch)
CASES = {
    "min64": (_cfg(64, 1, 8, 64, 1, channels=1), 1),
    "d128_mean": (_cfg(128, 1, 16, 192, 2, pool="mean"), 2),
    "d256_min": (_cfg(256, 1, 8, 64, 1), 3),
    "d256_batchable": (_cfg(256, 2, 24, 256, 8), 3),      # the smallest model where all four FFN reductions of a block have N % 256 == 0
    "d256_odd": (_cfg(256, 3, 16, 192, 5, pool="mean"), 2),
    "d256_attn": (_cfg(256, 2, 24, 128, 7, lora_pos="Attention"), 3),
    "d512_min": (_cfg(512, 1, 8, 64, 3), 1),
    "d768_odd": (_cfg(768, 2, 16, 320, 16), 2),
    "d1024_min": (_cfg(1024, 1, 16, 64, 3), 3),
    "d1024_t2": (_cfg(1024, 2, 8, 320, 16), 2),
    "d1024_sq": (_cfg(1024, 2, 24, 1024, 8, pool="mean"), 2),
    "d1024_attn": (_cfg(1024, 2, 16, 128, 21, lora_pos="Attention"), 2),      # 3 r = 63, the largest the runner accepts
    "p16c1": (_cfg(64, 2, 32, 128, 4, patch_size=16, channels=1), 5),         # patch dimension 256, image 32
    # added to the starting set: every row above has fewer than 64 token rows, where the float32 modes' tile rule (csrc/gemm.hip,
    # gemm_tile_choice: N >= 128 and M >= 64) keeps every GEMM on the 64x64 VALU kernel and 'fp32x3' is 'fp32' bit for bit. 70 rows put
    # the dense block on the matrix-core kernels (the three-piece bf16 split in 'fp32x3'), the last block's 7 cls rows stay below the rule.
    "d256_m70": (_cfg(256, 2, 24, 192, 3), 7),
    "d1024_m70": (_cfg(1024, 2, 24, 320, 5), 7),
}
# the fixtures the suite ran through ViTRunner before the sweep (oracle/recipe.py), for the fault models' second half
OLD_FIXTURES = {"cfg_small": (recipe.cfg_small(), 2), "cfg_small2": (recipe.cfg_small2(), 2), "cfg_full": (recipe.cfg_full(), 1)}


def tokens(cfg):
    return (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1


@contextlib.contextmanager
def _few_patches_allowed():
    from vit_pytorch_face import vit_face
    keep, vit_face.MIN_NUM_PATCHES = vit_face.MIN_NUM_PATCHES, 0
    try:
        yield
    finally:
        vit_face.MIN_NUM_PATCHES = keep


def build(cfg, dtype, dropout=0.0):
    """The `build` of tests/test_hip_large_rows.py with `channels` passed through (and the reference's 16-patch assertion lowered)."""
    import loralib as lora
    from vit_pytorch_face import ViT_face
    with _few_patches_allowed():
        m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                     dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], channels=cfg["channels"],
                     dropout=dropout, emb_dropout=dropout, lora_rank=cfg["lora_rank"], lora_pos=cfg.get("lora_pos", "FFN"),
                     pool=cfg.get("pool", "cls"))
    m.load_state_dict({k: torch.tensor(v) for k, v in recipe.make_state(cfg).items()}, strict=True)
    lora.mark_only_lora_as_trainable(m)
    return m.to("cuda").set_compute_dtype(dtype).train()


_INPUTS = {}


def inputs(cfg, B):
    """(images, labels, dlogits, demb) of a batch, seeded f32 / int64 numpy arrays. Cached: callers do not write to them."""
    key = (repr(sorted(cfg.items())), B)
    if key not in _INPUTS:
        _INPUTS[key] = (recipe.make_images(cfg, B), recipe.make_labels(cfg, B)) + LR.upstream(cfg, B)
    return _INPUTS[key]


def _run(cfg, args, dtype, keep=None):
    """-> dict(logits, emb, grads) of the restated forward in `dtype`, everything as float64 numpy."""
    grads = LR.lora_gradients(cfg, *args, keep=keep, dtype=dtype)[0]
    with torch.no_grad():
        logits, emb, _ = LR.forward(LR.state(cfg, dtype), torch.as_tensor(args[0]), torch.as_tensor(args[1]).long(), cfg, keep=keep, dtype=dtype)
    return dict(logits=logits.numpy().astype(np.float64), emb=emb.numpy().astype(np.float64), grads=grads)


_REFS = {}


def reference(name, keep=None, key=None):
    """The float64 reference of a table row, once per process. keep / key: a dropout variant (the masks and what identifies them)."""
    if (name, "f64", key) not in _REFS:
        cfg, B = CASES[name]
        _REFS[name, "f64", key] = _run(cfg, inputs(cfg, B), torch.float64, keep)
    return _REFS[name, "f64", key]


def cpu32(name, keep=None, key=None):
    """The float32 CPU run of the same reference."""
    if (name, "f32", key) not in _REFS:
        cfg, B = CASES[name]
        _REFS[name, "f32", key] = _run(cfg, inputs(cfg, B), torch.float32, keep)
    return _REFS[name, "f32", key]


def tensors(run):
    """{name: array} of everything a run is compared on: logits, emb and every LoRA gradient."""
    return dict(run["grads"], logits=run["logits"], emb=run["emb"])


def cpu_errors(name, keep=None, key=None):
    """e_cpu(t) = relative Frobenius error of the float32 CPU run against float64, for every tensor of `tensors`."""
    ref, lo = tensors(reference(name, keep, key)), tensors(cpu32(name, keep, key))
    return {k: LR.rel_fro(lo[k], ref[k]) for k in ref}


# ---------------------------------------------------------------------------------------------------------------- fault models
FAULTS = {
    "a": "softmax scale dim_head ** -0.5 in place of the reference's dim ** -0.5",
    "b": "LoRA scale 1 / 8 whatever the rank is",
    "c": "the last head's attention output zeroed",
    "d": "heads 12 .. read the values of heads 0 .. (a head index wrapped at 12)",
    "e": "LayerNorm statistics over the first 512 columns only",
    "f": "at depth 1, the FFN residual of the cls row taken from the block input instead of the attention output",
}
WRAP_HEADS, STAT_COLUMNS = 12, 512


def _layer_norm(x, w, b, fault):
    if fault != "e":
        return F.layer_norm(x, (x.shape[-1],), w, b, O.LN_EPS)
    part = x[..., :STAT_COLUMNS]
    mean, var = part.mean(-1, keepdim=True), part.var(-1, unbiased=False, keepdim=True)
    return (x - mean) * torch.rsqrt(var + O.LN_EPS) * w + b


def forward_with_fault(st, img, label, cfg, fault=None, dtype=torch.float64):
    """LR.forward without dropout (-> logits, emb), with one fault of FAULTS applied. Every fault is written as the wrong computation itself,
    not as a branch on the geometry: where it changes nothing (dim == dim_head, r == 8, no 13th head, no 513th column, depth > 1), that
    is the arithmetic's doing."""
    p, D, H, r, depth = cfg["patch_size"], cfg["dim"], cfg["heads"], cfg["lora_rank"], cfg["depth"]
    attn_lora = cfg.get("lora_pos", "FFN") == "Attention"
    s = 1.0 / (8 if fault == "b" else r)
    scale = (cfg["dim_head"] if fault == "a" else D) ** -0.5
    x = O.patchify(img.to(dtype), p)
    x = F.linear(x, st["patch_to_embedding.weight"], st["patch_to_embedding.bias"])
    B, T = x.shape[0], x.shape[1] + 1
    x = torch.cat((st["cls_token"].expand(B, -1, -1), x), 1) + st["pos_embedding"][:, :T]
    for i in range(depth):
        a, f = f"transformer.layers.{i}.0.fn", f"transformer.layers.{i}.1.fn"
        x0 = x
        xn = _layer_norm(x, st[f"{a}.norm.weight"], st[f"{a}.norm.bias"], fault)
        qkv = F.linear(xn, st[f"{a}.fn.to_qkv.weight"])
        if attn_lora:
            qkv = qkv + (xn @ O.merged_delta(st[f"{a}.fn.to_qkv.lora_A"], st[f"{a}.fn.to_qkv.lora_B"], r).t()) * s
        q, k, v = [t.reshape(B, T, H, -1).permute(0, 2, 1, 3) for t in qkv.chunk(3, -1)]
        if fault == "d":
            v = v[:, [h % WRAP_HEADS for h in range(H)]]
        att = (torch.einsum("bhid,bhjd->bhij", q, k) * scale).softmax(-1)
        o = torch.einsum("bhij,bhjd->bhid", att, v)
        if fault == "c":
            o = torch.cat((o[:, :H - 1], torch.zeros_like(o[:, H - 1:])), 1)
        o = o.permute(0, 2, 1, 3).reshape(B, T, -1)
        x = F.linear(o, st[f"{a}.fn.to_out.0.weight"], st[f"{a}.fn.to_out.0.bias"]) + x
        xn2 = _layer_norm(x, st[f"{f}.norm.weight"], st[f"{f}.norm.bias"], fault)
        z = F.linear(xn2, st[f"{f}.fn.net.0.weight"], st[f"{f}.fn.net.0.bias"])
        if attn_lora:
            y = F.linear(F.gelu(z), st[f"{f}.fn.net.3.weight"], st[f"{f}.fn.net.3.bias"])
        else:
            u1 = (xn2 @ st[f"{f}.fn.net.0.lora_A"].t()) * s
            z = z + u1 @ st[f"{f}.fn.net.0.lora_B"].t()
            h = F.gelu(z)
            u2 = (h @ st[f"{f}.fn.net.3.lora_A"].t()) * s
            y = F.linear(h, st[f"{f}.fn.net.3.weight"], st[f"{f}.fn.net.3.bias"]) + u2 @ st[f"{f}.fn.net.3.lora_B"].t()
        res = x
        if fault == "f" and i == 0 and i == depth - 1:      # the block that is block 0 and the cls-row-only last block at once
            res = torch.cat((x0[:, :1], x[:, 1:]), 1)
        x = y + res
    x = x.mean(dim=1) if cfg.get("pool", "cls") == "mean" else x[:, 0]
    emb = _layer_norm(x, st["mlp_head.0.weight"], st["mlp_head.0.bias"], fault)
    return O.cosface(emb, st["loss.weight"], label), emb


def fault_gradients(cfg, B, fault):
    """The float64 LoRA gradients of sum(dlogits * logits) + sum(demb * emb) through forward_with_fault. -> {name: float64 numpy}"""
    img, label, dlogits, demb = inputs(cfg, B)
    st = LR.state(cfg)
    logits, emb = forward_with_fault(st, torch.as_tensor(img), torch.as_tensor(label).long(), cfg, fault)
    names = [k for k in st if "lora_" in k]
    loss = (logits * torch.as_tensor(dlogits).double()).sum() + (emb * torch.as_tensor(demb).double()).sum()
    return {k: g.numpy() for k, g in zip(names, torch.autograd.grad(loss, [st[k] for k in names]))}
