"""Double-precision restatement of the ViT_face forward for the large-row schedule tests (tests/test_large_row_probes_host.py proves it
against the oracle, tests/test_hip_large_rows.py uses it as the reference; tests/test_hip_model.py takes its mask-injected forward).

No test lives here. What it adds to oracle.gslora_oracle.vit_forward:
  * the FFN intermediates of every block stay reachable: xn2 (LayerNorm 2 output), z (pre-GELU), h (GELU output behind its dropout), y (the
    FFN output in front of its dropout), u1 = s xn2 A1^T, u2 = s h A2^T with s = 1 / r;
  * the upstream gradients (dlogits, demb) are an input: the LoRA gradients are autograd of sum(dlogits * logits) + sum(demb * emb), which
    is what ViTRunner.backward(saved, dlogits, demb) accumulates;
  * for one chosen image, each of a block's four reductions (dB2 = dy^T u2, dA2 = v2^T h, dB1 = da^T u1, dA1 = v1^T xn2, with v2 = s dy B2
    and v1 = s da B1) is restated row by row, together with sum_m |Y[m, n] U[m, j]|, the scale of its rounding error;
  * dropout masks are injected (`keep`), at the sites and with the counter layout of the HIP path.
Everything runs in `dtype` (float64 unless a test wants the float32 CPU path)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import gslora_oracle as O
from oracle import recipe

SITE_EMB = 1_000_000      # the dropout site of the embedding (vit_runner.SITE_EMB); block i: 4 i (out-proj), 4 i + 1 (GELU), 4 i + 2 (FFN output)
REDUCTIONS = ("dB2", "dA2", "dB1", "dA1")


def ffn_names(i):
    """Reduction -> the state-dict name of the LoRA tensor it fills, for block i."""
    f = f"transformer.layers.{i}.1.fn.fn.net"
    return {"dB2": f"{f}.3.lora_B", "dA2": f"{f}.3.lora_A", "dB1": f"{f}.0.lora_B", "dA1": f"{f}.0.lora_A"}


def state(cfg, dtype=torch.float64, seed=1337):
    return O.to_torch(recipe.make_state(cfg, seed), requires_grad_lora=True, dtype=dtype)


def forward(st, img, label, cfg, keep=None, dtype=torch.float64):
    """-> (logits, emb, blocks). blocks[i]: dict(xn2, z, h, y, u1, u2) of block i, [B, T, .] tensors of the autograd graph (FFN site; an empty
    dict per block with the adapters on q / k / v). keep(n, site) -> n multipliers mask / (1 - p) of dropout site `site` (None: no dropout).
    The HIP path runs the last block under pool='cls' on the cls rows alone, so there its counters index a compact [B, width] tensor and
    the other rows, which reach no output, are left as they are."""
    p, D, H, r, depth = cfg["patch_size"], cfg["dim"], cfg["heads"], cfg["lora_rank"], cfg["depth"]
    attn_lora = cfg.get("lora_pos", "FFN") == "Attention"
    pool = cfg.get("pool", "cls")
    s = 1.0 / r
    x = O.patchify(img.to(dtype), p)
    x = F.linear(x, st["patch_to_embedding.weight"], st["patch_to_embedding.bias"])
    B, T = x.shape[0], x.shape[1] + 1
    x = torch.cat((st["cls_token"].expand(B, -1, -1), x), 1) + st["pos_embedding"][:, :T]

    def drop(t, i, site):
        if keep is None:
            return t
        width = t.shape[-1]
        if i == depth - 1 and pool == "cls":
            full = torch.ones(B, T, width, dtype=dtype)
            full[:, 0] = keep(B * width, site).to(dtype).reshape(B, width)
            return t * full
        return t * keep(B * T * width, site).to(dtype).reshape(B, T, width)

    x = drop(x, -1, SITE_EMB)
    blocks = []
    for i in range(depth):
        a, f = f"transformer.layers.{i}.0.fn", f"transformer.layers.{i}.1.fn"
        xn = F.layer_norm(x, (D,), st[f"{a}.norm.weight"], st[f"{a}.norm.bias"], O.LN_EPS)
        qkv = F.linear(xn, st[f"{a}.fn.to_qkv.weight"])
        if attn_lora:
            qkv = qkv + (xn @ O.merged_delta(st[f"{a}.fn.to_qkv.lora_A"], st[f"{a}.fn.to_qkv.lora_B"], r).t()) * s
        q, k, v = [t.reshape(B, T, H, -1).permute(0, 2, 1, 3) for t in qkv.chunk(3, -1)]
        att = (torch.einsum("bhid,bhjd->bhij", q, k) * D ** -0.5).softmax(-1)
        o = torch.einsum("bhij,bhjd->bhid", att, v).permute(0, 2, 1, 3).reshape(B, T, -1)
        x = drop(F.linear(o, st[f"{a}.fn.to_out.0.weight"], st[f"{a}.fn.to_out.0.bias"]), i, 4 * i) + x
        xn2 = F.layer_norm(x, (D,), st[f"{f}.norm.weight"], st[f"{f}.norm.bias"], O.LN_EPS)
        z = F.linear(xn2, st[f"{f}.fn.net.0.weight"], st[f"{f}.fn.net.0.bias"])
        if attn_lora:
            h = drop(F.gelu(z), i, 4 * i + 1)
            y = F.linear(h, st[f"{f}.fn.net.3.weight"], st[f"{f}.fn.net.3.bias"])
            blocks.append({})
        else:
            u1 = (xn2 @ st[f"{f}.fn.net.0.lora_A"].t()) * s
            z = z + u1 @ st[f"{f}.fn.net.0.lora_B"].t()
            h = drop(F.gelu(z), i, 4 * i + 1)
            u2 = (h @ st[f"{f}.fn.net.3.lora_A"].t()) * s
            y = F.linear(h, st[f"{f}.fn.net.3.weight"], st[f"{f}.fn.net.3.bias"]) + u2 @ st[f"{f}.fn.net.3.lora_B"].t()
            blocks.append(dict(xn2=xn2, z=z, h=h, y=y, u1=u1, u2=u2))
        x = drop(y, i, 4 * i + 2) + x
    x = x.mean(dim=1) if pool == "mean" else x[:, 0]
    emb = F.layer_norm(x, (D,), st["mlp_head.0.weight"], st["mlp_head.0.bias"], O.LN_EPS)
    return (None if label is None else O.cosface(emb, st["loss.weight"], label)), emb, blocks


def reduction_operands(st, cfg, blk, grads_zy, image):
    """The (Y, U) row operands [T, .] of the four reductions of one block for one image: gradient[n, j] = sum_m Y[m, n] U[m, j], transposed
    for the two lora_A tensors (dA[j, n]). grads_zy = (d loss / d z, d loss / d y) of that block."""
    r = cfg["lora_rank"]
    da, dy = grads_zy[0][image], grads_zy[1][image]
    i = blk["index"]
    n = ffn_names(i)
    v2 = (dy @ st[n["dB2"]].detach()) / r
    v1 = (da @ st[n["dB1"]].detach()) / r
    d = lambda t: t[image].detach()
    return {"dB2": (dy, d(blk["u2"])), "dA2": (d(blk["h"]), v2), "dB1": (da, d(blk["u1"])), "dA1": (d(blk["xn2"]), v1)}


def reduce_rows(Y, U, transposed, rows=None, u_rows=None):
    """sum over `rows` of Y[m, :]^T U[u_rows[m], :] (every row, U read at the same row, by default); transposed: the lora_A layout [j, n]."""
    rows = torch.arange(Y.shape[0]) if rows is None else torch.as_tensor(rows)
    u_rows = rows if u_rows is None else torch.as_tensor(u_rows)
    g = Y[rows].t() @ U[u_rows]
    return g.t() if transposed else g


def lora_gradients(cfg, img, label, dlogits, demb, keep=None, dtype=torch.float64, image=None, seed=1337):
    """LoRA gradients of sum(dlogits * logits) + sum(demb * emb) by autograd, in `dtype`. -> (grads, ops): grads {name: float64 numpy array};
    ops is None unless `image` is given (FFN site), then {name: (Y, U, transposed)} for the twelve reductions of that image — `reduce_rows`
    of them is that image's share of the gradient, `abs_addends` the sum of its absolute addends."""
    st = state(cfg, dtype, seed)
    to = lambda t: torch.as_tensor(t).to(dtype)
    logits, emb, blocks = forward(st, torch.as_tensor(img), torch.as_tensor(label).long(), cfg, keep=keep, dtype=dtype)
    names = [k for k in st if "lora_" in k]
    want = [st[k] for k in names]
    inner = [t for b in blocks if b for t in (b["z"], b["y"])] if image is not None else []
    loss = (logits * to(dlogits)).sum() + (emb * to(demb)).sum()
    got = torch.autograd.grad(loss, want + inner)
    grads = {k: g.detach().numpy().astype(np.float64) for k, g in zip(names, got)}
    if image is None:
        return grads, None
    ops, zy = {}, got[len(names):]
    for i, b in enumerate(blocks):
        b = dict(b, index=i)
        for red, (Y, U) in reduction_operands(st, cfg, b, (zy[2 * i], zy[2 * i + 1]), image).items():
            ops[ffn_names(i)[red]] = (Y, U, red in ("dA2", "dA1"))
    return grads, ops


def abs_addends(Y, U, transposed):
    """sum_m |Y[m, n] U[m, j]| elementwise, as a float64 numpy array in the gradient's layout."""
    return reduce_rows(Y.abs(), U.abs(), transposed).numpy().astype(np.float64)


def rel_fro(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


def cosine(a, ref):
    a, ref = np.asarray(a, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel()
    return float(a @ ref / (np.linalg.norm(a) * np.linalg.norm(ref)))


def probe(cfg, batch):
    """The fixed probe of the placement tests: one image with its label and its upstream row (dlogits [1, classes], demb [1, dim]), scaled
    as a row of a batch of `batch` images."""
    return (recipe.make_images(cfg, 1, seed=31, tag="probe"), recipe.make_labels(cfg, 1, seed=31, tag="probe_label"),
            recipe.normalish("probe_dlogits", (1, cfg["num_class"]), 31) / np.float32(batch),
            recipe.normalish("probe_demb", (1, cfg["dim"]), 31) / np.float32(batch))


def upstream(cfg, batch, seed=3):
    """The seeded f32 upstream gradients (dlogits [B, classes], demb [B, dim]) of a batch, divided by the batch."""
    return (recipe.normalish("dlogits", (batch, cfg["num_class"]), seed) / np.float32(batch),
            recipe.normalish("demb", (batch, cfg["dim"]), seed) / np.float32(batch))
