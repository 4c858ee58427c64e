"""Adversarial attention inputs and their float64 reference (tests/test_attention_probes_host.py, tests/test_hip_attention_edges.py).

Random inputs hide the faults an attention kernel is most likely to have: a padded key that leaks into the softmax weighs e^-lse, a
dropped last key or two swapped V rows move the output by a rounding error. Each probe here turns one such fault into an error of
order 1. Every builder is deterministic (its own torch.Generator) and returns f32 CPU tensors qkv [B*T, 3*H*64] (token-major) and
d_o [B*T, H*64]; the caller rounds them to the dtype under test and the reference sees the rounded values.

  neg      q = 8u + n/2, k = -8u + n/2, v = 1 + n (u: a unit vector per image and head): every real score is about -8, so a key of
           score 0 (a zero K row that escaped the tail mask) dominates the softmax.
  pos      q = k = 27u + 0.15 n: every scaled score is about +91, so exp(score) overflows f32 unless the row maximum is subtracted.
  spike    key j = 4 x the sum of the chosen queries {0, T//2, T-1} (orthogonal, length 4): those rows put all their weight on key j.
  uniform  q = 0: lse = log T, o = mean V, dV = mean dO, dK = 0, dQ in closed form — no reference needed.
"""
import math

import torch

HD = 64
SCALE = HD ** -0.5
POS_C = 27.0
SPIKE_BOOST = 4.0
SPIKE_GAP = 4.0
PROBES = ("neg", "pos", "uniform", "spike_last", "spike_first", "spike_tile", "spike_tile_m1")


def _gen(tag, B, T, H):
    return torch.Generator().manual_seed(7919 * PROBES.index(tag) + 1000003 * B + 1009 * T + H)


def _unit(g, B, H):
    u = torch.randn(B, 1, H, HD, generator=g)
    return u / u.norm(dim=-1, keepdim=True)


def _directed(tag, B, T, H, cq, ck, noise, g_mean, g_amp):
    g = _gen(tag, B, T, H)
    u = _unit(g, B, H)
    x = torch.randn(B, T, 3, H, HD, generator=g)
    x[:, :, 0].mul_(noise).add_(cq * u)
    x[:, :, 1].mul_(noise).add_(ck * u)
    x[:, :, 2].add_(1.0)
    return x.view(B * T, 3 * H * HD), (torch.randn(B * T, H * HD, generator=g) + g_mean) * g_amp


# The output gradients of neg / pos are sized by the backward's conditioning in bf16 (tests/test_attention_probes_host.py): `o` reaches the
# backward rounded to 16 bits, so delta = rowsum(dO o) carries |dO| x 8 half-ulps of o, and dQ multiplies that by the common component of
# the keys (8 or 27). neg: dO = 0.4 (1 + n) keeps a correct kernel within half of the dQ bound and the pad-leak mutant 10x outside the
# dK / dV bounds. pos: its noise is 0.15 n (scores spread like those of neg: sigma about 0.75 — at 0.5 n the softmax is so peaked that
# dP - delta is a difference of nearly equal numbers) and dO = n / 8; it has no backward mutant, it is there for the overflow.
def neg(B, T, H):
    return _directed("neg", B, T, H, 8.0, -8.0, 0.5, 1.0, 0.4)


def pos(B, T, H):
    return _directed("pos", B, T, H, POS_C, POS_C, 0.15, 0.0, 0.125)


def spike_queries(T):
    return sorted({0, T // 2, T - 1})


def spike_key(tag, T):
    """spike_last: the last key; spike_first: key 0; spike_tile / spike_tile_m1: the first key of the last 16-key tile and the key
    before it (None when T <= 16: there is no such tile)."""
    tile = 16 * ((T - 1) // 16)
    j = {"spike_last": T - 1, "spike_first": 0, "spike_tile": tile, "spike_tile_m1": tile - 1}[tag]
    return j if (tag in ("spike_last", "spike_first") or T > 16) else None


def spike(B, T, H, j, tag="spike_last"):
    g = _gen(tag, B, T, H)
    x = torch.randn(B, T, 3, H, HD, generator=g) * 0.5
    qi = spike_queries(T)
    # the chosen queries: orthogonal directions (their cross terms would eat into the gap), length 4
    d = torch.linalg.qr(x[:, qi, 0].permute(0, 2, 3, 1).double()).Q.float()         # [B, H, 64, nq]
    x[:, qi, 0] = 4.0 * d.permute(0, 3, 1, 2)
    x[:, j, 1] = SPIKE_BOOST * x[:, qi, 0].sum(1)
    s = torch.einsum("bihd,bjhd->bhij", x[:, qi, 0], x[:, :, 1]) * SCALE
    if T > 1:
        top2 = s.topk(2, -1).values
        assert (s.argmax(-1) == j).all() and ((top2[..., 0] - top2[..., 1]) >= SPIKE_GAP).all(), (T, j, (top2[..., 0] - top2[..., 1]).min())
    # the chosen rows' softmax is saturated: their dQ is delta's rounding error (|dO| x 8 half-ulps of the 16-bit o) times |k_j| = 28, so
    # their dO is a quarter of the others' (tests/test_attention_probes_host.py holds a correct bf16 kernel within half of the dQ bound)
    d_o = torch.randn(B, T, H * HD, generator=g)
    d_o[:, qi] *= 0.25
    return x.view(B * T, 3 * H * HD), d_o.view(B * T, H * HD)


def uniform(B, T, H):
    g = _gen("uniform", B, T, H)
    x = torch.randn(B, T, 3, H, HD, generator=g)
    x[:, :, 0] = 0.0
    return x.view(B * T, 3 * H * HD), torch.randn(B * T, H * HD, generator=g)


def make(tag, B, T, H):
    """(qkv, d_o) of the probe `tag`, or None where the probe does not exist at this T (spike_tile* at T <= 16)."""
    if tag == "neg":
        return neg(B, T, H)
    if tag == "pos":
        return pos(B, T, H)
    if tag == "uniform":
        return uniform(B, T, H)
    j = spike_key(tag, T)
    return None if j is None else spike(B, T, H, j, tag)


# ---------------------------------------------------------------------------------------------------------------- float64 reference
def split(qkv, B, T, H):
    """q, k, v [B, H, T, 64] in float64 (on the device of qkv)."""
    return qkv.double().view(B, T, 3, H, HD).permute(2, 0, 3, 1, 4)


def forward(q, k, v, scale):
    """o [B, H, Tq, 64], lse [B, H, Tq], P [B, H, Tq, Tk]."""
    s = torch.einsum("bhid,bhjd->bhij", q, k) * scale
    lse = s.logsumexp(-1)
    p = (s - lse[..., None]).exp()
    return p @ v, lse, p


def backward(q, k, v, p, d_o, scale):
    """dq, dk, dv of o = softmax(scale q k^T) v under the output gradient d_o [B, H, Tq, 64], written out (no autograd)."""
    dv = p.transpose(-1, -2) @ d_o
    dp = d_o @ v.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    return scale * (ds @ k), scale * (ds.transpose(-1, -2) @ q), dv


def merge_heads(x, B, T, H):
    return x.permute(0, 2, 1, 3).reshape(B * T, H * HD)


def reference(qkv, d_o, B, T, H, scale, chunk=16):
    """float64 o [B*T, H*64], lse [B, H, T], dqkv [B*T, 3*H*64] of the values given, on their device, `chunk` images at a time."""
    os_, ls, gs = [], [], []
    for b0 in range(0, B, chunk):
        n = min(chunk, B - b0)
        q, k, v = split(qkv[b0 * T:(b0 + n) * T], n, T, H)
        g = d_o[b0 * T:(b0 + n) * T].double().view(n, T, H, HD).permute(0, 2, 1, 3)
        o, lse, p = forward(q, k, v, scale)
        dq, dk, dv = backward(q, k, v, p, g, scale)
        os_.append(merge_heads(o, n, T, H))
        ls.append(lse)
        gs.append(torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(n * T, 3 * H * HD))
    return torch.cat(os_), torch.cat(ls), torch.cat(gs)


def uniform_closed_form(qkv, d_o, B, T, H, scale):
    """The q = 0 probe without a softmax: (o, lse, dqkv) from means alone (P = 1/T)."""
    _, k, v = split(qkv, B, T, H)
    g = d_o.double().view(B, T, H, HD).permute(0, 2, 1, 3)
    o = v.mean(2, keepdim=True).expand(-1, -1, T, -1)
    lse = torch.full((B, H, T), math.log(T), dtype=torch.float64, device=qkv.device)
    dv = g.mean(2, keepdim=True).expand(-1, -1, T, -1)
    dp = g @ v.transpose(-1, -2)                                    # dP_ij = dO_i . v_j
    dq = scale * ((dp - dp.mean(-1, keepdim=True)) / T) @ k         # delta_i = mean_j dP_ij
    dqkv = torch.stack([dq, torch.zeros_like(dq), dv], 0).permute(1, 3, 0, 2, 4).reshape(B * T, 3 * H * HD)
    return merge_heads(o, B, T, H), lse, dqkv


def to_head_major(qkv, B, T, H):
    return qkv.view(B, T, 3, H, HD).permute(0, 3, 2, 1, 4).contiguous().view(B * T, 3 * H * HD)
