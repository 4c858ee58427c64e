"""ViTRunner at the geometries of tests/geometry_cases.py: every LayerNorm width (64 .. 1024, so 1 .. 16 heads), depth 1, T = 2, batch 1,
ranks 1 2 3 5 7 16 21, mlp widths off a multiple of 256, one channel, patch dimensions 64 and 256 — shapes the runner accepts and no test
ran. tests/test_geometry_sweep_host.py proves the float64 reference against the oracle at every row and shows six fault models that the
four earlier fixtures cannot see far above the bounds used here.

One test per (case, mode): the runner is driven directly (forward(save=True), backward(saved, dlogits, demb)) and logits, emb and every
LoRA gradient are compared with float64. No bound is tuned to the output:
  fp32, fp32x3   per tensor e_gpu(t) <= C_F32 max_t' e_cpu(t'), e = relative Frobenius error against float64, e_cpu that of the float32 CPU run
                 of the same reference, measured here; C_F32 = 4 of tests/test_hip_large_rows.py. The maximum over the case's tensors
                 (logits and emb included) replaces a per-tensor e_cpu: a 64-element tensor at rank 1 can land on a lucky small one.
  bf16, fp16     gradients: GRAD_BAND of tests/test_hip_bf16_pinned.py (relative Frobenius, cosine); logits and emb: the absolute bars 0.25 and
                 0.05 of test_forward_bf16_close_to_reference.
Every e_gpu / bound ratio is printed (pytest -s); profiles/geometry_sweep.md has the worst per case and mode.

Further: dropout 0.1 against the mask-injected reference at widths 256 and 1024; determinism and independence from the other images of
a batch; HIP-graph replay against the eager step; the eval-mode merge and its round trip; a width outside the ladder (dim 192) fails at
its first forward with the library's message and leaves the process usable."""
import copy

import numpy as np
import pytest
import torch

import geometry_cases as G
import large_row_reference as LR
from test_hip_bf16_pinned import GRAD_BAND
from test_hip_large_rows import C_F32, U24

pytestmark = pytest.mark.gpu

MODES = ("fp32", "fp32x3", "bf16", "fp16")
LOGITS_BAR, EMB_BAR = 0.25, 0.05      # test_forward_bf16_close_to_reference (tests/test_hip_model.py): max |difference|, 16-bit modes
DROP_CALLS = 41


def run(m, img, y, dlogits, demb, drop_calls=None):
    """One forward(save=True) + backward of the runner -> dict(logits, emb, grads) as float64 numpy, and the dropout seed of the pass."""
    r = m.runner()
    params = {n: p for n, p in m.named_parameters() if p.requires_grad}
    for p in params.values():
        p.grad = None      # a fresh gradient bucket: attach_grads() zeroes it
    if drop_calls is not None:
        r.drop_calls = drop_calls
    cu = lambda a: torch.as_tensor(a).cuda()
    logits, emb, saved = r.forward(cu(img), cu(y), save=True)
    seed = (r.drop_seed << 20) + r.drop_calls
    r.backward(saved, cu(dlogits), cu(demb))
    torch.cuda.synchronize()
    f64 = lambda t: t.detach().float().cpu().numpy().astype(np.float64)
    return dict(logits=f64(logits), emb=f64(emb), grads={n: f64(p.grad) for n, p in params.items()}), seed


def check(tag, got, ref, mode, e_cpu):
    """The bounds of the module docstring on one run. -> the worst e_gpu / bound ratio."""
    worst = 0.0

    def ratio(what, value, bound):
        nonlocal worst
        worst = max(worst, value / bound)
        print(f"RATIO [{tag} {mode}] {what}: {value:.3e} / {bound:.3e} = {value / bound:.3f}")
        return value <= bound

    short = lambda k: k.split("layers.")[1] if "layers." in k else k
    assert set(got["grads"]) == set(ref["grads"])
    failed = []
    if mode in ("fp32", "fp32x3"):
        bound = C_F32 * max(e_cpu.values())
        for k, r in G.tensors(ref).items():
            if not ratio(short(k), LR.rel_fro(G.tensors(got)[k], r), bound):
                failed.append(k)
    else:
        for k, bar in (("logits", LOGITS_BAR), ("emb", EMB_BAR)):
            if not ratio(k, float(np.abs(got[k] - ref[k]).max()), bar):
                failed.append(k)
        for k, r in ref["grads"].items():
            cos = LR.cosine(got["grads"][k], r)
            ok = ratio(short(k), LR.rel_fro(got["grads"][k], r), GRAD_BAND[mode][0])
            if not (ok and ratio(short(k) + " 1-cos", 1.0 - cos, 1.0 - GRAD_BAND[mode][1])):
                failed.append(k)
    print(f"WORST [{tag} {mode}] {worst:.3f}")
    assert not failed, (tag, mode, failed)
    return worst


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(G.CASES))
def test_case_against_float64(name, mode):
    cfg, B = G.CASES[name]
    ref, e_cpu = G.reference(name), G.cpu_errors(name)
    assert all(e > 0 for e in e_cpu.values())
    torch.manual_seed(0)
    got, _ = run(G.build(cfg, mode), *G.inputs(cfg, B))
    for k, g in got["grads"].items():
        assert np.isfinite(g).all(), k
    check(name, got, ref, mode, e_cpu)


def test_token_major_qkv_with_layernorm_1_folded_in(monkeypatch):
    """fp16 folds LayerNorm 1 into the QKV GEMM (EPI_STORE_LN). Below 8 tokens the runner takes the token-major layout by itself (the d*_odd,
    d1024_t2 and d1024_attn rows above); here the same form at T = 10 through the QKV_HEAD_MAJOR knob, which no test had combined with the
    fold: the GEMM was handed T, which the token-major STORE_LN reads as the row stride of mean / rstd."""
    from gslora_hip import vit_runner
    name = "d256_batchable"
    cfg, B = G.CASES[name]
    assert G.tokens(cfg) >= vit_runner.QKV_HM_MIN_T and vit_runner.LN1_FOLD
    torch.manual_seed(0)
    m = G.build(cfg, "fp16")
    head_major, _ = run(m, *G.inputs(cfg, B))
    monkeypatch.setattr(vit_runner, "QKV_HEAD_MAJOR", False)
    token_major, _ = run(m, *G.inputs(cfg, B))
    check(name + " token-major", token_major, G.reference(name), "fp16", G.cpu_errors(name))
    same = all(np.array_equal(t, G.tensors(head_major)[k]) for k, t in G.tensors(token_major).items())
    print(f"[{name} fp16] token-major and head-major runs bit-identical: {same}")


# ---------------------------------------------------------------------------------------------------------------- dropout
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["d256_batchable", "d1024_sq"])
def test_dropout_against_the_mask_injected_reference(name, mode):
    """p = 0.1 at widths 256 and 1024: the 4-wide counter path of the LayerNorm backward's dropout copy at row lengths no model ran. The masks
    are gsl_dropout_mask at the run's seed and the runner's sites, injected into the float64 forward (and into its float32 run for e_cpu)."""
    from gslora_hip import ops
    cfg, B = G.CASES[name]
    p = 0.1
    torch.manual_seed(0)
    got, seed = run(G.build(cfg, mode, dropout=p), *G.inputs(cfg, B), drop_calls=DROP_CALLS)
    masks = {}

    def keep(n, site):
        if (n, site) not in masks:
            masks[n, site] = ops.dropout_mask(n, p, seed, site, "cuda").cpu().double() / (1 - p)
        return masks[n, site]

    dropped = float((keep(B * G.tokens(cfg) * cfg["dim"], LR.SITE_EMB) == 0).double().mean())
    assert abs(dropped - p) < 0.03, dropped
    key = ("dropout", seed)
    ref = G.reference(name, keep, key)
    assert LR.rel_fro(ref["emb"], G.reference(name)["emb"]) > 0.01      # the masks are in the reference
    check(name + " dropout", got, ref, mode, G.cpu_errors(name, keep, key))


# ---------------------------------------------------------------------------------------------------------------- determinism, independence
@pytest.mark.parametrize("name", ["d1024_t2", "d256_odd"])
def test_runs_are_bit_identical_and_images_independent(name):
    """bf16. Two identical runs: the same bits. A batch in which every image but one has an upstream row of exactly zero: the gradients of the
    one-image run of that image, within the placement bound of tests/test_hip_large_rows.py (a): 2.2 N 2^-24 sum|addends| per element, N = T
    rows per reduction (1 in a cls-row-only last block) — the forward rows of the image do not depend on its neighbours, the zero rows add
    exact zeros, and what is left is the order of an f32 sum of N addends."""
    cfg, B = G.CASES[name]
    T = G.tokens(cfg)
    img, lab, dl, de = G.inputs(cfg, B)
    torch.manual_seed(0)
    m = G.build(cfg, "bf16")
    a, _ = run(m, img, lab, dl, de)
    b, _ = run(m, img, lab, dl, de)
    for k, t in G.tensors(a).items():
        assert np.array_equal(t, G.tensors(b)[k]), k
    pos = B - 1
    dl1, de1 = np.zeros_like(dl), np.zeros_like(de)
    dl1[pos], de1[pos] = dl[pos], de[pos]
    batch, _ = run(m, img, lab, dl1, de1)
    one = (img[pos:pos + 1], lab[pos:pos + 1], dl[pos:pos + 1], de[pos:pos + 1])
    alone, _ = run(m, *one)
    print(f"[{name} independence] logits / emb of the image alone and in the batch bit-identical: "
          f"{np.array_equal(batch['logits'][pos], alone['logits'][0])} / {np.array_equal(batch['emb'][pos], alone['emb'][0])}")
    _, operands = LR.lora_gradients(cfg, *one, image=0)
    last = f"layers.{cfg['depth'] - 1}."
    worst = 0.0
    for k, g in batch["grads"].items():
        n = 1 if (last in k and cfg.get("pool", "cls") == "cls") else T
        bound = 2.2 * n * U24 * LR.abs_addends(*operands[k])
        d = np.abs(g - alone["grads"][k])
        assert np.linalg.norm(alone["grads"][k]) > 0
        worst = max(worst, float((d / bound).max()))
        print(f"RATIO [{name} independence] {k.split('layers.')[1]}: worst |difference| / bound {float((d / bound).max()):.3f}")
        assert (d <= bound).all(), (k, float((d / bound).max()))
    print(f"WORST [{name} independence] {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------- graph replay
@pytest.mark.parametrize("name", ["d256_batchable", "d1024_min"])
def test_graph_replay_is_the_eager_step(name):
    """GraphedStep against gs_lora_step on a twin model, fp16, dropout 0.1, in the pattern of tests/test_hip_graph.py: the packed meters and
    every LoRA parameter bit-identical over an eager first step, the capture and three replays."""
    from gslora_hip.optim import FusedAdamW
    from gslora_hip.step import GraphedStep, gs_lora_step
    from test_hip_graph import batch
    cfg, B = G.CASES[name]
    torch.manual_seed(0)
    m1 = G.build(cfg, "fp16", dropout=0.1)
    m2 = copy.deepcopy(m1)
    mk_opt = lambda m: FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)
    o1, o2 = mk_opt(m1), mk_opt(m2)
    crit = torch.nn.CrossEntropyLoss()
    kw = dict(beta=0.15, alpha=1e-2, BND=105.0, use_structure=True, group_type="block")
    g = GraphedStep(m2, o2, crit)
    for s in range(5):
        data = batch(cfg, B, s)
        p1 = gs_lora_step(m1, o1, crit, *data, **kw)
        p2 = g(*data, **kw)
        assert torch.isfinite(p1).all() and torch.equal(p1, p2), (s, p1.tolist(), p2.tolist())
        for (n, a), (_, c) in zip(m1.named_parameters(), m2.named_parameters()):
            if a.requires_grad:
                assert torch.equal(a, c), (s, n)
    assert (g.eager_steps, g.captures, g.replays) == (1, 1, 4)


# ---------------------------------------------------------------------------------------------------------------- eval-mode merge
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["d1024_min", "d256_attn"])
def test_merged_logits_hold_the_train_mode_bound_and_train_unmerges(name, mode):
    """eval() merges W += B A / r (loralib), the forward then runs the plain GEMMs: the logits hold the bound of the train-mode logits against
    the same float64 reference. train() un-merges with W -= B A / r. That is loralib's float32 arithmetic, not a restore: (W + d) - d is W up
    to one rounding of W + d and one of the difference, |W' - W| <= 2^-24 (|W + d| + |W'|), which is asserted per element together with
    the adapters' own bits; on the CPU 0.6 % .. 0.8 % of the elements of these weights (some hundred per matrix) come back one unit in the last place off, so
    bit-identical logits are not a property of the merge. The round-trip logits hold the train-mode bound, and a second forward of the
    un-merged model repeats the first bit for bit."""
    cfg, B = G.CASES[name]
    img, lab, _, _ = G.inputs(cfg, B)
    ref, e_cpu = G.reference(name), G.cpu_errors(name)
    torch.manual_seed(0)
    m = G.build(cfg, mode)
    cu = lambda a: torch.as_tensor(a).cuda()

    def logits_of():
        with torch.no_grad():
            lo, em = m(cu(img), cu(lab))
        return lo.float().cpu().numpy().astype(np.float64), em.float().cpu().numpy().astype(np.float64)

    def holds(tag, lo, em):
        if mode == "fp32":
            bound = C_F32 * max(e_cpu.values())
            vals = [("logits", LR.rel_fro(lo, ref["logits"]), bound), ("emb", LR.rel_fro(em, ref["emb"]), bound)]
        else:
            vals = [("logits", float(np.abs(lo - ref["logits"]).max()), LOGITS_BAR), ("emb", float(np.abs(em - ref["emb"]).max()), EMB_BAR)]
        for what, v, b in vals:
            print(f"RATIO [{name} {mode} {tag}] {what}: {v:.3e} / {b:.3e} = {v / b:.3f}")
            assert v <= b, (tag, what, v, b)

    adapted = {n: p.detach().clone() for n, p in m.named_parameters() if "lora_" not in n and (".net." in n or "to_qkv" in n) and n.endswith("weight")}
    lora = {n: p.detach().clone() for n, p in m.named_parameters() if "lora_" in n}
    before = logits_of()
    holds("train", *before)
    m.eval()
    merged = {n: p.detach().clone() for n, p in m.named_parameters() if n in adapted}
    changed = [n for n in adapted if not torch.equal(merged[n], adapted[n])]
    assert len(changed) == (1 if cfg.get("lora_pos") == "Attention" else 2) * cfg["depth"], changed
    holds("eval", *logits_of())
    m.train()
    for n, p in m.named_parameters():
        if n in lora:
            assert torch.equal(p, lora[n]), n
        if n in adapted:
            slack = 2.0 ** -24 * (merged[n].abs() + p.detach().abs())
            assert ((p.detach() - adapted[n]).abs() <= slack).all(), n
    after = logits_of()
    holds("round trip", *after)
    again = logits_of()
    assert np.array_equal(after[0], again[0]) and np.array_equal(after[1], again[1])


# ---------------------------------------------------------------------------------------------------------------- a width outside the ladder
def test_unsupported_width_fails_at_the_first_forward_and_leaves_the_process_usable():
    """dim 192 passes the constructor (192 % 64 == 0) and is no width of ln_for_width: the first forward raises with the library's text,
    in every mode, before and after a backward-capable call; a supported model built afterwards runs and passes its bound."""
    cfg = dict(G.CASES["d256_min"][0], dim=192, heads=3)
    B = 2
    img, lab, dl, de = G.inputs(cfg, B)
    for mode in ("fp16", "fp32"):
        m = G.build(cfg, mode)
        with pytest.raises(RuntimeError, match="unsupported LayerNorm width 192"):
            with torch.no_grad():
                m(torch.as_tensor(img).cuda(), torch.as_tensor(lab).cuda())
        with pytest.raises(RuntimeError, match="unsupported LayerNorm width 192"):
            run(m, img, lab, dl, de)
        torch.cuda.synchronize()
    name = "d256_min"
    good, gB = G.CASES[name]
    torch.manual_seed(0)
    got, _ = run(G.build(good, "fp32"), *G.inputs(good, gB))
    check(name + " after the refusal", got, G.reference(name), "fp32", G.cpu_errors(name))
