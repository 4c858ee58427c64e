"""The fp32x3 mode on the GPU: GSL_F32X3 (f32 tensors, every product as three bf16 pieces per operand on the bf16 matrix cores, six products) against
a float64 product with two yardsticks that are not the code under test — the exact-f32 kernel on the same operands and the host emulation of the
five-product set —, every f32 epilogue, non-finite operands, determinism, and the model / engine / evaluation layers at the bars of the f32 tests."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import recipe

pytestmark = pytest.mark.gpu

SHAPES = [(64, 128, 64, 0),        # one tile, two K tiles
          (130, 192, 64, 64),      # ragged M and N, the segment switch
          (394, 384, 128, 0),
          (256, 512, 512, 64)]
FAMILIES = ["uniform", "wide"]     # uniform [-1, 1) and randn * exp(4 randn)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    from gslora_hip import _lib, ops as _ops
    _lib.load()
    return _ops


def operands(family, rows, K, seed):
    g = torch.Generator().manual_seed(seed)
    if family == "uniform":
        return torch.rand(rows, K, generator=g) * 2 - 1
    return torch.randn(rows, K, generator=g) * torch.exp(4 * torch.randn(rows, K, generator=g))


def gemm(ops, A, W, K1, mode, **kw):
    """[A1 | A2] [W1 | W2]^T through gsl_gemm_nt, f32 output; A, W on the host, split at K1."""
    from gslora_hip import _lib as L
    Ad, Wd = A.cuda(), W.cuda()
    seg = dict(A2=Ad[:, K1:].contiguous(), W2=Wd[:, K1:].contiguous()) if A.shape[1] > K1 else {}
    out = torch.empty(A.shape[0], W.shape[0], device="cuda")
    kw.setdefault("epilogue", L.EPI_STORE_F32)
    return ops.gemm_nt(Ad[:, :K1].contiguous(), Wd[:, :K1].contiguous(), out, f32_mode=mode, **seg, **kw)


def ref64(A, W):
    a, w = A.double().numpy(), W.double().numpy()
    return a @ w.T, np.abs(a) @ np.abs(w).T


# ------------------------------------------------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("M,N,K1,K2", SHAPES)
def test_gemm_accuracy_against_f64_with_the_f32_kernel_and_five_products_as_yardsticks(ops, M, N, K1, K2, family):
    """e(out) = max |out - ref64| / (|A| |W|^T). Required: e_x3 <= 4 e_f32 (the product set itself contributes about a tenth of the f32 chain's
    rounding; the rest of the allowance is for what the bf16 MFMA's accumulator adds) and e_x3 <= 0.5 e_five (a missing product shows at 7 - 20 x
    e_f32 at K = 64). Measured ratios: profiles/f32x3.md."""
    A, W = operands(family, M, K1 + K2, 1), operands(family, N, K1 + K2, 2)
    ref, scale = ref64(A, W)
    err = lambda o: float((np.abs(o - ref) / scale).max())
    e_f32 = err(gemm(ops, A, W, K1, None).double().cpu().numpy())
    e_x3 = err(gemm(ops, A, W, K1, "x3").double().cpu().numpy())
    e_five = err(ops.f32x3_product_reference(A.numpy(), W.numpy(), ops.F32X3_FIVE))
    print(f"({M},{N},{K1},{K2}) {family}: e_f32 {e_f32:.3e} e_x3 {e_x3:.3e} e_five {e_five:.3e}  x3/f32 {e_x3 / e_f32:.3f}  x3/five {e_x3 / e_five:.4f}")
    assert e_x3 <= 4 * e_f32
    assert e_x3 <= 0.5 * e_five


def test_small_shapes_take_the_exact_f32_kernel(ops):
    """N < 128 or M < 64: GSL_F32X3 runs the VALU f32 kernel — the bits of GSL_F32."""
    for M, N in ((130, 64), (48, 256)):
        A, W = operands("uniform", M, 128, 3), operands("uniform", N, 128, 4)
        assert torch.equal(gemm(ops, A, W, 64, None), gemm(ops, A, W, 64, "x3"))


# ------------------------------------------------------------------------------------------------------------ 2. epilogues
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + 1000 * len(shape) + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def relerr(a, b):
    return (a - b).abs().max().item() / max(1e-12, b.abs().max().item())


@pytest.mark.parametrize("M,N,K1,K2", [(591, 192, 128, 64), (257, 2048, 512, 64)])
def test_every_f32_epilogue(ops, M, N, K1, K2):
    """The list tests/test_hip_ops.py::test_gemm_epilogues walks in f32, against the same host evaluation with that test's f32 tolerances."""
    from gslora_hip import _lib as L
    A1, W1 = rnd(M, K1, seed=1), rnd(N, K1, seed=2, scale=K1 ** -0.5)
    A2, W2 = rnd(M, K2, seed=3), rnd(N, K2, seed=4, scale=0.1)
    A2[:, 8:] = 0
    bias, res, aux = rnd(N, seed=5), rnd(M, N, seed=6), rnd(M, N, seed=7)
    acc = A1 @ W1.t() + A2 @ W2.t()
    c = lambda t: t.cuda()
    kw = dict(A2=c(A2), W2=c(W2), f32_mode="x3")
    out, outf = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
    ops.gemm_nt(c(A1), c(W1), out, alpha=0.5, bias=c(bias), **kw)                                      # STORE with alpha + bias
    assert relerr(out.cpu(), 0.5 * acc + bias) < 2e-5
    ops.gemm_nt(c(A1), c(W1), outf, epilogue=L.EPI_STORE_F32, **kw)
    assert relerr(outf.cpu(), acc) < 2e-5
    ops.gemm_nt(c(A1), c(W1), outf, epilogue=L.EPI_BIAS_RES_F32, bias=c(bias), res=c(res), **kw)
    assert relerr(outf.cpu(), acc + bias + res) < 2e-5
    out2 = torch.empty(M, N, device="cuda")
    ops.gemm_nt(c(A1), c(W1), out, epilogue=L.EPI_BIAS_GELU, bias=c(bias), out2=out2, **kw)           # BIAS_GELU (+ derivative)
    a = (acc + bias).requires_grad_(True)
    g = F.gelu(a)
    gp, = torch.autograd.grad(g.sum(), a)
    assert (out.cpu() - g.detach()).abs().max() < 2e-5 and (out2.cpu() - gp).abs().max() < 2e-5
    ops.gemm_nt(c(A1), c(W1), out, epilogue=L.EPI_MUL, aux=c(aux), **kw)
    assert relerr(out.cpu(), acc * aux) < 2e-5
    T = 197 if M % 197 == 0 else 13 if M % 13 == 0 else M                                             # PATCH
    pos, cls = rnd(T, N, seed=8), rnd(N, seed=9)
    ops.gemm_nt(c(A1), c(W1), outf, epilogue=L.EPI_PATCH, bias=c(bias), pos=c(pos), cls=c(cls), T=T, **kw)
    tok = torch.arange(M) % T
    assert relerr(outf.cpu(), torch.where((tok == 0)[:, None], cls[None, :].expand(M, N), acc + bias) + pos[tok]) < 2e-5


def test_dropout_epilogues_keep_the_f32_kernels_masks(ops):
    """Residual and GELU epilogues with p = 0.25: the kept / dropped pattern is the f32 kernel's (and gsl_dropout_mask's), dropped elements are
    exactly 0, kept ones meet the f32 tolerance."""
    from gslora_hip import _lib as L
    M, N, K = 256, 128, 64
    A, W, bias = rnd(M, K).cuda(), rnd(N, K).cuda(), rnd(N).cuda()
    zero = torch.zeros(M, N, device="cuda")
    keep = ops.dropout_mask(M * N, 0.25, 77, 5, "cuda").reshape(M, N).bool()
    got = {}
    for mode in (None, "x3"):
        o = torch.empty(M, N, device="cuda")
        ops.gemm_nt(A, W, o, epilogue=L.EPI_BIAS_RES_F32, bias=bias, res=zero, p_drop=0.25, seed=77, site=5, f32_mode=mode)
        h, gp = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
        ops.gemm_nt(A, W, h, epilogue=L.EPI_BIAS_GELU, bias=bias, out2=gp, p_drop=0.25, seed=77, site=5, f32_mode=mode)
        got[mode] = (o, h, gp)
    for t32, t3 in zip(got[None], got["x3"]):
        assert torch.equal(t32 == 0, t3 == 0)
        assert relerr(t3.cpu(), t32.cpu()) < 2e-5
    assert torch.equal(got["x3"][0] != 0, keep) and (got["x3"][2][~keep] == 0).all() and (got["x3"][1][~keep] == 0).all()
    ref = (A.cpu() @ W.cpu().t() + bias.cpu()) * keep.cpu().float() / 0.75
    assert relerr(got["x3"][0].cpu(), ref) < 2e-5


# ------------------------------------------------------------------------------------------------------------ 3. non-finite operands
@pytest.mark.parametrize("M,N,K1,K2", [(130, 192, 64, 64), (256, 512, 512, 64)])
def test_non_finite_operands_do_not_vanish(ops, M, N, K1, K2):
    """One NaN and one Inf in A and in W, in the first and the last K tile (the last one lies in the K2 segment): whatever the exact-f32 kernel
    turns non-finite is non-finite here, and every other element still meets the bounds of the accuracy test."""
    K = K1 + K2
    A, W = operands("uniform", M, K, 11), operands("uniform", N, K, 12)
    A[3, 5], A[M - 2, K - 3] = float("nan"), float("inf")
    W[7, 2], W[N - 5, K - 30] = float("inf"), float("nan")
    o32, o3 = gemm(ops, A, W, K1, None).cpu(), gemm(ops, A, W, K1, "x3").cpu()
    bad32, bad3 = ~torch.isfinite(o32), ~torch.isfinite(o3)
    expect = torch.zeros(M, N, dtype=torch.bool)
    expect[[3, M - 2], :] = True
    expect[:, [7, N - 5]] = True
    assert torch.equal(bad32, expect)                      # (the yardstick sees what the test planted)
    assert bad3[bad32].all()
    assert torch.equal(bad3, expect)                       # ... and nothing else is touched
    Af, Wf = torch.nan_to_num(A, 0.0, 0.0, 0.0), torch.nan_to_num(W, 0.0, 0.0, 0.0)      # the finite rows and columns never met the planted values
    ref, scale = ref64(Af, Wf)
    ok = (~expect).numpy()
    err = lambda o: float((np.abs(o.double().numpy() - ref) / scale)[ok].max())
    e_five = float((np.abs(ops.f32x3_product_reference(Af.numpy(), Wf.numpy(), ops.F32X3_FIVE) - ref) / scale)[ok].max())
    assert err(o3) <= 4 * err(o32) and err(o3) <= 0.5 * e_five


def test_the_largest_finite_values_split_exactly(ops):
    """|x| >= 2^128 - 2^119 would round hi up to Inf; the kernel's conversion saturates (FP16_OVFL), as the header says: such elements are ordinary
    operands, their rows and columns stay finite and meet the bounds of the accuracy test."""
    M, N, K1, K2 = 130, 192, 64, 64
    A, W = operands("uniform", M, K1 + K2, 13), operands("uniform", N, K1 + K2, 14) * 0.5
    fmax = torch.finfo(torch.float32).max
    A[9, 40], A[77, 100], A[120, 3] = fmax, -fmax, float(np.float32(2.0 ** 127) * np.float32(2.0 - 2.0 ** -8))
    ref, scale = ref64(A, W)
    o32, o3 = gemm(ops, A, W, K1, None).cpu(), gemm(ops, A, W, K1, "x3").cpu()
    assert torch.isfinite(o32).all() and torch.isfinite(o3).all()
    err = lambda o: float((np.abs(o.double().numpy() - ref) / scale).max())
    e_five = float((np.abs(ops.f32x3_product_reference(A.numpy(), W.numpy(), ops.F32X3_FIVE) - ref) / scale).max())
    print(f"largest finite values: e_f32 {err(o32):.3e} e_x3 {err(o3):.3e} e_five {e_five:.3e}")
    assert err(o3) <= 4 * err(o32) and err(o3) <= 0.5 * e_five


# ------------------------------------------------------------------------------------------------------------ 4. determinism
def test_the_same_call_twice_is_bit_identical(ops):
    M, N, K1, K2 = 394, 384, 128, 64
    A, W = operands("wide", M, K1 + K2, 21), operands("wide", N, K1 + K2, 22)
    a, b = gemm(ops, A, W, K1, "x3"), gemm(ops, A, W, K1, "x3")
    assert torch.equal(a, b)
    assert not torch.equal(a, gemm(ops, A, W, K1, None))      # (it is not the fmaf chain: the mode is live)


def test_graph_replay_of_the_step_is_bit_identical_to_eager():
    from gslora_hip.optim import FusedAdamW
    from gslora_hip.step import GraphedStep, gs_lora_step
    from test_hip_graph import batch, build
    cfg, b = recipe.cfg_small2(), 6
    m1 = build(cfg, "fp32x3", 0.1)
    m2 = copy.deepcopy(m1)
    assert m2.compute_mode == "fp32x3"
    mk_opt = lambda m: FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)
    o1, o2 = mk_opt(m1), mk_opt(m2)
    crit = torch.nn.CrossEntropyLoss()
    proto = torch.tensor(recipe.make_prototypes(cfg)).cuda()
    kw = dict(beta=0.15, alpha=1e-2, BND=105.0, use_structure=True, group_type="block", use_prototype=True, proto_table=proto, w_f=0.05, w_r=0.1, BND_pro=2.0)
    g = GraphedStep(m2, o2, crit)
    for s in range(4):
        xr, yr, xf, yf = batch(cfg, b, s)
        p1, p2 = gs_lora_step(m1, o1, crit, xr, yr, xf, yf, **kw), g(xr, yr, xf, yf, **kw)
        assert torch.equal(p1, p2), (s, p1.tolist(), p2.tolist())
        for (n, a), (_, c) in zip(m1.named_parameters(), m2.named_parameters()):
            assert not a.requires_grad or torch.equal(a, c), (s, n)
    assert (g.eager_steps, g.captures, g.replays) == (1, 1, 3)
    # the GEMM mode is part of what a captured launch bakes in: the plain f32 mode is another graph, not a replay of this one
    m2.set_compute_dtype("fp32")
    g(*batch(cfg, b, 4), **kw)
    assert (g.eager_steps, g.captures, g.replays) == (2, 1, 3)


# ------------------------------------------------------------------------------------------------------------ 5. model parity
@pytest.fixture
def x3_builds(monkeypatch):
    """`x3_builds(module, "build", ...)`: the module's model builders build 'fp32x3' models where the f32 tests ask for 'fp32' — those tests then run,
    fixtures and bars untouched, on this mode. Counts the GEMMs that went out as GSL_F32X3."""
    from gslora_hip import _lib as L, ops
    calls = {"x3": 0, "models": []}
    orig_code = ops.gemm_code

    def counting(dtype, f32_mode=None):
        c = orig_code(dtype, f32_mode)
        calls["x3"] += c == L.F32X3
        return c
    monkeypatch.setattr(ops, "gemm_code", counting)

    def patch(module, *names):
        for name in names:
            orig = getattr(module, name)

            def wrapped(cfg, *a, _orig=orig, **kw):
                a = tuple("fp32x3" if v == "fp32" else v for v in a)
                if not any(v == "fp32x3" for v in a) and kw.get("dtype", "fp32") == "fp32":
                    kw["dtype"] = "fp32x3"
                out = _orig(cfg, *a, **kw)
                m = out[0] if isinstance(out, tuple) else out
                assert m.compute_mode == "fp32x3" and m.compute_dtype is torch.float32
                calls["models"].append(m)
                return out
            monkeypatch.setattr(module, name, wrapped)
        return calls
    return patch


@pytest.mark.parametrize("tag", ["small_b5", "small2_b3", "full_b2"])
def test_forward_eval_and_round_trip_match_the_reference(tag, golden_dir, x3_builds):
    import test_hip_model as TM
    calls = x3_builds(TM, "build")
    TM.test_forward_f32_matches_reference(tag, golden_dir)      # logits and embeddings < 1e-4: train, eval (merged), round trip
    assert calls["x3"] > 0 and all(m.compute_mode == "fp32x3" for m in calls["models"])


@pytest.mark.parametrize("tag", ["small_b5", "small2_b3"])
def test_losses_and_lora_gradients_match_the_reference(tag, golden_dir, x3_builds):
    import test_hip_model as TM
    calls = x3_builds(TM, "build")
    TM.test_grads_f32_match_reference(tag, golden_dir)          # six losses and the 24 LoRA gradients within 1e-4 max(1, |g|), both hinge settings
    assert calls["x3"] > 0


def test_engine_three_steps_match_the_reference(golden_dir, x3_builds):
    import test_hip_model as TM
    calls = x3_builds(TM, "build")
    TM.test_full_engine_three_steps_f32_match_reference(golden_dir)
    assert calls["x3"] > 0 and calls["models"][0].compute_mode == "fp32x3"


def test_vits_face_matches_the_reference(golden_dir, x3_builds):
    import test_hip_vits as TV
    calls = x3_builds(TV, "build")
    TV.test_model_f32_matches_reference(golden_dir, "vits_small2_b3")
    assert calls["x3"] > 0


def test_modified_vit_matches_the_reference(golden_dir, tmp_path, x3_builds):
    import test_hip_vitb as TB
    calls = x3_builds(TB, "build_full", "build_sub")
    TB.test_forward_f32_and_head_surgery_match_reference("vitb_small2_b3", golden_dir, tmp_path)
    assert calls["x3"] > 0


def test_attention_lora_matches_the_reference(golden_dir, x3_builds):
    import test_hip_attn_lora as TA
    calls = x3_builds(TA, "build")
    TA.test_forward_merge_and_norms_match_reference(golden_dir)
    TA.test_grads_match_reference("fp32", 1e-4, golden_dir)
    assert calls["x3"] > 0


# ------------------------------------------------------------------------------------------------------------ 6. evaluation
def eval_model(dtype):
    from test_hip_model import build
    cfg = recipe.cfg_small2()
    m = build(cfg, dtype).train()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():      # adapters that do something, and a head whose predictions are not all one class
        for n, p in m.named_parameters():
            if "lora_B" in n:
                p.copy_(torch.randn(p.shape, generator=g).cuda() * 0.05)
    x = torch.tensor(recipe.make_images(cfg, 48, seed=31, tag="xe")).cuda()
    y = torch.tensor(recipe.make_labels(cfg, 48, seed=31, tag="ye", lo=0, hi=cfg["num_class"])).cuda()
    return m, cfg, [(x[:20], y[:20]), (x[20:], y[20:])]


def logits_in(m, mode, loader):
    own = m.compute_mode
    m.set_compute_dtype(mode).eval()
    try:
        with torch.no_grad():
            return torch.cat([m(x, y)[0].float() for x, y in loader])
    finally:
        m.set_compute_dtype(own).train()


def test_eval_data_in_fp32x3_on_an_fp16_trained_model(monkeypatch):
    import engine_cl
    m, cfg, loader = eval_model("fp16")
    l32, l3 = logits_in(m, "fp32", loader), logits_in(m, "fp32x3", loader)
    assert (l32 - l3).abs().max().item() < 1e-4 and not torch.equal(l32, l3)
    acc = {}
    for ev in ("fp32", "fp32x3"):
        monkeypatch.setattr(engine_cl, "EVAL_DTYPE", ev)
        acc[ev] = engine_cl.eval_data(m, loader, "cuda", "test", 0)
        assert m.compute_mode == "fp16" and m.compute_dtype is torch.float16 and m.gemm_mode is None      # back in fp16
    labels = torch.cat([y for _, y in loader])
    top2 = l32.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) >= 2e-4      # rows whose f32 prediction a 1e-4 logit error cannot move
    if clear.all():
        assert acc["fp32x3"] == acc["fp32"]
    assert torch.equal(l3.argmax(1)[clear], l32.argmax(1)[clear])
    assert abs(acc["fp32"] - 100.0 * (l32.argmax(1) == labels).float().mean().item()) < 1e-4


def test_evaluations_restore_the_fp32x3_mode(monkeypatch):
    """The restore trap: a model in fp32x3 evaluated in another dtype comes back in fp32x3 (its torch dtype alone says float32 = 'fp32')."""
    import engine_cl
    from test_hip_verification import verif_pairs
    from util.utils import perform_val
    m, cfg, loader = eval_model("fp32x3")
    u8, issame = verif_pairs(cfg, 20, 1)
    x = torch.tensor(u8.astype(np.float32))
    for ev in ("fp32", "fp16", "fp32x3", "model"):
        monkeypatch.setattr(engine_cl, "EVAL_DTYPE", ev)
        engine_cl.eval_data(m, loader, "cuda", "test", 0)
        assert m.compute_mode == "fp32x3", ev
        engine_cl.eval_data_per_class(m, loader, "cuda", "test", 0)
        assert m.compute_mode == "fp32x3", ev
        perform_val(False, "cuda", cfg["dim"], 16, m, [x, x.flip(3)], list(issame), 5)
        assert m.compute_mode == "fp32x3" and m.gemm_mode == "x3" and m.compute_dtype is torch.float32, ev


# ------------------------------------------------------------------------------------------------------------ 7. boundary
def test_the_mode_is_for_f32_tensors_and_for_gemm_nt_only(ops):
    from gslora_hip import _lib as L
    for dt in (torch.bfloat16, torch.float16):
        A, W, out = torch.zeros(64, 64, device="cuda", dtype=dt), torch.zeros(128, 64, device="cuda", dtype=dt), torch.empty(64, 128, device="cuda", dtype=dt)
        with pytest.raises(RuntimeError, match="float32"):
            ops.gemm_nt(A, W, out, f32_mode="x3")
    lib = L.load()
    x, g, b = torch.randn(8, 64, device="cuda"), torch.ones(64, device="cuda"), torch.zeros(64, device="cuda")
    y, mean, rstd = torch.empty(8, 64, device="cuda"), torch.empty(8, device="cuda"), torch.empty(8, device="cuda")
    y.fill_(7.0)
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()
    rc = lib.gsl_layernorm_fwd(p(x), 64, p(g), p(b), 1e-5, p(y), p(mean), p(rstd), 8, 64, L.F32X3, L.F32, None)
    assert rc == -1 and b"dtype" in lib.gsl_last_error()      # GSL_ERR_ARG
    torch.cuda.synchronize()
    assert (y == 7.0).all()                                  # nothing ran
    A, W, out = torch.zeros(64, 64, device="cuda"), torch.zeros(128, 64, device="cuda"), torch.empty(64, 128, device="cuda")
    with pytest.raises(RuntimeError):      # the 16-bit-only epilogues stay 16-bit only
        ops.gemm_nt(A, W, out, epilogue=L.EPI_BIAS_RES_BF16, bias=torch.zeros(128, device="cuda"), res=out, f32_mode="x3")
