"""GPU tests of gslora_hip.step.distill_step and the three loops over it on cfg_small (lora_rank = 0, CosFace, the --only_ffn rule, dropout 0):
one step per method against a step assembled from pieces that existed before (separate student forwards, losses.ce_sum_top1, torch for the
distance, torch.autograd, the same optimizer); the driver's real case of a deep-copied teacher; the real reference's loops
(tests/golden/distill_small*.npz); one 16-bit step per method against the f32 step; LwF without a teacher; an exotic criterion; the loops and
the driver; fresh processes in which the steps that existed before leave libgslora_fd.so closed.

Bars: values within the project's parity bar 1e-4 * max(1, |want|); the gradients of two routes within 1e-4 of the tensor's largest element;
weights within the parity bar (test_hip_ffn_train.bar_ok); against the fixture, the widening rule of tests/test_hip_scrub.py (allowance);
16-bit gradients of one step within the 6 % relative Frobenius error and cosine > 0.995 that tests/test_hip_ffn_train.py declares."""
import copy
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import recipe

import test_hip_ffn_train as T

pytestmark = pytest.mark.gpu

ARGS = dict(opt="adamw", weight_decay=0.05, opt_eps=1e-8, opt_betas=None, lr=1e-4)
METHODS = ("lwf", "der", "derpp", "fdr")
# (method of distill_step, lam, lam_aux): the reference's default lambdas (util/args.py:273-295)
HYPER = {"lwf": ("lwf", 0.5, 1.0), "der": ("der", 0.1, 0.0), "derpp": ("der", 0.1, 0.1), "fdr": ("fdr", 0.1, 0.0)}
FAR_SEED, FAR_LO, FAR_HI = 77, 0.7, 1.3      # tools/make_golden_distill.py


def make_far(teacher):
    """The fixture's `far` teacher: every FFN weight matrix multiplied element-wise by recipe.uniform("far::" + name, shape, 77, 0.7, 1.3)."""
    with torch.no_grad():
        for n, p in teacher.named_parameters():
            if "fn.fn.net" in n and n.endswith("weight"):
                p.mul_(torch.tensor(recipe.uniform("far::" + n, tuple(p.shape), FAR_SEED, FAR_LO, FAR_HI)).to(p))
    teacher.invalidate_operand_caches()
    return teacher


def setup(mode="fp32", far=True, lr=None, wd=None):
    """student, a frozen teacher (a deep copy; `far`: moved away as the fixture's), the optimizer, three forget batches of 3 and three
    remain batches of 2 (the fixture's loaders)."""
    from gslora_hip.optim import create_optimizer
    cfg = recipe.cfg_small(lora_rank=0)
    student = T.build(cfg, mode)
    teacher = copy.deepcopy(student).eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    if far:
        make_far(teacher)
    args = {**ARGS, **({} if lr is None else {"lr": lr}), **({} if wd is None else {"weight_decay": wd})}
    opt = create_optimizer(SimpleNamespace(**args), student)
    forget, remain = [], []
    for s in (40, 41, 42):
        x_r, y_r, x_f, y_f = T.batches(cfg, 3, s)
        forget.append((x_f, y_f))
        remain.append((x_r[:2], y_r[:2]))
    return student, teacher, opt, forget, remain


def step_of(method, student, teacher, opt, crit, forget, remain):
    from gslora_hip import step
    m, lam, lam_aux = HYPER[method]
    extra = dict(x_n=remain[1][0], y_n=remain[1][1]) if method == "derpp" else {}
    return step.distill_step(student, teacher, opt, crit, *forget[0], *remain[0], method=m, lam=lam, lam_aux=lam_aux, **extra)


def assembled_step(method, student, teacher, opt, forget, remain):
    """The route without libgslora_fd.so and without the fused forward. -> [ce_f, reg, ce_aux, total] as floats"""
    from gslora_hip import losses
    from gslora_hip.step import _arm_overflow_guard
    _, lam, lam_aux = HYPER[method]
    (x_f, y_f), (x_r, y_r), (x_n, y_n) = forget[0], remain[0], remain[1]
    ce = lambda logits, y: losses.ce_sum_top1(logits, y)[0] / float(y.shape[0])
    ce_f = ce(student(x_f.float(), y_f)[0], y_f)
    out_r, emb_r = student(x_r.float(), y_r)
    zero = torch.zeros((), device=x_f.device)
    reg, ce_aux = zero, zero
    if method == "lwf":
        ce_aux = ce(out_r, y_r)
        total = ce_f + lam * 0.0 + lam_aux * ce_aux
    else:
        with torch.no_grad():
            t_out, t_emb = teacher(x_r.float(), y_r)
        if method == "fdr":
            reg = torch.norm(out_r - t_out, 2, 1).mean()
        else:
            n = torch.norm(emb_r - t_emb, p=2)
            reg = n * n
        total = ce_f + lam * reg
        if method == "derpp":
            ce_aux = ce(student(x_n.float(), y_n)[0], y_n)
            total = total + lam_aux * ce_aux
    opt.zero_grad()
    total.backward()
    _arm_overflow_guard(student, opt)
    opt.step()
    return [v.item() for v in (ce_f, reg, ce_aux, total)]


def value_ok(got, want):
    return abs(got - want) <= 1e-4 * max(1.0, abs(want))


def compare_models(a_model, b_model, what):
    """Gradients the two routes handed the optimizer within 1e-4 of the tensor's largest element, weights within the parity bar."""
    for (n, a), b in zip(a_model.named_parameters(), b_model.parameters()):
        if a.requires_grad:
            want = b.grad.detach().double().cpu().numpy()
            err = np.abs(a.grad.detach().double().cpu().numpy() - want).max()
            print(f"{what} grad {n}: |want|_max {np.abs(want).max():.3e}, max err / (1e-4 |want|_max) = {err / max(1e-4 * np.abs(want).max(), 1e-300):.4f}")
            assert np.abs(want).max() > 0, n
            assert err <= 1e-4 * np.abs(want).max(), n
            assert T.bar_ok(a.detach().cpu(), b.detach().cpu(), f"{what} {n}"), n


@pytest.mark.parametrize("method", METHODS)
def test_distill_step_against_a_step_assembled_from_existing_pieces(method):
    from gslora_hip import _lib_fd
    crit = torch.nn.CrossEntropyLoss()
    s1, t1, o1, forget, remain = setup()
    s2, t2, o2, _, _ = setup()
    got = step_of(method, s1, t1, o1, crit, forget, remain)
    assert got.is_cuda and got.shape == (4,) and got.dtype == torch.float32
    got = got.cpu().numpy().astype(np.float64)
    want = assembled_step(method, s2, t2, o2, forget, remain)
    print(method, "got", got, "want", want)
    for k, name in enumerate(("ce_f", "reg", "ce_aux", "total")):
        assert value_ok(got[k], want[k]), (name, got[k], want[k])
    if method == "lwf":
        assert got[1] == 0.0 and got[2] > 0
    else:
        assert _lib_fd.loaded() and got[1] > 1e-2, "a far teacher: the distance is not a zero"
        assert (got[2] > 0) == (method == "derpp")
    compare_models(s1, s2, method)
    assert all(not p.requires_grad and p.grad is None for p in t1.parameters()), "the teacher receives nothing"


@pytest.mark.parametrize("method", ["der", "fdr"])
def test_the_first_step_against_a_copied_teacher(method):
    """The driver's real case: the teacher is a deep copy, dropout is 0, fp32 — the student's rows of the fused train-mode forward and the
    teacher's no-grad forward of the same images are the same bits, so the distance is an exact 0, its gradient an exact zero (FDR: the
    subgradient of the norm at 0) and the step is a cross-entropy-only step on the forget batch."""
    from gslora_hip import step
    crit = torch.nn.CrossEntropyLoss()
    s1, t1, o1, forget, remain = setup(far=False)
    s2, _, o2, _, _ = setup(far=False)
    got = step_of(method, s1, t1, o1, crit, forget, remain).cpu().numpy().astype(np.float64)
    print(method, "copy: reg =", repr(got[1]))
    assert got[1] == 0.0, "student rows and teacher rows of the same images are the same bits"
    assert got[3] == got[0] and got[2] == 0.0
    want = step.ffn_reg_step(s2, o2, crit, *forget[0]).cpu().numpy().astype(np.float64)
    assert value_ok(got[0], want[0])
    compare_models(s1, s2, f"{method} copy")


# ---------------------------------------------------------------------------------------------------------------- the reference's loops
def allowance(want32, want64):
    """tests/test_hip_scrub.py: the parity bar 1e-4 * max(1, |want|); where the reference's own f32 run leaves its f64 run by more than a
    quarter of that bar, four times that recorded deviation."""
    bar = 1e-4 * np.maximum(1.0, np.abs(want32))
    dev = np.abs(want32 - want64)
    return np.where(dev > bar / 4, 4 * dev, bar)


def recording():
    """An AverageMeter that keeps every value it was fed (the loops reset their meters in place)."""
    from util.utils import AverageMeter

    class Recording(AverageMeter):
        def __init__(self):
            super().__init__()
            self.seen = []

        def update(self, val, n=1):
            self.seen.append(float(val))
            super().update(val, n)
    return Recording()


METERS = {"lwf": ("losses_CE", "losses_KD", "losses_remain", "losses_total"), "der": ("losses_CE", "losses_DER", "losses_total"),
          "derpp": ("losses_CE", "losses_DER", "losses_total"), "fdr": ("losses_CE", "losses_FDR", "losses_total")}


def run_loop(method, student, teacher, opt, forget, remain, hyper, meters):
    from baselines.DERtrain import train_one_epoch_DER
    from baselines.FDRtrain import train_one_epoch_FDR
    from baselines.Lwftrain import train_one_epoch_Lwf
    lr, wd, lwf_kd, lwf_remain, lwf_T, der_lambda, der_plus_lambda, fdr_lambda = hyper
    common = dict(student_model=student, teacher_model=teacher, data_loader_cl_forget=forget, remain_loader=remain, criterion=torch.nn.CrossEntropyLoss(),
                  optimizer=opt, device=torch.device("cuda"), epoch=0, batch=0, task_i=0, testloader_forget=None, testloader_remain=None,
                  forget_acc_before=0.0, highest_H_mean=0.0, cfg={}, **meters)
    if method == "lwf":
        return train_one_epoch_Lwf(lambda_kd=lwf_kd, lambda_remain=lwf_remain, temperature=lwf_T, **common)
    if method in ("der", "derpp"):
        return train_one_epoch_DER(lambda_der=der_lambda, plus=method == "derpp", lambda_der_plus=der_plus_lambda, **common)
    return train_one_epoch_FDR(reg_lambda=fdr_lambda, **common)


@pytest.mark.parametrize("teacher_kind", ["copy", "far"])
@pytest.mark.parametrize("method", METHODS)
def test_the_loops_against_the_reference_fixture(golden_dir, method, teacher_kind):
    """tests/golden/distill_small*.npz (tools/make_golden_distill.py): the REAL loops, 3 steps per tag. Meters, the gradients the last step
    left and (far teacher) the final weights, against the reference's f32 run under the allowance and against its f64 run: per element the
    plain bar where the reference's f32 run stays within a quarter of it, else four times the recorded deviation."""
    g = np.load(os.path.join(golden_dir, "distill_small.npz"))
    t = np.load(os.path.join(golden_dir, f"distill_small_{method}.npz"))
    tag = f"{method}_{teacher_kind}"
    hyper = g["hyper"].tolist()
    student, teacher, opt, forget, remain = setup("fp32", far=teacher_kind == "far", lr=hyper[0], wd=hyper[1])
    names = [n for n, p in student.named_parameters() if p.requires_grad]
    assert names == g["trainable"].tolist()
    meters = {k: recording() for k in METERS[method]}
    out = run_loop(method, student, teacher, opt, forget, remain, hyper, meters)
    assert out[0] == 3 and len(out) == (6 if method == "lwf" else 5)
    got = np.array([meters[k].seen for k in METERS[method]]).T
    want, want64 = g[f"meters::{tag}"], g[f"meters64::{tag}"]
    assert got.shape == want.shape
    ratio = np.abs(got - want) / allowance(want, want64)
    ratio64 = np.abs(got - want64) / allowance(want64, want)
    print(f"{tag} meters: max |err| / allowance per column {ratio.max(0)}; vs the f64 run {ratio64.max(0)}")
    print(f"{tag} got\n{got}\nwant\n{want}")
    assert (ratio <= 1.0).all() and (ratio64 <= 1.0).all(), (ratio, ratio64)
    if method == "lwf":
        assert not got[:, 1].any(), "the KD meter reads an exact 0"
    elif teacher_kind == "copy":
        assert got[0, 1] == 0.0
    params = dict(student.named_parameters())
    kinds = [("grad", lambda p: p.grad)] + ([("final", lambda p: p)] if teacher_kind == "far" else [])
    for kind, pick in kinds:
        for n in names:
            w32 = t[f"{kind}::{tag}::{n}"].astype(np.float64)
            diff = t[f"{kind}_diff::{tag}::{n}"].astype(np.float64)
            scale = np.abs(w32).max() if kind == "grad" else max(1.0, np.abs(w32).max())      # gradients: per tensor, against |want|_max
            bar = 1e-4 * scale
            allow = np.where(np.abs(diff) > bar / 4, 4 * np.abs(diff), bar)      # per element
            v = pick(params[n]).detach().cpu().numpy().astype(np.float64)
            err, err64 = np.abs(v - w32), np.abs(v - (w32 + diff))
            print(f"{tag} {kind} {n}: |want|_max {np.abs(w32).max():.3e}, max err / allowance = {(err / allow).max():.3f}, "
                  f"vs the f64 run {(err64 / allow).max():.3f}; widened elements {(allow > bar).mean():.4f}")
            assert (err <= allow).all(), (kind, n)
            assert (err64 <= allow).all(), (kind, n, "the f64 run")


# ---------------------------------------------------------------------------------------------------------------- 16-bit modes
def one_step_grads(mode, method):
    student, teacher, opt, forget, remain = setup(mode)
    step_of(method, student, teacher, opt, torch.nn.CrossEntropyLoss(), forget, remain)
    return {n: p.grad.detach().double().cpu().numpy().copy() for n, p in student.named_parameters() if p.requires_grad}


@pytest.fixture(scope="module")
def f32_step_grads():
    return {method: one_step_grads("fp32", method) for method in METHODS}


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("mode", ["fp16", "bf16"])
def test_16bit_gradients_of_one_step(mode, method, f32_step_grads):
    """The tolerance tests/test_hip_ffn_train.py declares for the 16-bit FFN gradients against f32 — relative Frobenius error <= 6 %, cosine
    > 0.995 — per tensor, with a far teacher (the difference of the two networks' outputs stands well above the 16-bit forward error)."""
    got = one_step_grads(mode, method)
    for n, want in f32_step_grads[method].items():
        rel = np.linalg.norm(got[n] - want) / np.linalg.norm(want)
        cos = float((got[n] * want).sum() / (np.linalg.norm(got[n]) * np.linalg.norm(want)))
        print(f"{mode} {method} {n}: rel Frobenius {rel:.4f}, cosine {cos:.5f}")
        assert rel <= 0.06 and cos > 0.995, n


@pytest.mark.parametrize("mode", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("method", METHODS)
def test_a_four_step_loop_runs_in_every_mode(mode, method):
    """Four steps: finite meters, and no step was skipped by the overflow guard — every step moved the weights (a skipped step leaves them
    untouched) and the guard the optimizer read stayed below the fp16 limit."""
    student, teacher, opt, forget, remain = setup(mode)
    crit = torch.nn.CrossEntropyLoss()
    probe = next(p for n, p in student.named_parameters() if p.requires_grad and p.dim() == 2)
    rows, guards = [], []
    for k in range(4):
        before = probe.detach().clone()
        rows.append(step_of(method, student, teacher, opt, crit, forget[k % 3:] + forget[:k % 3], remain[k % 3:] + remain[:k % 3]))
        assert not torch.equal(before, probe.detach()), f"step {k} moved the weights"
        if opt.overflow_guard is not None:
            guards.append(opt.overflow_guard.detach().clone())
    rows = torch.stack(rows).cpu().numpy()
    assert np.isfinite(rows).all()
    if mode == "fp16":
        assert len(guards) == 4 and all(torch.isfinite(v).all() and float(v.max()) < 65504.0 for v in guards)
    else:
        assert not guards


# ---------------------------------------------------------------------------------------------------------------- LwF, exotic criterion
class _Raises(torch.nn.Module):
    def forward(self, *a, **k):
        raise AssertionError("LwF must not run its teacher")


def test_lwf_never_runs_its_teacher_and_reports_an_exact_zero():
    from gslora_hip import step
    student, _, opt, forget, remain = setup()
    got = step.distill_step(student, _Raises(), opt, torch.nn.CrossEntropyLoss(), *forget[0], *remain[0], method="lwf", lam=0.5, lam_aux=1.0)
    got = got.cpu().numpy()
    assert got[1] == 0.0 and np.signbit(got[1]) == False and got[3] == np.float32(got[0] + got[2])      # noqa: E712
    with pytest.raises(AssertionError, match="must not run its teacher"):
        step.distill_step(student, _Raises(), opt, torch.nn.CrossEntropyLoss(), *forget[0], *remain[0], method="fdr", lam=0.1)


@pytest.mark.parametrize("method", METHODS)
def test_an_exotic_criterion_keeps_its_semantics(method):
    """A weighted criterion (all ones: the same value) takes the criterion's own route through torch on the row segments."""
    s1, t1, o1, forget, remain = setup()
    s2, t2, o2, _, _ = setup()
    a = step_of(method, s1, t1, o1, torch.nn.CrossEntropyLoss(), forget, remain).cpu().numpy()
    b = step_of(method, s2, t2, o2, torch.nn.CrossEntropyLoss(weight=torch.ones(10).cuda()), forget, remain).cpu().numpy()
    assert a[1] == b[1], "the distance does not pass through the criterion"
    assert all(value_ok(float(b[i]), float(a[i])) for i in range(4))
    compare_models(s2, s1, f"{method} exotic")


# ---------------------------------------------------------------------------------------------------------------- the driver, laziness
@pytest.mark.parametrize("method", METHODS)
def test_the_driver_runs_two_tasks(method, tmp_path):
    import driver_distill
    from gslora_hip import _lib_fd
    common = ["--method", method, "--small", "--num_class", "20", "--per_forget_cls", "4", "--num_tasks", "2", "--epochs", "1", "--batch_size", "16",
              "--samples_per_class", "4", "--dropout", "0.0", "--dtype", "fp32", "--ffn_open"]
    rep, outdir, model = driver_distill.main(common + ["--outdir", str(tmp_path / "a")])
    lines = [json.loads(ln) for ln in open(os.path.join(outdir, "distill_report.jsonl"))]
    assert len(rep) == len(lines) == 2 and [r["task"] for r in lines] == [0, 1] and all(r["method"] == method and r["steps"] >= 1 for r in rep)
    assert all(np.isfinite(r[k]) for r in rep for k in ("forget_before", "forget_after", "remain_before", "remain_after"))
    assert all(np.isfinite(v) for r in rep for e in r["epochs"] for v in e.values() if v is not None)
    assert not any(p.requires_grad for n, p in model.named_parameters() if "fn.fn.net" not in n and "loss" not in n)
    assert _lib_fd.loaded() or method == "lwf"
    rep2, _, _ = driver_distill.main(common + ["--outdir", str(tmp_path / "b")])
    assert rep2 == rep, "the same report twice under the same seed"


CHILD = """
import sys
sys.path[:0] = [%r, %r, %r]
from types import SimpleNamespace
import torch
import loralib as lora
from oracle import recipe
from vit_pytorch_face import ViT_face
import test_hip_ffn_train as T
import test_hip_distill as D
from gslora_hip import _lib_fd, _lib_kd, step
from gslora_hip.optim import create_optimizer
args = SimpleNamespace(opt="adamw", weight_decay=0.05, opt_eps=1e-8, opt_betas=None, lr=1e-4)
crit = torch.nn.CrossEntropyLoss()
"""

EXISTING = CHILD + """
cfg = recipe.cfg_small(lora_rank=0)
m = T.build(cfg, "fp32")
x_r, y_r, x_f, y_f = T.batches(cfg, 3)
assert torch.isfinite(step.ffn_reg_step(m, create_optimizer(args, m), crit, x_r, y_r)).all()
import copy
t = copy.deepcopy(m).eval()
assert torch.isfinite(step.scrub_step(m, t, create_optimizer(args, m), crit, x_r, y_r, maximize=False, kd_T=2.0, sgda_gamma=0.99, sgda_alpha=0.001)).all()
h = T.build(cfg, "fp32")
for n, p in h.named_parameters():
    p.requires_grad = "loss" in n
assert torch.isfinite(step.head_probe_step(h, create_optimizer(args, h), crit, x_r, y_r)).all()
cfg = recipe.cfg_small()
m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
             dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], lora_rank=cfg["lora_rank"])
lora.mark_only_lora_as_trainable(m)
m = m.to("cuda").set_compute_dtype("fp32").train()
step.gs_lora_step(m, create_optimizer(args, m), crit, x_r, y_r, x_f, y_f, beta=0.15, alpha=0.01, BND=105.0)
torch.cuda.synchronize()
assert not _lib_fd.loaded() and "libgslora_fd" not in open("/proc/self/maps").read()
assert _lib_kd.loaded() and "libgslora_hip" in open("/proc/self/maps").read()
print("ok")
"""

LWF = CHILD + """
student, teacher, opt, forget, remain = D.setup()
out = D.step_of("lwf", student, teacher, opt, crit, forget, remain)
torch.cuda.synchronize()
assert torch.isfinite(out).all()
maps = open("/proc/self/maps").read()
assert not _lib_fd.loaded() and not _lib_kd.loaded() and "libgslora_fd" not in maps and "libgslora_kd" not in maps
assert "libgslora_hip" in maps and "libgslora_train" in maps
print("ok")
"""


@pytest.mark.parametrize("code", [EXISTING, LWF], ids=["existing-steps", "lwf"])
def test_fresh_processes_leave_the_fifth_library_closed(code):
    """A fresh process runs ffn_reg_step, scrub_step, head_probe_step and gs_lora_step: libgslora_fd.so is not loaded, not mapped. Another runs
    an LwF step: neither the fourth nor the fifth library is opened."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", code % (os.path.dirname(here), os.path.join(os.path.dirname(here), "gs-lora_amd"), here)],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
