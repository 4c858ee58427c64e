"""GPU tests of gslora_hip.step.scrub_step on cfg_small (lora_rank = 0, CosFace, the --only_ffn rule, dropout 0): one max step and one min
step against a step assembled from pieces that existed before (losses.ce_sum_top1, the torch formula for the KL, a per-tensor torch
param_dist, the same optimizer); the alternation of the reference's superepoch (five max + min passes, five min passes over one-batch
loaders: 15 steps) in every compute mode; what the loop must leave alone (the teacher, the student's logits under update_parameters); the
real reference's superepoch (tests/golden/scrub_small.npz); a fresh process in which the steps that existed before leave libgslora_kd.so closed.

Bounds: losses within the kernels' bound of tests/test_hip_kd_kernels.py plus the measured distance of the torch expression from float64;
the gradients of the two routes within 1e-4 of the tensor's largest element, weights within the project's parity bar 1e-4 * max(1, |want|)
(test_hip_ffn_train.bar_ok); 16-bit gradients of one step within the 6 % relative Frobenius error and cosine > 0.995 that
tests/test_hip_ffn_train.py declares, 16-bit final weights within that 6 % with the direction of the update held besides."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.optim.swa_utils import AveragedModel

from oracle import recipe

import test_hip_ffn_train as T
import test_hip_kd_kernels as K

pytestmark = pytest.mark.gpu

ARGS = dict(opt="adamw", weight_decay=0.05, opt_eps=1e-8, opt_betas=None, lr=1e-4)
HYPER = dict(kd_T=2.0, sgda_gamma=0.99, sgda_alpha=0.001)
SMOOTHING = 0.1


def setup(mode="fp32"):
    """student, teacher (a frozen copy with shifted FFN biases, so that the KL and its gradient are not zero), the averaged copy (shifted
    too: a non-zero distance), the optimizer, a forget batch of 3 and a remain batch of 2."""
    from gslora_hip.optim import create_optimizer
    cfg = recipe.cfg_small(lora_rank=0)
    student = T.build(cfg, mode)
    teacher = copy.deepcopy(student).eval()
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in teacher.named_parameters():
            p.requires_grad_(False)
            if "fn.fn.net" in n and n.endswith("bias"):
                p.add_(0.05 * torch.randn(p.shape, generator=gen).cuda())
    teacher.invalidate_operand_caches()
    swa = AveragedModel(student, avg_fn=lambda avg, new, n: 0.9 * avg + 0.1 * new)
    with torch.no_grad():
        for n, p in swa.named_parameters():
            if "fn.fn.net" in n:
                p.add_(0.01 * torch.randn(p.shape, generator=gen).cuda())
    opt = create_optimizer(SimpleNamespace(**ARGS), student)
    x_r, y_r, x_f, y_f = T.batches(cfg, 3, 40)
    return student, teacher, swa, opt, (x_f, y_f), (x_r[:2], y_r[:2])


def torch_kd(ys, yt, T_):
    return F.kl_div(F.log_softmax(ys / T_, dim=1), F.softmax(yt / T_, dim=1), reduction="sum") * T_ ** 2 / ys.shape[0]


def assembled_step(student, teacher, swa, opt, x, y, maximize):
    """The route without libgslora_kd.so; dist64: the distance term in float64, before the update."""
    from gslora_hip import losses
    from gslora_hip.step import _arm_overflow_guard
    logits, _ = student(x.float(), y)
    with torch.no_grad():
        t_logits, _ = teacher(x.float(), y)
    kd = torch_kd(logits, t_logits, HYPER["kd_T"])
    dist = SMOOTHING * sum(torch.norm(a - b) for a, b in zip(student.parameters(), swa.parameters()))
    if maximize:
        ce = torch.zeros((), device=kd.device)
        total = -kd + dist
    else:
        ce = losses.ce_sum_top1(logits, y)[0] / float(x.shape[0])
        total = HYPER["sgda_gamma"] * ce + HYPER["sgda_alpha"] * kd + dist
    dist64 = SMOOTHING * sum(torch.norm(a.detach().double() - b.detach().double()) for a, b in zip(student.parameters(), swa.parameters())).item()
    opt.zero_grad()
    total.backward()
    _arm_overflow_guard(student, opt)
    opt.step()
    return dict(kd=kd.item(), ce=ce.item(), total=total.item(), dist=dist.item(), dist64=dist64, ys=logits.detach().cpu().numpy(),
                yt=t_logits.cpu().numpy())


@pytest.mark.parametrize("maximize", [True, False])
def test_scrub_step_against_a_step_assembled_from_existing_pieces(maximize):
    from gslora_hip import _lib_kd, kd, step
    crit = torch.nn.CrossEntropyLoss()
    s1, t1, w1, o1, forget, remain = setup()
    s2, t2, w2, o2, _, _ = setup()
    x, y = forget if maximize else remain
    got = step.scrub_step(s1, t1, o1, crit, x, y, maximize=maximize, dist=kd.ParamDist(s1, w1, SMOOTHING), **HYPER)
    assert got.is_cuda and got.shape == (3,) and _lib_kd.loaded()
    got = got.cpu().numpy().astype(np.float64)
    a = assembled_step(s2, t2, w2, o2, x, y, maximize)
    kd_t, ce_t, total_t, ys, yt = a["kd"], a["ce"], a["total"], a["ys"], a["yt"]
    c_kd, c_ce = (-1.0, 0.0) if maximize else (HYPER["sgda_alpha"], HYPER["sgda_gamma"])
    r = K.reference(ys, yt, y.cpu().numpy(), HYPER["kd_T"], c_kd, c_ce)
    assert r["out"][0] > 1e-4, "the teacher differs from the student: the KL is not a zero"
    slack = [abs(kd_t - r["out"][0]), abs(ce_t - r["out"][1])]      # the torch expressions' own distance from float64
    print("kd", got[0], kd_t, r["out"][0], "ce", got[1], ce_t, r["out"][1], "total", got[2], total_t)
    assert abs(got[0] - kd_t) <= r["bound"][0] + slack[0]
    assert abs(got[1] - ce_t) <= r["bound"][1] + slack[1]
    # the total: the part's bound, the distance under the bound of tests/test_hip_kd_kernels.py ((ceil(nblk / 256) + 20) / 2 + 1 <= 12 per
    # norm, one add per entry, the product), the torch expressions' own distances from float64, and the last add on either side
    n_entries = len(list(s2.parameters()))
    b_dist = (12 + n_entries + 1) * K.E * a["dist64"]
    assert abs(got[2] - total_t) <= (r["bound"][2] + abs(c_kd) * slack[0] + abs(c_ce) * slack[1] + b_dist + abs(a["dist"] - a["dist64"])
                                     + 4 * K.E * (abs(total_t) + a["dist64"]))
    # the gradients the two routes handed the optimizer (p.grad survives the update): what scrub_step's coefficients and the distance's
    # gradient are checked by. The bar is the parity bar scaled to the tensor, 1e-4 * |want|_max without the floor of 1: one AdamW step at
    # lr = 1e-4 moves no weight by more than 1e-4, so the weights below could not tell a wrong magnitude
    side = "max" if maximize else "min"
    for (n, a), b in zip(s1.named_parameters(), s2.parameters()):
        if a.requires_grad:
            want = b.grad.detach().double().cpu().numpy()
            err = np.abs(a.grad.detach().double().cpu().numpy() - want).max()
            print(f"{side} grad {n}: |want|_max {np.abs(want).max():.3e}, max err / (1e-4 |want|_max) = {err / max(1e-4 * np.abs(want).max(), 1e-300):.4f}")
            assert err <= 1e-4 * np.abs(want).max(), n
            assert np.abs(want).max() > 0 or "loss" in n, "every FFN tensor has a gradient (the head's distance to its copy is 0)"
            assert T.bar_ok(a.detach().cpu(), b.detach().cpu(), f"{side} {n}"), n
    assert any(not torch.equal(a, b) for a, b in zip(s1.parameters(), t1.parameters()))


def superepoch(student, teacher, swa, opt, forget, remain, dist):
    """The alternation of the reference's loop over one-batch loaders: 5 x (max, min), then 5 x min. -> [15, 3] on the host (one sync)."""
    from gslora_hip import step
    crit, rows = torch.nn.CrossEntropyLoss(), []
    for i in range(10):
        if i < 5:
            rows.append(step.scrub_step(student, teacher, opt, crit, *forget, maximize=True, dist=dist, **HYPER))
        rows.append(step.scrub_step(student, teacher, opt, crit, *remain, maximize=False, dist=dist, **HYPER))
    swa.update_parameters(student)
    return torch.stack(rows).cpu().numpy()


@pytest.fixture(scope="module")
def f32_final():
    from gslora_hip import kd
    student, teacher, swa, opt, forget, remain = setup("fp32")
    rows = superepoch(student, teacher, swa, opt, forget, remain, kd.ParamDist(student, swa, SMOOTHING))
    return rows, {n: p.detach().cpu().numpy().copy() for n, p in student.named_parameters() if p.requires_grad}


def one_step_grads(mode, maximize):
    """The gradients one scrub_step hands the optimizer, from a fresh set-up."""
    from gslora_hip import kd, step
    student, teacher, swa, opt, forget, remain = setup(mode)
    step.scrub_step(student, teacher, opt, torch.nn.CrossEntropyLoss(), *(forget if maximize else remain), maximize=maximize,
                    dist=kd.ParamDist(student, swa, SMOOTHING), **HYPER)
    return {n: p.grad.detach().double().cpu().numpy().copy() for n, p in student.named_parameters() if p.requires_grad}


@pytest.fixture(scope="module")
def f32_step_grads():
    return {maximize: one_step_grads("fp32", maximize) for maximize in (False, True)}


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("mode", ["fp16", "bf16"])
def test_16bit_gradients_of_one_step(mode, maximize, f32_step_grads):
    """The tolerance tests/test_hip_ffn_train.py declares for the 16-bit FFN gradients against f32 — relative Frobenius error <= 6 %, cosine
    > 0.995 — per tensor, on what a min step differentiates (0.99 CE + 0.001 KL + the distance) and on what a max step does (-KL + the
    distance; the teacher of setup() is shifted far enough that the difference of the two softmaxes stands well above the 16-bit forward
    error of either network)."""
    got = one_step_grads(mode, maximize)
    for n, want in f32_step_grads[maximize].items():
        if not want.any():
            assert not got[n].any(), n
            continue
        rel = np.linalg.norm(got[n] - want) / np.linalg.norm(want)
        cos = float((got[n] * want).sum() / (np.linalg.norm(got[n]) * np.linalg.norm(want)))
        print(f"{mode} {'max' if maximize else 'min'} {n}: rel Frobenius {rel:.4f}, cosine {cos:.5f}")
        assert rel <= 0.06 and cos > 0.995, n


@pytest.mark.parametrize("mode", ["fp32", "fp16", "bf16"])
def test_the_fifteen_step_loop_runs_in_every_mode(mode, f32_final):
    from gslora_hip import kd
    student, teacher, swa, opt, forget, remain = setup(mode)
    frozen = [p.detach().clone() for p in teacher.parameters()]
    start = {n: p.detach().cpu().numpy().astype(np.float64) for n, p in student.named_parameters() if p.requires_grad}
    with torch.no_grad():
        t_before = teacher(forget[0].float(), forget[1])[0].clone()
        student.eval()
        s_before = student(forget[0].float(), forget[1])[0].clone()
        student.train()
    rows = superepoch(student, teacher, swa, opt, forget, remain, kd.ParamDist(student, swa, SMOOTHING))
    assert rows.shape == (15, 3) and np.isfinite(rows).all()
    assert (rows[[0, 2, 4, 6, 8], 1] == 0).all() and (rows[[1, 3, 5, 7, 9, 10, 11, 12, 13, 14], 1] > 0).all(), "CE on the min steps only"
    guard = student.runner().overflow_guard()
    if mode == "fp16":
        assert guard is not None and opt.overflow_guard is not None and opt.overflow_guard.data_ptr() == guard.data_ptr()
    else:
        assert guard is None and opt.overflow_guard is None
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(frozen, teacher.parameters())), "the teacher's parameters are untouched"
        assert torch.equal(t_before, teacher(forget[0].float(), forget[1])[0]), "... and so are its logits"
        student.eval()
        s_after = student(forget[0].float(), forget[1])[0].clone()
        assert not torch.equal(s_before, s_after), "the student's operand copies were re-made after the updates: its logits moved"
        swa.update_parameters(student)
        assert torch.equal(s_after, student(forget[0].float(), forget[1])[0]), "update_parameters leaves the student alone"
        student.train()
    want_rows, want = f32_final
    for n, p in student.named_parameters():
        if p.requires_grad:
            v = p.detach().cpu().numpy().astype(np.float64)
            rel = np.linalg.norm(v - want[n]) / np.linalg.norm(want[n])
            print(f"{mode} {n}: rel Frobenius to the f32 run {rel:.2e}")
            assert rel <= (0.0 if mode == "fp32" else 0.06), n
            # ... which a student that never trained would meet too (15 steps at lr 1e-4 move a weight by 1.5e-3 at most): the UPDATE
            # points where the f32 run's update points. Adam normalises every element, so the update's size says little and its
            # direction is what is held: more than half of the f32 update's length lies along it
            up, up32 = v - start[n], want[n] - start[n]
            cos = float((up * up32).sum() / max(np.linalg.norm(up) * np.linalg.norm(up32), 1e-300))
            print(f"{mode} {n}: |update| {np.linalg.norm(up):.3e} (f32 {np.linalg.norm(up32):.3e}), cosine {cos:.4f}")
            assert np.linalg.norm(up) > 0 and cos > 0.5, n
    if mode == "fp32":
        assert np.array_equal(rows, want_rows), "the same inputs give the same trajectory, bit for bit"


def test_smoothing_zero_and_the_exotic_criterion():
    from gslora_hip import kd, step
    student, teacher, swa, opt, forget, remain = setup()
    d0 = kd.ParamDist(student, swa, 0.0)
    a = step.scrub_step(student, teacher, opt, torch.nn.CrossEntropyLoss(), *remain, maximize=False, dist=d0, **HYPER).cpu().numpy()
    assert d0.table_dev is None, "smoothing 0 lays nothing out"
    s2, t2, w2, o2, _, _ = setup()
    b = step.scrub_step(s2, t2, o2, torch.nn.CrossEntropyLoss(label_smoothing=0.0, reduction="mean", weight=torch.ones(10).cuda()), *remain,
                        maximize=False, dist=None, **HYPER).cpu().numpy()
    # a weighted criterion (all ones: the same value) takes the criterion's own route: CE from torch, the KL part from the kernels
    assert a[0] == b[0] and all(abs(a[i] - b[i]) <= 1e-4 * max(1.0, abs(a[i])) for i in (1, 2)), "the parity bar"
    for (n, p), q in zip(student.named_parameters(), s2.parameters()):
        if p.requires_grad:
            assert T.bar_ok(p.detach().cpu(), q.detach().cpu(), n), n


def test_the_superepoch_loop_and_the_driver(tmp_path):
    """baselines.SCRUBtrain over one-batch loaders gives scrub_step's trajectory (the meters replay the packs); driver_scrub runs two tasks,
    writes two records, does not raise the forget accuracy of the first task, and repeats itself under the same seed."""
    import json
    import os
    import driver_scrub
    from baselines.SCRUBtrain import train_one_superepoch_SCRUB
    from gslora_hip import kd
    from util.utils import AverageMeter
    student, teacher, swa, opt, forget, remain = setup()
    rows = superepoch(student, teacher, swa, opt, forget, remain, kd.ParamDist(student, swa, SMOOTHING))
    s2, t2, w2, o2, _, _ = setup()
    names = ("losses_CE", "losses_total_forget", "losses_total_remain", "losses_kd_remain", "losses_kd_forget")
    cfg = dict(lr_decay_rate=0.1, lr_decay_epochs=100, sgda_learning_rate=ARGS["lr"])
    out = train_one_superepoch_SCRUB(s2, t2, w2, [forget], [remain], torch.nn.CrossEntropyLoss(), o2, torch.device("cuda"), 0, 0,
                                     task_i="0", testloader_forget=None, testloader_remain=None, forget_acc_before=0.0, highest_H_mean=0.0,
                                     cfg=cfg, sgda_smoothing=SMOOTHING, **{n: AverageMeter() for n in names}, **HYPER)
    assert len(out) == 8 and out[0] == 15 and out[7] is w2 and int(w2.n_averaged) == 1
    assert all(torch.equal(a, b) for a, b in zip(student.parameters(), s2.parameters())), "the loop is scrub_step in the reference's order"
    assert rows.shape == (15, 3) and all(out[k].count == 0 for k in (2, 4, 6)), "step 15 is a display step: the remain meters were reset"
    common = ["--small", "--num_class", "20", "--per_forget_cls", "4", "--num_tasks", "2", "--SCRUB_superepoch", "1", "--batch_size", "16",
              "--samples_per_class", "4", "--dropout", "0.0", "--dtype", "fp32", "--ffn_open"]
    rep, outdir, model = driver_scrub.main(common + ["--outdir", str(tmp_path / "a")])
    lines = [json.loads(ln) for ln in open(os.path.join(outdir, "scrub_report.jsonl"))]
    assert len(rep) == len(lines) == 2 and [r["task"] for r in lines] == [0, 1] and all(r["n_averaged"] == 1 for r in rep)
    assert np.isfinite(rep[0]["forget_after"]) and rep[0]["forget_after"] <= rep[0]["forget_before"]
    assert all(np.isfinite(v) for r in rep for e in r["superepochs"] for v in e.values() if v is not None)
    assert not any(p.requires_grad for n, p in model.named_parameters() if "fn.fn.net" not in n and "loss" not in n)
    rep2, _, _ = driver_scrub.main(common + ["--outdir", str(tmp_path / "b")])
    assert rep2 == rep, "the same report twice under the same seed"


# ---------------------------------------------------------------------------------------------------------------- the reference's superepoch
def allowance(want32, want64):
    """The project's parity bar 1e-4 * max(1, |want|); where the reference's own f32 run leaves its f64 run by more than a quarter of that
    bar, four times that recorded deviation (our GEMMs round in another order than torch's). From the fixture alone."""
    bar = 1e-4 * np.maximum(1.0, np.abs(want32))
    dev = np.abs(want32 - want64)
    return np.where(dev > bar / 4, 4 * dev, bar)


@pytest.mark.parametrize("tag", ["s0", "s1"])
def test_the_superepoch_against_the_reference_fixture(golden_dir, tag):
    """tests/golden/scrub_small.npz (tools/make_golden_scrub.py): the REAL train_one_superepoch_SCRUB, 15 steps, smoothing 0 (s0) and 0.1 (s1).
    The first max step starts from student == teacher: the KL and its gradient are exactly 0 here and rounding noise in the reference's f32
    run, which Adam's normalisation turns into steps of the size of lr — the recorded f32 - f64 deviations are what that costs. So two
    things are held: the reference's f32 run under the issue's allowance (per element for the weights), and the reference's f64 run —
    which, like this one, takes no noise step — under the plain bar 1e-4 * max(1, |want|)."""
    import os
    from baselines.SCRUBtrain import train_one_superepoch_SCRUB
    from gslora_hip.optim import create_optimizer
    from util.utils import AverageMeter

    class Recording(AverageMeter):
        def __init__(self):
            super().__init__()
            self.seen = []

        def update(self, val, n=1):
            self.seen.append(float(val))
            super().update(val, n)

    g = np.load(os.path.join(golden_dir, "scrub_small.npz"))
    lr, wd, kd_T, gamma, alpha, smoothing = g["hyper"].tolist()
    cfg = recipe.cfg_small(lora_rank=0)
    student = T.build(cfg, "fp32")
    assert [n for n, p in student.named_parameters() if p.requires_grad] == g["trainable"].tolist()
    teacher = copy.deepcopy(student).eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    swa = AveragedModel(student, avg_fn=lambda avg, new, n: 0.9 * avg + 0.1 * new)
    opt = create_optimizer(SimpleNamespace(**{**ARGS, "lr": lr, "weight_decay": wd}), student)
    x_r, y_r, x_f, y_f = T.batches(cfg, 3, 40)
    assert y_f.cpu().tolist() == g["y_forget"].tolist() and y_r[:2].cpu().tolist() == g["y_remain"].tolist()
    m = {k: Recording() for k in ("losses_CE", "losses_total_forget", "losses_total_remain", "losses_kd_remain", "losses_kd_forget")}
    out = train_one_superepoch_SCRUB(
        student=student, teacher=teacher, swa_model=swa, data_loader_forget=[(x_f, y_f)], remain_loader=[(x_r[:2], y_r[:2])],
        criterion=torch.nn.CrossEntropyLoss(), optimizer=opt, device=torch.device("cuda"), superepoch=0, batch=0, task_i=0, testloader_forget=None,
        testloader_remain=None, forget_acc_before=0.0, highest_H_mean=0.0, cfg=dict(lr_decay_rate=0.1, lr_decay_epochs=100, sgda_learning_rate=lr),
        kd_T=kd_T, sgda_smoothing=smoothing if tag == "s1" else 0.0, sgda_gamma=gamma, sgda_alpha=alpha, **m)
    assert out[0] == 15
    got_f = np.array([m["losses_kd_forget"].seen, m["losses_total_forget"].seen]).T
    got_r = np.array([m["losses_kd_remain"].seen, m["losses_CE"].seen, m["losses_total_remain"].seen]).T
    for what, got, want, want64 in (("forget", got_f, g[f"forget::{tag}"], g[f"forget64::{tag}"]), ("remain", got_r, g[f"remain::{tag}"], g[f"remain64::{tag}"])):
        assert got.shape == want.shape
        ratio = np.abs(got - want) / allowance(want, want64)
        print(f"{tag} {what}: max |err| / allowance per column {ratio.max(0)}; |err| vs the f64 run {np.abs(got - want64).max(0)}")
        assert (ratio <= 1.0).all(), (what, ratio)
        # against the f64 run the plain bar holds: like it, this run takes no noise step at the start (docstring)
        assert (np.abs(got - want64) <= 1e-4 * np.maximum(1.0, np.abs(want64))).all(), (what, "the f64 trajectory, under the plain bar")
    for n, p in student.named_parameters():
        if p.requires_grad:
            want, diff = g[f"final::{tag}::{n}"].astype(np.float64), g[f"final_diff::{tag}::{n}"].astype(np.float64)
            bar = 1e-4 * max(1.0, np.abs(want).max())
            allow = np.where(np.abs(diff) > bar / 4, 4 * np.abs(diff), bar)      # per element
            got = p.detach().cpu().numpy().astype(np.float64)
            err, err64 = np.abs(got - want), np.abs(got - (want + diff)).max()
            print(f"{tag} {n}: max err / allowance = {(err / allow).max():.3f}; max |err| vs the f64 run / bar = {err64 / bar:.4f}")
            assert (err <= allow).all(), n
            assert err64 <= bar, (n, "the f64 run's tensor, under the plain bar")
    assert bool(g[f"swa_is_final::{tag}"]) and all(torch.equal(a, b) for a, b in zip(swa.parameters(), student.parameters()))


def test_the_existing_steps_do_not_open_the_fourth_library():
    """A fresh process runs ffn_reg_step and gs_lora_step: libgslora_kd.so is not loaded, not mapped."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = """
import sys
sys.path[:0] = [%r, %r, %r]
from types import SimpleNamespace
import torch
import loralib as lora
from oracle import recipe
from vit_pytorch_face import ViT_face
import test_hip_ffn_train as T
from gslora_hip import _lib_kd, step
from gslora_hip.optim import create_optimizer
args = SimpleNamespace(opt="adamw", weight_decay=0.05, opt_eps=1e-8, opt_betas=None, lr=1e-4)
crit = torch.nn.CrossEntropyLoss()
cfg = recipe.cfg_small(lora_rank=0)
m = T.build(cfg, "fp32")
x_r, y_r, x_f, y_f = T.batches(cfg, 3)
out = step.ffn_reg_step(m, create_optimizer(args, m), crit, x_r, y_r)
assert torch.isfinite(out).all()
cfg = recipe.cfg_small()
m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
             dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], lora_rank=cfg["lora_rank"])
lora.mark_only_lora_as_trainable(m)
m = m.to("cuda").set_compute_dtype("fp32").train()
step.gs_lora_step(m, create_optimizer(args, m), crit, x_r, y_r, x_f, y_f, beta=0.15, alpha=0.01, BND=105.0)
torch.cuda.synchronize()
assert not _lib_kd.loaded() and "libgslora_kd" not in open("/proc/self/maps").read()
assert "libgslora_hip" in open("/proc/self/maps").read()
print("ok")
""" % (os.path.dirname(here), os.path.join(os.path.dirname(here), "gs-lora_amd"), here)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
