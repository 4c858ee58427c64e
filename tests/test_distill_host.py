"""CPU tests of the LwF / DER / DER++ / FDR baselines: the fifth product library's ABI (header, version script, bindings and exported symbols
agree), lazy loading, no spilled register in its kernels, the launch rule gsf_rowdist_plan, every
refusal with its text, the three loops' signatures and remain-draw order against the reference's recorded ones, the exact zero of LwF's
distillation term, and the refusals distill_step makes before any launch. The arithmetic is tested on the GPU (tests/test_hip_fd_kernels.py,
tests/test_hip_distill.py)."""
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from product_libs import exported, kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"gsf_last_error", "gsf_rowdist_plan", "gsf_rowdist_ws_elems", "gsf_rowdist_fwd", "gsf_rowdist_bwd"}
METHODS = ("lwf", "der", "derpp", "fdr")


def test_header_version_script_bindings_and_exports_of_the_fifth_library_agree():
    from gslora_hip import _lib_fd, build
    header = open(os.path.join(ROOT, "include", "gslora_fd.h")).read()
    protos = dict(re.findall(r"GSL_API [a-z *]+\b(gsf_[a-z0-9_]+)\(([^;]*)\);", header))
    assert set(protos) == set(_lib_fd.SIGNATURES) == exported(build.side_out("fd")) == ENTRY_POINTS
    for name, argtypes in _lib_fd.SIGNATURES.items():
        proto = protos[name]
        n = 0 if proto.strip() in ("", "void") else len(proto.split(","))
        assert n == len(argtypes), name
    script = open(os.path.join(ROOT, "gs-lora_amd", "csrc", "exports_fd.map")).read()
    assert "global: gsf_*;" in script and "local: *;" in script
    for lines in ("baselines/DERtrain.py", "baselines/FDRtrain.py"):
        assert lines in header, "the header comment names the reference files"
    enums = dict(re.findall(r"(GSF_[A-Z]+) = (\d)", header))
    assert enums == {"GSF_WAVE": str(_lib_fd.FD_WAVE), "GSF_BLOCK": str(_lib_fd.FD_BLOCK), "GSF_SQ": str(_lib_fd.FD_SQ),
                     "GSF_ROWNORM": str(_lib_fd.FD_ROWNORM)}


def test_importing_the_new_modules_and_collecting_the_gpu_tests_opens_no_library():
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import test_hip_fd_kernels, test_hip_distill\n"
            "import gslora_hip, gslora_hip._lib_fd as f, gslora_hip._lib_kd as k, gslora_hip.fd, gslora_hip.step\n"
            "import baselines.Lwftrain, baselines.DERtrain, baselines.FDRtrain, driver_distill\n"
            "assert not f.loaded() and not k.loaded()\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'libgslora_fd' not in maps and 'libgslora_kd' not in maps\n"
            "f.load(); assert f.loaded() and 'libgslora_fd' in open('/proc/self/maps').read()\n"
            "assert 'libgslora_kd' not in open('/proc/self/maps').read()\n" % (ROOT, os.path.join(ROOT, "gs-lora_amd"), os.path.join(ROOT, "tests")))
    subprocess.check_call([sys.executable, "-c", code])


def test_no_kernel_of_the_fifth_library_spills_registers():
    """Read from the code-object notes (product_libs.kernel_notes): every gfx950 kernel of libgslora_fd.so declares
    .vgpr_spill_count 0 and no private segment, and is bound by __launch_bounds__(256)."""
    from gslora_hip import build as B
    notes = kernel_notes(B.side_out("fd"))
    kernels, bad = [k[0] for k in notes], [k for k in notes if k[1] or k[2] or k[3] != 256]
    # rows (wave, block) x (16-byte, 4-byte), reduce, bwd (wave, block) x (16-byte, 4-byte)
    assert len(kernels) == 9 and sum("fd_rows" in k for k in kernels) == 4 and sum("fd_bwd" in k for k in kernels) == 4, kernels
    assert not bad, bad


def threshold():
    """The first W the workgroup-per-row kernel serves, found through gsf_rowdist_plan by bisection (the rule is monotone: checked below)."""
    from gslora_hip import _lib_fd as LF
    lo, hi = 1, 1 << 20
    assert LF.rowdist_plan(4, lo)[0] == LF.FD_WAVE and LF.rowdist_plan(4, hi)[0] == LF.FD_BLOCK
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if LF.rowdist_plan(4, mid)[0] == LF.FD_WAVE else (lo, mid)
    return hi


def test_the_plan_reaches_both_kernels_and_is_monotone_in_W():
    from gslora_hip import _lib_fd as LF
    thr = threshold()
    assert thr == 1025, "include/gslora_fd.h: a wave serves a row up to 1024 elements"
    kinds = [LF.rowdist_plan(9, W)[0] for W in list(range(1, 2200)) + [10572, 93431, 1 << 30]]
    assert kinds == sorted(kinds) and kinds[0] == LF.FD_WAVE and kinds[-1] == LF.FD_BLOCK
    assert all(LF.rowdist_plan(B, W)[0] == LF.rowdist_plan(1, W)[0] for B in (1, 4, 513) for W in (1, thr - 1, thr, 93431)), "W alone decides"
    for B in (1, 3, 4, 5, 9, 512):
        assert LF.rowdist_plan(B, thr - 1)[1:] == (-(-B // 4), B), "four rows per workgroup"
        assert LF.rowdist_plan(B, thr)[1:] == (B, B), "a workgroup per row"
        assert LF.rowdist_ws_elems(B, 93431) == B, "the widest head of the reference (93 431 classes) is served"


def test_every_refusal_has_its_text():
    """Each call is valid in all but one argument (pointers are never followed: the check comes before any launch)."""
    from gslora_hip import _lib_fd as LF
    lib = LF.load()
    P = 4096
    fwd = dict(a=P, ld_a=8, t=P, ld_t=8, B=2, W=8, mode=0, out=P, ws=P)
    bwd = dict(a=P, ld_a=8, t=P, ld_t=8, ws=P, gout=P, B=2, W=8, mode=1, coef=0.5, d=P, ld_d=8, acc=0)
    cases = [(dict(B=0), b"B >= 1"), (dict(W=0), b"W >= 1"), (dict(W=(1 << 30) + 1, ld_a=1 << 31, ld_t=1 << 31), b"W <= 2^30"),
             (dict(a=None), b"null a or t"), (dict(t=None), b"null a or t"), (dict(ld_a=7), b"ld_a >= W"), (dict(ld_t=7), b"ld_t >= W"),
             (dict(mode=2), b"mode is GSF_SQ or GSF_ROWNORM"), (dict(mode=-1), b"mode is GSF_SQ or GSF_ROWNORM")]
    for change, text in cases + [(dict(out=None), b"null out"), (dict(ws=None), b"null ws")]:
        assert lib.gsf_rowdist_fwd(*{**fwd, **change}.values(), None) == -1 and text in lib.gsf_last_error(), change
        assert b"gsf_rowdist_fwd" in lib.gsf_last_error()
    for change, text in cases + [(dict(ws=None), b"null ws, gout or d"), (dict(gout=None), b"null ws"), (dict(d=None), b"null ws"),
                                 (dict(ld_d=7), b"ld_d >= W")]:
        assert lib.gsf_rowdist_bwd(*{**bwd, **change}.values(), None) == -1 and text in lib.gsf_last_error(), change
        assert b"gsf_rowdist_bwd" in lib.gsf_last_error()
    assert lib.gsf_rowdist_ws_elems(0, 4) == -1 and lib.gsf_rowdist_ws_elems(4, 0) == -1 and lib.gsf_rowdist_ws_elems(4, (1 << 30) + 1) == -1
    with pytest.raises(RuntimeError, match="B >= 1, W >= 1"):
        LF.rowdist_plan(0, 5)
    with pytest.raises(RuntimeError, match="refused"):
        LF.rowdist_ws_elems(3, 0)


def test_the_python_wrappers_refuse_before_the_library():
    from baselines.DERtrain import DER_regularzaion_loss
    from baselines.FDRtrain import regularization_loss
    from gslora_hip import fd
    a = torch.zeros(2, 4)
    for call in (lambda: fd.row_dist(a, 0, 2, a, "sq", 1.0), lambda: DER_regularzaion_loss(a, a), lambda: regularization_loss(a, a)):
        with pytest.raises(RuntimeError, match="no CPU\\s+fallback"):
            call()
    with pytest.raises(ValueError, match="mode must be one of"):
        fd.row_dist(a, 0, 2, a, "kl", 1.0)
    assert list(inspect.signature(fd.row_dist).parameters) == ["full", "row0", "nrows", "t", "mode", "coef"]
    assert list(inspect.signature(DER_regularzaion_loss).parameters) == ["preds", "gts"]
    assert list(inspect.signature(regularization_loss).parameters) == ["outputs", "target_logits"]


def test_distill_step_signature_and_refusals_before_any_launch(monkeypatch):
    from gslora_hip import step
    sig = inspect.signature(step.distill_step)
    assert list(sig.parameters) == ["student", "teacher", "optimizer", "criterion", "x_f", "y_f", "x_r", "y_r", "method", "lam", "lam_aux", "x_n", "y_n"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("method", "lam", "lam_aux", "x_n", "y_n"))
    assert (sig.parameters["lam_aux"].default, sig.parameters["x_n"].default, sig.parameters["y_n"].default) == (0.0, None, None)
    kw = dict(method="fdr", lam=0.1)
    from vit_pytorch_face import ViT_face
    from vit_pytorch_face.modified_VIT import ModifiedViT
    geo = dict(loss_type="CosFace", GPU_ID=[0], num_class=10, image_size=40, patch_size=8, dim=64, depth=1, heads=1, mlp_dim=128)
    with_lora, plain = ViT_face(lora_rank=4, **geo), ViT_face(lora_rank=0, **geo)
    x, y = torch.zeros(2, 3, 40, 40), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="holds LoRA adapters \\(lora_rank = 4\\)"):
        step.distill_step(with_lora, plain, None, None, x, y, x, y, **kw)
    with pytest.raises(RuntimeError, match="ModifiedViT has no FFN weights that train on the HIP path"):
        step.distill_step(object.__new__(ModifiedViT), plain, None, None, x, y, x, y, **kw)      # (refused by its class alone)
    graphed = object.__new__(step.GraphedStep)
    with pytest.raises(RuntimeError, match="distill_step is eager; GraphedStep captures the LoRA-only step"):
        step.distill_step(graphed, plain, None, None, x, y, x, y, **kw)
    replicated = object.__new__(torch.nn.DataParallel)
    torch.nn.Module.__init__(replicated)
    replicated.device_ids, replicated.module = [0, 1], plain
    with pytest.raises(RuntimeError, match="nn.DataParallel over several devices is not supported"):
        step.distill_step(replicated, plain, None, None, x, y, x, y, **kw)
    with pytest.raises(ValueError, match="method must be one of"):
        step.distill_step(plain, plain, None, None, x, y, x, y, method="lirf", lam=0.1)
    with pytest.raises(ValueError, match="only with method 'der'"):
        step.distill_step(plain, plain, None, None, x, y, x, y, method="fdr", lam=0.1, x_n=x, y_n=y)
    with pytest.raises(ValueError, match="given together"):
        step.distill_step(plain, plain, None, None, x, y, x, y, method="der", lam=0.1, x_n=x)
    monkeypatch.setattr(step, "_world", lambda: 2)
    with pytest.raises(RuntimeError, match="distill_step runs in one process.*a process group of 2 ranks is active"):
        step.distill_step(plain, plain, None, None, x, y, x, y, **kw)
    assert "the teacher is NOT run" in step.distill_step.__doc__ and "L_old_kd_loss" in step.distill_step.__doc__


def loops():
    from baselines.DERtrain import train_one_epoch_DER
    from baselines.FDRtrain import train_one_epoch_FDR
    from baselines.Lwftrain import train_one_epoch_Lwf
    return dict(train_one_epoch_Lwf=train_one_epoch_Lwf, train_one_epoch_DER=train_one_epoch_DER, train_one_epoch_FDR=train_one_epoch_FDR)


def test_the_three_loops_have_the_reference_signatures(golden_dir):
    want = json.load(open(os.path.join(golden_dir, "distill_signatures.json")))
    assert set(want) == set(loops())
    for name, fn in loops().items():
        sig = inspect.signature(fn)
        assert list(sig.parameters) == want[name]["parameters"], name
        assert {n: p.default for n, p in sig.parameters.items() if p.default is not inspect.Parameter.empty} == want[name]["defaults"], name
    assert [want[n]["returns"] for n in ("train_one_epoch_Lwf", "train_one_epoch_DER", "train_one_epoch_FDR")] == [6, 5, 5]
    assert want["train_one_epoch_FDR"]["parameters"][2] == "criterion", "FDR takes the criterion third"
    from baselines import _distill
    assert (_distill.DISP_FREQ, _distill.VER_FREQ) == (5, 100)


def test_l_old_kd_loss_is_the_reference_s_recorded_zero(golden_dir):
    from baselines.Lwftrain import L_old_kd_loss
    g = np.load(os.path.join(golden_dir, "distill_small.npz"))
    rec = g["lwf_zero"]      # (C, value, largest gradient element) of the reference's function on CPU tensors
    assert rec[:, 0].tolist() == [2.0, 1000.0] and not rec[:, 1:].any(), "the reference's value and gradient are exact zeros"
    for C in (2, 1000):
        gen = torch.Generator().manual_seed(C)
        p = (3.0 * torch.randn(4, C, generator=gen)).requires_grad_(True)
        v = L_old_kd_loss(p, 3.0 * torch.randn(4, C, generator=gen), temperature=2.0)
        assert v.dim() == 0 and v.dtype == torch.float32 and v.item() == 0.0 and not v.requires_grad
    with pytest.raises(ValueError, match="num_class >= 2"):
        L_old_kd_loss(torch.zeros(4, 1), torch.zeros(4, 1))
    assert list(inspect.signature(L_old_kd_loss).parameters) == ["preds", "gts", "temperature"]
    assert inspect.signature(L_old_kd_loss).parameters["temperature"].default == 2.0


class _Meter:
    def __init__(self):
        self.updates = []
        self.val = self.avg = 0.0
        self.count = 0

    def update(self, v, n=1):
        self.updates.append((v, n))
        self.val = self.avg = v
        self.count += n

    def reset(self):
        self.count = 0


@pytest.mark.parametrize("method", METHODS)
def test_the_remain_draw_order_is_the_reference_s(golden_dir, method, monkeypatch):
    """The loop over CPU loaders of the fixture's shape (3 forget batches of 3, 3 remain batches of 2, labelled as the fixture's) with a stub
    step: the labels of the batches handed to the step, in order, are the ones the real reference loop handed its model."""
    from baselines import _distill
    g = np.load(os.path.join(golden_dir, "distill_small.npz"))
    want = g[f"labels::{method}_copy"]
    assert np.array_equal(want, g[f"labels::{method}_far"])
    per = 7 if method == "derpp" else 5      # per step: 3 forget labels, 2 remain (, 2 of the second remain batch)
    assert want.shape == (3 * per,)
    steps = want.reshape(3, per)
    forget = [(torch.zeros(3, 1), torch.from_numpy(steps[k, :3].copy())) for k in range(3)]
    # the remain loader's batches in loader order: step 1 sees batch 0; DER++ sees batch 1 inside step 1 and batch 2 in step 2
    order = [steps[0, 3:5], steps[0, 5:7], steps[1, 3:5]] if method == "derpp" else [steps[0, 3:5], steps[1, 3:5], steps[2, 3:5]]
    remain = [(torch.zeros(2, 1), torch.from_numpy(o.copy())) for o in order]
    assert len({tuple(o.tolist()) for o in order}) == 3, "the three remain batches are told apart by their labels"
    seen, calls = [], []

    def stub(student, teacher, optimizer, criterion, x_f, y_f, x_r, y_r, *, method, lam, lam_aux=0.0, x_n=None, y_n=None):
        seen.extend([y_f.numpy(), y_r.numpy()] + ([] if y_n is None else [y_n.numpy()]))
        calls.append((method, lam, lam_aux, x_n is not None))
        return torch.tensor([1.0, 2.0, 3.0, 4.0])

    monkeypatch.setattr(_distill, "distill_step", stub)
    fns = loops()
    model = torch.nn.Linear(1, 1)
    common = dict(student_model=model, teacher_model=torch.nn.Linear(1, 1), data_loader_cl_forget=forget, remain_loader=remain,
                  criterion=torch.nn.CrossEntropyLoss(), optimizer=None, device=torch.device("cpu"), epoch=0, batch=0, task_i=0,
                  testloader_forget=None, testloader_remain=None, forget_acc_before=0.0, highest_H_mean=0.5, cfg={})
    if method == "lwf":
        m = {k: _Meter() for k in ("losses_CE", "losses_KD", "losses_total", "losses_remain")}
        out = fns["train_one_epoch_Lwf"](lambda_kd=0.5, lambda_remain=1.0, temperature=2.0, **common, **m)
        assert len(out) == 6 and out[2:] == (m["losses_CE"], m["losses_KD"], m["losses_remain"], m["losses_total"])
        assert calls == [("lwf", 0.5, 1.0, False)] * 3
        assert [u[0] for u in m["losses_remain"].updates] == [3.0] * 3 and [u[0] for u in m["losses_KD"].updates] == [2.0] * 3
    elif method in ("der", "derpp"):
        m = {k: _Meter() for k in ("losses_CE", "losses_DER", "losses_total")}
        out = fns["train_one_epoch_DER"](lambda_der=0.1, plus=method == "derpp", lambda_der_plus=0.2, **common, **m)
        assert len(out) == 5 and out[2:] == (m["losses_CE"], m["losses_DER"], m["losses_total"])
        assert calls == [("der", 0.1, 0.2, method == "derpp")] * 3
    else:
        m = {k: _Meter() for k in ("losses_CE", "losses_FDR", "losses_total")}
        out = fns["train_one_epoch_FDR"](reg_lambda=0.3, **common, **m)
        assert len(out) == 5 and out[2:] == (m["losses_CE"], m["losses_FDR"], m["losses_total"])
        assert calls == [("fdr", 0.3, 0.0, False)] * 3
    assert out[:2] == (3, 0.5)
    assert np.array_equal(np.concatenate(seen), want)
    assert [u for u in m["losses_CE"].updates] == [(1.0, 3)] * 3 and [u for u in m["losses_total"].updates] == [(4.0, 3)] * 3
    assert model.training


def test_the_display_interval_resets_the_meters_in_place(monkeypatch, capsys):
    """Six steps from batch 0: step 5 is a display step (one flush, one line, the meters reset in place), step 6 is flushed at the return."""
    from baselines import _distill
    from baselines.FDRtrain import train_one_epoch_FDR
    monkeypatch.setattr(_distill, "distill_step", lambda *a, **k: torch.tensor([1.0, 2.0, 0.0, 3.0]))
    forget = [(torch.zeros(3, 1), torch.zeros(3, dtype=torch.int64))] * 6
    remain = [(torch.zeros(2, 1), torch.zeros(2, dtype=torch.int64))] * 2
    m = {k: _Meter() for k in ("losses_CE", "losses_FDR", "losses_total")}
    out = train_one_epoch_FDR(torch.nn.Linear(1, 1), torch.nn.Linear(1, 1), torch.nn.CrossEntropyLoss(), forget, remain, None, torch.device("cpu"),
                              0, 0, reg_lambda=0.1, task_i=0, testloader_forget=None, testloader_remain=None, forget_acc_before=0.0,
                              highest_H_mean=0.0, cfg={}, **m)
    assert out[0] == 6 and len(m["losses_FDR"].updates) == 6 and m["losses_FDR"].count == 3, "five updates were reset, one came after"
    assert capsys.readouterr().out.count("Training FDR Loss 2.0000") == 1


def test_the_driver_parses_the_reference_defaults_and_refuses(monkeypatch, capsys):
    import driver_distill
    a = driver_distill.get_args(["--method", "derpp"])
    # util/args.py:273-295 of the reference, typed here
    assert (a.Lwf_T, a.Lwf_lambda_kd, a.Lwf_lambda_remain, a.DER_lambda, a.DER_plus_lambda, a.FDR_lambda) == (2, 0.5, 1, 0.1, 0.1, 0.1)
    assert a.only_ffn and not a.ffn_open and a.opt == "adamw" and a.epochs == 1
    assert driver_distill.get_args(["--method", "lwf", "--Lwf_T", "3"]).Lwf_T == 3.0
    with pytest.raises(SystemExit):
        driver_distill.get_args(["--method", "lirf"])
    with pytest.raises(SystemExit):
        driver_distill.get_args(["--method", "lwf", "--num_class", "1"])
    assert "L_old_kd_loss is NaN for one class" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        driver_distill.get_args([])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        driver_distill.main(["--method", "fdr", "--small"])


def test_the_fixtures_hold_arrays_only_and_regenerate_to_the_same_bits(golden_dir, tmp_path):
    files = ["distill_small.npz"] + [f"distill_small_{m}.npz" for m in METHODS]
    g = np.load(os.path.join(golden_dir, files[0]), allow_pickle=False)
    names = g["trainable"].tolist()
    assert len(names) == 9 and g["hyper"].shape == (8,)
    for method in METHODS:
        path = os.path.join(golden_dir, f"distill_small_{method}.npz")
        assert os.path.getsize(path) < (1 << 20)
        t = np.load(path, allow_pickle=False)
        assert all(t[k].dtype == np.float32 for k in t.files)
        k = 4 if method == "lwf" else 3
        for teacher in ("copy", "far"):
            tag = f"{method}_{teacher}"
            assert g[f"meters::{tag}"].shape == g[f"meters64::{tag}"].shape == (3, k)
            assert sum(f.startswith(f"grad::{tag}::") for f in t.files) == sum(f.startswith(f"grad_diff::{tag}::") for f in t.files) == 9
            assert sum(f.startswith(f"final::{tag}::") for f in t.files) == (9 if teacher == "far" else 0)
            m = g[f"meters::{tag}"]
            if method == "lwf":      # CE + 0.5 * 0 + 1 * CE_remain
                assert not m[:, 1].any() and np.allclose(m[:, 3], m[:, 0] + m[:, 2], rtol=1e-6, atol=0)
            else:
                assert (m[:, 1] > 1e-2).all() if teacher == "far" else m[0, 1] == 0.0, "a far teacher stands off; a copy starts at distance 0"
                if method != "derpp":
                    assert np.allclose(m[:, 2], m[:, 0] + 0.1 * m[:, 1], rtol=1e-6, atol=0)
                else:
                    assert (m[:, 2] > m[:, 0] + 0.1 * m[:, 1]).all(), "DER++ adds a positive cross-entropy"
    from oracle.make_golden import REF
    if not os.path.isdir(os.path.join(REF, "vit_pytorch_face")):
        pytest.skip("the reference sources are not on this machine")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_golden_distill.py"), "--out", str(tmp_path)], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL)
    for f in files:
        old, new = np.load(os.path.join(golden_dir, f)), np.load(os.path.join(str(tmp_path), f))
        assert sorted(old.files) == sorted(new.files)
        for k in old.files:
            assert old[k].dtype == new[k].dtype and old[k].shape == new[k].shape and np.array_equal(old[k], new[k]), (f, k)
    assert json.load(open(os.path.join(str(tmp_path), "distill_signatures.json"))) == json.load(open(os.path.join(golden_dir, "distill_signatures.json")))
