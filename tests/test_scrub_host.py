"""CPU tests of the SCRUB loss side: the fourth product library's ABI (header, version script, bindings and exported symbols agree),
lazy loading, no spilled register in its kernels, the launch rule gsk_kd_plan, the host-side layout of
the batched parameter distance, every refusal with its text, the step schedule of util/sgda_utils.py against values worked by hand, and the
refusals scrub_step makes before any launch. The arithmetic is tested on the GPU (tests/test_hip_kd_kernels.py, tests/test_hip_scrub.py)."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from product_libs import exported, kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"gsk_last_error", "gsk_kd_plan", "gsk_kd_ws_elems", "gsk_kd_ce_fwd", "gsk_kd_ce_bwd", "gsk_param_dist_layout",
                "gsk_param_dist_fwd", "gsk_param_dist_bwd"}


def test_header_version_script_bindings_and_exports_of_the_fourth_library_agree():
    from gslora_hip import _lib_kd, build
    header = open(os.path.join(ROOT, "include", "gslora_kd.h")).read()
    protos = dict(re.findall(r"GSL_API [a-z *]+\b(gsk_[a-z0-9_]+)\(([^;]*)\);", header))
    assert set(protos) == set(_lib_kd.SIGNATURES) == exported(build.side_out("kd")) == ENTRY_POINTS
    for name, argtypes in _lib_kd.SIGNATURES.items():
        proto = protos[name]
        n = 0 if proto.strip() in ("", "void") else len(proto.split(","))
        assert n == len(argtypes), name
    script = open(os.path.join(ROOT, "gs-lora_amd", "csrc", "exports_kd.map")).read()
    assert "global: gsk_*;" in script and "local: *;" in script
    for lines in ("util/sgda_utils.py", "baselines/SCRUBtrain.py"):
        assert lines in header, "the header comment names the reference files"
    body = re.search(r"typedef struct gsk_dist_entry \{(.*?)\} gsk_dist_entry;", header, re.S).group(1)
    fields = re.findall(r"\b(\w+);", body)
    assert fields == [f[0] for f in _lib_kd.DistEntry._fields_]
    assert ctypes.sizeof(_lib_kd.DistEntry) == 56


def test_collecting_the_gpu_tests_opens_no_library():
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import test_hip_kd_kernels, test_hip_scrub\n"
            "from gslora_hip import _lib_kd\n"
            "assert not _lib_kd.loaded()\n" % (ROOT, os.path.join(ROOT, "gs-lora_amd"), os.path.join(ROOT, "tests")))
    subprocess.check_call([sys.executable, "-c", code])


def test_the_fourth_library_is_opened_lazily():
    """(Imports and a ParamDist with smoothing 0; that the existing STEP paths leave it closed is checked on the GPU, in a fresh process:
    tests/test_hip_scrub.py::test_the_existing_steps_do_not_open_the_fourth_library.)"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import gslora_hip, gslora_hip._lib_kd as k, gslora_hip.kd, gslora_hip.step, gslora_hip.reg, util.sgda_utils, engine_reg, engine_cl\n"
            "import torch\n"
            "assert not k.loaded()\n"
            "assert 'libgslora_kd' not in open('/proc/self/maps').read()\n"
            "m, a = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)\n"
            "d = gslora_hip.kd.ParamDist(m, a, 0.0)\n"      # smoothing 0: nothing is laid out
            "z = d.loss(); assert z.dim() == 0 and z.item() == 0.0 and not z.requires_grad\n"
            "assert not k.loaded()\n"
            "k.load(); assert k.loaded() and 'libgslora_kd' in open('/proc/self/maps').read()\n"
            "assert 'libgslora_reg' not in open('/proc/self/maps').read()\n" % (ROOT, os.path.join(ROOT, "gs-lora_amd")))
    subprocess.check_call([sys.executable, "-c", code])


def test_no_kernel_of_the_fourth_library_spills_registers():
    """Read from the code-object notes (product_libs.kernel_notes): every gfx950 kernel of libgslora_kd.so declares
    .vgpr_spill_count 0 and no private segment, and is bound by __launch_bounds__(256)."""
    from gslora_hip import build as B
    notes = kernel_notes(B.side_out("kd"))
    kernels, bad = [k[0] for k in notes], [k for k in notes if k[1] or k[2] or k[3] != 256]
    # kd rows (wave, block), reduce, bwd (wave, block); param_dist partial, reduce, bwd
    assert len(kernels) == 8 and sum("kd_" in k for k in kernels) == 5 and sum("param_dist" in k for k in kernels) == 3, kernels
    assert not bad, bad


def threshold():
    """The first C the workgroup-per-row kernel serves, found through gsk_kd_plan by bisection (the rule is monotone: checked below)."""
    from gslora_hip import _lib_kd as LK
    lo, hi = 1, 1 << 20
    assert LK.kd_plan(4, lo)[0] == LK.KD_WAVE and LK.kd_plan(4, hi)[0] == LK.KD_BLOCK
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if LK.kd_plan(4, mid)[0] == LK.KD_WAVE else (lo, mid)
    return hi


def test_the_plan_reaches_both_kernels_and_is_monotone_in_C():
    from gslora_hip import _lib_kd as LK
    thr = threshold()
    assert thr == 1025, "DESIGN.md section 9m: a wave holds 16 values per lane of each row"
    kinds = [LK.kd_plan(9, C)[0] for C in list(range(1, 2200)) + [10572, 93431, 1 << 30]]
    assert kinds == sorted(kinds) and kinds[0] == LK.KD_WAVE and kinds[-1] == LK.KD_BLOCK
    assert all(LK.kd_plan(B, C)[0] == LK.kd_plan(1, C)[0] for B in (1, 4, 513) for C in (1, thr - 1, thr, 93431)), "the kernel depends on C alone"
    for B in (1, 3, 4, 5, 9, 512):
        assert LK.kd_plan(B, thr - 1)[1:] == (-(-B // 4), 5 * B), "four rows per workgroup"
        assert LK.kd_plan(B, thr)[1:] == (B, 5 * B), "a workgroup per row"
        assert LK.kd_ws_elems(B, 100) == 5 * B >= 3 * B, "the workspace covers the three log-sum-exps of every row"


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 70001, 2 ** 20, 2 ** 20 + 1, 3 * 2 ** 20 + 5])
def test_param_dist_layout(n):
    """Entries in parameter order; the partition of gsr_reg_multi_layout; frozen entries without a place in the gradient buffer; trainable
    places multiples of four elements, disjoint, ascending."""
    from gslora_hip import _lib_kd as LK
    sizes = [5, n, 3, n, 7, 1, 2]
    train = [True, False, True, True, False, False, True]
    entries = [(0x1000 * (k + 1), 0x100000 * (k + 1), sizes[k], train[k]) for k in range(7)]
    table, total, bwd, g_elems = LK.param_dist_layout(entries)
    blk = bblk = goff = 0
    spans = []
    for k in range(7):
        e, nb = table[k], min(1024, -(-sizes[k] // 1024))
        assert (e.p, e.q, e.n) == entries[k][:3], "parameter order"
        assert (e.nblk, e.chunk, e.blk0, e.bblk0) == (nb, -(-sizes[k] // nb), blk, bblk), k
        assert e.nblk * e.chunk >= e.n > (e.nblk - 1) * e.chunk      # every workgroup has work
        blk += nb
        if train[k]:
            assert e.goff == goff and e.goff % 4 == 0
            spans.append((e.goff, e.goff + e.n))
            goff += (sizes[k] + 3) // 4 * 4
            bblk += nb
        else:
            assert e.goff == -1
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "disjoint"
    assert (total, bwd, g_elems) == (blk, bblk, goff)
    # nothing trains: no backward workgroup, no gradient element
    _, total, bwd, g_elems = LK.param_dist_layout([(0x1000, 0x2000, n, False)])
    assert (bwd, g_elems) == (0, 0) and total == min(1024, -(-n // 1024))


def test_every_refusal_has_its_text():
    """Each call is valid in all but one argument (pointers are never followed: the check comes before any launch)."""
    from gslora_hip import _lib_kd as LK
    lib = LK.load()
    P = 4096
    fwd = dict(ys=P, ld_s=8, yt=P, ld_t=8, labels=P, B=2, C=8, T=2.0, c_kd=1.0, c_ce=1.0, out=P, ws=P)
    bwd = dict(ys=P, ld_s=8, yt=P, ld_t=8, labels=P, ws=P, gout=P, B=2, C=8, T=2.0, c_kd=1.0, c_ce=1.0, d=P, ld_d=8, acc=0)
    cases = [(dict(T=0.0), b"T > 0"), (dict(T=-1.0), b"T > 0"), (dict(T=float("nan")), b"T > 0"), (dict(ld_s=7), b"ld_s >= C"),
             (dict(ld_t=7), b"ld_t >= C"), (dict(B=0), b"B >= 1"), (dict(C=0), b"C >= 1"), (dict(ys=None), b"null logits"),
             (dict(yt=None), b"null logits"), (dict(labels=None), b"labels == NULL needs c_ce == 0")]
    for change, text in cases + [(dict(out=None), b"null out"), (dict(ws=None), b"null ws")]:
        assert lib.gsk_kd_ce_fwd(*{**fwd, **change}.values(), None) == -1 and text in lib.gsk_last_error(), change
        assert b"gsk_kd_ce_fwd" in lib.gsk_last_error()
    for change, text in cases + [(dict(ws=None), b"null ws, gout or d"), (dict(gout=None), b"null ws"), (dict(d=None), b"null ws"),
                                 (dict(ld_d=7), b"ld_d >= C")]:
        assert lib.gsk_kd_ce_bwd(*{**bwd, **change}.values(), None) == -1 and text in lib.gsk_last_error(), change
        assert b"gsk_kd_ce_bwd" in lib.gsk_last_error()
    assert lib.gsk_kd_ws_elems(0, 4) == -1 and lib.gsk_kd_ws_elems(4, 0) == -1 and lib.gsk_kd_ws_elems(4, (1 << 30) + 1) == -1
    with pytest.raises(RuntimeError, match="B >= 1, C >= 1"):
        LK.kd_plan(0, 5)
    with pytest.raises(RuntimeError, match="1 <= n < 2\\^31"):
        LK.param_dist_layout([(P, P, 0, True)])
    with pytest.raises(RuntimeError, match="null tensor"):
        LK.param_dist_layout([(P, None, 4, True)])
    with pytest.raises(RuntimeError, match="4-byte aligned"):
        LK.param_dist_layout([(P, P + 2, 4, True)])
    with pytest.raises(RuntimeError, match="1 <= n_entries"):
        LK.param_dist_layout([])
    assert lib.gsk_param_dist_fwd(None, 1, 1, 0.5, P, P, P, None) == -1 and b"null table" in lib.gsk_last_error()
    assert lib.gsk_param_dist_fwd(P, 1, 1, 0.5, P, P, None, None) == -1 and b"null ws" in lib.gsk_last_error()
    assert lib.gsk_param_dist_fwd(P, 2, 1, 0.5, P, P, P, None) == -1 and b"n_entries <= total_blocks" in lib.gsk_last_error()
    assert lib.gsk_param_dist_bwd(P, 1, 0, 0.5, P, P, P, None) == -1 and b"1 <= bwd_blocks" in lib.gsk_last_error()
    assert lib.gsk_param_dist_bwd(P, 1, 1, 0.5, None, P, P, None) == -1 and b"null table, gout, norms or g" in lib.gsk_last_error()
    assert lib.gsk_param_dist_bwd(P, 1, 1, 0.5, P, P, P + 2, None) == -1 and b"g is 4-byte aligned" in lib.gsk_last_error()


def test_the_python_wrappers_refuse_before_the_library():
    from gslora_hip import kd
    ys = torch.zeros(2, 4)
    with pytest.raises(RuntimeError, match="no CPU\\s+fallback"):
        kd.kd_ce(ys, ys, None, 2.0, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="no CPU\\s+fallback"):
        kd.DistillKL(2.0)(ys, ys)
    model, same, longer = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2), torch.nn.Sequential(torch.nn.Linear(2, 2), torch.nn.Linear(1, 1, bias=False))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kd.ParamDist(model, same, 0.1)
    with pytest.raises(ValueError, match="the model has 2 parameters, the averaged copy 3"):
        kd.ParamDist(model, longer, 0.1)
    d = kd.ParamDist(model, torch.nn.Linear(2, 2), 0.0)      # the two models are held weakly (a cache may key on them): this copy is gone
    with pytest.raises(RuntimeError, match="no longer exists"):
        d._pairs()
    assert "0.0 times a finite distance is 0" in kd.ParamDist.__doc__
    assert list(inspect.signature(kd.kd_ce).parameters) == ["ys", "yt", "labels", "T", "c_kd", "c_ce"]
    assert list(inspect.signature(kd.DistillKL.__init__).parameters) == ["self", "T"]
    assert list(inspect.signature(kd.DistillKL.forward).parameters) == ["self", "y_s", "y_t"]


class _Opt:
    def __init__(self, lr):
        self.param_groups = [{"lr": lr}, {"lr": lr}]


def test_adjust_learning_rate_against_values_worked_by_hand():
    """lr_decay_epochs (3, 5, 9), rate 0.1, base 0.01. Epochs 0..3: no entry is strictly below the epoch -> 0.01 returned and the optimizer
    NOT written; 4, 5: one -> 0.001; 6..9: two -> 0.0001; 10: three -> 0.00001."""
    from util import sgda_utils as U
    assert list(inspect.signature(U.adjust_learning_rate).parameters) == ["epoch", "opt", "optimizer"]
    assert list(inspect.signature(U.param_dist).parameters) == ["model", "swa_model", "p"]
    from gslora_hip import kd
    assert U.DistillKL is kd.DistillKL
    opt = {"lr_decay_epochs": [3, 5, 9], "lr_decay_rate": 0.1, "sgda_learning_rate": 0.01}
    by_hand = {0: 0.01, 2: 0.01, 3: 0.01, 4: 0.001, 5: 0.001, 6: 0.0001, 9: 0.0001, 10: 0.00001, 100: 0.00001}
    for epoch, want in by_hand.items():
        o = _Opt(0.5)
        got = U.adjust_learning_rate(epoch, opt, o)
        assert got == pytest.approx(want, rel=1e-12), epoch
        wrote = [g["lr"] for g in o.param_groups]
        assert wrote == ([0.5, 0.5] if epoch <= 3 else [got, got]), "below and at the first decay epoch the optimizer keeps its rate"
    assert U.adjust_learning_rate(7, {**opt, "lr_decay_epochs": []}, _Opt(1.0)) == 0.01
    # the single epoch the reference's config stores (lr_decay_epochs = args.scrub_decay_epoch): at 100 nothing, at 101 one decay
    single = {**opt, "lr_decay_epochs": 100}
    assert U.adjust_learning_rate(100, single, _Opt(1.0)) == 0.01 and U.adjust_learning_rate(101, single, _Opt(1.0)) == pytest.approx(0.001, rel=1e-12)


def test_scrub_step_signature_and_refusals_before_any_launch(monkeypatch):
    from gslora_hip import step
    sig = inspect.signature(step.scrub_step)
    assert list(sig.parameters) == ["student", "teacher", "optimizer", "criterion", "x", "y", "maximize", "kd_T", "sgda_gamma", "sgda_alpha", "dist"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("maximize", "kd_T", "sgda_gamma", "sgda_alpha", "dist"))
    assert sig.parameters["dist"].default is None
    kw = dict(maximize=True, kd_T=2.0, sgda_gamma=0.99, sgda_alpha=0.001)
    from vit_pytorch_face import ViT_face
    from vit_pytorch_face.modified_VIT import ModifiedViT
    geo = dict(loss_type="CosFace", GPU_ID=[0], num_class=10, image_size=40, patch_size=8, dim=64, depth=1, heads=1, mlp_dim=128)
    with_lora, plain = ViT_face(lora_rank=4, **geo), ViT_face(lora_rank=0, **geo)
    x, y = torch.zeros(2, 3, 40, 40), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="holds LoRA adapters \\(lora_rank = 4\\)"):
        step.scrub_step(with_lora, plain, None, None, x, y, **kw)
    with pytest.raises(RuntimeError, match="ModifiedViT has no FFN weights that train on the HIP path"):
        step.scrub_step(object.__new__(ModifiedViT), plain, None, None, x, y, **kw)      # (refused by its class alone: nothing of it is read)
    graphed = object.__new__(step.GraphedStep)
    with pytest.raises(RuntimeError, match="scrub_step is eager; GraphedStep captures the LoRA-only step"):
        step.scrub_step(graphed, plain, None, None, x, y, **kw)
    monkeypatch.setattr(step, "_world", lambda: 2)
    with pytest.raises(RuntimeError, match="scrub_step runs in one process.*a process group of 2 ranks is active"):
        step.scrub_step(plain, plain, None, None, x, y, **kw)


REFERENCE_PARAMETERS = ["student", "teacher", "swa_model", "data_loader_forget", "remain_loader", "criterion", "optimizer", "device", "superepoch",
                        "batch", "losses_CE", "losses_total_forget", "losses_total_remain", "losses_kd_remain", "losses_kd_forget", "task_i",
                        "testloader_forget", "testloader_remain", "forget_acc_before", "highest_H_mean", "cfg", "kd_T", "sgda_smoothing", "sgda_gamma",
                        "sgda_alpha", "testloader_open"]      # reference baselines/SCRUBtrain.py:11-38


def test_the_superepoch_loop_has_the_reference_parameters():
    from baselines.SCRUBtrain import DISP_FREQ, VER_FREQ, ScrubForgetQueue, ScrubRemainQueue, train_one_superepoch_SCRUB
    sig = inspect.signature(train_one_superepoch_SCRUB)
    assert list(sig.parameters) == REFERENCE_PARAMETERS and len(REFERENCE_PARAMETERS) == 26
    defaults = {n: p.default for n, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(kd_T=2.0, sgda_smoothing=0.0, sgda_gamma=0.99, sgda_alpha=0.001, testloader_open=None)
    assert (DISP_FREQ, VER_FREQ) == (5, 100)
    assert ScrubRemainQueue.ORDER == ("losses_kd_remain", "losses_CE", "losses_total_remain") and ScrubForgetQueue.ORDER[::2] == (
        "losses_kd_forget", "losses_total_forget")


def test_the_driver_parses_the_reference_defaults_and_refuses(monkeypatch, capsys):
    import driver_scrub
    a = driver_scrub.get_args([])
    # util/args.py:244-266 of the reference, typed here
    assert (a.sgda_smoothing, a.sgda_gamma, a.sgda_alpha, a.kd_T, a.SCRUB_superepoch, a.scrub_decay_epoch) == (0.0, 0.99, 0.001, 2.0, 10, 100)
    assert all(type(getattr(a, n)) is float for n in ("sgda_smoothing", "sgda_gamma", "sgda_alpha", "kd_T"))
    assert type(a.SCRUB_superepoch) is int and type(a.scrub_decay_epoch) is int and a.opt == "adamw" and a.only_ffn and not a.ffn_open
    cfg = driver_scrub.scrub_cfg(driver_scrub.get_args(["--lr", "0.003", "--scrub_decay_epoch", "7"]), "out")
    assert (cfg["lr_decay_rate"], cfg["lr_decay_epochs"], cfg["sgda_learning_rate"]) == (0.1, 7, 0.003)      # config.py:107-110
    for opt in ("sgd", "adam", "rmsp"):
        with pytest.raises(SystemExit):
            driver_scrub.get_args(["--opt", opt])
        assert "none of those branches matches" in capsys.readouterr().err
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        driver_scrub.main(["--small"])


def test_the_fixture_holds_arrays_only_and_regenerates_to_the_same_bits(golden_dir, tmp_path):
    path = os.path.join(golden_dir, "scrub_small.npz")
    assert os.path.getsize(path) < (1 << 20)
    g = np.load(path, allow_pickle=False)
    assert all(g[k].dtype.kind in "fiuUb" for k in g.files)
    for tag in ("s0", "s1"):
        assert g[f"forget::{tag}"].shape == g[f"forget64::{tag}"].shape == (5, 2) and g[f"remain::{tag}"].shape == g[f"remain64::{tag}"].shape == (10, 3)
        assert sum(k.startswith(f"final::{tag}::") for k in g.files) == len(g["trainable"]) == 9
        for n in g["trainable"].tolist():
            assert g[f"final_diff::{tag}::{n}"].shape == g[f"final::{tag}::{n}"].shape and g[f"final_diff::{tag}::{n}"].dtype == np.float32
    assert g["y_forget"].shape == (3,) and g["y_remain"].shape == (2,)
    # smoothing 0: the max steps' total is -kd; the min steps' total is gamma CE + alpha kd (the fixture is consistent with its own columns)
    lr, wd, kd_T, gamma, alpha, smoothing = g["hyper"].tolist()
    assert np.allclose(g["forget::s0"][:, 1], -g["forget::s0"][:, 0], rtol=1e-6, atol=0)
    assert np.allclose(g["remain::s0"][:, 2], gamma * g["remain::s0"][:, 1] + alpha * g["remain::s0"][:, 0], rtol=1e-6, atol=0)
    assert (g["forget::s1"][1:, 1] > -g["forget::s1"][1:, 0]).all(), "smoothing 0.1 adds a positive distance once the student has moved"
    from oracle.make_golden import REF
    if not os.path.isdir(os.path.join(REF, "vit_pytorch_face")):
        pytest.skip("the reference sources are not on this machine")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_golden_scrub.py"), "--out", str(tmp_path)], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL)
    new = np.load(os.path.join(str(tmp_path), "scrub_small.npz"))
    assert sorted(g.files) == sorted(new.files)
    for k in g.files:
        assert g[k].dtype == new[k].dtype and g[k].shape == new[k].shape and np.array_equal(g[k], new[k]), k
