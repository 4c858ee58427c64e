"""CPU tests of the linear probe (a trainable classifier head, reference train/backbone_forget_main.py:596-600, 657-670): the optimizer's
param groups, the C ABI of gsl_head_wgrad, the refusals that need no device, and the fixtures of tools/make_golden_head_probe.py, which
regenerate to the same bits where the reference sources are present."""
import math
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import recipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("head_probe_small2_cosface_b3", "head_probe_small2_arcface_b3", "head_probe_small2_softmax_b3", "head_probe_small6_engine",
            "head_open_small2_b3")
ARGS = SimpleNamespace(opt="adamw", lr=1e-2, weight_decay=0.05, opt_eps=1e-8, opt_betas=None)


def make(loss_type="CosFace", cfg=None, **kw):
    from vit_pytorch_face import ViT_face
    cfg = cfg or recipe.cfg_small2()
    return ViT_face(loss_type=loss_type, GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"],
                    patch_size=cfg["patch_size"], dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"],
                    lora_rank=cfg["lora_rank"], **kw)


def only_head(m):      # backbone_forget_main.py:596-600
    for n, p in m.named_parameters():
        p.requires_grad = "loss" in n
    return m


def groups_of(m):
    from gslora_hip.optim import create_optimizer
    names = {id(p): n for n, p in m.named_parameters()}
    return [([names[id(p)] for p in g["params"]], g["weight_decay"]) for g in create_optimizer(ARGS, m).param_groups]


def test_lora_only_model_gets_exactly_todays_groups():
    import loralib as lora
    m = make()
    lora.mark_only_lora_as_trainable(m)
    lora_names = [n for n, _ in m.named_parameters() if "lora_" in n]
    assert groups_of(m) == [(lora_names, 0.05)]      # one decay group, the LoRA tensors in named_parameters order: as before this feature


@pytest.mark.parametrize("loss_type", ["CosFace", "ArcFace", "Softmax"])
def test_head_parameters_get_groups_of_their_own(loss_type):
    m = only_head(make(loss_type))
    want = [(["loss.bias"], 0.0)] if loss_type == "Softmax" else []
    assert groups_of(m) == want + [(["loss.weight"], 0.05)]      # timm's rule: decay on the weight, none on a bias
    for n, p in m.named_parameters():      # LoRA and the head (the baselines' --ffn_open)
        p.requires_grad = "lora_" in n or "loss" in n
    lora_names = [n for n, _ in m.named_parameters() if "lora_" in n]
    # the LoRA group first and whole (one contiguous range of the flat bucket), the head's groups behind it
    assert groups_of(m) == [(lora_names, 0.05)] + want + [(["loss.weight"], 0.05)]


def test_vits_face_shares_the_head_names_and_modified_vit_has_none():
    from vit_pytorch_face import ModifiedViT, ViT_face, ViTs_face
    assert ViT_face.trainable_head == ViTs_face.trainable_head == ("loss.weight", "loss.bias")
    assert ModifiedViT.trainable_head == ()


def test_header_prototype_signature_and_export():
    from gslora_hip import _lib
    header = open(os.path.join(ROOT, "include", "gslora_hip.h")).read()
    declared = set(re.findall(r"\b(gsl_[a-z0-9_]+)\s*\(", header)) - {"gsl_dropout_keep"}
    assert "gsl_head_wgrad" in declared and declared == set(_lib.SIGNATURES) and len(_lib.SIGNATURES) == 59
    proto = re.search(r"GSL_API int gsl_head_wgrad\(([^;]*)\);", header).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES["gsl_head_wgrad"]) == 15
    comment = header[:header.index("GSL_API int gsl_head_wgrad")]
    for lines in ("backbone_forget_main.py:596-600", ":657-670", "vit_face.py:181-207"):
        assert lines in comment, "the header comment names the reference lines"
    for doc in ("README.md", "DESIGN.md"):
        assert "55" in open(os.path.join(ROOT, doc)).read()
    lib = _lib.load()
    assert hasattr(lib, "gsl_head_wgrad")
    so = os.path.join(ROOT, "gs-lora_amd", "gslora_hip", "libgslora_hip.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    assert {ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln} == set(_lib.SIGNATURES)


def test_entry_point_checks_its_arguments_before_any_launch():
    from gslora_hip import _lib
    L = _lib.load()
    p = 16      # a non-null address that is never dereferenced: the argument check fails first
    call = lambda **kw: L.gsl_head_wgrad(*[{**dict(dl=p, emb=p, W=p, label=p, cos_y=p, dW=p, db=None, B=4, C=10, D=64, kind=0, s=64.0, m=0.5,
                                                  easy=0, stream=None), **kw}[k]
                                          for k in ("dl", "emb", "W", "label", "cos_y", "dW", "db", "B", "C", "D", "kind", "s", "m", "easy", "stream")])
    for bad in (dict(kind=3), dict(B=0), dict(C=0), dict(D=1025), dict(D=0), dict(dW=None), dict(kind=1, label=None), dict(kind=1, cos_y=None),
                dict(kind=0, db=p), dict(kind=1, db=p), dict(kind=0, W=None)):
        assert call(**bad) == -1 and b"gsl_head_wgrad" in L.gsl_last_error(), bad


def test_cpu_tensors_raise_the_no_cpu_fallback_error():
    from gslora_hip import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.head_wgrad(torch.zeros(2, 5), torch.zeros(2, 64), torch.zeros(5, 64), "cosface")
    cfg = recipe.cfg_small2()
    m = only_head(make())      # a trainable head passes the trainability check; the CPU input is what is refused
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 3, cfg["image_size"], cfg["image_size"]), torch.zeros(2, dtype=torch.long))


def test_any_other_trainable_parameter_still_raises():
    import loralib as lora
    cfg = recipe.cfg_small2()
    x, y = torch.zeros(2, 3, cfg["image_size"], cfg["image_size"]), torch.zeros(2, dtype=torch.long)
    m = make()
    lora.mark_only_lora_as_trainable(m)
    m.pos_embedding.requires_grad = True
    with pytest.raises(RuntimeError, match=r"'pos_embedding' requires a gradient.*LoRA parameters and the classifier head \(loss.weight, loss.bias\) only"):
        m(x, y)
    with torch.no_grad():      # ... and under no_grad the check does not apply: the CPU refusal is reached
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(x, y)


def test_modified_vit_head_stays_frozen_and_says_why():
    import loralib as lora
    from vit_pytorch_face import ModifiedViT
    from vit_pytorch_face.modified_VIT import vit_b_16
    m = ModifiedViT(vit_b_16(image_size=64, num_layers=1, num_heads=1, hidden_dim=64, mlp_dim=128, num_classes=10))
    lora.mark_only_lora_as_trainable(m)
    m.heads.head.weight.requires_grad = True
    with pytest.raises(RuntimeError, match=r"'heads.head.weight' requires a gradient.*LoRA parameters only.*reference freezes it for imagenet100"):
        m(torch.zeros(2, 3, 64, 64))


def test_graphed_step_and_probe_step_refusals():
    from gslora_hip import step
    from gslora_hip.optim import create_optimizer
    m = only_head(make())
    gs = step.GraphedStep(m, create_optimizer(ARGS, m), torch.nn.CrossEntropyLoss())
    z = torch.zeros(1)
    with pytest.raises(RuntimeError, match="GraphedStep captures the LoRA-only step.*trainable classifier head"):
        gs(z, z, z, z, beta=0.1, alpha=0.0, BND=1.0)
    assert step._head_trains(m) and not step._head_trains(torch.nn.Linear(2, 2))


def test_graphed_step_leaves_other_trainable_tensors_to_the_models_own_refusal():
    import loralib as lora
    from gslora_hip import step
    from gslora_hip.optim import create_optimizer
    m = make()
    lora.mark_only_lora_as_trainable(m)
    m.pos_embedding.requires_grad = True
    gs = step.GraphedStep(m, create_optimizer(ARGS, m), torch.nn.CrossEntropyLoss())
    cfg = recipe.cfg_small2()
    x, y = torch.zeros(2, 3, cfg["image_size"], cfg["image_size"]), torch.zeros(2, dtype=torch.long)
    with pytest.raises(RuntimeError, match="'pos_embedding' requires a gradient") as e:
        gs(x, y, x, y, beta=0.1, alpha=0.0, BND=1.0)
    assert "GraphedStep" not in str(e.value)


def test_a_process_group_refuses_the_trainable_head_before_any_launch(monkeypatch):
    from gslora_hip import step
    from gslora_hip.optim import create_optimizer
    m = only_head(make())
    opt, crit, z = create_optimizer(ARGS, m), torch.nn.CrossEntropyLoss(), torch.zeros(1)
    monkeypatch.setattr(step, "_world", lambda: 2)
    with pytest.raises(RuntimeError, match="head_probe_step runs in one process.*2 ranks"):
        step.head_probe_step(m, opt, crit, z, z)
    with pytest.raises(RuntimeError, match="data-parallel gs_lora_step all-reduces the flat LoRA gradient bucket only.*trainable classifier head"):
        step.gs_lora_step(m, opt, crit, z, z, z, z, beta=0.1, alpha=0.0, BND=1.0)


def test_driver_flag_and_probe_trainability_rule():
    import driver_cl
    import driver_probe
    assert driver_cl.get_args([]).probe_epochs == 0 and driver_cl.get_args(["--probe_epochs", "3"]).probe_epochs == 3
    m = make("Softmax")
    assert driver_probe.mark_only_head_as_trainable(m) == ["loss.weight", "loss.bias"]
    assert [n for n, p in m.named_parameters() if p.requires_grad] == ["loss.weight", "loss.bias"]
    assert driver_probe.ProbeMeterQueue.ORDER == ("losses", "top1")


def test_fixtures_hold_arrays_only_and_the_arcface_case_straddles_the_threshold(golden_dir):
    for tag in FIXTURES:
        path = os.path.join(golden_dir, f"{tag}.npz")
        assert os.path.getsize(path) < (1 << 20)
        g = np.load(path, allow_pickle=False)      # raises on an object array
        assert all(g[k].dtype.kind in "fiuU" for k in g.files), tag
    g = np.load(os.path.join(golden_dir, "head_probe_small2_arcface_b3.npz"))
    th, c = math.cos(math.pi - 0.5), g["cos_y"]
    assert (c > th).any() and (c < th).any() and (np.abs(c - th) > 1e-3).all()      # both branches of phi, none on the edge
    assert (c > 1e-3).any() and (c < -1e-3).any()                                    # ... and of the easy_margin variant
    assert {"easy_logits", "easy_loss", "easy_prec1", "easy_grad::loss.weight", "state::loss.weight"} <= set(g.files)
    g = np.load(os.path.join(golden_dir, "head_probe_small2_softmax_b3.npz"))
    assert "grad::loss.bias" in g.files and np.abs(g["grad::loss.bias"]).max() > 0
    g = np.load(os.path.join(golden_dir, "head_open_small2_b3.npz"))
    assert "grad1::loss.weight" in g.files and sum("lora_" in k for k in g.files) == 12


def test_fixtures_regenerate_to_the_same_bits(golden_dir, tmp_path):
    from oracle.make_golden import REF
    if not os.path.isdir(os.path.join(REF, "vit_pytorch_face")):
        pytest.skip("the reference sources are not on this machine")
    # a child process: the generator installs import shims and patches torch for the reference's sake
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_golden_head_probe.py"), "--out", str(tmp_path)],
                          stdout=subprocess.DEVNULL)
    for tag in FIXTURES:
        old, new = np.load(os.path.join(golden_dir, f"{tag}.npz")), np.load(os.path.join(str(tmp_path), f"{tag}.npz"))
        assert sorted(old.files) == sorted(new.files), tag
        for k in old.files:
            assert old[k].dtype == new[k].dtype and old[k].shape == new[k].shape, (tag, k)
            assert old[k].tobytes() == new[k].tobytes(), (tag, k)
