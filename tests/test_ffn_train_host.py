"""CPU tests of FFN-weight training: the second product library's ABI (header, bindings and exported symbols agree; the first library's ABI is
what it was), no spilled register in its kernels, the trainability rule and its refusals, the optimizer grouping, the fixtures and their
generator. The arithmetic is tested on the GPU (tests/test_hip_wgrad_edges.py, test_hip_reg_quad.py, test_hip_ffn_train.py)."""
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import recipe
from product_libs import exported, kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("ffn_train_small2_b3", "ffn_l2_small_engine")
ARGS = SimpleNamespace(opt="adamw", lr=1e-2, weight_decay=0.05, opt_eps=1e-8, opt_betas=None)


def make(lora_rank=0, cls=None, **kw):
    from vit_pytorch_face import ViT_face
    cfg = recipe.cfg_small2(lora_rank=lora_rank)
    return (cls or ViT_face)(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                             dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], lora_rank=lora_rank, **kw)


def only_ffn(m, head=True):
    for n, p in m.named_parameters():
        p.requires_grad = "fn.fn.net" in n or (head and "loss" in n)
    return m


def inputs():
    cfg = recipe.cfg_small2()
    return torch.zeros(2, 3, cfg["image_size"], cfg["image_size"]), torch.zeros(2, dtype=torch.long)


def test_header_bindings_and_exports_of_the_second_library_agree():
    from gslora_hip import _lib_train, build
    header = open(os.path.join(ROOT, "include", "gslora_train.h")).read()
    declared = set(re.findall(r"\b(gst_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib_train.SIGNATURES) == exported(build.side_out("train"))
    assert {"gst_wgrad", "gst_wgrad_plan", "gst_wgrad_ws_elems", "gst_reg_quad_fwd", "gst_reg_quad_bwd"} <= declared
    for name, argtypes in _lib_train.SIGNATURES.items():
        proto = re.search(r"GSL_API [a-z *]+\b" + name + r"\(([^;]*)\);", header).group(1)
        n = 0 if proto.strip() in ("", "void") else len(proto.split(","))
        assert n == len(argtypes), name
    for lines in ("train_own_forget_cl.py:432-439", "vit_face.py:330-333", "engine_cl.py:455-457"):
        assert lines in header, "the header comment names the reference lines"


def test_the_first_library_keeps_its_abi():
    from gslora_hip import _lib, build
    header = open(os.path.join(ROOT, "include", "gslora_hip.h")).read()
    declared = set(re.findall(r"\b(gsl_[a-z0-9_]+)\s*\(", header)) - {"gsl_dropout_keep"}
    assert declared == set(_lib.SIGNATURES) == exported(build.OUT) and len(declared) == 59      # (57 + the two LoRA-gradient plan queries)
    assert not any(n.startswith("gst_") for n in exported(build.OUT)) and not any(n.startswith("gsl_") for n in exported(build.side_out("train")))


def test_the_second_library_is_opened_lazily():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import gslora_hip._lib_train as t, gslora_hip.step, gslora_hip.vit_runner, vit_pytorch_face, engine_cl\n"
            "assert not t.loaded()\n"
            "assert 'libgslora_train' not in open('/proc/self/maps').read()\n"
            "t.load(); assert t.loaded() and 'libgslora_train' in open('/proc/self/maps').read()\n" % (ROOT, os.path.join(ROOT, "gs-lora_amd")))
    subprocess.check_call([sys.executable, "-c", code])


def test_no_kernel_of_the_second_library_spills_registers():
    """Read from the code-object notes (product_libs.kernel_notes): every gfx950 kernel of libgslora_train.so declares .vgpr_spill_count 0
    and no private segment; every kernel is bound by __launch_bounds__ (a .max_flat_workgroup_size of 256, not the default 1024)."""
    from gslora_hip import build as B
    notes = kernel_notes(B.side_out("train"))
    kernels, bad = [k[0] for k in notes], [k for k in notes if k[1] or k[2] or k[3] != 256]
    assert len(kernels) == 7 and sum("wgrad_partial" in k for k in kernels) == 3, kernels      # three formats of the GEMM, its reduce, three of the regulariser
    assert not bad, bad


def test_ffn_names_train_only_without_lora():
    import loralib as lora
    x, y = inputs()
    m = only_ffn(make(0))
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    assert len(names) == 13 and names[-1] == "loss.weight" and all(re.fullmatch(r"transformer\.layers\.\d\.1\.fn\.fn\.net\.[03]\.(weight|bias)", n) for n in names[:-1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # the trainability check passes; the CPU input is what is refused
        m(x, y)
    m = make(8)
    lora.mark_only_lora_as_trainable(m)
    m.transformer.layers[1][1].fn.fn.net[3].bias.requires_grad = True
    with pytest.raises(RuntimeError, match=r"'transformer.layers.1.1.fn.fn.net.3.bias' requires a gradient.*holds LoRA adapters \(lora_rank = 8\).*lora_rank = 0"):
        m(x, y)
    m = only_ffn(make(0))
    m.transformer.layers[0][0].fn.fn.to_out[0].weight.requires_grad = True      # any other weight of the backbone is still refused
    with pytest.raises(RuntimeError, match=r"to_out.0.weight' requires a gradient.*classifier head \(loss.weight, loss.bias\) only.*fn.fn.net"):
        m(x, y)


def test_vits_face_shares_the_rule_and_modified_vit_keeps_refusing():
    import loralib as lora
    from vit_pytorch_face import ModifiedViT, ViT_face, ViTs_face
    from vit_pytorch_face.modified_VIT import vit_b_16
    assert ViT_face.trainable_ffn == ViTs_face.trainable_ffn == "fn.fn.net" and ModifiedViT.trainable_ffn == ""
    m = ModifiedViT(vit_b_16(image_size=64, num_layers=1, num_heads=1, hidden_dim=64, mlp_dim=128, num_classes=10))
    lora.mark_only_lora_as_trainable(m)
    name, p = next((n, p) for n, p in m.named_parameters() if "mlp" in n and n.endswith(".weight") and "lora_" not in n)
    p.requires_grad = True
    with pytest.raises(RuntimeError, match=re.escape(repr(name)) + r" requires a gradient.*LoRA parameters only"):
        m(torch.zeros(2, 3, 64, 64))


def test_process_group_and_graphed_step_refuse_trainable_ffn_weights(monkeypatch):
    from gslora_hip import step
    from gslora_hip.optim import create_optimizer
    import loralib as lora
    m, lora_model = only_ffn(make(0), head=False), make(8)
    lora.mark_only_lora_as_trainable(lora_model)
    assert step._ffn_trains(m) and not step._ffn_trains(lora_model) and not step._ffn_trains(torch.nn.Linear(2, 2))
    opt, crit, z = create_optimizer(ARGS, m), torch.nn.CrossEntropyLoss(), torch.zeros(1)
    gs = step.GraphedStep(m, opt, crit)
    with pytest.raises(RuntimeError, match="GraphedStep captures the LoRA-only step.*trainable FFN weights"):
        gs(z, z, z, z, beta=0.1, alpha=0.0, BND=1.0)
    monkeypatch.setattr(step, "_world", lambda: 2)
    with pytest.raises(RuntimeError, match="ffn_reg_step runs in one process.*2 ranks"):
        step.ffn_reg_step(m, opt, crit, z, z)
    with pytest.raises(RuntimeError, match="data-parallel gs_lora_step all-reduces the flat LoRA gradient bucket only.*trainable FFN weights"):
        step.gs_lora_step(m, opt, crit, z, z, z, z, beta=0.1, alpha=0.0, BND=1.0)


def test_optimizer_groups_ffn_biases_without_decay_weights_with_and_the_head_behind():
    from gslora_hip.optim import create_optimizer
    m = only_ffn(make(0))
    names = {id(p): n for n, p in m.named_parameters()}
    groups = [([names[id(p)] for p in g["params"]], g["weight_decay"]) for g in create_optimizer(ARGS, m).param_groups]
    ffn = [n for n in names.values() if "fn.fn.net" in n]
    assert groups == [([n for n in ffn if n.endswith(".bias")], 0.0), ([n for n in ffn if n.endswith(".weight")], 0.05), (["loss.weight"], 0.05)]
    assert len(groups[0][0]) == len(groups[1][0]) == 6


def test_get_reg_loss_without_terms_is_a_zero_and_the_epoch_stub_stays():
    import engine_cl
    z = engine_cl.get_reg_loss(make(0), None, 1.0, torch.device("cpu"))
    assert z.dim() == 0 and z.item() == 0.0
    with pytest.raises(NotImplementedError):
        engine_cl.train_one_epoch_regularzation()


def test_fixtures_hold_arrays_only(golden_dir):
    for tag in FIXTURES:
        path = os.path.join(golden_dir, f"{tag}.npz")
        assert os.path.getsize(path) < (1 << 20)
        g = np.load(path, allow_pickle=False)
        assert all(g[k].dtype.kind in "fiuU" for k in g.files), tag
    g = np.load(os.path.join(golden_dir, "ffn_train_small2_b3.npz"))
    grads = [k for k in g.files if k.startswith("grad::")]
    assert len(grads) == 13 and sum("fn.fn.net" in k for k in grads) == 12 and all(np.abs(g[k]).max() > 0 for k in grads)
    g = np.load(os.path.join(golden_dir, "ffn_l2_small_engine.npz"))
    assert g["losses"].shape == (3, 3) and g["losses"][0][1] == 0.0      # step 1: the weights are the task's, the term is exactly zero
    assert all(0.2 < reg / ce < 5.0 for ce, reg, _ in g["losses"][1:])      # ... then about as large as the cross-entropy
    assert sum(k.startswith("final::") for k in g.files) == len(g["trainable"]) == 9


def test_fixtures_regenerate_to_the_same_bits(golden_dir, tmp_path):
    from oracle.make_golden import REF
    if not os.path.isdir(os.path.join(REF, "vit_pytorch_face")):
        pytest.skip("the reference sources are not on this machine")
    # a child process: the generator installs import shims and patches torch for the reference's sake
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_golden_ffn_train.py"), "--out", str(tmp_path)], stdout=subprocess.DEVNULL)
    for tag in FIXTURES:
        old, new = np.load(os.path.join(golden_dir, f"{tag}.npz")), np.load(os.path.join(str(tmp_path), f"{tag}.npz"))
        assert sorted(old.files) == sorted(new.files), tag
        for k in old.files:
            assert old[k].dtype == new[k].dtype and old[k].shape == new[k].shape and np.array_equal(old[k], new[k]), (tag, k)
