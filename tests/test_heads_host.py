"""CPU tests of the ArcFace / Softmax heads of ViT_face (reference vit_pytorch_face/vit_face.py:14-143, 503-521): construction,
the reference's parameter names and shapes (tests/golden/{arcface,softmax}_small2_b3.npz hold its named_parameters order), the ArcFace
constants, the model spec handed to the runner, SFace's refusal, the margin entry points of the library and driver_cl --head."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import recipe


def make(loss_type, cfg=None, **kw):
    from vit_pytorch_face import ViT_face
    cfg = cfg or recipe.cfg_small2()
    return ViT_face(loss_type=loss_type, GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"],
                    patch_size=cfg["patch_size"], dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"],
                    lora_rank=cfg["lora_rank"], **kw)


@pytest.mark.parametrize("loss_type,fixture", [("ArcFace", "arcface_small2_b3"), ("Softmax", "softmax_small2_b3")])
def test_heads_construct_with_the_reference_parameter_tree(golden_dir, loss_type, fixture):
    m = make(loss_type)
    names = [n for n, _ in m.named_parameters()]
    assert names == list(np.load(os.path.join(golden_dir, fixture + ".npz"))["param_names"])
    cfg = recipe.cfg_small2()
    shapes = dict(recipe.param_shapes(cfg))
    if loss_type == "Softmax":
        shapes["loss.bias"] = (cfg["num_class"],)
    assert {n: tuple(p.shape) for n, p in m.named_parameters()} == {n: tuple(s) for n, s in shapes.items()}
    assert m.loss.weight.shape == (cfg["num_class"], cfg["dim"])
    if loss_type == "Softmax":
        assert (m.loss.bias == 0).all()      # nn.init.zeros_ (reference :32)


def test_arcface_constants_and_defaults():
    from vit_pytorch_face import ArcFace
    h = ArcFace(in_features=64, out_features=10, device_id=[0])
    assert (h.s, h.m, h.easy_margin) == (64.0, 0.5, False)
    assert h.cos_m == math.cos(0.5) and h.sin_m == math.sin(0.5)
    assert h.th == math.cos(math.pi - 0.5) and h.mm == math.sin(math.pi - 0.5) * 0.5
    h2 = ArcFace(64, 10, None, s=30.0, m=0.3, easy_margin=True)
    assert (h2.s, h2.m, h2.easy_margin, h2.cos_m, h2.th) == (30.0, 0.3, True, math.cos(0.3), math.cos(math.pi - 0.3))
    with pytest.raises(RuntimeError):
        h(torch.zeros(1, 64), torch.zeros(1, dtype=torch.long))      # the arithmetic lives in the fused HIP head


def test_model_spec_takes_the_head_and_a_user_set_margin():
    m = make("ArcFace")
    sp = m.hip_spec()
    assert (sp.head_kind, sp.cos_s, sp.cos_m, sp.easy_margin, sp.head_b) == ("arcface", 64.0, 0.5, False, None)
    assert sp.head_w is m.loss.weight
    m.loss.s, m.loss.m, m.loss.easy_margin = 32.0, 0.3, True
    sp = m.hip_spec()
    assert (sp.cos_s, sp.cos_m, sp.easy_margin) == (32.0, 0.3, True)
    s = make("Softmax").hip_spec()
    assert s.head_kind == "softmax" and s.head_b is not None and s.head_b.shape == (12,)
    c = make("CosFace", pool="mean").hip_spec()
    assert (c.head_kind, c.cos_s, c.cos_m, c.easy_margin, c.pool) == ("cosface", 64.0, 0.35, False, "mean")


def test_sface_is_refused_with_the_reason():
    with pytest.raises(NotImplementedError, match="SFaceLoss.*6-tuple"):
        make("SFace")
    with pytest.raises(NotImplementedError):
        make("NoSuchHead")


def test_library_exports_the_margin_entry_points():
    from gslora_hip import _lib
    L = _lib.load()
    for name in ("gsl_head_fwd_margin", "gsl_head_bwd_margin"):
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gslora_hip.h")).read()
    assert "gsl_head_fwd_margin(" in hdr and "gsl_head_bwd_margin(" in hdr


def test_driver_parses_head():
    import driver_cl
    assert driver_cl.get_args([]).head == "CosFace"
    for h in ("CosFace", "ArcFace", "Softmax"):
        assert driver_cl.get_args(["--head", h]).head == h
    with pytest.raises(SystemExit):
        driver_cl.get_args(["--head", "SFaceLoss"])
