"""CPU tests of ViTs_face (reference vit_pytorch_face/vits_face.py:414-509): the reference's parameter tree (tests/golden/vits_*.npz hold
its named_parameters order and shapes), a strict load of a state built like the fixtures', the constructor's refusals, the spec handed
to the runner, the gsl_unfold_patches entry point of the library and driver_cl --net."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import recipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def vits_state(cfg, k, seed=1337):      # = tools/make_golden_vits.py
    st = recipe.make_state(cfg, seed=seed)
    fan_in = cfg["channels"] * k * k
    bound = 1.0 / float(np.sqrt(fan_in))
    st["patch_to_embedding.weight"] = np.ascontiguousarray(
        recipe.uniform("patch_to_embedding.weight", (cfg["dim"], fan_in), seed, -bound, bound), dtype=np.float32)
    return st


def make(cfg=None, loss_type="CosFace", k=12, pad=4, **kw):
    from vit_pytorch_face import ViTs_face
    cfg = cfg or recipe.cfg_small2()
    args = dict(loss_type=loss_type, GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                ac_patch_size=k, pad=pad, dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"],
                lora_rank=cfg["lora_rank"])
    args.update(kw)
    return ViTs_face(**args)


@pytest.mark.parametrize("fixture,k,pad,head", [("vits_small2_b3", 12, 4, "CosFace"), ("vits_k10p1_small2_b3", 10, 1, "ArcFace")])
def test_parameter_tree_is_the_references(golden_dir, fixture, k, pad, head):
    g = np.load(os.path.join(golden_dir, fixture + ".npz"))
    m = make(k=k, pad=pad, loss_type=head)
    names = [n for n, _ in m.named_parameters()]
    assert names == list(g["param_names"])
    for (n, p), sh in zip(m.named_parameters(), g["param_shapes"]):
        assert tuple(p.shape) == tuple(int(v) for v in sh[:p.dim()]) and not sh[p.dim():].any(), n
    cfg = recipe.cfg_small2()
    assert m.patch_to_embedding.weight.shape == (cfg["dim"], 3 * k * k)
    # the keys are ViT_face's: only the patch weight's shape differs
    assert set(m.state_dict()) == set(recipe.param_shapes(cfg))


def test_state_loads_strict_and_matches_the_fixture_state(golden_dir):
    cfg = recipe.cfg_small2()
    m = make()
    st = vits_state(cfg, 12)
    res = m.load_state_dict({n: torch.tensor(v) for n, v in st.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m.patch_to_embedding.weight, torch.tensor(st["patch_to_embedding.weight"]))
    with pytest.raises(RuntimeError):
        m.load_state_dict({n: torch.tensor(v) for n, v in recipe.make_state(cfg).items()}, strict=True)      # a [dim, 192] patch weight


def test_constructor_refusals_give_the_reason():
    cfg = recipe.cfg_small2()
    with pytest.raises(NotImplementedError, match="dim_head = 64"):
        make(dim_head=32)
    with pytest.raises(NotImplementedError, match="multiples of 64"):
        make(dim=96)
    with pytest.raises(NotImplementedError, match="multiples of 64"):
        make(mlp_dim=200)
    # k 4, pad 3 at stride 8 on 48 px: 7 x 7 windows, pos_embedding has 36 rows after the cls row
    with pytest.raises(ValueError, match="49 windows.*36 rows"):
        make(k=4, pad=3)
    with pytest.raises(ValueError, match="pad"):
        make(k=8, pad=8)
    with pytest.raises(NotImplementedError, match="SFaceLoss.*6-tuple"):
        make(loss_type="SFace")
    with pytest.raises(AssertionError):
        make(pool="max")
    with pytest.raises(AssertionError):
        make(cfg=dict(cfg, image_size=50))
    # patch_dim is free (432 and 300 are not multiples of 64), fewer windows than rows is allowed (the reference slices pos_embedding)
    assert make(k=12, pad=4).num_tokens == 37 and make(k=10, pad=1).num_tokens == 37
    assert make(k=16, pad=0).num_tokens == 1 + 5 * 5


def test_spec_carries_the_unfold_stage_and_the_vit_face_spec_does_not():
    from vit_pytorch_face import ViT_face
    sp = make(k=10, pad=1, loss_type="ArcFace", pool="mean").hip_spec()
    assert (sp.patch_kernel, sp.patch_stride, sp.patch_pad, sp.image_size, sp.num_tokens) == (10, 8, 1, 48, 37)
    assert (sp.head_kind, sp.pool, sp.lora_site, sp.patch_is_conv) == ("arcface", "mean", "ffn", False)
    cfg = recipe.cfg_small2()
    v = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=48, patch_size=8, dim=128, depth=3, heads=2,
                 mlp_dim=256, lora_rank=8).hip_spec()
    assert (v.patch_kernel, v.patch_stride, v.patch_pad, v.image_size) == (0, 0, 0, None)


def test_package_exports_the_real_class():
    import vit_pytorch_face
    from vit_pytorch_face import vit_face, vits_face
    assert vit_pytorch_face.ViTs_face is vits_face.ViTs_face is vit_face.ViTs_face
    assert "Unfold" in repr(make())


def test_library_exports_the_unfold_entry_point():
    from gslora_hip import _lib
    L = _lib.load()
    assert getattr(L, "gsl_unfold_patches") is not None
    c = ctypes
    assert _lib.SIGNATURES["gsl_unfold_patches"] == [c.c_void_p, c.c_void_p] + [c.c_int] * 9 + [c.c_void_p]
    hdr = open(os.path.join(ROOT, "include", "gslora_hip.h")).read()
    decl = re.search(r"GSL_API int gsl_unfold_patches\(([^)]*)\);", hdr)
    assert decl is not None
    args = [a.strip() for a in decl.group(1).split(",")]
    assert args == ["const float* img", "void* out", "int B", "int C", "int H", "int W", "int k", "int stride", "int pad", "int ldo",
                    "int dtype", "gsl_stream_t s"]


def test_library_refuses_bad_unfold_arguments_before_any_launch():
    """Argument checks run on the host: with null pointers every call returns GSL_ERR_ARG without touching a device."""
    from gslora_hip import _lib
    L = _lib.load()
    f = L.gsl_unfold_patches
    assert f(None, None, 2, 3, 48, 48, 12, 8, 4, 448, _lib.F16, None) == -1
    assert b"argument check failed" in L.gsl_last_error()


def test_unfold_geometry():
    from gslora_hip.ops import unfold_geometry
    assert unfold_geometry(112, 112, 12, 8, 4) == (14, 14)
    assert unfold_geometry(48, 48, 10, 8, 1) == (6, 6)
    assert unfold_geometry(40, 40, 16, 8, 4) == (5, 5)
    assert unfold_geometry(48, 48, 8, 8, 0) == (6, 6)
    x = torch.rand(1, 3, 48, 48)
    assert torch.nn.functional.unfold(x, 10, padding=1, stride=8).shape[-1] == 36


def test_driver_parses_net():
    import driver_cl
    assert driver_cl.get_args([]).net == "VIT"
    assert driver_cl.get_args(["--net", "VITs"]).net == "VITs"
    assert driver_cl.get_args(["-n", "VITs", "--small"]).net == "VITs"
    with pytest.raises(SystemExit):
        driver_cl.get_args(["--net", "VIT_B16"])
