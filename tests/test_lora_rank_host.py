"""LoRA ranks above 16, the parts that need no GPU: what the models refuse at construction, the workspace sizes of the rank-32 / rank-64
reductions, the U-column rule in the header and in INTEGRATION.md, and the fixtures of tools/make_golden_lora_rank.py."""
import os

import numpy as np
import pytest

from oracle import recipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def vit_face(cfg, **kw):
    from vit_pytorch_face import ViT_face
    return ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                    dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], lora_rank=cfg["lora_rank"],
                    lora_pos=cfg.get("lora_pos", "FFN"), **kw)


def test_rank_65_is_refused_at_construction_by_every_family():
    from util.utils import replace_ffn_with_lora
    from vit_pytorch_face import ModifiedViT, ViTs_face
    from vit_pytorch_face.modified_VIT import vit_b_16
    cfg = recipe.cfg_small2(lora_rank=65)
    with pytest.raises(NotImplementedError, match=r"lora_rank 65 exceeds 64.*LoRA K segment"):
        vit_face(cfg)
    with pytest.raises(NotImplementedError, match=r"lora_rank 65 exceeds 64.*LoRA K segment"):
        ViTs_face(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                  ac_patch_size=12, pad=4, dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], lora_rank=65)
    c = recipe.cfg_vitb_small2()
    vit = vit_b_16(image_size=c["image_size"], patch_size=c["patch_size"], num_layers=c["depth"], num_heads=c["heads"],
                   hidden_dim=c["dim"], mlp_dim=c["mlp_dim"], num_classes=c["num_class"])
    with pytest.raises(NotImplementedError, match=r"lora_rank 65 exceeds 64.*LoRA K segment"):
        replace_ffn_with_lora(ModifiedViT(vit), rank=65).hip_spec()


def test_rank_64_and_attention_rank_21_construct():
    assert vit_face(recipe.cfg_small2(lora_rank=64)).lora_rank == 64
    assert vit_face(recipe.cfg_small_attn(lora_rank=21)).lora_rank == 21


def test_attention_site_rank_22_is_refused_at_construction():
    with pytest.raises(NotImplementedError, match=r"3 \* lora_rank = 66 must not exceed 64.*LoRA K segment"):
        vit_face(recipe.cfg_small_attn(lora_rank=22))
    assert vit_face(recipe.cfg_small2(lora_rank=22)).lora_rank == 22      # the FFN site holds it


def test_pack_geometry_takes_the_rank_from_the_lora_tensor_not_from_its_smaller_side():
    """lora_A is [r, in] and lora_B [out, r]: at r = 64 on a 64-wide model both sides are equal, and the pack is [64, in] / [out, 64]."""
    from gslora_hip.vit_runner import PADK, ViTRunner
    g = ViTRunner.PACK_GEOM
    r, K, N = 64, 64, 128
    assert g["A_rows"](r, K, r) == (K, 1, r, K, PADK, K) and g["AT_cols"](r, K, r) == (1, K, K, r, K, PADK)
    assert g["B_cols"](N, r, r) == (r, 1, N, r, N, PADK) and g["BT_rows"](N, r, r) == (1, r, r, N, PADK, N)
    assert PADK == 64


def test_workspace_grows_with_the_padded_rank():
    from gslora_hip import _lib as L
    from gslora_hip.ops import _LgradDesc
    lib = L.load()
    for M, N in ((700, 768), (333, 136), (201728, 2048)):
        w = {r: lib.gsl_lora_grad_ws_elems(M, N, r) for r in (8, 16, 17, 32, 33, 64)}
        assert 0 < w[8] < w[16] < w[32] < w[64] and w[17] == w[32] and w[33] == w[64], w
    def batch(r):
        d = (_LgradDesc * 1)(_LgradDesc(16, 768, 16, 64, 700, 768, r, 1, 0, 16, r, 1))
        return lib.gsl_lora_grad_batch_ws_elems(d, 1)
    assert batch(16) > 0 and batch(32) == 2 * batch(16) and batch(64) == 4 * batch(16)
    assert batch(65) == -1 and batch(0) == -1
    assert "r in [1,64]" in lib.gsl_last_error().decode()


def test_the_u_column_rule_is_written_down():
    hdr = open(os.path.join(ROOT, "include", "gslora_hip.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for text in (hdr, integ):
        assert "8 * ceil(r / 8)" in text and "[0, r)" in text


FIXTURE_KEYS = {
    "rank32_small2_b3": ("arcface_small2_b3", ()),
    "rank64_small2_b3": ("arcface_small2_b3", ("grad_inactive::",)),
    "rank20_attn_small_b3": ("arcface_attn_small_b3", ()),
    "rank48_vitb_small2_b3": ("vitb_small2_b3", ()),
    "rank32_small6_engine": ("arcface_small6_engine", ("param1::", "param3::")),
}


@pytest.mark.parametrize("tag", list(FIXTURE_KEYS))
def test_fixture_keys_and_size(golden_dir, tag):
    """The keys of the rank-8 sibling (less the families the tool drops to stay below 1 MB), finite arrays, LoRA shapes of the rank."""
    sibling, dropped = FIXTURE_KEYS[tag]
    path = os.path.join(golden_dir, f"{tag}.npz")
    assert os.path.getsize(path) < 1_000_000
    g, s = np.load(path), np.load(os.path.join(golden_dir, f"{sibling}.npz"))
    want = {k for k in s.files if not k.startswith(dropped)} if dropped else set(s.files)
    assert set(g.files) == want, sorted(set(g.files) ^ want)
    rank = int(tag[4:6])
    for k in g.files:
        if g[k].dtype.kind == "f":
            assert np.isfinite(g[k]).all(), k
        if k.startswith("grad1::") and k.endswith("lora_A"):
            assert g[k].shape[0] == (3 * rank if "attn" in tag else rank), (k, g[k].shape)
