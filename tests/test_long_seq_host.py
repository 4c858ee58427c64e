"""CPU tests of the long-sequence bound (GSL_ATTN_MAX_T = 1025 tokens): the constructors refuse a geometry above it and name it, accept
one at it, and the attention entry points refuse a longer sequence in their argument check, before any launch."""
import pytest

from oracle import recipe


def vit_face(image_size, patch_size=8):
    from vit_pytorch_face import ViT_face
    c = recipe.cfg_small2()
    return ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=c["num_class"], image_size=image_size, patch_size=patch_size, dim=c["dim"],
                    depth=1, heads=c["heads"], mlp_dim=c["mlp_dim"], lora_rank=c["lora_rank"])


def test_vit_face_refuses_more_than_1025_tokens():
    assert vit_face(256).num_tokens == 1025      # 32 x 32 patches + cls: the bound itself
    assert vit_face(128).num_tokens == 257
    with pytest.raises(NotImplementedError, match=r"ViT_face: this geometry gives 1090 tokens.*at most 1025"):
        vit_face(264)      # 33 x 33 patches


def test_vits_face_refuses_more_than_1025_tokens():
    from vit_pytorch_face import ViTs_face
    c = recipe.cfg_small2()
    kw = dict(loss_type="CosFace", GPU_ID=[0], num_class=c["num_class"], dim=c["dim"], depth=1, heads=c["heads"], mlp_dim=c["mlp_dim"])
    assert ViTs_face(image_size=128, patch_size=8, ac_patch_size=12, pad=4, **kw).num_tokens == 257
    with pytest.raises(NotImplementedError, match=r"ViTs_face: this geometry gives 1090 tokens.*at most 1025"):
        ViTs_face(image_size=132, patch_size=4, ac_patch_size=4, pad=0, **kw)      # 33 x 33 windows


def test_modified_vit_refuses_more_than_1025_tokens():
    from vit_pytorch_face import ModifiedViT
    from vit_pytorch_face.modified_VIT import vit_b_16
    small = dict(num_layers=1, num_heads=1, hidden_dim=64, mlp_dim=128, num_classes=10)
    assert ModifiedViT(vit_b_16(image_size=512, **small)).hip_spec().num_tokens == 1025
    with pytest.raises(NotImplementedError, match=r"ModifiedViT: this geometry gives 1090 tokens.*at most 1025"):
        ModifiedViT(vit_b_16(image_size=528, **small))


def test_attention_entry_points_refuse_more_than_1025_tokens_before_any_launch():
    from gslora_hip import _lib
    from gslora_hip import ops
    assert ops.ATTN_MAX_T == 1025
    L = _lib.load()
    p = 16      # a non-null address that is never dereferenced: the argument check fails first
    for dt in (_lib.F32, _lib.BF16, _lib.F16):
        assert L.gsl_attention_fwd(p, p, p, 1, 1026, 1, 0.125, dt, 0, None) == -1
        assert b"T <= 1025" in L.gsl_last_error()
        assert L.gsl_attention_bwd(p, p, p, p, p, p, 1, 1026, 1, 0.125, dt, 0, None) == -1
        assert b"T <= 1025" in L.gsl_last_error()
        assert L.gsl_attention_fwd_cls(p, p, p, p, 1, 1026, 1, 0.125, dt, 0, None) == -1
        assert b"T <= 1025" in L.gsl_last_error()
