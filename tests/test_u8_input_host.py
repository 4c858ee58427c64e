"""CPU tests of the uint8 image input (ToTensor() + Normalize() fused into the patch gathers): the two entry points in the header, the
version script and the ctypes table; the [C, 256] value table against its defining expression; the opt-in on the model and the driver
flag; the refusals of the library before any launch."""
import ctypes
import os
import re

import pytest
import torch

from oracle import recipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AWKWARD = ((0.1234567, 0.5, 0.9), (0.0371, 1.7, 0.333))


def definition(u, mean, std):
    """The float32 image a uint8 batch stands for: ToTensor() then Normalize(mean, std), in torchvision's operation order."""
    mean, std = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    return u.to(torch.float32).div(255).sub(mean[None, :, None, None]).div(std[None, :, None, None])


def small_vit(**kw):
    from vit_pytorch_face import ViT_face
    cfg = recipe.cfg_small2()
    return ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                    dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], lora_rank=cfg["lora_rank"], **kw)


def test_header_version_script_and_ctypes_table_agree_on_the_u8_entry_points():
    from gslora_hip import _lib
    L = _lib.load()
    c = ctypes
    hdr = open(os.path.join(ROOT, "include", "gslora_hip.h")).read()
    want = {
        "gsl_patchify_u8": (["const uint8_t* img", "int layout", "const float* table", "void* out", "int B", "int C", "int H", "int W", "int p",
                             "int dtype", "gsl_stream_t s"], [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p] + [c.c_int] * 6 + [c.c_void_p]),
        "gsl_unfold_patches_u8": (["const uint8_t* img", "int layout", "const float* table", "void* out", "int B", "int C", "int H", "int W",
                                   "int k", "int stride", "int pad", "int ldo", "int dtype", "gsl_stream_t s"],
                                  [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p] + [c.c_int] * 9 + [c.c_void_p]),
    }
    for name, (args, sig) in want.items():
        assert getattr(L, name) is not None
        assert _lib.SIGNATURES[name] == sig
        decl = re.search(r"GSL_API int " + name + r"\(([^)]*)\);", hdr)
        assert decl is not None, name
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == args
    assert re.search(r"enum gsl_u8_layout \{ GSL_U8_NCHW = 0, GSL_U8_NHWC = 1 \};", hdr)
    assert (_lib.U8_NCHW, _lib.U8_NHWC) == (0, 1)
    assert "train/train_own_forget_cl.py:131-147" in hdr
    assert "gsl_*" in open(os.path.join(ROOT, "gs-lora_amd", "csrc", "exports.map")).read()


@pytest.mark.parametrize("name,pair", [("totensor", ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))),
                                       ("imagenet", ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))), (None, AWKWARD)])
def test_value_table_equals_the_definition_bit_for_bit(name, pair):
    from gslora_hip import ops
    if name is not None:
        assert ops.INPUT_NORMS[name] == pair
    mean, std = pair
    tab = ops.u8_norm_table(mean, std)
    assert tab.shape == (3, 256) and tab.dtype == torch.float32 and tab.is_contiguous()
    # every byte in every channel, in an image-shaped batch (the vectorised path of the CPU kernels) and one pixel at a time
    u = torch.arange(256, dtype=torch.uint8).reshape(1, 1, 16, 16).expand(2, 3, 16, 16).contiguous()
    x = definition(u, mean, std)
    for c in range(3):
        assert torch.equal(tab[c].view(torch.int32), x[0, c].reshape(-1).view(torch.int32)), c
        for b in (0, 1, 127, 128, 254, 255):
            one = definition(torch.full((1, 3, 1, 1), b, dtype=torch.uint8), mean, std)
            assert tab[c, b].item() == one[0, c, 0, 0].item()
    assert torch.equal(ops.u8_reference(u, mean, std), x)
    if name == "totensor":
        assert torch.equal(tab[0], torch.arange(256, dtype=torch.float32) / 255.0)


def test_value_table_refuses_bad_pairs():
    from gslora_hip import ops
    with pytest.raises(ValueError, match="per channel"):
        ops.u8_norm_table((0.0, 0.0), (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="non-zero"):
        ops.u8_norm_table((0.0, 0.0, 0.0), (1.0, 0.0, 1.0))


def test_set_input_norm_is_an_opt_in_on_every_model_family():
    from vit_pytorch_face import ModifiedViT, ViT_face, ViTs_face
    from gslora_hip import ops
    for cls in (ViT_face, ViTs_face, ModifiedViT):
        assert cls.input_norm is None and callable(cls.set_input_norm)
    m = small_vit()
    assert m.input_norm is None
    assert m.set_input_norm() is m and m.input_norm == ops.INPUT_NORM_TOTENSOR
    assert m.set_input_norm("imagenet").input_norm == ops.INPUT_NORM_IMAGENET
    assert m.set_input_norm(*AWKWARD).input_norm == AWKWARD
    assert m.set_input_norm(None).input_norm is None
    with pytest.raises(ValueError, match="unknown name"):
        m.set_input_norm("cifar")
    with pytest.raises(ValueError, match="non-zero"):
        m.set_input_norm((0.0, 0.0, 0.0), (1.0, 1.0, 0.0))
    import copy
    assert copy.deepcopy(m.set_input_norm("imagenet")).input_norm == ops.INPUT_NORM_IMAGENET


def test_step_keeps_bytes_only_for_an_opted_in_model():
    """Host logic of gs_lora_step's input handling: without set_input_norm a uint8 batch is a value cast (the reference's inputs.float());
    with it the bytes go through untouched; float batches are never touched."""
    from gslora_hip.step import _model_input
    m = small_vit()
    u = torch.randint(0, 256, (2, 3, 48, 48), dtype=torch.uint8)
    x = torch.rand(2, 3, 48, 48)
    got = _model_input(m, u)
    assert got.dtype == torch.float32 and torch.equal(got, u.float())
    assert _model_input(m, x) is x
    m.set_input_norm()
    assert _model_input(m, u) is u
    assert _model_input(m, x) is x
    assert _model_input(torch.nn.Linear(2, 2), u).dtype == torch.float32      # any other module: the cast


def test_step_refuses_a_uint8_and_a_float_batch_in_one_step():
    from gslora_hip.step import gs_lora_step
    m = small_vit().set_input_norm()
    u = torch.zeros(2, 3, 48, 48, dtype=torch.uint8)
    y = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="both uint8 or both float"):
        gs_lora_step(m, None, torch.nn.CrossEntropyLoss(), u, y, u.float(), y, beta=0.1, alpha=0.0, BND=1.0)


def test_layout_is_read_from_the_strides():
    from gslora_hip import _lib, ops
    u = torch.randint(0, 256, (2, 3, 8, 8), dtype=torch.uint8)
    assert ops._u8_source(u)[0] == _lib.U8_NCHW
    nhwc = torch.randint(0, 256, (2, 8, 8, 3), dtype=torch.uint8).permute(0, 3, 1, 2)      # a decoder's [B, H, W, C] bytes
    lay, t = ops._u8_source(nhwc)
    assert lay == _lib.U8_NHWC and t is nhwc
    lay, t = ops._u8_source(u.to(memory_format=torch.channels_last))
    assert lay == _lib.U8_NHWC
    lay, t = ops._u8_source(u[:, :, ::2])      # neither: copied to NCHW
    assert lay == _lib.U8_NCHW and t.is_contiguous()


def test_prefetcher_keeps_dtype_and_layout_of_a_host_batch():
    """No device here: the pass-through path hands a uint8 / channels_last batch on as it is."""
    from util.data_prefetcher import data_prefetcher
    u = torch.randint(0, 256, (2, 3, 8, 8), dtype=torch.uint8).to(memory_format=torch.channels_last)
    it = data_prefetcher([(u, torch.zeros(2, dtype=torch.int64))], "cpu", prefetch=True)
    s, _ = it.next()
    assert s.dtype == torch.uint8 and s.is_contiguous(memory_format=torch.channels_last) and torch.equal(s, u)


def test_driver_parses_u8_input_and_builds_the_same_images_as_bytes():
    import driver_cl
    assert driver_cl.get_args([]).u8_input is False
    assert driver_cl.get_args(["--u8_input", "--small", "-n", "VITs"]).u8_input is True
    xf, yf = driver_cl.synthetic_dataset(4, 2, 48, 7)
    xu, yu = driver_cl.synthetic_dataset(4, 2, 48, 7, u8=True)
    assert xu.dtype == torch.uint8 and torch.equal(yf, yu)
    assert torch.equal(definition(xu, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), xf)


def test_library_refuses_bad_u8_arguments_before_any_launch():
    """Argument checks run on the host: with null pointers every call returns GSL_ERR_ARG without touching a device."""
    from gslora_hip import _lib
    L = _lib.load()
    assert L.gsl_patchify_u8(None, 0, None, None, 2, 3, 48, 48, 8, _lib.F16, None) == -1
    assert b"gsl_patchify_u8: argument check failed" in L.gsl_last_error()
    assert L.gsl_unfold_patches_u8(None, 0, None, None, 2, 3, 48, 48, 12, 8, 4, 448, _lib.F16, None) == -1
    assert b"gsl_unfold_patches_u8: argument check failed" in L.gsl_last_error()
    # fake, never dereferenced addresses: every check below fails on the host
    img, tab, out = 0x10000, 0x20000, 0x30000
    assert L.gsl_patchify_u8(img, 2, tab, out, 2, 3, 48, 48, 8, _lib.F16, None) == -1 and b"layout" in L.gsl_last_error()
    assert L.gsl_patchify_u8(img, 0, None, out, 2, 3, 48, 48, 8, _lib.F16, None) == -1 and b"null" in L.gsl_last_error()
    assert L.gsl_patchify_u8(img, 0, tab, out + 4, 2, 3, 48, 48, 8, _lib.F16, None) == -1 and b"aligned" in L.gsl_last_error()
    assert L.gsl_patchify_u8(img, 0, tab, out, 2, 3, 48, 44, 8, _lib.F16, None) == -1
    assert L.gsl_patchify_u8(img, 0, tab, out, 2, 3, 48, 48, 8, 7, None) == -1 and b"bad dtype" in L.gsl_last_error()
    f = L.gsl_unfold_patches_u8
    assert f(img, -1, tab, out, 2, 3, 48, 48, 12, 8, 4, 448, _lib.F16, None) == -1 and b"layout" in L.gsl_last_error()
    assert f(img, 1, None, out, 2, 3, 48, 48, 12, 8, 4, 448, _lib.F16, None) == -1 and b"null" in L.gsl_last_error()
    assert f(img, 1, tab, out + 8, 2, 3, 48, 48, 12, 8, 4, 448, _lib.F16, None) == -1 and b"aligned" in L.gsl_last_error()
    assert f(img + 4, 1, tab, out, 2, 3, 48, 48, 12, 8, 4, 448, _lib.F16, None) == -1 and b"aligned" in L.gsl_last_error()
    assert f(img, 1, tab, out, 2, 3, 48, 48, 12, 8, 12, 448, _lib.F16, None) == -1
    assert f(img, 1, tab, out, 2, 3, 48, 48, 12, 8, 4, 424, _lib.F16, None) == -1
    assert f(img, 1, tab, out, 2, 3, 48, 48, 12, 8, 4, 448, 9, None) == -1 and b"bad dtype" in L.gsl_last_error()


def test_new_kernels_are_in_the_product_library():
    """The spill and barrier checks of tests/test_host_logic.py walk every kernel of the product library: the uint8 gathers must be in it."""
    from gslora_hip import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in (b"patchify_u8_wide_kernel", b"patchify_u8_kernel", b"unfold_patches_u8_kernel"):
        assert name in blob, name
