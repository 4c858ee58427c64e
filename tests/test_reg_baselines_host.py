"""CPU tests of the regularisation baselines (L2 / EWC / MAS): the third product library's ABI (header, bindings and exported symbols agree),
lazy loading, no spilled register in its kernels, the host-side layout of the batched
regulariser against the partition rule of gst_reg_quad_fwd, the epoch loop's signature, the fixtures and the driver's refusal without a GPU.
The arithmetic is tested on the GPU (tests/test_hip_reg_kernels.py, tests/test_hip_reg_baselines.py)."""
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
FIXTURES = ("importance_small", "reg_epoch_small_engine")
REFERENCE_PARAMETERS = ["model", "criterion", "data_loader_cl_forget", "optimizer", "device", "epoch", "batch", "reg_lambda", "regularization_terms",
                        "losses_CE", "losses_regularization", "losses_total", "task_i", "testloader_forget", "testloader_remain",
                        "forget_acc_before", "highest_H_mean", "cfg", "testloader_open"]      # reference engine_cl.py:463-483


def test_header_bindings_and_exports_of_the_third_library_agree():
    from gslora_hip import _lib_reg, build
    header = open(os.path.join(ROOT, "include", "gslora_reg.h")).read()
    protos = dict(re.findall(r"GSL_API [a-z *]+\b(gsr_[a-z0-9_]+)\(([^;]*)\);", header))
    assert set(protos) == set(_lib_reg.SIGNATURES) == exported(build.side_out("reg"))
    assert {"gsr_importance_acc", "gsr_sq_mean_fwd", "gsr_sq_mean_bwd", "gsr_sq_mean_ws_elems", "gsr_reg_multi_layout", "gsr_reg_multi_fwd",
            "gsr_reg_multi_bwd", "gsr_last_error"} == set(protos)
    for name, argtypes in _lib_reg.SIGNATURES.items():
        proto = protos[name]
        n = 0 if proto.strip() in ("", "void") else len(proto.split(","))
        assert n == len(argtypes), name
    for lines in ("train_own_forget_cl.py:1501-1509", "train_own_forget_cl.py:1548-1549", "engine_cl.py:449-459"):
        assert lines in header, "the header comment names the reference lines"
    # the struct of the entry table: the ctypes mirror has the header's fields in the header's order, and the size a 64-bit build gives it
    body = re.search(r"typedef struct gsr_reg_entry \{(.*?)\} gsr_reg_entry;", header, re.S).group(1)
    fields = re.findall(r"\b(\w+);", body)
    assert fields == [f[0] for f in _lib_reg.RegEntry._fields_]
    import ctypes
    assert ctypes.sizeof(_lib_reg.RegEntry) == 56


def test_the_third_library_is_opened_lazily():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import gslora_hip._lib_reg as r, gslora_hip.reg, gslora_hip.step, engine_reg, engine_cl, driver_reg\n"
            "assert not r.loaded()\n"
            "assert 'libgslora_reg' not in open('/proc/self/maps').read()\n"
            "r.load(); assert r.loaded() and 'libgslora_reg' in open('/proc/self/maps').read()\n"
            "assert 'libgslora_train' not in open('/proc/self/maps').read()\n" % (ROOT, os.path.join(ROOT, "gs-lora_amd")))
    subprocess.check_call([sys.executable, "-c", code])


def test_no_kernel_of_the_third_library_spills_registers():
    """Read from the code-object notes (product_libs.kernel_notes): every gfx950 kernel of libgslora_reg.so declares
    .vgpr_spill_count 0 and no private segment, and is bound by __launch_bounds__(256)."""
    from gslora_hip import build as B
    notes = kernel_notes(B.side_out("reg"))
    kernels, bad = [k[0] for k in notes], [k for k in notes if k[1] or k[2] or k[3] != 256]
    # importance_acc; sq_mean partial, reduce, bwd; reg_multi partial, reduce, bwd
    assert len(kernels) == 7 and sum("reg_multi" in k for k in kernels) == 3 and sum("sq_mean" in k for k in kernels) == 3, kernels
    assert not bad, bad


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2 ** 20, 2 ** 20 + 1, 3 * 2 ** 20 + 5])
def test_layout_has_the_partition_of_gst_reg_quad_fwd(n):
    """gsr_reg_multi_layout is a host function (no GPU here): three terms of (a small tensor, a tensor of n elements). nblk = min(1024,
    ceil(n / 1024)) — what gst_reg_quad_ws_elems of the second library answers for the same n — and chunk = ceil(n / nblk)."""
    from gslora_hip import _lib_reg as LR, _lib_train as LT
    small = 5
    entries = [(0x1000, 0x2000 + k * 16, None if k == 1 else 0x3000, small) for k in range(3)]
    entries = [e for k in range(3) for e in (entries[k], (0x100000, 0x200000 + k * 16, None if k == 1 else 0x300000, n))]
    table, total, bwd, g_elems = LR.reg_multi_layout(entries, 3, 2)
    nblk = min(1024, -(-n // 1024))
    assert nblk == LT.load().gst_reg_quad_ws_elems(n)
    blk = 0
    for k in range(3):
        for t, (nn, nb) in enumerate(((small, 1), (n, nblk))):
            e = table[2 * k + t]
            assert (e.n, e.nblk, e.chunk, e.blk0) == (nn, nb, -(-nn // nb), blk), (k, t)
            assert e.nblk * e.chunk >= e.n > (e.nblk - 1) * e.chunk      # every workgroup has work
            assert (e.omega is None) == (k == 1) and e.goff == (0 if t == 0 else 8)
            blk += nb
    assert total == blk == 3 * (1 + nblk) and bwd == 1 + nblk and g_elems == 8 + (n + 3) // 4 * 4


def test_layout_refuses_what_it_cannot_lay_out():
    from gslora_hip import _lib_reg as LR
    with pytest.raises(RuntimeError, match="same p and n"):
        LR.reg_multi_layout([(0x1000, 0x2000, None, 5), (0x1010, 0x2000, None, 5)], 2, 1)
    with pytest.raises(RuntimeError, match="1 <= n < 2\\^31"):
        LR.reg_multi_layout([(0x1000, 0x2000, None, 0)], 1, 1)
    with pytest.raises(RuntimeError, match="null tensor"):
        LR.reg_multi_layout([(0x1000, None, None, 4)], 1, 1)
    lib = LR.load()
    assert lib.gsr_importance_acc(4096, 4096, 0, 0, 1.0, 1.0, None, None, None) == -1 and b"1 <= n < 2^31" in lib.gsr_last_error()
    assert lib.gsr_importance_acc(4096, 4096, 4, 2, 1.0, 1.0, None, None, None) == -1 and b"kind" in lib.gsr_last_error()
    assert lib.gsr_importance_acc(4096, 4098, 4, 0, 1.0, 1.0, None, None, None) == -1 and b"4-byte aligned" in lib.gsr_last_error()
    assert lib.gsr_sq_mean_ws_elems(0, 4) == -1 and lib.gsr_sq_mean_ws_elems(1 << 16, 1 << 15) == -1
    assert lib.gsr_sq_mean_fwd(4096, 3, 2, 4, 4096, 4096, None) == -1 and b"ldx >= C" in lib.gsr_last_error()
    assert lib.gsr_reg_multi_fwd(4096, 2, 1, 4096, 4096, None) == -1 and lib.gsr_reg_multi_bwd(4096, 1, 1, 1, None, 4096, None) == -1


def test_the_epoch_loop_has_the_reference_parameters_and_the_stub_stays():
    import engine_cl
    import engine_reg
    sig = inspect.signature(engine_reg.train_one_epoch_regularzation)
    assert list(sig.parameters) == REFERENCE_PARAMETERS and len(REFERENCE_PARAMETERS) == 19
    assert sig.parameters["testloader_open"].default is None
    assert all(p.default is inspect.Parameter.empty for n, p in sig.parameters.items() if n != "testloader_open")
    with pytest.raises(NotImplementedError):
        engine_cl.train_one_epoch_regularzation()
    assert engine_reg.RegMeterQueue.ORDER[:3] == ("losses_CE", "losses_regularization", "losses_total")


def test_ffn_reg_step_takes_reg_terms_by_their_loss_method():
    """A dict or None goes to step.reg_loss as before; an object with .loss() is asked for the term (checked here without a GPU: the call
    reaches the model, which refuses CPU tensors, only after the dispatch was decided — so the dispatch is read from the source)."""
    from gslora_hip import reg, step
    src = inspect.getsource(step.ffn_reg_step)
    assert "regularization_terms.loss(" in src and "reg_loss(model, regularization_terms, reg_lambda, logits.device)" in src
    assert callable(reg.RegTerms.loss) and reg.KINDS == ("l2", "ewc", "mas")
    rt = reg.RegTerms(torch.nn.Linear(2, 2), None, 0.5)      # no terms: nothing is laid out, the loss is a zero
    z = rt.loss("cpu")
    assert z.dim() == 0 and z.item() == 0.0
    with pytest.raises(ValueError, match="kind 'si'"):
        reg.calculate_importance(torch.nn.Linear(2, 2), [], "si")
    ones = reg.calculate_importance(torch.nn.Linear(2, 3), None, "l2")
    assert sorted(ones) == ["bias", "weight"] and all(bool((v == 1).all()) for v in ones.values()) and ones.skipped == 0


def test_fixtures_hold_arrays_only(golden_dir):
    for tag in FIXTURES:
        path = os.path.join(golden_dir, f"{tag}.npz")
        assert os.path.getsize(path) < (1 << 20)
        g = np.load(path, allow_pickle=False)
        assert all(g[k].dtype.kind in "fiuU" for k in g.files), tag
    g = np.load(os.path.join(golden_dir, "importance_small.npz"))
    names = g["trainable"].tolist()
    assert len(names) == 9 and g["batch_sizes"].tolist() == [3, 2]
    for n in names:
        for kind in ("ewc", "mas", "ewc_online"):
            assert g[f"{kind}::{n}"].dtype == np.float32 and (g[f"{kind}::{n}"] >= 0).all() and g[f"{kind}::{n}"].max() > 0
        # the accumulation the generator states, restated: the fixture is consistent with its own per-batch gradients
        ewc = sum(torch.tensor(g[f"grad_ewc::{b}::{n}"]) ** 2 * s / 2 for b, s in enumerate((3, 2)))
        assert np.allclose(ewc.numpy(), g[f"ewc::{n}"], rtol=1e-6, atol=0) and np.allclose(2 * ewc.numpy(), g[f"ewc_online::{n}"], rtol=1e-6, atol=0)
    g = np.load(os.path.join(golden_dir, "reg_epoch_small_engine.npz"))
    assert g["steps"].shape == (5, 3) and g["returned"].shape == (3, 4) and int(g["batch"]) == 6
    assert np.allclose(g["steps"][:, 0] + g["steps"][:, 1], g["steps"][:, 2], rtol=1e-6)
    assert all(0.1 < reg / ce < 5.0 for ce, reg, _ in g["steps"])      # the two terms weigh about as much as the cross-entropy
    assert sum(k.startswith("final::") for k in g.files) == len(g["trainable"]) == 9


def test_fixtures_regenerate_to_the_same_bits(golden_dir, tmp_path):
    from oracle.make_golden import REF
    if not os.path.isdir(os.path.join(REF, "vit_pytorch_face")):
        pytest.skip("the reference sources are not on this machine")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_golden_reg_baselines.py"), "--out", str(tmp_path)],
                          stdout=subprocess.DEVNULL)
    for tag in FIXTURES:
        old, new = np.load(os.path.join(golden_dir, f"{tag}.npz")), np.load(os.path.join(str(tmp_path), f"{tag}.npz"))
        assert sorted(old.files) == sorted(new.files), tag
        for k in old.files:
            assert old[k].dtype == new[k].dtype and old[k].shape == new[k].shape and np.array_equal(old[k], new[k]), (tag, k)


def test_the_driver_parses_its_flags_and_refuses_without_a_gpu(monkeypatch):
    import driver_reg
    a = driver_reg.get_args(["--ewc", "--small"])
    assert a.ewc and not a.l2 and not a.MAS and a.only_ffn and not a.online and not a.ffn_open
    assert (a.l2_lambda, a.ewc_lambda, a.mas_lambda) == (0.1, 0.1, 0.1)      # the reference's defaults (util/args.py:205-217)
    assert driver_reg.kind_of(driver_reg.get_args(["--MAS", "--mas_lambda", "3"])) == ("mas", 3.0)
    with pytest.raises(SystemExit):
        driver_reg.get_args(["--ewc", "--l2"])
    with pytest.raises(SystemExit):
        driver_reg.get_args([])      # one of --l2 | --ewc | --MAS is required
    assert "only_ffn" in driver_reg.__doc__ and "always" in driver_reg.get_args.__doc__ + driver_reg.__doc__.lower()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        driver_reg.main(["--small", "--ewc"])
    from vit_pytorch_face import ViT_face
    m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=10, image_size=48, patch_size=8, dim=64, depth=2, heads=1, mlp_dim=128, lora_rank=0)
    assert len(driver_reg.mark_only_ffn_as_trainable(m)) == 8 and driver_reg.mark_only_ffn_as_trainable(m, True)[-1] == "loss.weight"
