"""CPU tests of the LIRF baseline: the two half-network modules (the reference's state-dict keys, a full-checkpoint load, the depth // 2 split,
their refusals), the sixth product library's ABI (header, version script, bindings and exported symbols agree; it cross-compiles for gfx950;
no kernel spills; it stays closed in a process that runs the other steps' host paths), lirf_step's signature and the refusals it makes
before any launch, the loop's signatures against the reference's recorded ones and its structure with a stubbed step, and the driver's
arguments. The arithmetic is tested on the GPU (tests/test_hip_at_kernels.py, tests/test_hip_lirf.py)."""
import inspect
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from product_libs import exported, kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"gsa_last_error", "gsa_at_plan", "gsa_at_ws_elems", "gsa_at_fwd", "gsa_at_bwd"}
GEO = dict(loss_type="CosFace", GPU_ID=[0], num_class=10, image_size=40, patch_size=8, dim=64, heads=1, mlp_dim=128)


def halves(depth, lora_rank=0, **kw):
    from vit_pytorch_face import ViT_face, ViT_face_low, ViT_face_up
    geo = dict(GEO, depth=depth, lora_rank=lora_rank, **kw)
    return ViT_face(**geo), ViT_face_low(**geo), ViT_face_up(**geo)


# ---------------------------------------------------------------------------------------------------------------- the modules
def test_the_halves_have_the_reference_keys_and_load_a_full_checkpoint(golden_dir):
    want = json.load(open(os.path.join(golden_dir, "lirf_signatures.json")))
    from oracle import recipe
    from vit_pytorch_face import ViT_face, ViT_face_low, ViT_face_up
    for tag, cfg in (("depth2", recipe.cfg_small(lora_rank=0)), ("depth3", recipe.cfg_small2(lora_rank=0))):
        kw = dict(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                  dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], lora_rank=0)
        full, low, up = ViT_face(**kw), ViT_face_low(**kw), ViT_face_up(**kw)
        assert list(low.state_dict()) == want[f"ViT_face_low::{tag}"] and list(up.state_dict()) == want[f"ViT_face_up::{tag}"]
        k = cfg["depth"] // 2
        res = low.load_state_dict(full.state_dict(), strict=False)
        assert not res.missing_keys and res.unexpected_keys
        assert all(re.match(rf"transformer\.layers\.({'|'.join(str(i) for i in range(k, cfg['depth']))})\.", n) for n in res.unexpected_keys)
        res = up.load_state_dict(full.state_dict(), strict=False)
        assert not res.missing_keys and not res.unexpected_keys
        for n, p in full.state_dict().items():
            assert torch.equal(up.state_dict()[n], p) and (n not in low.state_dict() or torch.equal(low.state_dict()[n], p)), n
    for cls in (ViT_face_low, ViT_face_up):
        sig = inspect.signature(cls.__init__)
        rec = want[f"{cls.__name__}::init"]
        assert [n for n in sig.parameters if n != "self"] == rec["parameters"]
        assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in sig.parameters.items() if n != "self")
        for n, d in rec["defaults"].items():
            assert sig.parameters[n].default == d, n


def test_construction_without_the_required_keywords_is_still_not_implemented():
    from vit_pytorch_face import ViT_face_low, ViT_face_up
    for cls in (ViT_face_low, ViT_face_up):
        with pytest.raises(NotImplementedError, match="loss_type, GPU_ID, num_class, image_size, patch_size, dim, depth, heads, mlp_dim"):
            cls()
        with pytest.raises(NotImplementedError, match="missing depth$"):
            cls(**GEO)
        with pytest.raises(NotImplementedError, match="depth must be at least 2"):
            cls(**GEO, depth=1)


@pytest.mark.parametrize("depth", [2, 3, 6])
def test_the_split_is_depth_over_two(depth):
    full, low, up = halves(depth)
    k = depth // 2
    assert len(low.transformer.layers) == k and len(up.transformer.layers) == depth and low.split == up.split == k
    sl, su = low.hip_spec(), up.hip_spec()
    assert len(sl.blocks) == k and sl.stream_out and not sl.stream_in and sl.final_ln is None and sl.block0 == 0
    assert len(su.blocks) == depth - k and su.stream_in and not su.stream_out and su.block0 == k
    assert su.blocks[0].l1 is up.transformer.layers[k][1].fn.fn.net[0]
    from vit_pytorch_face.vit_face import low_up_pair
    sp = low_up_pair(low, up).hip_spec()
    assert len(sp.blocks) == depth and sp.boundary == k and not sp.stream_in and not sp.stream_out
    assert sp.blocks[k - 1].l1 is low.transformer.layers[k - 1][1].fn.fn.net[0] and sp.blocks[k].l1 is up.transformer.layers[k][1].fn.fn.net[0]
    assert sp.patch_w is low.patch_to_embedding.weight and sp.head_w is up.loss.weight and sp.final_ln is up.mlp_head[0]
    assert low_up_pair(low, up) is low_up_pair(low, up)


def test_the_modules_refuse_what_they_do_not_run():
    from vit_pytorch_face.vit_face import low_up_forward
    _, low, up = halves(3)
    x, mid = torch.zeros(2, 3, 40, 40), torch.zeros(2, 26, 64)
    with pytest.raises(NotImplementedError, match="attention masks"):
        low(x, None, torch.ones(1))
    with pytest.raises(NotImplementedError, match="attention masks"):
        up(mid, None, torch.ones(1))
    for call in (lambda: low(x), lambda: up(mid)):
        with pytest.raises(RuntimeError, match="gslora_hip.step.lirf_step"):      # trainable parameters, gradients enabled
            call()
    for m in (low, up):
        for p in m.parameters():
            p.requires_grad_(False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # frozen: a forward, which needs the GPU
        low(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        up(mid)
    with pytest.raises(ValueError, match=r"the lower half's stream \[B, 26, 64\]"):
        up(torch.zeros(2, 25, 64))
    with pytest.raises(RuntimeError, match="a pass over both halves is a training pass"):
        low_up_forward(low, up, x, torch.zeros(2, dtype=torch.int64))
    low.transformer.layers[0][0].fn.norm.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match="trains the FFN linears"):
        low_up_forward(low, up, x, torch.zeros(2, dtype=torch.int64))


def test_lirf_step_signature_and_refusals_before_any_launch(monkeypatch):
    from gslora_hip import step
    sig = inspect.signature(step.lirf_step)
    assert list(sig.parameters) == ["student_low", "deposit_low", "teacher_low", "teacher_up", "optimizer", "criterion", "x_f", "y_f", "x_r", "y_r",
                                    "split", "T", "alpha", "_at_weight"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("split", "T", "alpha", "_at_weight"))
    assert sig.parameters["_at_weight"].default == -300.0
    for text in ("--only_ffn", "deposit_low receives no .grad", "[CE, AT, KP, PT_RE, total, REPLAY]"):
        assert text in step.lirf_step.__doc__
    full, low, up = halves(3)
    _, lora_low, _ = halves(3, lora_rank=4)
    x, y = torch.zeros(2, 3, 40, 40), torch.zeros(2, dtype=torch.int64)
    kw = dict(split=5, T=2.0, alpha=0.5)
    with pytest.raises(RuntimeError, match="holds LoRA adapters \\(lora_rank = 4\\)"):
        step.lirf_step(lora_low, low, low, up, None, None, x, y, x, y, **kw)
    with pytest.raises(RuntimeError, match="student_low must be a ViT_face_low, got ViT_face"):
        step.lirf_step(full, low, low, up, None, None, x, y, x, y, **kw)
    with pytest.raises(RuntimeError, match="teacher_up must be a ViT_face_up, got ViT_face_low"):
        step.lirf_step(low, low, low, low, None, None, x, y, x, y, **kw)
    graphed = object.__new__(step.GraphedStep)
    with pytest.raises(RuntimeError, match="lirf_step is eager; GraphedStep captures the LoRA-only step"):
        step.lirf_step(graphed, low, low, up, None, None, x, y, x, y, **kw)
    replicated = object.__new__(torch.nn.DataParallel)
    torch.nn.Module.__init__(replicated)
    replicated.device_ids, replicated.module = [0, 1], low
    with pytest.raises(RuntimeError, match="nn.DataParallel over several devices is not supported"):
        step.lirf_step(replicated, low, low, up, None, None, x, y, x, y, **kw)
    for split in (0, -1, 10, 11):
        with pytest.raises(ValueError, match="split .* must cut the 10 classes"):
            step.lirf_step(low, low, low, up, None, None, x, y, x, y, split=split, T=2.0, alpha=0.5)
    monkeypatch.setattr(step, "_world", lambda: 2)
    with pytest.raises(RuntimeError, match="lirf_step runs in one process; .*a process group of 2 ranks is active"):
        step.lirf_step(low, low, low, up, None, None, x, y, x, y, **kw)


# ---------------------------------------------------------------------------------------------------------------- the library
def test_header_version_script_bindings_and_exports_of_the_sixth_library_agree():
    from gslora_hip import _lib_at, build
    header = open(os.path.join(ROOT, "include", "gslora_at.h")).read()
    protos = dict(re.findall(r"GSL_API [a-z *]+\b(gsa_[a-z0-9_]+)\(([^;]*)\);", header))
    assert set(protos) == set(_lib_at.SIGNATURES) == exported(build.side_out("at")) == ENTRY_POINTS
    for name, argtypes in _lib_at.SIGNATURES.items():
        proto = protos[name]
        n = 0 if proto.strip() in ("", "void") else len(proto.split(","))
        assert n == len(argtypes), name
    script = open(os.path.join(ROOT, "gs-lora_amd", "csrc", "exports_at.map")).read()
    assert "global: gsa_*;" in script and "local: *;" in script
    assert "baselines/LIRFtrain.py" in header
    assert (_lib_at.MAX_T, _lib_at.MAX_D) == tuple(int(re.search(rf"#define {k} (\d+)", header).group(1)) for k in ("GSA_MAX_T", "GSA_MAX_D"))
    src = open(os.path.join(ROOT, "gs-lora_amd", "csrc", "at.hip")).read()
    assert "getenv" not in src and "atomic" not in src.lower(), "no environment reads, no atomics"


def test_the_sixth_library_cross_compiles_for_gfx950_without_spills(tmp_path):
    """A fresh compile of csrc/at.hip for gfx950 on a machine without a GPU, and — read from the code-object notes, as
    tests/test_distill_host.py reads the fifth library's — every kernel declares .vgpr_spill_count 0, no private segment and
    __launch_bounds__(256)."""
    from gslora_hip import build as B
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), f"{hipcc}: the project cannot be built without hipcc (set HIPCC to its path)"
    obj = os.path.join(str(tmp_path), "at.o")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-c",
                           os.path.join(B.CSRC, "at.hip"), "-o", obj])
    assert os.path.getsize(obj) > 0
    notes = kernel_notes(B.side_out("at"))
    kernels, bad = [k[0] for k in notes], [k for k in notes if k[1] or k[2] or k[3] != 256]
    # sums (f32, f16, bf16), images, value, backward (3 stream types x 3 gradient-stream types)
    assert len(kernels) == 14 and sum("at_sumsq" in k for k in kernels) == 3 and sum("at_bwd" in k for k in kernels) == 9, kernels
    assert not bad, bad


def test_the_plan_cuts_the_token_axis_and_refusals_have_their_text():
    from gslora_hip import _lib_at as LA
    lib = LA.load()
    for B, T, D in ((1, 26, 64), (3, 37, 128), (5, 26, 576), (2, 197, 512), (1, 1025, 1024), (512, 197, 512), (4096, 65, 512)):
        nsplit, chunk, ws = LA.at_plan(B, T, D)
        assert 1 <= nsplit <= 64 and (nsplit - 1) * chunk < T <= nsplit * chunk, "every split holds a token, together all of them"
        assert ws == B * nsplit * 2 * D + B == LA.at_ws_elems(B, T, D)
        assert nsplit == 1 or chunk >= 16 or nsplit == 64
    assert LA.at_plan(512, 197, 512)[0] == 1 and LA.at_plan(1, 1025, 1024)[0] > 32
    P = 4096
    fwd = dict(xs=P, ld_s=64, xt=P, ld_t=64, dtype=0, B=2, T=26, D=64, loss=P, G=P, at_s=None, at_t=None, ws=P)
    cases = [(dict(B=0), b"B >= 1, T >= 1"), (dict(T=0), b"B >= 1, T >= 1"), (dict(T=1026), b"T <= 1025"), (dict(D=96, ld_s=96, ld_t=96), b"multiple of 64"),
             (dict(D=1088, ld_s=1088, ld_t=1088), b"multiple of 64"), (dict(xs=None), b"null xs or xt"), (dict(G=None), b"null loss, G or ws"),
             (dict(dtype=3), b"dtype is GSL_F32, GSL_BF16 or GSL_F16"), (dict(ld_s=60), b"leading dimension >= D"), (dict(xs=P + 4), b"16-byte aligned rows"),
             (dict(ld_t=66), b"16-byte aligned rows"), (dict(dtype=1, ld_s=68), b"16-byte aligned rows"), (dict(G=P + 4), b"G 16-byte aligned")]
    for change, text in cases:
        assert lib.gsa_at_fwd(*{**fwd, **change}.values(), None) == -1 and text in lib.gsa_last_error(), change
        assert b"gsa_at_fwd" in lib.gsa_last_error()
    bwd = dict(xs=P, ld_s=64, x_dtype=2, G=P, coef=P, scale=P, B=2, T=26, D=64, dmid=P, ld_d=64, d_dtype=2)
    for change, text in [(dict(coef=None), b"null xs, G, coef, scale or dmid"), (dict(dmid=None), b"null xs"), (dict(ld_d=63), b"leading dimension >= D"),
                         (dict(d_dtype=3), b"dtype is"), (dict(dmid=P + 8), b"16-byte aligned rows"), (dict(B=1 << 20, T=1025), b"B * T <= 2^24")]:
        assert lib.gsa_at_bwd(*{**bwd, **change}.values(), None) == -1 and text in lib.gsa_last_error(), change
        assert b"gsa_at_bwd" in lib.gsa_last_error()
    assert lib.gsa_at_ws_elems(0, 26, 64) == -1
    with pytest.raises(RuntimeError, match="refused"):
        LA.at_ws_elems(2, 26, 100)


def test_the_python_wrappers_refuse_before_the_library():
    from baselines import LIRFtrain
    from gslora_hip import at
    x = torch.zeros(2, 26, 64)
    for call in (lambda: at.at(x), lambda: at.at_loss(x, x), lambda: at.at_loss_value_and_table(x, 2, 26, x), lambda: LIRFtrain.at(x),
                 lambda: LIRFtrain.at_loss(x, x), lambda: at.at_inject(x, x, torch.zeros(2, 64), torch.zeros(1), None)):
        with pytest.raises(RuntimeError, match="no CPU\\s+fallback"):
            call()
    assert list(inspect.signature(at.at_loss_value_and_table).parameters) == ["xs", "B", "T", "xt"]
    assert list(inspect.signature(at.at_inject).parameters)[:5] == ["dmid", "xs", "G", "coef", "scale"]
    assert list(inspect.signature(LIRFtrain.at).parameters) == ["x"] and list(inspect.signature(LIRFtrain.at_loss).parameters) == ["x", "y"]
    for fn in (at.at, at.at_loss, LIRFtrain.at, LIRFtrain.at_loss):
        assert "not differentiable" in fn.__doc__.replace("NOT", "not")
    assert LIRFtrain.AT().p == 2


def test_the_other_steps_leave_the_sixth_library_closed():
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import torch\n"
            "import test_hip_at_kernels, test_hip_lirf\n"
            "import gslora_hip, gslora_hip._lib_at as a, gslora_hip.at, gslora_hip.step as step, gslora_hip.kd, gslora_hip.fd\n"
            "import baselines.LIRFtrain, baselines.DERtrain, baselines.SCRUBtrain, driver_lirf, driver_distill\n"
            "from vit_pytorch_face import ViT_face, ViT_face_low, ViT_face_up\n"
            "geo = dict(loss_type='CosFace', GPU_ID=[0], num_class=10, image_size=40, patch_size=8, dim=64, depth=2, heads=1, mlp_dim=128, lora_rank=0)\n"
            "m, low, up = ViT_face(**geo), ViT_face_low(**geo), ViT_face_up(**geo)\n"
            "x, y = torch.zeros(2, 3, 40, 40), torch.zeros(2, dtype=torch.int64)\n"
            "for call in (lambda: step.distill_step(m, m, None, None, x, y, x, y, method='fdr', lam=0.1),\n"
            "             lambda: step.scrub_step(m, m, None, None, x, y, maximize=True, kd_T=2.0, sgda_gamma=1.0, sgda_alpha=1.0),\n"
            "             lambda: step.ffn_reg_step(m, None, None, x, y),\n"
            "             lambda: step.gs_lora_step(m, None, None, x, y, x, y, beta=0.1, alpha=0.01, BND=100.0),\n"
            "             lambda: step.lirf_step(low, low, low, up, None, None, x, y, x, y, split=0, T=2.0, alpha=0.5)):\n"
            "    try:\n"
            "        call()\n"
            "    except (RuntimeError, ValueError, NotImplementedError, AttributeError, TypeError):\n"
            "        pass      # (no GPU: every step ends in its own refusal, after its host path)\n"
            "assert not a.loaded() and 'libgslora_at' not in open('/proc/self/maps').read()\n"
            "a.load(); assert a.loaded() and 'libgslora_at' in open('/proc/self/maps').read()\n" % (ROOT, os.path.join(ROOT, "gs-lora_amd"), os.path.join(ROOT, "tests")))
    subprocess.check_call([sys.executable, "-c", code])


# ---------------------------------------------------------------------------------------------------------------- the loop
def test_the_loop_functions_have_the_reference_signatures(golden_dir):
    from baselines import LIRFtrain
    want = json.load(open(os.path.join(golden_dir, "lirf_signatures.json")))
    for name in ("train_one_epoch_LIRF", "eval_data_LIRF", "evaluate_LIRF"):
        sig = inspect.signature(getattr(LIRFtrain, name))
        assert list(sig.parameters) == want[name]["parameters"], name
        assert {n: p.default for n, p in sig.parameters.items() if p.default is not inspect.Parameter.empty} == want[name]["defaults"], name
    assert want["train_one_epoch_LIRF"]["returns"] == 8
    assert (LIRFtrain.DISP_FREQ, LIRFtrain.VER_FREQ) == (5, 5)


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def test_the_loop_with_a_stubbed_step(monkeypatch, capsys):
    """Meter order, the reset every fifth batch, the remain loader's restart, the evaluation every fifth batch with the H-mean formula, the
    return arity."""
    from baselines import LIRFtrain
    from util.utils import AverageMeter
    calls, evals = [], []

    def step(s, d, t, u, opt, crit, x_f, y_f, x_r, y_r, *, split, T, alpha):
        k = len(calls)
        calls.append((int(x_f[0]), int(x_r[0]), split, T, alpha, s.training, d.training, t.training, u.training))
        return torch.tensor([10.0 + k, 20.0 + k, 30.0 + k, 40.0 + k, 50.0 + k, 60.0 + k])

    def eval_data(s, u, loader, device, mode, batch=0):
        evals.append((mode, batch, s.training))
        return {"forget": 30.0, "remain": 80.0, "open": 1.0}[mode.split("-")[0]]

    monkeypatch.setattr(LIRFtrain, "lirf_step", step)
    monkeypatch.setattr(LIRFtrain, "eval_data_LIRF", eval_data)
    nets = [_Net() for _ in range(4)]
    forget = [(torch.full((3,), float(i)), torch.zeros(3)) for i in range(11)]
    remain = [(torch.full((2,), 100.0 + i), torch.zeros(2)) for i in range(4)]
    names = ("losses_CE", "losses_AT", "kd_lossesKP", "losses_pt_re", "losses_total", "losses_remain")
    meters = [AverageMeter() for _ in names]
    opt = torch.optim.SGD(nets[0].parameters(), lr=0.125)
    out = LIRFtrain.train_one_epoch_LIRF(*nets, forget, remain, torch.nn.CrossEntropyLoss(), opt, torch.device("cpu"), 0, 0, *meters, "t", "F", "R",
                                         70.0, 0.0, dict(PER_FORGET_CLS=4, LIRF_T=2.0, LIRF_alpha=0.5), testloader_open="O")
    assert len(out) == 8 and out[0] == 11 and list(out[2:]) == meters
    assert [c[0] for c in calls] == list(range(11))
    assert [c[1] for c in calls] == [100, 101, 102, 103, 100, 101, 102, 103, 100, 101, 102], "the remain loader starts again when exhausted"
    assert all(c[2:] == (4, 2.0, 0.5, True, True, False, False) for c in calls), "student and deposit train(), the teachers eval()"
    # batches 0 .. 4 and 5 .. 9 were displayed and reset; the eleventh step alone is left in the meters
    for j, m in enumerate(meters):
        assert m.count == 3 and m.val == 10.0 * (j + 1) + 10, names[j]
    text = capsys.readouterr().out
    assert "Task t Epoch 1 Batch 5" in text and "Task t Epoch 1 Batch 10" in text and "Batch 11" not in text
    assert "Training CE Loss 14.0000 (12.0000)" in text and "Training AT Loss 24.0000 (22.0000)" in text
    assert "Training total Loss 54.0000 (52.0000)" in text and "Training remain Loss 64.0000 (62.0000)" in text
    assert [e[:2] for e in evals] == [("forget-t", 4), ("remain-t", 4), ("open-t", 4), ("forget-t", 9), ("remain-t", 9), ("open-t", 9)]
    drop = 70.0 - 30.0
    assert out[1] == 2 * drop * 80.0 / (drop + 80.0 + 1e-8)
    assert nets[0].training, "the student is back in train() after an evaluation"
    assert LIRFtrain.evaluate_LIRF(nets[0], nets[3], "F", "R", torch.device("cpu"), 0, 0, "t", 70.0, 99.0, {}, opt) == 99.0


# ---------------------------------------------------------------------------------------------------------------- the driver
def test_the_driver_parses_the_reference_defaults_and_has_no_cpu_fallback(monkeypatch):
    import driver_lirf
    a = driver_lirf.get_args([])
    assert (a.LIRF_T, a.LIRF_alpha) == (10, 0.1) and isinstance(driver_lirf.get_args(["--LIRF_T", "2"]).LIRF_T, float)
    assert driver_lirf.get_args(["--LIRF_alpha", "0.5", "--vit_depth", "2", "--small"]).vit_depth == 2
    for bad in (["--per_forget_cls", "0"], ["--per_forget_cls", "100"], ["--vit_depth", "1"]):
        with pytest.raises(SystemExit):
            driver_lirf.get_args(bad)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        driver_lirf.main(["--small"])
    _, low, _ = halves(3)
    names = driver_lirf.mark_student(low)
    assert len(names) == 4 and all("fn.fn.net" in n for n in names)
