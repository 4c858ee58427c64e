"""CPU tests of the l2 prototype distance and of precision@k: the fixtures of tools/make_golden_proto_l2.py regenerate to the same bits
where the reference sources are present, get_prototype_loss / train_accuracy argument handling, the no-tie property of the top-k fixture
inputs, and the C ABI of the five new entry points (header = exports = _lib.SIGNATURES)."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"gsl_proto_l2_fwd", "gsl_proto_l2_bwd", "gsl_loss_tail_l2", "gsl_topk_max_k", "gsl_topk_hits"}
FIXTURES = ("proto_l2_small2_b3", "proto_l2_small6_engine", "topk_small")


def test_fixtures_regenerate_to_the_same_bits(golden_dir, tmp_path):
    from oracle.make_golden import REF
    if not os.path.isdir(os.path.join(REF, "vit_pytorch_face")):
        pytest.skip("the reference sources are not on this machine")
    # a child process: the generator installs import shims and patches torch for the reference's sake
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_golden_proto_l2.py"), "--out", str(tmp_path)],
                          stdout=subprocess.DEVNULL)
    for tag in FIXTURES:
        old, new = np.load(os.path.join(golden_dir, f"{tag}.npz")), np.load(os.path.join(str(tmp_path), f"{tag}.npz"))
        assert sorted(old.files) == sorted(new.files), tag
        for k in old.files:
            assert old[k].dtype == new[k].dtype and old[k].shape == new[k].shape, (tag, k)
            assert old[k].tobytes() == new[k].tobytes(), (tag, k)


def test_fixtures_hold_arrays_only_and_the_keys_of_their_models(golden_dir):
    a, b = np.load(os.path.join(golden_dir, "proto_l2_small2_b3.npz")), np.load(os.path.join(golden_dir, "arcface_small2_b3.npz"))
    assert set(b.files) <= set(a.files) and set(a.files) - set(b.files) == {k for k in a.files if k.startswith("hyper_")}
    a, b = np.load(os.path.join(golden_dir, "proto_l2_small6_engine.npz")), np.load(os.path.join(golden_dir, "arcface_small6_engine.npz"))
    assert set(b.files) <= set(a.files) and set(a.files) - set(b.files) == {k for k in a.files if k.startswith("hyper_")}
    for tag in FIXTURES:
        path = os.path.join(golden_dir, f"{tag}.npz")
        assert os.path.getsize(path) < (1 << 20)
        g = np.load(path, allow_pickle=False)      # raises on an object array
        assert all(g[k].dtype.kind in "fiuU" for k in g.files), tag
    g = np.load(os.path.join(golden_dir, "proto_l2_small2_b3.npz"))
    # losses1 = [ce_f, ce_r, total, structure, l2_f, l2_r]: the prototype hinge is active in losses1 / grad1 and inactive in *_inactive
    assert 0.1 < g["losses1"][4] < g["hyper_BND_pro"]


def test_get_prototype_loss_argument_handling():
    import engine_cl
    sig = inspect.signature(engine_cl.get_prototype_loss)
    assert list(sig.parameters) == ["output", "labels", "prototype_dict", "distance"] and sig.parameters["distance"].default == "kl"
    emb, y = torch.zeros(2, 8), torch.zeros(2, dtype=torch.long)
    proto = {0: torch.zeros(8)}
    # any other string: the reference's initial value (engine_cl.py:586, :603), before any device work
    assert engine_cl.get_prototype_loss(emb, y, proto, distance="euclidean") == 0.0
    assert engine_cl.get_prototype_loss(emb, y, proto, distance="L2") == 0.0
    for d in ("kl", "l2"):      # served distances run on the device: CPU tensors are refused loudly, not emulated
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            engine_cl.get_prototype_loss(emb, y, proto, distance=d)


def test_step_and_engines_take_the_distance():
    import driver_cl
    import engine
    import engine_cl
    from gslora_hip import losses, step
    assert inspect.signature(step.gs_lora_step).parameters["proto_distance"].default == "kl"
    assert losses.check_proto_distance("l2") == "l2" and losses.check_proto_distance("kl") == "kl"
    with pytest.raises(ValueError, match="proto_distance"):
        losses.check_proto_distance("cosine")
    for name in ("proto_l2_sum", "proto_l2_sum_split", "loss_tail_l2"):
        assert hasattr(step.HipBackend, name)
    for mod in (engine, engine_cl):
        assert 'cfg.get("PROTO_DISTANCE", "kl")' in inspect.getsource(mod.train_one_epoch)
    assert driver_cl.get_args([]).pro_distance == "kl" and driver_cl.get_args(["--pro_distance", "l2"]).pro_distance == "l2"
    with pytest.raises(SystemExit):
        driver_cl.get_args(["--pro_distance", "cosine"])


def test_graph_key_separates_the_distances():
    from gslora_hip.step import GraphedStep

    class Net(torch.nn.Module):
        compute_dtype = torch.float32

        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

    net = Net()
    g = GraphedStep(net, torch.optim.AdamW(net.parameters(), lr=0.1), torch.nn.CrossEntropyLoss())
    x, y = torch.zeros(2, 3, 8, 8), torch.zeros(2, dtype=torch.long)
    kw = dict(beta=0.1, alpha=0.1, BND=1.0, use_prototype=True, proto_table=torch.zeros(4, 8))
    k_kl, k_l2 = g._key(x, y, x, y, dict(kw, proto_distance="kl")), g._key(x, y, x, y, dict(kw, proto_distance="l2"))
    assert k_kl != k_l2 and k_kl == g._key(x, y, x, y, dict(kw, proto_distance="kl"))


def test_topk_argument_handling():
    from util.utils import train_accuracy
    assert list(inspect.signature(train_accuracy).parameters) == ["output", "target", "topk"]
    out, y = torch.zeros(4, 6), torch.zeros(4, dtype=torch.long)
    for bad in ((), (0,), (1, 7), (-1, 2)):      # k must lie in [1, number of classes] (torch.topk refuses the rest in the reference)
        with pytest.raises(ValueError, match="topk"):
            train_accuracy(out, y, topk=bad)
    for ks in ((1,), (1, 5), [5, 1, 3]):      # served tuples run on the device: CPU tensors are refused loudly
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            train_accuracy(out, y, topk=ks)


def test_topk_fixture_inputs_have_no_tie_at_any_kth_place(golden_dir):
    g = np.load(os.path.join(golden_dir, "topk_small.npz"))
    lo, y = torch.tensor(g["logits"]), torch.tensor(g["labels"])
    srt = torch.sort(lo, dim=1, descending=True).values
    assert (srt[:, :-1] > srt[:, 1:]).all(), "every row strictly ordered: no tie at any place, so torch.topk's choice is unambiguous"
    rank = (lo > lo.gather(1, y[:, None])).sum(1)      # the count the HIP kernel takes
    n = lo.shape[0]
    for name in ("1_5", "5_1_3"):
        ks = g[f"topk_{name}"].tolist()
        want = [np.float32(float((rank < k).sum()) * np.float32(100.0 / n)) for k in ks]
        assert ks == {"1_5": [1, 5], "5_1_3": [5, 1, 3]}[name]
        assert g[f"perk_{name}"].tolist() == [float(w) for w in want]
        assert g[f"ret_{name}"] == g[f"perk_{name}"][0]      # the reference returns its first entry (util/utils.py:368)
        assert 0 < min(want) and max(want) < 100      # every k sees hits and misses


def test_header_signatures_and_exports_hold_the_new_entry_points():
    from gslora_hip import _lib
    header = open(os.path.join(ROOT, "include", "gslora_hip.h")).read()
    declared = set(re.findall(r"\b(gsl_[a-z0-9_]+)\s*\(", header)) - {"gsl_dropout_keep"}      # as tests/test_verification_host.py
    assert NEW <= declared and declared == set(_lib.SIGNATURES)
    for name in NEW:      # prototype arity == binding arity
        proto = re.search(r"GSL_API int " + name + r"\(([^;]*)\);", header).group(1).strip()
        n = 0 if proto == "void" else len(proto.split(","))
        assert n == len(_lib.SIGNATURES[name]), name
    # the l2 pair and the l2 tail mirror their KL counterparts argument for argument
    assert _lib.SIGNATURES["gsl_proto_l2_fwd"] == _lib.SIGNATURES["gsl_proto_kl_fwd"]
    assert _lib.SIGNATURES["gsl_proto_l2_bwd"] == _lib.SIGNATURES["gsl_proto_kl_bwd"]
    assert _lib.SIGNATURES["gsl_loss_tail_l2"] == _lib.SIGNATURES["gsl_loss_tail"]
    for name, lines in (("gsl_proto_l2_fwd", "engine_cl.py:593-594"), ("gsl_topk_hits", "util/utils.py:354-368")):
        assert lines in header[:header.index("GSL_API int " + name)], "the header comment names the reference lines"
    assert "gsl_*" in open(os.path.join(ROOT, "gs-lora_amd", "csrc", "exports.map")).read()
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
    so = os.path.join(ROOT, "gs-lora_amd", "gslora_hip", "libgslora_hip.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True)
    if nm.returncode == 0:
        exported = {ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln}
        assert exported == set(_lib.SIGNATURES)


def test_new_entry_points_check_their_arguments_before_any_launch():
    import ctypes
    from gslora_hip import _lib, ops
    L = _lib.load()
    p = 16      # a non-null address that is never dereferenced: the argument check fails first
    assert L.gsl_topk_max_k() == 16 == ops.topk_max_k()
    assert L.gsl_proto_l2_fwd(p, p, p, p, p, 0, 8, 4, None) == -1 and b"gsl_proto_l2_fwd" in L.gsl_last_error()
    assert L.gsl_proto_l2_bwd(p, p, p, None, 1.0, p, 2, 8, 4, 0, None) == -1 and b"gsl_proto_l2_bwd" in L.gsl_last_error()
    # the l2 tail needs the prototype term, and keeps the bounds of gsl_loss_tail (0 < nr < N <= 256 rows, C and D <= 1024)
    assert L.gsl_loss_tail_l2(p, p, 8, 4, 10, None, None, 0, 0, None, 0., 0., 0., 0., 0., 0., p, p, None, None) == -1
    assert b"emb, proto and demb are required" in L.gsl_last_error()
    assert L.gsl_loss_tail_l2(p, p, 257, 4, 10, p, p, 8, 4, None, 0., 0., 0., 0., 0., 0., p, p, p, None) == -1
    assert L.gsl_loss_tail_l2(p, p, 8, 4, 10, p, p, 1025, 4, None, 0., 0., 0., 0., 0., 0., p, p, p, None) == -1
    ks = (ctypes.c_int * 17)(*range(1, 18))
    assert L.gsl_topk_hits(p, p, 4, 10, ks, 17, p, None) == -1 and b"nk <= 16" in L.gsl_last_error()
    assert L.gsl_topk_hits(p, p, 4, 10, (ctypes.c_int * 2)(1, 0), 2, p, None) == -1 and b"k > 0" in L.gsl_last_error()
