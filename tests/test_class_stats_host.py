"""CPU tests of the per-class evaluation: the C ABI of the three entry points of csrc/classstat.hip (header = exports = _lib.SIGNATURES,
argument checks before any launch), util.utils.write_class_accuracy against the lines the real reference wrote
(tests/golden/class_stats_small.npz, tools/make_golden_class_stats.py), the fixture's own consistency, and the Python surface."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"gsl_class_stats", "gsl_class_embed_sum", "gsl_class_finish"}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "class_stats_small.npz"), allow_pickle=False)      # raises on an object array


def test_header_signatures_and_exports_hold_the_three_entry_points():
    from gslora_hip import _lib
    header = open(os.path.join(ROOT, "include", "gslora_hip.h")).read()
    declared = set(re.findall(r"\b(gsl_[a-z0-9_]+)\s*\(", header)) - {"gsl_dropout_keep"}      # as tests/test_host_logic.py
    assert NEW <= declared and declared == set(_lib.SIGNATURES)
    for name in NEW:      # prototype arity == binding arity
        proto = re.search(r"GSL_API int " + name + r"\(([^;]*)\);", header).group(1).strip()
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]), name
    for name, lines in (("gsl_class_stats", "test_own.py:120-130"), ("gsl_class_embed_sum", "util/utils.py:540-542"),
                        ("gsl_class_finish", "util/utils.py:547")):
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


def test_entry_points_check_their_arguments_before_any_launch():
    from gslora_hip import _lib
    L = _lib.load()
    p = 16      # a non-null address that is never dereferenced: the argument check fails first
    good = dict(stats=(p, 10, p, 4, 10, p, p, p, None, None), esum=(p, 8, p, 4, 8, 10, p, p, p, None), fin=(p, p, p, 10, 8, p, p, None))
    entry = dict(stats=L.gsl_class_stats, esum=L.gsl_class_embed_sum, fin=L.gsl_class_finish)

    def refused(which, **change):
        args = list(good[which])
        for i, v in change.items():
            args[int(i[1:])] = v
        rc = entry[which](*args)
        return rc == -1 and entry[which].__name__.encode() in L.gsl_last_error()

    # gsl_class_stats(logits, ld, labels, B, C, count, hit, bad, confusion, stream): confusion alone is nullable
    for i in (0, 2, 5, 6, 7):
        assert refused("stats", **{f"a{i}": None}), i
    assert refused("stats", a4=0) and refused("stats", a4=-3) and refused("stats", a3=0)      # C <= 0, B <= 0
    assert refused("stats", a1=9) and refused("stats", a1=0) and refused("stats", a1=-10)      # row stride below C
    # gsl_class_embed_sum(emb, ld, labels, B, D, C, sum, count, bad, stream)
    for i in (0, 2, 6, 7, 8):
        assert refused("esum", **{f"a{i}": None}), i
    assert refused("esum", a5=0) and refused("esum", a5=-1) and refused("esum", a4=0) and refused("esum", a3=0)
    assert refused("esum", a1=7) and refused("esum", a4=(1 << 20) + 1, a1=1 << 21)      # row stride below D; D beyond the grid's reach
    # gsl_class_finish(count, hit, sum, C, D, acc, proto, stream): acc needs hit, proto needs sum and D > 0, one output at least
    assert refused("fin", a0=None) and refused("fin", a3=0) and refused("fin", a3=-2)
    assert refused("fin", a5=None, a6=None) and refused("fin", a1=None) and refused("fin", a2=None) and refused("fin", a4=0)


def test_write_class_accuracy_reproduces_the_reference_file(golden, tmp_path):
    from util.utils import write_class_accuracy
    want = "".join(line + "\n" for line in golden["stats_lines"].tolist()).encode()
    path = str(tmp_path / "class_accuracy.txt")
    # the reference's own lists (floats), and what eval_data_per_class returns (int64 tensors)
    write_class_accuracy(path, golden["stats_correct"].tolist(), golden["stats_total"].tolist())
    assert open(path, "rb").read() == want
    write_class_accuracy(path, torch.tensor(golden["stats_correct"]).long(), torch.tensor(golden["stats_total"]).long())
    assert open(path, "rb").read() == want
    write_class_accuracy(path, [1, 0], [3, 0])      # a class without samples: the reference divides by zero there
    assert open(path).read() == "33.3333 %\n nan %\n"      # "%4.4f" of NaN
    with pytest.raises(ValueError, match="write_class_accuracy"):
        write_class_accuracy(path, [1, 2], [3])


def test_fixture_is_self_consistent(golden, golden_dir):
    g = golden
    assert os.path.getsize(os.path.join(golden_dir, "class_stats_small.npz")) < (1 << 20)
    assert all(g[k].dtype.kind in "fiuU" for k in g.files)
    y, tot, cor = g["stats_labels"], g["stats_total"], g["stats_correct"]
    C = tot.shape[0]
    assert np.array_equal(np.bincount(y, minlength=C), tot) and (cor <= tot).all() and (tot > 0).all()
    assert y.shape[0] % int(g["stats_batch"]) == 0      # the reference's loop indexes range(batch_size): full batches only
    assert g["stats_accuracy"] == 100 * cor.sum() / tot.sum() and 0 < cor.sum() < tot.sum()
    assert g["stats_lines"].tolist() == ["%4.4f %%" % (100 * c / t) for c, t in zip(cor.tolist(), tot.tolist())]
    py, keys = g["proto_labels"], g["proto_keys"].tolist()
    assert keys == sorted(set(py.tolist())) and int(g["proto_absent"]) not in keys
    assert len(set(np.bincount(py).tolist())) > 2 and py.shape[0] % int(g["proto_batch"]) != 0      # unequal classes, ragged last batch
    assert g["proto_vals"].shape == (len(keys), 128) and g["proto_vals"].dtype == np.float32


def test_python_surface():
    import driver_cl
    import engine
    import engine_cl
    from gslora_hip import ops
    want = ["model", "dataloader", "device", "mode", "batch", "num_classes", "confusion"]
    for mod in (engine, engine_cl):
        sig = inspect.signature(mod.eval_data_per_class)
        assert list(sig.parameters) == want
        assert (sig.parameters["batch"].default, sig.parameters["num_classes"].default, sig.parameters["confusion"].default) == (0, None, False)
    assert list(inspect.signature(engine_cl.eval_data).parameters) == want[:5]      # eval_data itself is untouched
    assert driver_cl.get_args([]).per_class is False and driver_cl.get_args(["--per_class"]).per_class is True
    assert inspect.signature(driver_cl.run_tasks).parameters["per_class"].default is None
    # device work on CPU tensors is refused loudly, not emulated
    lo, y, cnt, bad = torch.zeros(4, 6), torch.zeros(4, dtype=torch.long), torch.zeros(6, dtype=torch.long), torch.zeros(1, dtype=torch.long)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.class_stats(lo, y, cnt, cnt.clone(), bad)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.class_embed_sum(lo, y, torch.zeros(6, 6), cnt, bad)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.class_finish(cnt, hit=cnt.clone())
    with pytest.raises(ValueError, match="number of classes"):
        ops.ClassStats(0, "cpu")
