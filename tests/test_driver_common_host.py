"""CPU tests of what the drivers share (gs-lora_amd/driver_common.py): the class split of a task, the geometry, and every driver's
parsed arguments against the ones recorded before the shared options moved into add_common_args (tests/golden/driver_args.json)."""
import importlib
import json
import os
import random

import pytest


def test_task_classes_forgets_from_the_back_of_the_order():
    from driver_common import task_classes
    order = list(range(20))
    random.Random(5).shuffle(order)
    assert order != sorted(order)
    for task_i, (st, en) in enumerate(((16, 20), (12, 16), (8, 12), (4, 8))):
        remain_cls, forget_cls = task_classes(order, 20, 4, task_i)
        assert forget_cls == order[st:en] and remain_cls == order[:st]
        assert len(forget_cls) == 4 and not set(forget_cls) & set(remain_cls)
    assert task_classes(order, 20, 4, 4) == ([], order[0:4])


def test_geometry_is_the_paper_s_or_the_small_one():
    from driver_common import geometry
    assert geometry(False) == dict(image_size=112, patch_size=8, dim=512, depth=6, heads=8, mlp_dim=2048)
    assert geometry(True) == dict(image_size=48, patch_size=8, dim=128, depth=3, heads=2, mlp_dim=256)
    assert geometry(True, 4)["depth"] == 4 and geometry(False, None)["depth"] == 6
    a = geometry(True)
    a["depth"] = 9
    assert geometry(True)["depth"] == 3, "a fresh dictionary every call"


@pytest.mark.parametrize("driver", ["driver_cl", "driver_probe", "driver_reg", "driver_scrub", "driver_distill", "driver_lirf"])
def test_every_driver_parses_what_it_parsed_before(driver, golden_dir, monkeypatch):
    monkeypatch.delenv("GSLORA_DTYPE", raising=False)
    rec = json.load(open(os.path.join(golden_dir, "driver_args.json")))[driver]
    mod = importlib.import_module("driver_cl" if driver == "driver_probe" else driver)      # driver_probe.main parses with driver_cl.get_args
    assert vars(mod.get_args(rec["argv"])) == rec["args"]


def test_the_baseline_drivers_share_one_trainability_rule():
    import driver_common
    import driver_reg
    assert driver_reg.mark_only_ffn_as_trainable is driver_common.mark_only_ffn_as_trainable
