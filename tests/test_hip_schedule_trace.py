"""The launch schedule of ViTRunner, pinned call by call (tests/schedule_trace.py says what one event holds): one forward with save=True
and its backward per configuration, on the smallest shapes that reach every form of the adapted linear layer, against the sequence the
runner issued before the adapted-linear step became one helper (tests/golden/schedule_trace_parent.json). Same ops calls, same order,
same arguments, same buffers. A change of the schedule that is meant shows here as the first differing call; the fixture is then
recorded again on the GPU, from the repository root (tools/README.md):
`PYTHONPATH=.:gs-lora_amd python tests/test_hip_schedule_trace.py tests/golden/schedule_trace_parent.json`."""
import json
import os
import sys

import pytest
import torch

from oracle import recipe

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "schedule_trace_parent.json")

# name -> (model configuration, compute dtype, images, dropout, vit_runner knobs, mode)
SMALL2 = recipe.cfg_small2()
CONFIGS = {
    "few_bf16": (SMALL2, "bf16", 3, 0.0, {}, "train"),                                     # in-kernel form on the ring kernel, batched reductions
    "full_bf16": (SMALL2, "bf16", 222, 0.0, {}, "train"),                                  # 8214 rows >= INK_MIN_ROWS: u1c, mulgrad
    "full_unfused": (SMALL2, "bf16", 222, 0.0, {"FUSE_LORA_GRAD": False}, "train"),        # EPI_MUL* in-kernel dX, four separate reductions
    "few_kseg": (SMALL2, "bf16", 3, 0.0, {"INK_SMALL": False}, "train"),                   # skinny GEMM + K segment everywhere, split FFN1-dX
    "few_f32": (SMALL2, "fp32", 3, 0.0, {}, "train"),
    "few_fp16": (SMALL2, "fp16", 3, 0.0, {}, "train"),                                     # gscale through the reductions
    "few_drop": (SMALL2, "bf16", 3, 0.1, {}, "train"),                                     # site / seed / p_drop of every launch
    "rank32": (recipe.cfg_small2(lora_rank=32), "bf16", 3, 0.0, {}, "train"),              # rank > 16: never in-kernel
    "attn_site": (recipe.cfg_small_attn(), "bf16", 3, 0.0, {}, "train"),                   # q / k / v adapters, frozen FFN backward
    "ln_lora": (recipe.cfg_full(), "bf16", 2, 0.0, {"FWD_STREAM": "bf16", "LN_LORA": True}, "train"),
    "two_batches": (SMALL2, "bf16", (2, 1), 0.0, {}, "train"),                             # the fused remain / forget forward
    "eval_merged": (SMALL2, "bf16", 3, 0.0, {}, "eval"),                                   # merged weights: no adapter launches
}


def build(cfg, dtype, dropout):
    import loralib as lora
    from vit_pytorch_face import ViT_face
    m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                 dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], dropout=dropout, emb_dropout=dropout,
                 lora_rank=cfg["lora_rank"], lora_pos=cfg.get("lora_pos", "FFN"))
    m.load_state_dict({k: torch.tensor(v) for k, v in recipe.make_state(cfg).items()}, strict=True)
    lora.mark_only_lora_as_trainable(m)
    return m.to("cuda").set_compute_dtype(dtype)


def trace(name, setknob):
    """The events of configuration `name`. setknob(module, attribute, value) sets a vit_runner knob (monkeypatch.setattr in the test)."""
    from gslora_hip import vit_runner
    from schedule_trace import ScheduleTrace
    cfg, dtype, images, dropout, knobs, mode = CONFIGS[name]
    for k, v in knobs.items():
        setknob(vit_runner, k, v)
    torch.manual_seed(0)
    m = build(cfg, dtype, dropout)
    m = m.train() if mode == "train" else m.eval()
    parts = images if isinstance(images, tuple) else (images,)
    n = sum(parts)
    x = torch.tensor(recipe.make_images(cfg, n)).cuda()
    y = torch.tensor(recipe.make_labels(cfg, n)).cuda()
    img = x if len(parts) == 1 else tuple(x.split(list(parts)))
    r = m.runner()
    with ScheduleTrace() as t:
        t.hook(r)
        if mode == "eval":
            with torch.no_grad():
                r.forward(img, y, save=False)
        else:
            logits, emb, saved = r.forward(img, y, save=True)
            r.backward(saved, torch.ones_like(logits), torch.ones_like(emb))
        torch.cuda.synchronize()
    return t.events


def dump(traces, path):
    """One compact line per call."""
    with open(path, "w") as f:
        f.write("{\n")
        for k, (name, events) in enumerate(traces.items()):
            f.write(json.dumps(name) + ": [\n")
            f.write(",\n".join(json.dumps(e, separators=(",", ":")) for e in events))
            f.write("\n]" + ("," if k + 1 < len(traces) else "") + "\n")
        f.write("}\n")


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_schedule_is_the_recorded_one(name, recorded, monkeypatch):
    got = json.loads(json.dumps(trace(name, monkeypatch.setattr)))      # (tuples -> lists, as the fixture went through JSON)
    want = recorded[name]
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            print(f"{name}: first differing call is #{k}\n  recorded: {json.dumps(w)}\n  now:      {json.dumps(g)}")
            for j in range(max(0, k - 3), k):
                print(f"  (#{j} before it: {json.dumps(want[j])})")
        assert g == w, f"{name}: call #{k} differs from the recorded schedule"
    if len(got) != len(want):
        extra = (got if len(got) > len(want) else want)[min(len(got), len(want))]
        pytest.fail(f"{name}: {len(got)} calls, {len(want)} recorded; the first call beyond the shorter list: {json.dumps(extra)}")


if __name__ == "__main__":      # record the fixture (the module docstring has the command line)
    from gslora_hip import vit_runner as R
    out = {}
    for cname, (_, _, _, _, knobs, _) in CONFIGS.items():
        before = {k: getattr(R, k) for k in knobs}
        try:
            out[cname] = trace(cname, setattr)
        finally:
            for k, v in before.items():
                setattr(R, k, v)
        print(f"{cname}: {len(out[cname])} calls")
    dump(out, sys.argv[1])
