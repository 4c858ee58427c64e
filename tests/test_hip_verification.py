"""Face verification on the GPU (util.utils.perform_val, util/verification.py, csrc/verif.hip) against the real reference's results in
tests/golden/verification_small.npz (tools/make_golden_verification.py).

 (1) the metric kernels on the golden's f32 distances: accuracy, best thresholds, tpr, fpr equal the reference's bit for bit (f64);
 (2) perform_val end to end in f32 parity mode: embeddings within the f32 bar (1e-4), xnorm within 1e-4 relative, every distance closer to the
     reference's than half the fixture's smallest distance-to-threshold gap, and THEN every output equal to the reference's;
 (3) the 16-bit evaluation modes: only pairs whose reference distance lies within the measured distance error of a threshold may flip;
 (4) API behaviour: ragged batches, restored model state, uint8 input, the other backbones, argument errors, determinism, the driver."""
import os

import numpy as np
import pytest
import torch

from oracle import recipe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["model", "p603_f10", "p50_f5", "nosame", "ties"]
THRESHOLDS = np.arange(0, 4, 0.01)
N_PAIRS, BATCH = 120, 50


@pytest.fixture(scope="module")
def gold():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    return np.load(os.path.join(ROOT, "tests", "golden", "verification_small.npz"))


def verif_pairs(cfg, n_pairs, seed):      # = tools/make_golden_verification.py
    S = cfg["image_size"]

    def image(ident, k):
        base = recipe.uniform(f"verif_id{ident}", (3, 1, 1), seed, 0.1, 0.9)
        if k:      # the second image of an identity: its colour moved by 0.08 per channel, so that same pairs keep clear of threshold 0
            base = base + 0.08 * np.sign(recipe.uniform(f"verif_twin{ident}", (3, 1, 1), seed, -1.0, 1.0))
        noise = recipe.uniform(f"verif_noise{ident}_{k}", (3, S, S), seed, 0.0, 1.0)
        return np.floor((0.6 * base + 0.4 * noise) * 255.0).clip(0, 255).astype(np.uint8)

    imgs, issame = [], []
    for p in range(n_pairs):
        imgs += [image(p, 0), image(p, 1)] if p % 2 == 0 else [image(p, 0), image(n_pairs + p, 0)]
        issame.append(p % 2 == 0)
    return np.stack(imgs), np.array(issame)


def build_model(dtype="fp32", train=False):
    import loralib as lora
    from vit_pytorch_face import ViT_face
    cfg = recipe.cfg_small2()
    m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                 dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], lora_rank=cfg["lora_rank"])
    m.load_state_dict({k: torch.tensor(v) for k, v in recipe.make_state(cfg).items()})
    lora.mark_only_lora_as_trainable(m)
    return m.to("cuda").set_compute_dtype(dtype).train(train), cfg


def golden_set(gold, cfg):
    """The fixture's pair set as perform_val takes it: [images, flipped images] holding the byte values as floats (load_bin's range)."""
    u8, issame = verif_pairs(cfg, N_PAIRS, int(gold["pair_seed"]))
    assert np.array_equal(issame.astype(np.uint8), gold["issame"])
    x = torch.tensor(u8.astype(np.float32))
    return [x, x.flip(3)], list(issame)


def embed(model, cfg, data_set, batch=BATCH):
    from util.utils import pair_embeddings
    was = model.training
    model.eval()
    try:
        return pair_embeddings("cuda", cfg["dim"], batch, model, data_set)
    finally:
        model.train(was)


# ------------------------------------------------------------------------------------------------------------ (1) the metric kernels
@pytest.mark.parametrize("case", CASES)
def test_metric_kernels_equal_the_reference_bit_for_bit(gold, case):
    from util import verification as V
    d, same, F = gold[f"{case}::dist32"], gold[f"{case}::issame"], int(gold[f"{case}::folds"])
    tpr, fpr, acc, best, _ = V.roc_from_dist(THRESHOLDS, torch.tensor(d).cuda(), same, F)
    for name, got in (("accuracy", acc), ("best_thresholds", best), ("tpr", tpr), ("fpr", fpr)):
        want = gold[f"{case}::{name}"]
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.array_equal(got, want), (case, name, np.abs(got - want).max())


def test_pair_dist_kernel_against_numpy(gold):
    """sum + normalise + squared distance + xnorm on the golden's reference embeddings, f32 kernel against the reference's f64 arithmetic;
    a zero row stays zero (sklearn's rule); the plain form on the normalised embeddings gives the same distances bit for bit."""
    from gslora_hip import ops
    e0, e1 = gold["emb0"].copy(), gold["emb1"].copy()
    e0[6], e1[6] = 0.0, 0.0      # a zero sum row
    e1[9] = -e0[9]               # e0 + e1 = 0 with non-zero norms
    s = e0.astype(np.float64) + e1.astype(np.float64)
    nrm = np.linalg.norm(s, axis=1, keepdims=True)
    nrm[nrm == 0] = 1.0
    n = s / nrm
    want = np.sum(np.square(n[0::2] - n[1::2]), 1)
    xn = (np.linalg.norm(e0.astype(np.float64), axis=1).sum() + np.linalg.norm(e1.astype(np.float64), axis=1).sum()) / (2 * len(e0))
    dist, xnorm, nemb = ops.verif_pair_dist(torch.tensor(e0).cuda(), torch.tensor(e1).cuda(), want_normed=True)
    err = np.abs(dist.cpu().numpy().astype(np.float64) - want).max()
    print(f"pair_dist: max |dist - f64| {err:.3e}, xnorm rel {abs(xnorm.item() - xn) / xn:.3e}")
    assert err < 1e-6 and abs(xnorm.item() - xn) / xn < 1e-6      # f32 sums of 128 terms of magnitude <= 4
    assert np.abs(nemb.cpu().numpy() - n).max() < 1e-6 and not nemb[6].any() and not nemb[9].any()
    assert torch.equal(ops.verif_sq_dist(nemb[0::2], nemb[1::2]), dist)
    dist2, xnorm2, _ = ops.verif_pair_dist(torch.tensor(e0).cuda(), torch.tensor(e1).cuda())
    assert torch.equal(dist2, dist) and torch.equal(xnorm2, xnorm)


# ------------------------------------------------------------------------------------------------------------ (2) end to end, f32
def test_perform_val_f32_equals_the_reference(gold, monkeypatch):
    import engine_cl
    from gslora_hip import ops
    from util import verification as V
    from util.utils import perform_val
    monkeypatch.setattr(engine_cl, "EVAL_DTYPE", "fp32")
    model, cfg = build_model("fp32")
    data_set, issame = golden_set(gold, cfg)
    e0, e1 = embed(model, cfg, data_set)
    e_emb = max((e0.cpu() - torch.tensor(gold["emb0"])).abs().max().item(), (e1.cpu() - torch.tensor(gold["emb1"])).abs().max().item())
    dist, xnorm, nemb = ops.verif_pair_dist(e0, e1, want_normed=True)
    e_dist = np.abs(dist.cpu().numpy().astype(np.float64) - gold["dist"]).max()
    e_xn = abs(xnorm.item() - float(gold["xnorm"])) / float(gold["xnorm"])
    min_gap = float(gold["min_gap"])
    print(f"f32: max |emb - ref| {e_emb:.3e}, max |dist - ref| {e_dist:.3e} (min_gap {min_gap:.3e}), xnorm rel {e_xn:.3e}")
    assert e_emb < 1e-4 and e_xn < 1e-4
    assert min_gap >= 1e-4 and e_dist < min_gap / 2      # the condition under which every decision dist < thr is the reference's
    acc, std, xn, thr, roc = perform_val(False, "cuda", cfg["dim"], BATCH, model, data_set, issame, 10)
    assert acc == float(gold["acc_mean"]) and std == float(gold["acc_std"]) and thr == float(gold["thr_mean"])
    assert abs(xn - float(gold["xnorm"])) / float(gold["xnorm"]) < 1e-4
    assert roc.dtype == torch.float32 and roc.shape == (2, 400)
    assert np.array_equal(roc.numpy(), np.stack([gold["fpr"], gold["tpr"]]).astype(np.float32))
    tpr, fpr, accuracy, best = V.evaluate(nemb, issame, 10)
    for got, name in ((tpr, "tpr"), (fpr, "fpr"), (accuracy, "accuracy"), (best, "best_thresholds")):
        assert np.array_equal(got, gold[name]), name
    for far in ("1e-1", "1e-2"):
        got = np.array(V.calculate_val(THRESHOLDS, nemb[0::2], nemb[1::2], np.asarray(issame), float(far), 10))
        assert np.array_equal(got, gold[f"val_{far}"]), (far, got, gold[f"val_{far}"])
    t = float(gold["best_thresholds"][0])
    d64, same = gold["dist"], np.asarray(issame)
    tp, fp = int(((d64 < t) & same).sum()), int(((d64 < t) & ~same).sum())
    assert V.calculate_accuracy(t, dist, issame) == (tp / same.sum(), fp / (~same).sum(), (tp + (~same).sum() - fp) / len(same))
    assert V.calculate_val_far(t, dist, issame) == (tp / same.sum(), fp / (~same).sum())


# ------------------------------------------------------------------------------------------------------------ (3) 16-bit evaluation
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_perform_val_16bit_modes_flip_only_pairs_near_a_threshold(gold, monkeypatch, dt):
    """A pair may change a decision only if its reference distance lies within the measured max |dist_hip - dist_ref| of a threshold; that set
    must stay below 10 % of the pairs for the fixture to say anything. Measured (MI355X): see profiles/verification.md."""
    import engine_cl
    from gslora_hip import ops
    from util import verification as V
    from util.utils import perform_val
    model, cfg = build_model(dt)
    data_set, issame = golden_set(gold, cfg)
    same = np.asarray(issame)
    e0, e1 = embed(model, cfg, data_set)
    dist = ops.verif_pair_dist(e0, e1)[0]
    d_hip, d_ref = dist.cpu().numpy().astype(np.float64), gold["dist"]
    err = np.abs(d_hip - d_ref).max()
    near = np.abs(d_ref[:, None] - THRESHOLDS[None, :]) <= err      # [P, Tn]: the decisions that may legitimately differ
    may_flip = near.any(1)
    print(f"{dt}: max |dist - ref| {err:.3e}, pairs within that of a threshold {int(may_flip.sum())} / {len(d_ref)}")
    assert may_flip.sum() <= 0.10 * len(d_ref), "fixture unsuitable: too many reference distances near a threshold for this error"
    dec_hip, dec_ref = d_hip[:, None] < THRESHOLDS[None, :], d_ref[:, None] < THRESHOLDS[None, :]
    assert np.array_equal(dec_hip[~near], dec_ref[~near])      # every other decision is the reference's
    # accuracy of the whole set at each of the reference's best thresholds: off by at most the pairs that may flip there
    for t in np.unique(gold["best_thresholds"]):
        ti = int(np.argmin(np.abs(THRESHOLDS - t)))
        ref_acc = float(((dec_ref[:, ti] & same) | (~dec_ref[:, ti] & ~same)).sum()) / len(same)
        got = V.calculate_accuracy(THRESHOLDS[ti], dist, issame)[2]
        assert abs(got - ref_acc) <= near[:, ti].sum() / len(same) + 1e-12, (t, got, ref_acc)
    # perform_val in this evaluation dtype (whatever the model trains in) reports the metric of exactly these distances
    monkeypatch.setattr(engine_cl, "EVAL_DTYPE", dt)
    model.set_compute_dtype("fp32")
    acc, std, xn, thr, roc = perform_val(False, "cuda", cfg["dim"], BATCH, model, data_set, issame, 10)
    assert model.compute_dtype == torch.float32
    tpr, fpr, accuracy, best, _ = V.roc_from_dist(THRESHOLDS, dist, issame, 10)
    assert acc == accuracy.mean() and std == accuracy.std() and thr == best.mean()
    assert np.array_equal(roc.numpy(), np.stack([fpr, tpr]).astype(np.float32))
    assert np.isfinite(xn) and xn > 0


# ------------------------------------------------------------------------------------------------------------ (4) API behaviour
def test_ragged_batches_equal_one_batch_and_calls_repeat_bit_for_bit(gold):
    from util.utils import perform_val
    model, cfg = build_model("fp32")
    data_set, issame = golden_set(gold, cfg)
    a = embed(model, cfg, data_set, batch=BATCH)      # 50 + 50 + 50 + 50 + 40
    b = embed(model, cfg, data_set, batch=240)
    c = embed(model, cfg, data_set, batch=64)         # 64 + 64 + 64 + 48
    for x, y in ((a, b), (a, c)):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    r1 = perform_val(False, "cuda", cfg["dim"], BATCH, model, data_set, issame, 10)
    r2 = perform_val(False, "cuda", cfg["dim"], 240, model, data_set, issame, 10)
    r3 = perform_val(False, "cuda", cfg["dim"], BATCH, model, data_set, issame, 10)
    for r in (r2, r3):
        assert r[:4] == r1[:4] and torch.equal(r[4], r1[4])


def test_model_mode_dtype_and_merge_state_are_restored(gold, monkeypatch):
    import engine_cl
    import loralib as lora
    from util.utils import perform_val
    monkeypatch.setattr(engine_cl, "EVAL_DTYPE", "fp32")
    model, cfg = build_model("fp16", train=True)
    data_set, issame = golden_set(gold, cfg)
    layers = [m for m in model.modules() if isinstance(m, lora.Linear)]
    assert layers and model.training and not any(m.merged for m in layers)
    perform_val(False, "cuda", cfg["dim"], BATCH, model, data_set, issame, 10)
    assert model.training and model.compute_dtype == torch.float16 and not any(m.merged for m in layers)
    model.eval()
    perform_val(False, "cuda", cfg["dim"], BATCH, model, data_set, issame, 10)
    assert not model.training and model.compute_dtype == torch.float16 and all(m.merged for m in layers)

    class Wrapped(torch.nn.Module):      # multi_gpu=True: the model is taken out of its DataParallel-style wrapper
        def __init__(self, module):
            super().__init__()
            self.module = module
    r = perform_val(True, "cuda", cfg["dim"], BATCH, Wrapped(model), data_set, issame, 10)
    assert r[:4] == perform_val(False, "cuda", cfg["dim"], BATCH, model, data_set, issame, 10)[:4]


def test_uint8_pair_set_equals_the_float_one_bit_for_bit(gold):
    from gslora_hip import ops
    from util.utils import perform_val
    model, cfg = build_model("fp32")
    model.set_input_norm("totensor")
    u8, issame = verif_pairs(cfg, N_PAIRS, int(gold["pair_seed"]))
    u = torch.tensor(u8)
    x = ops.u8_reference(u, *ops.INPUT_NORM_TOTENSOR)
    ru = perform_val(False, "cuda", cfg["dim"], BATCH, model, [u, u.flip(3)], list(issame), 10)
    rf = perform_val(False, "cuda", cfg["dim"], BATCH, model, [x, x.flip(3)], list(issame), 10)
    assert ru[:4] == rf[:4] and torch.equal(ru[4], rf[4])
    eu, ef = embed(model, cfg, [u, u.flip(3)]), embed(model, cfg, [x, x.flip(3)])
    assert torch.equal(eu[0], ef[0]) and torch.equal(eu[1], ef[1])


def test_vits_face_and_modified_vit_run(gold):
    import loralib as lora
    from util.utils import perform_val, replace_ffn_with_lora
    from vit_pytorch_face import ViTs_face
    from vit_pytorch_face.modified_VIT import ModifiedViT, vit_b_16
    cfg = recipe.cfg_small2()
    u8, issame = verif_pairs(cfg, 20, 5)
    x = torch.tensor(u8.astype(np.float32) / 255.0)
    torch.manual_seed(0)
    vits = ViTs_face(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                     dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], lora_rank=cfg["lora_rank"],
                     ac_patch_size=12, pad=4)
    lora.mark_only_lora_as_trainable(vits)
    vits = vits.to("cuda").set_compute_dtype("fp32")
    r = perform_val(False, "cuda", cfg["dim"], 16, vits, [x, x.flip(3)], list(issame), 5)
    assert 0.0 <= r[0] <= 1.0 and np.isfinite(r[2]) and r[2] > 0 and r[4].shape == (2, 400)
    c2 = recipe.cfg_vitb_small2()
    vit = vit_b_16(image_size=c2["image_size"], patch_size=c2["patch_size"], num_layers=c2["depth"], num_heads=c2["heads"],
                   hidden_dim=c2["dim"], mlp_dim=c2["mlp_dim"], num_classes=c2["num_class"])
    tv = replace_ffn_with_lora(ModifiedViT(vit), rank=c2["lora_rank"])
    tv.load_state_dict({k: torch.tensor(v) for k, v in recipe.make_tv_state(c2).items()}, strict=True)
    tv = tv.to("cuda").set_compute_dtype("fp32")
    x2 = torch.tensor(recipe.make_images(c2, 40, seed=3, tag="verif_tv"))
    r = perform_val(False, "cuda", c2["dim"], 16, tv, [x2, x2.flip(3)], [p % 2 == 0 for p in range(20)], 5)
    assert 0.0 <= r[0] <= 1.0 and np.isfinite(r[2]) and r[2] > 0
    from util.utils import pair_embeddings
    tv.eval()      # the embedding perform_val takes is forward()'s second output (modified_VIT.py:33)
    with torch.no_grad():
        emb = tv(x2[:4].cuda())[1]
    e0, _ = pair_embeddings("cuda", c2["dim"], 4, tv, [x2[:4], x2[:4].flip(3)])
    assert torch.equal(e0, emb)


def test_argument_errors(gold):
    from util import verification as V
    from util.utils import perform_val
    model, cfg = build_model("fp32")
    data_set, issame = golden_set(gold, cfg)
    small = [data_set[0][:10], data_set[1][:10]]
    with pytest.raises(ValueError, match="greater than the number of samples"):
        perform_val(False, "cuda", cfg["dim"], BATCH, model, small, issame[:5], 10)
    e = torch.zeros(20, 8, device="cuda")
    with pytest.raises(NotImplementedError, match="pca"):
        V.evaluate(e, issame[:10], 5, pca=2)
    with pytest.raises(ValueError, match="greater than the number of samples"):
        V.evaluate(e[:8], issame[:4], 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.evaluate(e.cpu(), issame[:10], 5)


def test_driver_reports_verification_for_every_task(tmp_path):
    import driver_cl
    rep, out, model = driver_cl.main(["--small", "--verify_pairs", "64", "--num_class", "20", "--num_tasks", "2", "--per_forget_cls", "4",
                                      "--epochs", "1", "--batch_size", "16", "--samples_per_class", "4", "--dtype", "fp16",
                                      "--outdir", str(tmp_path)])
    assert len(rep) == 2
    for rec in rep:
        v = rec["verification"]
        assert v["pairs"] == 64 and 0.0 <= v["accuracy"] <= 1.0 and v["xnorm"] > 0 and 0.0 <= v["best_threshold"] < 4.0
    assert model.training
    rep0, _, _ = driver_cl.main(["--small", "--num_class", "20", "--num_tasks", "1", "--per_forget_cls", "4", "--epochs", "1", "--batch_size", "16",
                                 "--samples_per_class", "4", "--dtype", "fp16", "--outdir", str(tmp_path / "off")])
    assert "verification" not in rep0[0]
