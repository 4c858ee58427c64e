"""The reference and the probes of tests/test_hip_large_rows.py, proven on the CPU before a GPU sees them.

 1. tests/large_row_reference.py against the oracle: its float64 LoRA gradients are those of oracle.gslora_oracle.vit_forward + autograd in
    float64 (batch 3 and batch 222, pool 'cls' and 'mean', adapters on the FFN and on q / k / v); its row-by-row restatement of the four
    reductions of a block sums to the autograd gradient; the float32 CPU oracle stays within 1e-6 relative Frobenius per tensor of the
    float64 one (so float64 is a reference for float32 kernels, and float32 autograd a yardstick for them), no tensor of zero norm.
 2. Fault model: what the placement probes must be able to see. The probe image sits at position 221 of batch 222 (rows 8177 .. 8213, so
    row 8192 is its token 15); on the reductions of blocks 0 and 1, four faults a tiled kernel can commit — the last token row dropped,
    every row from 8192 on dropped, row 8191 counted twice, U read one row late — each move EVERY one of the eight tensors by more than 5e-3
    relative Frobenius (asked: at least one; the placement test bounds every tensor, so every tensor has to discriminate). 5e-3 is a
    condition on the probe, five times the 1e-3 cap of the placement test, not a tolerance of a kernel.
    Measured on the least-affected tensor: last row dropped 7.5e-3, row 8191 twice 8.1e-3, rows from 8192 on 0.10, U one row late 1.0.
 3. Placement bound: float32 sums of the same 37 addends in two different row orders differ elementwise by at most
    2.2 * 37 * 2^-24 * sum|addends| (each order is within (N - 1) u sum|addends| of the exact sum, u = 2^-24; the factor 1.1 pays for
    addends that are themselves 16-bit-rounded values). This is the bound tests/test_hip_large_rows.py holds the kernels to."""
import numpy as np
import pytest
import torch

import large_row_reference as LR
from oracle import gslora_oracle as O
from oracle import recipe

CFG = recipe.cfg_small2()
T = 37
PROBE_BATCH, PROBE_POS = 222, 221      # rows 8177 .. 8213: the image that straddles row 8192
FAULT_FLOOR = 5e-3


def _oracle_grads(cfg, img, label, dlogits, demb, dtype):
    st = O.to_torch(recipe.make_state(cfg), requires_grad_lora=True, dtype=dtype)
    logits, emb = O.vit_forward(st, torch.tensor(img), torch.tensor(label), cfg, dtype=dtype)
    names = [k for k in st if "lora_" in k]
    loss = (logits * torch.tensor(dlogits).to(dtype)).sum() + (emb * torch.tensor(demb).to(dtype)).sum()
    return {k: g.numpy().astype(np.float64) for k, g in zip(names, torch.autograd.grad(loss, [st[k] for k in names]))}


def _batch(cfg, b):
    return (recipe.make_images(cfg, b), recipe.make_labels(cfg, b)) + LR.upstream(cfg, b)


@pytest.fixture(scope="module")
def ref222():
    """(helper float64, oracle float64) gradients at batch 222 under the seeded upstream."""
    args = _batch(CFG, 222)
    return LR.lora_gradients(CFG, *args)[0], _oracle_grads(CFG, *args, torch.float64)


@pytest.mark.parametrize("variant", ["cls", "mean", "attention", "rank17"])
def test_helper_equals_oracle_f64_batch3(variant):
    cfg = {"cls": CFG, "mean": dict(CFG, pool="mean"), "attention": recipe.cfg_small_attn(), "rank17": recipe.cfg_small2(lora_rank=17)}[variant]
    args = _batch(cfg, 3)
    got, want = LR.lora_gradients(cfg, *args)[0], _oracle_grads(cfg, *args, torch.float64)
    assert sorted(got) == sorted(want) and len(got) == (6 if variant == "attention" else 12)
    for k in want:
        assert np.linalg.norm(want[k]) > 0, k
        assert LR.rel_fro(got[k], want[k]) < 1e-12, (k, LR.rel_fro(got[k], want[k]))


def test_helper_equals_oracle_f64_batch222(ref222):
    got, want = ref222
    for k in want:
        assert np.linalg.norm(want[k]) > 0, k
        assert LR.rel_fro(got[k], want[k]) < 1e-12, (k, LR.rel_fro(got[k], want[k]))


def test_f32_cpu_autograd_within_1e6_of_f64():
    """Batch 222 under a cross-entropy loss, handed over as its upstream dlogits = (softmax - onehot) / B, demb = 0. Measured here: 0.8e-7 ..
    3.3e-7 per tensor (under the seeded random upstream of the GPU tests, whose rows cancel more: 2.9e-7 .. 6.3e-7, and up to 1.3e-6 with
    another CPU's BLAS - which is why the GPU test of the float32 modes measures this error itself instead of assuming it)."""
    img, lab, _, demb = _batch(CFG, 222)
    with torch.no_grad():
        logits, _ = O.vit_forward(O.to_torch(recipe.make_state(CFG), dtype=torch.float64), torch.tensor(img), torch.tensor(lab), CFG, dtype=torch.float64)
    dlogits = torch.softmax(logits, 1)
    dlogits[torch.arange(222), torch.tensor(lab)] -= 1
    args = (img, lab, (dlogits / 222).float().numpy(), np.zeros_like(demb))
    f64, f32 = _oracle_grads(CFG, *args, torch.float64), _oracle_grads(CFG, *args, torch.float32)
    helper = LR.lora_gradients(CFG, *args)[0]
    assert len(f64) == 12
    for k in f64:
        assert np.linalg.norm(f64[k]) > 0, k      # no case skipped
        assert LR.rel_fro(helper[k], f64[k]) < 1e-12, k
        e = LR.rel_fro(f32[k], f64[k])
        print(f"{k}: norm {np.linalg.norm(f64[k]):.3e}  f32 CPU vs f64 {e:.2e}")
        assert e < 1e-6, (k, e)


def test_row_restatement_sums_to_autograd():
    """The reductions of the three images of a batch, restated row by row, add up to the autograd gradient of the batch (twelve tensors);
    so do the 37 rows of the probe image alone."""
    args = _batch(CFG, 3)
    total = None
    for b in range(3):
        grads, ops = LR.lora_gradients(CFG, *args, image=b)
        part = {k: LR.reduce_rows(*v).numpy() for k, v in ops.items()}
        total = part if total is None else {k: total[k] + part[k] for k in part}
    assert sorted(total) == sorted(grads)
    for k in grads:
        assert LR.rel_fro(total[k], grads[k]) < 1e-12, k
    grads, ops = LR.lora_gradients(CFG, *LR.probe(CFG, PROBE_BATCH), image=0)
    for k in grads:
        assert np.linalg.norm(grads[k]) > 0, k
        assert LR.rel_fro(LR.reduce_rows(*ops[k]).numpy(), grads[k]) < 1e-12, k
        assert (LR.abs_addends(*ops[k]) >= np.abs(grads[k]) * (1 - 1e-12)).all(), k


def _faults():
    """name -> (rows summed, row of U each reads) in token indices of the probe image at PROBE_POS; global row = PROBE_POS * T + token."""
    base = PROBE_POS * T
    assert base < 8191 < 8192 < base + T - 1
    rows = np.arange(T)
    t8192 = 8192 - base
    return {
        "last token row dropped": (rows[:-1], rows[:-1]),
        "rows from 8192 on dropped": (rows[:t8192], rows[:t8192]),
        "row 8191 counted twice": (np.concatenate([rows, [t8192 - 1]]), np.concatenate([rows, [t8192 - 1]])),
        "U read one row late": (rows, (rows + 1) % T),      # (the row behind the image's last is the next image's cls row: here its own)
    }


def test_fault_model_reaches_every_tensor_of_blocks_0_and_1():
    grads, ops = LR.lora_gradients(CFG, *LR.probe(CFG, PROBE_BATCH), image=0)
    names = [n for i in (0, 1) for n in LR.ffn_names(i).values()]
    weakest = {}
    for fault, (rows, u_rows) in _faults().items():
        moved = {}
        for k in names:
            Y, U, tr = ops[k]
            moved[k] = LR.rel_fro(LR.reduce_rows(Y, U, tr, rows, u_rows).numpy(), grads[k])
        weakest[fault] = min(moved.values())
        print(f"{fault}: " + "  ".join(f"{k.split('layers.')[1].replace('.1.fn.fn.net', '')} {v:.3e}" for k, v in moved.items()))
        assert max(moved.values()) > FAULT_FLOOR, fault      # what the probe design is asked for
        assert min(moved.values()) > FAULT_FLOOR, (fault, moved)      # and what a per-tensor bound needs
    print("least-affected tensor per fault: " + ", ".join(f"{f}: {v:.3e}" for f, v in weakest.items()))


def _f32_sum(Y, U, order, split=None):
    """float32 accumulation of the outer products Y[m]^T U[m] in the given row order; split: two partial sums (rows before / from it)."""
    Y, U = Y.float(), U.float()
    acc = [torch.zeros(Y.shape[1], U.shape[1]), torch.zeros(Y.shape[1], U.shape[1])]
    for m in order:
        acc[int(split is not None and m >= split)] += torch.outer(Y[m], U[m])
    return (acc[0] + acc[1]).double().numpy()


@pytest.mark.parametrize("round16", [None, torch.bfloat16, torch.float16])
def test_placement_bound_covers_two_row_orders(round16):
    """Sequential, reversed, shuffled, and split-at-a-tile-border float32 sums of the probe's addends (as they are, and with the operands
    rounded to a 16-bit format first, as the kernels hold them) against each other: within 2.2 N 2^-24 sum|addends| of the float64 helper."""
    _, ops = LR.lora_gradients(CFG, *LR.probe(CFG, PROBE_BATCH), image=0)
    rng = np.random.default_rng(0)
    orders = [(list(range(T)), None), (list(range(T))[::-1], None), (list(rng.permutation(T)), None), (list(range(T)), 8192 - PROBE_POS * T),
              (list(rng.permutation(T)), 9)]
    worst = 0.0
    for i in (0, 1):
        for k in LR.ffn_names(i).values():
            Y, U, tr = ops[k]
            bound = 2.2 * T * 2.0 ** -24 * LR.abs_addends(Y, U, False)
            if round16 is not None:
                Y, U = Y.to(round16).double(), U.to(round16).double()
            sums = [_f32_sum(Y, U, o, s) for o, s in orders]
            for s in sums[1:]:
                d = np.abs(s - sums[0])
                worst = max(worst, float((d / bound).max()))
                assert (d <= bound).all(), (k, float((d / bound).max()))
    print(f"worst |difference| / bound over the orders ({round16}): {worst:.3f}")
