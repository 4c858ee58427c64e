"""CPU side of the model geometry sweep (tests/geometry_cases.py; the GPU side is tests/test_hip_geometry_sweep.py).

 (1) The reference is right at every row: LR.forward in float64 equals oracle.gslora_oracle.vit_forward in float64 on logits and emb to
     float64 rounding, every LoRA tensor's reference gradient is non-zero, and the float32 CPU run differs from float64 on every tensor
     (e_cpu > 0: the float32 bound of the GPU file is a product with it).
 (2) The table covers the ladder: gsl_layernorm_fwd is probed at every multiple of 64 up to 1024 (as tests/test_row_host_side_host.py gets
     its refusals: the address 16, no device); the widths it does not refuse are exactly the widths of the table. A width added to
     ln_for_width fails this test until the table has a row for it.
 (3) Fault models, the recorded reason the sweep exists. Six wrong computations (geometry_cases.FAULTS), each applied in float64 to a copy of
     the reference forward that is bit-identical to it without a fault. Each moves a LoRA gradient of a new case by more than 100 x that
     case's float32 bound and more than the bf16 band, and leaves the gradients of the fixtures the suite had before unmoved where the
     arithmetic says so: (a) at cfg_small (dim == dim_head), (b) at rank 8, (d) below 13 heads, (e) up to 512 columns, (f) from depth 2 on.
     (e) at width 768 is not unmoved — the statistics would miss 256 columns — and no ViT_face fixture had that width: d768_odd is one of
     the rows that show it."""
import numpy as np
import pytest
import torch

import geometry_cases as G
import large_row_reference as LR
from oracle import gslora_oracle as O
from oracle import recipe
from test_hip_bf16_pinned import GRAD_BAND
from test_hip_large_rows import C_F32

F64_ROUNDING = 1e-12
UNMOVED = 1e-12       # a fault that is the same arithmetic up to the order of a float64 sum


@pytest.mark.parametrize("name", list(G.CASES))
def test_reference_equals_the_oracle_and_every_gradient_is_live(name):
    cfg, B = G.CASES[name]
    img, label, _, _ = G.inputs(cfg, B)
    assert cfg["heads"] * 64 == cfg["dim"] and cfg["dim_head"] == 64 and G.tokens(cfg) in (2, 5, 10)
    ref = G.reference(name)
    with torch.no_grad():
        logits, emb = O.vit_forward(O.to_torch(recipe.make_state(cfg), dtype=torch.float64), torch.as_tensor(img), torch.as_tensor(label), cfg,
                                    dtype=torch.float64)
    assert LR.rel_fro(ref["logits"], logits.numpy()) <= F64_ROUNDING and LR.rel_fro(ref["emb"], emb.numpy()) <= F64_ROUNDING
    assert ref["logits"].shape == (B, cfg["num_class"]) and ref["emb"].shape == (B, cfg["dim"])
    per_block = 2 if cfg.get("lora_pos") == "Attention" else 4
    assert len(ref["grads"]) == per_block * cfg["depth"]
    for k, g in ref["grads"].items():
        assert np.linalg.norm(g) > 0, k
    e_cpu = G.cpu_errors(name)
    assert set(e_cpu) == set(ref["grads"]) | {"logits", "emb"}
    for k, e in e_cpu.items():
        assert 0 < e < 1e-5, (k, e)
    print(f"[{name}] e_cpu {min(e_cpu.values()):.2e} .. {max(e_cpu.values()):.2e}, smallest gradient norm "
          f"{min(np.linalg.norm(g) for g in ref['grads'].values()):.3g}")


@pytest.mark.parametrize("name", ["d256_min", "d1024_attn", "d256_odd"])
def test_the_fault_free_copy_is_the_reference_forward_bit_for_bit(name):
    cfg, B = G.CASES[name]
    img, label, _, _ = G.inputs(cfg, B)
    st = LR.state(cfg)
    with torch.no_grad():
        a = G.forward_with_fault(st, torch.as_tensor(img), torch.as_tensor(label), cfg)
        b = LR.forward(st, torch.as_tensor(img), torch.as_tensor(label), cfg)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    got = G.fault_gradients(cfg, B, None)
    for k, g in G.reference(name)["grads"].items():
        assert np.array_equal(got[k], g), k


# ---------------------------------------------------------------------------------------------------------------- (2)
LN_FWD = dict(x=16, x_row_stride=128, gamma=16, beta=16, eps=1e-5, y=16, mean=16, rstd=16, M=5, D=128, dtype=0, x_dtype=0, stream=None)
UNSUPPORTED = -3


@pytest.mark.skipif(torch.cuda.is_available(), reason="build-machine test: at a supported width the probe is a launch on the address 16")
def test_the_table_has_exactly_the_widths_the_library_runs():
    from gslora_hip import _lib
    L = _lib.load()
    assert len(LN_FWD) == len(_lib.SIGNATURES["gsl_layernorm_fwd"])
    runs = []
    for D in range(64, 1025, 64):
        rc = L.gsl_layernorm_fwd(*dict(LN_FWD, D=D, x_row_stride=D).values())
        err = L.gsl_last_error().decode()
        if rc == UNSUPPORTED:
            assert err == f"gsl_layernorm_fwd: unsupported LayerNorm width {D}", err
        else:      # every check passed and the launch found no device
            assert rc != 0 and "argument check" not in err and "unsupported" not in err, (D, rc, err)
            runs.append(D)
    assert len(runs) >= 6
    in_table = sorted({cfg["dim"] for cfg, _ in G.CASES.values()})
    assert in_table == runs, f"the library runs the widths {runs}, the table has rows for {in_table}"


def test_the_table_reaches_what_the_sweep_is_for():
    cases = G.CASES
    get = lambda key, default=None: {cfg.get(key, default) for cfg, _ in cases.values()}
    assert 1 in get("depth") and {2, 5, 10} == {G.tokens(cfg) for cfg, _ in cases.values()} and 1 in {B for _, B in cases.values()}
    assert {1, 2, 3, 5, 7} <= get("lora_rank") and {192, 320} <= get("mlp_dim") and 1 in get("channels")
    assert {64, 256} <= {cfg["channels"] * cfg["patch_size"] ** 2 for cfg, _ in cases.values()}
    assert {4, 16} <= get("heads") and {"cls", "mean"} == get("pool", "cls") and {"FFN", "Attention"} == get("lora_pos", "FFN")
    for name, (cfg, B) in cases.items():
        if cfg.get("lora_pos") == "Attention":
            assert 3 * cfg["lora_rank"] <= 64, name
    assert 3 * cases["d1024_attn"][0]["lora_rank"] == 63
    assert max(B * G.tokens(cfg) for cfg, B in cases.values() if cfg["dim"] in (256, 1024)) >= 64      # the float32 tile rule's other side
    # d256_batchable: all four FFN reductions of a block contract tensors whose width is a multiple of 256; d256_odd / d768_odd: two do not
    for name, all_batchable in (("d256_batchable", True), ("d256_odd", False), ("d768_odd", False)):
        cfg = cases[name][0]
        assert (cfg["dim"] % 256 == 0 and cfg["mlp_dim"] % 256 == 0) == all_batchable and cfg["dim"] % 256 == 0


# ---------------------------------------------------------------------------------------------------------------- (3)
# fault -> the new cases it is shown on, chosen by what the fault touches: a width other than 64, a rank other than 8, the last head, a 13th
# head, a 513th column, depth 1. (e) is the weak one: statistics over 512 of 768 or 1024 like columns are close to the row's, and the
# gradients move by 2 % .. 6 % — 7e3 x the float32 bound and above the fp16 band (1 %) at every wide row, above the bf16 band (6 %) at
# d1024_attn alone (measured over all five rows wider than 512 after d768_odd and d1024_min, the first choice, stayed below it). (f) likewise:
# one block's attention output is a small part of the stream, the five depth-1 rows move by 2 % .. 10 %, above the bf16 band at min64 alone.
SHOWN_ON = {"a": ("d256_min", "d1024_t2"), "b": ("d256_min", "d768_odd"), "c": ("d256_min", "d1024_min"), "d": ("d1024_min", "d1024_t2"),
            "e": ("d768_odd", "d1024_attn"), "f": ("d256_min", "d512_min", "min64")}
# fault -> the earlier fixtures it cannot move, and new rows on the same side of the rule
HIDDEN_ON = {"a": ("cfg_small", "min64"), "b": ("cfg_small2", "cfg_full", "d256_batchable"), "d": ("cfg_small", "cfg_small2", "cfg_full", "d768_odd"),
             "e": ("cfg_small", "cfg_small2", "cfg_full"), "f": ("cfg_small", "cfg_small2", "d768_odd")}
_TRUE = {}


def _case(name):
    return G.CASES[name] if name in G.CASES else G.OLD_FIXTURES[name]


def _true_gradients(name):
    if name not in _TRUE:
        _TRUE[name] = G.reference(name)["grads"] if name in G.CASES else G.fault_gradients(*_case(name), None)
    return _TRUE[name]


def _moved(name, fault):
    true, faulty = _true_gradients(name), G.fault_gradients(*_case(name), fault)
    return {k: LR.rel_fro(faulty[k], true[k]) for k in true}


@pytest.mark.parametrize("fault", list(G.FAULTS))
def test_fault_is_far_above_the_bounds_on_a_new_case(fault):
    """On every case of SHOWN_ON the fault moves a tensor by more than 100 x the case's float32 bound C_F32 max_t e_cpu(t) and more than the
    fp16 band; on at least one of them by more than the bf16 band too."""
    above_bf16 = 0
    for name in SHOWN_ON[fault]:
        bar32 = 100 * C_F32 * max(G.cpu_errors(name).values())
        moved = _moved(name, fault)
        worst = max(moved, key=moved.get)
        print(f"[fault {fault} on {name}] moves {worst.split('layers.')[1]} by {moved[worst]:.3g} = {moved[worst] / bar32 * 100:.3g} x the float32 "
              f"bound; {sum(v > GRAD_BAND['bf16'][0] for v in moved.values())} of {len(moved)} tensors above the bf16 band")
        assert moved[worst] > max(bar32, GRAD_BAND["fp16"][0]), (name, worst, moved[worst], bar32)
        above_bf16 += moved[worst] > max(bar32, GRAD_BAND["bf16"][0])
    assert above_bf16 >= 1, G.FAULTS[fault]


@pytest.mark.parametrize("fault", list(HIDDEN_ON))
def test_fault_is_invisible_on_the_earlier_fixtures(fault):
    for name in HIDDEN_ON[fault]:
        cfg = _case(name)[0]
        assert {"a": cfg["dim"] == cfg["dim_head"], "b": cfg["lora_rank"] == 8, "d": cfg["heads"] <= G.WRAP_HEADS,
                "e": cfg["dim"] <= G.STAT_COLUMNS, "f": cfg["depth"] > 1}[fault], name
        moved = _moved(name, fault)
        assert max(moved.values()) <= UNMOVED, (name, moved)
