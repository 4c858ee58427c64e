"""oracle/head_probes.py on the CPU: the f32 emulation of csrc/head.hip's summation order stays under every bound on every table case, every
fault model exceeds a bound or changes an exact output on every case it is named for, the same sums with the lanes reversed (a legal
order) stay under every bound, the exempt ill-conditioned places are exactly the planted ones, and no random ArcFace case has a label
cosine within its own bound of the branch point. tests/test_hip_head_edges.py holds the kernels to the same bounds."""
import numpy as np
import pytest

from oracle import head_probes as P

BIG = {c.name for c in P.TABLE if c.C * c.D > 4_000_000}      # the 64-class weight-gradient tiles at 16449 classes: emulated at one width only
EMULATED = [c for c in P.TABLE if c.name not in BIG or c.name == "wt_d132_c16449"]


def ids(c):
    return c.name


def has_label(case, v):
    return bool((P.labels_of(case) == v).any())


def nwv(case):
    return P.fwd_threads(case.B) // 64


def label_used(case):
    """The kernel of the case reads the labels."""
    return (case.kernel in ("fwd", "logits_t") and not P.is_linear(case.form)) or (P.is_arc(case.form) and not P.opt(case, "de"))


def per_class(case):
    return case.kernel == "wgrad" and not P.wgrad_tile(case)[0]


def wgrad_round(case):
    return 16 * (2 if case.D > 512 else 4)


def phi_differs(case, at=None):
    """The margin changes the logit of some valid label (at: of some label `at`): everywhere but on the lower branch of the easy margin."""
    d = P.make(case)
    lab = d["label"][P.valid_labels(d["label"], case.C)]
    rows = np.ones(len(lab), bool) if at is None else lab == at
    if not P.is_arc(case.form) or not P.arc_constants(case.form).easy:
        return bool(rows.any())
    return bool((P.fwd64(d, case)["above"] & rows).any())


def column0_margin_shows(case):
    """A margin applied at column 0 of an image without a valid label changes something: not on the lower branch of the easy margin
    (phi = cos, d phi = 1), which is where a backward's cos_y = 0 of such an image lies."""
    if not label_used(case) or case.regime == "planted":
        return False
    d = P.make(case)
    bad = ~P.valid_labels(d["label"], case.C)
    if not bad.any():
        return False
    if not (P.is_arc(case.form) and P.arc_constants(case.form).easy):
        return True
    return case.kernel in ("fwd", "logits_t") and bool((P.fwd64(d, case)["cos"][bad, 0] > 0).any())


def dphi_shows(case, rows):
    """d phi / d cos differs from 1 on one of the rows: the label cosine lies on the phi branch."""
    d = P.make(case)
    return bool((rows & (P.dphi64(d["cos_y"], P.arc_constants(case.form)) != 1.0)).any())


def cosine_1d(case):
    return case.D == 1 and not P.is_linear(case.form)      # dW of a cosine head is 0 in one dimension: the projection removes everything


# fault -> the cases it is named for: those whose shape and values reach the changed line
NAMED = {
    "round_last_dropped": lambda c: c.kernel == "fwd" and c.C > 4 * nwv(c),
    "dead_slot_stored": lambda c: c.kernel == "fwd" and not P.is_linear(c.form) and c.C % (5 * nwv(c)) != 0 and phi_differs(c, c.C - 1),
    "label_truncated": lambda c: label_used(c) and has_label(c, 2 ** 32 + 3) and c.C > 3,
    "margin_at_column0": column0_margin_shows,
    "branch_ge": lambda c: c.regime == "planted" or c.name == "fwd_zero_emb_arcface_easy",
    "no_max0": lambda c: c.regime == "planted",
    "no_floor": lambda c: c.regime == "planted",
    "cos_y_after_margin": lambda c: c.kernel in ("fwd", "logits_t") and P.is_arc(c.form) and phi_differs(c),
    "mean_div_tm1": lambda c: c.kernel == "fwd" and c.pool == "mean" and c.T > 1,
    "mean_from_token1": lambda c: c.kernel == "fwd" and c.pool == "mean" and c.T > 1,
    "var_div_dm1": lambda c: c.kernel == "fwd",
    "rstd_no_eps": lambda c: c.kernel == "fwd" and c.regime in ("unit", "zero_emb"),
    "no_projection": lambda c: c.kernel in ("bwd", "de_t") and not P.is_linear(c.form) and not P.opt(c, "de") and c.regime not in ("zero_emb", "tiny_emb", "pow2"),
    "dphi_at_y_and_255": lambda c: c.kernel == "bwd" and P.is_arc(c.form) and not P.opt(c, "de") and dphi_shows(c, (P.labels_of(c) >= 256) & (P.labels_of(c) < c.C)),
    "zero_fill_short": lambda c: c.kernel == "bwd" and c.pool == "cls" and c.T > 1 and not P.opt(c, "compact"),
    "compact_counter": lambda c: c.kernel == "bwd" and P.opt(c, "compact") and P.opt(c, "p0.1"),
    "mean_grad_undivided": lambda c: c.kernel == "bwd" and c.pool == "mean",
    "scale_pow2_off": lambda c: c.regime == "pow2",
    "gscale_inverse": lambda c: P.opt(c, "scaled"),
    "wave15_dropped": lambda c: per_class(c) and c.B >= 16 and not cosine_1d(c),
    "dead_row_contributes": lambda c: per_class(c) and c.B % wgrad_round(c) != 0 and c.regime != "zero_emb" and not cosine_1d(c),
    "zero_w_projected": lambda c: c.regime == "tiny_w",
    "emb_clamp_projected": lambda c: c.regime == "tiny_emb",
    "ktile_tail_not_zeroed": lambda c: (c.kernel == "logits_t" and c.D % 32 != 0) or (c.kernel == "de_t" and c.C % 128 != 0)
                             or (c.kernel == "wgrad_t" and c.B % P.wgrad_tile(c)[1] != 0),
}
PAIRS = [(f, c) for f in P.FAULTS for c in EMULATED if NAMED[f](c)]


def test_every_fault_model_is_named_for_a_case():
    assert set(NAMED) == set(P.FAULTS)
    assert {f for f, _ in PAIRS} == set(P.FAULTS)


@pytest.mark.parametrize("case", EMULATED, ids=ids)
def test_emulation_stays_under_every_bound(case):
    r = P.emulate(P.make(case), case)
    print("EMU", case.name, " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("case", EMULATED, ids=ids)
def test_reversed_lanes_stay_under_every_bound(case):
    """The negative control: the same terms in another legal order. A bound that catches this is too tight to survive the device."""
    r = P.emulate(P.make(case), case, reverse=True)
    print("REV", case.name, " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("fault,case", PAIRS, ids=lambda v: v if isinstance(v, str) else v.name)
def test_fault_models_break_a_bound_or_an_exact_output(fault, case):
    r = P.emulate(P.make(case), case, fault=fault)
    print("FAULT", fault, case.name, " ".join(f"{k}={v:.3g}" for k, v in r.items()))
    assert max(r.values()) > 1.0, r


def test_the_rsqrt_constant_is_twice_what_the_cpu_shows():
    u = P.cpu_rsqrt_ulps()
    print(f"CPU rsqrt {u:.3f} ulp")
    assert 2 * u <= P.U_RSQRT


def test_exempt_places_are_exactly_the_planted_ones():
    for case in P.cases("fwd") + P.cases("logits_t"):
        d = P.make(case)
        got = (P.emulate_fwd if case.kernel == "fwd" else P.emulate_logits_tiled)(d, case)
        _, ill = P.judge_fwd(d, case, got)
        want = np.zeros(case.B, bool)
        if case.regime == "parallel" and P.is_arc(case.form):
            want[0::2] = True      # +e-hat on the even images: cos = 1 on the phi branch; -e-hat falls on the other branch
        assert (ill == want).all(), (case.name, ill)


def test_no_random_arcface_cosine_sits_on_the_branch_point():
    """Inside its own bound of th (or of 0, easy margin) the f32 comparison and the float64 one may differ, and a fault in the compare
    would hide behind that. If this fails, change the seed (the case's name), not the rule."""
    for case in P.TABLE:
        if not P.is_arc(case.form) or case.regime in ("planted", "zero_emb", "zero_w", "tiny_w"):
            continue
        d = P.make(case)
        f = P.fwd64(d, case)
        a = P.arc_constants(case.form)
        ok = P.valid_labels(d["label"], case.C)
        cy = f["cos"][np.arange(case.B)[ok], d["label"][ok]]
        b = P.fwd_bounds(d, case, f)["cos_y"][ok]
        assert (np.abs(cy - (0.0 if a.easy else a.th)) > b).all(), case.name


def test_table_reaches_the_edges_it_names():
    fwd = P.cases("fwd")
    assert {c.D for c in fwd} >= set(P.FWD_D)
    assert {c.C for c in fwd if c.B == 3} >= set(P.FWD_C_1024T) and {c.C for c in fwd if c.B == 129} == set(P.FWD_C_256T)
    assert {(c.T, c.pool) for c in fwd} >= {(T, p) for T in (1, 2, 5) for p in ("cls", "mean")}
    labels = np.concatenate([P.labels_of(c) for c in fwd if c.B == 3 and c.regime == "unit"])
    assert {0, -1, 2 ** 32 + 3} <= set(labels.tolist())
    assert all(v in P.labels_of(P.BY_NAME["fwd_b129_c100"]).tolist() for v in (0, 63, 64, 99, -1, 100, 2 ** 32 + 3))
    bwd = P.cases("bwd")
    assert {c.C for c in bwd if c.B == 6} == {1, 255, 256, 257, 1023, 1024}
    assert {tuple(c.opt.split()[0][2:]) for c in bwd if c.opt.startswith("t_")} | {tuple("fff")} == {tuple(t) for t in P.ROW_TRIPLES}
    wg = [c for c in P.cases("wgrad") if c.regime == "unit"]
    assert {c.C for c in wg} >= {1, 2, 255, 256, 257, 258, 1024, 1025, 1100}
    assert {c.D for c in wg} >= {1, 3, 4, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024}
    assert {c.B for c in wg} >= {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130}
    assert all(not P.wgrad_tile(c)[0] for c in P.cases("wgrad")) and all(P.wgrad_tile(c)[0] for c in P.cases("wgrad_t"))
    assert {(c.D, c.C) for c in P.cases("wgrad_t")} >= {(D, C) for D in (4, 132, 260, 516) for C in (1041, 16449)}


def test_the_planted_power_of_two_maximum_is_exact():
    case = P.BY_NAME["bwd_scaled_pow2"]
    d = P.make(case)
    ref = P.bwd64(d, case)
    assert ref["amax"].tolist() == [4.0, 2.0] and P.loss_scale(4.0) == 256.0 and P.loss_scale(np.nextafter(np.float32(4), np.float32(0))) == 512.0
    got = P.emulate_bwd(d, case)
    assert got["gscale"].tolist() == [256.0, 1.0 / 256.0] and got["dx"][0, 0].tolist() == [1024.0, 0.0, -1024.0, 0.0]


def test_dropout_restatement_keeps_nine_in_ten():
    keep = P.drop_keep(np.arange(1 << 16, dtype=np.uint64), 0.1, *P.DROP_SEED_SITE)
    assert abs(keep.mean() - 0.9) < 0.01 and P.drop_keep(np.arange(8, dtype=np.uint64), 0.0, 1, 2).all()
