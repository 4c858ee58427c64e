"""oracle/loss_probes.py on the CPU: the f32 emulation of csrc/loss.hip's summation order stays under every bound on every table case, every
fault model exceeds a bound or changes an exact output on every case it is named for, the table reaches what its cases are named for, and
the float32 restatement of the scalar tail agrees with the float64 one. tests/test_hip_loss_edges.py holds the kernels to the same bounds."""
import numpy as np
import pytest

from oracle import loss_probes as P

K_CE, K_PROTO = 0.37, -1.3
SMALL = [c for c in P.TABLE if c.name != "big"]            # "big" (1027 x 2049) is the device's determinism case; its rows are of the kinds below


def ids(c):
    return c.name


def ce_ratios(d, em):
    x, y = d["x"], d["y"]
    ref = P.ce(x, y, K_CE)
    b_loss = P.bound_loss(x, y)
    out = dict(lse=P.ratio(em["lse"], ref["lse"], P.bound_lse(x)), loss=P.ratio(em["loss"], ref["loss"], b_loss))
    if "g" in em:
        out["dlogits"] = P.ratio(em["g"], ref["g"], P.bound_dlogits(x, y, K_CE))
    out["sum"] = P.ratio(P.emulate_sum(em["loss"]), ref["loss"].sum(), P.bound_sum(ref["loss"], b_loss))
    out["hit"] = float((em["hit"] != ref["hit"]).sum())
    return out


@pytest.mark.parametrize("case", SMALL, ids=ids)
def test_emulation_stays_under_every_bound(case):
    d = P.make(case)
    r = ce_ratios(d, P.emulate_ce(d["x"], d["y"], K_CE))
    a, t, py = d["a"], d["t"], d["py"]
    rk, ek = P.kl(a, t, py, K_PROTO), P.emulate_kl(a, t, py, K_PROTO)
    r2, e2 = P.l2(a, t, py, K_PROTO), P.emulate_l2(a, t, py, K_PROTO)
    r.update(kl=P.ratio(ek["row"], rk["row"], P.bound_kl(a, t, py)), demb_kl=P.ratio(ek["g"], rk["g"], P.bound_demb_kl(a, t, py, K_PROTO)),
             l2=P.ratio(e2["row"], r2["row"], P.bound_l2(a, t, py)), demb_l2=P.ratio(e2["g"], r2["g"], P.bound_demb_l2(a, t, py, K_PROTO)),
             kl_sum=P.ratio(P.emulate_sum(ek["row"]), rk["row"].sum(), P.bound_sum(rk["row"], P.bound_kl(a, t, py))),
             l2_sum=P.ratio(P.emulate_sum(e2["row"]), r2["row"].sum(), P.bound_sum(r2["row"], P.bound_l2(a, t, py))))
    print("EMU", case.name, " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    assert r.pop("hit") == 0
    assert max(r.values()) <= 1.0, r


def test_the_exp_log_constants_are_twice_what_the_cpu_shows():
    e, l = P.cpu_exp_log_ulps()
    print(f"CPU exp {e:.3f} ulp, log {l:.3f} ulp")
    assert 2 * e <= P.U_EXP and 2 * l <= P.U_LOG


# ---------------------------------------------------------------------------------------------------------------- the table is what it says
def test_table_covers_the_widths_rows_and_regimes():
    assert {c.n for c in P.TABLE if c.B == 5 and c.regime == "unit"} == set(P.WIDTHS)
    assert {c.B for c in P.TABLE if c.n == 65} == set(P.ROWS)
    assert {c.regime for c in P.TABLE} == set(P.REGIMES) | {"unit"}
    assert all(P.cp_of(n) != n for n in P.WIDTHS) and {P.cp_of(n) < n for n in P.WIDTHS} == {True, False}      # Cp != C, both directions


@pytest.mark.parametrize("case", SMALL, ids=ids)
def test_cases_reach_what_they_are_named_for(case):
    d = P.make(case)
    x, y, n = d["x"], d["y"], case.n
    r = np.arange(case.B)
    assert ((0 <= y) & (y < n)).all() and ((0 <= d["py"]) & (d["py"] < P.cp_of(n))).all()
    want = {P.place(p, n) for p in P.POS[:max(1, min(4, case.B))]}
    if case.regime in ("unit", "plus1e4", "minus1e4", "spread200", "neginf"):
        assert set(y.tolist()) == want and (x.argmax(1) == d["mpos"]).all() and set(d["mpos"].tolist()) <= {P.place(p, n) for p in P.POS}
        if case.B >= 8:
            assert set(d["mpos"].tolist()) == {P.place(p, n) for p in P.POS}
            hit = P.ce(x, y)["hit"]
            assert 0 < hit.sum() < case.B                    # both outcomes of top-1
    if case.regime == "plus1e4":
        assert x.min() > 9e3
    if case.regime == "minus1e4":
        assert x.max() < -9e3
    if case.regime == "spread200":
        e = np.exp((x - x.max(1, keepdims=True)).astype(np.float32))
        assert ((e > 0).sum(1) == 1).all()                   # every exp but one underflows to zero in f32
    if case.regime == "cosface":
        loss = P.ce(x, y)["loss"]
        assert np.abs(x).max() <= 64 and (x.argmax(1) == y).all() and loss.max() < 2e-2 and loss.min() > 0
    if case.regime == "neginf":
        assert np.isinf(x).any() and np.isfinite(x[r, y]).all() and np.isfinite(P.ce(x, y)["loss"]).all()
    if case.regime in ("tie_lane", "tie_cross"):
        f, s = d["first"], d["second"]
        assert (x[r, f] == x[r, s]).all() and (x.max(1) == x[r, f]).all() and ((x == x.max(1, keepdims=True)).sum(1) == 2).all()
        same_lane = (f % 64) == (s % 64)
        assert same_lane.all() if case.regime == "tie_lane" else (~same_lane).all()
        if case.regime == "tie_cross":
            assert ((s - f) == 3).any() and ((s - f) == 67).any()      # the same pass, and another pass of another lane
        assert (y == f).any() and (y == s).any() and (P.ce(x, y)["hit"] == (y == f)).all()
    if case.regime == "ints":
        ks = (1, 2, 5, 16)
        srt = -np.sort(-x, 1)
        assert all((srt[:, k - 1] == srt[:, k]).any() for k in ks)      # ties at the k-th place


def test_the_zero_hinge_is_exactly_zero():
    name, s, n_r, n_f, h = P.TAIL_GRID[2]
    assert name == "zero" and np.float32(h.BND) - np.float32(s.ce_f) / np.float32(n_f) == 0 and np.float32(h.BND_pro) - np.float32(s.kl_f) / np.float32(n_f) == 0
    total, meters, coefs = P.tail32(s, n_r, n_f, None, h)
    assert meters[0] == 0 and meters[6] == 0 and coefs[1] == 0 and coefs[2] == 0
    hinges = {nm: (h.BND - s.ce_f / n_f, h.BND_pro - s.kl_f / n_f) for nm, s, n_r, n_f, h in P.TAIL_GRID}
    assert min(hinges["active"]) > 0 and max(hinges["inactive"]) < 0 and min(hinges["odd_sizes"]) > 0


# ---------------------------------------------------------------------------------------------------------------- the scalar tail
@pytest.mark.parametrize("has_proto", [True, False])
@pytest.mark.parametrize("structure", [None, P.STRUCTURE])
@pytest.mark.parametrize("row", P.TAIL_GRID, ids=lambda r: r[0])
def test_tail32_agrees_with_tail64(row, structure, has_proto):
    """Within 4 ulps of the largest magnitude an output is made of (bound_tail's 8 E): a check of the restatement itself."""
    name, s, n_r, n_f, h = row
    t32, t64 = P.tail32(s, n_r, n_f, structure, h, has_proto), P.tail64(s, n_r, n_f, structure, h, has_proto)
    b = P.bound_tail(s, n_r, n_f, structure, h, has_proto)
    for what, g, ref, bd in zip(("total", "meters", "coefs"), t32, t64, b):
        assert P.ratio(g, ref, bd) <= 1.0, (name, what, g, ref)
    if not has_proto:
        assert t64[1][6] == h.w_f * max(h.BND_pro, 0.0) and t64[1][7] == 0                # logged, and absent from the total
        st = 0.0 if structure is None else structure
        assert abs(t64[0] - (h.beta * max(h.BND - s.ce_f / n_f, 0.0) + s.ce_r / n_r + h.alpha * st)) < 1e-12
        assert (t64[2][2:4] == 0).all()


def test_tail_keeps_a_nan_forget_sum():
    name, s, n_r, n_f, h = P.TAIL_GRID[0]
    for bad in (s._replace(ce_f=np.nan), s._replace(kl_f=np.nan)):
        for tail in (P.tail32, P.tail64):
            total, meters, coefs = tail(bad, n_r, n_f, None, h)
            assert np.isnan(total) and np.isnan(meters[2]) and np.isfinite(meters[1]) and np.isfinite(coefs).all()


# ---------------------------------------------------------------------------------------------------------------- fault models
def cases_of(fault):
    names = P.FAULT_CASES[fault]
    assert names, fault
    return [P.BY_NAME[n] for n in names]


def exceeds(r):
    r = dict(r)
    return r.pop("hit", 0) > 0 or max(r.values()) > 1.0


@pytest.mark.parametrize("fault,fn", [("last_element_dropped", P.fault_last_element_dropped), ("pass17_dropped", P.fault_pass17_dropped),
                                      ("no_max_subtraction", P.fault_no_max_subtraction), ("label_off_by_one", P.fault_label_off_by_one),
                                      ("row_stride_plus_one", P.fault_row_stride_plus_one)])
def test_row_faults_exceed_a_bound(fault, fn):
    for case in cases_of(fault):
        d = P.make(case)
        r = ce_ratios(d, fn(d))
        assert r["loss"] > 1.0 or r["lse"] > 1.0, (fault, case.name, r)
        assert exceeds(r), (fault, case.name, r)


def test_named_cases_are_the_ones_the_issue_lists():
    assert {P.BY_NAME[n].n for n in P.FAULT_CASES["last_element_dropped"]} == {65, 129, 1025, 2049}
    assert {P.BY_NAME[n].n for n in P.FAULT_CASES["pass17_dropped"]} == {1025, 2049}
    assert {P.BY_NAME[n].B for n in P.FAULT_CASES["sum_stops_at_256"]} == {257, 513, 1027}


def test_sum_faults_exceed_the_bound():
    for fault, fn in (("sum_stops_at_256", P.fault_sum_stops_at_256), ("mean_for_sum", P.fault_mean_for_sum)):
        for case in cases_of(fault):
            d = P.make(case)
            kinds = [(P.l2(d["a"], d["t"], d["py"])["row"], P.bound_l2(d["a"], d["t"], d["py"]))]
            if case.n >= 2:                                   # one class: every row loss is 0, and so is its sum under any fault
                kinds.append((P.ce(d["x"], d["y"])["loss"], P.bound_loss(d["x"], d["y"])))
            for rows, b in kinds:
                assert P.ratio(fn(rows.astype(np.float32)), rows.sum(), P.bound_sum(rows, b)) > 1.0, (fault, case.name)
            hits = P.ce(d["x"], d["y"])["hit"]
            if hits.sum() > 0 and fault == "mean_for_sum":
                assert fn(hits.astype(np.float32)) != hits.sum()


def test_tie_to_last_changes_hit():
    for case in cases_of("tie_to_last"):
        d = P.make(case)
        assert (P.fault_tie_to_last(d) != P.ce(d["x"], d["y"])["hit"]).all(), case.name      # every row: the label sits on one of the equals


def test_prototype_faults_exceed_a_bound():
    for case in cases_of("kl_direction"):
        d = P.make(case)
        a, t, py = d["a"], d["t"], d["py"]
        assert P.ratio(P.fault_kl_direction(d)["row"], P.kl(a, t, py)["row"], P.bound_kl(a, t, py)) > 1.0, case.name
    for case in cases_of("l2_grad_half"):
        d = P.make(case)
        a, t, py = d["a"], d["t"], d["py"]
        assert P.ratio(P.fault_l2_grad_half(d, K_PROTO)["g"], P.l2(a, t, py, K_PROTO)["g"], P.bound_demb_l2(a, t, py, K_PROTO)) > 1.0, case.name
    for case in cases_of("neighbour_label_prototype"):
        d = P.make(case)
        a, t, py = d["a"], d["t"], d["py"]
        assert (np.roll(py, -1) != py).any()
        fk, f2 = P.fault_neighbour_label_prototype(d)
        assert case.n == 1 or P.ratio(fk["row"], P.kl(a, t, py)["row"], P.bound_kl(a, t, py)) > 1.0, case.name      # width 1: the KL is 0
        assert P.ratio(f2["row"], P.l2(a, t, py)["row"], P.bound_l2(a, t, py)) > 1.0, case.name


def test_forget_rows_with_the_remain_coefficient_exceed_the_bound():
    c_r, c_f = 1.0 / 3, -0.15 / 2
    for case in cases_of("forget_rows_take_remain_coef"):
        d = P.make(case)
        nr = max(1, case.B // 2)
        g = P.fault_forget_rows_take_remain_coef(d, nr, c_r, c_f)[nr:]
        x, y = d["x"][nr:], d["y"][nr:]
        assert P.ratio(g, P.ce(x, y, c_f)["g"], P.bound_dlogits(x, y, c_f)) > 1.0, case.name


@pytest.mark.parametrize("has_proto", [True, False])
def test_tail_faults_change_a_coefficient(has_proto):
    for name, s, n_r, n_f, h in P.TAIL_GRID:
        right = P.tail32(s, n_r, n_f, None, h, has_proto)[2]
        assert n_r != n_f
        assert (P.fault_swapped_sizes(s, n_r, n_f, None, h, has_proto)[2] != right).any(), name
        if name == "zero":                                    # the only rows that can show relu'(0) = 1
            wrong = P.fault_relu_grad_one_at_zero(s, n_r, n_f, None, h, has_proto)[2]
            assert wrong[1] != right[1] and (not has_proto or wrong[2] != right[2])
