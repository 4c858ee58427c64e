"""The loss kernels (csrc/loss.hip: gsl_ce_fwd / bwd, gsl_proto_{kl,l2}_{fwd,bwd}, gsl_topk_hits, gsl_loss_combine[_pack], gsl_loss_tail[_l2])
at their edges, on the probes of oracle/loss_probes.py: every lane-stride end of the row width, row counts around the 4-row block and into
the second and third trip of the batch sum, labels and row maxima at 0 / 63 / 64 / C - 1, ties of the maximum inside a lane and across
lanes, logits offset by +-1e4, a spread of 200, CosFace-like confident rows, -inf logits, accumulation, out-of-range labels, a prototype
table with Cp != C, the scalar tail against an independent statement of its formula, the one-launch tail against float64, top-k ties.

Every entry point is called through gslora_hip._lib so that every tensor — the scratch and result buffers the ops wrappers allocate
themselves included — sits between NaN bands (tests/guard_bands.py): inputs unchanged, no output element unwritten, nothing written beyond
the documented sizes (2B / B floats of row_ws, 14 of out14, nk of hits). Floating-point results are held per element to the float64
references under the bounds of oracle/loss_probes.py (no tolerance of this file's own; tests/test_loss_probes_host.py shows on the CPU
that an f32 restatement of the kernels stays under them and that each fault model exceeds them); hit, hits and the scalar tail's bits are
compared exactly. Each comparison prints its largest error / bound ratio (pytest -s; profiles/loss_kernel_tests.md).

Finding this file was written against: the hinges of the scalar tail took relu with fmaxf, which drops a NaN — a NaN forget-side sum (a
forget label out of range, a forget class without a prototype) left a FINITE total and finite meters, so the deferred meter read that is
meant to stop such a run saw nothing (test_nan_forget_sums_reach_the_total, test_tail_label_beyond_the_prototype_table[forget],
test_tail_nan_prototype_row[forget], test_pack_without_forget_rows). And accumulate = 1 was not fl(old + g): the compiler fused the add
into the product that forms g, in the unrolled pairs of the backward loops only (test_backward_accumulates_scales_and_zeroes,
test_out_of_range_label)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from guard_bands import NAN_SENTINEL, Banded, ptr
from oracle import loss_probes as P

pytestmark = pytest.mark.gpu

F32 = torch.float32
NF = np.float32
K_CE, K_PROTO = 0.37, -1.3
CASES = list(P.TABLE)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    from gslora_hip import _lib
    _lib.load()
    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def In(a):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return Banded(t.shape, t.dtype, t)


def Scalar(v):
    return None if v is None else In(np.array([v], dtype=NF))


def Out(*shape):
    return Banded(shape, F32, sentinel=NAN_SENTINEL[F32])


def call(lib, entry, *args):
    lib.check(getattr(lib.load(), entry)(*args, stream()), entry)


def settled(t, outputs):
    torch.cuda.synchronize()
    for n, b in t.items():
        if b is not None and not getattr(b, "accumulates", False):
            assert b.bands_intact(), ("input changed or bands of" if b.is_input else "bands of", n)
    for n in outputs:
        assert t[n].unwritten() == 0, ("unwritten elements in", n)


def host(b):
    return b.view.cpu().numpy()


def under(what, got, ref, bound):
    r = P.ratio(got, ref, bound)
    print(f"RATIO {what} {r:.3f}")
    assert r <= 1.0, (what, r)
    return r


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------- the entry points, banded
def ce_fwd(lib, x, y):
    B, C = x.shape
    t = dict(x=In(x), y=In(y), out2=Out(2), ws=Out(2 * B))
    call(lib, "gsl_ce_fwd", ptr(t["x"]), ptr(t["y"]), ptr(t["out2"]), ptr(t["ws"]), B, C)
    settled(t, ("out2", "ws"))
    ws, out2 = host(t["ws"]).reshape(B, 2), host(t["out2"])
    return dict(loss=ws[:, 0].copy(), hit=ws[:, 1].copy(), sum=out2[0], hits=out2[1])


def grad_buffer(shape, old):
    if old is None:
        return Out(*shape)
    g = In(old)
    g.accumulates = True
    return g


def grad_result(g, old):
    if old is None:
        assert g.bands_intact() and g.unwritten() == 0
    else:
        assert g.outside_intact(), "something outside the accumulated gradient changed"
    return host(g).copy()


def ce_bwd(lib, x, y, coef, scale=1.0, old=None):
    B, C = x.shape
    t = dict(x=In(x), y=In(y), coef=Scalar(coef), g=grad_buffer((B, C), old))
    call(lib, "gsl_ce_bwd", ptr(t["x"]), ptr(t["y"]), ptr(t["coef"]), float(scale), ptr(t["g"]), B, C, 0 if old is None else 1)
    settled(t, ())
    return grad_result(t["g"], old)


def proto_fwd(lib, kind, a, py, tab):
    B, D = a.shape
    t = dict(a=In(a), y=In(py), tab=In(tab), out1=Out(1), ws=Out(B))
    call(lib, f"gsl_proto_{kind}_fwd", ptr(t["a"]), ptr(t["y"]), ptr(t["tab"]), ptr(t["out1"]), ptr(t["ws"]), B, D, tab.shape[0])
    settled(t, ("out1", "ws"))
    return dict(row=host(t["ws"]).copy(), sum=host(t["out1"])[0])


def proto_bwd(lib, kind, a, py, tab, coef, scale=1.0, old=None):
    B, D = a.shape
    t = dict(a=In(a), y=In(py), tab=In(tab), coef=Scalar(coef), g=grad_buffer((B, D), old))
    call(lib, f"gsl_proto_{kind}_bwd", ptr(t["a"]), ptr(t["y"]), ptr(t["tab"]), ptr(t["coef"]), float(scale), ptr(t["g"]), B, D, tab.shape[0],
         0 if old is None else 1)
    settled(t, ())
    return grad_result(t["g"], old)


def topk(lib, x, y, ks):
    B, C = x.shape
    t = dict(x=In(x), y=In(y), hits=Banded((len(ks),), torch.int32))          # the sentinel 0x5A5A5A5A is the garbage the call must clear
    arr = (ctypes.c_int * len(ks))(*ks)
    call(lib, "gsl_topk_hits", ptr(t["x"]), ptr(t["y"]), B, C, arr, len(ks), ptr(t["hits"]))
    torch.cuda.synchronize()
    assert all(b.bands_intact() for b in t.values())
    return host(t["hits"]).astype(np.int64)


def split14(total, meters, coefs):
    return host(total)[0].copy(), host(meters).copy(), host(coefs).copy()


def combine(lib, s, n_r, n_f, structure, h, has_proto=True):
    t = dict(ce_r=Scalar(s.ce_r), ce_f=Scalar(s.ce_f), kl_f=Scalar(s.kl_f) if has_proto else None, kl_r=Scalar(s.kl_r) if has_proto else None,
             st=Scalar(structure), hit_r=Scalar(s.hit_r), hit_f=Scalar(s.hit_f), total=Out(1), meters=Out(8), coefs=Out(5))
    call(lib, "gsl_loss_combine", ptr(t["ce_r"]), ptr(t["ce_f"]), ptr(t["kl_f"]), ptr(t["kl_r"]), ptr(t["st"]), ptr(t["hit_r"]), ptr(t["hit_f"]),
         float(n_r), float(n_f), *map(float, h), ptr(t["total"]), ptr(t["meters"]), ptr(t["coefs"]))
    settled(t, ("total", "meters", "coefs"))
    return split14(t["total"], t["meters"], t["coefs"])


def combine_pack(lib, s, n_r, n_f, structure, h, has_proto=True):
    pack = np.array([s.ce_r, s.ce_f, s.hit_r, s.hit_f, n_r, n_f, s.kl_f, s.kl_r], dtype=NF)
    t = dict(pack=In(pack), st=Scalar(structure), total=Out(1), meters=Out(8), coefs=Out(5))
    call(lib, "gsl_loss_combine_pack", ptr(t["pack"]), ptr(t["st"]), 1 if has_proto else 0, *map(float, h), ptr(t["total"]), ptr(t["meters"]),
         ptr(t["coefs"]))
    settled(t, ("total", "meters", "coefs"))
    return split14(t["total"], t["meters"], t["coefs"])


def tail_buffers(x, y, a, tab, structure):
    N, C = x.shape
    t = dict(x=In(x), y=In(y), a=None if a is None else In(a), tab=None if tab is None else In(tab), st=Scalar(structure), out14=Out(14),
             dlogits=Out(N, C), demb=None if a is None else Out(*a.shape))
    return t


def tail_args(t, N, nr, C, D, Cp, h):
    return (ptr(t["x"]), ptr(t["y"]), N, nr, C, ptr(t["a"]), ptr(t["tab"]), D, Cp, ptr(t["st"]), *map(float, h), ptr(t["out14"]), ptr(t["dlogits"]),
            ptr(t["demb"]))


def tail(lib, kind, x, y, nr, a, tab, structure, h):
    """gsl_loss_tail (kind "kl"; a None: no prototype term) or gsl_loss_tail_l2 -> (total, meters, coefs, dlogits, demb)."""
    N, C = x.shape
    D, Cp = (a.shape[1], tab.shape[0]) if a is not None else (0, 0)
    t = tail_buffers(x, y, a, tab, structure)
    call(lib, "gsl_loss_tail_l2" if kind == "l2" else "gsl_loss_tail", *tail_args(t, N, nr, C, D, Cp, h))
    settled(t, ("out14", "dlogits") + (("demb",) if a is not None else ()))
    o = host(t["out14"]).copy()
    return o[0], o[1:9], o[9:14], host(t["dlogits"]).copy(), None if a is None else host(t["demb"]).copy()


# ---------------------------------------------------------------------------------------------------------------- widths x rows x regimes
@functools.lru_cache(maxsize=4)
def refs(name):
    """The case's arrays and float64 references, computed once, shared, never written to."""
    d = P.make(P.BY_NAME[name])
    x, y, a, t, py = d["x"], d["y"], d["a"], d["t"], d["py"]
    r = dict(d=d, ce=P.ce(x, y, K_CE), kl=P.kl(a, t, py, K_PROTO), l2=P.l2(a, t, py, K_PROTO))
    r["b_loss"], r["b_kl"], r["b_l2"] = P.bound_loss(x, y), P.bound_kl(a, t, py), P.bound_l2(a, t, py)
    return r


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_cross_entropy_on_the_table(lib, case):
    """gsl_ce_fwd and gsl_ce_bwd (accumulate = 0): row loss, hit, the two sums and dlogits."""
    R = refs(case.name)
    d, ref = R["d"], R["ce"]
    x, y = d["x"], d["y"]
    got = ce_fwd(lib, x, y)
    under(f"{case.name} loss", got["loss"], ref["loss"], R["b_loss"])
    under(f"{case.name} ce_sum", got["sum"], ref["loss"].sum(), P.bound_sum(ref["loss"], R["b_loss"]))
    assert same_bits(got["hit"], ref["hit"].astype(NF)), (case.name, "hit")
    assert got["hits"] == ref["hit"].sum(), (case.name, "hits")
    g = ce_bwd(lib, x, y, K_CE)
    under(f"{case.name} dlogits", g, ref["g"], P.bound_dlogits(x, y, K_CE))
    if case.regime == "neginf":
        assert np.isfinite(got["loss"]).all() and (g[np.isinf(x)] == 0).all() and np.isinf(x).any()
    if case.regime == "cosface":
        e_row = np.abs(got["loss"].astype(np.float64) - ref["loss"])
        i = int(e_row.argmax())
        e_sum, s = abs(float(got["sum"]) - ref["loss"].sum()), ref["loss"].sum()
        print(f"COSFACE {case.name} row: |err| {e_row[i]:.3e} on loss {ref['loss'][i]:.3e} (rel {e_row[i] / ref['loss'][i]:.3e}); "
              f"largest rel {np.max(e_row / ref['loss']):.3e}; batch of {case.B}: |err| {e_sum:.3e} on {s:.3e} (rel {e_sum / s:.3e}), "
              f"mean-loss err {e_sum / case.B:.3e}")


@pytest.mark.parametrize("case", [c for c in CASES if c.regime == "unit"], ids=lambda c: c.name)
def test_prototype_distances_on_the_table(lib, case):
    """gsl_proto_{kl,l2}_{fwd,bwd} (accumulate = 0) with the width D = n and a table of Cp != n rows."""
    R = refs(case.name)
    d = R["d"]
    a, t, py = d["a"], d["t"], d["py"]
    assert t.shape[0] != case.n
    for kind, b_row, b_g in (("kl", R["b_kl"], P.bound_demb_kl), ("l2", R["b_l2"], P.bound_demb_l2)):
        ref = R[kind]
        got = proto_fwd(lib, kind, a, py, t)
        under(f"{case.name} {kind} row", got["row"], ref["row"], b_row)
        under(f"{case.name} {kind}_sum", got["sum"], ref["row"].sum(), P.bound_sum(ref["row"], b_row))
        under(f"{case.name} demb_{kind}", proto_bwd(lib, kind, a, py, t, K_PROTO), ref["g"], b_g(a, t, py, K_PROTO))


def test_non_finite_logits_as_the_header_states(lib):
    """-inf at the label: +inf; +inf or NaN anywhere (not at the maximum's or the label's place here): NaN; the other rows keep their bits."""
    d = P.make(P.BY_NAME["w129_b5"])
    x, y = d["x"], d["y"]
    base = ce_fwd(lib, x, y)
    x2 = x.copy()
    x2[0, y[0]] = -np.inf
    x2[1, 5] = np.inf
    x2[2, 70] = np.nan
    got = ce_fwd(lib, x2, y)
    assert got["loss"][0] == np.inf and np.isnan(got["loss"][1]) and np.isnan(got["loss"][2]) and same_bits(got["loss"][3:], base["loss"][3:])
    assert (got["hit"][:2] == 0).all() and base["hit"][2] == 1 and same_bits(got["hit"][2:], base["hit"][2:])            # the arg-max skips a NaN: hit is that of the row's other logits (the loss stops the run)


# ---------------------------------------------------------------------------------------------------------------- backward variants
@pytest.mark.parametrize("kind", ["ce", "kl", "l2"])
def test_backward_accumulates_scales_and_zeroes(lib, kind):
    d = P.make(P.BY_NAME["w129_b5"])
    if kind == "ce":
        x, y = d["x"], d["y"]
        run = lambda coef, scale=1.0, old=None: ce_bwd(lib, x, y, coef, scale, old)
        ref = lambda k: (P.ce(x, y, k)["g"], P.bound_dlogits(x, y, k))
    else:
        a, t, py = d["a"], d["t"], d["py"]
        run = lambda coef, scale=1.0, old=None: proto_bwd(lib, kind, a, py, t, coef, scale, old)
        f, b = (P.kl, P.bound_demb_kl) if kind == "kl" else (P.l2, P.bound_demb_l2)
        ref = lambda k: (f(a, t, py, k)["g"], b(a, t, py, k))
    g0 = run(K_CE)
    old = np.random.default_rng(5).standard_normal(g0.shape).astype(NF) * NF(0.01)
    assert same_bits(run(K_CE, old=old), old + g0), (kind, "accumulate = 1 is not fl(old + g)")
    z = run(0.0)
    assert (z == 0).all(), (kind, "coef = 0")
    for coef, scale in ((-0.8, 1.0), (0.37, 2.5), (-0.8, 1.0 / 3)):
        k = float(NF(coef)) * float(NF(scale))
        under(f"{kind} bwd coef {coef} scale {scale:.3f}", run(coef, scale), *ref(k))


BAD_LABELS = (-1, None, 2 ** 31 + 3)            # None: the class count itself


@pytest.mark.parametrize("bad", BAD_LABELS, ids=["-1", "C", "2^31+3"])
def test_out_of_range_label(lib, bad):
    """Row 2 (a third wave of a block) carries the bad label: NaN loss / sum / gradient row, the other rows bit for bit, and nothing read
    out of bounds (the bands around logits, the table and every output)."""
    d = P.make(P.BY_NAME["w65_b257"])
    x, y, a, t, py = d["x"], d["y"], d["a"], d["t"], d["py"]
    ok = np.arange(len(y)) != 2
    y2, py2 = y.copy(), py.copy()
    y2[2] = x.shape[1] if bad is None else bad
    py2[2] = t.shape[0] if bad is None else bad
    f0, f1 = ce_fwd(lib, x, y), ce_fwd(lib, x, y2)
    assert np.isnan(f1["loss"][2]) and f1["hit"][2] == 0 and np.isnan(f1["sum"]) and f1["hits"] == f0["hits"] - f0["hit"][2]
    assert same_bits(f1["loss"][ok], f0["loss"][ok]) and same_bits(f1["hit"][ok], f0["hit"][ok])
    g0, g1 = ce_bwd(lib, x, y, K_CE), ce_bwd(lib, x, y2, K_CE)
    assert np.isnan(g1[2]).all() and same_bits(g1[ok], g0[ok])
    old = np.full_like(g0, 0.25)
    g2 = ce_bwd(lib, x, y2, K_CE, old=old)
    assert np.isnan(g2[2]).all() and same_bits(g2[ok], (old + g0)[ok])
    for kind in ("kl", "l2"):
        p0, p1 = proto_fwd(lib, kind, a, py, t), proto_fwd(lib, kind, a, py2, t)
        assert np.isnan(p1["row"][2]) and np.isnan(p1["sum"]) and same_bits(p1["row"][ok], p0["row"][ok])
        q0, q1 = proto_bwd(lib, kind, a, py, t, K_PROTO), proto_bwd(lib, kind, a, py2, t, K_PROTO)
        assert np.isnan(q1[2]).all() and same_bits(q1[ok], q0[ok])
    ks = [1, 5]
    assert (topk(lib, x, y2, ks) == P.topk_hits(x, y2, ks)).all() and (topk(lib, x, y, ks) == P.topk_hits(x, y, ks)).all()


@pytest.mark.parametrize("kind", ["kl", "l2"])
def test_prototype_table_smaller_than_the_label_range_and_nan_rows(lib, kind):
    """Cp = 7 rows under D = 65: label 7 (valid for a 65-wide row, beyond the table) and a table row of NaN both give a NaN row."""
    d = P.make(P.BY_NAME["w65_b5"])
    a, t, py = d["a"], d["t"], d["py"].copy()
    assert t.shape[0] == 7
    base = proto_fwd(lib, kind, a, py, t)
    py[1] = 7
    t2 = t.copy()
    t2[py[3]] = np.nan
    keep = np.array([r not in (1, 3) and py[r] != py[3] for r in range(5)])
    got = proto_fwd(lib, kind, a, py, t2)
    assert np.isnan(got["row"][[1, 3]]).all() and np.isnan(got["sum"]) and same_bits(got["row"][keep], base["row"][keep]) and keep.any()
    g = proto_bwd(lib, kind, a, py, t2, K_PROTO)
    assert np.isnan(g[[1, 3]]).all() and np.isfinite(g[keep]).all()


# ---------------------------------------------------------------------------------------------------------------- the scalar tail
GRID = [(row, st, hp) for row in P.TAIL_GRID for st in (None, P.STRUCTURE) for hp in (True, False)]


@pytest.mark.parametrize("row,structure,has_proto", GRID, ids=lambda v: v[0] if isinstance(v, tuple) else str(v))
def test_scalar_tail_equals_its_float32_restatement(lib, row, structure, has_proto):
    """gsl_loss_combine and gsl_loss_combine_pack against oracle.loss_probes.tail32, bit for bit (contraction is off in the kernels' function
    and f32 division is IEEE), and under the derived float64 bound as a backstop."""
    name, s, n_r, n_f, h = row
    want = P.tail32(s, n_r, n_f, structure, h, has_proto)
    ref, bound = P.tail64(s, n_r, n_f, structure, h, has_proto), P.bound_tail(s, n_r, n_f, structure, h, has_proto)
    for form, fn in (("combine", combine), ("pack", combine_pack)):
        got = fn(lib, s, n_r, n_f, structure, h, has_proto)
        for what, g, w, r64, b in zip(("total", "meters", "coefs"), got, want, ref, bound):
            assert same_bits(np.asarray(g, dtype=NF), np.asarray(w, dtype=NF)), (form, name, what, g, w)
            under(f"tail {form} {name} st={structure} proto={has_proto} {what}", g, r64, b)
    if name == "zero":
        assert got[1][0] == 0 and got[2][1] == 0 and (not has_proto or (got[1][6] == 0 and got[2][2] == 0))      # relu(0) = 0, relu'(0) = 0
    if not has_proto:
        assert got[1][6] == NF(h.w_f) * max(NF(h.BND_pro), NF(0)) and got[1][7] == 0 and got[2][2] == 0 and got[2][3] == 0


@pytest.mark.parametrize("which", ["ce_f", "kl_f"])
def test_nan_forget_sums_reach_the_total(lib, which):
    """A NaN forget-side sum (what an out-of-range forget label or a forget class without a prototype produces) must show in the total and
    in its meter, as torch's relu shows it; the remain-side meters stay finite."""
    name, s, n_r, n_f, h = P.TAIL_GRID[0]
    bad = s._replace(**{which: float("nan")})
    for fn in (combine, combine_pack):
        total, meters, coefs = fn(lib, bad, n_r, n_f, None, h)
        assert np.isnan(total) and np.isnan(meters[2]) and np.isnan(meters[0 if which == "ce_f" else 6]), (fn.__name__, total, meters)
        assert np.isfinite(meters[[1, 4, 5, 7]]).all() and coefs[1 if which == "ce_f" else 2] == 0 and np.isfinite(coefs).all()


def test_pack_without_forget_rows(lib):
    """n_f = 0 in the pack (not checked, include/gslora_hip.h): the empty mean's 0 / 0 turns the forget side and the total NaN, the remain side
    is that of the remain rows alone."""
    name, s, n_r, n_f, h = P.TAIL_GRID[0]
    s0 = s._replace(ce_f=0.0, hit_f=0.0, kl_f=0.0)
    total, meters, coefs = combine_pack(lib, s0, n_r, 0.0, None, h)
    want = P.tail32(s0, n_r, 0.0, None, h)
    assert np.isnan(total) and np.isnan(meters[[0, 2, 4, 6]]).all() and coefs[1] == 0 and coefs[2] == 0
    for i in (1, 5, 7):
        assert meters[i] == want[1][i]
    assert same_bits(coefs, want[2])


# ---------------------------------------------------------------------------------------------------------------- the one-launch tail
H_TAIL = P.Hyper(0.15, 60.0, 0.01, 0.3, 0.7, 5000.0)            # both hinges active at every shape: four distinct, non-zero coefficients
TAIL_SHAPES = ([(N, nr, 65, 65) for N in (2, 16, 17, 33, 256) for nr in sorted({1, N // 2, N - 1})]
               + [(17, 5, 1, 1024), (17, 12, 1024, 1), (33, 16, 1024, 1024), (256, 255, 1024, 1024), (2, 1, 1, 1), (16, 15, 1024, 65), (256, 1, 65, 1024)])


@functools.lru_cache(maxsize=2)
def tail_inputs(N, C, D):
    d = P.make(P.Case(f"tail_{N}_{C}", N, C, "unit"))
    a = P.make(P.Case(f"tail_{N}_{D}", N, D, "unit"))["a"]
    tab = (np.random.default_rng(N + 7 * C + 13 * D).standard_normal((C + 3, D)) * 1.5).astype(NF)            # Cp = C + 3
    return d["x"], d["y"], a, tab


def tail_reference(kind, x, y, nr, a, tab, structure, h):
    """float64: (total, meters, coefs), their bounds, dlogits and demb with their bounds, from the two row ranges."""
    N = len(y)
    rr, ff = slice(0, nr), slice(nr, N)
    c = P.ce(x, y)
    b_loss = P.bound_loss(x, y)
    has = a is not None
    if has:
        fn, brow = (P.l2, P.bound_l2) if kind == "l2" else (P.kl, P.bound_kl)
        p, b_p = fn(a, tab, y)["row"], brow(a, tab, y)
    else:
        p, b_p = np.zeros(N), np.zeros(N)
    s = P.Sums(c["loss"][rr].sum(), c["loss"][ff].sum(), p[ff].sum(), p[rr].sum(), c["hit"][rr].sum(), c["hit"][ff].sum())
    sb = P.Sums(P.bound_sum(c["loss"][rr], b_loss[rr]), P.bound_sum(c["loss"][ff], b_loss[ff]), P.bound_sum(p[ff], b_p[ff]), P.bound_sum(p[rr], b_p[rr]), 0, 0)
    t64 = P.tail64(s, nr, N - nr, structure, h, has)
    bt = P.bound_tail(s, nr, N - nr, structure, h, has, sum_bounds=sb)
    co = t64[2]
    assert co[0] != 0 and co[1] != 0 and (not has or (co[2] != 0 and co[3] != 0 and len(set(co[:4])) == 4))
    dl = np.concatenate([P.ce(x[rr], y[rr], co[0])["g"], P.ce(x[ff], y[ff], co[1])["g"]])
    b_dl = np.concatenate([P.bound_dlogits(x[rr], y[rr], co[0]), P.bound_dlogits(x[ff], y[ff], co[1])]) + 8 * P.E * np.abs(dl)      # the coefficient's own roundings
    de = b_de = None
    if has:
        bg = P.bound_demb_l2 if kind == "l2" else P.bound_demb_kl
        de = np.concatenate([fn(a[rr], tab, y[rr], co[3])["g"], fn(a[ff], tab, y[ff], co[2])["g"]])
        b_de = np.concatenate([bg(a[rr], tab, y[rr], co[3]), bg(a[ff], tab, y[ff], co[2])]) + 8 * P.E * np.abs(de)
    return t64, bt, dl, b_dl, de, b_de


@pytest.mark.parametrize("kind", ["kl", "l2", "none"])
@pytest.mark.parametrize("N,nr,C,D", TAIL_SHAPES, ids=lambda v: str(v))
def test_one_launch_tail_against_float64(lib, kind, N, nr, C, D):
    x, y, a, tab = tail_inputs(N, C, D)
    if kind == "none":
        a = tab = None
    structure = P.STRUCTURE if N % 2 else None
    got = tail(lib, kind, x, y, nr, a, tab, structure, H_TAIL)
    t64, bt, dl, b_dl, de, b_de = tail_reference(kind, x, y, nr, a, tab, structure, H_TAIL)
    what = f"tail {kind} N{N} nr{nr} C{C} D{D}"
    under(f"{what} total", got[0], t64[0], bt[0])
    under(f"{what} meters", got[1], t64[1], bt[1])
    under(f"{what} coefs", got[2], t64[2], bt[2])
    under(f"{what} dlogits", got[3], dl, b_dl)
    if a is not None:
        under(f"{what} demb", got[4], de, b_de)


@pytest.mark.parametrize("regime", ["tie_lane", "tie_cross"])
def test_one_launch_tail_counts_ties_by_the_first_index(lib, regime):
    """The register form of the row (RegRow) on the tie rows: the two accuracy meters are those of the first-index rule, the rest as before."""
    d = P.make(P.BY_NAME[f"{regime}_w129_b8"])
    x, y, nr = d["x"], d["y"], 3
    hit = P.ce(x, y)["hit"]
    assert (hit == (y == d["first"])).all() and 0 < hit[:nr].sum() < nr and 0 < hit[nr:].sum() < 8 - nr
    total, meters, coefs, dl, _ = tail(lib, "none", x, y, nr, None, None, None, H_TAIL)
    t64, bt, ref_dl, b_dl, _, _ = tail_reference("none", x, y, nr, None, None, None, H_TAIL)
    under(f"tail {regime} meters", meters, t64[1], bt[1])
    assert meters[4] == NF(hit[nr:].sum()) * (NF(100) / NF(8 - nr)) and meters[5] == NF(hit[:nr].sum()) * (NF(100) / NF(nr))
    under(f"tail {regime} dlogits", dl, ref_dl, b_dl)


@pytest.mark.parametrize("where", ["remain", "forget"])
@pytest.mark.parametrize("kind", ["kl", "l2"])
def test_tail_label_beyond_the_prototype_table(lib, kind, where):
    """C = 65 classes, a table of Cp = 7 rows: a label valid for the cross entropy and beyond Cp turns ONLY the prototype term NaN."""
    N, nr = 17, 5
    x, y, a, tab = tail_inputs(N, 65, 65)
    row = 2 if where == "remain" else 9
    y2 = y % 7
    y2[row] = 64
    base = tail(lib, kind, x, y2, nr, a, tab, None, H_TAIL)            # the whole table (Cp = 68): label 64 has a prototype
    total, meters, coefs, dl, de = tail(lib, kind, x, y2, nr, a, tab[:7], None, H_TAIL)
    proto_meter = 7 if where == "remain" else 6
    assert np.isnan(total) and np.isnan(meters[2]) and np.isnan(meters[proto_meter]), (total, meters)
    assert same_bits(np.delete(meters, [2, proto_meter]), np.delete(base[1], [2, proto_meter])), (meters, base[1])
    ok = np.arange(N) != row
    assert np.isfinite(dl).all() and same_bits(dl[ok], base[3][ok]) and np.isnan(de[row]).all() and np.isfinite(de[ok]).all()


@pytest.mark.parametrize("where", ["remain", "forget"])
@pytest.mark.parametrize("kind", ["kl", "l2"])
def test_tail_nan_prototype_row(lib, kind, where):
    """A table row of NaN (a class without a prototype) does the same."""
    N, nr = 17, 5
    x, y, a, tab = tail_inputs(N, 65, 65)
    row = 2 if where == "remain" else 9
    y = y.copy()
    assert 30 not in y
    y[row] = 30                                                # a class no other image has
    base = tail(lib, kind, x, y, nr, a, tab, None, H_TAIL)
    tab2 = tab.copy()
    tab2[30] = np.nan
    total, meters, coefs, dl, de = tail(lib, kind, x, y, nr, a, tab2, None, H_TAIL)
    proto_meter = 7 if where == "remain" else 6
    assert np.isnan(total) and np.isnan(meters[2]) and np.isnan(meters[proto_meter]), (total, meters)
    assert same_bits(np.delete(meters, [2, proto_meter]), np.delete(base[1], [2, proto_meter]))
    ok = np.arange(N) != row
    assert same_bits(dl, base[3]) and np.isnan(de[row]).all() and np.isfinite(de[ok]).all()


@pytest.mark.parametrize("why,kw,names", [("N = 257", dict(N=257), "N <= 256"), ("nr = 0", dict(nr=0), "0 < nr"), ("nr = N", dict(nr=8), "nr < N"),
                                          ("C = 1025", dict(C=1025), "C and D <= 1024"), ("l2 without emb", dict(kind="l2", emb=False), "emb")])
def test_tail_refusals_name_the_argument_and_launch_nothing(lib, why, kw, names):
    N, nr, C, D = kw.get("N", 8), kw.get("nr", 3), kw.get("C", 65), 65
    kind, emb = kw.get("kind", "kl"), kw.get("emb", True)
    x, y = np.ones((N, C), dtype=NF), np.zeros(N, dtype=np.int64)
    a, tab = (np.ones((N, D), dtype=NF), np.ones((4, D), dtype=NF))
    t = tail_buffers(x, y, a, tab, None)
    args = list(tail_args(t, N, nr, C, D, 4, H_TAIL))
    if not emb:
        args[5] = None
    entry = "gsl_loss_tail_l2" if kind == "l2" else "gsl_loss_tail"
    with pytest.raises(RuntimeError, match=rf"\): {entry}: .*{names}"):
        call(lib, entry, *args)
    torch.cuda.synchronize()
    for n in ("out14", "dlogits", "demb"):
        assert t[n].bands_intact() and t[n].unwritten() == t[n].rows * t[n].cols, (why, "wrote", n)


# ---------------------------------------------------------------------------------------------------------------- precision@k
@pytest.mark.parametrize("name", ["ints_w129_b8", "w65_b1027", "w1_b5", "w2049_b5", "tie_cross_w129_b8"])
def test_topk_hits_follow_the_header_rule(lib, name):
    """nk = 16 values of k, among them 1, 2, 5, 16, C and C + 3; integer logits tie at every k-th place."""
    d = P.make(P.BY_NAME[name])
    x, y = d["x"], d["y"]
    C = x.shape[1]
    ks = [1, 2, 5, 16, C, C + 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13]
    assert len(ks) == 16
    want = P.topk_hits(x, y, ks)
    got = topk(lib, x, y, ks)
    assert (got == want).all(), (name, got, want)
    assert got[4] == len(y) and got[5] == len(y)                       # k >= C: every valid row
    if P.BY_NAME[name].regime == "unit":                              # tie-free rows: torch.topk's answer
        xt, yt = torch.from_numpy(x), torch.from_numpy(y)
        for k, g in zip(ks, got):
            assert g == int((xt.topk(min(k, C), 1).indices == yt[:, None]).any(1).sum()), (name, k)
    assert (topk(lib, x, y, ks[:3]) == want[:3]).all()                 # nk < 16: hits [3]


# ---------------------------------------------------------------------------------------------------------------- determinism
def test_two_identical_calls_give_the_same_bits(lib):
    R = refs("big")
    d = R["d"]
    x, y, a, t, py = d["x"], d["y"], d["a"], d["t"], d["py"]
    assert x.shape == (1027, 2049)
    f1, f2 = ce_fwd(lib, x, y), ce_fwd(lib, x, y)
    assert all(same_bits(f1[k], f2[k]) for k in f1)
    assert same_bits(ce_bwd(lib, x, y, K_CE), ce_bwd(lib, x, y, K_CE))
    for kind in ("kl", "l2"):
        p1, p2 = proto_fwd(lib, kind, a, py, t), proto_fwd(lib, kind, a, py, t)
        assert all(same_bits(p1[k], p2[k]) for k in p1)
        assert same_bits(proto_bwd(lib, kind, a, py, t, K_PROTO), proto_bwd(lib, kind, a, py, t, K_PROTO))
    ks = [1, 5, 2049]
    assert (topk(lib, x, y, ks) == topk(lib, x, y, ks)).all()
    xs, ys, as_, tab = tail_inputs(256, 1024, 1024)
    for kind in ("kl", "l2"):
        o1, o2 = tail(lib, kind, xs, ys, 100, as_, tab, P.STRUCTURE, H_TAIL), tail(lib, kind, xs, ys, 100, as_, tab, P.STRUCTURE, H_TAIL)
        assert all(same_bits(u, v) for u, v in zip(o1, o2))


# ---------------------------------------------------------------------------------------------------------------- gslora_hip/losses.py
def test_ce_and_kl_nodes_are_differentiable_and_match_torch(lib):
    """The CE and KL autograd nodes, single and split (nr) forms, at N = 7, nr = 3, against torch autograd in float64."""
    from gslora_hip import losses
    N, nr, C, D = 7, 3, 65, 129
    x, y, _, _ = tail_inputs(N, C, D)
    a, tab = tail_inputs(N, C, D)[2], tail_inputs(N, C, D)[3]
    up = 3.0
    xt, yt, at, tt = (torch.from_numpy(v).cuda() for v in (x, y, a, tab))
    # float64 autograd
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    a64 = torch.from_numpy(a).double().requires_grad_(True)
    t64 = torch.from_numpy(tab).double()[torch.from_numpy(y)]
    ce64 = torch.nn.functional.cross_entropy(x64, torch.from_numpy(y), reduction="none")
    kl64 = (torch.softmax(t64, 1) * (torch.log_softmax(t64, 1) - torch.log_softmax(a64, 1))).sum(1)
    b_loss, b_kl = P.bound_loss(x, y), P.bound_kl(a, tab, y)
    # single forms
    xg = xt.clone().requires_grad_(True)
    s, hits = losses.ce_sum_top1(xg, yt)
    under("node ce_sum", s.item(), ce64.sum().item(), P.bound_sum(ce64.detach().numpy(), b_loss))
    assert hits.item() == P.ce(x, y)["hit"].sum() and not hits.requires_grad
    (g,) = torch.autograd.grad(s * up, xg)
    (g64,) = torch.autograd.grad(ce64.sum() * up, x64, retain_graph=True)
    under("node ce grad", g.cpu().numpy(), g64.numpy(), P.bound_dlogits(x, y, up))
    ag = at.clone().requires_grad_(True)
    k = losses.proto_kl_sum(ag, yt, tt)
    under("node kl_sum", k.item(), kl64.sum().item(), P.bound_sum(kl64.detach().numpy(), b_kl))
    (g,) = torch.autograd.grad(k * up, ag)
    (g64,) = torch.autograd.grad(kl64.sum() * up, a64, retain_graph=True)
    under("node kl grad", g.cpu().numpy(), g64.numpy(), P.bound_demb_kl(a, tab, y, up))
    # split forms: different upstream gradients on the two ranges; an unused range gets exact zeros
    rr, ff = slice(0, nr), slice(nr, N)
    xg = xt.clone().requires_grad_(True)
    ce_r, hit_r, ce_f, hit_f = losses.ce_sum_top1_split(xg, yt, nr)
    under("node split ce_r", ce_r.item(), ce64[rr].sum().item(), P.bound_sum(ce64[rr].detach().numpy(), b_loss[rr]))
    under("node split ce_f", ce_f.item(), ce64[ff].sum().item(), P.bound_sum(ce64[ff].detach().numpy(), b_loss[ff]))
    assert hit_r.item() == P.ce(x, y)["hit"][rr].sum() and hit_f.item() == P.ce(x, y)["hit"][ff].sum()
    (g,) = torch.autograd.grad(ce_r * 2.0 - ce_f * 0.5, xg)
    (g64,) = torch.autograd.grad(ce64[rr].sum() * 2.0 - ce64[ff].sum() * 0.5, x64, retain_graph=True)
    bound = np.concatenate([P.bound_dlogits(x[rr], y[rr], 2.0), P.bound_dlogits(x[ff], y[ff], -0.5)])
    under("node split ce grad", g.cpu().numpy(), g64.numpy(), bound)
    xg = xt.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(losses.ce_sum_top1_split(xg, yt, nr)[2] * up, xg)
    assert (g[rr] == 0).all() and (g[ff] != 0).any()
    ag = at.clone().requires_grad_(True)
    kl_f, kl_r = losses.proto_kl_sum_split(ag, yt, tt, nr)
    under("node split kl_f", kl_f.item(), kl64[ff].sum().item(), P.bound_sum(kl64[ff].detach().numpy(), b_kl[ff]))
    under("node split kl_r", kl_r.item(), kl64[rr].sum().item(), P.bound_sum(kl64[rr].detach().numpy(), b_kl[rr]))
    (g,) = torch.autograd.grad(kl_r * 2.0 - kl_f * 0.5, ag)
    (g64,) = torch.autograd.grad(kl64[rr].sum() * 2.0 - kl64[ff].sum() * 0.5, a64)
    bound = np.concatenate([P.bound_demb_kl(a[rr], tab, y[rr], 2.0), P.bound_demb_kl(a[ff], tab, y[ff], -0.5)])
    under("node split kl grad", g.cpu().numpy(), g64.numpy(), bound)
