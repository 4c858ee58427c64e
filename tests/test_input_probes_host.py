"""The patch-gather probes of oracle/input_probes.py, checked on the CPU for every row of the table tests/test_hip_patch_edges.py runs:

(a) the references agree with index arithmetic of another kind: unfold_ref with torch.nn.functional.unfold and with gather_index(),
    patchify_ref with gather_index() and, where the case is small enough to loop over, with a four-loop gather; on the index image every
    non-zero output element names the pixel gather_index() says it comes from;
(b) every fault model changes at least one compared element of each case it is aimed at (I.FAULT_TARGET), in f32 on the index image and
    in bf16 / fp16 on the value image (the widest rounding must not hide it);
(c) store() is the fp16 table of csrc/gsl_common.h (65520 -> 0x7bff, 1e6 -> 0x7bff, Inf -> 0x7c00, NaN stays NaN), rounds bf16 to
    nearest even, and keeps the sign of a zero; u8_image() is a plain lookup; the byte generators hold what they promise;
(d) the table reaches the paths it names (thread counts around one grid sweep, row counts around UNF_ROWS, the nch ladder).

Pure torch / numpy: no GPU and no library."""
import functools

import pytest
import torch
import torch.nn.functional as Fn

from oracle import input_probes as I

F32, BF16, F16 = I.F32, I.BF16, I.F16
NAMES = [c.name for c in I.TABLE]
SMALL = [c.name for c in I.TABLE if "sweep" not in c.tags]


@functools.lru_cache(maxsize=2)
def index_ref(name):
    case = I.BY_NAME[name]
    img = I.make(case, "index")
    return case, img, I.reference(case, img)


@pytest.mark.parametrize("name", NAMES)
def test_references_agree_with_index_arithmetic(name):
    case, img, ref = index_ref(name)
    T, cols = I.geometry(case)
    assert ref.shape == (case.B * T, cols) and ref.dtype == F32
    got = I.gather(case, img)
    assert torch.equal(I.bits(got), I.bits(ref))                      # +0 everywhere a zero stands
    idx = torch.from_numpy(I.gather_index(case))
    assert torch.equal(ref.long() - 1, idx)                           # element i holds i + 1; a zero is index -1
    assert (ref.view(case.B, T, cols)[:, 0] == 0).all()
    if case.op == "unfold":
        k, C = case.a, case.C
        x = Fn.unfold(img, k, padding=case.pad, stride=case.stride).transpose(1, 2)
        r3 = ref.view(case.B, T, cols)
        assert torch.equal(r3[:, 1:, :C * k * k], x) and (r3[:, :, C * k * k:] == 0).all()
    elif "sweep" not in case.tags:
        assert torch.equal(I.four_loops(img, case.a), ref)


def differs(a, b):
    return not torch.equal(I.bits(a), I.bits(b))


@pytest.mark.parametrize("fault,name", [(f, n) for f in I.FAULTS for n in I.FAULT_TARGET[f]])
def test_index_fault_models_are_caught(fault, name):
    case, img, ref = index_ref(name)
    bad = I.gather(case, img, fault)
    assert bad.shape == ref.shape and differs(bad, ref), (fault, name)
    val = I.make(case, "value")
    for dt in (BF16, F16):
        assert differs(I.store(I.gather(case, val, fault), dt), I.store(I.reference(case, val), dt)), (fault, name, dt)


@pytest.mark.parametrize("name", I.FAULT_TARGET["nhwc_as_nchw"])
@pytest.mark.parametrize("what", ["leak", "all"])
def test_nhwc_read_as_nchw_is_caught(name, what):
    case = I.BY_NAME[name]
    u, tab = I.make(case, what)
    ref = I.reference(case, I.u8_image(u, tab))
    for dt in I.DTYPES:
        assert differs(I.store(I.fault_nhwc_as_nchw(case, u, tab), dt), I.store(ref, dt)), (name, dt)


@pytest.mark.parametrize("fault", ["last_chunk_dropped", "last_block_dropped"])
def test_dropped_tails_are_caught(fault):
    fn = getattr(I, "fault_" + fault)
    for name in I.FAULT_TARGET[fault]:
        case, img, ref = index_ref(name)
        bad = fn(ref)
        assert differs(bad, ref) and int(torch.isnan(bad).sum()) > 0, (fault, name)
        # the dropped part may hold zeros only (the zero fill of a ladder row): a zero-initialised output would hide it, the sentinel does not
        assert differs(fn(ref, sentinel=7.0), ref)


def test_store_is_the_saturating_convert_of_the_kernels():
    x = torch.tensor([65520.0, 1e6, -65520.0, -1e6, float("inf"), float("-inf"), 65504.0, 65519.9, 1.0, 0.0, -0.0, 1e-8, 2.0 ** -25, 3e-8])
    h = I.store(x, F16).view(torch.int16).tolist()
    u = [v & 0xffff for v in h]
    assert u[:6] == [0x7bff, 0x7bff, 0xfbff, 0xfbff, 0x7c00, 0xfc00]
    assert u[6:11] == [0x7bff, 0x7bff, 0x3c00, 0x0000, 0x8000]
    assert u[11:] == [0x0000, 0x0000, 0x0001]              # below half the smallest subnormal, the tie to even, above it
    assert torch.isnan(I.store(torch.tensor([float("nan")]), F16)).all() and torch.isnan(I.store(torch.tensor([float("nan")]), BF16)).all()
    b = I.store(torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1e6, 65520.0, float("inf"), -0.0]), BF16).view(torch.int16).tolist()
    assert [v & 0xffff for v in b] == [0x3f80, 0x3f82, 0xc974, 0x4780, 0x7f80, 0x8000]      # ties to even; no clamp at fp16's range
    y = torch.tensor([65520.0, float("nan"), -0.0])
    assert I.store(y, F32) is y
    assert I.bits(torch.tensor([float("nan"), -float("nan")])).tolist() == [-1, -1]


def test_u8_image_is_a_lookup_and_the_generators_hold_what_they_promise():
    for name in ("p_c17_global", "u_nch5", "p_wide_16x24", "u_k1_nch1"):
        case = I.BY_NAME[name]
        u, tab = I.make(case, "leak")
        assert not (u == I.BAND_BYTE).any() and torch.isnan(tab[:, I.BAND_BYTE]).all() and (tab[:, 0] != 0).all()
        assert int(torch.isnan(tab).sum()) == case.C
        x = I.u8_image(u, tab)
        for (b, c, h, w) in ((0, 0, 0, 0), (case.B - 1, case.C - 1, case.H - 1, case.W - 1), (0, case.C // 2, case.H // 2, 1)):
            assert x[b, c, h, w] == tab[c, int(u[b, c, h, w])]
        ua, ta = I.make(case, "all")
        assert (ta[:, 0] != 0).all() and torch.isfinite(ta).all()
        if case.H * case.W >= 256:
            assert all(len(set(ua[0, c].flatten().tolist())) == 256 for c in range(case.C))
    sat = I.make(I.BY_NAME[I.SATURATION[0]], "value_sat")
    for v in I.SPECIALS[:4]:
        assert (sat == v).any()
    assert torch.isnan(sat).any() and torch.isnan(I.make(I.BY_NAME[I.SATURATION[1]], "leak_sat")[1]).any()
    assert (I.nhwc_bytes(torch.arange(24, dtype=torch.uint8).view(1, 2, 3, 4))[:4].tolist()) == [0, 12, 1, 13]


def test_the_table_reaches_the_paths_it_names():
    sweep = {n: I.BY_NAME[n] for n in ("p_sweep_narrow", "p_sweep_wide")}
    c = sweep["p_sweep_narrow"]
    assert c.a % 8 != 0 and 0 < c.B * I.geometry(c)[0] * c.a * c.a - I.GRID_SWEEP <= 256
    c = sweep["p_sweep_wide"]
    assert c.a % 8 == 0 and c.C == 1 and 0 < c.B * I.geometry(c)[0] * c.a * c.a // 8 - I.GRID_SWEEP <= 256
    assert [I.BY_NAME[f"u_rows{r}"].B * I.geometry(I.BY_NAME[f"u_rows{r}"])[0] for r in (31, 32, 33, 65)] == [31, 32, 33, 65]
    ladder = [c for c in I.TABLE if "ladder" in c.tags]
    assert sorted(c.ldo // 8 for c in ladder) == [255, 256, 257, 263, 264, 265, 494, 512]
    for c in ladder:
        k = c.a
        assert c.C * k * k <= c.ldo <= 4096 and I.geometry(c)[0] == 7 and c.pad > 0
    for c in I.TABLE:
        if c.op == "unfold":
            assert c.ldo % 8 == 0 and c.C * c.a * c.a <= c.ldo and 0 <= c.pad < c.a
        else:
            assert c.H % c.a == 0 and c.W % c.a == 0
    assert I.BY_NAME["u_nch5"].ldo // 8 == 5 and I.BY_NAME["u_k1_nch1"].ldo // 8 == 1
    assert max(c.C for c in I.TABLE) > I.U8_LDS_MAX_C
    assert any(c.B * c.C * c.H * c.W % 8 for c in I.TABLE if c.op == "unfold")
    h = I.HOLE
    assert h.H + h.pad == 32768 and I.geometry(h)[0] == 262137
    assert len(I.BY_NAME) == len(I.TABLE)
