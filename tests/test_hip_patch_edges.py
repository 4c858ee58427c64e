"""The four patch gathers (csrc/patch.hip: gsl_patchify, gsl_patchify_u8, gsl_unfold_patches, gsl_unfold_patches_u8) at their edges, on the
case table of oracle/input_probes.py, through the C ABI, for f32, bf16 and fp16 outputs. Every comparison is of bits with
store(reference): a gather computes nothing, so this file has no tolerance. (A NaN compares as a NaN: the converts are free in the payload.)

Paths reached. Patchify: H != W both ways, one patch, C = 1 / 3 (the wide 8-pixel form of the u8 kernel) and C = 2 / 4 / 17 (the narrow
form; 17: value table in global memory), p = 1, 3, 4, 8, 16, a second grid-stride trip of the narrow and of the wide thread map, an
image pointer one byte off its 8-byte boundary (the launch falls back to the narrow kernel). Unfold: Lh != Lw both ways, stride > k,
stride = 1 with pad = k - 1, k = 1, one window per image, nch = ldo / 8 of 1, 2, 5 (odd), the wide rows nch = 255, 256, 257, 512 (step_r = 0
from 257 on) each with a longer zero fill, B T = 31, 32, 33, 65 around UNF_ROWS, C = 17, and for bytes both layouts, C = 2 and 4 in NHWC
and images whose byte count is no multiple of 8 (the last, partial word). H = 32767 with pad = 1 in a test of its own.

What a kernel may touch. Float images sit between NaN bands: an out-of-image tap that loads instead of giving 0 is a NaN in the first
rows of image 0 or the last of the last image. Byte images sit between bands of 0x5A; the `leak` batches hold the other 255 values and
their table has table[c][0x5A] = NaN, so a tap on a band byte is a NaN; the `all` batches hold every byte value in every channel.
Both tables have table[c][0] != 0: a padding zero must be +0, not the value of byte 0. The value tables are banded inputs as well.
Outputs are NaN-sentinel buffers, contiguous and as the first rows of a longer buffer: bands intact, no element unwritten, inputs
unchanged. The f32 outputs come from the index image (element i holds i + 1): every element names its source pixel.

Saturation: 65520, -1e6, +-Inf, NaN and -0 planted in the image, and in the value table, must store as store() says in all three
formats (fp16: 0x7bff, 0xfbff, Inf and NaN kept; csrc/gsl_common.h).

Findings this file was written against.
 1. The H + pad hole of gsl_unfold_patches (found by reading; test_h_32767_with_padding). The K-padding columns were marked by a table
    entry with kh = 0x7fff alone. At H + pad >= 32768 the first window row (h0 = -pad) has h = 32767 - pad < H, in range, and so is
    w = w0 for every window but the first of a row: the padding column loaded img[base], row -pad of the image — memory in front of
    it — and stored that instead of 0. Fixed in the table, not by a refusal: the entry now also carries kw = 0xffff, and
    w = w0 + 65535 >= 65535 - 63 is beyond every accepted W < 32768 whatever H is (pad < k <= 64 since C k k <= 4096). The gather loop is
    unchanged (no instruction added), every H < 32768 stays usable, and gsl_unfold_patches_u8, which tests te.y >= 0 and never had the
    hole, needs no new rule. The test uses full-size banded buffers, so the unfixed code would have read a NaN of the band, never
    memory outside the allocation.
 2. Nothing else: every other case passed as written."""
import functools

import pytest
import torch

from guard_bands import NAN_SENTINEL, Banded, ptr
from oracle import input_probes as I

pytestmark = pytest.mark.gpu

F32, BF16, F16 = I.F32, I.BF16, I.F16
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
CASES = list(I.TABLE)
PLACEMENTS = ("contiguous", "rows")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    from gslora_hip import ops as _ops
    from gslora_hip import _lib
    _lib.load()
    return _ops


def ident(v):
    return NAME.get(v, getattr(v, "name", str(v)))


def stream():
    return torch.cuda.current_stream().cuda_stream


def case_of(name):
    return I.HOLE if name == I.HOLE.name else I.BY_NAME[name]


@functools.lru_cache(maxsize=4)
def source(name, what):
    """The CPU inputs of a case, built once, shared, never written to."""
    return I.make(case_of(name), what)


@functools.lru_cache(maxsize=4)
def expected(name, what, dt):
    """bits(store(reference)) on the device."""
    case, src = case_of(name), source(name, what)
    img = src if torch.is_tensor(src) else I.u8_image(*src)
    return I.bits(I.store(I.reference(case, img), dt)).cuda()


def Out(case, dt, placement):
    """contiguous: exactly the output between the bands. rows: the first rows of a buffer three rows longer."""
    T, cols = I.geometry(case)
    if placement == "contiguous":
        return Banded((case.B * T, cols), dt, sentinel=NAN_SENTINEL[dt])
    return Banded((case.B * T, cols), dt, ld=cols, pad_rows=3, sentinel=NAN_SENTINEL[dt])


def settled(what, ins, out, want):
    torch.cuda.synchronize()
    for b in ins:
        assert b.bands_intact(), (what, "an input changed")
    assert out.bands_intact(), (what, "a store outside the output")
    assert out.unwritten() == 0, (what, "unwritten elements")
    got = I.bits(out.view)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError((what, f"{len(bad)} elements differ, the first at (row, column) {bad[0].tolist()}"))


def placements(case):
    return PLACEMENTS[:1] if "sweep" in case.tags else PLACEMENTS


def run_float(ops, case, dt, what, placement):
    from gslora_hip import _lib as L
    lib = L.load()
    img = source(case.name, what)
    x, out = Banded(img.shape, F32, img), Out(case, dt, placement)
    if case.op == "patchify":
        L.check(lib.gsl_patchify(ptr(x), ptr(out), case.B, case.C, case.H, case.W, case.a, ops.code(dt), stream()), "gsl_patchify")
    else:
        L.check(lib.gsl_unfold_patches(ptr(x), ptr(out), case.B, case.C, case.H, case.W, case.a, case.stride, case.pad, case.ldo, ops.code(dt),
                                       stream()), "gsl_unfold_patches")
    settled((case.name, NAME[dt], what, placement), (x,), out, expected(case.name, what, dt))
    return out


def run_u8(ops, case, dt, what, layout, placement, off=0):
    """off: the image starts `off` bytes behind an 8-byte boundary (the bytes around it are band bytes)."""
    from gslora_hip import _lib as L
    lib = L.load()
    u, tab = source(case.name, what)
    flat = u.reshape(-1) if layout == "nchw" else I.nhwc_bytes(u)
    if off:
        flat = torch.cat([torch.full((off,), I.BAND_BYTE, dtype=torch.uint8), flat, torch.full((8 - off,), I.BAND_BYTE, dtype=torch.uint8)])
    x, t, out = Banded(flat.shape, torch.uint8, flat), Banded(tab.shape, F32, tab), Out(case, dt, placement)
    code = L.U8_NCHW if layout == "nchw" else L.U8_NHWC
    if case.op == "patchify":
        L.check(lib.gsl_patchify_u8(ptr(x) + off, code, ptr(t), ptr(out), case.B, case.C, case.H, case.W, case.a, ops.code(dt), stream()),
                "gsl_patchify_u8")
    else:
        assert off == 0
        L.check(lib.gsl_unfold_patches_u8(ptr(x), code, ptr(t), ptr(out), case.B, case.C, case.H, case.W, case.a, case.stride, case.pad, case.ldo,
                                          ops.code(dt), stream()), "gsl_unfold_patches_u8")
    settled((case.name, NAME[dt], what, layout, placement, off), (x, t), out, expected(case.name, what, dt))
    return out


# ---------------------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("dt", I.DTYPES, ids=ident)
@pytest.mark.parametrize("case", CASES, ids=ident)
def test_float_gather(ops, case, dt):
    """f32: the index image (every element names its source pixel). 16-bit: the value image."""
    what = "index" if dt == F32 else "value"
    for placement in placements(case):
        run_float(ops, case, dt, what, placement)


@pytest.mark.parametrize("dt", I.DTYPES, ids=ident)
@pytest.mark.parametrize("case", CASES, ids=ident)
def test_u8_gather(ops, case, dt):
    """Both layouts; the band-leak bytes (arbitrary table, NaN at the band byte) in both placements, all byte values (affine table)
    contiguous. The sweep cases run the band-leak bytes only."""
    for layout in ("nchw", "nhwc"):
        for placement in placements(case):
            run_u8(ops, case, dt, "leak", layout, placement)
        if "sweep" not in case.tags:
            run_u8(ops, case, dt, "all", layout, "contiguous")


@pytest.mark.parametrize("dt", I.DTYPES, ids=ident)
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_misaligned_u8_image_takes_the_narrow_kernel_and_gives_the_same_bits(ops, layout, dt):
    """p = 8, C = 3 with the image one byte behind an 8-byte boundary: the wide form's aligned 8-byte loads would take the band byte in
    front and shift every pixel; the launch must use the one-byte form."""
    case = I.BY_NAME["p_wide_16x24"]
    assert case.a == 8 and case.C == 3
    a = run_u8(ops, case, dt, "leak", layout, "contiguous", off=1)
    b = run_u8(ops, case, dt, "leak", layout, "contiguous")
    assert torch.equal(I.bits(a.view), I.bits(b.view))


# ---------------------------------------------------------------------------------------------------------------- saturation
@pytest.mark.parametrize("dt", I.DTYPES, ids=ident)
@pytest.mark.parametrize("name", I.SATURATION)
def test_saturation_inf_and_nan_store_as_the_format_says(ops, name, dt):
    case = I.BY_NAME[name]
    img = source(name, "value_sat")
    for v in I.SPECIALS[:4]:
        assert (img == v).any()
    out = run_float(ops, case, dt, "value_sat", "contiguous")
    got = out.view.float()
    assert torch.isnan(got).any() and (got == float("inf")).any() and (got == float("-inf")).any()
    if dt == F16:
        assert (got == 65504.0).any() and (got == -65504.0).any()          # 65520 and -1e6, saturated
        assert int(torch.isinf(got).sum()) == int(torch.isinf(I.reference(case, img)).sum())      # and nothing finite became Inf
    for layout in ("nchw", "nhwc"):
        run_u8(ops, case, dt, "leak_sat", layout, "contiguous")


# ---------------------------------------------------------------------------------------------------------------- H + pad >= 32768
@pytest.mark.parametrize("dt", I.DTYPES, ids=ident)
def test_h_32767_with_padding(ops, dt):
    """C = 1, W = 8, k = 3, stride = 1, pad = 1, H = 32767 (finding 1): the call runs, the K padding (columns 9 .. 15) is zero in all
    262137 rows and the bits are store(unfold_ref). The image and the output are real, full-size, banded buffers."""
    case = I.HOLE
    out = run_float(ops, case, dt, "index" if dt == F32 else "value", "contiguous")
    assert out.view.shape == (262137, 16)
    assert int(torch.count_nonzero(I.bits(out.view)[:, case.C * case.a * case.a:])) == 0
    for layout in ("nchw", "nhwc"):
        o = run_u8(ops, case, dt, "leak", layout, "contiguous")
        assert int(torch.count_nonzero(I.bits(o.view)[:, case.C * case.a * case.a:])) == 0


# ---------------------------------------------------------------------------------------------------------------- the Python wrappers
@pytest.mark.parametrize("dt", I.DTYPES, ids=ident)
@pytest.mark.parametrize("case", [c for c in CASES if "nonsquare" in c.tags], ids=ident)
def test_python_wrappers_on_the_non_square_cases(ops, case, dt):
    """ops.patchify / ops.unfold_patches (the K padded to a multiple of 64) from floats and from bytes of both layouts."""
    def call(img, table=None):
        if case.op == "patchify":
            return ops.patchify(img, case.a, dt, table=table)
        return ops.unfold_patches(img, case.a, case.stride, case.pad, dt, table=table)

    def want(img):
        ref = I.patchify_ref(img, case.a) if case.op == "patchify" else I.unfold_ref(img, case.a, case.stride, case.pad, I.kpad(case.C, case.a))
        return I.bits(I.store(ref, dt)).cuda()
    img = source(case.name, "index" if dt == F32 else "value")
    got = call(img.cuda())
    assert got.dtype == dt and torch.equal(I.bits(got), want(img))
    u, tab = source(case.name, "all")
    w = want(I.u8_image(u, tab))
    for src in (u.cuda(), u.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)):
        assert torch.equal(I.bits(call(src, tab.cuda())), w)
