"""The exact-integer GEMM probes of oracle/gemm_probes.py, checked on the CPU, for every row of the table tests/test_hip_gemm_edges.py runs:

(a) exactness: every expected value, and every intermediate a kernel rounds (t = lora_scale * A P^T, the 16-bit output the fused reductions
    re-read), makes the round trip through bf16, fp16 and f32 — so torch.equal is the right comparison on the device;
(b) the fault models the probes and the guard bands of tests/guard_bands.py exist for each change a compared element or a band: an output
    shifted by 4 columns, a dropped last row, a dropped last K tile, a dropped K2 segment (or rank-r term), row M of a padded operand added
    into a reduction, an ignored ldw, an 8-wide store at n = N - 4.

The last test calls gsl_gemm_tile_choice — host code of the library — and so needs the cross-compiled libgslora_hip.so (build() of
__graft_entry__.py; no GPU), as tests/test_proto_l2_host.py does; everything else here is pure torch."""
import functools

import pytest
import torch

from guard_bands import BAND, Banded
from oracle import gemm_probes as G

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
GEMM_LIKE = [c.name for c in G.TABLE if c.kind in ("gemm", "lora", "mulgrad")]
REDUCTIONS = [c.name for c in G.TABLE if c.kind in ("mulgrad", "lgrad")]


@functools.lru_cache(maxsize=2)
def built(name):
    """(case, operands, accumulator) — built once per table row, shared, never written to."""
    case = G.BY_NAME[name]
    d = G.make(case)
    acc = None if case.kind == "lgrad" else (G.accumulate(d) if case.kind == "gemm" else G.accumulate_lora(d))
    return case, d, acc


def keep_mask(case):
    return torch.randint(0, 2, (case.M, case.N), generator=torch.Generator().manual_seed(case.M + case.N)).float()


def exact_outputs(case, d, acc):
    """name -> float64 reference of everything the device test compares with torch.equal."""
    keep = keep_mask(case)
    if case.kind == "gemm":
        names = [n for n in G.EXACT_GEMM if n != "qkv_hm" or (case.N % 192 == 0 and case.M % G.PATCH_T == 0)]
        return {n: G.epilogue(n, acc, d, keep if n.endswith("_drop") else None) for n in names}
    if case.kind == "lora":
        out = {n: G.epilogue_lora(n, acc, d, keep if n.endswith("_drop") else None) for n in G.EXACT_LORA}
        out["tout"] = G.tout(d)
        return out
    if case.kind == "mulgrad":
        o, g1, g2 = G.mulgrad(d, case.r)
        return {"out": o, "tout": G.tout(d), "G1": g1, "G2": g2}
    return {f"G@{col}": G.lora_grad(d, case.r, col) for col in (0, case.r, 2 * case.r)}


@pytest.mark.parametrize("name", [c.name for c in G.TABLE])
def test_operands_follow_the_recipe(name):
    case, d, _ = built(name)
    if case.kind == "lgrad":
        return
    A = torch.cat([d["A1"]] + ([d["A2"]] if case.K2 else []), 1)
    assert set(A.unique().tolist()) <= {-1.0, 0.0, 1.0}
    nz = (A != 0).view(case.M, -1, 64).sum(-1)
    assert (nz >= 1).all(), "a 64-wide K tile of a row without a non-zero"
    assert (nz.sum(-1) <= 64).all(), "more than 64 non-zeros in a row"
    assert set(d["aux"].unique().tolist()) <= {-2.0, -1.0, 1.0, 2.0}


@pytest.mark.parametrize("name", [c.name for c in G.TABLE])
def test_every_expected_value_is_exact_in_every_dtype(name):
    case, d, acc = built(name)
    for what, ref in exact_outputs(case, d, acc).items():
        for dt in DTYPES:
            if what in ("G1", "G2") or what.startswith("G@"):
                dt = torch.float32      # the gradient bucket is f32
            assert G.survives(ref, dt), (name, what, dt, ref.abs().max().item())
    for v in d.values():      # the operands themselves
        assert all(G.survives(v.double(), dt) for dt in DTYPES), name
    if case.kind in ("lora", "mulgrad"):
        assert all(G.survives(G.lora_t(d), dt) for dt in DTYPES), (name, "t")
    if case.kind in ("mulgrad", "lgrad"):      # the partial sums of any summation order: below 2^24 in units of the finest step (1/8)
        o = G.mulgrad(d, case.r)[0] if case.kind == "mulgrad" else d["Y"].double()
        assert case.M * o.abs().max().item() * 8 < 2 ** 24, name


# ---------------------------------------------------------------------------------------------------------------- fault models
def placements(case, pad_ld_to=4):
    """The three output placements of the device test: contiguous between bands, a column block of padded rows, cls rows."""
    N = case.N
    ld = -(-(N + 40) // pad_ld_to) * pad_ld_to
    return {"contiguous": dict(), "padded": dict(ld=ld, col0=8, pad_rows=2), "cls_rows": dict(ld=7 * N)}


def kernel_store(b, ref, shift=0, rows=None, wide_tail=False):
    """What a kernel with the given fault leaves in the buffer of b: it addresses row m, column n as base + m * ld + n. A contiguous
    placement is one row of M * N elements to the helper and M rows of N elements to the kernel."""
    M, N = ref.shape
    ld = N if b.rows == 1 and M > 1 else b.row_step * b.ld
    rows = M if rows is None else rows
    start = BAND + b.col0 + torch.arange(rows) * ld + shift
    if wide_tail:      # the 8-wide store of the column group at n = N - 4: four elements behind column N - 1, before the rows land
        b.buf[(start[:, None] + N + torch.arange(4)[None, :]).reshape(-1)] = 0
    b.buf[(start[:, None] + torch.arange(N)[None, :]).reshape(-1)] = ref[:rows].reshape(-1).to(b.buf.dtype)


def caught(b, ref):
    return not (torch.equal(b.view.double().view(ref.shape), ref) and b.bands_intact())


@pytest.mark.parametrize("name", GEMM_LIKE)
def test_store_faults_change_a_compared_element_or_a_band(name):
    case, d, acc = built(name)
    ref = (G.epilogue("store", acc, d) if case.kind == "gemm" else acc)
    for where, kw in placements(case).items():
        def run(**fault):
            b = Banded((case.M, case.N), torch.bfloat16, device="cpu", **kw)
            kernel_store(b, ref, **fault)
            return b
        assert not caught(run(), ref), (name, where, "a correct store must pass")
        assert caught(run(shift=4), ref), (name, where, "output shifted by 4 columns")
        assert caught(run(rows=case.M - 1), ref), (name, where, "last row dropped")
        b = run(wide_tail=True)
        assert torch.equal(b.view.double().view(ref.shape), ref) and not b.bands_intact(), (name, where, "8-wide store at n = N - 4: only a band shows it")


@pytest.mark.parametrize("name", GEMM_LIKE)
def test_operand_faults_change_a_compared_element(name):
    case, d, acc = built(name)
    lora = case.kind != "gemm"
    epi = (lambda a: a) if lora else (lambda a: G.epilogue("store", a, d))
    ref = epi(acc)
    dropped = G.accumulate_lora(d, drop_last_k_tile=True) if lora else G.accumulate(d, drop_last_k_tile=True)
    assert not torch.equal(epi(dropped), ref), (name, "last K tile dropped")
    if lora:
        assert not torch.equal(epi(G.accumulate_lora(d, drop_rank_term=True)), ref), (name, "rank-r term dropped")
    elif case.K2:
        assert not torch.equal(epi(G.accumulate(d, drop_k2=True)), ref), (name, "K2 segment dropped")
    # ldw ignored: W is the second column block of a [N, 2 K] matrix whose other half is a band; a kernel that steps rows by K reads it
    K = case.K1
    wide = Banded((case.N, K), torch.float32, d["W1"], ld=2 * K, col0=K, device="cpu")
    first = BAND + K
    w_bad = wide.buf[first:first + case.N * K].view(case.N, K)
    bad = epi((G.accumulate_lora if lora else G.accumulate)(dict(d, W1=w_bad)))
    assert not torch.equal(bad, ref), (name, "ldw ignored")
    assert torch.equal(epi((G.accumulate_lora if lora else G.accumulate)(dict(d, W1=wide.view))), ref)


@pytest.mark.parametrize("name", REDUCTIONS)
def test_a_row_too_many_or_too_few_changes_a_reduction(name):
    case, d, _ = built(name)
    M, N, r = case.M, case.N, case.r
    band = lambda n: torch.full((n,), G.BAND_FILL)      # row M of an operand between bands or with pad rows: the band's fill
    if case.kind == "mulgrad":
        _, g1, g2 = G.mulgrad(d, r)
        _, b1, b2 = G.mulgrad(d, r, extra_row=(band(N), band(16), band(N), band(16)))
        assert not torch.equal(b1, g1) and not torch.equal(b2, g2), (name, "row M added into G1 / G2")
        short = {k: (v[:M - 1] if v.shape[0] == M else v) for k, v in d.items()}
        _, s1, s2 = G.mulgrad(short, r)
        assert not torch.equal(s1, g1) and not torch.equal(s2, g2), (name, "last row dropped from G1 / G2")
    else:
        for col in (0, r, 2 * r):
            g = G.lora_grad(d, r, col)
            assert not torch.equal(G.lora_grad(d, r, col, extra_row=(band(N), band(64))), g), (name, "row M added")
            short = dict(d, Y=d["Y"][:M - 1], U=d["U"][:M - 1])
            assert not torch.equal(G.lora_grad(short, r, col), g), (name, "last row dropped")


def test_lora_grad_batch_entries_are_exact():
    for e in G.make_lgrad_batch():
        for col in (0, 16):
            assert G.survives(G.lora_grad(e, e["r"], col), torch.float32)


def test_banded_placement_covers_pad_columns_and_rows():
    b = Banded((3, 8), torch.float32, ld=16, col0=8, row_step=2, pad_rows=1, device="cpu")
    assert b.bands_intact() and b.unwritten() == 24
    b.view.fill_(1.0)
    assert b.bands_intact() and b.unwritten() == 0
    for off in (BAND + 7, BAND + 16, BAND + 16 + 8, BAND + 5 * 16 + 3, BAND - 1, BAND + 6 * 16):      # pad column, row between, row behind, bands
        c = Banded((3, 8), torch.float32, ld=16, col0=8, row_step=2, pad_rows=1, device="cpu")
        c.buf[off] = 0.0
        assert not c.bands_intact(), off
    src = torch.arange(24.0).view(3, 8)
    i = Banded((3, 8), torch.float32, src, ld=16, col0=8, pad_rows=2, device="cpu")
    assert torch.equal(i.view, src) and i.bands_intact()
    assert torch.isnan(i.buf).sum() == i.buf.numel() - 24
    i.view[1, 2] = -1.0
    assert not i.bands_intact()


# ---------------------------------------------------------------------------------------------------------------- the tile rule (host code)
def rule_as_documented(M, N, K, lora=False, has_out2=False):
    """The shape-to-kernel rule as csrc/gemm.hip documents it, restated: variant 1 / 3 / 8 from the 256x256 tile count, the 64-row ring kernel up
    to 256 tiles of 128x128, its wide form above 768 tiles of 64x64 and its K-split form from K = 1024 on at most 256 tiles."""
    up = lambda a, b: -(-a // b)
    if has_out2 and not lora:
        return "RING256X128"
    few = M < 1024 or up(M, 256) * up(N, 256) < 128
    if few and up(M, 128) * up(N, 128) <= 256:
        t64 = up(M, 64) * up(N, 64)
        return "RING64_WIDE" if t64 > 768 else "RING64_KSPLIT" if K >= 1024 and t64 <= 256 else "RING64"
    if lora:
        return "P8"
    return "128" if few else ("P8" if N >= 512 else "RING256X128")


def test_tile_choice_names_every_table_row_and_follows_the_documented_rule():
    """gsl_gemm_tile_choice is host code: the rows of the table, and a sweep of shapes around every threshold of the rule, on the CPU."""
    from gslora_hip import _lib as L
    from gslora_hip import ops
    for c in G.TABLE:
        if c.tile is None:
            continue
        K, lora = c.K1 + c.K2, c.kind == "lora"
        if c.f32:
            assert ops.gemm_tile_choice(c.M, c.N, K, torch.float32) == getattr(L, "TILE_" + c.tile), c.name
            x3 = "F32X3_MFMA" if c.tile == "F32_MFMA" else c.tile
            assert ops.gemm_tile_choice(c.M, c.N, K, torch.float32, f32_mode="x3") == getattr(L, "TILE_" + x3), c.name
        else:
            for dt in (torch.bfloat16, torch.float16):
                assert ops.gemm_tile_choice(c.M, c.N, K, dt, in_kernel_lora=lora) == getattr(L, "TILE_" + c.tile), c.name
    Ms = (1, 63, 64, 65, 130, 900, 1023, 1024, 1541, 1576, 1800, 2600, 8192, 9000, 16200, 32512, 32513, 32600, 33490, 201728)
    Ns = (4, 64, 68, 124, 128, 132, 192, 388, 508, 512, 516, 768, 2048, 2052, 4100, 4228)
    for M in Ms:
        for N in Ns:
            for K in (64, 1024, 1088):
                for lora in (False, True):
                    want = rule_as_documented(M, N, K, lora)
                    assert ops.gemm_tile_choice(M, N, K, torch.bfloat16, in_kernel_lora=lora) == getattr(L, "TILE_" + want), (M, N, K, lora)
            assert ops.gemm_tile_choice(M, N, 64, torch.float16, has_out2=True) == L.TILE_RING256X128
            f32 = "F32_MFMA" if N >= 128 and M >= 64 else "F32_VALU"
            assert ops.gemm_tile_choice(M, N, 64, torch.float32) == getattr(L, "TILE_" + f32), (M, N)
    lib = L.load()
    assert lib.gsl_gemm_tile_choice(0, 64, 64, L.BF16, 0, 0) == -1 and lib.gsl_gemm_tile_choice(64, 64, 64, L.F32, 0, 1) == -1
    assert lib.gsl_gemm_tile_choice(64, 64, 64, 7, 0, 0) == -1


def test_runner_asks_the_library_which_rows_take_the_in_kernel_lora_form(monkeypatch):
    """ViTRunner.lora_in_kernel asks gsl_gemm_tile_choice for the few-row case. The yardstick is the expression it held before, a
    restatement of the tile rule with its own copies of the 256 and 128 tile sizes: same answer at every shape, dtype and rank, with the
    few-row form on and off, and from the memo as from the first call."""
    from gslora_hip import vit_runner as R

    def old(runner, dtype, rows, N):
        if dtype not in R.OP16 or runner._rank > 16:
            return False
        if rows >= R.INK_MIN_ROWS:
            return True
        if N is None or not R.INK_SMALL:
            return False
        t256 = ((rows + 255) // 256) * ((N + 255) // 256)
        t128 = ((rows + 127) // 128) * ((N + 127) // 128)
        return (rows < 1024 or t256 < 128) and t128 <= 256

    runner = R.ViTRunner(None)
    seen = set()
    for ink_small in (True, False):
        monkeypatch.setattr(R, "INK_SMALL", ink_small)
        for rank in (8, 32):
            runner._rank = rank
            for dtype in (torch.bfloat16, torch.float16, torch.float32):
                for rows in (1, 63, 64, 111, 1023, 1024, 4096, 8191, 8192, 33490):
                    for N in (64, 128, 256, 512, 2048):
                        for K in (128, 2048):      # (K picks among the three ring tiles only)
                            for again in range(2):
                                got = runner.lora_in_kernel(dtype, rows, N, K)
                                assert got is old(runner, dtype, rows, N), (ink_small, rank, dtype, rows, N, K, again)
                                seen.add(got)
    assert seen == {True, False}
