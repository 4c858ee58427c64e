"""GPU edge tests of gst_wgrad (libgslora_train.so): dW[n, k] (+)= c sum_m Y[m, n] X[m, k], db[n] (+)= c sum_m Y[m, n].

Every operand, output and the workspace sits between the guard bands of tests/guard_bands.py, contiguous or as a column block of a wider
tensor (ldy = N + 64, ldx = 2 K, ldw = K + 40): every band must be intact and every input unchanged.

Exact-integer probes: operand values are integers in [-3, 3] (exact in f32, bf16 and fp16), |sum| <= 9 M < 2^24 for every M used, so the f32
result is exact whatever the order of the sum and is compared with torch.equal against the exact product (float64 on integers); the same
holds with gscale = {2^11, 2^-11} and with accumulate = 1 onto an integer dW. The integers are drawn independently per element, so every
row, column, slab, split and tile carries its own values. Fault models the table catches, each a one-line mutation of csrc/train.hip:
  a slab dropped           the first `rb += KS` -> `rb += 2 * KS` in the row-slab loop (every split of more than one slab)
  a row too many           `ma < r1` -> `ma <= r1` in gload (M = rows_per_split - 1, 31, 63: the row behind the split is a live row or the NaN band)
  a split counted twice    `sp < nsplit` -> `sp <= nsplit` in the reduce, or `r0 = split * rps` -> `(split ? split - 1 : 0) * rps` (M > rows_per_split)
  a tile column off        `k0 = (tile % tiles_k) * WG_TILE` -> `(tile % tiles_n) * WG_TILE` (N != K with more than one tile)
  db from the wrong tile   `k0 == 0` -> `k0 == WG_TILE` in do_db (K = 64: no such tile, db unwritten; K > 128: written twice is harmless,
                           written by a tile that skipped rows is not), or `n0 + tid` -> `k0 + tid` in the db store
"""
import pytest
import torch

from guard_bands import Banded

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def LT():
    from gslora_hip import _lib_train
    return _lib_train


def ints(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, shape, generator=g).float()


def run_case(dtype, M, N, K, *, db, gscale, placed, accumulate, seed, Yv=None, Xv=None):
    """One banded call. -> (dW, db or None, want_dW, want_db) on the device, f32; asserts the bands."""
    lt = LT()
    Yv = ints((M, N), seed) if Yv is None else Yv
    Xv = ints((M, K), seed + 1) if Xv is None else Xv
    Y = Banded((M, N), dtype, Yv, **(dict(ld=N + 64, col0=32) if placed else {}))
    X = Banded((M, K), dtype, Xv, **(dict(ld=2 * K, col0=32) if placed else {}))
    w0 = ints((N, K), seed + 2) if accumulate else None
    b0 = ints((N,), seed + 3) if accumulate else None
    dW = Banded((N, K), torch.float32, w0, **(dict(ld=K + 40, col0=8) if placed else {}))
    dB = Banded((N,), torch.float32, b0) if db else None
    ws = Banded((lt.wgrad_ws_elems(M, N, K, dtype),), torch.float32)
    gs = Banded((4,), torch.float32, torch.tensor([2.0 ** 11, 2.0 ** -11, 0.0, 0.0])) if gscale else None
    lt.wgrad(Y.view, X.view, dW.view, dB.view if db else None, accumulate=accumulate, ws=ws.view, gscale=gs.view if gscale else None)
    torch.cuda.synchronize()
    assert Y.bands_intact() and X.bands_intact(), "an input changed"
    assert ws.bands_intact(), "a store outside the workspace"
    assert gs is None or gs.bands_intact()
    if accumulate:
        assert dW.outside_intact() and (dB is None or dB.outside_intact()), "a store outside an accumulated output"
    else:
        assert dW.bands_intact() and dW.unwritten() == 0 and (dB is None or (dB.bands_intact() and dB.unwritten() == 0))
    c = 2.0 ** -11 if gscale else 1.0
    Yd, Xd = Y.view.double(), X.view.double()      # the stored operand values
    want_w = (Yd.t() @ Xd) * c + (w0.cuda().double() if accumulate else 0.0)
    want_b = Yd.sum(0) * c + (b0.cuda().double() if accumulate else 0.0)
    return dW.view.clone(), (dB.view.clone() if db else None), want_w, want_b


def check_exact(dtype, M, N, K, flags, seed):
    db, gscale, placed, accumulate = flags
    got_w, got_b, want_w, want_b = run_case(dtype, M, N, K, db=db, gscale=gscale, placed=placed, accumulate=accumulate, seed=seed)
    what = f"M={M} N={N} K={K} db={db} gscale={gscale} placed={placed} accumulate={accumulate}"
    assert torch.equal(got_w.double(), want_w), f"dW {what}: {int((got_w.double() != want_w).sum())} elements differ"
    if db:
        assert torch.equal(got_b.double(), want_b), f"db {what}"


def flag_cycle(i):
    """(db, gscale, placed, accumulate): all sixteen combinations over sixteen consecutive cases."""
    return bool(i & 1), bool(i & 2), bool(i & 4), bool(i & 8)


def split_edge_rows(dtype, N, K):
    """For the plans at M = 700 and M = 1300: rows_per_split - 1, rows_per_split, rows_per_split + 1, the Ms themselves and, next below
    each, an M whose own plan leaves one row to its last split."""
    lt, out = LT(), []
    for M0 in (700, 1300):
        _, _, nsplit, rps = lt.wgrad_plan(M0, N, K, dtype)
        assert nsplit > 1 and rps % 32 == 0 and (nsplit - 1) * rps < M0 <= nsplit * rps
        out += [rps - 1, rps, rps + 1, M0]
        one = next(m for m in range(M0, 1, -1) if lt.wgrad_plan(m, N, K, dtype)[2] > 1 and (m - 1) % lt.wgrad_plan(m, N, K, dtype)[3] == 0)
        out.append(one)
    return out


@pytest.mark.parametrize("name", list(DTYPES))
def test_exact_integer_products_over_row_counts_and_split_edges(name):
    dtype = DTYPES[name]
    N, K = 192, 320      # more than one tile each way, a half tile at both edges, N != K
    rows = [1, 3, 31, 32, 33, 63, 64, 65] + split_edge_rows(dtype, N, K)
    assert max(rows) * 9 < 2 ** 24
    for i, M in enumerate(rows):
        check_exact(dtype, M, N, K, flag_cycle(i), seed=1000 + i)
        check_exact(dtype, M, N, K, flag_cycle(15 - i % 16), seed=2000 + i)
    # one tile, and the FFN's 64 tiles: the split edges again
    for N2, K2 in ((64, 64), (2048, 512)):
        for i, M in enumerate(split_edge_rows(dtype, N2, K2)[:5]):
            check_exact(dtype, M, N2, K2, flag_cycle(i + 3), seed=3000 + i)


@pytest.mark.parametrize("name", list(DTYPES))
def test_exact_integer_products_over_tile_edges_and_model_widths(name):
    dtype = DTYPES[name]
    tn, tk, _, _ = LT().wgrad_plan(65, 128, 128, dtype)
    widths = lambda t: sorted({64, t - 64, t, t + 64, 2 * t + 64, 128, 256, 512, 2048} - {0})
    i = 0
    for N in widths(tn):      # N and K independently
        check_exact(dtype, 65, N, tk, flag_cycle(i), seed=4000 + i)
        i += 1
    for K in widths(tk):
        check_exact(dtype, 65, tn, K, flag_cycle(i), seed=4000 + i)
        i += 1
    for N, K in ((2048, 512), (512, 2048), (tn + 64, 2 * tk + 64), (2 * tn + 64, tk + 64)):      # the FFN's own shapes, both edges at once
        check_exact(dtype, 33, N, K, flag_cycle(i), seed=4000 + i)
        i += 1


@pytest.mark.parametrize("name", list(DTYPES))
def test_every_flag_combination_at_one_shape_and_two_calls_give_the_same_bits(name):
    dtype = DTYPES[name]
    for i in range(16):
        check_exact(dtype, 131, 192, 320, flag_cycle(i), seed=5000 + i)
    g = torch.Generator().manual_seed(7)
    Yv, Xv = torch.randn(700, 256, generator=g), torch.randn(700, 192, generator=g)
    a = run_case(dtype, 700, 256, 192, db=True, gscale=False, placed=True, accumulate=False, seed=0, Yv=Yv, Xv=Xv)
    b = run_case(dtype, 700, 256, 192, db=True, gscale=False, placed=False, accumulate=False, seed=0, Yv=Yv, Xv=Xv)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "the bits depend on the call or on the placement"


@pytest.mark.parametrize("name", ["f32", "fp16"])
def test_a_captured_graph_replays_the_same_bits(name):
    lt, dtype = LT(), DTYPES[name]
    M, N, K = 700, 192, 320
    g = torch.Generator().manual_seed(17)
    Y, X = torch.randn(M, N, generator=g).cuda().to(dtype), torch.randn(M, K, generator=g).cuda().to(dtype)
    ws = torch.empty(lt.wgrad_ws_elems(M, N, K, dtype), device="cuda")
    gs = torch.tensor([2.0 ** 11, 2.0 ** -11, 0.0, 0.0], device="cuda")
    eager_w, eager_b = torch.empty(N, K, device="cuda"), torch.empty(N, device="cuda")
    lt.wgrad(Y, X, eager_w, eager_b, ws=ws, gscale=gs)
    dW, db = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lt.wgrad(Y, X, dW, db, ws=ws, gscale=gs)
    for _ in range(2):
        dW.fill_(float("nan"))
        db.fill_(float("nan"))
        ws.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dW, eager_w) and torch.equal(db, eager_b)
    gs.copy_(torch.tensor([2.0 ** 9, 2.0 ** -9, 0.0, 0.0]))      # the scale is read from device memory: a replay follows it
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dW, eager_w * 4.0)


def elementwise_bound(Y, X):
    """M * 2^-23 * sum_m |y x| per element: the worst case of an f32 sum of M exactly representable products in any order, with one bit of
    slack for the matrix core's internal rounding."""
    return Y.shape[0] * 2.0 ** -23 * (Y.double().abs().t() @ X.double().abs())


@pytest.mark.parametrize("name", list(DTYPES))
def test_random_values_stay_within_the_f32_summation_bound(name):
    dtype = DTYPES[name]
    M, N, K = 1300, 768, 256
    g = torch.Generator().manual_seed(11)
    Yv, Xv = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    got_w, got_b, want_w, want_b = run_case(dtype, M, N, K, db=True, gscale=False, placed=False, accumulate=False, seed=0, Yv=Yv, Xv=Xv)
    Ys, Xs = Yv.cuda().to(dtype), Xv.cuda().to(dtype)
    bound = elementwise_bound(Ys, Xs)
    ratio = ((got_w.double() - want_w).abs() / bound).max().item()
    rb = ((got_b.double() - want_b).abs() / (M * 2.0 ** -23 * Ys.double().abs().sum(0))).max().item()
    print(f"gst_wgrad {name} ({M}, {N}, {K}): max |err| / bound = {ratio:.4f} (dW), {rb:.4f} (db)")
    assert ratio <= 1.0 and rb <= 1.0


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_agrees_with_the_rank_64_block_route_of_the_product_library(name):
    """What the parent commit could compute: gsl_lora_grad with r = 64 over the 64-column blocks of X gives the same product."""
    from gslora_hip import ops
    dtype = DTYPES[name]
    M, N, K = 700, 768, 128
    g = torch.Generator().manual_seed(13)
    Y, X = torch.randn(M, N, generator=g).cuda().to(dtype), torch.randn(M, K, generator=g).cuda().to(dtype)
    dW = torch.empty(N, K, device="cuda")
    LT().wgrad(Y, X, dW)
    blocks = torch.zeros(N, K, device="cuda")
    for k0 in range(0, K, 64):
        ops.lora_grad(Y, X[:, k0:k0 + 64], blocks[:, k0:], K, 1, 64, accumulate=False)
    ratio = ((dW.double() - blocks.double()).abs() / (2.0 * elementwise_bound(Y, X))).max().item()
    print(f"gst_wgrad against the block route, {name}: max |diff| / (2 bound) = {ratio:.4f}")
    assert ratio <= 1.0


def test_refusals_come_before_any_launch():
    lt = LT()
    lib = lt.load()
    p = 4096      # a non-null, 16-byte aligned address that is never dereferenced: the argument check fails first
    base = dict(Y=p, ldy=128, X=p, ldx=64, dW=p, ldw=64, db=None, M=5, N=128, K=64, dtype=1, acc=0, ws=p, gs=None, st=None)
    call = lambda **kw: lib.gst_wgrad(*[{**base, **kw}[k] for k in base])
    for bad, word in ((dict(N=96), "N % 64"), (dict(K=100, ldx=128), "K % 64"), (dict(ldy=64), "ldy >= N"), (dict(ldx=32), "ldx >= K"),
                      (dict(ldw=63), "ldw >= K"), (dict(Y=p + 2), "rows of Y"), (dict(ldy=132), "rows of Y"), (dict(X=p + 8), "rows of X"),
                      (dict(ldx=68), "rows of X"), (dict(ws=None), "null ws"), (dict(dtype=3), "dtype"), (dict(dtype=-1), "dtype"),
                      (dict(M=0), "M >= 1"), (dict(dW=None), "null operand")):
        assert call(**bad) == -1, bad
        msg = lib.gst_last_error().decode()
        assert "gst_wgrad" in msg and word in msg, (bad, msg)
    assert lib.gst_wgrad_ws_elems(5, 96, 64, 1) == -1
    with pytest.raises(RuntimeError, match="K % 64"):
        lt.wgrad_plan(5, 64, 65, torch.float32)
    torch.cuda.synchronize()
