"""Exact-integer GEMM probes and their float64 reference (tests/test_gemm_probes_host.py, tests/test_hip_gemm_edges.py).

Random normal operands hide the faults a GEMM kernel is most likely to have behind a max-normalised tolerance: a dropped K tile, a row
too many in a reduction, a store four columns off. Here every operand is a small integer (or a small multiple of a power of two), chosen so
that the correct result and every intermediate the kernels round are exactly representable in f32, bf16 and fp16: the comparison is
torch.equal in every dtype and on every kernel, whatever the summation order.

  A1, A2   ternary {-1, 0, 1}; every 64-wide K tile of every row holds the same number (>= 1) of non-zeros, at most 64 per row over
           K1 + K2 — a dropped K tile or K2 segment shows. The in-kernel-LoRA forms get 4 non-zeros per row: their t = A P^T / 8 adds
           eighths, and integer + eighths has to stay below 32 to survive bf16's 8 bits.
  W1, W2   ternary, dense. P [16, K] (rows >= r zero) and Q [N, 32] (columns >= r zero) ternary.
  alpha    0.5 (STORE, STORE_F32, MUL: the epilogues that honour it), lora_scale 1/8, dropout p = 0.5 (scale exactly 2).
  bias, pos, cls in [-4, 4], res in [-8, 8], aux in {-2, -1, 1, 2}, Y / Y2 in [-4, 4], U / U1 ternary.

Largest magnitudes (tests/test_gemm_probes_host.py checks the round trip of every value): plain |acc| <= 64, BIAS_RES and PATCH with dropout
(64 + 4 + 4) * 2 + 8 = 152 — integers below 256 —, MUL 0.5 * 64 * 2 = 64 in halves; LoRA |acc| <= 4 + 16 * 0.5 = 12 in eighths, (12 + 4) + 8 = 24
without and 40 in quarters with dropout. The sums over m of the reductions stay below 1300 * 24 * 8 < 2^24 eighths: exact in f32 in any order.

LGRAD_EDGES is the table of gsl_lora_grad at ranks 1 - 16, one row per path of its launch plan (tests/test_lora_grad_plan_host.py,
tests/test_hip_lora_grad_edges.py); its operands come from make(..., edge_rows=...), which takes the zeros out of the first and last row of
every row split so that a dropped or doubled boundary row moves every element of the result.

Every builder is deterministic (its own torch.Generator) and returns float32 CPU tensors; the references take tensors on any device and
return float64 on that device."""
import collections

import torch

ALPHA = 0.5
P_DROP = 0.5
LORA_SCALE = 0.125
PATCH_T = 13                    # tokens per image of the PATCH epilogues (M need not be a multiple: the token of row m is m % T)
BAND_FILL = float("nan")        # what surrounds every input the kernels read (tests/guard_bands.py)

# name, entry (gemm = gsl_gemm_nt, lora = gsl_gemm_nt_lora, mulgrad, lgrad = gsl_lora_grad), shape, rank, the gsl_gemm_tile the row is named
# for (16-bit operands), and whether float32 runs the row too
Case = collections.namedtuple("Case", "name kind M N K1 K2 r tile f32")
TABLE = (
    Case("ring64_direct_store", "gemm", 130, 68, 64, 64, 0, "RING64", False),
    Case("ring64", "gemm", 65, 192, 128, 0, 0, "RING64", False),
    Case("ring64_wide", "gemm", 1541, 2052, 64, 64, 0, "RING64_WIDE", False),            # 25 x 33 = 825 small tiles > 768 slots
    Case("ring64_ksplit", "gemm", 130, 132, 1024, 64, 0, "RING64_KSPLIT", False),
    Case("tile128", "gemm", 900, 4228, 64, 64, 0, "128", False),                         # 8 x 34 = 272 blocks, M < 1024
    Case("ring256x128_n68", "gemm", 32600, 68, 64, 0, 0, "RING256X128", False),          # 128 x 1 tiles of 256 x 256
    Case("ring256x128_n388", "gemm", 16200, 388, 64, 64, 0, "RING256X128", False),       # 64 x 2
    Case("p8_n4100", "gemm", 1800, 4100, 64, 64, 0, "P8", False),                        # 8 x 17 = 136 tiles, N % 8 == 4: direct stores
    Case("p8_n4104", "gemm", 1800, 4104, 64, 64, 0, "P8", False),                        # N % 8 == 0: the staged epilogues on ragged tiles
    Case("lora_ring64", "lora", 130, 68, 128, 0, 8, "RING64", False),
    Case("lora_p8", "lora", 1800, 4100, 64, 0, 4, "P8", False),
    Case("mulgrad_n264", "mulgrad", 300, 264, 64, 0, 5, None, False),
    Case("mulgrad_n520", "mulgrad", 1300, 520, 128, 0, 16, None, False),
    Case("f32_valu", "gemm", 65, 68, 64, 64, 0, "F32_VALU", True),
    Case("f32_mfma", "gemm", 130, 132, 64, 64, 0, "F32_MFMA", True),
    Case("lgrad_n132", "lgrad", 333, 132, 0, 0, 4, None, True),                          # f32 only: vector width 4
    Case("lgrad_n136", "lgrad", 333, 136, 0, 0, 4, None, True),                          # 16-bit: vector width 8
    Case("lgrad_n768", "lgrad", 700, 768, 0, 0, 16, None, True),
)
BY_NAME = {c.name: c for c in TABLE}
LGRAD_BATCH = ((333, 256, 4), (700, 768, 16))      # (M, N, r) of the two entries of the lora_grad_batch case

# gsl_lora_grad at ranks 1 - 16, one row per launch-plan path (tests/test_lora_grad_plan_host.py holds every claim to gsl_lora_grad_plan,
# tests/test_hip_lora_grad_edges.py runs the rows): name, shape, rank, operand kind ("16": bf16 and fp16, "f32"), then the path the row is
# named for — form, reduce form, row splits, rows per split, column groups of the VALU form — and ystep: Y's rows are ystep * N elements
# apart (the compact cls rows of a 197-token model). |sums| <= 4 * 16385 + 4 < 2^24: exact in f32 in any order.
LgCase = collections.namedtuple("LgCase", "name M N r kind form reduce nsplit rps CG ystep")
LGRAD_EDGES = tuple(LgCase(*row) for row in (
    ("mfma_first_m", 64, 256, 8, "16", "MFMA", "DIRECT", 2, 32, 0, 1),                      # the form's first M: two full splits
    ("mfma_one_row_tail", 65, 256, 1, "16", "MFMA", "DIRECT", 3, 32, 0, 1),                 # last split of one row; R = 8 ...
    ("mfma_one_row_tail", 65, 256, 3, "16", "MFMA", "DIRECT", 3, 32, 0, 1),
    ("mfma_one_row_tail", 65, 256, 8, "16", "MFMA", "DIRECT", 3, 32, 0, 1),
    ("mfma_one_row_tail", 65, 256, 9, "16", "MFMA", "DIRECT", 3, 32, 0, 1),                 # ... and R = 16
    ("mfma_one_row_tail", 65, 256, 16, "16", "MFMA", "DIRECT", 3, 32, 0, 1),
    ("mfma_two_row_tail_one_launch", 130, 2048, 8, "16", "MFMA", "ONE_LAUNCH", 5, 32, 0, 1),    # 8 column blocks
    ("mfma_one_launch_boundary", 65, 1024, 8, "16", "MFMA", "ONE_LAUNCH", 3, 32, 0, 1),     # N * R == 8192 exactly
    ("mfma_capped_splits", 1057, 256, 5, "16", "MFMA", "DIRECT", 17, 64, 0, 1),             # 34 slabs, cap 32: two slabs per split, last split 33 rows
    ("mfma_two_level", 2049, 256, 8, "16", "MFMA", "TWO_LEVEL", 65, 32, 0, 1),              # level-1 slabs of 32 / 32 / 1 splits
    ("mfma_two_level", 2049, 256, 16, "16", "MFMA", "TWO_LEVEL", 65, 32, 0, 1),             # (R = 16 on the two levels: N * R = 4096)
    ("mfma_two_level", 2049, 768, 7, "16", "MFMA", "TWO_LEVEL", 65, 32, 0, 1),
    ("mfma_two_level", 2049, 768, 8, "16", "MFMA", "TWO_LEVEL", 65, 32, 0, 1),
    ("mfma_one_launch_many_splits", 2081, 512, 16, "16", "MFMA", "ONE_LAUNCH", 66, 32, 0, 1),   # the four waves own 17 / 17 / 16 / 16 splits
    ("mfma_over_160_splits", 5153, 1024, 8, "16", "MFMA", "TWO_LEVEL", 162, 32, 0, 1),      # although N * R >= 8192
    ("valu_smallest", 1, 8, 1, "16", "VALU", "DIRECT", 1, 1, 64, 1),                        # one column group, four row phases, one row
    ("valu_smallest", 1, 4, 1, "f32", "VALU", "DIRECT", 1, 1, 64, 1),
    ("valu_smallest", 5, 4, 2, "f32", "VALU", "DIRECT", 1, 5, 64, 1),                       # fewer rows than a batch of loads (4 x 4 phases)
    ("valu_unaligned_block", 259, 72, 8, "16", "VALU", "DIRECT", 3, 87, 64, 1),             # rows 64 + 23 per LDS fill
    ("valu_cg128", 63, 256, 16, "16", "VALU", "DIRECT", 1, 63, 128, 1),                     # M < 64 on an MFMA-shaped N; two row phases
    ("valu_cg128", 300, 520, 9, "16", "VALU", "DIRECT", 3, 100, 128, 1),
    ("valu_cg256", 130, 1024, 7, "f32", "VALU", "DIRECT", 2, 65, 256, 1),                   # one row phase: no phase combine
    ("valu_cg256", 70, 2056, 8, "16", "VALU", "DIRECT", 1, 70, 256, 1),                     # a second column block with one active group
    ("valu_two_level", 4225, 8, 3, "16", "VALU", "TWO_LEVEL", 34, 125, 64, 1),              # level-1 slabs of 32 / 2 splits
    ("valu_two_level", 4225, 8, 9, "16", "VALU", "TWO_LEVEL", 34, 125, 128, 1),             # (R = 16 on the VALU form's two levels)
    ("valu_two_level", 4225, 4, 3, "f32", "VALU", "TWO_LEVEL", 34, 125, 64, 1),
    ("valu_two_level", 16385, 8, 3, "16", "VALU", "TWO_LEVEL", 129, 128, 64, 1),            # last split and last level-1 slab of ONE row
    ("cls_rows", 8, 512, 8, "16", "VALU", "DIRECT", 1, 8, 64, 197),                         # the 8 cls rows through the single call
    ("cls_rows", 8, 2048, 8, "16", "VALU", "DIRECT", 1, 8, 256, 197),
))
LGRAD_EDGE_IDS = tuple(f"{c.name}-{c.M}x{c.N}-r{c.r}-{c.kind}" for c in LGRAD_EDGES)


def padded_rank(r):
    """R of the partial layout part[split][n][R] of gsl_lora_grad."""
    return 8 if r <= 8 else 16 if r <= 16 else 32 if r <= 32 else 64


def make_lgrad_edges(M, N, edge_rows):
    """Y [M, N], U [M, 64] and G0 [N, 16] (rank r uses G0[:, :r]) of an LGRAD_EDGES shape, with the edge_rows option of make()."""
    return make(Case(f"lgrad_edges_{M}x{N}", "lgrad", M, N, 0, 0, 16, None, True), edge_rows=edge_rows)


# epilogues with an exact reference, by the name the tests use
EXACT_GEMM = ("store", "store_f32", "bias_res_f32", "bias_res_16", "bias_res_f32_drop", "bias_res_16_drop", "mul", "patch", "patch_16", "qkv_hm")
EXACT_LORA = ("store", "bias_res_f32", "bias_res_16", "bias_res_16_drop", "mul")


def _gen(case, salt=0):
    return torch.Generator().manual_seed(1000003 * case.M + 1009 * case.N + 31 * case.K1 + 7 * case.K2 + case.r + 7919 * salt)


def per_tile(case):
    """Non-zeros per 64-wide K tile of a row of A."""
    nt = (case.K1 + case.K2) // 64
    if case.kind in ("lora", "mulgrad"):
        return 4 // nt
    return max(1, min(4, 64 // nt))


def ternary(g, *shape):
    return torch.randint(-1, 2, shape, generator=g).float()


def small_int(g, lim, *shape):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def ternary_rows(g, M, K, c):
    """[M, K] ternary with exactly c non-zeros in every 64-wide tile of every row."""
    nt = K // 64
    idx = torch.rand(M, nt, 64, generator=g).argsort(-1)[..., :c]
    sign = torch.randint(0, 2, (M, nt, c), generator=g).float() * 2 - 1
    return torch.zeros(M, nt, 64).scatter_(2, idx, sign).view(M, K)


def split_edge_rows(M, *rps):
    """The first and the last row of every row split of an M-row reduction, for each rows-per-split in rps (a launch plan's `rps`: split k
    owns the rows [k rps, min(M, (k + 1) rps)); the slabs of a two-level reduce begin and end at split edges). Sorted, unique."""
    rows = set()
    for p in rps:
        for r0 in range(0, M, p):
            rows.update((r0, min(M, r0 + p) - 1))
    return tuple(sorted(rows))


def make(case, edge_rows=None):
    """The operands of one table row: a dict of float32 CPU tensors. edge_rows (lgrad rows only; default off, and the other rows keep
    the values they have without it): on these rows Y has no zero — it is in +-{1..4} — and U is +-1 in all of its 64 columns, so that
    Y[m, n] U[m, j] != 0 for every n and j: such a row dropped from the sum, or counted twice, moves every element of the result."""
    g = _gen(case)
    M, N, r = case.M, case.N, case.r
    d = {}
    if case.kind == "lgrad":
        d["Y"], d["U"] = small_int(g, 4, M, N), ternary(g, M, 64)
        d["G0"] = small_int(g, 4, N, r)
        if edge_rows is not None:
            rows = torch.tensor(edge_rows, dtype=torch.long)
            ge = _gen(case, salt=101)
            y = torch.randint(1, 5, (len(rows), N), generator=ge).float() * (torch.randint(0, 2, (len(rows), N), generator=ge).float() * 2 - 1)
            u = torch.randint(0, 2, (len(rows), 64), generator=ge).float() * 2 - 1
            d["Y"][rows], d["U"][rows] = torch.where(d["Y"][rows] != 0, d["Y"][rows], y), torch.where(d["U"][rows] != 0, d["U"][rows], u)
        return d
    c = per_tile(case)
    d["A1"], d["W1"] = ternary_rows(g, M, case.K1, c), ternary(g, N, case.K1)
    if case.K2:
        d["A2"], d["W2"] = ternary_rows(g, M, case.K2, c), ternary(g, N, case.K2)
    d["bias"], d["res"] = small_int(g, 4, N), small_int(g, 8, M, N)
    d["aux"] = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (M, N), generator=g)]
    if case.kind == "gemm":
        d["pos"], d["cls"] = small_int(g, 4, PATCH_T, N), small_int(g, 4, N)
    else:
        P, Q = torch.zeros(16, case.K1), torch.zeros(N, 32)
        P[:r], Q[:, :r] = ternary(g, r, case.K1), ternary(g, N, r)
        d["P"], d["Q"] = P, Q
    if case.kind == "mulgrad":
        d["U1"], d["Y2"] = ternary(g, M, 16), small_int(g, 4, M, N)
        d["G1_0"], d["G2_0"] = small_int(g, 4, N, r), small_int(g, 4, N, r)
    return d


def make_lgrad_batch():
    out = []
    for i, (M, N, r) in enumerate(LGRAD_BATCH):
        g = _gen(Case("batch", "lgrad", M, N, 0, 0, r, None, False), salt=i + 1)
        out.append(dict(Y=small_int(g, 4, M, N), U=ternary(g, M, 64), G0=small_int(g, 4, N, r), r=r))
    return out


# ---------------------------------------------------------------------------------------------------------------- float64 reference
def dd(t):
    return None if t is None else t.double()


def accumulate(d, drop_last_k_tile=False, drop_k2=False):
    """A1 W1^T + A2 W2^T in float64 (the fault models of the host test: without the last 64-wide K tile / without the K2 segment)."""
    segs = [(d["A1"], d["W1"])] + ([(d["A2"], d["W2"])] if "A2" in d and not drop_k2 else [])
    if drop_last_k_tile:
        A, W = segs[-1]
        segs[-1] = (A[:, :A.shape[1] - 64], W[:, :W.shape[1] - 64])
    return sum(dd(A) @ dd(W).t() for A, W in segs)


def lora_t(d):
    """t = lora_scale * A P^T, [M, 16] (what the kernel rounds to 16 bits and stores, zero padded, to tout [M, 64])."""
    return LORA_SCALE * (dd(d["A1"]) @ dd(d["P"]).t())


def accumulate_lora(d, drop_rank_term=False, drop_last_k_tile=False):
    acc = accumulate(d, drop_last_k_tile=drop_last_k_tile)
    return acc if drop_rank_term else acc + lora_t(d) @ dd(d["Q"])[:, :16].t()


def tout(d):
    t = lora_t(d)
    return torch.cat([t, torch.zeros(t.shape[0], 48, dtype=t.dtype, device=t.device)], 1)


def qkv_head_major(x, T):
    """STORE_QKV_HM: row b T + t, column (which, h, d) of [M, 3 H 64] -> [b][h][which][t][d], as an [M, N] tensor again."""
    M, N = x.shape
    H = N // 192
    return x.view(M // T, T, 3, H, 64).permute(0, 3, 2, 1, 4).reshape(M, N)


def epilogue(name, acc, d, keep=None):
    """The exact epilogues on a float64 accumulator. keep [M, N]: the dropout mask of the *_drop forms (p = 0.5: kept values double)."""
    dm = 1.0 if keep is None else dd(keep) / (1.0 - P_DROP)
    M = acc.shape[0]
    if name in ("store", "store_f32"):
        return ALPHA * acc
    if name == "qkv_hm":
        return qkv_head_major(ALPHA * acc, PATCH_T)
    if name.startswith("bias_res"):
        return (acc + dd(d["bias"])) * dm + dd(d["res"])
    if name == "mul":
        return ALPHA * acc * dd(d["aux"])
    if name.startswith("patch"):
        tok = torch.arange(M, device=acc.device) % PATCH_T
        base = torch.where((tok == 0)[:, None], dd(d["cls"])[None, :].expand_as(acc), acc + dd(d["bias"]))
        return (base + dd(d["pos"])[tok]) * dm
    raise KeyError(name)


def epilogue_lora(name, acc, d, keep=None):
    """The in-kernel-LoRA form has no alpha: STORE and MUL take the accumulator as it is."""
    if name == "store":
        return acc
    if name == "mul":
        return acc * dd(d["aux"])
    return epilogue(name, acc, d, keep)


def mulgrad(d, r, extra_row=None):
    """out = (A W^T + t Q^T) * aux, G1 = G1_0 + out^T U1[:, :r], G2 = G2_0 + Y2^T t[:, :r] (accumulate on). extra_row: the fault model of
    a reduction that runs one row too far — (out row, U1 row, Y2 row, t row) of the row behind the last one."""
    out = accumulate_lora(d) * dd(d["aux"])
    t = lora_t(d)
    g1 = dd(d["G1_0"]) + out.t() @ dd(d["U1"])[:, :r]
    g2 = dd(d["G2_0"]) + dd(d["Y2"]).t() @ t[:, :r]
    if extra_row is not None:
        o_x, u_x, y_x, t_x = (dd(x) for x in extra_row)
        g1 = g1 + o_x[:, None] * u_x[None, :r]
        g2 = g2 + y_x[:, None] * t_x[None, :r]
    return out, g1, g2


def lora_grad(d, r, col=0, extra_row=None):
    """G0 + Y^T U[:, col : col + r]."""
    g = dd(d["G0"]) + dd(d["Y"]).t() @ dd(d["U"])[:, col:col + r]
    if extra_row is not None:
        y_x, u_x = (dd(x) for x in extra_row)
        g = g + y_x[:, None] * u_x[None, col:col + r]
    return g


def survives(x, dtype):
    """Does every value of x make the round trip through dtype?"""
    return torch.equal(x.to(dtype).to(x.dtype), x)

