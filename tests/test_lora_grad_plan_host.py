"""The launch plan of gsl_lora_grad / gsl_lora_grad_batch at ranks 1 - 16, on the CPU: gsl_lora_grad_plan and gsl_lora_grad_batch_plan are
host code of libgslora_hip.so (the lg_form / lg_plan / lgb_plan the launches call; nothing is dereferenced), so this file needs the
cross-compiled library (build() of __graft_entry__.py) and no GPU, as tests/test_gemm_probes_host.py does for gsl_gemm_tile_choice.

(a) Every row of oracle/gemm_probes.py LGRAD_EDGES — the table tests/test_hip_lora_grad_edges.py runs — takes the path it is named for:
    form, reduce form, padded rank, row splits, rows per split, column groups. Together the rows reach every (form, reduce form, R) that
    exists, the `steps <= 64` cap of the MFMA form and CG = 64 / 128 / 256. The shape notes of tests/test_hip_lora_rank.py are held to the
    same export (its docstring once said (700, 768) reaches the two-level reduce; it takes the single launch).
(b) The refusals of the launches, with their messages, from the plan exports.
(c) A fault model on the probe operands the device test uses (small integers; the first and last row of every split without a zero):
    against the float64 reference, a row behind the last one added, the first row of a split counted twice, a last split dropped and a last
    level-1 slab dropped each change the result of every row of the table, and EVERY element of it wherever the fault is one row — the
    extra row, the doubled row, and the dropped split / slab of the rows whose last split / slab is one row (M = 65, 2049, 2081, 5153 on
    the MFMA form: one per reduce kernel; M = 16385 = 128 * 128 + 1 on the VALU form's two levels, the smallest M at which its rule leaves
    a one-row last split that is also a whole level-1 slab). A part of several rows can cancel at single elements whatever its edge rows
    hold (every product is at most 4): there the test asserts that the result differs and that the part's edge rows alone would have
    moved every element."""
import functools

import pytest
import torch

from oracle import gemm_probes as G

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
FAN = 32      # splits per level-1 slab of the two-level reduce (LG_FAN of csrc/lora.hip)


def dtypes_of(c):
    return (F32,) if c.kind == "f32" else (BF16, F16)


@pytest.fixture(scope="module")
def ops():
    from gslora_hip import _lib, ops as _ops
    _lib.load()
    return _ops


def claimed(L, c):
    """The plan a table row is named for, as gsl_lora_grad_plan reports one."""
    bx = c.N // 256 if c.form == "MFMA" else -(-(c.N // (4 if c.kind == "f32" else 8)) // c.CG)
    return (getattr(L, "LGRAD_" + c.form), G.padded_rank(c.r), bx, c.nsplit, c.rps, c.CG, getattr(L, "LGRAD_REDUCE_" + c.reduce))


@pytest.mark.parametrize("c", G.LGRAD_EDGES, ids=G.LGRAD_EDGE_IDS)
def test_every_table_row_takes_the_path_it_is_named_for(ops, c):
    from gslora_hip import _lib as L
    for dt in dtypes_of(c):
        for ldy in (c.N * c.ystep, (c.N + 64) * c.ystep):      # the contiguous and the padded placement of the device test
            assert tuple(ops.lora_grad_plan_args(c.M, c.N, c.r, dt, ldy=ldy)) == claimed(L, c), (c, dt, ldy)
    assert -(-c.M // c.rps) == c.nsplit


def test_the_table_reaches_every_path():
    seen = {(c.form, c.reduce, G.padded_rank(c.r)) for c in G.LGRAD_EDGES}
    reachable = {(f, red, R) for f in ("MFMA", "VALU") for red in ("DIRECT", "TWO_LEVEL", "ONE_LAUNCH") for R in (8, 16)
                 if not (f == "VALU" and red == "ONE_LAUNCH")}
    assert seen == reachable
    assert {c.CG for c in G.LGRAD_EDGES if c.form == "VALU"} == {64, 128, 256}
    capped = [c for c in G.LGRAD_EDGES if c.form == "MFMA" and c.rps > 32]      # the `steps <= 64` cap: more than 32 slabs in 32 splits
    assert capped and all(32 < -(-c.M // 32) <= 64 for c in capped)
    assert {c.M - (c.nsplit - 1) * c.rps for c in G.LGRAD_EDGES if c.form == "MFMA"} >= {1, 2, 32, 33}      # rows of the last split
    two = [c for c in G.LGRAD_EDGES if c.reduce == "TWO_LEVEL"]
    assert {c.nsplit % FAN for c in two} >= {1, 2} and all(c.nsplit > FAN for c in two)      # splits of the last level-1 slab


def rule(M, N, r, dt):
    """The plan rule restated from the comments of csrc/lora.hip: (form, R, bx, nsplit, rps, CG, reduce) by name."""
    up = lambda a, b: -(-a // b)
    R = G.padded_rank(r)
    if dt != F32 and N % 256 == 0 and M >= 64:      # matrix cores: 32-row slabs, about 1024 workgroups, at most 32 splits up to 64 slabs
        form, CG, bx, steps = "MFMA", 0, N // 256, up(M, 32)
        n0 = min(steps, max(1, 1024 // bx))
        if steps <= 64:
            n0 = min(n0, FAN)
        rps = up(steps, n0) * 32
    else:                                           # VALU: at least 128 rows per split, about 768 workgroups
        ncol = N // (4 if dt == F32 else 8)
        form, CG = "VALU", 256 if ncol >= 256 else 128 if ncol > 64 or R > 8 else 64
        bx = up(ncol, CG)
        rps = up(M, max(1, min(up(M, 128), max(1, 768 // bx))))
    nsplit = up(M, rps)
    one = form == "MFMA" and nsplit <= 160 and N * R >= 8192
    return form, R, bx, nsplit, rps, CG, "ONE_LAUNCH" if one else "TWO_LEVEL" if nsplit > FAN else "DIRECT"


def test_the_plan_around_every_threshold_of_the_rule(ops):
    """The export against the restated rule around its thresholds: M = 64, 32 / 64 slabs, 160 splits, N * R = 8192, the column groups."""
    from gslora_hip import _lib as L
    seen = set()
    for dt in (BF16, F16, F32):
        for N in (8, 248, 256, 264, 512, 520, 1024, 2048, 2056):
            for M in (1, 63, 64, 65, 1024, 1025, 2048, 2049, 4096, 4097, 5120, 5121, 5153, 12608):
                for r in (1, 8, 9, 16):
                    form, R, bx, nsplit, rps, CG, red = rule(M, N, r, dt)
                    want = (getattr(L, "LGRAD_" + form), R, bx, nsplit, rps, CG, getattr(L, "LGRAD_REDUCE_" + red))
                    assert tuple(ops.lora_grad_plan_args(M, N, r, dt)) == want, (dt, M, N, r)
                    seen.add((form, red))
    assert len(seen) == 5
    assert rule(12608, 512, 8, F16)[-1] == rule(12608, 768, 8, F16)[-1] == "TWO_LEVEL"      # the benchmark's reductions
    # an unaligned U or Y, a row stride off 16 bytes and a 16-wide U above rank 16 leave the matrix-core form
    assert ops.lora_grad_plan_args(65, 256, 8, BF16).form == L.LGRAD_MFMA
    assert ops.lora_grad_plan_args(65, 256, 5, BF16, u_addr=(1 << 20) + 10).form == L.LGRAD_VALU
    assert ops.lora_grad_plan_args(65, 256, 8, BF16, y_addr=(1 << 20) + 8).form == L.LGRAD_VALU
    assert ops.lora_grad_plan_args(65, 256, 8, BF16, ldy=260).form == L.LGRAD_VALU
    assert ops.lora_grad_plan_args(65, 256, 8, BF16, u_addr=(1 << 20) + 32).form == L.LGRAD_MFMA      # column 16 of a 64-wide tensor


def test_workspace_query_covers_the_plan_and_takes_every_legal_size(ops):
    """gsl_lora_grad_ws_elems: at least the partials and the level-1 slabs of the plan, for every table row; N = 4 (legal in f32) once
    divided by zero column blocks in the plan of the 8-wide form; sizes and ranks every call is refused with give 0."""
    from gslora_hip import _lib as L
    lib = L.load()
    for c in G.LGRAD_EDGES:
        need = (c.nsplit + -(-c.nsplit // FAN)) * c.N * G.padded_rank(c.r)
        assert lib.gsl_lora_grad_ws_elems(c.M, c.N, c.r) >= need, c
    assert lib.gsl_lora_grad_ws_elems(1, 4, 1) == 2 * 4 * 8 and lib.gsl_lora_grad_ws_elems(4225, 4, 3) == (34 + 2) * 4 * 8
    assert lib.gsl_lora_grad_ws_elems(5, 12, 2) == 2 * 12 * 8
    for M, N, r in ((0, 256, 8), (65, 0, 8), (65, 256, 0), (65, 256, 65), (65, 6, 2), (65, 3, 2)):
        assert lib.gsl_lora_grad_ws_elems(M, N, r) == 0, (M, N, r)


def test_shape_notes_of_the_rank_tests(ops):
    """What the docstring of tests/test_hip_lora_rank.py says about its shapes, asked of the export."""
    from gslora_hip import _lib as L
    want = {(65, 256): (L.LGRAD_MFMA, L.LGRAD_REDUCE_ONE_LAUNCH, 3), (700, 768): (L.LGRAD_MFMA, L.LGRAD_REDUCE_ONE_LAUNCH, 22),
            (1300, 2048): (L.LGRAD_MFMA, L.LGRAD_REDUCE_ONE_LAUNCH, 21), (5153, 256): (L.LGRAD_MFMA, L.LGRAD_REDUCE_TWO_LEVEL, 162)}
    for (M, N), (form, red, nsplit) in want.items():
        for r in (17, 32, 64):
            p = ops.lora_grad_plan_args(M, N, r, BF16)
            assert (p.form, p.reduce, p.nsplit) == (form, red, nsplit), (M, N, r, p)
    for M, N, dt, red, nsplit in ((333, 132, F32, "DIRECT", 3), (333, 136, F16, "DIRECT", 3), (5, 256, BF16, "DIRECT", 1), (700, 768, F32, "DIRECT", 6),
                                  (4225, 8, F16, "TWO_LEVEL", 34)):
        p = ops.lora_grad_plan_args(M, N, 17, dt)
        assert (p.form, p.reduce, p.nsplit, p.R) == (L.LGRAD_VALU, getattr(L, "LGRAD_REDUCE_" + red), nsplit, 32), (M, N, p)


def test_batch_plan(ops):
    """Every entry runs the aligned MFMA body from M = 1; the splits of an entry follow the column blocks of its group of 24."""
    ent = [(M, N, (3, 8, 16)[i % 3]) for i, (M, N) in enumerate((M, N) for M in (1, 8, 33, 65, 2049) for N in (256, 768))]
    plans = ops.lora_grad_batch_plan(ent)
    target = min(32, 1024 // sum(N // 256 for _, N, _ in ent))
    for (M, N, r), p in zip(ent, plans):
        steps = -(-M // 32)
        rps = -(-steps // min(steps, target)) * 32
        assert tuple(p) == (G.padded_rank(r), N // 256, -(-M // rps), rps), ((M, N, r), p)
    assert plans[0].nsplit == 1 and plans[-1].nsplit > 1
    # 25 entries: the 25th is planned with the second group, alone — its splits do not see the column blocks of the first 24
    many = [(2049, 2048, 8)] * 25
    plans = ops.lora_grad_batch_plan(many)
    assert plans[0] == plans[23] and plans[0].rps == -(-65 // (1024 // (24 * 8))) * 32 and plans[24].rps == 96 and plans[24].nsplit == 22


def refused(fn, *a, **kw):
    from gslora_hip import _lib as L
    with pytest.raises(RuntimeError) as e:
        fn(*a, **kw)
    assert "argument check failed" in str(e.value)
    return L.load().gsl_last_error().decode()


def test_refusals_name_the_argument(ops):
    rank_msg = "r in [1,64], ldu >= max(16, r) (zero-padded), ldu % 8 == 0"
    assert rank_msg in refused(ops.lora_grad_plan_args, 65, 256, 0, BF16)
    assert rank_msg in refused(ops.lora_grad_plan_args, 65, 256, 17, BF16, ldu=16)
    assert rank_msg in refused(ops.lora_grad_plan_args, 65, 256, 8, BF16, ldu=20)
    assert rank_msg in refused(ops.lora_grad_plan_args, 65, 256, 65, BF16, ldu=72)
    assert "N must be a multiple of the vector width" in refused(ops.lora_grad_plan_args, 65, 252, 8, BF16)
    assert "N must be a multiple of the vector width" in refused(ops.lora_grad_plan_args, 65, 6, 2, F32)
    assert tuple(ops.lora_grad_plan_args(65, 252, 8, F32))      # (a multiple of 4 is enough for f32)
    assert "null/size" in refused(ops.lora_grad_plan_args, 0, 256, 8, BF16)
    assert "null/size" in refused(ops.lora_grad_plan_args, 65, 256, 8, BF16, ldy=248)
    assert "null/size" in refused(ops.lora_grad_plan_args, 65, 256, 8, BF16, u_addr=0)
    from gslora_hip.ops import _LgradDesc
    import ctypes
    from gslora_hip import _lib as L

    def batch(M=65, N=256, r=8, ldy=None, ldu=64, y=1 << 20, u=1 << 20):
        arr = (_LgradDesc * 1)(_LgradDesc(y, N if ldy is None else ldy, u, ldu, M, N, r, 0, 0, 1 << 20, r, 1))
        out = (ctypes.c_int * 4)()
        rc = L.load().gsl_lora_grad_batch_plan(arr, 1, out)
        ws = L.load().gsl_lora_grad_batch_ws_elems(arr, 1)
        assert (rc == 0) == (ws >= 0), "the plan export and the workspace query refuse the same descriptors"
        return rc, L.load().gsl_last_error().decode(), tuple(out)
    assert batch() == (0, batch()[1], (8, 1, 3, 32))
    batch_msg = "r in [1,64], ldu >= 16 (above rank 16: >= 8 * ceil(r / 8)), N % 256 == 0, 16-byte rows"
    for kw in (dict(r=0), dict(r=17, ldu=16), dict(N=264), dict(ldu=20), dict(ldy=260), dict(r=65, ldu=72)):
        rc, msg, _ = batch(**kw)
        assert rc != 0 and batch_msg in msg, kw
    rc, msg, _ = batch(u=(1 << 20) + 10)
    assert rc != 0 and "16-byte aligned operands" in msg
    rc, msg, _ = batch(M=0)
    assert rc != 0 and "null/size" in msg


# ---------------------------------------------------------------------------------------------------------------- fault model
@functools.lru_cache(maxsize=None)
def probe(M, N, rps):
    d = G.make_lgrad_edges(M, N, G.split_edge_rows(M, rps))
    return d


def ref(d, r, rows=None):
    """G0 + Y^T U[:, :r] in float64 over the given rows (an index tensor: a row may be missing or twice in it)."""
    sub = d if rows is None else dict(d, Y=d["Y"][rows], U=d["U"][rows])
    return G.lora_grad(dict(sub, G0=d["G0"][:, :r]), r)


def test_edge_rows_option_leaves_the_default_operands_alone():
    c = G.Case("x", "lgrad", 130, 72, 0, 0, 16, None, True)
    plain, edged = G.make(c), G.make(c, edge_rows=G.split_edge_rows(130, 32))
    rows = torch.tensor(G.split_edge_rows(130, 32))
    assert rows.tolist() == [0, 31, 32, 63, 64, 95, 96, 127, 128, 129]
    keep = torch.ones(130, dtype=torch.bool)
    keep[rows] = False
    for k in ("Y", "U", "G0"):
        assert torch.equal(G.make(c)[k], plain[k])
        assert torch.equal(plain[k][keep] if k != "G0" else plain[k], edged[k][keep] if k != "G0" else edged[k])
    assert (edged["Y"][rows] != 0).all() and (edged["Y"][rows].abs() <= 4).all() and (edged["U"][rows].abs() == 1).all()
    assert (plain["Y"][rows] == 0).any() and (plain["U"][rows] == 0).any()
    same = plain["Y"][rows] != 0
    assert torch.equal(edged["Y"][rows][same], plain["Y"][rows][same])      # only the zeros of an edge row change


@pytest.mark.parametrize("c", G.LGRAD_EDGES, ids=G.LGRAD_EDGE_IDS)
def test_faults_at_split_edges_change_the_result(c):
    d, M, r = probe(c.M, c.N, c.rps), c.M, c.r
    good = ref(d, r)
    assert G.survives(good, F32) and 4 * M + 4 < 2 ** 24
    assert all(G.survives(v.double(), dt) and G.survives(8 * v.double(), dt) for v in (d["Y"], d["U"]) for dt in (F32, BF16, F16))
    everywhere = lambda bad: bool((bad != good).all())      # NaN != x is True: a band row added counts
    idx = torch.arange(M)
    # the row behind the last one (a band: NaN) added
    band = lambda n: torch.full((n,), G.BAND_FILL)
    assert everywhere(G.lora_grad(dict(d, G0=d["G0"][:, :r]), r, extra_row=(band(c.N), band(64)))), "row M added"
    # the first row of a split counted twice, the last row of a split dropped: every split
    for k in range(c.nsplit):
        r0, r1 = k * c.rps, min(M, (k + 1) * c.rps)
        assert everywhere(ref(d, r, torch.cat([idx, idx[r0:r0 + 1]]))), (k, "first row of the split twice")
        assert everywhere(ref(d, r, torch.cat([idx[:r1 - 1], idx[r1:]]))), (k, "last row of the split dropped")
    if c.nsplit == 1:
        return

    def part_dropped(first, what):
        bad = ref(d, r, idx[:first])
        assert not torch.equal(bad, good), what
        if M - first == 1:
            assert everywhere(bad), what
        else:      # several rows: its two edge rows alone move every element unless they cancel each other there
            y, u = d["Y"][[first, M - 1]].double(), d["U"][[first, M - 1], :r].double()
            assert bool(((y[0][:, None] * u[0][None, :]) != 0).all()) and bool(((y[1][:, None] * u[1][None, :]) != 0).all()), what
    part_dropped((c.nsplit - 1) * c.rps, "last split dropped")
    if c.reduce == "TWO_LEVEL":
        part_dropped(((c.nsplit - 1) // FAN) * FAN * c.rps, "last level-1 slab dropped")


def test_one_row_parts_exist_for_every_reduce_kernel():
    """The rows where a dropped last split (and, on two levels, a dropped last slab) is one row, so that it moves every element."""
    one_row = {(c.form, c.reduce) for c in G.LGRAD_EDGES if c.M - (c.nsplit - 1) * c.rps == 1}
    assert one_row >= {("MFMA", "DIRECT"), ("MFMA", "TWO_LEVEL"), ("MFMA", "ONE_LAUNCH"), ("VALU", "TWO_LEVEL")}
    for form in ("MFMA", "VALU"):      # the last level-1 slab is that one row
        assert any(c.form == form and c.reduce == "TWO_LEVEL" and c.M - ((c.nsplit - 1) // FAN) * FAN * c.rps == 1 for c in G.LGRAD_EDGES)
