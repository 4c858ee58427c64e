"""The attention kernel rule on the CPU: gsl_attention_kernel_choice (ops.attention_kernel) is host code of the library — the function the four
attention entry points ask before they launch — and needs only the cross-compiled libgslora_hip.so (build() of __graft_entry__.py; no GPU), as
the tile-rule test of tests/test_gemm_probes_host.py does. Without a device the library counts 256 CUs (an MI355X has as many).

Every row of the rule's table once, a sweep across every threshold against the rule restated here, the arguments the entry points refuse, and
bf16 == fp16 everywhere. The GPU tests that compare two kernels bit for bit (tests/test_hip_ops.py, tests/test_hip_attention_edges.py) assert with
the same function that their shapes reach the kernel their docstrings name."""
import os
import re

import torch

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DIRECTIONS = ("fwd", "bwd", "cls_fwd", "cls_bwd")


def cus():
    """The CU count the library's rule sees: the current device's, 256 without one."""
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count if torch.cuda.is_available() else 256


def rule_as_documented(direction, dt, T, items, n_cus):
    """(direction, dtype, T, items = B * H, CUs) -> the name of the gsl_attn_kernel, restated from the table of include/gslora_hip.h."""
    if direction == "cls_bwd":
        return "BWD_CLS"
    if direction == "cls_fwd":
        return "FWD_CLS_LONG" if T > 256 else "FWD_CLS"
    d = direction.upper()
    if dt == F32:
        return f"{d}_F32_LONG" if T > 224 else f"{d}_F32"
    if T > 224:
        return f"{d}_LONG"
    if T <= 64:
        return f"{d}_T64"
    if d == "FWD" and T <= 208 and items >= 2 * n_cus:
        return "FWD_PERSISTENT"
    if d == "BWD" and 192 < T <= 208 and items >= 8 * n_cus:
        return "BWD_MERGED"
    wide = items < n_cus
    return ("FWD_1024" if wide else "FWD_512") if d == "FWD" else ("BWD_FUSED_1024" if wide else "BWD_FUSED_512")


def test_enumerators_match_the_header():
    from gslora_hip import _lib as L
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gslora_hip.h")).read()
    body = hdr[hdr.index("enum gsl_attn_kernel {"):]
    body = body[:body.index("};")]
    names = re.findall(r"GSL_(ATTN_\w+) = (\d+)", body)
    assert len(names) == 17
    for name, value in names:
        assert getattr(L, name) == int(value), name


# direction, dtype, B, T, H -> kernel: every row of the table once, at 256 CUs (n x 256 items as B = 32 n images x 8 heads)
ROWS = [
    ("fwd", BF16, 2, 225, 2, "FWD_LONG"), ("fwd", F16, 300, 64, 8, "FWD_T64"), ("fwd", BF16, 64, 197, 8, "FWD_PERSISTENT"),
    ("fwd", BF16, 64, 209, 8, "FWD_512"), ("fwd", F16, 31, 197, 8, "FWD_1024"), ("fwd", BF16, 32, 197, 8, "FWD_512"),
    ("fwd", F32, 3, 300, 2, "FWD_F32_LONG"), ("fwd", F32, 3, 64, 2, "FWD_F32"), ("fwd", F32, 3, 224, 2, "FWD_F32"),
    ("bwd", BF16, 2, 1025, 2, "BWD_LONG"), ("bwd", F16, 300, 2, 8, "BWD_T64"), ("bwd", BF16, 256, 197, 8, "BWD_MERGED"),
    ("bwd", BF16, 256, 192, 8, "BWD_FUSED_512"), ("bwd", BF16, 256, 209, 8, "BWD_FUSED_512"), ("bwd", F16, 255, 197, 8, "BWD_FUSED_512"),
    ("bwd", BF16, 3, 197, 8, "BWD_FUSED_1024"), ("bwd", F32, 3, 225, 2, "BWD_F32_LONG"), ("bwd", F32, 3, 197, 2, "BWD_F32"),
    ("cls_fwd", BF16, 3, 256, 2, "FWD_CLS"), ("cls_fwd", F32, 3, 257, 2, "FWD_CLS_LONG"), ("cls_bwd", F16, 3, 5000, 2, "BWD_CLS"),
    ("cls_bwd", F32, 3, 26, 1, "BWD_CLS"),
]


def test_every_row_of_the_table():
    from gslora_hip import _lib as L
    from gslora_hip import ops
    seen = set()
    for direction, dt, B, T, H, want in ROWS:
        assert rule_as_documented(direction, dt, T, B * H, 256) == want
        seen.add(want)
        here = want if cus() == 256 else rule_as_documented(direction, dt, T, B * H, cus())      # (a device with another CU count)
        assert ops.attention_kernel(B, T, H, dt, direction=direction) == getattr(L, "ATTN_" + here), (direction, dt, B, T, H)
    assert len(seen) == 17      # every enumerator is some row's


def test_sweep_across_every_threshold_follows_the_documented_rule():
    from gslora_hip import _lib as L
    from gslora_hip import ops
    n = cus()
    for direction in DIRECTIONS:
        for T in (2, 64, 65, 192, 193, 208, 209, 224, 225, 256, 257, 1025):
            for items in (n - 1, n, 2 * n - 1, 2 * n, 8 * n - 1, 8 * n):
                got = {dt: ops.attention_kernel(items, T, 1, dt, direction=direction) for dt in (BF16, F16, F32)}
                for dt in (BF16, F32):
                    assert got[dt] == getattr(L, "ATTN_" + rule_as_documented(direction, dt, T, items, n)), (direction, dt, T, items)
                assert got[F16] == got[BF16], (direction, T, items)
                # the rule sees B * H, not B: the same items as 8 heads (the head-major layout changes nothing either)
                if items % 8 == 0:
                    assert ops.attention_kernel(items // 8, T, 8, BF16, layout=1, direction=direction) == got[BF16], (direction, T, items)


def test_arguments_the_entry_points_refuse():
    from gslora_hip import _lib as L
    from gslora_hip import ops
    lib = L.load()
    for direction in DIRECTIONS:
        cls = direction.startswith("cls")
        for dt in (BF16, F16, F32):
            assert ops.attention_kernel(3, 197, 2, dt, direction=direction) >= 0
            assert ops.attention_kernel(0, 197, 2, dt, direction=direction) == -1
            assert ops.attention_kernel(3, 1, 2, dt, direction=direction) == -1
            assert ops.attention_kernel(3, 197, 0, dt, direction=direction) == -1
            assert ops.attention_kernel(3, 1025, 2, dt, direction=direction) >= 0
            assert (ops.attention_kernel(3, 1026, 2, dt, direction=direction) == -1) == (direction != "cls_bwd")      # the cls backward takes any T
            # head-major input: 16-bit only in the dense entries; the cls entries take layouts 0 .. 2 in either dtype
            assert (ops.attention_kernel(3, 197, 2, dt, layout=1, direction=direction) == -1) == (dt == F32 and not cls)
            assert (ops.attention_kernel(3, 197, 2, dt, layout=2, direction=direction) == -1) == (not cls)
            assert ops.attention_kernel(3, 197, 2, dt, layout=3, direction=direction) == -1
            assert ops.attention_kernel(3, 197, 2, dt, layout=-1, direction=direction) == -1
        d = L.ATTN_DIRECTIONS[direction]
        assert lib.gsl_attention_kernel_choice(3, 197, 2, 7, 0, d) == -1      # an unknown dtype
        assert lib.gsl_attention_kernel_choice(3, 197, 2, L.F32X3, 0, d) == -1      # (gsl_gemm_nt only)
    assert lib.gsl_attention_kernel_choice(3, 197, 2, L.BF16, 0, 4) == -1 and lib.gsl_attention_kernel_choice(3, 197, 2, L.BF16, 0, -1) == -1
