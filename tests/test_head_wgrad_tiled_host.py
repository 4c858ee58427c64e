"""CPU tests of the class-tiled head weight gradient: the kernel is in the product library (where the spill and barrier checks of
tests/test_host_logic.py walk it), the header states the dispatch, the C ABI is what it was, the entry point's refusals hold above 1024
classes, and no LDS array of the new kernel has a run-time dimension."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "gslora_hip.h")).read()


def test_tiled_kernel_is_in_the_product_library():
    from gslora_hip import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"head_wgrad_tiled_kernel" in blob
    assert b"head_wgrad_kernel" in blob      # ... beside the per-class kernel, which C <= 1024 and the fallback still run


def test_header_states_the_dispatch_the_preconditions_and_the_fallback():
    hdr = header()
    comment = hdr[hdr.index("K10w head weight gradient"):hdr.index("GSL_API int gsl_head_wgrad")]
    for words in ("C <= 1024", "C > 1024", "D % 4 == 0", "emb 16-byte aligned", "falls back", "never refused", "one chain", "ascending b",
                  "backbone_forget_main.py:596-600", ":657-670", "vit_face.py:181-207"):
        assert words in comment, words


def test_no_entry_point_was_added_or_changed():
    from gslora_hip import _lib
    hdr = header()
    declared = set(re.findall(r"\b(gsl_[a-z0-9_]+)\s*\(", hdr)) - {"gsl_dropout_keep"}
    assert declared == set(_lib.SIGNATURES) and len(_lib.SIGNATURES) == 59      # (57 + the two LoRA-gradient plan queries)
    proto = re.search(r"GSL_API int gsl_head_wgrad\(([^;]*)\);", hdr).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES["gsl_head_wgrad"]) == 15


def test_entry_point_checks_its_arguments_before_any_launch_at_1100_classes():
    """tests/test_head_probe_host.py::test_entry_point_checks_its_arguments_before_any_launch with C = 1100: the same refusals, in front of
    the dispatch."""
    from gslora_hip import _lib
    L = _lib.load()
    p = 16      # a non-null, 16-byte-aligned address that is never dereferenced: the argument check fails first
    call = lambda **kw: L.gsl_head_wgrad(*[{**dict(dl=p, emb=p, W=p, label=p, cos_y=p, dW=p, db=None, B=4, C=1100, D=64, kind=0, s=64.0, m=0.5,
                                                  easy=0, stream=None), **kw}[k]
                                          for k in ("dl", "emb", "W", "label", "cos_y", "dW", "db", "B", "C", "D", "kind", "s", "m", "easy", "stream")])
    for bad in (dict(kind=3), dict(B=0), dict(D=1025), dict(D=0), dict(dW=None), dict(kind=1, label=None), dict(kind=1, cos_y=None),
                dict(kind=0, db=p), dict(kind=1, db=p), dict(kind=0, W=None), dict(dl=None), dict(emb=None)):
        assert call(**bad) == -1 and b"gsl_head_wgrad" in L.gsl_last_error(), bad
    assert call(C=0) == -1 and b"gsl_head_wgrad" in L.gsl_last_error()


def test_no_lds_array_of_the_tiled_kernel_has_a_run_time_dimension():
    src = open(os.path.join(ROOT, "gs-lora_amd", "csrc", "head.hip")).read()
    assert src.count("void head_wgrad_tiled_kernel(") == 1
    body = src[src.index("void head_wgrad_tiled_kernel("):src.index("constexpr int HWT_WIDE_C")]
    shared = re.findall(r"__shared__[^;]*;", body)
    assert len(shared) == 2
    consts = set()
    for line in re.findall(r"constexpr int ([^;]*);", body):
        consts |= set(re.findall(r"\b([A-Z][A-Z0-9]*)\s*=", line))
    for decl in shared:
        dims = re.findall(r"\[([^\]]*)\]", decl)
        assert dims and all(re.fullmatch(r"[A-Z_0-9 *+]+", d) for d in dims), decl      # compile-time tile constants only
        for d in dims:
            assert set(re.findall(r"[A-Z]+", d)) <= consts, (decl, consts)                # ... each a constexpr of the kernel
    for name in ("BK", "LDE", "LDG"):      # none of them is derived from B or C
        expr = re.search(rf"\b{name} = ([^;,]*)[;,]", body).group(1)
        assert not re.search(r"\b[BC]\b", expr), (name, expr)
    # the kernel sits behind head_wgrad_kernel, outside the two regions tests/test_head_large_c_host.py counts
    assert src.index("void head_wgrad_kernel(") < src.index("void head_wgrad_tiled_kernel(")
    assert src.index("// compact != 0 (pool = 'cls' only)") < src.index("void head_wgrad_tiled_kernel(")
