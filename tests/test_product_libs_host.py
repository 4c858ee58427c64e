"""CPU tests of what the six product libraries have in common: each exports exactly its binding's names under its own prefix and nobody
else's, the build's table of side libraries says what it builds, nothing is stale after build(), and the one loader behind the six bindings
(gslora_hip/_cdll.py) keeps its messages. Each library's ABI against its header is tested in that library's own *_host.py file."""
import importlib
import os

import pytest

from product_libs import exported

# binding module, prefix, number of exported entry points; the side libraries in the order build() makes them
LIBS = {"hip": ("_lib", "gsl_", 59), "train": ("_lib_train", "gst_", 7), "reg": ("_lib_reg", "gsr_", 8), "kd": ("_lib_kd", "gsk_", 8),
        "fd": ("_lib_fd", "gsf_", 5), "at": ("_lib_at", "gsa_", 5)}


def out_of(tag):
    from gslora_hip import build
    return build.OUT if tag == "hip" else build.side_out(tag)


def test_every_library_exports_its_binding_s_names_under_its_own_prefix():
    for tag, (mod, prefix, n) in LIBS.items():
        binding = importlib.import_module("gslora_hip." + mod)
        got = exported(out_of(tag))
        assert got == set(binding.SIGNATURES) and len(got) == n, tag
        assert all(s.startswith(prefix) for s in got), tag
        assert binding.LIB_PATH == out_of(tag) or tag == "hip"      # the first library's path can be overridden (GSLORA_HIP_LIB)
        others = tuple(p for _, p, _ in LIBS.values() if p != prefix)
        assert not any(s.startswith(others) for s in got), tag


def test_the_table_of_side_libraries_is_what_build_makes():
    from gslora_hip import build
    assert list(build.SIDE_LIBS) == [t for t in LIBS if t != "hip"] == ["train", "reg", "kd", "fd", "at"]
    for tag, sources in build.SIDE_LIBS.items():
        assert sources == [tag + ".hip"]
        assert build.side_out(tag) == os.path.join(build.HERE, f"libgslora_{tag}.so")
        for dep in (os.path.join(build.CSRC, sources[0]), os.path.join(build.CSRC, f"exports_{tag}.map"),
                    os.path.join(os.path.dirname(os.path.dirname(build.HERE)), "include", f"gslora_{tag}.h")):
            assert os.path.exists(dep), dep
        assert build.needs_build_side(tag) is False, "nothing is stale after build()"
    assert build.needs_build() is False
    assert not [n for n in dir(build) if n.startswith(("OUT_", "build_", "needs_build_")) and n not in ("OUT_DEV", "build_side", "needs_build_side")]


def test_build_goes_through_the_table_in_its_order(monkeypatch):
    from gslora_hip import build
    calls = []
    monkeypatch.setattr(build, "build_side", lambda tag, force=False, verbose=True: calls.append((tag, force, verbose)))
    monkeypatch.setattr(build, "needs_build", lambda dev=False: False)      # this test compiles nothing
    build.build(verbose=False)
    assert calls == [(tag, False, False) for tag in build.SIDE_LIBS]
    calls.clear()
    build.build(dev=True, verbose=False)
    assert calls == [], "the dev build leaves the side libraries alone"


def test_the_loader_keeps_its_messages(tmp_path):
    from gslora_hip import _cdll, _lib_fd
    closing = "The DER / FDR baselines have no fallback."
    missing = str(tmp_path / "libgslora_fd.so")
    lib = _cdll.LazyLib(missing, _lib_fd.SIGNATURES, _lib_fd._RESTYPES, "gsf_last_error", closing)
    with pytest.raises(RuntimeError) as e:
        lib.load()
    assert str(e.value) == (f"libgslora_fd.so not found at {missing}. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                            f"(hipcc --offload-arch=gfx950). {closing}")
    assert not lib.loaded()
    junk = tmp_path / "libjunk.so"
    junk.write_bytes(b"not an ELF file")
    with pytest.raises(RuntimeError, match=f"^cannot load {junk}: "):
        _cdll.LazyLib(str(junk), {}, {}, "gsf_last_error", closing).load()
    invented = dict(_lib_fd.SIGNATURES, gsf_rowdist_invented=[])
    lib = _cdll.LazyLib(lambda: _lib_fd.LIB_PATH, invented, _lib_fd._RESTYPES, "gsf_last_error", closing)
    with pytest.raises(RuntimeError) as e:
        lib.load()
    assert str(e.value) == f"{_lib_fd.LIB_PATH} does not export gsf_rowdist_invented; rebuild the extension"
    assert not lib.loaded()
    lib = _cdll.LazyLib(lambda: _lib_fd.LIB_PATH, _lib_fd.SIGNATURES, _lib_fd._RESTYPES, "gsf_last_error", closing)
    assert not lib.loaded()
    assert lib.load() is lib.load() and lib.loaded()
    lib.check(0, "x")
    assert lib.nonneg(3, "f(1)") == 3
    assert lib.load().gsf_rowdist_ws_elems(0, 0) < 0      # a refused call: the library keeps why
    why = lib.load().gsf_last_error().decode()
    assert "gsf_rowdist_ws_elems" in why
    with pytest.raises(RuntimeError) as e:
        lib.check(1, "x")
    assert str(e.value) == f"x failed (code 1): {why}"
    with pytest.raises(RuntimeError) as e:
        lib.nonneg(-1, "gsf_rowdist_ws_elems(0, 0)")
    assert str(e.value) == f"gsf_rowdist_ws_elems(0, 0) refused: {why}"


def test_the_bindings_are_bound_to_one_loader_each_and_import_no_torch_of_their_own():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import gslora_hip._cdll, gslora_hip._lib as L\n"
            "assert 'torch' not in sys.modules and not [m for m in sys.modules if m.startswith('gslora_hip._lib_')]\n"
            "assert 'libgslora' not in open('/proc/self/maps').read()\n"
            "L.load(); assert 'libgslora_hip.so' in open('/proc/self/maps').read() and 'torch' not in sys.modules\n" % os.path.join(root, "gs-lora_amd"))
    subprocess.check_call([sys.executable, "-c", code])
    from gslora_hip import _cdll
    for mod, _, _ in list(LIBS.values())[1:]:
        binding = importlib.import_module("gslora_hip." + mod)
        assert isinstance(binding._L, _cdll.LazyLib)
        assert (binding.load, binding.loaded, binding.check) == (binding._L.load, binding._L.loaded, binding._L.check)
