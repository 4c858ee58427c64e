"""What the host tests read out of a built library: its exported names, its gfx950 code objects and each kernel's notes (the *_host.py
tests of the libraries, tests/test_host_logic.py, tests/test_product_libs_host.py)."""
import os
import re
import struct
import subprocess
import tempfile

import pytest

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def exported(so):
    nm = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    return {ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln}


def gfx950_code_objects(so):
    """The gfx950 entries of every clang offload bundle embedded in `so`, as bytes."""
    data = open(so, "rb").read()
    for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data):
        base = m.start()
        off = base + 32
        for _ in range(struct.unpack_from("<Q", data, base + 24)[0]):
            o, sz, tl = struct.unpack_from("<QQQ", data, off); off += 24
            triple = data[off:off + tl].decode(); off += tl
            if "gfx950" in triple and sz:
                yield data[base + o:base + o + sz]


def kernel_notes(so):
    """-> [(name, vgpr_spill_count, private_segment_fixed_size, max_flat_workgroup_size)] of every gfx950 kernel of `so`, read from the
    code-object notes. Skips the calling test where llvm-readelf is missing."""
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not in this image")
    kernels = []
    with tempfile.TemporaryDirectory() as d:
        for co in gfx950_code_objects(so):
            fn = os.path.join(d, "co.elf")
            open(fn, "wb").write(co)
            notes = subprocess.run([READELF, "--notes", fn], capture_output=True, text=True, check=True).stdout
            for blk in notes.split("- .agpr_count")[1:]:
                kernels.append((re.search(r"\.name:\s+(\S+)", blk).group(1),
                                *(int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))
                                  for key in ("vgpr_spill_count", "private_segment_fixed_size", "max_flat_workgroup_size"))))
    return kernels
