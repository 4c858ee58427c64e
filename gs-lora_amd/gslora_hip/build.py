"""Build libgslora_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

Two libraries from the same sources:
  libgslora_hip.so      the PRODUCT: the kernels its launch rules reach (gemm_tile_choice, attn_kernel_choice) and no others,
                        -fvisibility=hidden (exactly the entry points of include/gslora_hip.h are exported), no getenv() on any launch path.
  libgslora_hip_dev.so  the LAB (-DGSL_DEV): additionally the GEMM variants that lost their A/Bs (csrc/gemm_dev_*.inc), the two-kernel
                        attention backward at T > 64, and the ablation / variant knobs and cycle-stamp buffers that tools/bench_gemm*.py,
                        tools/bench_attn.py and tools/probes/ drive through the environment (csrc/gemm_dev_launch.inc,
                        csrc/attention_dev_launch.inc). Built on demand (`python -m gslora_hip.build --dev`), selected with GSLORA_HIP_LIB; never loaded
                        by default.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "csrc")
SOURCES = ["gemm.hip", "norm.hip", "lora.hip", "patch.hip", "head.hip", "loss.hip", "attention.hip", "verif.hip", "classstat.hip"]
# translation units that are compiled a second time with -DGSL_OP_F16: the same kernels with IEEE fp16 MFMA operands (dtype GSL_F16), in
# namespace gsl_h16, behind hidden h16_<entry> symbols that the exported entry points forward to (csrc/gsl_common.h, csrc/gsl_h16.h)
SOURCES_F16 = ["gemm.hip", "attention.hip"]
HEADERS = ["gsl_common.h", "gsl_h16.h", "exports.map", "gelu_g8_table.inc"]
DEV_ONLY = ["gemm_dev_a.inc", "gemm_dev_b.inc", "gemm_dev_c.inc", "gemm_dev_launch.inc", "gemm_w4.inc", "gemm_o4.inc", "attention_dev_launch.inc"]
OUT = os.path.join(HERE, "libgslora_hip.so")
OUT_DEV = os.path.join(HERE, "libgslora_hip_dev.so")
# The side libraries, in build order: tag -> sources. Each is libgslora_<tag>.so with the public header include/gslora_<tag>.h, the version
# script csrc/exports_<tag>.map and the objects under build/<tag>; built by build() with the product library, same flags, and opened only by
# a process that uses it (gslora_hip/_lib_<tag>.py). train (gst_): the weight-gradient GEMM and quadratic regulariser of the FFN-training
# step; reg (gsr_): importance accumulation, MAS's objective and the batched regulariser of L2 / EWC / MAS; kd (gsk_): SCRUB's distillation
# + cross-entropy row loss and batched parameter distance; fd (gsf_): the student-teacher row distance of DER / DER++ / FDR; at (gsa_): the
# attention-transfer term of LIRF.
SIDE_LIBS = {"train": ["train.hip"], "reg": ["reg.hip"], "kd": ["kd.hip"], "fd": ["fd.hip"], "at": ["at.hip"]}


def side_out(tag):
    return os.path.join(HERE, f"libgslora_{tag}.so")


def needs_build(dev=False):
    out = OUT_DEV if dev else OUT
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS + (DEV_ONLY if dev else [])]
    deps.append(os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "gslora_hip.h"))
    return any(os.path.getmtime(d) > t for d in deps)


def needs_build_side(tag):
    out = side_out(tag)
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    inc = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include")
    deps = [os.path.join(CSRC, s) for s in SIDE_LIBS[tag] + ["gsl_common.h", "gsl_chunks.h", f"exports_{tag}.map"]]
    deps += [os.path.join(inc, h) for h in ("gslora_hip.h", f"gslora_{tag}.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build_side(tag, force=False, verbose=True):
    """libgslora_<tag>.so: same flags as the product library, linked against csrc/exports_<tag>.map."""
    out = side_out(tag)
    if not force and not needs_build_side(tag):
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(HERE, "build", tag)
    os.makedirs(objdir, exist_ok=True)
    objs = []
    for src in SIDE_LIBS[tag]:
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        objs.append(obj)
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print("[gslora_hip.build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + os.path.join(CSRC, f"exports_{tag}.map"), "-o", out] + objs
    if verbose:
        print("[gslora_hip.build]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return out


def build(force=False, verbose=True, dev=False, defines=(), out=None, tag=None):
    """defines / out / tag: an A/B build of the product sources with extra -D flags into another file (tools/probes/, never loaded by
    default: `GSLORA_HIP_LIB=<out> python bench.py`). The plain product build (no dev, no variant) also builds every side library."""
    variant = out is not None
    if not variant and not dev:
        for side in SIDE_LIBS:
            build_side(side, force=force, verbose=verbose)
    out = out or (OUT_DEV if dev else OUT)
    if not variant and not force and not needs_build(dev):
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(HERE, "build", tag or ("dev" if dev else "prod"))
    os.makedirs(objdir, exist_ok=True)
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden"] + (["-DGSL_DEV"] if dev else []) + list(defines)
    procs = []
    objs = []
    units = [(src, src.replace(".hip", ".o"), []) for src in SOURCES] + [(src, src.replace(".hip", "_f16.o"), ["-DGSL_OP_F16"]) for src in SOURCES_F16]
    units.sort(key=lambda u: u[0] != "gemm.hip")      # the two gemm.hip compiles dominate: start them first
    for src, oname, extra in units:      # one hipcc per translation unit, in parallel
        obj = os.path.join(objdir, oname)
        objs.append(obj)
        cmd = [hipcc] + flags + extra + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print("[gslora_hip.build]", " ".join(cmd), flush=True)
        procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, p in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + os.path.join(CSRC, "exports.map"), "-o", out] + objs
    if verbose:
        print("[gslora_hip.build]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return out


if __name__ == "__main__":
    # python -m gslora_hip.build [--force] [--dev] [--variant NAME -DX=1 ...]  (variant -> <repo>/build_variants/libgslora_hip_NAME.so)
    if "--variant" in sys.argv:
        name = sys.argv[sys.argv.index("--variant") + 1]
        vdir = os.path.join(os.path.dirname(os.path.dirname(HERE)), "build_variants")
        os.makedirs(vdir, exist_ok=True)
        print(build(defines=[a for a in sys.argv if a.startswith("-D")], out=os.path.join(vdir, f"libgslora_hip_{name}.so"), tag="variant_" + name,
                    dev="--dev" in sys.argv))
    else:
        build(force="--force" in sys.argv, dev="--dev" in sys.argv)
