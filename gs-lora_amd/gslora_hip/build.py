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
# the second product library (include/gslora_train.h, prefix gst_): the weight-gradient GEMM and the quadratic regulariser of the FFN-training
# step. One translation unit, its own version script; built by build() with the first, opened only by a process that trains FFN weights.
TRAIN_SOURCES = ["train.hip"]
TRAIN_HEADERS = ["gsl_common.h", "exports_train.map"]
OUT_TRAIN = os.path.join(HERE, "libgslora_train.so")
# the third product library (include/gslora_reg.h, prefix gsr_): importance accumulation, MAS's objective and the batched quadratic regulariser
# of the L2 / EWC / MAS baselines. Made the way the second one is; opened only by a process that runs those baselines.
REG_SOURCES = ["reg.hip"]
REG_HEADERS = ["gsl_common.h", "exports_reg.map"]
OUT_REG = os.path.join(HERE, "libgslora_reg.so")
# the fourth product library (include/gslora_kd.h, prefix gsk_): the distillation + cross-entropy row loss and the batched parameter distance
# of the SCRUB baseline. Made the way the third one is; opened only by a process that runs a SCRUB step.
KD_SOURCES = ["kd.hip"]
KD_HEADERS = ["gsl_common.h", "exports_kd.map"]
OUT_KD = os.path.join(HERE, "libgslora_kd.so")
# the fifth product library (include/gslora_fd.h, prefix gsf_): the student-teacher row distance of the DER / DER++ and FDR baselines. Made the
# way the fourth one is; opened only by a process that takes a DER or FDR step.
FD_SOURCES = ["fd.hip"]
FD_HEADERS = ["gsl_common.h", "exports_fd.map"]
OUT_FD = os.path.join(HERE, "libgslora_fd.so")
# the sixth product library (include/gslora_at.h, prefix gsa_): the attention-transfer term of the LIRF baseline on the stream between the two
# half networks. Made the way the fifth one is; opened only by a process that takes a LIRF step.
AT_SOURCES = ["at.hip"]
AT_HEADERS = ["gsl_common.h", "exports_at.map"]
OUT_AT = os.path.join(HERE, "libgslora_at.so")


def needs_build(dev=False):
    out = OUT_DEV if dev else OUT
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS + (DEV_ONLY if dev else [])]
    deps.append(os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "gslora_hip.h"))
    return any(os.path.getmtime(d) > t for d in deps)


def _needs_build_side(out, sources, headers, header):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    inc = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include")
    deps = [os.path.join(CSRC, s) for s in sources + headers] + [os.path.join(inc, h) for h in ("gslora_hip.h", header)]
    return any(os.path.getmtime(d) > t for d in deps)


def needs_build_train():
    return _needs_build_side(OUT_TRAIN, TRAIN_SOURCES, TRAIN_HEADERS, "gslora_train.h")


def needs_build_reg():
    return _needs_build_side(OUT_REG, REG_SOURCES, REG_HEADERS, "gslora_reg.h")


def needs_build_kd():
    return _needs_build_side(OUT_KD, KD_SOURCES, KD_HEADERS, "gslora_kd.h")


def needs_build_fd():
    return _needs_build_side(OUT_FD, FD_SOURCES, FD_HEADERS, "gslora_fd.h")


def needs_build_at():
    return _needs_build_side(OUT_AT, AT_SOURCES, AT_HEADERS, "gslora_at.h")


def build_train(force=False, verbose=True):
    """libgslora_train.so: same flags as the product library, linked against csrc/exports_train.map."""
    if not force and not needs_build_train():
        return OUT_TRAIN
    return _build_side(OUT_TRAIN, TRAIN_SOURCES, "exports_train.map", "train", verbose)


def build_reg(force=False, verbose=True):
    """libgslora_reg.so: same flags as the product library, linked against csrc/exports_reg.map."""
    if not force and not needs_build_reg():
        return OUT_REG
    return _build_side(OUT_REG, REG_SOURCES, "exports_reg.map", "reg", verbose)


def build_kd(force=False, verbose=True):
    """libgslora_kd.so: same flags as the product library, linked against csrc/exports_kd.map."""
    if not force and not needs_build_kd():
        return OUT_KD
    return _build_side(OUT_KD, KD_SOURCES, "exports_kd.map", "kd", verbose)


def build_fd(force=False, verbose=True):
    """libgslora_fd.so: same flags as the product library, linked against csrc/exports_fd.map."""
    if not force and not needs_build_fd():
        return OUT_FD
    return _build_side(OUT_FD, FD_SOURCES, "exports_fd.map", "fd", verbose)


def build_at(force=False, verbose=True):
    """libgslora_at.so: same flags as the product library, linked against csrc/exports_at.map."""
    if not force and not needs_build_at():
        return OUT_AT
    return _build_side(OUT_AT, AT_SOURCES, "exports_at.map", "at", verbose)


def _build_side(out, sources, version_script, tag, verbose):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(HERE, "build", tag)
    os.makedirs(objdir, exist_ok=True)
    objs = []
    for src in sources:
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        objs.append(obj)
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print("[gslora_hip.build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + os.path.join(CSRC, version_script), "-o", out] + objs
    if verbose:
        print("[gslora_hip.build]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return out


def build(force=False, verbose=True, dev=False, defines=(), out=None, tag=None):
    """defines / out / tag: an A/B build of the product sources with extra -D flags into another file (tools/probes/, never loaded by
    default: `GSLORA_HIP_LIB=<out> python bench.py`). The plain product build (no dev, no variant) also builds libgslora_train.so,
    libgslora_reg.so, libgslora_kd.so, libgslora_fd.so and libgslora_at.so."""
    variant = out is not None
    if not variant and not dev:
        build_train(force=force, verbose=verbose)
        build_reg(force=force, verbose=verbose)
        build_kd(force=force, verbose=verbose)
        build_fd(force=force, verbose=verbose)
        build_at(force=force, verbose=verbose)
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
