#!/usr/bin/env python3
"""python tools/diff_device_code.py PARENT.so NEW.so [NAME_PART ...]

Is the device code of two builds of the library the same? Every gfx950 code object of both files is disassembled
(llvm-objdump -d --no-show-raw-insn) and the instruction text compared function by function; addresses and the padding between
functions (s_nop, s_code_end) are ignored. Prints the counts, the names present on one side only and the names whose code differs, and
for every NAME_PART (say ln_ head_ lora_grad_) how many kernels (.kd descriptors) carry it on either side. Exit status 1 unless both
sides have the same functions with the same code. CPU only: nothing is loaded or run."""
import os
import re
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/llvm/bin/llvm-objdump")


def code_objects(path):
    """the gfx950 entries of every offload bundle in the file (one bundle per translation unit)"""
    blob = open(path, "rb").read()
    for m in re.finditer(MAGIC, blob):
        base = m.start()
        (n,) = struct.unpack_from("<Q", blob, base + len(MAGIC))
        pos = base + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, pos)
            triple = blob[pos + 24:pos + 24 + tlen].decode()
            pos += 24 + tlen
            if "gfx950" in triple and size:
                yield blob[base + off:base + off + size]


def functions(path):
    """name -> [instruction text, ...] (one per code object that defines the name), and the kernel names (symbols with a .kd descriptor)"""
    funcs, kernels = {}, set()
    for co in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", f.name], check=True, capture_output=True, text=True).stdout
            syms = subprocess.run([OBJDUMP, "-t", f.name], check=True, capture_output=True, text=True).stdout
        kernels |= {ln.split()[-1][:-3] for ln in syms.splitlines() if ln.endswith(".kd")}
        body = None
        for line in dis.splitlines():
            head = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if head:
                body = []
                funcs.setdefault(head.group(1), []).append(body)
            elif body is not None and line.strip():
                insn = line.split("//")[0].strip()
                if insn and not insn.startswith(("s_nop", "s_code_end")):
                    body.append(insn)
    return {k: sorted("\n".join(b) for b in v) for k, v in funcs.items()}, kernels


def main():
    fa, ka = functions(sys.argv[1])
    fb, kb = functions(sys.argv[2])
    both = sorted(set(fa) & set(fb))
    differ = [n for n in both if fa[n] != fb[n]]
    print(f"functions: {len(fa)} parent, {len(fb)} new, {len(both)} on both sides, {len(differ)} differ; kernels: {len(ka)} parent, {len(kb)} new")
    for part in sys.argv[3:]:
        print(f"kernels with '{part}': {sum(part in k for k in ka)} parent, {sum(part in k for k in kb)} new")
    for title, names in (("only in parent", sorted(set(fa) - set(fb))), ("only in new", sorted(set(fb) - set(fa))), ("differ", differ)):
        for n in names:
            print(f"{title}: {n}")
    return 0 if fa and not differ and set(fa) == set(fb) and ka == kb else 1


if __name__ == "__main__":
    sys.exit(main())
