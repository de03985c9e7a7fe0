#!/usr/bin/env python3
"""Are the kernels of two builds the same instructions?  Needs no GPU.

  python tools/compare_kernels.py OLD_BUILD_DIR NEW_BUILD_DIR intra_recon intra_recon_qp cu_qp deblock sao_frame

For every named object file (kvazaar_amd/csrc/build/NAME.o of two checkouts) the gfx950 code object is taken out of the fat binary and
disassembled with llvm-objdump -d; per function the instructions are compared without addresses, encodings and symbol names.  Every
function of the old build must have a function of the new build with the same instructions: "identical", or "identical but for
addresses" where only the pc-relative offsets of constant tables differ (s_add_u32 / s_addc_u32 after s_getpc_b64).  Exit status 1 if a
function differs.  This is how a change to a shared kernel header is shown to leave the existing kernels alone."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--" + os.environ.get("ARCH", "gfx950")


def functions(obj):
    """{symbol: [instruction]} of the device code in a hipcc object file"""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "a.fatbin"), os.path.join(d, "a.co")
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co])
        text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    out, cur = {}, None
    for line in text.splitlines():
        line = line.strip()
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line and line != "..." and "file format" not in line and not line.startswith("Disassembly"):
            cur.append(re.sub(r"\s+", " ", re.sub(r"//.*$", "", re.sub(r"<[^>]*>", "", line))).strip())
    return out


def without_addresses(body):
    return [re.sub(r"(s_addc?_u32 s\d+, s\d+, )0x[0-9a-f]+", r"\1ADDR", l) for l in body]


def main():
    old_dir, new_dir, names = sys.argv[1], sys.argv[2], sys.argv[3:]
    differs = 0
    for n in names:
        old, new = functions(os.path.join(old_dir, n + ".o")), functions(os.path.join(new_dir, n + ".o"))
        for sym, body in old.items():
            if any(b == body for b in new.values()):
                verdict = "identical"
            elif any(without_addresses(b) == without_addresses(body) for b in new.values()):
                verdict = "identical but for addresses"
            else:
                verdict = "DIFFERS"
                differs += 1
            print("%-16s %7d instructions  %-28s %s" % (n, len(body), verdict, sym))
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
