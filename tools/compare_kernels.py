#!/usr/bin/env python3
"""Are the kernels of a translation unit the same, instruction for instruction, in two source trees?
    python tools/compare_kernels.py <other tree> gsss_fast_vmf_d3.hip gsss_fast_bingham.hip
compiles each unit's device code for gfx950 from this tree and from the other one (the build's flags), disassembles both code
objects with llvm-objdump and compares the function bodies by name.  Two things are normalised: a kernel whose template
arguments only gained a trailing `false` flag and an empty argument pack is the same kernel, and the literal that follows
s_getpc_b64 (the pc-relative address of a table) depends on where the object was laid out, not on the kernel.
The name normalisation is that of ONE change -- the BATCH flag and BatchBlock pack that run_kernel, screened_kernel and fast_kernel
gained with TargetBatch: a tree with further template parameters reports its kernels as missing, and `replace` below needs the
new suffix."""
import os, re, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from geosss_amd import build

LLVM = os.path.join(os.path.dirname(os.path.realpath(build.hipcc())), "..", "lib", "llvm", "bin")


def functions(tree, unit, tmp, tag):
    co, elf = os.path.join(tmp, f"{tag}.co"), os.path.join(tmp, f"{tag}.elf")
    subprocess.run([build.hipcc(), *build.CXXFLAGS, *build.source_flags(unit), "--cuda-device-only", "-c",
                    os.path.join(tree, "geosss_amd", "csrc", unit), "-o", co], check=True, capture_output=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                    f"--targets=hip-amdgcn-amd-amdhsa--{build.ARCH}", f"--input={co}", f"--output={elf}"], check=True)
    out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", elf],
                         check=True, capture_output=True, text=True).stdout
    cur, since_pc, d = None, 99, {}
    for line in out.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:$", line)
        if m:
            cur = re.sub(r"DpT\d+_$", "", m.group(1).replace("Lb0EJEEEvNS", "EEvNS"))
            d[cur] = []
        elif cur and line.strip():
            ins = re.sub(r"\s*//.*$", "", line).strip()
            since_pc = 0 if ins.startswith("s_getpc_b64") else since_pc + 1
            if since_pc in (1, 2) and ins.startswith(("s_add_u32", "s_addc_u32")):
                ins = re.sub(r"0x[0-9a-f]+$", "<pcrel>", ins)
            d[cur].append(ins)
    return d


def main():
    other, units = sys.argv[1], sys.argv[2:]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for unit in units:
            a, b = functions(other, unit, tmp, "other"), functions(HERE, unit, tmp, "this")
            same = [k for k in a if a[k] == b.get(k)]
            diff = [k for k in a if k in b and a[k] != b[k]]
            gone = [k for k in a if k not in b]
            bad += len(diff) + len(gone)
            print(f"{unit}: {len(a)} kernels there, {len(b)} here; identical bodies: {len(same)} ({sum(len(a[k]) for k in same)} "
                  f"instructions), different: {len(diff)}, missing here: {len(gone)}, new here: {len([k for k in b if k not in a])}")
            for k in diff + gone:
                print("   ", k)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
