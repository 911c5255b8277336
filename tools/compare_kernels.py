#!/usr/bin/env python3
"""Are the kernels the same, instruction for instruction, in two source trees?
    python tools/compare_kernels.py <other tree> [gsss_fast_vmf_d3.hip gsss_fast_bingham.hip ...]
compiles each unit's device code for gfx950 from this tree and from the other one (the build's flags), disassembles both code
objects with llvm-objdump and compares the function bodies by their mangled names.  No unit named: every unit of
build.sources().  Reported per unit and for the union of the kernels over all units (a kernel may move between units; in the
union a name counts as different if any of its bodies differs).  Normalised: the literal that follows s_getpc_b64 (the
pc-relative address of a table) and the padding behind a function depend on where the object was laid out, not on the kernel.  Up to 16 compilations run in
parallel (--jobs)."""
import argparse, concurrent.futures as cf, os, re, subprocess, sys, tempfile

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
            cur = m.group(1)
            d[cur] = []
        elif cur and line.strip() and line.strip() != "...":  # ("...": objdump's mark for the zero padding behind a function)
            ins = re.sub(r"\s*//.*$", "", line).strip()
            since_pc = 0 if ins.startswith("s_getpc_b64") else since_pc + 1
            if since_pc in (1, 2) and ins.startswith(("s_add_u32", "s_addc_u32")):
                ins = re.sub(r"0x[0-9a-f]+$", "<pcrel>", ins)
            d[cur].append(ins)
    return d


def report(label, a, b):
    """a, b: {kernel: body} there and here.  Prints one line (and the offenders), returns how many differ or are missing."""
    same = [k for k in a if a[k] == b.get(k)]
    diff = [k for k in a if k in b and a[k] != b[k]]
    gone = [k for k in a if k not in b]
    new = [k for k in b if k not in a]
    print(f"{label}: {len(a)} kernels there, {len(b)} here; identical bodies: {len(same)} ({sum(len(a[k]) for k in same)} "
          f"instructions), different: {len(diff)}, missing here: {len(gone)}, new here: {len(new)}")
    for k in diff + gone + new:
        print("   ", "different" if k in diff else "missing  " if k in gone else "new      ", k)
    return len(diff) + len(gone) + len(new)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other", help="the other source tree")
    ap.add_argument("units", nargs="*", help="translation units (default: every unit of the build)")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    units = a.units or build.sources()
    for unit in units:
        build.source_flags(unit)  # (probe the optional flags once, before the threads)
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(max(1, min(16, a.jobs))) as ex:
        def side(tree, tag):
            def one(unit):
                if not os.path.exists(os.path.join(tree, "geosss_amd", "csrc", unit)):
                    return {}
                return functions(tree, unit, tmp, f"{tag}_{unit}")
            return one
        there = list(ex.map(side(a.other, "other"), units))
        here = list(ex.map(side(HERE, "this"), units))
    union_there, union_here = {}, {}
    for union, per_unit in ((union_there, there), (union_here, here)):
        for fns in per_unit:
            for k, body in fns.items():  # one name, several bodies (weak copies in several units): all of them
                union.setdefault(k, set()).add(tuple(body))
    for unit, x, y in zip(units, there, here):
        report(unit, x, y)
    bad = report("union of all units", union_there, union_here)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
