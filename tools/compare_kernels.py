#!/usr/bin/env python3
"""Are the kernels the same, instruction for instruction, in two source trees?
    python tools/compare_kernels.py <other tree> [gsss_fast_vmf_d3.hip gsss_fast_bingham.hip ...]
compiles each unit's device code for gfx950 from this tree and from the other one (the build's flags), disassembles both code
objects with llvm-objdump and compares the function bodies by their mangled names.  No unit named: every unit of
build.sources().  Reported per unit and for the union of the kernels over all units (a kernel may move between units; in the
union a name counts as different if any of its bodies differs).  Normalised: the literal that follows s_getpc_b64 (the
pc-relative address of a table) and the padding behind a function depend on where the object was laid out, not on the kernel.  Up to 16 compilations run in
parallel (--jobs).  A body that differs is also compared by its count per opcode with s_nop and s_waitcnt left out: equal
counts mean the same work in another order ("scheduling only"); failing that, equal counts over every opcode that ends in _f64,
every opcode that begins with global_, flat_ or buffer_, and s_barrier mean "the same arithmetic and memory work" around other
integer and scalar bookkeeping.  The exit status is 0 if no kernel differs by more than its schedule -- with --same-work-ok, by
more than that bookkeeping -- (and, with --resources, in no figure), else 1.
    python tools/compare_kernels.py --resources <other tree> [units ...]
compares each kernel's resource figures as well, in the code object's metadata: VGPRs (all of them; AGPRs are among them and
also given alone), SGPRs, spills, scratch and static LDS bytes, and the wavefronts per SIMD that the registers allow (512 / VGPRs
in blocks of 8, at most 8: derived, not stored)."""
import argparse, collections, concurrent.futures as cf, os, re, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from geosss_amd import build

LLVM = os.path.join(os.path.dirname(os.path.realpath(build.hipcc())), "..", "lib", "llvm", "bin")


RESOURCE_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                 "private_segment_fixed_size", "group_segment_fixed_size")


def resources(elf):
    """{kernel: its figures} from the AMDGPU metadata note (a kernel's entry starts at the list's own indent; a key the entry
    does not carry counts as -1)."""
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", elf], check=True, capture_output=True, text=True).stdout
    d = {}
    for entry in re.split(r"^  - (?=\.)", notes, flags=re.M)[1:]:
        name = re.search(r"^\s*\.name:\s*(\S+)", entry, re.M)
        if not name:
            continue
        found = (re.search(rf"^\s*\.{k}:\s*(\d+)", entry, re.M) for k in RESOURCE_KEYS)
        fig = tuple(int(m.group(1)) if m else -1 for m in found)
        d[name.group(1)] = fig + (min(8, 512 // max(8, -(-fig[0] // 8) * 8)),)
    return d


def scheduling_only(x, y):
    def count(body):
        return collections.Counter(i.split()[0] for i in body if not i.startswith(("s_nop", "s_waitcnt")))
    return count(x) == count(y)


def same_work(x, y):
    def count(body):
        ops = (i.split()[0] for i in body)
        return collections.Counter(o for o in ops if o.endswith("_f64") or o.startswith(("global_", "flat_", "buffer_")) or o == "s_barrier")
    return count(x) == count(y)


# how far a differing body is from the other one
VERDICTS = ("scheduling only", "same arithmetic and memory work", "OTHER OPCODE COUNTS")


def functions(tree, unit, tmp, tag, want_resources=False):
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
    return d, (resources(elf) if want_resources else {})


def report(label, a, b, sched=None, allow=0):
    """a, b: {kernel: body} there and here (resources: its figures; the union: the set of its bodies or figures).  `sched`:
    {kernel: the worst verdict (index into VERDICTS) of its differing bodies}, filled from the units' bodies and read for the
    union.  Prints one line and the offenders; returns how many are missing, new or differ by a verdict beyond `allow`."""
    same = [k for k in a if a[k] == b.get(k)]
    diff = [k for k in a if k in b and a[k] != b[k]]
    gone = [k for k in a if k not in b]
    new = [k for k in b if k not in a]
    print(f"{label}: {len(a)} kernels there, {len(b)} here; identical: {len(same)}, different: {len(diff)}, "
          f"missing here: {len(gone)}, new here: {len(new)}")
    worse, by_verdict = 0, [0] * len(VERDICTS)
    for k in diff + gone + new:
        note, verdict = "", len(VERDICTS) - 1
        if k in diff and isinstance(a[k], list):  # one unit's bodies
            verdict = 0 if scheduling_only(a[k], b[k]) else (1 if same_work(a[k], b[k]) else 2)
            if sched is not None:
                sched[k] = max(verdict, sched.get(k, 0))
            note = f"  [{len(a[k])} -> {len(b[k])} instructions, {VERDICTS[verdict]}]"
        elif k in diff and isinstance(a[k], tuple):  # one unit's resource figures
            note = f"  {a[k]} -> {b[k]}"
        elif k in diff and sched is not None and k in sched:  # the union of the bodies
            verdict = sched[k]
            note = f"  [{VERDICTS[verdict]}]"
        worse += verdict > allow
        by_verdict[verdict] += k in diff
        print("   ", "different" if k in diff else "missing  " if k in gone else "new      ", k + note)
    if diff:
        print(f"    of the different: scheduling only {by_verdict[0]}, same arithmetic and memory work {by_verdict[1]}, "
              f"more than that {by_verdict[2]}")
    return worse


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other", help="the other source tree")
    ap.add_argument("units", nargs="*", help="translation units (default: every unit of the build)")
    ap.add_argument("--resources", action="store_true", help="also compare resource figures " + str(RESOURCE_KEYS + ("waves/SIMD",)))
    ap.add_argument("--same-work-ok", action="store_true",
                    help='the exit status treats "same arithmetic and memory work" like "scheduling only"')
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    units = a.units or build.sources()
    for unit in units:
        build.source_flags(unit)  # (probe the optional flags once, before the threads)
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(max(1, min(16, a.jobs))) as ex:
        def side(tree, tag):
            def one(unit):
                if not os.path.exists(os.path.join(tree, "geosss_amd", "csrc", unit)):
                    return {}, {}
                return functions(tree, unit, tmp, f"{tag}_{unit}", a.resources)
            return one
        there = list(ex.map(side(a.other, "other"), units))
        here = list(ex.map(side(HERE, "this"), units))
    bad, allow = 0, 1 if a.same_work_ok else 0
    for what in range(2 if a.resources else 1):  # the bodies, then the resource figures
        union_there, union_here, sched = {}, {}, ({} if what == 0 else None)
        for union, per_unit in ((union_there, there), (union_here, here)):
            for fns in per_unit:
                for k, body in fns[what].items():  # one name, several bodies (weak copies in several units): all of them
                    union.setdefault(k, set()).add(tuple(body))
        for unit, x, y in zip(units, there, here):
            report(unit + (" resources" if what else ""), x[what], y[what], sched, allow)
        bad += report("union of all units" + (" resources" if what else ""), union_there, union_here, sched, allow)
    # exit status: 0 if every kernel is identical or differs by an allowed verdict only (and, with --resources, in no figure)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
