"""Compares the device code of two builds of one HIP source kernel by kernel, instruction by instruction.

    hipcc --offload-arch=gfx950 <the Makefile's HIPFLAGS> --cuda-device-only -S csrc/bq_render.hip -o this.s
    (the same on the other checkout -> parent.s)
    python tools/kernel_isa_diff.py parent.s this.s [--show N]

Every function of namespace bq in the first file is matched to the function of the second file with the same base name and
the same leading boolean template arguments (a kernel that gained trailing template parameters, as the render kernels did with
SOLID, matches its instantiation whose added booleans are all 0; where that rule finds several, the one with the same mangled
name); comments, directives and the numbering of branch labels are
dropped, everything else -- opcodes, registers, operands, order -- is compared.  Prints one line per kernel, IDENTICAL or
DIFFERENT (--show N: the first N lines of a unified diff), and exits 1 when any kernel differs or has no counterpart.
DESIGN.md section 27 uses it to show that the eight kernels of gpu_render_density are the code they were."""
import argparse
import difflib
import re
import sys


def functions(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_ZN2bq\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        s = line.strip()
        if not s or s.startswith(";") or (s.startswith(".") and not s.startswith(".LBB")):
            continue
        s = re.sub(r"\s*;.*", "", s)
        out[cur].append(re.sub(r"\.LBB\d+_", ".LBBn_", s))
    return out


def key(name):
    """(base name, leading boolean template arguments) of a mangled bq:: function"""
    m = re.match(r"_ZN2bq(\d+)", name)
    start = m.end()
    base, rest = name[start:start + int(m.group(1))], name[start + int(m.group(1)):]
    t = re.match(r"I((?:Lb[01]E)*)", rest)
    return base, tuple(re.findall(r"Lb([01])E", t.group(1))) if t else ()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--show", type=int, default=0)
    args = ap.parse_args()
    old, new = functions(args.old), functions(args.new)
    bad = 0
    for name, code in old.items():
        base, bools = key(name)
        match = [n for n in new if key(n)[0] == base and key(n)[1][:len(bools)] == bools and all(b == "0" for b in key(n)[1][len(bools):])]
        if len(match) != 1 and name in new:     # instantiations that differ in other than boolean arguments: by the whole mangled name
            match, base = [name], name
        if len(match) != 1:
            print(f"{base}{list(bools)}: {len(match)} counterparts")
            bad += 1
            continue
        same = code == new[match[0]]
        bad += not same
        print(f"{base}{list(bools)}: {len(code)} / {len(new[match[0]])} instructions, {'IDENTICAL' if same else 'DIFFERENT'}")
        if not same and args.show:
            for l in list(difflib.unified_diff(code, new[match[0]], lineterm="", n=1))[:args.show]:
                print("    " + l)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
