"""Compares the device code of two builds of one HIP source kernel by kernel, instruction by instruction.

    hipcc --offload-arch=gfx950 <the Makefile's HIPFLAGS> --cuda-device-only -S csrc/bq_render.hip -o this.s
    (the same on the other checkout -> parent.s)
    python tools/kernel_isa_diff.py parent.s this.s [--show N] [--pair OLD=NEW ...] [--forgive-kernarg-offset]

Every function of namespace bq in the first file is matched to the function of the second file with the same base name and
the same leading boolean template arguments (a kernel that gained trailing template parameters, as the render kernels did with
SOLID, matches its instantiation whose added booleans are all 0; where that rule finds several, the one with the same mangled
name); comments, directives and the numbering of branch labels are
dropped, everything else -- opcodes, registers, operands, order -- is compared.  Prints one line per kernel, IDENTICAL or
DIFFERENT (--show N: the first N lines of a unified diff), and exits 1 when any kernel differs or has no counterpart.
DESIGN.md section 27 uses it to show that the eight kernels of gpu_render_density are the code they were.

--pair OLD=NEW (repeatable) names the counterpart of a renamed kernel by its mangled names: OLD of the first file is compared
with NEW of the second (the fp32 / fp64 sweep kernels that became instantiations of one template, DESIGN.md "Twin sweep
kernels").  Kernels of the second file that nothing was compared with are listed as NEW ONLY and fail the run.

--forgive-kernarg-offset treats two lines as equal when both are the same scalar load from the kernel-argument pointer (the
user SGPR pair the kernel descriptor assigns to it) into the same registers and differ only in the immediate offset: a kernel
that gained an empty trailing argument finds its hidden arguments eight bytes further on.  All forgiven offsets of a kernel must
have grown by the same amount, and no load at or behind the first of them may have stayed.  Every forgiven line is counted and
printed per kernel."""
import argparse
import difflib
import re
import sys


def functions(path):
    """{mangled name: instructions} and {mangled name: the SGPR pair that holds the kernel-argument pointer}"""
    out, kernarg, cur, desc, first = {}, {}, None, None, 0
    for line in open(path):
        m = re.match(r"^(_ZN2bq\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        m = re.match(r"\s*\.amdhsa_kernel (\w+)", line)
        if m:
            desc, first = m.group(1), 0
            continue
        m = re.match(r"\s*\.amdhsa_user_sgpr_(private_segment_buffer|dispatch_ptr|queue_ptr|kernarg_segment_ptr) (\d)", line)
        if m and int(m.group(2)):       # the user SGPRs are handed out in this order
            if m.group(1) == "kernarg_segment_ptr":
                kernarg[desc] = f"s[{first}:{first + 1}]"
            first += 4 if m.group(1) == "private_segment_buffer" else 2
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
    return out, kernarg


def key(name):
    """(base name, leading boolean template arguments) of a mangled bq:: function"""
    m = re.match(r"_ZN2bq(\d+)", name)
    start = m.end()
    base, rest = name[start:start + int(m.group(1))], name[start + int(m.group(1)):]
    t = re.match(r"I((?:Lb[01]E)*)", rest)
    return base, tuple(re.findall(r"Lb([01])E", t.group(1))) if t else ()


def kernarg_load(line, ptr):
    """(opcode, destination), offset of a scalar load whose base is the kernel-argument pointer and whose offset is an immediate"""
    m = re.match(r"(s_load_dword\w*)\s+(\S+),\s*(s\[\d+:\d+\]),\s*(0x[0-9a-f]+|\d+)$", line)
    return ((m.group(1), m.group(2)), int(m.group(4), 0)) if m and m.group(3) == ptr else (None, 0)


def forgive(old, new, ptr_old, ptr_new):
    """`new` with the offsets of its kernel-argument loads set to `old`'s where the lines otherwise agree; the forgiven pairs.
    Arguments that moved behind a new one all moved by the same distance: the rule holds only when every forgiven offset grew by
    one and the same amount and no kernel-argument load at or behind the first moved offset stayed where it was (a reordering of
    the explicit arguments is not forgiven)."""
    if len(old) != len(new):
        return new, []
    out, forgiven, deltas, kept = [], [], set(), []
    for a, b in zip(old, new):
        (ka, oa), (kb, ob) = kernarg_load(a, ptr_old), kernarg_load(b, ptr_new)
        if a != b and ka is not None and ka == kb:
            forgiven.append((a, b))
            deltas.add(ob - oa)
            b = a
        elif ka is not None and a == b:
            kept.append(oa)
        out.append(b)
    if forgiven:
        first = min(kernarg_load(a, ptr_old)[1] for a, _ in forgiven)
        if len(deltas) != 1 or min(deltas) <= 0 or any(o >= first for o in kept):
            return new, []
    return out, forgiven


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--show", type=int, default=0)
    ap.add_argument("--pair", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--forgive-kernarg-offset", action="store_true")
    args = ap.parse_args()
    (old, ptr_old), (new, ptr_new) = functions(args.old), functions(args.new)
    pairs = dict(p.split("=", 1) for p in args.pair)
    bad, seen = 0, set()
    for name, code in old.items():
        base, bools = key(name)
        if name in pairs:
            match, label = [n for n in new if n == pairs[name]], f"{name} -> {pairs[name]}"
        else:
            match = [n for n in new if key(n)[0] == base and key(n)[1][:len(bools)] == bools and all(b == "0" for b in key(n)[1][len(bools):])]
            if len(match) != 1 and name in new:     # instantiations that differ in other than boolean arguments: by the whole mangled name
                match, base = [name], name
            label = f"{base}{list(bools)}"
        if len(match) != 1:
            print(f"{label}: {len(match)} counterparts")
            bad += 1
            continue
        seen.add(match[0])
        other, forgiven = new[match[0]], []
        if args.forgive_kernarg_offset:
            other, forgiven = forgive(code, other, ptr_old.get(name), ptr_new.get(match[0]))
        same = code == other
        bad += not same
        verdict = "IDENTICAL" if same else "DIFFERENT"
        if same and forgiven:
            verdict = f"IDENTICAL but for {len(forgiven)} kernel-argument offset(s)"
        print(f"{label}: {len(code)} / {len(other)} instructions, {verdict}")
        for a, b in forgiven:
            print(f"    forgiven: {a}  ->  {b}")
        if not same and args.show:
            for l in list(difflib.unified_diff(code, other, lineterm="", n=1))[:args.show]:
                print("    " + l)
    if pairs:
        for n in new:
            if n not in seen:
                print(f"{n}: NEW ONLY")
                bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
