#!/usr/bin/env python3
"""Compare two device assembly files kernel by kernel.

    hipcc $(FLAGS) --cuda-device-only -S csrc/conv_dma.hip -o before.s      (FLAGS: csrc/Makefile)
    ... the same on the other tree -> after.s
    tools/compare_kernel_isa.py before.s after.s [--label NAME]

A refactor that must not change what the GPU executes is checked this way without a GPU: every kernel (and every device function that
was not inlined) of the two builds is compared line by line after dropping comments, debug directives and blank lines.  Per kernel the
tool prints `identical`, or the first differing line together with the register / scratch / LDS figures of both builds.  It compares two
builds; it does not look for particular instructions.  Exit status 1 if any kernel differs or exists on one side only.
"""
import argparse
import re
import sys

FIGURES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
DROP = re.compile(r"^\s*\.(loc|file|cfi_\w+|cv_\w+|ident|addrsig\w*)\b")
FUNC = re.compile(r"^([A-Za-z_$][\w$.]*):")


def strip(line):
    line = line.split(";", 1)[0].rstrip()           # (no string operands carry ';' in device assembly bodies)
    if not line.strip() or DROP.match(line):
        return None
    return " ".join(line.split())


def parse_figures(path):
    """The per-kernel records of the amdhsa.kernels metadata: figures keyed by kernel name (keys of a record are sorted, `.name` among them)."""
    out, rec = {}, {}
    inside = False
    with open(path, errors="replace") as f:
        for raw in f:
            s = raw.rstrip("\n")
            if s.strip() == "amdhsa.kernels:":
                inside = True
                continue
            if not inside:
                continue
            if s.startswith("amdhsa.") or s.strip() == "...":
                break
            if s.startswith("  - "):                     # a new kernel record
                if ".name" in rec:
                    out[rec[".name"]] = rec
                rec = {}
                s = "    " + s[4:]
            m = re.match(r"^    (\.[a-z_]+):\s*(\S+)\s*$", s)
            if m and (m.group(1) in FIGURES or m.group(1) == ".name"):
                rec[m.group(1)] = m.group(2).strip("'\"")
    if ".name" in rec:
        out[rec[".name"]] = rec
    return out


def parse_bodies(path):
    bodies, cur, funcs = {}, None, set()
    with open(path, errors="replace") as f:
        for raw in f:
            s = raw.strip()
            if s.startswith("amdhsa.kernels:") or s.startswith(".amdgpu_metadata"):
                break
            m = re.match(r"^\.type\s+([^\s,]+),@function", s)
            if m:
                funcs.add(m.group(1))
                continue
            m = FUNC.match(raw)
            if m:
                cur = m.group(1) if m.group(1) in funcs else None      # (data objects such as the per-file __hip_cuid_* are no code)
                if cur:
                    bodies.setdefault(cur, [])
                continue
            if s.startswith(".amdhsa_kernel "):
                cur = s.split()[1] + " [descriptor]"
                bodies.setdefault(cur, [])
                continue
            if cur is None:
                continue
            t = strip(raw)
            if t is not None and not t.startswith((".section", ".p2align", ".globl", ".protected", ".type", ".size", ".weak", ".hidden", ".text", ".set ")):
                bodies[cur].append(t)
            if s == ".end_amdhsa_kernel" or s.startswith(".Lfunc_end"):
                cur = None
    return bodies


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--label", default=None, help="heading printed above the report")
    args = ap.parse_args()
    b0, b1 = parse_bodies(args.before), parse_bodies(args.after)
    f0, f1 = parse_figures(args.before), parse_figures(args.after)
    names = sorted(n for n in set(b0) | set(b1) if not n.endswith(" [descriptor]"))
    same = diff = 0
    print(f"== {args.label or args.before + ' vs ' + args.after}: {len(names)} kernels / functions")
    for n in names:
        if n not in b0 or n not in b1:
            print(f"{n}: only in {'after' if n not in b0 else 'before'}")
            diff += 1
            continue
        x = b0[n] + b0.get(n + " [descriptor]", [])
        y = b1[n] + b1.get(n + " [descriptor]", [])
        if x == y and f0.get(n) == f1.get(n):
            print(f"{n}: identical ({len(b0[n])} lines)")
            same += 1
            continue
        diff += 1
        k = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
        print(f"{n}: DIFFERS at line {k + 1} ({len(x)} vs {len(y)} lines)")
        print(f"    before: {x[k] if k < len(x) else '<end>'}")
        print(f"    after:  {y[k] if k < len(y) else '<end>'}")
        for fig in FIGURES:
            print(f"    {fig}: {f0.get(n, {}).get(fig, '?')} -> {f1.get(n, {}).get(fig, '?')}")
    print(f"== {same} identical, {diff} different")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
