#!/usr/bin/env python3
"""Two device listings of the same translation unit, compared function by
function (kernels and the device functions that stayed out of line):

    hipcc $HIPFLAGS --cuda-device-only -S csrc/engine.hip -o a.s     (each build)
    python scripts/kernel_listing_diff.py a.s b.s

Per function: whether the instruction text is equal (comments, debug and
alignment-free directives dropped; block labels renumbered per function) and,
for a kernel, whether its .amdhsa_* directives are; the instruction counts of
both.  Exit status 1 when a function differs or exists in one listing only
(profiles/psloop/device_code.txt).
"""
import re
import sys

DROP = re.compile(r"\s*\.(loc|file|cfi_\w+|ident|addrsig\w*|section|text|p2align|type|size|globl|weak|protected|hidden)\b")


def functions(path):
    """{name: (instruction lines, amdhsa lines or None)}"""
    text, amdhsa = {}, {}
    cur = kern = None
    types = set()
    lines = open(path, errors="replace").read().splitlines()
    for line in lines:
        m = re.match(r"\s*\.type\s+([\w.$]+),@function", line)
        if m:
            types.add(m.group(1))
    for line in lines:
        m = re.match(r"([\w.$]+):", line)
        if m and m.group(1) in types:
            cur = m.group(1)
            text[cur] = []
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            cur = None
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+([\w.$]+)", line)
        if m:
            kern = m.group(1)
            amdhsa[kern] = []
            continue
        if re.match(r"\s*\.end_amdhsa_kernel", line):
            kern = None
            continue
        body = line.split(";")[0].rstrip()
        if not body.strip():
            continue
        if kern is not None:
            amdhsa[kern].append(" ".join(body.split()))
        elif cur is not None and not DROP.match(body):
            # block labels carry the function's ordinal in the file: .LBB12_3 -> .LBB_3
            text[cur].append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", " ".join(body.split())))
    return {n: (t, amdhsa.get(n)) for n, t in text.items()}


def n_instr(t):
    return sum(1 for x in t if not x.endswith(":") and not x.startswith("."))


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    bad = 0
    print(f"{'function':<60} {'kind':<6} {'text':<9} {'amdhsa':<9} {'instr a':>8} {'instr b':>8}")
    for n in sorted(set(a) | set(b)):
        short = n if len(n) <= 60 else n[:57] + "..."
        if n not in a or n not in b:
            print(f"{short:<60} only in {'a' if n in a else 'b'}")
            bad += 1
            continue
        (ta, ha), (tb, hb) = a[n], b[n]
        kind = "kernel" if ha is not None or hb is not None else "func"
        same_t, same_h = ta == tb, ha == hb
        bad += not (same_t and same_h)
        print(f"{short:<60} {kind:<6} {'identical' if same_t else 'DIFFERS':<9} "
              f"{('identical' if same_h else 'DIFFERS') if kind == 'kernel' else '-':<9} {n_instr(ta):>8} {n_instr(tb):>8}")
    nk = sum(1 for n in a if a[n][1] is not None)
    print(f"{len(a)} functions in a ({nk} kernels), {len(b)} in b; {bad} differ or are missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
