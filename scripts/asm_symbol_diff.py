#!/usr/bin/env python3
"""Compare kernels between two builds' assembly listings (`make asm` output, *.s).

    asm_symbol_diff.py BEFORE AFTER OLD_SYMBOL=NEW_SYMBOL [OLD=NEW ...]
    asm_symbol_diff.py --all BEFORE AFTER

BEFORE and AFTER are each one listing or several joined by commas: a kernel is looked up in
whichever listing of its side defines it. --all pairs every kernel of either side with the kernel
of the same name on the other; a kernel that only one side has counts as a difference.

For each pair two things are compared line by line: the instructions between the symbol's label
and its kernel descriptor (comments and the symbol's own name stripped, the function's number
taken out of local labels), and the descriptor's .amdhsa_kernel ... .end_amdhsa_kernel block
(registers, LDS, scratch, kernarg size). Exit status 1 if any pair differs. DESIGN.md §4.16 used it
to show that the static instantiations of temporal_accumulate did not change when the MOTION
parameter was added, §4.18 that no kernel changed when rt_kernel.hip was split.
"""
import re
import sys


def kernels(paths):
    """{kernel name: (instructions, descriptor)} over the listings, each a list of lines."""
    found = {}
    for path in paths.split(","):
        lines = [line.split(";")[0].rstrip() for line in open(path).read().splitlines()]
        for k, line in enumerate(lines):
            if not line.strip().startswith(".amdhsa_kernel "):
                continue
            name = line.split()[1]
            if name in found:
                sys.exit(f"{name}: defined twice in {paths}")
            end = next(i for i in range(k, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
            start = max(i for i in range(k) if lines[i] == name + ":")
            found[name] = (body(lines[start + 1:k], name), [l.strip().replace(name, "SYM") for l in lines[k:end]])
    return found


def body(lines, symbol):
    out = []
    for line in lines:
        if line.strip().startswith(".section"):
            break  # (the kernel descriptor follows)
        if not line or line.lstrip().startswith((".loc", ".file", ".cfi")):
            continue
        line = re.sub(r"\.L([A-Za-z_]*)\d+_(\d+)", r".L\1_\2", line.replace(symbol, "SYM"))
        out.append(re.sub(r"\.L([A-Za-z_]*)\d+\b", r".L\1", line))
    return out


def main(argv):
    every = argv[1:2] == ["--all"]
    before, after = (kernels(p) for p in argv[2 if every else 1:][:2])
    pairs = sorted(set(before) | set(after)) if every else argv[3:]
    bad = 0
    for pair in pairs:
        old, new = pair.split("=") if "=" in pair else (pair, pair)
        if old not in before or new not in after:
            print(f"{pair}: MISSING {'before' if old not in before else 'after'}")
            bad += 1
            continue
        (a, da), (b, db) = before[old], after[new]
        same = a == b and da == db
        what = "identical" if same else "DIFFERENT" + (" instructions" if a != b else "") + (" descriptor" if da != db else "")
        print(f"{old if old == new else old + ' -> ' + new}: {len(a)} / {len(b)} lines, descriptor {len(da)} / {len(db)}, {what}")
        bad += 0 if same else 1
    print(f"{len(pairs)} kernels, {len(pairs) - bad} identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
