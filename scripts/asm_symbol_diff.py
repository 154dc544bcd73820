#!/usr/bin/env python3
"""Compare the machine code of kernels between two assembly listings (`make asm` output, *.s).

    asm_symbol_diff.py before.s after.s OLD_SYMBOL=NEW_SYMBOL [OLD=NEW ...]

For each pair the instructions between the symbol's label and its .Lfunc_end are taken, comments
and the symbol's own name are stripped, and the two bodies are compared line by line. Exit status 1
if any pair differs. DESIGN.md §4.16 used it to show that the static instantiations of
temporal_accumulate did not change when the MOTION parameter was added.
"""
import re
import sys


def body(path, symbol):
    lines = open(path).read().splitlines()
    start = next(i for i, line in enumerate(lines) if line.split(";")[0].strip() == symbol + ":")
    out = []
    for line in lines[start + 1:]:
        if line.strip().startswith((".Lfunc_end", ".section", ".rodata")):
            break  # (the kernel descriptor that follows holds the kernarg size: not instructions)
        line = line.split(";")[0].rstrip()
        if not line or line.lstrip().startswith((".loc", ".file", ".cfi")):
            continue
        out.append(re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", ".L", line.replace(symbol, "SYM")))
    return out


def main(argv):
    before, after, pairs = argv[1], argv[2], argv[3:]
    bad = 0
    for pair in pairs:
        old, new = pair.split("=")
        a, b = body(before, old), body(after, new)
        same = a == b
        print(f"{old} -> {new}: {len(a)} / {len(b)} lines, {'identical' if same else 'DIFFERENT'}")
        bad += 0 if same else 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
