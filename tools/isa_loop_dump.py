#!/usr/bin/env python3
"""Print the hot loop of one fast-path instantiation of mcd::loglike_kernel as gfx950 assembly, for annotation.

    python tools/isa_loop_dump.py ISA.s "BGFIXED fixed, narrow" [--prefetch]
    python tools/isa_loop_dump.py ISA.s "BGFIXED fixed, narrow, prefetch, bounded"

ISA.s is the device assembly of csrc/mcd_kernels.hip (hipcc -save-temps; tools/isa_mix.py leaves it in /tmp/isa_mix).
The loop is located with tools/isa_mix.py's rules; for the narrow-range variants the rescale block behind the loop's
closing branch is printed after it.  A tally of the vector instructions by opcode closes the listing.
"""
import os
import re
import sys
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_mix  # noqa: E402


def loop_lines(asm, name, prefetch):
    bounded = name == isa_mix.BOUNDED[1]
    if bounded:
        tag, trips, selector = isa_mix.BOUNDED[0], isa_mix.BOUNDED[4], isa_mix.BOUNDED[5]
    else:
        for row in isa_mix.KERNELS:
            if row[1] == name:
                tag, trips, selector = row[0], row[4], row[5]
                if prefetch and len(row) > 6:
                    trips, selector = row[6][1], row[6][2]
                break
        else:
            raise SystemExit("unknown kernel %r" % name)
        tag = tag + ("Lb1ELi4ELb0EE" if prefetch else "Lb0ELi4ELb0EE")
    a = next(i for i, l in enumerate(asm) if l.startswith("_ZN3mcd12_GLOBAL__N_114loglike_kernel" + tag))
    e = next(i for i in range(a, len(asm)) if asm[i].startswith(".Lfunc_end"))
    k = asm[a:e]
    labels = {l.split(":")[0]: i for i, l in enumerate(k) if re.match(r"^\.LBB\d+_\d+:", l)}
    spans = []
    for i, l in enumerate(k):
        m = re.search(r"s_cbranch_\w+ (\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            spans.append((labels[m.group(1)], i))
    inner = [sp for sp in spans if not any(o != sp and sp[0] <= o[0] and o[1] <= sp[1] for o in spans)]
    ranked = sorted(inner, key=lambda sp: sp[1] - sp[0], reverse=True)
    hits = [sp for sp in ranked if selector is None or selector(Counter(isa_mix._ops(k[sp[0]:sp[1]])))]
    best = (hits or ranked)[0]
    body = k[best[0]:best[1] + 1]
    blk = isa_mix.rescale_block(k, labels, best, bounded, trips)
    extra = k[blk[0]:blk[1] + 1] if blk else []
    return body, extra


def main():
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    asm = open(sys.argv[1]).read().split("\n")
    body, extra = loop_lines(asm, sys.argv[2], "--prefetch" in sys.argv[3:])
    code = lambda ls: [l for l in ls if l.startswith("\t") and not l.strip().startswith((";", "."))]
    for l in code(body):
        print(l.strip())
    if extra:
        print("; ---- rescale block (every %s iteration)" % ("fourth (R = 32)" if sys.argv[2] == isa_mix.BOUNDED[1] else "second"))
        for l in code(extra):
            print(l.strip())
    tally = Counter(isa_mix._ops(code(body)))
    print("; ---- loop body VALU by opcode:", ", ".join("%s %d" % kv for kv in sorted(tally.items()) if kv[0].startswith("v_")))


if __name__ == "__main__":
    main()
