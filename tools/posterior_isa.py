#!/usr/bin/env python3
"""Instruction mix of the sample loop of mcd::posterior_slice_kernel (csrc/mcd_posterior.hip), from the gfx950 ISA hipcc
emits, counted the way tools/isa_mix.py counts the main kernel's loops.

    python tools/posterior_isa.py              # compiles csrc/mcd_posterior.hip with -save-temps into a temporary
                                               # directory, prints one line per instantiation
    python tools/posterior_isa.py --json OUT   # also writes the table as JSON (tools/posterior_probe.py reads the rows)

One iteration of the loop is one (star, sample) term per lane.  For every instantiation the row gives the VALU
instructions per term, how many of them are f64 arithmetic, the scalar loads inside the loop (the sample's derived
constants: wave-uniform, through the scalar cache) and the vector loads inside the loop (must be none: the star record
is loaded once, before the loop).
"""
import json
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
MODELS = {0: "CONST", 1: "BGFIXED", 2: "BGGAUSS", 3: "PROFILE", 4: "PROFILE_BGGAUSS", 5: "PROFILE_BGDENS",
          6: "PROFILE_BGFIXED", 7: "DOUBLE", 8: "DOUBLE_BGGAUSS", 10: "CONST_ESCALE", 11: "PROFILE_ESCALE"}
# analyse() reports the seven models of the reference's running classes unless told otherwise (the tests that quote
# its table count them); the double Lynden-Bell models: analyse(models=DOUBLE_MODELS), tests/test_double_resources_cpu.py
BASE_MODELS, DOUBLE_MODELS, ALL_MODELS = tuple(range(7)), (7, 8), tuple(range(9))
ESCALE_MODELS = (10, 11)      # the error-scale models: analyse(models=ESCALE_MODELS), `--escale` on the command line
# _ZN3mcd12_GLOBAL__N_122posterior_slice_kernelILi<model>ELb<free>ELb<mem>E<d|f>EEvPKT2_...
_NAME = re.compile(r"^(_ZN3mcd12_GLOBAL__N_122posterior_slice_kernelILi(\d+)ELb(\d)ELb(\d)E([df])E\w*):")


def _ops(lines):
    return [l.split()[0] for l in lines if l.startswith("\t") and not l.strip().startswith((";", "."))]


def compile_isa(out):
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c",
                    os.path.join(CSRC, "mcd_posterior.hip"), "-o", os.path.join(out, "p.o"), "-save-temps=obj"],
                   check=True, capture_output=True)
    return os.path.join(out, "mcd_posterior-hip-amdgcn-amd-amdhsa-gfx950.s")


def analyse(out=None, models=None):
    """Rows (dicts) per slice-kernel instantiation; `out`: directory for the compiler's temporaries (default: a fresh
    temporary directory)."""
    if out is None:
        out = tempfile.mkdtemp(prefix="posterior_isa_")
    asm = open(compile_isa(out)).read().split("\n")
    rows = []
    for a, line in enumerate(asm):
        m = _NAME.match(line)
        if not m:
            continue
        e = next(i for i in range(a, len(asm)) if asm[i].startswith(".Lfunc_end"))
        k = asm[a:e]
        labels = {l.split(":")[0]: i for i, l in enumerate(k) if re.match(r"^\.LBB\d+_\d+:", l)}
        spans = []
        for i, l in enumerate(k):
            b = re.search(r"s_cbranch_\w+ (\.LBB\d+_\d+)", l)
            if b and b.group(1) in labels and labels[b.group(1)] < i:
                spans.append((labels[b.group(1)], i))
        # the sample loop: the longest backward-branch span (the only loop of the kernel unless the compiler unrolls)
        lo, hi = max(spans, key=lambda sp: sp[1] - sp[0])
        body = Counter(_ops(k[lo:hi + 1]))
        # one trip = one term: the compiler does not unroll a loop of a few hundred instructions with a run-time trip count
        valu = sum(v for o, v in body.items() if o.startswith("v_"))
        f64 = sum(v for o, v in body.items() if o.startswith("v_") and "f64" in o and not o.startswith(("v_ldexp", "v_frexp")))
        rows.append({"kernel": m.group(1), "model": MODELS[int(m.group(2))], "model_id": int(m.group(2)), "free_centre": m.group(3) == "1",
                     "membership": m.group(4) == "1", "precision": "f64" if m.group(5) == "d" else "f32",
                     "loop_lines": hi - lo, "valu_per_term": valu, "f64_per_term": f64,
                     "s_load_in_loop": sum(v for o, v in body.items() if o.startswith("s_load")),
                     "vector_loads_in_loop": sum(v for o, v in body.items() if o.startswith(("global_load", "flat_load", "buffer_load"))),
                     "scratch_in_loop": sum(v for o, v in body.items() if o.startswith("scratch_"))})
    return [r for r in rows if "model_id" not in r or r["model_id"] in (BASE_MODELS if models is None else models)]


def main():
    escale = "--escale" in sys.argv
    sys.argv = [a for a in sys.argv if a != "--escale"]
    rows = analyse(models=ESCALE_MODELS if escale else ALL_MODELS)
    print("{0:16s} {1:5s} {2:4s} {3:4s} {4:>10s} {5:>8s} {6:>7s} {7:>7s}".format("model", "free", "mem", "prec", "VALU/term",
                                                                               "f64", "s_load", "vload"))
    for r in sorted(rows, key=lambda r: (r["precision"], r["model"], r["free_centre"], r["membership"])):
        print("{0:16s} {1:5s} {2:4s} {3:4s} {4:10d} {5:8d} {6:7d} {7:7d}".format(
            r["model"], str(r["free_centre"]), str(r["membership"]), r["precision"], r["valu_per_term"], r["f64_per_term"],
            r["s_load_in_loop"], r["vector_loads_in_loop"]))
    if len(sys.argv) == 3 and sys.argv[1] == "--json":
        with open(sys.argv[2], "w") as f:
            json.dump({"generated_by": "tools/posterior_isa.py", "rows": rows}, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    sys.exit(main())
