#!/usr/bin/env python3
"""Register and scratch use of the kernels of csrc/mcd_loo_expect.hip, from hipcc's resource-usage remarks for gfx950
(the sibling of tools/predictive_resources.py).

    python tools/loo_expect_resources.py              # one line per instantiation, then the table per family
    python tools/loo_expect_resources.py --json OUT   # also writes the rows as JSON

Compiles the device side of the unit with -Rpass-analysis=kernel-resource-usage and reads the remarks: VGPRs, SGPRs,
scratch bytes per lane, spills, LDS and occupancy of every loox_term_kernel<MODEL, FREE, MODE, T> (MODE: 0 lnL only, 1 the
four predictive rows, 2 those and pit_mix) and loox_tail_kernel<XR> (DESIGN.md section 3.15 quotes the table;
tests/test_loo_expect_cpu.py asserts section 3.12's rule: no scratch, no spill, at most 128 VGPRs).
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
MODELS = {0: "CONST", 1: "BGFIXED", 2: "BGGAUSS", 3: "PROFILE", 4: "PROFILE_BGGAUSS", 5: "PROFILE_BGDENS",
          6: "PROFILE_BGFIXED", 7: "DOUBLE", 8: "DOUBLE_BGGAUSS", 10: "CONST_ESCALE", 11: "PROFILE_ESCALE"}
# analyse() reports the seven models of the reference's running classes unless told otherwise (the tests that quote
# its table count them); the double Lynden-Bell models: analyse(models=DOUBLE_MODELS), tests/test_double_resources_cpu.py
BASE_MODELS, DOUBLE_MODELS, ALL_MODELS = tuple(range(7)), (7, 8), tuple(range(9))
ESCALE_MODELS = (10, 11)      # the error-scale models: analyse(models=ESCALE_MODELS), `--escale` on the command line
_TERM = re.compile(r"loox_term_kernelILi(\d+)ELb(\d)ELi(\d)E([df])E")
_TAIL = re.compile(r"loox_tail_kernelILi(\d)EE")
_FIELD = re.compile(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\w+) \[-Rpass")
KEYS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize": "scratch_bytes_per_lane",
        "Occupancy": "occupancy", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill", "LDS Size": "lds_bytes"}


def remarks(out=None):
    if out is None:
        out = tempfile.mkdtemp(prefix="loo_expect_resources_")
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "mcd_loo_expect.hip"),
                          "-o", os.path.join(out, "mcd_loo_expect.o")], check=True, capture_output=True, text=True)
    return res.stderr


def analyse(out=None, models=None):
    """Rows (dicts) per kernel instantiation of the unit."""
    rows, row = [], None
    for line in remarks(out).split("\n"):
        if "remark: Function Name:" in line:
            name = line.split("Function Name:")[1].split()[0]
            s, m = _TERM.search(name), _TAIL.search(name)
            if s:
                row = {"kernel": "term", "model": MODELS[int(s.group(1))], "model_id": int(s.group(1)), "free_centre": s.group(2) == "1",
                       "mode": int(s.group(3)), "precision": "f64" if s.group(4) == "d" else "f32"}
            elif m:
                row = {"kernel": "tail", "extra_rows": int(m.group(1))}
            else:
                row = {"kernel": name}
            row["symbol"] = name
            rows.append(row)
            continue
        f = _FIELD.search(line)
        if f and row is not None and f.group(1).strip() in KEYS and f.group(2).isdigit():
            row[KEYS[f.group(1).strip()]] = int(f.group(2))
    return [r for r in rows if "model_id" not in r or r["model_id"] in (BASE_MODELS if models is None else models)]


def families(rows):
    """(family, precision) -> largest VGPRs / SGPRs / scratch over its instantiations.  Families: the cluster part
    (CONST / PROFILE) x centre mode x MODE for the term kernels, and the three tail kernels."""
    fam = {}
    for r in rows:
        if r["kernel"] == "term":
            key = ("{0} {1} mode {2}".format("PROFILE" if r["model"].startswith("PROFILE") else "CONST",
                                             "free" if r["free_centre"] else "fixed", r["mode"]), r["precision"])
        elif r["kernel"] == "tail":
            key = ("tail +{0} rows".format(r["extra_rows"]), "f64")
        else:
            continue
        f = fam.setdefault(key, {"vgprs": 0, "sgprs": 0, "scratch_bytes_per_lane": 0, "occupancy": 99, "count": 0})
        for k in ("vgprs", "sgprs", "scratch_bytes_per_lane"):
            f[k] = max(f[k], r[k])
        f["occupancy"] = min(f["occupancy"], r["occupancy"])
        f["count"] += 1
    return fam


def main():
    escale = "--escale" in sys.argv
    sys.argv = [a for a in sys.argv if a != "--escale"]
    rows = analyse(models=ESCALE_MODELS if escale else ALL_MODELS)
    for r in rows:
        print(r)
    print("{0:22s} {1:4s} {2:>3s} {3:>6s} {4:>6s} {5:>8s} {6:>10s}".format("family", "prec", "n", "VGPRs", "SGPRs", "scratch",
                                                                         "waves/SIMD"))
    for (name, prec), f in sorted(families(rows).items()):
        print("{0:22s} {1:4s} {2:3d} {3:6d} {4:6d} {5:8d} {6:10d}".format(name, prec, f["count"], f["vgprs"], f["sgprs"],
                                                                         f["scratch_bytes_per_lane"], f["occupancy"]))
    if len(sys.argv) == 3 and sys.argv[1] == "--json":
        with open(sys.argv[2], "w") as fh:
            json.dump({"generated_by": "tools/loo_expect_resources.py", "rows": rows}, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    sys.exit(main())
