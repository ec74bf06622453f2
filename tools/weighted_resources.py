#!/usr/bin/env python3
"""Register and scratch use of the kernels of csrc/mcd_weighted.hip, from hipcc's resource-usage remarks for gfx950 (the
sibling of tools/holdout_resources.py).

    python tools/weighted_resources.py              # one line per instantiation
    python tools/weighted_resources.py --json OUT   # also writes the rows as JSON (profiles/weighted_resources.json)

DESIGN.md section 3.20 quotes the table; tests/test_bootstrap_cpu.py asserts that no instantiation uses scratch memory
or LDS.
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
ALL_MODELS, ESCALE_MODELS = tuple(range(9)), (10, 11)      # analyse() reports the first nine unless told otherwise
SCHEMES = {0: "exponential", 1: "poisson", 2: "explicit"}
_MAIN = re.compile(r"weighted_grad_kernelILi(\d+)ELb(\d)ELi(\d)EE")
_FIELD = re.compile(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\w+) \[-Rpass")
KEYS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize": "scratch_bytes_per_lane",
        "Occupancy": "occupancy", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill", "LDS Size": "lds_bytes"}


def analyse(models=None):
    """Rows (dicts) per kernel instantiation of the unit: 9 models x {fixed, free centre} x 3 schemes."""
    out = tempfile.mkdtemp(prefix="weighted_resources_")
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "mcd_weighted.hip"),
                          "-o", os.path.join(out, "mcd_weighted.o")], check=True, capture_output=True, text=True)
    rows, row = [], None
    for line in res.stderr.split("\n"):
        if "remark: Function Name:" in line:
            name = line.split("Function Name:")[1].split()[0]
            m = _MAIN.search(name)
            row = None
            if m:
                row = {"kernel": "weighted_grad", "model": MODELS[int(m.group(1))], "model_id": int(m.group(1)),
                       "free_centre": m.group(2) == "1", "scheme": SCHEMES[int(m.group(3))], "symbol": name}
                rows.append(row)
            continue
        f = _FIELD.search(line)
        if f and row is not None and f.group(1).strip() in KEYS and f.group(2).isdigit():
            row[KEYS[f.group(1).strip()]] = int(f.group(2))
    rows.sort(key=lambda r: (r["model_id"], r["free_centre"], r["scheme"]))
    return [r for r in rows if r["model_id"] in (ALL_MODELS if models is None else models)]


def main():
    escale = "--escale" in sys.argv
    sys.argv = [a for a in sys.argv if a != "--escale"]
    rows = analyse(models=ESCALE_MODELS if escale else ALL_MODELS)
    print("{0:16s} {1:6s} {2:12s} {3:>6s} {4:>6s} {5:>8s} {6:>5s} {7:>10s}".format("model", "centre", "scheme", "VGPRs", "SGPRs",
                                                                                "scratch", "LDS", "waves/SIMD"))
    for r in rows:
        print("{0:16s} {1:6s} {2:12s} {3:6d} {4:6d} {5:8d} {6:5d} {7:10d}".format(
            r["model"], "free" if r["free_centre"] else "fixed", r["scheme"], r["vgprs"], r["sgprs"],
            r["scratch_bytes_per_lane"], r["lds_bytes"], r["occupancy"]))
    if len(sys.argv) == 3 and sys.argv[1] == "--json":
        with open(sys.argv[2], "w") as fh:
            json.dump({"generated_by": "tools/weighted_resources.py", "rows": rows}, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    sys.exit(main())
