#!/usr/bin/env python3
"""Register and scratch use of the kernels of csrc/mcd_replicate.hip, from hipcc's resource-usage remarks for gfx950 (the
sibling of tools/holdout_resources.py).

    python tools/replicate_resources.py              # one line per instantiation
    python tools/replicate_resources.py --json OUT   # also writes the rows as JSON (profiles/replicate_resources.json)

DESIGN.md section 3.18 quotes the table; tests/test_replicate_cpu.py asserts that no instantiation uses scratch or spills.
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
_MAIN = re.compile(r"replicate_kernelILi(\d+)ELb(\d)EE")
_FIELD = re.compile(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\w+) \[-Rpass")
KEYS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize": "scratch_bytes_per_lane",
        "Occupancy": "occupancy", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill", "LDS Size": "lds_bytes"}


def analyse(models=None):
    """Rows (dicts) per kernel instantiation of the unit."""
    out = tempfile.mkdtemp(prefix="replicate_resources_")
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "mcd_replicate.hip"),
                          "-o", os.path.join(out, "mcd_replicate.o")], check=True, capture_output=True, text=True)
    rows, row = [], None
    for line in res.stderr.split("\n"):
        if "remark: Function Name:" in line:
            name = line.split("Function Name:")[1].split()[0]
            m = _MAIN.search(name)
            if m:
                row = {"kernel": "replicate", "model": MODELS[int(m.group(1))], "model_id": int(m.group(1)), "free_centre": m.group(2) == "1"}
            else:
                row = {"kernel": "reduce" if "replicate_reduce_kernel" in name else name}
            row["symbol"] = name
            rows.append(row)
            continue
        f = _FIELD.search(line)
        if f and row is not None and f.group(1).strip() in KEYS and f.group(2).isdigit():
            row[KEYS[f.group(1).strip()]] = int(f.group(2))
    return [r for r in rows if "model_id" not in r or r["model_id"] in (BASE_MODELS if models is None else models)]


def markdown(rows):
    """The table of DESIGN.md section 3.18."""
    lines = ["| kernel | model | centre | VGPRs | SGPRs | scratch [B/lane] | spills (V / S) | LDS [B] | waves / SIMD |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in sorted(rows, key=lambda r: (r["kernel"] != "replicate", r.get("model", ""), r.get("free_centre", False))):
        lines.append("| `{0}` | {1} | {2} | {3} | {4} | {5} | {6} / {7} | {8} | {9} |".format(
            r["kernel"], "`%s`" % r["model"] if "model" in r else "-",
            ("free" if r["free_centre"] else "fixed") if "free_centre" in r else "-", r["vgprs"], r["sgprs"],
            r["scratch_bytes_per_lane"], r["vgpr_spill"], r["sgpr_spill"], r["lds_bytes"], r["occupancy"]))
    return "\n".join(lines)


def main():
    escale = "--escale" in sys.argv
    sys.argv = [a for a in sys.argv if a != "--escale"]
    rows = analyse(models=ESCALE_MODELS if escale else ALL_MODELS)
    print(markdown(rows))
    if len(sys.argv) == 3 and sys.argv[1] == "--json":
        with open(sys.argv[2], "w") as fh:
            json.dump({"generated_by": "tools/replicate_resources.py", "rows": rows}, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    sys.exit(main())
