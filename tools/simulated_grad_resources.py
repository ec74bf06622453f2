#!/usr/bin/env python3
"""Register, scratch and LDS use of the kernel of csrc/mcd_simulated_grad.hip, from hipcc's resource-usage remarks for
gfx950 (the sibling of tools/simulated_resources.py, whose parsing it shares).

    python tools/simulated_grad_resources.py              # one line per instantiation
    python tools/simulated_grad_resources.py --json OUT   # also writes the rows as JSON (profiles/simulated_grad_resources.json)

DESIGN.md section 3.23 quotes the table; tests/test_simulated_grad_cpu.py asserts that no instantiation uses scratch memory
or LDS.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from weighted_resources import ALL_MODELS, CSRC, ESCALE_MODELS, KEYS, MODELS, _FIELD  # noqa: E402

_MAIN = re.compile(r"(simulated_grad)_kernelILi(\d+)ELb(\d)EE")


def analyse(models=None):
    """Rows (dicts) per kernel instantiation of the unit: 9 models x {fixed, free centre}."""
    out = tempfile.mkdtemp(prefix="simulated_grad_resources_")
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "mcd_simulated_grad.hip"),
                          "-o", os.path.join(out, "mcd_simulated_grad.o")], check=True, capture_output=True, text=True)
    rows, row = [], None
    for line in res.stderr.split("\n"):
        if "remark: Function Name:" in line:
            name = line.split("Function Name:")[1].split()[0]
            m = _MAIN.search(name)
            row = None
            if m:
                row = {"kernel": m.group(1), "model": MODELS[int(m.group(2))], "model_id": int(m.group(2)),
                       "free_centre": m.group(3) == "1", "symbol": name}
                rows.append(row)
            continue
        f = _FIELD.search(line)
        if f and row is not None and f.group(1).strip() in KEYS and f.group(2).isdigit():
            row[KEYS[f.group(1).strip()]] = int(f.group(2))
    rows.sort(key=lambda r: (r["kernel"], r["model_id"], r["free_centre"]))
    return [r for r in rows if r["model_id"] in (ALL_MODELS if models is None else models)]


def main():
    escale = "--escale" in sys.argv
    sys.argv = [a for a in sys.argv if a != "--escale"]
    rows = analyse(models=ESCALE_MODELS if escale else ALL_MODELS)
    print("{0:16s} {1:16s} {2:6s} {3:>6s} {4:>6s} {5:>8s} {6:>5s} {7:>10s}".format(
        "kernel", "model", "centre", "VGPRs", "SGPRs", "scratch", "LDS", "waves/SIMD"))
    for r in rows:
        print("{0:16s} {1:16s} {2:6s} {3:6d} {4:6d} {5:8d} {6:5d} {7:10d}".format(
            r["kernel"], r["model"], "free" if r["free_centre"] else "fixed", r["vgprs"], r["sgprs"],
            r["scratch_bytes_per_lane"], r["lds_bytes"], r["occupancy"]))
    if len(sys.argv) == 3 and sys.argv[1] == "--json":
        with open(sys.argv[2], "w") as fh:
            json.dump({"generated_by": "tools/simulated_grad_resources.py", "rows": rows}, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    sys.exit(main())
