#!/usr/bin/env python3
"""Register and scratch use of the kernels of csrc/mcd_weighted_value.hip, from hipcc's resource-usage remarks for gfx950
(the sibling of tools/weighted_resources.py, whose parsing it shares).

    python tools/weighted_value_resources.py              # one line per instantiation, with the gradient kernel's VGPRs
    python tools/weighted_value_resources.py --json OUT   # also writes the rows as JSON (profiles/weighted_value_resources.json)

DESIGN.md section 3.21 quotes the table beside section 3.20's; tests/test_weighted_value_cpu.py asserts that no
instantiation uses scratch memory or LDS.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from weighted_resources import ALL_MODELS, CSRC, ESCALE_MODELS, KEYS, MODELS, ROOT, SCHEMES, _FIELD  # noqa: E402

_MAIN = re.compile(r"weighted_value_kernelILi(\d+)ELb(\d)ELi(\d)EE")


def analyse(models=None):
    """Rows (dicts) per kernel instantiation of the unit: 9 models x {fixed, free centre} x 3 schemes."""
    out = tempfile.mkdtemp(prefix="weighted_value_resources_")
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "mcd_weighted_value.hip"),
                          "-o", os.path.join(out, "mcd_weighted_value.o")], check=True, capture_output=True, text=True)
    rows, row = [], None
    for line in res.stderr.split("\n"):
        if "remark: Function Name:" in line:
            name = line.split("Function Name:")[1].split()[0]
            m = _MAIN.search(name)
            row = None
            if m:
                row = {"kernel": "weighted_value", "model": MODELS[int(m.group(1))], "model_id": int(m.group(1)),
                       "free_centre": m.group(2) == "1", "scheme": SCHEMES[int(m.group(3))], "symbol": name}
                rows.append(row)
            continue
        f = _FIELD.search(line)
        if f and row is not None and f.group(1).strip() in KEYS and f.group(2).isdigit():
            row[KEYS[f.group(1).strip()]] = int(f.group(2))
    rows.sort(key=lambda r: (r["model_id"], r["free_centre"], r["scheme"]))
    return [r for r in rows if r["model_id"] in (ALL_MODELS if models is None else models)]


def gradient_vgprs():
    """{(model_id, free_centre, scheme): VGPRs} of the gradient kernels, from the committed profiles/weighted_resources.json."""
    with open(os.path.join(ROOT, "profiles", "weighted_resources.json")) as fh:
        return {(r["model_id"], r["free_centre"], r["scheme"]): r["vgprs"] for r in json.load(fh)["rows"]}


def main():
    escale = "--escale" in sys.argv
    sys.argv = [a for a in sys.argv if a != "--escale"]
    rows = analyse(models=ESCALE_MODELS if escale else ALL_MODELS)
    grad = gradient_vgprs()
    print("{0:16s} {1:6s} {2:12s} {3:>6s} {4:>6s} {5:>8s} {6:>5s} {7:>10s} {8:>10s}".format(
        "model", "centre", "scheme", "VGPRs", "SGPRs", "scratch", "LDS", "waves/SIMD", "grad VGPRs"))
    for r in rows:
        g = grad.get((r["model_id"], r["free_centre"], r["scheme"]), 0)         # (0: not in the committed gradient table)
        print("{0:16s} {1:6s} {2:12s} {3:6d} {4:6d} {5:8d} {6:5d} {7:10d} {8:10d}{9}".format(
            r["model"], "free" if r["free_centre"] else "fixed", r["scheme"], r["vgprs"], r["sgprs"],
            r["scratch_bytes_per_lane"], r["lds_bytes"], r["occupancy"], g, "  MORE than the gradient" if r["vgprs"] > g else ""))
    if len(sys.argv) == 3 and sys.argv[1] == "--json":
        with open(sys.argv[2], "w") as fh:
            json.dump({"generated_by": "tools/weighted_value_resources.py", "rows": rows}, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    sys.exit(main())
