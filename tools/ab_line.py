#!/usr/bin/env python3
"""One summary line of a bench.py result file (tools/ab_bench.sh style A/B runs):  python tools/ab_line.py NAME FILE"""
import json
import sys

d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
roof = d.get("roofline") or {}
one = roof.get("kernel_us_one_lane")
print("{0:24s} step {1:8.2f} us   kernel {2:8.2f} us   one lane {3}".format(
    sys.argv[1], d["ms_per_step"] * 1e3, roof.get("kernel_us", float("nan")), "{0:.2f} us".format(one) if one else "-"))
