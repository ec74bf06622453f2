"""Static check of the bounded narrow-range BGFIXED loop (the instantiation C3's timed launches run): its VALU count per
term, no exponent clamp in the loop, and the 8-waves-per-SIMD register budget without scratch (cross-compiled)."""
import os
import re
import sys

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_mix
    out = str(tmp_path_factory.mktemp("isa_bounded"))
    rows = isa_mix.analyse(out)
    return isa_mix, rows, os.path.join(out, "mcd_kernels-hip-amdgcn-amd-amdhsa-gfx950.s")


def test_bounded_loop_instruction_count(isa):
    isa_mix, rows, _ = isa
    table = {r["name"]: r for r in rows}
    bounded = table[isa_mix.BOUNDED[1]]
    assert bounded["valu_per_term"] <= 22.5, bounded
    # the f64 work is the level-2 loop's; only integer / move instructions went
    level2 = table["BGFIXED fixed, narrow, prefetch"]
    assert bounded["f64_per_term"] == level2["f64_per_term"]
    assert bounded["other_per_term"] < level2["other_per_term"] - 1.0


def test_bounded_loop_has_no_exponent_clamp(isa):
    isa_mix, _, path = isa
    import isa_loop_dump
    asm = open(path).read().split("\n")
    body, extra = isa_loop_dump.loop_lines(asm, isa_mix.BOUNDED[1], True)
    def ops(lines):
        return [l.split()[0] for l in lines if l.startswith("\t") and not l.strip().startswith((";", "."))]
    assert ops(body).count("v_rsq_f64_e32") == 8 and "v_frexp_mant_f64_e32" not in ops(body)
    assert "v_frexp_mant_f64_e32" in ops(extra)            # the rescale sits in its own block, once per R terms
    assert not any(o.startswith("v_max_i32") for o in ops(body + extra))


def test_bounded_kernels_registers_and_scratch(isa):
    _, _, path = isa
    asm = open(path).read()
    names = re.findall(r"\.amdhsa_kernel (_ZN3mcd12_GLOBAL__N_114loglike_kernelILi1ELb0EddLi2ELb1ELi(?:4|8|16)ELb1EE\S*)", asm)
    assert len(names) == 3, names
    for name in names:
        meta = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S).group(1)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1)) <= 64
