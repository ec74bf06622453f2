"""Static check of the gfx950 code of the double Lynden-Bell kernels (cross-compiled by tools/isa_mix.py, no GPU needed).

The second component rides on PROFILE's loop: per term two more instructions for its cross product, one sum (m_2 = rho_2^2 +
r^2), the product m_1 m_2 and three more multiply-adds for the common numerator -- seven f64 instructions, and NO second
reciprocal sequence (DESIGN 3.19 has the listing).  MARGIN is that measured difference, 7.0 (already a multiple of 0.5);
the same margin holds between the two Gaussian-background loops, whose cluster part is the same code."""
import os
import re
import sys

import pytest

from conftest import ROOT

MARGIN = 7.0


@pytest.fixture(scope="module")
def isa_build(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_mix
    out = str(tmp_path_factory.mktemp("isa_mix_double"))
    rows = isa_mix.analyse(out)
    return {r["name"]: r for r in rows}, os.path.join(out, "mcd_kernels-hip-amdgcn-amd-amdhsa-gfx950.s")


@pytest.mark.parametrize("double, single", [("DOUBLE fixed centre", "PROFILE fixed centre"),
                                            ("DOUBLE_BGGAUSS fixed", "PROFILE_BGGAUSS fixed"),
                                            ("DOUBLE fixed centre, prefetch", "PROFILE fixed centre, prefetch")])
def test_second_component_costs_seven_instructions_and_no_reciprocal(isa_build, double, single):
    table = isa_build[0]
    assert double in table and single in table, sorted(table)
    d, s = table[double], table[single]
    assert d["stars_per_iteration"] == s["stars_per_iteration"]
    assert d["valu_per_term"] <= s["valu_per_term"] + MARGIN, (d["valu_per_term"], s["valu_per_term"])
    assert d["trans_f64_per_term"] == s["trans_f64_per_term"]          # v_rcp_f64 / v_rsq_f64: one reciprocal, shared
    assert d["other_per_term"] <= s["other_per_term"]                  # nothing but f64 arithmetic was added


def test_double_kernels_use_scalar_record_loads_and_no_scratch(isa_build):
    asm = open(isa_build[1]).read()
    # models 7 and 8, fixed and free centre, plain (FAST 0) and fast (FAST 1), without and with the prefetch, 4 waves
    tags = ["ILi{0}ELb{1}EddLi{2}ELb{3}ELi4E".format(m, f, fast, pf) for m in (7, 8) for f in (0, 1)
            for fast, pf in ((0, 0), (1, 0), (1, 1))]
    tags += ["ILi7ELb0EddLi1ELb0ELi8E", "ILi7ELb0EddLi1ELb0ELi16E", "ILi8ELb0EddLi1ELb0ELi8E"]      # the combining workgroups
    for tag in tags:
        m = re.search(r"\n(_ZN3mcd12_GLOBAL__N_114loglike_kernel" + tag + r"[^\n:]*):[^\n]*\n(.*?)\n\.Lfunc_end", asm, re.S)
        assert m, tag
        body = m.group(2)
        assert "s_load_dwordx" in body                       # star records arrive through the scalar cache
        meta = re.search(r"\.amdhsa_kernel " + re.escape(m.group(1)) + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S).group(1)
        # the 8-wave Gaussian-background kernels are held to 128 registers by their launch bound and spill a few dwords
        # outside the loop, as MODEL_BGGAUSS's does (tests/test_isa_budget.py: 32 bytes)
        limit = 32 if tag == "ILi8ELb0EddLi1ELb0ELi8E" else 0
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) <= limit, tag
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1)) <= 128, tag


def test_no_float32_or_level_two_instantiation_was_built(isa_build):
    """float32 catalogues are refused at creation and level_verdict never returns 2 for the double models: the main kernel
    has no such instantiations to build."""
    asm = open(isa_build[1]).read()
    for m in (7, 8):
        for f in (0, 1):
            assert "loglike_kernelILi{0}ELb{1}EddLi2E".format(m, f) not in asm
            assert "loglike_kernelILi{0}ELb{1}Ef".format(m, f) not in asm
            assert "loglike_kernelILi{0}ELb{1}EddLi1E".format(m, f) in asm
