"""The kernels every summary launcher builds for the double Lynden-Bell models (7 and 8), compiled for gfx950 by the
resource tools of tools/, held to the rules the older tests hold models 0 .. 6 to: no scratch, no spills, at most 128
VGPRs, no LDS where the family uses none, sample constants through the scalar cache.  (The tools report models 0 .. 6
unless asked: analyse(models=DOUBLE_MODELS).)"""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


def doubles(module, *args):
    rows = module.analyse(*args, models=module.DOUBLE_MODELS)
    mine = [r for r in rows if "model_id" in r]
    assert mine and all(r["model_id"] in (7, 8) and r["model"].startswith("DOUBLE") for r in mine)
    base = module.analyse.__defaults__                       # the default stays the seven original models
    assert base[-1] is None and module.BASE_MODELS == tuple(range(7)) and module.ALL_MODELS == tuple(range(9))
    return mine


def test_holdout_kernels():
    import holdout_resources
    rows = doubles(holdout_resources)
    assert len(rows) == 2 * 2                                # two models x two centre modes
    for r in rows:
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
        assert r["lds_bytes"] == 0 and r["vgprs"] <= 128, r


def test_replicate_kernels():
    import replicate_resources
    rows = doubles(replicate_resources)
    assert len(rows) == 2 * 2
    for r in rows:
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
        assert r["lds_bytes"] == 0, r


def test_predictive_kernels(tmp_path):
    import predictive_resources
    rows = doubles(predictive_resources, str(tmp_path))
    assert len(rows) == 2 * (2 * 2 + 1 * 2)                  # two precisions x (two models x two centres + MIX for model 8)
    for r in rows:
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0, r
        assert r["lds_bytes"] == 0 and r["vgprs"] <= 128, r


def test_loo_expectation_kernels(tmp_path):
    import loo_expect_resources
    rows = doubles(loo_expect_resources, str(tmp_path))
    assert len(rows) == 2 * (2 * 2 * 2 + 1 * 2)              # ... x {lnL only, predictive rows} + pit_mix for model 8
    for r in rows:
        assert r["scratch_bytes_per_lane"] == 0, r
        assert r["vgpr_spill"] == 0 and r["agprs"] == 0, r
        assert r["vgprs"] <= 128, r


def test_posterior_kernels(tmp_path):
    import posterior_isa
    rows = doubles(posterior_isa, str(tmp_path))
    assert len(rows) == 2 * 2 * (1 + 1 * 2)                  # two precisions x two centres x (model 7 + model 8 with / without membership)
    for r in rows:
        assert r["s_load_in_loop"] >= 1, r
        assert r["vector_loads_in_loop"] == 0, r
        assert r["scratch_in_loop"] == 0, r
