"""CPU: the per-term tolerance of the float32 per-star terms and per-star posterior summaries (tests/f32_term_helper.py;
DESIGN.md section 5), for all 7 models x fixed / free centre, at the shapes tests/test_gpu_f32_terms.py runs on the device.

  * every cell is inside the float32 accuracy domain (csrc/mcd_guard.h: f32_domain), nothing skipped;
  * the NumPy float32 restatement of the term is within (C/2) u A of the longdouble oracle: this pins the measurement C
    comes from (the F32_TERM_NP32 lines);
  * the host build of the same templates (tests/emul/f32_emul.cpp: star_components<float>, mixture_lnl<float>, both modes of
    per_star_kernel; posterior_term<float> through PostAcc) is within C u A per term and per summary field (the
    F32_TERM_HOST_ACCURACY lines);
  * the bound bites: each planted defect exceeds it in every cell it touches;
  * outside the domain (un-moved variant_helper.make_case) the ratio is reported, not asserted."""
import numpy as np
import pytest

import emul_helper as emul
import f32_helper as fh
import f32_term_helper as th
import posterior_helper as ph
import predictive_helper as pr
import variant_helper as vh

pytestmark = pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="no extended-precision long double on this platform")

ALL_N = sorted(set(th.PER_STAR_N) | set(th.POST_N) | set(th.PRED_N))
S_MAX = max(th.POST_S)


def rows_of(n):
    """All 257 sample rows at the posterior shapes, three rows where only the per-star kernel runs."""
    return list(range(S_MAX)) if n <= max(th.POST_N) else list(th.PER_STAR_ROWS)


def name(model, free):
    return "model {0} {1}".format(model, "free" if free else "fixed")


@pytest.mark.parametrize("model,free", th.CELLS, ids=th.IDS)
def test_every_cell_is_inside_the_float32_domain(model, free):
    for n in th.stars(ALL_N, free):
        case, _ = fh.cached_case(model, free, n)
        inside, kv, kt, _, reason = emul.f32_domain(case["cat"], case["params"][:S_MAX], model, case["centre"])
        assert inside, (n, kv, kt, reason)


@pytest.mark.parametrize("model,free", th.CELLS, ids=th.IDS)
def test_terms_of_the_restatement_and_the_host_build(model, free):
    mix = th.BG[model] != 0
    w = {k: (0.0, None) for k in ("np32 l", "np32 p", "rounded l", "rounded p", "host l", "host p")}

    def note(key, r, n):
        top, at = th.worst(r)
        if top > w[key][0]:
            w[key] = (top, (n,) + at)

    for n in th.stars(ALL_N, free):
        rows = rows_of(n)
        t = th.cached_terms(model, free, n, rows)
        case = t.case
        np32, at_rounded = t.np32(), t.exact_at_rounded()
        host_l, host_p = emul.per_star_f32(case["cat"], case["params"][rows], model, case["centre"])
        unit_l, unit_p = th.U * t.a_l, (th.U * t.a_p + th.FLOOR) if mix else None
        note("np32 l", th.ratio(np32["l"], t.exact["l"], unit_l), n)
        note("rounded l", th.ratio(at_rounded["l"], t.exact["l"], unit_l), n)
        note("host l", th.ratio(host_l, t.exact["l"], unit_l), n)
        if mix:
            note("np32 p", th.ratio(np32["p"], t.exact["p"], unit_p), n)
            note("rounded p", th.ratio(at_rounded["p"], t.exact["p"], unit_p), n)
            note("host p", th.ratio(host_p, t.exact["p"], unit_p), n)
        if n in (2, 65, 4099):
            # the record-level longdouble restatement is the reference's own per-star formula (arctan2 form, unrounded
            # columns): they differ by the float64 rounding of the records, 1e-5 of u A
            want_l, want_p = t.oracle()
            assert np.max(np.abs(t.exact["l"] - want_l) / (1 + np.abs(want_l))) < 1e-11, n
            if mix:
                assert np.max(np.abs(t.exact["p"] - want_p)) < 1e-11, n
    print("F32_TERM_NP32 {0}: value {1:.2f} u A at (N, row, star) {2}, membership {3:.2f} at {4}; exact at rounded inputs: "
          "{5:.2f} / {6:.2f}".format(name(model, free), w["np32 l"][0], w["np32 l"][1], w["np32 p"][0], w["np32 p"][1],
                                     w["rounded l"][0], w["rounded p"][0]))
    print("F32_TERM_HOST_ACCURACY {0} terms: value {1:.2f} u A at (N, row, star) {2}, membership {3:.2f} at {4}; "
          "bound C = {5}".format(name(model, free), w["host l"][0], w["host l"][1], w["host p"][0], w["host p"][1], th.C))
    assert w["np32 l"][0] <= th.C / 2 and w["np32 p"][0] <= th.C / 2, w
    assert w["rounded l"][0] <= th.C / 2 and w["rounded p"][0] <= th.C / 2, w
    assert w["host l"][0] <= th.C and w["host p"][0] <= th.C, w


@pytest.mark.parametrize("model,free", th.CELLS, ids=th.IDS)
def test_summaries_of_the_restatement_and_the_host_build(model, free):
    """lppd, lnl_var, pmem_mean, pmem_std at N x S of the device file: the per-term bounds propagated through the exact
    reduction.  The restatement's float32 terms, reduced exactly, within half the bound; the host build within it."""
    mem = th.BG[model] != 0
    worst = {}
    for n in th.stars(th.POST_N, free):
        t = th.cached_terms(model, free, n, range(S_MAX))
        case = t.case
        np32 = t.np32()
        for s in th.POST_S:
            x, p = t.exact["l"][:s], t.exact["p"][:s] if mem else None
            want, bound = th.posterior_summary(x, p, t.bound_l()[:s], t.bound_p()[:s] if mem else None)
            _, half = th.posterior_summary(x, p, t.bound_l(th.C / 2)[:s], t.bound_p(th.C / 2)[:s] if mem else None)
            rest = th.reduce_terms(np32["l"][:s], np32["p"][:s] if mem else None)
            host = dict(zip(th.POST_FIELDS, emul.posterior_f32(case["cat"], case["params"][:s], model, case["centre"], mem)))
            for f in want:
                for who, got, b in (("np32", rest[f], half[f]), ("host", host[f], bound[f])):
                    ok = np.abs(np.asarray(got, dtype=th.L) - want[f]) <= b
                    assert np.all(ok), (who, f, n, s, int(np.argmin(ok)))
                    with np.errstate(divide="ignore", invalid="ignore"):
                        r = np.where(b > 0, np.abs(np.asarray(got, dtype=th.L) - want[f]) / b, 0).astype(np.float64)
                    i = int(np.argmax(r))
                    if r[i] > worst.get((who, f), (0.0,))[0]:
                        worst[(who, f)] = (float(r[i]), n, s, i)
            if s == 1:
                assert np.all(host["lnl_var"] == 0) and (not mem or np.all(host["pmem_std"] == 0))
    for (who, f), (r, n, s, i) in sorted(worst.items()):
        print("F32_TERM_HOST_ACCURACY {0} {1} {2}: {3:.3f} of its bound at N = {4}, S = {5}, star {6}".format(
            name(model, free), who, f, r, n, s, i))


@pytest.mark.parametrize("model,free", th.CELLS, ids=th.IDS)
def test_predictive_fields_of_the_restatement_and_the_host_build(model, free):
    """mcd_posterior_predictive on a float32 catalogue: d and n from star_d_n<float>, the rest in float64.  Every (star,
    sample) quantity of the restatement within (C/2) u A of its own amplification; every output of the host build
    (tests/emul/predictive_emul.cpp with f32) within the propagated bound."""
    mix = model in pr.MIX_MODELS
    top, worst = {}, {}
    for n in (2 if (free and n == 1) else n for n in th.PRED_N):
        rows = S_MAX if n < 4099 else 65                # (the 257 x 4099 cell is left to the device file: 3 s of longdouble here)
        case = fh.cached_case(model, free, n)[0]
        rec, wp = th.records(case, range(rows))
        exact = pr.sample_terms(case["cat"], case["params"][:rows], model, case["centre"], th.L)
        amp = th.predictive_amplification(th.term(rec, wp, model, free, th.L, geometry_only=True), rec, wp, model, free, mix)
        np32 = th.predictive_np32(th.rounded(rec), th.rounded(wp), model, free, mix)
        assert set(amp) == set(np32) == set(exact)
        for k in amp:
            r = th.ratio(np32[k], exact[k], th.U * amp[k] + th.L(1e-13) * np.maximum(1, np.abs(exact[k])))
            top[k] = max(top.get(k, 0.0), float(r.max()))
        for s in (s for s in th.PRED_S if s <= rows):
            want, bound = th.predictive_summary({k: v[:s] for k, v in exact.items()}, {k: v[:s] for k, v in amp.items()})
            host = pr.predictive(case["cat"], case["params"][:s], model, case["centre"], mix=mix, f32=True)
            assert set(host) == set(want)
            for f in want:
                err = np.abs(host[f].astype(th.L) - want[f])
                assert np.all(err <= bound[f]), (f, n, s, int(np.argmax(err / bound[f])))
                r = (err / bound[f]).astype(np.float64)
                i = int(np.argmax(r))
                if r[i] > worst.get(f, (0.0,))[0]:
                    worst[f] = (float(r[i]), n, s, i)
    print("F32_TERM_NP32 {0} predictive terms, u A: {1}".format(
        name(model, free), ", ".join("{0} {1:.2f}".format(k, v) for k, v in sorted(top.items()))))
    for f, (r, n, s, i) in sorted(worst.items()):
        print("F32_TERM_HOST_ACCURACY {0} host {1}: {2:.3f} of its bound at N = {3}, S = {4}, star {5}".format(
            name(model, free), f, r, n, s, i))
    assert max(top.values()) <= th.C / 2, top


def touched(defect, model):
    return th.BG[model] != 0 if defect == "one_minus_m" else True


@pytest.mark.parametrize("model,free", th.CELLS, ids=th.IDS)
def test_the_bound_bites(model, free):
    """Each defect planted in the restatement must put a term (a summary field, for the shifted sample row) beyond the bound
    at every shape of the cell it touches: ln 2 pi truncated to 1.8379; (1 - m) dropped from the background branch; the sign
    of v_maxy flipped; the record of star i - 1 read for star i; the walker row of sample s - 1 read for sample s beyond
    the first slice."""
    mem = th.BG[model] != 0
    for defect in th.DEFECTS[:4]:
        if not touched(defect, model):
            continue
        least = np.inf
        for n in th.stars(th.PER_STAR_N, free):
            if defect == "star_shift" and n == 1:
                continue
            t = th.cached_terms(model, free, n, rows_of(n))
            bad = t.np32(defect)
            top = th.worst(th.ratio(bad["l"], t.exact["l"], t.bound_l()))[0]
            assert top > 1, (defect, n, top)
            least = min(least, top)
        print("F32_TERM_DEFECT {0} {1}: the worst term is at least {2:.3g} x its bound at every N".format(
            name(model, free), defect, least))
    least = np.inf
    for n in th.stars(th.POST_N, free):
        t = th.cached_terms(model, free, n, range(S_MAX))
        for s in (65, 257):
            slice_len = ph.plan(n, s)[1]
            assert slice_len < s
            x, p = t.exact["l"][:s], t.exact["p"][:s] if mem else None
            want, bound = th.posterior_summary(x, p, t.bound_l()[:s], t.bound_p()[:s] if mem else None)
            bad = th.term(th.rounded(t.rec), th.rounded(t.wp[:s]), model, free, np.float32, "sample_shift", slice_len)
            got = th.reduce_terms(bad["l"], bad["p"] if mem else None)
            top = max(float(np.max(np.abs(got[f] - want[f]) / bound[f])) for f in want)
            if (model, free, n, s) == (6, False, 1, 257):
                # the one star of this cell belongs to the fixed background (p ~ 0) in the rows beyond the first slice: its term does not depend on them
                # and the defect touches nothing -- the figure is printed; every other cell with one star is asserted
                print("F32_TERM_DEFECT {0} sample_shift at N = 1, S = {1}: {2:.3g} x the bound".format(name(model, free), s, top))
                continue
            assert top > 1, ("sample_shift", n, s, top)
            least = min(least, top)
    print("F32_TERM_DEFECT {0} sample_shift: the worst summary is at least {1:.3g} x its bound at every (N, S)".format(
        name(model, free), least))


@pytest.mark.parametrize("model,free,n", [(2, True, 257), (4, False, 65), (6, True, 65)], ids=["2-free", "4-fixed", "6-free"])
def test_outside_the_domain_the_ratio_is_reported(model, free, n):
    """variant_helper.make_case as it is: compact catalogues with a free centre (kappa_theta 40 - 200 x its limit), a velocity
    scale that leaves the float32 ranges (model 4 at N = 65).  per_star() and the summary launchers give no warning there; this is what the model says about the
    float32 restatement and the host build.  Reported, not asserted (only that the case IS outside, and finite)."""
    case = vh.make_case(model, free, n)
    rows = list(range(65))
    inside, kv, kt, _, reason = emul.f32_domain(case["cat"], case["params"][rows], model, case["centre"])
    assert not inside
    t = th.Terms(case, rows)
    np32 = t.np32()
    host_l, host_p = emul.per_star_f32(case["cat"], case["params"][rows], model, case["centre"])
    assert np.all(np.isfinite(host_l)) and np.all(np.isfinite(host_p))
    print("F32_TERM_OUTSIDE {0} (kappa_v {1:.3g}, kappa_theta {2:.3g}: {3}): value np32 {4:.2f} / host {5:.2f} u A, "
          "membership {6:.2f} / {7:.2f}; largest |error| of a value {8:.2e}, largest u A {9:.2e}".format(
              name(model, free), kv, kt, reason, th.worst(th.ratio(np32["l"], t.exact["l"], th.U * t.a_l))[0],
              th.worst(th.ratio(host_l, t.exact["l"], th.U * t.a_l))[0],
              th.worst(th.ratio(np32["p"], t.exact["p"], th.U * t.a_p + th.FLOOR))[0],
              th.worst(th.ratio(host_p, t.exact["p"], th.U * t.a_p + th.FLOOR))[0],
              float(np.max(np.abs(host_l - t.exact["l"]))), float(np.max(th.U * t.a_l))))
