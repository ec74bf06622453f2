"""GPU: the float32 per-star terms and per-star summaries against the reference's formulas in numpy.longdouble on the
UNROUNDED inputs, each term within C u A of tests/f32_term_helper.py and each summary field within the
bound propagated from it.  The inputs are f32_helper.f32_case (inside the float32 accuracy domain:
tests/test_f32_terms_cpu.py asserts it for every cell of this file; these entry points do not consult the domain).

  * loglike_per_star / membership (per_star_kernel<..., float>, one thread per star, 256 per block): models 1, 2, 4, 5, 6 x
    fixed / free centre x N in (1, 2, 63, 64, 65, 255, 256, 257, 4099), three rows each;
  * pointwise_posterior (posterior_slice_kernel / posterior_merge_kernel): all 7 models x fixed / free x N in (1, 63, 65, 130)
    x S in (1, 2, 64, 65, 257) -- S = 1 makes lppd_i the term itself, the only route to the terms of CONST / PROFILE in
    float32; S = 65 is two slices of 33 + 32, S = 257 five with a short last one -- all four fields, and S = 257 again in
    three passes of 100 rows (per-pass plans and the merge of the kept state);
  * psis_loo / psis_loo_expect at S = 257 in one pass and in three: bit for bit equal (the float32 row offset of the sample table);
  * posterior_predictive: N in (1, 65, 4099) x S in (1, 65, 257), every field.
A free centre with one star has no float32 domain (the star is the centroid): N = 1 is a fixed-centre shape.  "f32" and
"f32acc64" catalogues run ONE instantiation of these kernels (the accumulator type is a template argument of the main kernel
only): bit for bit equal, asserted.  The F32_TERM_ACCURACY lines report the worst |device - exact| / bound per cell."""
import numpy as np
import pytest

import f32_helper as fh
import f32_term_helper as th
import predictive_helper as pr
import variant_helper as vh

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="no extended-precision long double on this platform")]

S_MAX = max(th.POST_S)
PER_STAR_CELLS = [(m, f) for m, f in th.CELLS if m in th.PER_STAR_MODELS]
PER_STAR_IDS = ["{0}-{1}".format(m, "free" if f else "fixed") for m, f in PER_STAR_CELLS]


@pytest.fixture(scope="module")
def native():
    from mcmc_dynamics_amd import _native
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    return native.default_context()


def name(model, free):
    return "model {0} {1}".format(model, "free" if free else "fixed")


class Worst(object):
    """The largest |got - want| / bound per key, where it was, and every element beyond its bound."""

    def __init__(self):
        self.top, self.failures = {}, []

    def note(self, key, got, want, bound, where):
        err = np.abs(np.asarray(got, dtype=th.L) - want)
        assert np.all(np.isfinite(np.asarray(got, dtype=np.float64))), (key, where)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err > 0, err / bound, 0).astype(np.float64)        # err = bound = 0 (a variance at S = 1) is 0
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        if r[i] > self.top.get(key, (-1.0,))[0]:
            self.top[key] = (float(r[i]), where + tuple(int(j) for j in i))
        if not r[i] <= 1:
            self.failures.append((key, where + tuple(int(j) for j in i), float(r[i])))

    def report(self, cell, what):
        for key, (r, where) in sorted(self.top.items()):
            print("F32_TERM_ACCURACY {0} {1} {2}: worst {3:.3f} of its bound at {4}".format(cell, what, key, r, where))


@pytest.mark.parametrize("model,free", PER_STAR_CELLS, ids=PER_STAR_IDS)
def test_per_star_terms_against_the_80_bit_oracle(native, ctx, model, free):
    w = Worst()
    for n in th.stars(th.PER_STAR_N, free):
        t = th.cached_terms(model, free, n, th.PER_STAR_ROWS)
        want_l, want_p = t.oracle()
        g32 = vh.catalog(native, ctx, t.case, precision="f32")
        g64acc = vh.catalog(native, ctx, t.case, precision="f32acc64")
        for k, row in enumerate(th.PER_STAR_ROWS):
            params = t.case["params"][row]
            got_l, got_p = g32.loglike_per_star(params), g32.membership(params)
            assert got_l.shape == (n,) and got_p.shape == (n,)
            assert got_l.tobytes() == g32.loglike_per_star(params).tobytes(), ("value not repeatable", n, row)
            assert got_p.tobytes() == g32.membership(params).tobytes(), ("membership not repeatable", n, row)
            # one kernel instantiation serves both float32 precisions
            assert got_l.tobytes() == g64acc.loglike_per_star(params).tobytes(), ("f32 / f32acc64 values differ", n, row)
            assert got_p.tobytes() == g64acc.membership(params).tobytes(), ("f32 / f32acc64 memberships differ", n, row)
            w.note("value", got_l, want_l[k], t.bound_l()[k], (n, row))
            w.note("membership", got_p, want_p[k], t.bound_p()[k], (n, row))
        g32.close()
        g64acc.close()
    w.report(name(model, free), "per_star (N, row, star)")
    assert set(w.top) == {"value", "membership"}
    assert not w.failures, w.failures


@pytest.mark.parametrize("model,free", th.CELLS, ids=th.IDS)
def test_pointwise_posterior_against_the_80_bit_oracle(native, ctx, model, free):
    mem = th.BG[model] != 0
    w = Worst()
    for n in th.stars(th.POST_N, free):
        t = th.cached_terms(model, free, n, range(S_MAX))
        x_all, p_all = t.oracle()
        g = vh.catalog(native, ctx, t.case, precision="f32")
        for s in th.POST_S:
            table = np.ascontiguousarray(t.case["params"][:s])
            x, p = x_all[:s], p_all[:s] if mem else None
            want, bound = th.posterior_summary(x, p, t.bound_l()[:s], t.bound_p()[:s] if mem else None)
            got = g.pointwise_posterior(table, membership=mem)
            assert set(got) == set(want)
            again = g.pointwise_posterior(table, membership=mem)
            for f in want:
                assert got[f].tobytes() == again[f].tobytes(), ("not repeatable", f, n, s)
                w.note(f, got[f], want[f], bound[f], (n, s))
            if s == 1:
                # lppd_i is the term itself: held to the per-term bound directly, not through the propagation
                w.note("term (S = 1)", got["lppd"], x[0], t.bound_l()[0], (n, s))
                assert np.all(got["lnl_var"] == 0) and (not mem or np.all(got["pmem_std"] == 0))
            if s == S_MAX and n == 65:
                # three passes of 100, 100 and 57 rows: the per-pass slice plans and the merge through the kept state, on
                # float32 terms.  (Every pass writes its derived rows at row 0 of the one pass buffer: the row offset of
                # upload_samples is 0 here and is reached by the PSIS launchers only -- the test after this one.)
                g.set_option("posterior_pass", th.POST_PASS)
                passes = g.pointwise_posterior(table, membership=mem)
                g.set_option("posterior_pass", 65536)
                for f in want:
                    scale = np.maximum(np.abs(got[f]), 1.0)
                    assert np.max(np.abs(passes[f] - got[f]) / scale) < 1e-13, ("passes", f, n, s)
                    w.note(f, passes[f], want[f], bound[f], (n, s))
        if n == 65:
            other = vh.catalog(native, ctx, t.case, precision="f32acc64")
            table = np.ascontiguousarray(t.case["params"][:65])
            a, b = g.pointwise_posterior(table, membership=mem), other.pointwise_posterior(table, membership=mem)
            for f in a:
                assert a[f].tobytes() == b[f].tobytes(), ("f32 / f32acc64 differ", f)
            other.close()
        g.close()
    w.report(name(model, free), "pointwise_posterior (N, S, star)")
    assert set(w.top) == set(th.POST_FIELDS[:4 if mem else 2]) | {"term (S = 1)"}
    assert not w.failures, w.failures


@pytest.mark.parametrize("model,free", th.CELLS, ids=th.IDS)
def test_psis_sample_table_is_filled_in_passes_at_the_float32_row_offset(native, ctx, model, free):
    """psis_loo and psis_loo_expect derive ALL S sample rows into one [S][KD] table before their term kernels run; with
    option posterior_pass = 100 the rows of S = 257 arrive in passes of 100, 100 and 57 and upload_samples writes pass p at
    byte offset 100 p x KD x 4 of a float32 catalogue (x 8 of a float64 one).  The table a pass plan leaves is the same
    table, so every output is bit for bit the one-pass output; a row offset in the wrong precision would put the second and
    third pass elsewhere.  (No accuracy bound here: the PSIS tail selection is not a first-order function of the terms.)"""
    t = th.cached_terms(model, free, 65, range(S_MAX))
    table = np.ascontiguousarray(t.case["params"][:S_MAX])
    mix = model in pr.MIX_MODELS
    for precision in ("f32", "f32acc64"):
        g = vh.catalog(native, ctx, t.case, precision=precision)
        one = g.psis_loo(table), g.psis_loo_expect(table, mixture=mix)
        g.set_option("posterior_pass", th.POST_PASS)
        many = g.psis_loo(table), g.psis_loo_expect(table, mixture=mix)
        g.close()
        for a, b in zip(one, many):
            assert set(a) == set(b)
            for f in a:
                assert f not in ("elpd_loo", "lppd") or np.all(np.isfinite(a[f])), (precision, f)
                assert a[f].tobytes() == b[f].tobytes(), ("the pass plan changed the bits", precision, f)


def pred_stars(free):
    """predictive_helper.MATRIX_N; with a free centre the lone star is replaced by two (no domain at N = 1)."""
    return tuple(2 if (free and n == 1) else n for n in th.PRED_N)


@pytest.mark.parametrize("model,free", th.CELLS, ids=th.IDS)
def test_posterior_predictive_against_the_80_bit_oracle(native, ctx, model, free):
    mix = model in pr.MIX_MODELS
    w = Worst()
    for n in pred_stars(free):
        case = fh.cached_case(model, free, n)[0]
        rec, wp = th.records(case, range(S_MAX))
        exact = pr.sample_terms(case["cat"], case["params"][:S_MAX], model, case["centre"], th.L)
        amp = th.predictive_amplification(th.term(rec, wp, model, free, th.L, geometry_only=True), rec, wp, model, free, mix)
        g = vh.catalog(native, ctx, case, precision="f32")
        for s in th.PRED_S:
            table = np.ascontiguousarray(case["params"][:s])
            want, bound = th.predictive_summary({k: v[:s] for k, v in exact.items()}, {k: v[:s] for k, v in amp.items()})
            got = g.posterior_predictive(table, mixture=mix)
            assert set(got) == set(want)
            for f in want:
                w.note(f, got[f], want[f], bound[f], (n, s))
        g.close()
    w.report(name(model, free), "posterior_predictive (N, S, star)")
    assert len(w.top) == (9 if mix else 8)
    assert not w.failures, w.failures
