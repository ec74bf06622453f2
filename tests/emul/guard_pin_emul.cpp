// TEST INFRASTRUCTURE ONLY -- the guard of csrc/mcd_guard.h on one parameter table, through nothing but the names the file
// had before the error-scale models (compute_stats, table_ranges, guard_verdict, level_verdict, GuardRanges): the same source
// builds against an older mcd_guard.h, which is how the values pinned in tests/test_escale_guard_cpu.py were made.  Never
// loaded by the product package.
#include <cstdint>

#include "mcd_guard.h"
#include "mcd_math.h"

using namespace mcd;

// out[0] = guard_verdict (0 / 1), out[1] = level_verdict, out[2] = GuardRanges.n_min, out[3] = n_max (0 where the verdict
// returned before it formed them)
extern "C" void guard_pin(int model, int free_centre, int64_t n, const double* ra, const double* dec, const double* v,
                          const double* verr, const double* lnbg, const double* pmember, const double* density, double ra_c,
                          double dec_c, int k, const double* params, int64_t n_rows, double* out) {
    const CatalogStats st = compute_stats(n, v, verr, lnbg, pmember, density, bg_kind(model), is_profile(model) ? ra : nullptr,
                                          dec, free_centre == 0, ra_c, dec_c);
    const ParamRanges pr = table_ranges(model, free_centre != 0, k, params, n_rows);
    GuardRanges g;
    out[0] = guard_verdict(st, model, false, n_rows, pr, &g) ? 1.0 : 0.0;
    out[1] = (double)level_verdict(st, model, false, n_rows, pr);
    out[2] = g.n_min;
    out[3] = g.n_max;
}
