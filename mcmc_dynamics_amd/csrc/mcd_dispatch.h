// mcd_dispatch.h -- runtime (model, free_centre) and term precision -> compile-time constants, written once for every
// launcher of the library and for the host builds of the same arithmetic (tests/emul).  No HIP types.
#pragma once

#include <type_traits>

#include "mcd_math.h"

namespace mcd {

// The list of the models of the reference's running classes (mcd_math.h: Model, kNumModels); the double Lynden-Bell models
// follow in MCD_DOUBLE_MODEL_LIST below, and a launcher reaches both lists through dispatch_any_model
#define MCD_MODEL_LIST(X)                                                                                           \
    X(MODEL_CONST) X(MODEL_BGFIXED) X(MODEL_BGGAUSS) X(MODEL_PROFILE) X(MODEL_PROFILE_BGGAUSS) X(MODEL_PROFILE_BGDENS) \
    X(MODEL_PROFILE_BGFIXED)

// f(std::integral_constant<int, M>{}, std::bool_constant<FREE>{}) of the matching pair; `fallback`, without a call of f,
// for a model outside [0, kNumModels).  What a model or a centre lacks is an `if constexpr` inside f.
template <class F, class R>
R dispatch_model(int model, bool free_centre, F&& f, R fallback) {
#define MCD_MODEL_COUNT(M) +1
    static_assert(0 MCD_MODEL_LIST(MCD_MODEL_COUNT) == kNumModels, "MCD_MODEL_LIST names every model");
#undef MCD_MODEL_COUNT
#define MCD_MODEL_CASE(M)                                                                   \
    case M:                                                                                 \
        return free_centre ? f(std::integral_constant<int, M>{}, std::true_type{})          \
                           : f(std::integral_constant<int, M>{}, std::false_type{});
    switch (model) { MCD_MODEL_LIST(MCD_MODEL_CASE) }
#undef MCD_MODEL_CASE
    return fallback;
}
#undef MCD_MODEL_LIST

// The launchers' dispatcher: the models of dispatch_model and, behind them, the double Lynden-Bell models (models
// kNumModels .. kNumAllModels - 1; mcd_math.h: is_double).  The launchers reach it through dispatch_launch_model below;
// dispatch_model keeps the list of the reference's running classes, which the host builds of the older test harnesses are
// written for.
#define MCD_DOUBLE_MODEL_LIST(X) X(MODEL_DOUBLE) X(MODEL_DOUBLE_BGGAUSS)
template <class F, class R>
R dispatch_any_model(int model, bool free_centre, F&& f, R fallback) {
#define MCD_MODEL_COUNT(M) +1
    static_assert(kNumModels MCD_DOUBLE_MODEL_LIST(MCD_MODEL_COUNT) == kNumAllModels, "MCD_DOUBLE_MODEL_LIST names every further model");
#undef MCD_MODEL_COUNT
#define MCD_MODEL_CASE(M)                                                                   \
    case M:                                                                                 \
        return free_centre ? f(std::integral_constant<int, M>{}, std::true_type{})          \
                           : f(std::integral_constant<int, M>{}, std::false_type{});
    switch (model) { MCD_DOUBLE_MODEL_LIST(MCD_MODEL_CASE) }
#undef MCD_MODEL_CASE
    return dispatch_model(model, free_centre, static_cast<F&&>(f), fallback);
}
#undef MCD_DOUBLE_MODEL_LIST

// The launchers' dispatcher since the error-scale models (ids 10 and 11, id 9 is unassigned; mcd_math.h: is_escale,
// is_launch_model): those two, and behind them everything dispatch_any_model lists.  Every launcher of the library calls this one;
// dispatch_any_model keeps its nine models, which the host builds of the double models' test harness are written for.
#define MCD_ESCALE_MODEL_LIST(X) X(MODEL_CONST_ESCALE) X(MODEL_PROFILE_ESCALE)
template <class F, class R>
R dispatch_launch_model(int model, bool free_centre, F&& f, R fallback) {
#define MCD_MODEL_COUNT(M) +1
    static_assert(kNumAllModels + 1 MCD_ESCALE_MODEL_LIST(MCD_MODEL_COUNT) == kNumLaunchModels, "MCD_ESCALE_MODEL_LIST names every further model but the unassigned id 9");
#undef MCD_MODEL_COUNT
#define MCD_MODEL_CASE(M)                                                                   \
    case M:                                                                                 \
        return free_centre ? f(std::integral_constant<int, M>{}, std::true_type{})          \
                           : f(std::integral_constant<int, M>{}, std::false_type{});
    switch (model) { MCD_ESCALE_MODEL_LIST(MCD_MODEL_CASE) }
#undef MCD_MODEL_CASE
    return dispatch_any_model(model, free_centre, static_cast<F&&>(f), fallback);
}
#undef MCD_ESCALE_MODEL_LIST

// f(T{}) with the type of the terms: double for precision 0 (MCD_F64), float for the float32 catalogues
template <class F>
auto dispatch_term_type(int precision, F&& f) {
    return precision == 0 ? f(double{}) : f(float{});
}

// ... for a launcher that knows its MODEL: the error-scale models are float64 only (mcd_catalog_create refuses the float32
// precisions for them), so no float instantiation is built for them and a float precision returns `refused`
template <int MODEL, class F, class R>
R dispatch_model_term_type(int precision, F&& f, R refused) {
    if constexpr (is_escale(MODEL)) return precision == 0 ? f(double{}) : refused;
    else return precision == 0 ? f(double{}) : f(float{});
}

}  // namespace mcd
