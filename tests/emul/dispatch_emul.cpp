// TEST INFRASTRUCTURE ONLY -- the library's compile-time dispatch (csrc/mcd_dispatch.h) behind a C interface, so that
// tests/test_dispatch_cpu.py can see which constants each runtime value reaches.  Never loaded by the product package.
#include "mcd_dispatch.h"

using namespace mcd;

extern "C" int emul_num_models() { return kNumModels; }

// M * 2 + FREE of the pair the functor was called with, or `fallback`; *calls counts the functor's calls
extern "C" int emul_dispatch_model(int model, int free_centre, int fallback, int* calls) {
    return dispatch_model(model, free_centre != 0, [&](auto M, auto FREE) {
        ++*calls;
        return decltype(M)::value * 2 + (decltype(FREE)::value ? 1 : 0);
    }, fallback);
}

// bytes of the term type a precision selects
extern "C" int emul_dispatch_term_bytes(int precision) {
    return dispatch_term_type(precision, [](auto t) { return (int)sizeof(t); });
}
