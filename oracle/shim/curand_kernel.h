// curand_kernel.h — project-written stand-in for the part of NVIDIA's closed cuRAND device API that the reference's
// integrator.h, grid.h and form_factors.h call: curandState, curand_init, curand_uniform.  TEST INFRASTRUCTURE ONLY: it is
// found on the include paths of oracle/ref_integrator_harness.cpp and oracle/ref_solver_harness.cpp and nowhere else.  It
// restates nothing of the reference.
//
// Two modes, chosen per state:
//   stream   (script == nullptr): curand_init(seed, subsequence, 0) is the oracle's po_rng_init and curand_uniform the
//            oracle's po_rng_uniform.  The XORWOW step and the 2^67 skip-ahead behind them are pinned against rocRAND
//            (tests/test_rng_vs_rocrand.py); cuRAND's seed scramble and its word-to-float mapping are closed and stay
//            UNPINNED: whole frames rendered through this mode pin the integrator, not the generator.
//   scripted (script != nullptr): curand_uniform maps the next caller-supplied raw 32-bit word x to x * 2^-32 + 2^-33,
//            evaluated in binary32 (0xFFFFFFFF gives exactly 1.0f).  Every draw is counted in `used`; a draw past the end
//            of the script sets `overrun` and returns 1.0f.
#pragma once
#include <stdint.h>

extern "C" {
void po_rng_init(uint64_t seed, uint64_t subsequence, uint32_t state[6]);
float po_rng_uniform(uint32_t state[6]);
}

struct curandStateXORWOW {
    uint32_t s[6];
    const uint32_t* script;
    int n_script, used, overrun;
};
typedef curandStateXORWOW curandState_t;
typedef curandStateXORWOW curandState;

static inline float ptmi_shim_word_to_uniform(uint32_t x) { return (float)x * 0x1p-32f + 0x1p-33f; }

static inline void curand_init(unsigned long long seed, unsigned long long subsequence, unsigned long long offset,
                               curandState* state) {
    (void)offset;   // 0 at every call site of the reference (integrator.h render_init, form_factors.h formfactor_rand_init)
    po_rng_init(seed, subsequence, state->s);
    state->script = nullptr;
    state->n_script = state->used = state->overrun = 0;
}

static inline float curand_uniform(curandState* state) {
    if (!state->script) { state->used++; return po_rng_uniform(state->s); }
    if (state->used >= state->n_script) { state->overrun = 1; return 1.0f; }
    return ptmi_shim_word_to_uniform(state->script[state->used++]);
}
