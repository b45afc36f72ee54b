// TEST INFRASTRUCTURE ONLY: the HOST form of the noise floor of m17hip_wide_squelch_floor — m17cxx/detail/core.h's squelch_floor_key, squelch_floor_median,
// squelch_floor, squelch_track and squelch_floor_level, compiled by the host compiler.  Built and loaded by tests/squelch_floor_lib.py (g++ -O2
// -ffp-contract=off).  The planes come from spectrum_lib; the levels go to squelch_lib's and squelch_slots_lib's host forms as given levels do.
#include "../../m17-cxx-demod_amd/include/m17cxx/detail/core.h"

#include <stddef.h>

namespace core = mobilinkd::core;

extern "C" {

uint32_t sf_key(float x) { return core::squelch_floor_key(x); }

uint32_t sf_nan(void) { return core::SQUELCH_FLOOR_NAN; }

float sf_median(const float* row, uint32_t N) { return core::squelch_floor_median(row, N); }

float sf_floor(float med, uint32_t B, uint32_t J, float floor_min) { return core::squelch_floor(med, B, J, floor_min); }

float sf_track(float F, float f, float rise, float fall) { return core::squelch_track(F, f, rise, fall); }

float sf_level(float F, float ratio) { return core::squelch_floor_level(F, ratio); }

// One block's floor for S sources: plane[S][N] of J frames; carry[S] is stepped in place (left as it is where J == 0); out[4][S] = med | F' | open | close —
// what squelch_floor_kernel does, a source after the other.
void sf_block(const float* plane, uint32_t N, uint32_t J, uint32_t S, uint32_t B, float open_ratio, float close_ratio, float rise, float fall,
              float floor_min, float* carry, float* out)
{
    for (uint32_t s = 0; s < S; ++s) {
        const float med = core::squelch_floor_median(plane + (size_t)s * N, N);
        float F = carry[s];
        if (J) F = core::squelch_track(F, core::squelch_floor(med, B, J, floor_min), rise, fall);
        carry[s] = F;
        out[s] = med;
        out[S + s] = F;
        out[2 * (size_t)S + s] = core::squelch_floor_level(F, open_ratio);
        out[3 * (size_t)S + s] = core::squelch_floor_level(F, close_ratio);
    }
}

}
