// TEST INFRASTRUCTURE ONLY: the HOST form of the raster survey of m17hip_wide_survey — m17cxx/detail/core.h's chan_power and the two-level sum
// (CHAN_SURVEY_GROUP powers per group, both levels chains of plain float adds from +0 in ascending order) over z words handed in, compiled by the host
// compiler.  The z are the channeliser's (tests/cxx/raster_oracle.cpp through tests/raster_lib.py).  Built and loaded by tests/survey_lib.py
// (g++ -O2 -ffp-contract=off; the fmaf in chan_power is explicit).
#include "../../m17-cxx-demod_amd/include/m17cxx/detail/core.h"

#include <stddef.h>

namespace core = mobilinkd::core;

extern "C" {

uint32_t so_group(void) { return core::CHAN_SURVEY_GROUP; }

// z: [nb][n][2], the z of nb bins at the n outputs of one block; times[J]: the block's survey times, ascending, each < n.  out[nb]: the plane's words.
// single != 0: ONE ascending chain over all J powers in place of the two levels (what the definition is NOT; the tests show that the two differ).
void so_plane(const float* z, size_t nb, size_t n, const uint32_t* times, size_t J, int single, float* out)
{
    for (size_t b = 0; b < nb; ++b) {
        const float* zb = z + 2 * b * n;
        float P = 0.0f;
        if (single) {
            for (size_t j = 0; j < J; ++j) P = P + core::chan_power(zb[2 * times[j]], zb[2 * times[j] + 1]);
        } else {
            for (size_t g = 0; g * core::CHAN_SURVEY_GROUP < J; ++g) {
                float q = 0.0f;
                for (size_t j = g * core::CHAN_SURVEY_GROUP; j < J && j < (g + 1) * core::CHAN_SURVEY_GROUP; ++j)
                    q = q + core::chan_power(zb[2 * times[j]], zb[2 * times[j] + 1]);
                P = P + q;
            }
        }
        out[b] = P;
    }
}

}
