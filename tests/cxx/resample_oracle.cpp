// TEST INFRASTRUCTURE ONLY: the HOST form of the resampling tuner of m17hip_wide_resample — m17cxx/detail/core.h's ddc_resample compiled by the host
// compiler, the same text the kernel's arithmetic is.  One channel on one source row, with the source's history, the feed's sample count and the channel's
// carry in / out, as wide2_oracle.cpp has it for two integer stages.  Built and loaded by tests/resample_lib.py (g++ -O2 -ffp-contract=off).
#include "../../m17-cxx-demod_amd/include/m17cxx/detail/core.h"

#include <stddef.h>
#include <vector>

namespace core = mobilinkd::core;

extern "C" {

// row: (n / U) * D * R1 interleaved I,Q samples of one source (format 1: int16, 2: float32, 3: uint8, as M17HIP_IQ_*), n a multiple of U; hist: the
// H = (ceil(L2 / U) - 1) R1 + L1 - 1 converted samples in front of the row ([H][2], oldest first), on return those in front of the next row; count: the
// feed's sample index of the row's first sample; carry[2]: the z in front of the row's first output, on return the row's last z.  out[n]: the discriminated
// floats; zout ([n][2]) may be NULL.
void ro_resample(const void* row, int format, size_t n, uint32_t R1, const float* h1, uint32_t L1, uint32_t U, uint32_t D, const float* h2, uint32_t L2,
                 int32_t fcw, uint64_t count, float* hist, float* carry, float gain, float* out, float* zout)
{
    const size_t J2 = (L2 + U - 1) / U, H = (J2 - 1) * R1 + L1 - 1, NU = n / U * D, W = NU * R1;
    std::vector<float> x(2 * (H + W)), mixed(2 * (H + W)), u(2 * (J2 - 1 + NU)), z(2 * n + 2);
    for (size_t k = 0; k < 2 * H; ++k) x[k] = hist[k];
    for (size_t k = 0; k < 2 * W; ++k) {
        if (format == 1) x[2 * H + k] = (float)((const int16_t*)row)[k];
        else if (format == 2) x[2 * H + k] = ((const float*)row)[k];
        else x[2 * H + k] = core::ddc_u8(((const uint8_t*)row)[k]);
    }
    core::ddc_resample(h1, L1, R1, h2, L2, U, D, x.data() + 2 * H, (uint32_t)fcw, (uint32_t)count, (uint32_t)n, mixed.data(), u.data(), z.data(), carry, gain,
                       out);
    if (zout) for (size_t k = 0; k < 2 * n; ++k) zout[k] = z[k];
    for (size_t k = 0; k < 2 * H; ++k) hist[k] = x[2 * W + k];
}

}
