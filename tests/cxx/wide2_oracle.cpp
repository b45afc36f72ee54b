// TEST INFRASTRUCTURE ONLY: the HOST form of the two-stage tuner of m17hip_wide_config2 — m17cxx/detail/core.h (ddc_mix, ddc_fir2 and the discriminator
// behind them) compiled by the host compiler, the same text the kernel's arithmetic is.  One channel on one source row, with the source's history, the feed's
// sample count and the channel's carry in / out, as wide_oracle.cpp has it for one stage.  Built and loaded by tests/wide2_lib.py (g++ -O2 -ffp-contract=off).
#include "../../m17-cxx-demod_amd/include/m17cxx/detail/core.h"

#include <stddef.h>
#include <vector>

namespace core = mobilinkd::core;

extern "C" {

// row: n * R1 * R2 interleaved I,Q samples of one source (format 1: int16, 2: float32, 3: uint8, as M17HIP_IQ_*); hist: the H = (L2 - 1) R1 + L1 - 1 converted
// samples in front of the row ([H][2], oldest first), on return those in front of the next row; count: the feed's sample index of the row's first sample;
// carry[2]: the z in front of the row's first output, on return the row's last z.  out[n]: the discriminated floats; zout ([n][2]) may be NULL.
void wo2_tune(const void* row, int format, size_t n, uint32_t R1, const float* h1, uint32_t L1, uint32_t R2, const float* h2, uint32_t L2, int32_t fcw,
              uint64_t count, float* hist, float* carry, float gain, float* out, float* zout)
{
    const size_t H = (size_t)(L2 - 1) * R1 + L1 - 1, W = n * R1 * R2;
    std::vector<float> x(2 * (H + W)), mixed(2 * (H + W)), u(2 * ((size_t)L2 - 1 + n * R2)), z(2 * n);
    for (size_t k = 0; k < 2 * H; ++k) x[k] = hist[k];
    for (size_t k = 0; k < 2 * W; ++k) {
        if (format == 1) x[2 * H + k] = (float)((const int16_t*)row)[k];
        else if (format == 2) x[2 * H + k] = ((const float*)row)[k];
        else x[2 * H + k] = core::ddc_u8(((const uint8_t*)row)[k]);
    }
    for (size_t k = 0; k < H + W; ++k)   // (sample k of the row is index H + k here; the history's indices wrap below the count like any other)
        core::ddc_mix(x[2 * k], x[2 * k + 1], (uint32_t)fcw, (uint32_t)(count + k - H), mixed[2 * k], mixed[2 * k + 1]);
    core::ddc_fir2(h1, L1, R1, h2, L2, R2, mixed.data() + 2 * H, (uint32_t)n, L2 - 1, u.data() + 2 * ((size_t)L2 - 1), z.data());
    float pre = carry[0], pim = carry[1];
    for (size_t m = 0; m < n; ++m) {
        out[m] = core::fm_discriminate(z[2 * m], z[2 * m + 1], pre, pim, gain);
        if (zout) { zout[2 * m] = z[2 * m]; zout[2 * m + 1] = z[2 * m + 1]; }
        pre = z[2 * m]; pim = z[2 * m + 1];
    }
    carry[0] = pre; carry[1] = pim;
    for (size_t k = 0; k < 2 * H; ++k) hist[k] = x[2 * W + k];
}

}
