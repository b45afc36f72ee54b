// TEST INFRASTRUCTURE ONLY: the HOST form of the tuner of m17hip_upload_wide — m17cxx/detail/core.h (nco, ddc_mix, ddc_tap / ddc_fir, ddc_u8 and the
// discriminator behind them) compiled by the host compiler, the same text the kernel compiles.  One channel on one source row, with the source's history, the
// feed's sample count and the channel's carry in / out, and the pieces on arrays for the tests of the arithmetic itself.  Built and loaded by
// tests/wide_lib.py (g++ -O2 -ffp-contract=off).
#include "../../m17-cxx-demod_amd/include/m17cxx/detail/core.h"

#include <stddef.h>
#include <vector>

namespace core = mobilinkd::core;

extern "C" {

void wo_nco(const uint32_t* p, size_t n, float* c, float* s)
{
    for (size_t k = 0; k < n; ++k) core::nco(p[k], c[k], s[k]);
}
// the filter's sum over L mixed samples, oldest first in `mixed` ([L][2]): z[0..1]
void wo_fir(const float* h, uint32_t L, const float* mixed, float* z)
{
    core::ddc_fir(h, L, mixed + 2 * (size_t)(L - 1), z[0], z[1]);
}
// row: n * R interleaved I,Q samples of one source (format 1: int16, 2: float32, 3: uint8, as M17HIP_IQ_*); hist: the L - 1 converted samples in front of the
// row ([L-1][2], oldest first), on return those in front of the next row; count: the feed's sample index of the row's first sample; carry[2]: the z in front
// of the row's first output, on return the row's last z.  out[n]: the discriminated floats; zout ([n][2]) may be NULL.
void wo_tune(const void* row, int format, size_t n, uint32_t R, const float* h, uint32_t L, int32_t fcw, uint64_t count, float* hist, float* carry, float gain,
             float* out, float* zout)
{
    const size_t H = L - 1, W = n * R;
    std::vector<float> x(2 * (H + W)), mixed(2 * (H + W));
    for (size_t k = 0; k < 2 * H; ++k) x[k] = hist[k];
    for (size_t k = 0; k < 2 * W; ++k) {
        if (format == 1) x[2 * H + k] = (float)((const int16_t*)row)[k];
        else if (format == 2) x[2 * H + k] = ((const float*)row)[k];
        else x[2 * H + k] = core::ddc_u8(((const uint8_t*)row)[k]);
    }
    for (size_t k = 0; k < H + W; ++k)   // (sample k of the row is index H + k here; the history's indices wrap below the count like any other)
        core::ddc_mix(x[2 * k], x[2 * k + 1], (uint32_t)fcw, (uint32_t)(count + k - H), mixed[2 * k], mixed[2 * k + 1]);
    float pre = carry[0], pim = carry[1];
    for (size_t m = 0; m < n; ++m) {
        float re, im;
        core::ddc_fir(h, L, &mixed[2 * (H + m * R + R - 1)], re, im);
        out[m] = core::fm_discriminate(re, im, pre, pim, gain);
        if (zout) { zout[2 * m] = re; zout[2 * m + 1] = im; }
        pre = re; pim = im;
    }
    carry[0] = pre; carry[1] = pim;
    for (size_t k = 0; k < 2 * H; ++k) hist[k] = x[2 * W + k];
}

}
