// TEST INFRASTRUCTURE ONLY: the HOST form of the channeliser of m17hip_wide_raster — m17cxx/detail/core.h (chan_fold, chan_pass1, chan_pass2, ddc_u8 and the
// discriminator behind them) compiled by the host compiler, the same text the kernel's arithmetic is.  Some bins of one source row, with the source's history,
// the feed's sample count and the bins' carries in / out, as wide_oracle.cpp has it for the tuner.  Built and loaded by tests/raster_lib.py
// (g++ -O2 -ffp-contract=off).
#include "../../m17-cxx-demod_amd/include/m17cxx/detail/core.h"

#include <stddef.h>
#include <vector>

namespace core = mobilinkd::core;

extern "C" {

// M = M1 x M2 as the library factors it: 0 where it refuses M
int ro_factor(uint32_t M, uint32_t* M1, uint32_t* M2) { return core::chan_factor(M, *M1, *M2) ? 1 : 0; }

// row: n * R interleaved I,Q samples of one source (format 1: int16, 2: float32, 3: uint8, as M17HIP_IQ_*); hist: the L - 1 converted samples in front of the
// row ([L-1][2], oldest first), on return those in front of the next row; count: the feed's sample index of the row's first sample (all 64 bits; only
// count mod M enters); tw: the twiddle table ([M][2]); k[nb]: the bins mod M; carry[nb][2]: the z in front of the row's first output, on return the row's
// last z.  out[nb][n]: the discriminated floats; zout ([nb][n][2]) may be NULL.  Returns 0 where M does not factor.
int ro_chan(const void* row, int format, size_t n, uint32_t R, const float* h, uint32_t L, uint32_t M, const float* tw, const uint32_t* k, uint32_t nb,
            uint64_t count, float* hist, float* carry, float gain, float* out, float* zout)
{
    uint32_t M1, M2;
    if (!core::chan_factor(M, M1, M2)) return 0;
    const size_t H = L - 1, W = n * R;
    std::vector<float> x(2 * (H + W) + 2), w(2 * (size_t)M), a(2 * (size_t)M);
    for (size_t j = 0; j < 2 * H; ++j) x[j] = hist[j];
    for (size_t j = 0; j < 2 * W; ++j) {
        if (format == 1) x[2 * H + j] = (float)((const int16_t*)row)[j];
        else if (format == 2) x[2 * H + j] = ((const float*)row)[j];
        else x[2 * H + j] = core::ddc_u8(((const uint8_t*)row)[j]);
    }
    for (size_t m = 0; m < n; ++m) {
        const size_t newest = H + m * R + R - 1;                 // in x; the feed's sample count + m R + R - 1
        const uint32_t mm = (uint32_t)((count + m * R + R - 1) % M);
        for (uint32_t r = 0; r < M; ++r) core::chan_fold(h, L, M, (mm + M - r) % M, &x[2 * newest], w[2 * r], w[2 * r + 1]);
        for (uint32_t r1 = 0; r1 < M1; ++r1)
            for (uint32_t k2 = 0; k2 < M2; ++k2) core::chan_pass1(w.data(), M1, M2, tw, r1, k2, a[2 * (r1 * M2 + k2)], a[2 * (r1 * M2 + k2) + 1]);
        for (uint32_t b = 0; b < nb; ++b) {
            float re, im;
            core::chan_pass2(a.data(), M1, M2, tw, k[b], re, im);
            out[b * n + m] = core::fm_discriminate(re, im, carry[2 * b], carry[2 * b + 1], gain);
            if (zout) { zout[2 * (b * n + m)] = re; zout[2 * (b * n + m) + 1] = im; }
            carry[2 * b] = re; carry[2 * b + 1] = im;
        }
    }
    for (size_t j = 0; j < 2 * H; ++j) hist[j] = x[2 * W + j];
    return 1;
}

}
