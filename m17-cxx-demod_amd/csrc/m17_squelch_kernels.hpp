// K-1q: the spectrum squelch in front of the three tuners (m17hip_wide_squelch): per block and channel, the band power around the channel's frequency word in
// the block's own spectrum plane against the source's levels, with hysteresis and a hang time.  The words are core::squelch_bin, squelch_band, squelch_level
// and squelch_step's (detail/core.h: the host form gives the same words).  The squelched instantiations of tune_kernel, tune2_kernel and resample_kernel read
// the state word this kernel leaves (SquelchIn, squelch_zero: csrc/m17_wide_kernels.hpp) and, where the channel is closed, store zeros and return before they
// mix a sample.  gfx950 / CDNA4, wave64.
#pragma once

#include "m17_common.hpp"
#include "m17_wide_kernels.hpp"

namespace m17 {

constexpr int SQUELCH_THREADS = 64;

// A lane per channel.  Channel c listens to source table[c] at the frequency word table[maxC + c]; plane[S][N] is the block's spectrum of J frames;
// levels[S] are the sources' open levels and levels[S + s] their close levels.  hold[c] is the channel's count in front of this block (the host zeroes the
// whole array in front of the first block after m17hip_wide_squelch or m17hip_demod_reset).  Writes hold[c], state[c] = h' | open << 31 and band[c].  Vector stores only, no
// atomics.
__global__ __launch_bounds__(SQUELCH_THREADS) void wide_squelch_kernel(const float* __restrict__ plane, uint32_t logn, uint32_t J,
                                                                       const uint32_t* __restrict__ table, uint32_t maxC, const float* __restrict__ levels,
                                                                       uint32_t S, uint32_t B, uint32_t hang, uint32_t* __restrict__ hold,
                                                                       uint32_t* __restrict__ state, float* __restrict__ band, uint32_t C)
{
    const uint32_t c = blockIdx.x * SQUELCH_THREADS + threadIdx.x;
    if (c >= C) return;
    const uint32_t s = table[c], N = 1u << logn;
    const uint32_t k = core::squelch_bin((int32_t)table[maxC + c], logn);
    const float b = core::squelch_band(plane + (size_t)s * N, N, k, B);
    const uint32_t h = hold[c];
    const uint32_t word = core::squelch_step(h, b, core::squelch_level(levels[s], J), core::squelch_level(levels[S + s], J), hang, J);
    hold[c] = word & ~core::SQUELCH_OPEN;
    state[c] = word;
    band[c] = b;
}

}  // namespace m17
