// K-1p: the source spectrum beside whichever kernel a wideband configuration launches (m17hip_wide_spectrum): per SOURCE and bin, the power of the windowed
// N-point FFT of the source block's frames, summed over the block.  Frame f starts at block sample first + f hop (core::spec_frames: where the feed's sample
// index is a multiple of hop); the window is core::spec_window, the FFT core::spec_item1 / spec_item2 over a bit-reversed load, the power core::chan_power,
// and the sum has the survey's two levels (core::CHAN_SURVEY_GROUP = 16 frames per group, plain float adds from +0 in ascending order): spectrum_kernel
// leaves a group's sums in a scratch array, chan_survey_sum_kernel (csrc/m17_chan_survey_kernels.hpp, as it stands) adds the groups.  It reads src only.
// Vector stores only, no atomics.  gfx950 / CDNA4, wave64.
//
// THE WORKGROUP is four waves and keeps F frames of N float2 in LDS beside the N / 2 twiddles.  A frame of N points has N / 2 butterflies per stage and
// N / 4 items per two-stage pass: at N = 4096 that is four items a lane and pass, at N = 64 a quarter of ONE wave, so small N takes several frames of its
// group per pass — F = SPECTRUM_PASS_POINTS / N, at most the group's 16 — and every lane has an item.  Each lane keeps the sums of its bins k = tid + 256 m in
// registers across the passes and adds frame after frame to them, so the add order is the definition's whatever F is.
// LDS: 8 F N + 4 N bytes — 8.4 KB at 64, 16.5 to 20 KB from 128 to 1024 (eight workgroups on a CU's 160 KB: all its wave slots), 24 KB at 2048, 48 KB at
// 4096 (three workgroups: twelve waves hide the eight barriers of a pass).  What hides a pass's barriers is the OTHER workgroups on the CU, as
// m17_chan_survey_kernels.hpp found for its sub-tile, so F N is kept at 2048 points rather than at what 64 KB would hold; NOTES.md has what was measured.
// THE LOAD puts sample i of a frame at v[bitrev(i)].  Lanes that take consecutive i write N / 2 float2 apart — one bank, 64 lanes deep; lanes that take
// consecutive bitrev(i) read 64 separate lines.  spectrum_load_index splits a wave's six lane bits: three are i's lowest (eight consecutive samples, a
// 32-byte run of int16 pairs), three are i's highest (eight consecutive float2 of LDS), so a store is eight deep in place of 64.
#pragma once

#include "m17_chan_survey_kernels.hpp"

namespace m17 {

constexpr int SPECTRUM_THREADS = 256;
#ifndef M17_SPECTRUM_PASS_POINTS
#define M17_SPECTRUM_PASS_POINTS 2048
#endif
constexpr uint32_t SPECTRUM_PASS_POINTS = M17_SPECTRUM_PASS_POINTS;   // F N: points of all the frames a pass holds (one frame is always taken)
__host__ __device__ inline uint32_t spectrum_frames_per_pass(uint32_t N)
{
    const uint32_t f = SPECTRUM_PASS_POINTS / N;
    return f < 1 ? 1 : f > core::CHAN_SURVEY_GROUP ? core::CHAN_SURVEY_GROUP : f;
}
__host__ __device__ inline size_t spectrum_lds_bytes(uint32_t N, uint32_t F) { return ((size_t)F * N + N / 2) * sizeof(float2); }
// The sample of a frame that item q < N of the load takes (a bijection of [0, N), logn >= 6): q's bits 0..2 are i's, q's bits 3..5 are i's highest three,
// the rest of q goes in between.
__host__ __device__ inline uint32_t spectrum_load_index(uint32_t q, uint32_t logn)
{
    return (q & 7u) | ((q >> 6) << 3) | (((q >> 3) & 7u) << (logn - 3));
}

// Grid (groups of 16 frames, sources); frame j of the block starts at its sample first + j hop, j < J, and first + (J - 1) hop + N <= W.  A group goes
// through passes of F frames:
// 1. Load, window and bit-reversed store of the pass's frames in one sweep; the twiddles go beside them once.
// 2. The FFT's stages in ascending order between barriers: stage 1 alone where logn is odd, then two stages per sweep (core::spec_item2).
// 3. Lane tid adds the powers of its bins, frame ascending, to the sums it keeps; after the last pass the group's sums go to scratch[source][group][k].
// window: [N]; tw: [N / 2].
template <typename IQT>
__global__ __launch_bounds__(SPECTRUM_THREADS) void spectrum_kernel(const IQT* __restrict__ src, size_t spitch, const float* __restrict__ window,
                                                                    const float2* __restrict__ tw, uint32_t logn, uint32_t hop, uint32_t first, uint32_t J,
                                                                    uint32_t F, float* __restrict__ scratch)
{
    extern __shared__ float2 spectrum_lds[];
    const uint32_t N = 1u << logn, s = blockIdx.y, grp = blockIdx.x, tid = threadIdx.x;
    const uint32_t j0 = grp * core::CHAN_SURVEY_GROUP, nj = J - j0 < core::CHAN_SURVEY_GROUP ? J - j0 : core::CHAN_SURVEY_GROUP;   // (j0 < J)
    float2* twl = spectrum_lds;
    float2* v = twl + N / 2;
    const IQT* row = src + (size_t)s * spitch;
    for (uint32_t a = tid; a < N / 2; a += SPECTRUM_THREADS) twl[a] = tw[a];
    float acc[4096 / SPECTRUM_THREADS];
#pragma unroll
    for (uint32_t m = 0; m < 4096 / SPECTRUM_THREADS; ++m) acc[m] = 0.0f;
    for (uint32_t q0 = 0; q0 < nj; q0 += F) {
        const uint32_t nf = nj - q0 < F ? nj - q0 : F;
        for (uint32_t it = tid; it < (nf << logn); it += SPECTRUM_THREADS) {
            const uint32_t f = it >> logn, i = spectrum_load_index(it & (N - 1), logn);
            const float2 x = iq_float(row[(size_t)first + (size_t)(j0 + q0 + f) * hop + i]);
            float2 y;
            core::spec_window(window[i], x.x, x.y, y.x, y.y);
            v[(f << logn) + core::spec_bitrev(i, logn)] = y;
        }
        __syncthreads();
        uint32_t st = 1;
        if (logn & 1u) {
            for (uint32_t it = tid; it < (nf << (logn - 1)); it += SPECTRUM_THREADS)
                core::spec_item1(reinterpret_cast<float*>(v + ((it >> (logn - 1)) << logn)), reinterpret_cast<const float*>(twl), logn, 1, it & (N / 2 - 1));
            __syncthreads();
            st = 2;
        }
        for (; st < logn; st += 2) {
            for (uint32_t it = tid; it < (nf << (logn - 2)); it += SPECTRUM_THREADS)
                core::spec_item2(reinterpret_cast<float*>(v + ((it >> (logn - 2)) << logn)), reinterpret_cast<const float*>(twl), logn, st, it & (N / 4 - 1));
            __syncthreads();
        }
#pragma unroll
        for (uint32_t m = 0; m < 4096 / SPECTRUM_THREADS; ++m) {
            const uint32_t k = tid + m * SPECTRUM_THREADS;
            if (k < N)
                for (uint32_t f = 0; f < nf; ++f) { const float2 z = v[(f << logn) + k]; acc[m] = acc[m] + core::chan_power(z.x, z.y); }
        }
        __syncthreads();   // (the next pass's load writes v)
    }
#pragma unroll
    for (uint32_t m = 0; m < 4096 / SPECTRUM_THREADS; ++m) {
        const uint32_t k = tid + m * SPECTRUM_THREADS;
        if (k < N) scratch[(((size_t)s * gridDim.x + grp) << logn) + k] = acc[m];
    }
}

}  // namespace m17
