// K-1s: the raster survey beside the channeliser (m17hip_wide_survey): per SOURCE and bin, the power of the channeliser's z summed over the block's survey
// times — output n of a block that began at output N0 of the feed is one iff (N0 + n + 1) % stride == 0.  z is chan_kernel's word (core::chan_fold,
// chan_pass1, chan_pass2 over the same history, count and twiddles), whoever listens; the power is core::chan_power, and the sum has two levels
// (core::CHAN_SURVEY_GROUP = 16 times per group, both levels plain float adds from +0 in ascending order): chan_survey_kernel leaves a group's sums in a
// scratch array, chan_survey_sum_kernel adds the groups.  Vector stores only, no atomics.  gfx950 / CDNA4, wave64.
//
// THE WORKGROUP is four waves, not chan_kernel's sixteen.  chan_kernel has TT M items per pass with TT up to 31 and fills 64 KB of LDS, so sixteen waves
// have work and two workgroups fill a CU's wave slots.  Here a survey time needs a window of L samples of its own once stride * decim >= L (the usual case:
// stride 48 at decim 50 against 1601 taps), so LDS buys few times per sub-tile and a pass has only TS M items: 1024 threads would idle most of the time and
// still hold the CU's slots.  With 256 threads a lane has about one item per time and pass, and the sum step is exactly one lane per bin (M <= 256).
// THE SUB-TILE is sized to 32 KB, not to the 64 KB a workgroup may have: what hides a pass's latencies and its five barriers here is OTHER workgroups on the
// CU, and LDS decides how many there are.  At 192 bins / 1601 taps / stride 48 that is ONE time per sub-tile (17 432 bytes: eight workgroups, all 32 wave
// slots of a CU); measured against larger budgets in one call, 64 sources x 1000 times: 0.378 ms at 32 KB, 0.474 ms at 48 KB (two times), 0.722 ms at 64 KB
// (four times) — NOTES.md.  At the limits (M 256, 4096 taps) one time needs 38 928 bytes and is taken whatever the budget; small shapes get all 16 times of
// a group at once.
#pragma once

#include "m17_chan_kernels.hpp"

namespace m17 {

constexpr int SURVEY_THREADS = 256;
constexpr uint32_t SURVEY_LDS_TARGET = 32768;   // LDS a sub-tile is sized to; one time is always taken, whatever it needs (38 928 bytes at the limits)
// Samples between the windows of consecutive survey times in LDS: stride * R where they overlap (one run of samples serves all), L where they are disjoint.
__host__ __device__ inline uint32_t survey_wpitch(uint32_t L, uint32_t R, uint32_t stride)
{
    const uint64_t sr = (uint64_t)stride * R;
    return sr < L ? (uint32_t)sr : L;
}
// The sub-tile's LDS in float2: (TS - 1) WP + L converted samples, the M twiddles and two planes of TS rows of M | 1 (chan_kernel's odd pitch) — the partial
// sums, later the powers (one float each), and the first pass's sums.
__host__ __device__ inline size_t survey_lds_bytes(uint32_t L, uint32_t WP, uint32_t M, uint32_t TS)
{
    return ((size_t)(TS - 1) * WP + L + M + 2 * (size_t)TS * chan_pitch(M)) * sizeof(float2);
}
__host__ __device__ inline uint32_t survey_tile(uint32_t L, uint32_t WP, uint32_t M)
{
    uint32_t TS = 1;
    while (TS < core::CHAN_SURVEY_GROUP && survey_lds_bytes(L, WP, M, TS + 1) <= SURVEY_LDS_TARGET) ++TS;
    return TS;
}

// Grid (groups of 16 survey times, sources); survey time j of the block is its output first + j stride, j < J.  A group goes through sub-tiles of TS times:
// 1. The sub-tile's converted samples go to LDS: the window of time q begins at q WP, its newest sample at q WP + L - 1 (the block's sample (t + 1) R - 1;
//    below 0 the source's carried history, as in chan_kernel).  The twiddles go beside them once.
// 2. The fold and 3. pass 1: chan_kernel's items and lane orders, a row per time.
// 4. Pass 2 for ALL M bins, an item per (bin, time) with the time fastest; the power goes into the plane the partial sums have left, a float per item.
// 5. Lane k adds bin k's powers of the sub-tile, time ascending, to the sum it keeps in a register across sub-tiles; the group's sum goes to
//    scratch[source][group][k].
// `cm` as in chan_kernel.
template <typename IQT>
__global__ __launch_bounds__(SURVEY_THREADS) void chan_survey_kernel(const IQT* __restrict__ src, size_t spitch, uint32_t W, const float2* __restrict__ hist,
                                                                     const float* __restrict__ taps, uint32_t L, uint32_t R, uint32_t M1, uint32_t M2,
                                                                     const float2* __restrict__ tw, uint32_t cm, uint32_t first, uint32_t stride, uint32_t J,
                                                                     uint32_t WP, uint32_t TS, float* __restrict__ scratch)
{
    extern __shared__ float2 survey_lds[];
    const uint32_t s = blockIdx.y, grp = blockIdx.x, tid = threadIdx.x, M = M1 * M2, H = L - 1, MP = chan_pitch(M);
    const uint32_t j0 = grp * core::CHAN_SURVEY_GROUP, nj = J - j0 < core::CHAN_SURVEY_GROUP ? J - j0 : core::CHAN_SURVEY_GROUP;   // (j0 < J)
    float2* xs = survey_lds;
    float2* twl = xs + (size_t)(TS - 1) * WP + L;
    float2* wz = twl + M;
    float2* ab = wz + (size_t)TS * MP;
    float* pw = reinterpret_cast<float*>(wz);
    const IQT* row = src + (size_t)s * spitch;
    const float2* hs = hist + (size_t)s * H;
    for (uint32_t a = tid; a < M; a += SURVEY_THREADS) twl[a] = tw[a];
    float acc = 0.0f;
    for (uint32_t q0 = 0; q0 < nj; q0 += TS) {
        const uint32_t ts = nj - q0 < TS ? nj - q0 : TS;
        const uint64_t n1 = (uint64_t)first + (uint64_t)(j0 + q0) * stride + 1;   // the sub-tile's first time, + 1
        const uint32_t NX = (ts - 1) * WP + L;
#pragma unroll 4
        for (uint32_t a = tid; a < NX; a += SURVEY_THREADS) {
            uint32_t q = 0, off = a;
            if (WP == L) { q = a / L; off = a - q * L; }   // (disjoint windows: each its own L samples)
            const int64_t k = (int64_t)((n1 + (uint64_t)q * stride) * R) - (int64_t)L + off;
            float2 v = make_float2(0.0f, 0.0f);
            if (k >= 0) { if (k < (int64_t)W) v = iq_float(row[k]); }
            else if (k >= -(int64_t)H) v = hs[(int64_t)H + k];
            xs[a] = v;
        }
        __syncthreads();
        for (uint32_t it = tid; it < ts * M; it += SURVEY_THREADS) {
            const uint32_t g = it / M, r = it - g * M;
            const uint32_t i0 = (uint32_t)(((n1 + (uint64_t)g * stride) * R + (uint64_t)cm + 2 * M - 1 - r) % M);
            float2 w;
            core::chan_fold(taps, L, M, i0, reinterpret_cast<const float*>(xs + (size_t)g * WP + L - 1), w.x, w.y);
            wz[g * MP + r] = w;
        }
        __syncthreads();
        for (uint32_t it = tid; it < ts * M; it += SURVEY_THREADS) {
            const uint32_t g = it / M, e = it - g * M, k2 = e / M1, r1 = e - k2 * M1;
            float2 a;
            core::chan_pass1(reinterpret_cast<const float*>(wz + g * MP), M1, M2, reinterpret_cast<const float*>(twl), r1, k2, a.x, a.y);
            ab[g * MP + r1 * M2 + k2] = a;
        }
        __syncthreads();
        for (uint32_t it = tid; it < ts * M; it += SURVEY_THREADS) {
            const uint32_t k = it / ts, g = it - k * ts;
            float2 z;
            core::chan_pass2(reinterpret_cast<const float*>(ab + g * MP), M1, M2, reinterpret_cast<const float*>(twl), k, z.x, z.y);
            pw[k * TS + g] = core::chan_power(z.x, z.y);
        }
        __syncthreads();
        if (tid < M)
            for (uint32_t g = 0; g < ts; ++g) acc = acc + pw[tid * TS + g];
        // (the next sub-tile writes xs, which nothing has read since the fold, and pw only behind its own first barrier)
    }
    if (tid < M) scratch[((size_t)s * gridDim.x + grp) * M + tid] = acc;
}

// A lane per (source, bin): the groups' sums added in ascending order from +0 (G == 0: +0).
__global__ __launch_bounds__(256) void chan_survey_sum_kernel(const float* __restrict__ scratch, uint32_t G, uint32_t M, uint32_t S, float* __restrict__ plane)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * M) return;
    const uint32_t s = i / M, k = i - s * M;
    float acc = 0.0f;
    for (uint32_t g = 0; g < G; ++g) acc = acc + scratch[((size_t)s * G + g) * M + k];
    plane[i] = acc;
}

}  // namespace m17
