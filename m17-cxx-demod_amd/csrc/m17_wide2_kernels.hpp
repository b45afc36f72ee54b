// K-1 in two stages (m17hip_wide_config2): the tuner for sources above 16 x 48 kSPS.  Per channel, mix its source to the channel's offset, low-pass with taps1
// and keep every R1-th sample (u), low-pass the u with taps2, keep every R2-th (z) and discriminate:
//   u[p] = sum_i taps1[i] mixed[p R1 + R1 - 1 - i],  z[n] = sum_i taps2[i] u[n R2 + R2 - 1 - i],  y[n] = gain * arg(z[n] conj(z[n-1]))
// into the rows of the context's FLOAT input slab.  The arithmetic is core::ddc_mix, ddc_tap and fm_discriminate (detail/core.h: core::ddc_fir2 is the host
// form of the same words).  tune_kernel, wide_carry_kernel and wide_hist_kernel (m17_wide_kernels.hpp) stay as they are; the last two run behind this kernel
// as they run behind tune_kernel.  gfx950 / CDNA4, wave64.
#pragma once

#include "m17_wide_kernels.hpp"

namespace m17 {

constexpr uint32_t WIDE2_LDS = 65536;   // dynamic LDS a launch may ask for with no attribute raised, in bytes
constexpr int WIDE2_GROUP = 16;         // samples per lane whose loads are in flight together while a chunk is filled
// the tile's LDS in float2: R2 planes of WIDE_TILE + J2 u (J2 = ceil(L2 / R2)), the tile's z, and one CHUNK of stage 1: R1 planes of 4 Q + J1 - 1 mixed
// samples (J1 = ceil(L1 / R1)) under 4 Q consecutive u.  Q, the u per chain of a chunk, is WIDE_THREADS where that fits — 34.7 KB at 10 x 5 with the default
// taps — and otherwise the most that does: 40 at R1 = R2 = 16, L1 = 256, L2 = 1024, the smallest there is.
__host__ __device__ inline uint32_t wide2_j(uint32_t L, uint32_t R) { return (L + R - 1) / R; }
__host__ __device__ inline uint32_t wide2_q(uint32_t L1, uint32_t R1, uint32_t L2, uint32_t R2)
{
    const uint32_t fixed = R2 * (WIDE_TILE + wide2_j(L2, R2)) + WIDE_Z;                       // <= 5360
    const uint32_t places = (WIDE2_LDS / (uint32_t)sizeof(float2) - fixed) / R1;              // of one chunk plane: >= 177
    const uint32_t q = (places + 1 - wide2_j(L1, R1)) / WIDE_PER_LANE;
    return q < (uint32_t)WIDE_THREADS ? q : (uint32_t)WIDE_THREADS;
}
__host__ __device__ inline size_t wide2_lds_bytes(uint32_t L1, uint32_t R1, uint32_t L2, uint32_t R2)
{
    const uint32_t P1 = WIDE_PER_LANE * wide2_q(L1, R1, L2, R2) + wide2_j(L1, R1) - 1;
    return ((size_t)R2 * (WIDE_TILE + wide2_j(L2, R2)) + (size_t)R1 * P1 + WIDE_Z) * sizeof(float2);
}

// The filter of tune_kernel's step 2 over a polyphase image of R planes of P places: chain q of the lane sums, from +0 and in the order i = 0 .. L - 1,
// tap i = R j + rho against plane R - 1 - rho at place (lane + q stride) + J - 1 - j.  `base` is the image at the lane's place 0.  STRIDE: the chains'
// distance where the compiler may know it (it pairs the lane's four 8-byte reads into two ds_read2st64_b64 then), 0: `stride`.  All lanes read ONE plane at
// consecutive places per chain, whatever R is, so the bank argument of tune_kernel's comment holds for both stages; taps are scalar loads, WIDE_TAPS at a time.
template <int STRIDE>
__device__ __forceinline__ void wide_chains(const float2* base, uint32_t P, uint32_t R, uint32_t J, const float* __restrict__ taps, uint32_t L, uint32_t stride,
                                            float2 (&z)[WIDE_PER_LANE])
{
    const uint32_t sq = STRIDE ? (uint32_t)STRIDE : stride;
#pragma unroll
    for (int q = 0; q < WIDE_PER_LANE; ++q) z[q] = make_float2(0.0f, 0.0f);
    uint32_t off = (R - 1) * P + J - 1, rho = 0, jrow = J - 1;
    auto step = [&](float t) {
        const float2* p = base + off;
#pragma unroll
        for (int q = 0; q < WIDE_PER_LANE; ++q) {
            const float2 v = p[q * sq];
            core::ddc_tap(t, v.x, v.y, z[q].x, z[q].y);
        }
        if (++rho == R) { rho = 0; --jrow; off = (R - 1) * P + jrow; }
        else off -= P;
    };
    uint32_t i = 0;
    for (; i + WIDE_TAPS <= L; i += WIDE_TAPS) {
        float t[WIDE_TAPS];
#pragma unroll
        for (int k = 0; k < WIDE_TAPS; ++k) t[k] = taps[i + k];
#pragma unroll
        for (int k = 0; k < WIDE_TAPS; ++k) step(t[k]);
    }
    for (; i < L; ++i) step(taps[i]);
}

// Grid (tiles of WIDE_TILE outputs, channels), one wave per workgroup, as tune_kernel.  With w the number of a z of the tile (z w is output n0 + w - 1):
// 1. Stage 2 wants the u of the tile in polyphase order over R2: u number e of the tile (e = 0 is u (n0 - J2) R2 of the block) in plane e % R2 at e / R2 —
//    tune_kernel's image with u for mixed samples.  They do not fit beside their mixed samples at the larger configurations, so stage 1 makes them in CHUNKS
//    of 4 Q consecutive u: the chunk's (4 Q + J1 - 1) R1 mixed samples go into LDS once, in polyphase order over R1 (sample k of the block: k < 0 the source's
//    carried history of H = (L2 - 1) R1 + L1 - 1 converted samples; below that and behind the row's end zero, which no stored output reads; phase fcw *
//    (count + k)); lane l < Q runs the four chains of u number l, l + Q, l + 2 Q, l + 3 Q of the chunk and stores them into the u planes.  Only the u under
//    the z that an output of the block reads are made: the last chunk of a tile is partly filled as a rule.
// 2. Stage 2 is tune_kernel's step 2 over the u planes with (L2, R2), and 3. the z go through LDS into the discriminator as there: the block's output 0 has
//    the channel's carry in front, a later tile recomputes the z in front of it, the block's last z goes to znew[c] for wide_carry_kernel.
// Samples are read one by one (a sample is aligned to its own size, nothing more is asked of the rows); vector stores only, no atomics.
// METER, SQUELCH: as tune_kernel's.
template <typename IQT, bool METER = false, bool SQUELCH = false, typename... PW>
__global__ __launch_bounds__(WIDE_THREADS) void tune2_kernel(const IQT* __restrict__ src, size_t spitch, uint32_t W, const float2* __restrict__ hist,
                                                             const float* __restrict__ taps1, uint32_t L1, uint32_t R1, const float* __restrict__ taps2,
                                                             uint32_t L2, uint32_t R2, uint32_t Q, const uint32_t* __restrict__ table, uint32_t maxC,
                                                             uint32_t count, float* __restrict__ dst, size_t dpitch, uint32_t T,
                                                             const float2* __restrict__ carry, float2* __restrict__ znew, float gain, PW... pw)
{
    extern __shared__ float2 wide2_lds[];
    // the workgroups in launch order go through the CHANNELS of one tile before the next tile: those in flight together read the same stretch of the few
    // sources, which the caches then hold (channels slowest, each of them streams its whole source past the others')
    const uint32_t lane = threadIdx.x;
    const uint64_t wg = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const uint32_t c = (uint32_t)(wg % gridDim.y), n0 = (uint32_t)(wg / gridDim.y) * WIDE_TILE;
    if constexpr (SQUELCH) {
        if (squelch_closed(c, (uint32_t)(wg / gridDim.y), pw...)) {
            squelch_zero(c, n0, T - n0 < (uint32_t)WIDE_TILE ? T : n0 + WIDE_TILE, T, dst + (size_t)c * dpitch + XPRE, znew, pw...);
            return;
        }
    }
    const uint32_t s = table[c], fcw = table[maxC + c];
    const uint32_t J1 = wide2_j(L1, R1), J2 = wide2_j(L2, R2), P2 = WIDE_TILE + J2, K = WIDE_PER_LANE * Q, P1 = K + J1 - 1;
    const uint32_t H = (L2 - 1) * R1 + L1 - 1;
    float2* uplanes = wide2_lds;
    float2* chunk = uplanes + (size_t)R2 * P2;
    float2* zbuf = chunk + (size_t)R1 * P1;
    const IQT* row = src + (size_t)s * spitch;
    const float2* hs = hist + (size_t)s * H;
    const uint32_t wmax = T - n0 < (uint32_t)WIDE_TILE ? T - n0 : (uint32_t)WIDE_TILE;   // the tile's last z that an output of the block reads
    const uint32_t NU = (wmax + J2) * R2;                                                 // the u under z 0 .. wmax: <= R2 P2
    const int64_t p0 = ((int64_t)n0 - (int64_t)J2) * R2;                                  // the block's number of the tile's u 0
    const uint32_t plane0 = lane % R1, place0 = lane / R1, dplane = WIDE_THREADS % R1, dplace = WIDE_THREADS / R1;
    for (uint32_t e0 = 0; e0 < NU; e0 += K) {
        // chunk sample v (plane v % R1, place v / R1) is sample kc + v of the block: u e0 + e reads plane R1 - 1 - rho at place e + J1 - 1 - j
        // Lanes take CONSECUTIVE samples, WIDE2_GROUP x 64 at a time: where all of those lie inside the row (a condition the wave shares) their loads are
        // issued together and then mixed — with one load in flight per wave the fill waits for memory sample after sample, and a workgroup's LDS leaves
        // few other waves to fill the gaps.  Plane and place of a lane's sample advance by 64 % R1 and 64 / R1: no division.
        const int64_t kc = (p0 + (int64_t)e0 + 1 - (int64_t)J1) * R1;
        const uint32_t NV = R1 * ((NU - e0 < K ? NU - e0 : K) + J1 - 1);   // the samples under the chunk's u: the first places of every plane
        uint32_t plane = plane0, place = place0;
        for (uint32_t v0 = 0; v0 < NV; v0 += WIDE2_GROUP * WIDE_THREADS) {
            const int64_t kb = kc + (int64_t)v0;
            if (kb >= 0 && kb + (int64_t)(WIDE2_GROUP * WIDE_THREADS) <= (int64_t)W) {   // (loads behind the chunk's last sample stay inside the row; unused)
                const IQT* p = row + kb + lane;
                const uint32_t m0 = count + (uint32_t)kb + lane;
                IQT x[WIDE2_GROUP];
#pragma unroll
                for (int g = 0; g < WIDE2_GROUP; ++g) x[g] = p[g * WIDE_THREADS];
#pragma unroll
                for (int g = 0; g < WIDE2_GROUP; ++g) {
                    if (v0 + g * WIDE_THREADS + lane < NV) {
                        const float2 v = iq_float(x[g]);
                        float2 m;
                        core::ddc_mix(v.x, v.y, fcw, m0 + (uint32_t)(g * WIDE_THREADS), m.x, m.y);
                        chunk[plane * P1 + place] = m;
                    }
                    plane += dplane; place += dplace;
                    if (plane >= R1) { plane -= R1; ++place; }
                }
            } else {
                for (int g = 0; g < WIDE2_GROUP; ++g) {
                    if (v0 + g * WIDE_THREADS + lane < NV) {
                        const int64_t k = kb + g * WIDE_THREADS + lane;
                        float2 v = make_float2(0.0f, 0.0f);
                        if (k >= 0) { if (k < (int64_t)W) v = iq_float(row[k]); }
                        else if (k >= -(int64_t)H) v = hs[(int64_t)H + k];
                        float2 m;
                        core::ddc_mix(v.x, v.y, fcw, count + (uint32_t)k, m.x, m.y);
                        chunk[plane * P1 + place] = m;
                    }
                    plane += dplane; place += dplace;
                    if (plane >= R1) { plane -= R1; ++place; }
                }
            }
        }
        __syncthreads();
        if (lane < Q) {
            float2 u[WIDE_PER_LANE];
            if (Q == (uint32_t)WIDE_THREADS) wide_chains<WIDE_THREADS>(chunk + lane, P1, R1, J1, taps1, L1, Q, u);
            else wide_chains<0>(chunk + lane, P1, R1, J1, taps1, L1, Q, u);
#pragma unroll
            for (int q = 0; q < WIDE_PER_LANE; ++q) {
                const uint32_t e = e0 + lane + q * Q;
                if (e < NU) uplanes[(e % R2) * P2 + e / R2] = u[q];
            }
        }
        __syncthreads();   // (the next chunk's samples overwrite these; behind the last chunk: the u planes are whole)
    }
    float2 z[WIDE_PER_LANE];
    wide_chains<WIDE_THREADS>(uplanes + lane, P2, R2, J2, taps2, L2, WIDE_THREADS, z);
    if (n0 == 0 && lane == 0) z[0] = carry[c];
#pragma unroll
    for (int q = 0; q < WIDE_PER_LANE; ++q) zbuf[lane + q * WIDE_THREADS] = z[q];
    __syncthreads();
    float* d = dst + (size_t)c * dpitch + XPRE;
#pragma unroll
    for (int q = 0; q < WIDE_PER_LANE; ++q) {
        const uint32_t w = lane + q * WIDE_THREADS;
        if (w == 0) continue;
        const uint32_t n = n0 + w - 1;
        if (n >= T) continue;
        const float2 b = zbuf[w - 1];
        d[n] = core::fm_discriminate(z[q].x, z[q].y, b.x, b.y, gain);
        if constexpr (METER) meter_put(c, n, z[q], pw...);
        if (n == T - 1) znew[c] = z[q];
    }
}

}  // namespace m17
