// K-1 with a resampling second stage (m17hip_wide_resample): the tuner for sources whose rate is no integer multiple of 48 kSPS — 48000 R1 D / U samples per
// second, U <= D coprime (2.048 MSPS is R1 = 16, U / D = 3 / 8).  Per channel, mix its source to the channel's offset, low-pass with taps1 and keep every
// R1-th sample (u) as tune2_kernel does, then resample the u by U / D through taps2 and discriminate:
//   N_n = n D + D - 1,  i0 = N_n mod U,  b = N_n div U,  z[n] = sum_{j : i0 + U j < L2} taps2[i0 + U j] u[b - j],  y[n] = gain * arg(z[n] conj(z[n-1]))
// into the rows of the context's FLOAT input slab.  The arithmetic is core::ddc_mix, ddc_tap and fm_discriminate (detail/core.h: core::ddc_resample is the host
// form of the same words; at U = 1 they are tune2_kernel's).  tune2_kernel, wide_chains, wide_carry_kernel and wide_hist_kernel stay as they are; the last two
// run behind this kernel as they run behind the tuners.  gfx950 / CDNA4, wave64.
#pragma once

#include "m17_wide2_kernels.hpp"

namespace m17 {

// THE TILE.  A block holds a multiple of U outputs; a GROUP is U consecutive outputs n = U t + r, r < U, over D new u.  Output U t + r reads u from
// b = t D + c_r down, c_r = ((r + 1) D - 1) div U < D, with the taps i0_r + U j, i0_r = ((r + 1) D - 1) mod U: a residue class r is an integer decimator by
// D over the u with a sub-filter of at most J2 = ceil(L2 / U) taps.  A tile is G groups.  Its LDS in float2:
//   1 + D (G + JD)   one place of padding, then D planes of G + JD u, JD = ceil(J2 / D): tune2's polyphase image over D, with JD groups of u in front of
//                    the tile's own (the sub-filters' history, recomputed per tile as in tune2)
//   G U + 1          the tile's z: the one in front of its first output and one per output
//   R1 (4 Q + J1 - 1)  one chunk of stage 1, as in tune2: Q u per chain, J1 = ceil(L1 / R1)
// Q(G) is the most that fits WIDE2_LDS beside the first two, and WIDE_THREADS at the most.  THE RULE: G is the value in 1 .. 255 with Q(G) >= 1 that makes
// (G + JD) / (G Q(G)) smallest — the u made per output times the share of the wave stage 1 leaves idle — and of equal ones the smallest; compared exactly, as
// (G + JD) G' Q(G') < (G' + JD) G Q(G) in 64 bits.  255 groups and 64 u per chain at 2.048 MSPS with the default taps (16 x 3 / 8: 55.6 KB); at the limits
// (R1 = 16, L1 = 256, D = 125, L2 = 4096) G = 13, Q = 34 at U = 1 and G = 22, Q = 64 at U = 32.  EVERY accepted configuration has a G: the planes of G = 1
// hold D (1 + JD) < J2 + 2 D <= 4346 u, the z at most 33 and a chunk of Q = 1 at most 16 * 19 = 304 mixed samples, of the 8192.
__host__ __device__ inline uint32_t resample_q(uint32_t L1, uint32_t R1, uint32_t L2, uint32_t U, uint32_t D, uint32_t G)
{
    const uint32_t JD = wide2_j(wide2_j(L2, U), D), J1 = wide2_j(L1, R1);
    const uint32_t fixed = 1 + D * (G + JD) + G * U + 1, room = WIDE2_LDS / (uint32_t)sizeof(float2);
    if (fixed >= room) return 0;
    const uint32_t places = (room - fixed) / R1;
    if (places + 1 < J1 + WIDE_PER_LANE) return 0;
    const uint32_t q = (places + 1 - J1) / WIDE_PER_LANE;
    return q < (uint32_t)WIDE_THREADS ? q : (uint32_t)WIDE_THREADS;
}
inline uint32_t resample_groups(uint32_t L1, uint32_t R1, uint32_t L2, uint32_t U, uint32_t D)
{
    const uint64_t JD = wide2_j(wide2_j(L2, U), D);
    uint32_t best = 1;
    uint64_t bq = resample_q(L1, R1, L2, U, D, 1);
    for (uint32_t G = 2; G < (uint32_t)WIDE_Z; ++G) {
        const uint64_t q = resample_q(L1, R1, L2, U, D, G);
        if (!q) break;   // (Q falls as G grows)
        if ((G + JD) * best * bq < (best + JD) * G * q) { best = G; bq = q; }
    }
    return best;
}
__host__ __device__ inline size_t resample_lds_bytes(uint32_t L1, uint32_t R1, uint32_t L2, uint32_t U, uint32_t D, uint32_t G, uint32_t Q)
{
    const uint32_t JD = wide2_j(wide2_j(L2, U), D);
    return ((size_t)1 + (size_t)D * (G + JD) + (size_t)G * U + 1 + (size_t)R1 * (WIDE_PER_LANE * Q + wide2_j(L1, R1) - 1)) * sizeof(float2);
}

// One residue class over the u planes: chain q of the lane is number k = lane + 64 q of the class (group k - 1 of the tile; k = 0 is the group in front of
// it), summed from +0 in the order j = 0, 1, ... with tap i0 + U j against u c - j of its group: plane (c - j) mod D at place k - 1 + JD + floor((c - j) / D).
// `base` is plane 0 at the lane's place JD - 1 of chain 0.  All lanes read ONE plane at consecutive places, as in wide_chains; the taps are scalar loads at
// stride U, WIDE_TAPS at a time.  NQ chains; FULL: every k < 64 NQ is one of the tile (no index is clamped and the chains' distance is a constant the
// compiler can pair reads over), else the last chain's k is clamped to `kmax` — its lanes behind that read a place that exists and their sums are dropped.
template <int NQ, bool FULL>
__device__ __forceinline__ void resample_chains(const float2* base, uint32_t lane, uint32_t kmax, uint32_t P, uint32_t D, uint32_t c, const float* __restrict__ taps,
                                                uint32_t i0, uint32_t U, uint32_t L, float2 (&z)[WIDE_PER_LANE])
{
    const uint32_t klast = (NQ - 1) * WIDE_THREADS + lane;
    const int32_t last = FULL ? (NQ - 1) * WIDE_THREADS : (int32_t)(klast < kmax ? klast : kmax) - (int32_t)lane;   // chain NQ - 1's distance from chain 0
#pragma unroll
    for (int q = 0; q < NQ; ++q) z[q] = make_float2(0.0f, 0.0f);
    uint32_t plane = c, row = 0;
    int32_t off = (int32_t)(c * P);   // off = plane * P - row: the places go down as j goes up
    auto step = [&](float t) {
        const float2* p = base + off;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float2 v = p[q == NQ - 1 ? last : q * WIDE_THREADS];
            core::ddc_tap(t, v.x, v.y, z[q].x, z[q].y);
        }
        if (plane == 0) { plane = D - 1; ++row; off = (int32_t)((D - 1) * P) - (int32_t)row; }
        else { --plane; off -= (int32_t)P; }
    };
    uint32_t i = i0;
    for (; L > (WIDE_TAPS - 1) * U && i < L - (WIDE_TAPS - 1) * U; i += WIDE_TAPS * U) {
        float t[WIDE_TAPS];
#pragma unroll
        for (int k = 0; k < WIDE_TAPS; ++k) t[k] = taps[i + k * U];
#pragma unroll
        for (int k = 0; k < WIDE_TAPS; ++k) step(t[k]);
    }
    for (; i < L; i += U) step(taps[i]);
}

// Grid (tiles of G groups, channels), one wave per workgroup, the workgroups in tune2_kernel's order.  T, the block's outputs, is a multiple of U.  With g0
// the tile's first group and w the number of a z of the tile (z w is output g0 U + w - 1; w = 0 is the z in front of the tile):
// 1. Stage 1 is tune2_kernel's: u number e of the tile (e = 0 is u (g0 - JD) D of the block) goes to plane e % D at place e / D, made in chunks of 4 Q
//    consecutive u from (4 Q + J1 - 1) R1 mixed samples with the loads grouped.  Sample k of the block: k < 0 the source's carried history of
//    H = (J2 - 1) R1 + L1 - 1 converted samples; below that and behind the row's end zero, which no stored output reads; phase fcw * (count + k).  Only the u
//    under the groups that the block holds are made.
// 2. Stage 2 goes through the residue classes one after another, the lanes over the groups (resample_chains): z of class r and number k is z w =
//    r + 1 + U (k - 1) of the tile, kept for w = 0 .. the tile's outputs — k = 0 is the z in front of the tile for r = U - 1 and nothing for the others (it
//    reads the place in front of its plane: the padding in front of plane 0) — and stored to the z buffer; the block's output 0 has the channel's carry in
//    front, a later tile recomputes the z in front of it.
// 3. Output n = g0 U + w - 1 is z w against z w - 1, lanes over consecutive w; the block's last z goes to znew[c] for wide_carry_kernel.
// Samples are read one by one (a sample is aligned to its own size, nothing more is asked of the rows); vector stores only, no atomics.  Every z is the same
// chain whatever G and Q are: the result does not depend on the tile rule.
// METER, SQUELCH: as tune_kernel's (a closed workgroup's tile is its groups' outputs).
template <typename IQT, bool METER = false, bool SQUELCH = false, typename... PW>
__global__ __launch_bounds__(WIDE_THREADS) void resample_kernel(const IQT* __restrict__ src, size_t spitch, uint32_t W, const float2* __restrict__ hist,
                                                                const float* __restrict__ taps1, uint32_t L1, uint32_t R1, const float* __restrict__ taps2,
                                                                uint32_t L2, uint32_t U, uint32_t D, uint32_t G, uint32_t Q,
                                                                const uint32_t* __restrict__ table, uint32_t maxC, uint32_t count, float* __restrict__ dst,
                                                                size_t dpitch, uint32_t T, const float2* __restrict__ carry, float2* __restrict__ znew, float gain,
                                                                PW... pw)
{
    extern __shared__ float2 resample_lds[];
    const uint32_t lane = threadIdx.x;
    const uint64_t wg = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const uint32_t c = (uint32_t)(wg % gridDim.y), g0 = (uint32_t)(wg / gridDim.y) * G;
    if constexpr (SQUELCH) {
        if (squelch_closed(c, (uint32_t)(wg / gridDim.y), pw...)) {
            squelch_zero(c, g0 * U, (T / U - g0 < G ? T / U : g0 + G) * U, T, dst + (size_t)c * dpitch + XPRE, znew, pw...);
            return;
        }
    }
    const uint32_t s = table[c], fcw = table[maxC + c];
    const uint32_t J1 = wide2_j(L1, R1), J2 = wide2_j(L2, U), JD = wide2_j(J2, D), P2 = G + JD, K = WIDE_PER_LANE * Q, P1 = K + J1 - 1;
    const uint32_t H = (J2 - 1) * R1 + L1 - 1;
    float2* uplanes = resample_lds + 1;
    float2* zbuf = uplanes + (size_t)D * P2;
    float2* chunk = zbuf + (size_t)G * U + 1;
    const IQT* row = src + (size_t)s * spitch;
    const float2* hs = hist + (size_t)s * H;
    const uint32_t groups = T / U - g0 < G ? T / U - g0 : G;   // the tile's groups that the block holds
    const uint32_t NU = (groups + JD) * D;                     // the u under them: <= D P2
    const int64_t p0 = ((int64_t)g0 - (int64_t)JD) * D;        // the block's number of the tile's u 0
    const uint32_t plane0 = lane % R1, place0 = lane / R1, dplane = WIDE_THREADS % R1, dplace = WIDE_THREADS / R1;
    if (lane == 0) resample_lds[0] = make_float2(0.0f, 0.0f);
    for (uint32_t e0 = 0; e0 < NU; e0 += K) {
        // chunk sample v (plane v % R1, place v / R1) is sample kc + v of the block: u e0 + e reads plane R1 - 1 - rho at place e + J1 - 1 - j
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
                if (e < NU) uplanes[(e % D) * P2 + e / D] = u[q];
            }
        }
        __syncthreads();   // (the next chunk's samples overwrite these; behind the last chunk: the u planes are whole)
    }
    const uint32_t wmax = groups * U;                           // the tile's last z that an output of the block reads
    const uint32_t NQ = groups / WIDE_THREADS + 1;              // chains that hold a number k <= groups
    const float2* base = uplanes + (JD - 1) + lane;             // (k = 0, JD = 1, j beyond c: one place in front of the plane)
    for (uint32_t r = 0; r < U; ++r) {
        const uint32_t N = (r + 1) * D - 1, cr = N / U, i0 = N % U;
        float2 z[WIDE_PER_LANE];
        if (groups == (uint32_t)WIDE_Z - 1) resample_chains<4, true>(base, lane, groups, P2, D, cr, taps2, i0, U, L2, z);
        else if (NQ == 4) resample_chains<4, false>(base, lane, groups, P2, D, cr, taps2, i0, U, L2, z);
        else if (NQ == 3) resample_chains<3, false>(base, lane, groups, P2, D, cr, taps2, i0, U, L2, z);
        else if (NQ == 2) resample_chains<2, false>(base, lane, groups, P2, D, cr, taps2, i0, U, L2, z);
        else resample_chains<1, false>(base, lane, groups, P2, D, cr, taps2, i0, U, L2, z);
#pragma unroll
        for (int q = 0; q < WIDE_PER_LANE; ++q) {
            const uint32_t k = lane + q * WIDE_THREADS;
            if ((uint32_t)q >= NQ || k > groups) continue;
            if (k == 0) { if (r == U - 1) zbuf[0] = g0 == 0 ? carry[c] : z[q]; }
            else zbuf[r + 1 + U * (k - 1)] = z[q];
        }
    }
    __syncthreads();
    float* d = dst + (size_t)c * dpitch + XPRE;
    for (uint32_t w = 1 + lane; w <= wmax; w += WIDE_THREADS) {
        const uint32_t n = g0 * U + w - 1;
        const float2 a = zbuf[w], b = zbuf[w - 1];
        d[n] = core::fm_discriminate(a.x, a.y, b.x, b.y, gain);
        if constexpr (METER) meter_put(c, n, a, pw...);
        if (n == T - 1) znew[c] = a;
    }
}

}  // namespace m17
