// K-1c: the channeliser in front of the chain (wideband IQ input on a raster, m17hip_wide_raster): per SOURCE and output time, fold the taps over the
// source's samples into M partial sums, w[r] = sum_{i = i0, i0 + M, ...} h[i] x[m_n - i], and take the M-point DFT of them in two passes of small direct
// DFTs (M = M1 x M2), the second pass for the bins some channel listens to only; then discriminate, y[n] = gain * arg(z[n] conj(z[n-1])), into the rows of
// the context's FLOAT input slab.  Mixing and filtering are shared by all the channels of a source: nothing here is per channel but the last M1 steps and
// the store.  The arithmetic is core::chan_fold, chan_pass1, chan_pass2 and fm_discriminate (detail/core.h: the host form gives the same words).
// gfx950 / CDNA4, wave64.
#pragma once

#include "m17_common.hpp"
#include "m17_wide_kernels.hpp"

namespace m17 {

constexpr int CHAN_THREADS = 1024;            // sixteen waves per workgroup: the passes are latency-bound, and two workgroups of up to 64 KB fill a CU's waves
constexpr uint32_t CHAN_TILE_MAX = 31;        // outputs per tile at most (32 z with the one in front)
constexpr uint32_t CHAN_LDS_BYTES = 65536;    // LDS per workgroup at most
// The tile's LDS in float2: the TT R + L converted samples under TT + 1 output times, the M twiddles, and two planes of TT + 1 rows — the partial sums,
// later the z, and the first pass's sums.  A row is M | 1 float2: an odd pitch, so that lanes which differ in the output time alone (pass 2) read 64
// different banks where a pitch of 192 or 256 float2 would put them all on one.  TT is the largest tile that fits: 5 at the limits (R = 64, M = 256,
// L = 4096), 13 at 2.4 MSPS / 192 bins / 1601 taps.
__host__ __device__ inline uint32_t chan_pitch(uint32_t M) { return M | 1u; }
__host__ __device__ inline uint32_t chan_tile(uint32_t L, uint32_t R, uint32_t M)
{
    const uint32_t fit = (CHAN_LDS_BYTES / (uint32_t)sizeof(float2) - L - M - 2 * chan_pitch(M)) / (R + 2 * chan_pitch(M));
    return fit < CHAN_TILE_MAX ? fit : CHAN_TILE_MAX;
}
__host__ __device__ inline size_t chan_lds_bytes(uint32_t L, uint32_t R, uint32_t M, uint32_t TT)
{
    return ((size_t)TT * R + L + M + 2 * (size_t)(TT + 1) * chan_pitch(M)) * sizeof(float2);
}
// The channel table as the kernel reads it, S sources and P (bin, channel) pairs of which U distinct per source:
//   [0 .. S]            first pair of source s (word S: P)
//   [S + 1 .. 2 S + 1]  first distinct bin of source s (the last word: U)
//   then P pairs of two words (k = bin mod M, channel), then U words k.
__host__ __device__ inline size_t chan_table_words(uint32_t S, uint32_t P) { return 2 * ((size_t)S + 1) + 3 * (size_t)P; }

// Grid (tiles of TT outputs, sources); a source nobody listens to ends at once.  Output time g of the tile is output n0 + g - 1 of the block: g = 0 is the
// z in front of the tile's first output, recomputed (in front of the block's output 0 it is the channel's carry, read in step 5).
// 1. The tile's converted samples go to LDS once: sample a is the block's sample n0 R - L + a (below 0: the source's carried history of H = L - 1 samples;
//    below that and behind the row's end: zero, which no stored output reads).  The twiddles go beside them.
// 2. The fold, an item per (time, residue r): taps i0, i0 + M, ... with i0 = (count + k_n - r) mod M.  Across consecutive r the samples are consecutive
//    float2 in LDS (no bank conflict) and the taps a run of consecutive floats, descending (coalesced, from the cache).
// 3. Pass 1, an item per (time, k2, r1) with r1 fastest: sixteen lanes read consecutive partial sums against ONE twiddle (a broadcast; with k2 fastest
//    the twiddles' stride of M1 k2 float2 put a wave's reads on two banks).
// 4. Pass 2, an item per (distinct bin of the source, time) with the time fastest, the z into the plane the partial sums have left.
// 5. The store, an item per ((bin, channel) pair, time) with the time fastest, so a wave writes runs of TT consecutive floats; the block's last z goes to
//    znew[channel] (wide_carry_kernel follows, as behind the tuners).
// `cm` is the feed's sample count at the block's start mod M, taken by the host from all 64 bits.  Vector stores only, no atomics.
// METER: as tune_kernel's, per (bin, channel) pair: two channels on one bin get the same power.
template <typename IQT, bool METER = false, typename... PW>
__global__ __launch_bounds__(CHAN_THREADS) void chan_kernel(const IQT* __restrict__ src, size_t spitch, uint32_t W, const float2* __restrict__ hist,
                                                            const float* __restrict__ taps, uint32_t L, uint32_t R, uint32_t M1, uint32_t M2,
                                                            const float2* __restrict__ tw, const uint32_t* __restrict__ table, uint32_t S, uint32_t cm,
                                                            uint32_t TT, uint32_t C, float* __restrict__ dst, size_t dpitch, uint32_t T,
                                                            const float2* __restrict__ carry, float2* __restrict__ znew, float gain, PW... pw)
{
    extern __shared__ float2 chan_lds[];
    const uint32_t s = blockIdx.y, tid = threadIdx.x, n0 = blockIdx.x * TT, M = M1 * M2, H = L - 1;
    const uint32_t p0 = table[s], np = table[s + 1] - p0, u0 = table[S + 1 + s], nu = table[S + 2 + s] - u0;
    if (np == 0) return;
    const uint32_t* pairs = table + 2 * (S + 1) + 2 * (size_t)p0;
    const uint32_t* ubins = table + 2 * (S + 1) + 2 * (size_t)table[S] + u0;
    const uint32_t NX = TT * R + L, NW = TT + 1, MP = chan_pitch(M);
    const uint32_t nw = T - n0 + 1 < NW ? T - n0 + 1 : NW;   // output times of this tile (n0 < T)
    float2* xs = chan_lds;
    float2* twl = xs + NX;
    float2* wz = twl + M;
    float2* ab = wz + (size_t)NW * MP;
    const IQT* row = src + (size_t)s * spitch;
    const float2* hs = hist + (size_t)s * H;
    const int64_t kb = (int64_t)n0 * R - (int64_t)L;
#pragma unroll 4
    for (uint32_t a = tid; a < NX; a += CHAN_THREADS) {
        const int64_t k = kb + a;
        float2 v = make_float2(0.0f, 0.0f);
        if (k >= 0) { if (k < (int64_t)W) v = iq_float(row[k]); }
        else if (k >= -(int64_t)H) v = hs[(int64_t)H + k];
        xs[a] = v;
    }
    for (uint32_t a = tid; a < M; a += CHAN_THREADS) twl[a] = tw[a];
    __syncthreads();
    for (uint32_t it = tid; it < nw * M; it += CHAN_THREADS) {
        const uint32_t g = it / M, r = it - g * M;
        // the newest sample of time g is the block's sample (n0 + g) R - 1, place g R + L - 1 of xs; + M keeps the sum above zero at n0 + g = 0
        const uint32_t i0 = (uint32_t)(((uint64_t)(n0 + g) * R + (uint64_t)cm + 2 * M - 1 - r) % M);
        float2 w;
        core::chan_fold(taps, L, M, i0, reinterpret_cast<const float*>(xs + (size_t)g * R + L - 1), w.x, w.y);
        wz[g * MP + r] = w;
    }
    __syncthreads();
    for (uint32_t it = tid; it < nw * M; it += CHAN_THREADS) {
        const uint32_t g = it / M, e = it - g * M, k2 = e / M1, r1 = e - k2 * M1;
        float2 a;
        core::chan_pass1(reinterpret_cast<const float*>(wz + g * MP), M1, M2, reinterpret_cast<const float*>(twl), r1, k2, a.x, a.y);
        ab[g * MP + r1 * M2 + k2] = a;
    }
    __syncthreads();
    for (uint32_t it = tid; it < nw * nu; it += CHAN_THREADS) {
        const uint32_t j = it / nw, g = it - j * nw, k = ubins[j];
        float2 z;
        core::chan_pass2(reinterpret_cast<const float*>(ab + g * MP), M1, M2, reinterpret_cast<const float*>(twl), k, z.x, z.y);
        wz[k * NW + g] = z;
    }
    __syncthreads();
    const uint32_t tt = nw - 1;   // outputs of this tile
    for (uint32_t it = tid; it < np * tt; it += CHAN_THREADS) {
        const uint32_t p = it / tt, g = it - p * tt + 1, k = pairs[2 * p], c = pairs[2 * p + 1];
        if (c >= C) continue;
        const uint32_t n = n0 + g - 1;
        const float2 z = wz[k * NW + g], b = n == 0 ? carry[c] : wz[k * NW + g - 1];
        dst[(size_t)c * dpitch + XPRE + n] = core::fm_discriminate(z.x, z.y, b.x, b.y, gain);
        if constexpr (METER) meter_put(c, n, z, pw...);
        if (n == T - 1) znew[c] = z;
    }
}

}  // namespace m17
