// K-2: the wideband signal generator behind the modulator (m17hip_synth_wide, ABI 617): every int16 baseband of the context's input slab FM-modulated
// and put at its offset into the wide IQ stream of its source, at 48000 P / Q samples per second.  The words are core.h's (wtx_index, wtx_step, wtx_within,
// wtx_theta, wtx_phase, wtx_add, wtx_noise, wtx_i16, wtx_u8): integer ring arithmetic up to the oscillator's argument, so neither the scan of the first
// kernel nor the tiling of the second can change a bit.  Vector stores only, no atomics.  gfx950 / CDNA4, wave64.
//
// wide_tx_prefix_kernel   one wave per channel: the prefix A2[k] = A2_carry + sum_{i<k} (b[i-1] + b[i]) of its row, four samples a lane and a wave scan per
//                         256 samples, written as the phase base K P^2 A2[k] (uint64) to the scratch plane; the carries advance.
// wide_tx_mux_kernel      one workgroup per (source, tile of WTX_TILE wideband samples), four outputs a lane 256 apart (every store of a wave is 64
//                         consecutive samples).  The source's channels come from a host-made list in ascending order, WTX chunks of them at a time: the few
//                         baseband samples and phase bases the tile spans are staged in LDS once per workgroup, then every lane adds channel after channel.
#pragma once

#include "m17_common.hpp"

namespace m17 {

constexpr int WTX_THREADS = 256;
constexpr uint32_t WTX_PER_LANE = 4, WTX_TILE = WTX_THREADS * WTX_PER_LANE;
constexpr uint32_t WTX_SCAN = 256;             // samples per wave and pass of the prefix kernel
constexpr uint32_t WTX_LDS_BUDGET = 32768;     // bytes of staging a workgroup asks for at most (one channel of a tile at P / Q = 1 is 10 KB)
constexpr uint32_t WTX_CHUNK_MAX = 64;
constexpr uint32_t WTX_ENTRY = 4;              // words per entry of the list: channel, fcw, phase0, amplitude

// baseband samples a tile can span: k of its last sample minus k of its first, plus one, at the latest place r0 = P - 1 its first can have
__host__ __device__ inline uint32_t wtx_span(uint32_t P, uint32_t Q) { return (uint32_t)(((uint64_t)(P - 1) + (uint64_t)(WTX_TILE - 1) * Q) / P) + 1; }
__host__ __device__ inline uint32_t wtx_chan_bytes(uint32_t NK) { return 8 * NK + 2 * (NK + 1); }   // NK bases and NK + 1 samples (b[k - 1] of the first)
__host__ __device__ inline uint32_t wtx_chunk(uint32_t NK)
{
    const uint32_t ch = WTX_LDS_BUDGET / wtx_chan_bytes(NK);
    return ch < 1 ? 1 : ch > WTX_CHUNK_MAX ? WTX_CHUNK_MAX : ch;
}
__host__ __device__ inline size_t wtx_lds_bytes(uint32_t NK, uint32_t CH) { return ((size_t)CH * wtx_chan_bytes(NK) + 7) / 8 * 8; }
// words of the device table for S sources and n listed channels: first[S + 1], then the entries
__host__ __device__ inline size_t wtx_table_words(uint32_t S, uint32_t n) { return (size_t)S + 1 + (size_t)WTX_ENTRY * n; }

__device__ __forceinline__ uint64_t wtx_shfl_up(uint64_t v, uint32_t o)
{
    const uint32_t lo = __shfl_up((uint32_t)v, o), hi = __shfl_up((uint32_t)(v >> 32), o);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wtx_shfl(uint64_t v, int lane)
{
    const uint32_t lo = __shfl((uint32_t)v, lane), hi = __shfl((uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

// Grid (maxC); x: the int16 slab (rows of xpitch, XPRE in front); n samples a row; KP2 = K P^2 mod 2^64.  Channel c < C: plane[c][k] = KP2 A2[k], k < n,
// a2[c] += sum, last_out[c] = b[n - 1].  Channel c >= C: last_out[c] = last_in[c] (its feed has no block here; a2[c] stays).
__global__ __launch_bounds__(64) void wide_tx_prefix_kernel(const int16_t* __restrict__ x, size_t xpitch, uint32_t C, uint32_t n, uint64_t KP2,
                                                            uint64_t* __restrict__ a2, const int32_t* __restrict__ last_in, int32_t* __restrict__ last_out,
                                                            uint64_t* __restrict__ plane, size_t ppitch)
{
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    if (c >= C) {
        if (lane == 0) last_out[c] = last_in[c];
        return;
    }
    const int16_t* row = x + (size_t)c * xpitch + XPRE;
    uint64_t* out = plane + (size_t)c * ppitch;
    uint64_t carry = a2[c];
    const int32_t last = last_in[c];
    for (uint32_t i0 = 0; i0 < n; i0 += WTX_SCAN) {
        const uint32_t i = i0 + 4u * lane;
        int32_t b[5];
        b[0] = i == 0 ? last : i - 1 < n ? (int32_t)row[i - 1] : 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) b[q + 1] = i + q < n ? (int32_t)row[i + q] : 0;
        uint64_t ex[4], tot = 0;   // ex[q]: the steps of this lane's samples before q
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            ex[q] = tot;
            tot += i + q < n ? core::wtx_step(b[q], b[q + 1]) : 0ull;
        }
        uint64_t inc = tot;
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint64_t t = wtx_shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        const uint64_t before = carry + (inc - tot);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q)
            if (i + q < n) out[i + q] = KP2 * (before + ex[q]);
        carry += wtx_shfl(inc, 63);
    }
    if (lane == 0) {
        a2[c] = carry;
        last_out[c] = (int32_t)row[n - 1];
    }
}

__device__ __forceinline__ void wtx_store(float2* d, float re, float im) { *d = make_float2(re, im); }
__device__ __forceinline__ void wtx_store(short2* d, float re, float im) { *d = make_short2(core::wtx_i16(re), core::wtx_i16(im)); }
__device__ __forceinline__ void wtx_store(uchar2* d, float re, float im) { *d = make_uchar2(core::wtx_u8(re), core::wtx_u8(im)); }

// Grid (tiles of WTX_TILE samples of a row of W, S sources).  table: first[S + 1] | entries (channel, fcw, phase0, amplitude), those of source s at
// first[s] .. first[s + 1] - 1 in ascending channel order.  c0: the feed's sample count at the block's start; last: b[-1] per channel; NK = wtx_span(P, Q),
// CH = wtx_chunk(NK); LDS wtx_lds_bytes(NK, CH): [CH][NK] bases, then [CH][NK + 1] samples, entry i of a channel b[k0 + i - 1].
// Sample i of the tile: m Q = k0 P + r0 + i Q, so k = k0 + (r0 + i Q) div P and r = (r0 + i Q) mod P in 32 bits — core::wtx_index's words.
template <typename OUT>
__global__ __launch_bounds__(WTX_THREADS) void wide_tx_mux_kernel(const int16_t* __restrict__ x, size_t xpitch, const uint64_t* __restrict__ plane, size_t ppitch,
                                                                  const int32_t* __restrict__ last, const uint32_t* __restrict__ table, uint32_t S, uint32_t P,
                                                                  uint32_t Q, uint64_t K, uint32_t W, uint64_t c0, uint32_t NK, uint32_t CH, float sigma,
                                                                  uint64_t seed, OUT* __restrict__ dst, size_t dpitch)
{
    extern __shared__ uint64_t wtx_lds[];
    const uint32_t s = blockIdx.y, m0 = blockIdx.x * WTX_TILE, tid = threadIdx.x;
    const uint32_t n = W - m0 < WTX_TILE ? W - m0 : WTX_TILE;   // (m0 < W)
    uint32_t k0, r0, kl, rl;
    core::wtx_index(m0, P, Q, k0, r0);
    core::wtx_index(m0 + n - 1, P, Q, kl, rl);
    const uint32_t nk = kl - k0 + 1;   // <= NK
    const uint32_t NB = NK + 1;
    uint64_t* lbase = wtx_lds;
    int16_t* lb = reinterpret_cast<int16_t*>(wtx_lds + (size_t)CH * NK);
    uint32_t ko[WTX_PER_LANE], r[WTX_PER_LANE];
    float re[WTX_PER_LANE], im[WTX_PER_LANE];
#pragma unroll
    for (uint32_t j = 0; j < WTX_PER_LANE; ++j) {
        const uint32_t t = r0 + (tid + j * WTX_THREADS) * Q;   // (below 2000 + 1024 * 32)
        ko[j] = t / P;                                         // (< NK for every lane, the ones past n included: they read staged words and store nothing)
        r[j] = t % P;
        re[j] = 0.0f; im[j] = 0.0f;
    }
    const uint32_t a0 = table[s], a1 = table[s + 1];
    const uint32_t* ent = table + S + 1;
    for (uint32_t a = a0; a < a1; a += CH) {
        const uint32_t nc = a1 - a < CH ? a1 - a : CH;
        __syncthreads();   // (the chunk before has been read)
        for (uint32_t it = tid; it < nc * nk; it += WTX_THREADS) {
            const uint32_t ci = it / nk, i = it - ci * nk, ch = ent[WTX_ENTRY * (a + ci)];
            lbase[ci * NK + i] = plane[(size_t)ch * ppitch + k0 + i];
        }
        for (uint32_t it = tid; it < nc * (nk + 1); it += WTX_THREADS) {
            const uint32_t ci = it / (nk + 1), i = it - ci * (nk + 1), ch = ent[WTX_ENTRY * (a + ci)];
            lb[ci * NB + i] = k0 + i == 0 ? (int16_t)last[ch] : x[(size_t)ch * xpitch + XPRE + (k0 + i - 1)];
        }
        __syncthreads();
        for (uint32_t ci = 0; ci < nc; ++ci) {
            const uint32_t* e = ent + WTX_ENTRY * (a + ci);
            const uint32_t fcw = e[1], ph0 = e[2];
            const float amp = __uint_as_float(e[3]);
#pragma unroll
            for (uint32_t j = 0; j < WTX_PER_LANE; ++j) {
                const uint64_t base = lbase[ci * NK + ko[j]];
                const int32_t bp = lb[ci * NB + ko[j]], b = lb[ci * NB + ko[j] + 1];
                const uint64_t theta = core::wtx_theta(base, K, core::wtx_within(bp, b, r[j], P));
                core::wtx_add(amp, core::wtx_phase(theta, fcw, (uint32_t)c0 + m0 + tid + j * WTX_THREADS, ph0), re[j], im[j]);
            }
        }
    }
    const uint64_t ns = core::wtx_noise_stream(seed, s);
    OUT* row = dst + (size_t)s * dpitch + m0;
#pragma unroll
    for (uint32_t j = 0; j < WTX_PER_LANE; ++j) {
        const uint32_t i = tid + j * WTX_THREADS;
        if (i >= n) continue;
        if (sigma > 0.0f) core::wtx_noise(ns, c0 + m0 + i, sigma, re[j], im[j]);
        wtx_store(row + i, re[j], im[j]);
    }
}

}  // namespace m17
