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

// ---- the time-resolved squelch (m17hip_wide_squelch_slots): a decision per SLOT — a group of core::CHAN_SURVEY_GROUP frames, whose sums spectrum_kernel has
// left in its scratch[S][G][N] — and a skip per TILE of the tuner's outputs.  Three kernels on the block's stream behind spectrum_kernel; the words are
// core::squelch_slot_frames, squelch_slot_of, squelch_tile_span and squelch_tile_open's beside the four above.  Vector stores only, no atomics.
__host__ __device__ inline uint32_t squelch_slot_words(uint32_t G) { return G ? (G + 31u) / 32u : 1u; }   // words of a channel's slot flags
__host__ __device__ inline uint32_t squelch_tile_words(uint32_t tiles) { return (tiles + 31u) / 32u; }   // words of a channel's tile mask (tiles >= 1)

// 1. A lane per (channel, slot): band[c][g] = the band of scratch[source][g] around the channel's bin.  G >= 1.
__global__ __launch_bounds__(SQUELCH_THREADS) void squelch_slots_band_kernel(const float* __restrict__ scratch, uint32_t logn, uint32_t G,
                                                                             const uint32_t* __restrict__ table, uint32_t maxC, uint32_t B,
                                                                             float* __restrict__ band, uint32_t C)
{
    const uint64_t i = (uint64_t)blockIdx.x * SQUELCH_THREADS + threadIdx.x;
    if (i >= (uint64_t)C * G) return;
    const uint32_t c = (uint32_t)(i / G), g = (uint32_t)(i % G);
    const uint32_t s = table[c], N = 1u << logn;
    const uint32_t k = core::squelch_bin((int32_t)table[maxC + c], logn);
    band[i] = core::squelch_band(scratch + (((size_t)s * G + g) << logn), N, k, B);
}

// 2. A lane per channel: the recurrence over the block's slots from hold[c].  Writes hold[c], state[c] = the last slot's word (h | open << 31 where the block
// has no slot) and the slots' open flags, bits[c][squelch_slot_words(G)], bit g & 31 of word g >> 5.
__global__ __launch_bounds__(SQUELCH_THREADS) void squelch_slots_step_kernel(const float* __restrict__ band, uint32_t G, uint32_t J,
                                                                             const uint32_t* __restrict__ table, const float* __restrict__ levels, uint32_t S,
                                                                             uint32_t hang, uint32_t* __restrict__ hold, uint32_t* __restrict__ state,
                                                                             uint32_t* __restrict__ bits, uint32_t C)
{
    const uint32_t c = blockIdx.x * SQUELCH_THREADS + threadIdx.x;
    if (c >= C) return;
    const uint32_t s = table[c], SW = squelch_slot_words(G);
    const float lo = levels[s], lc = levels[S + s];
    uint32_t word = core::squelch_step(hold[c], 0.0f, 0.0f, 0.0f, hang, 0);   // (G == 0: open, the count as it is)
    uint32_t h = word & ~core::SQUELCH_OPEN, acc = 0;
    const float* b = band + (size_t)c * G;
    uint32_t* o = bits + (size_t)c * SW;
    for (uint32_t g = 0; g < G; ++g) {
        const uint32_t Jg = core::squelch_slot_frames(J, g);
        word = core::squelch_step(h, b[g], core::squelch_level(lo, Jg), core::squelch_level(lc, Jg), hang, Jg);
        h = word & ~core::SQUELCH_OPEN;
        acc |= (word >> 31) << (g & 31u);
        if ((g & 31u) == 31u) { o[g >> 5] = acc; acc = 0; }
    }
    if (G == 0 || (G & 31u)) o[G >> 5] = acc;
    hold[c] = h;
    state[c] = word;
}

// 3. A lane per (channel, word of 32 tiles): mask[c][MW], bit t & 31 of word t >> 5 set where tile t of TO outputs (of T, made from W block samples) is
// tuned; the bits beyond the block's last tile are 0.
__global__ __launch_bounds__(SQUELCH_THREADS) void squelch_slots_tile_kernel(const uint32_t* __restrict__ bits, uint32_t G, uint32_t first, uint32_t hop,
                                                                             uint32_t lead, uint32_t TO, uint32_t T, uint32_t W, uint32_t tiles, uint32_t MW,
                                                                             uint32_t* __restrict__ mask, uint32_t C)
{
    const uint64_t i = (uint64_t)blockIdx.x * SQUELCH_THREADS + threadIdx.x;
    if (i >= (uint64_t)C * MW) return;
    const uint32_t c = (uint32_t)(i / MW), m = (uint32_t)(i % MW);
    const uint32_t* o = bits + (size_t)c * squelch_slot_words(G);
    uint32_t word = 0;
    for (uint32_t j = 0; j < 32u && m * 32u + j < tiles; ++j) {
        uint32_t a, e;
        core::squelch_tile_span(m * 32u + j, TO, T, W, a, e);
        word |= (core::squelch_tile_open(o, G, first, hop, lead, a, e) ? 1u : 0u) << j;
    }
    mask[i] = word;
}

// ---- the sources' noise floor (m17hip_wide_squelch_floor): the levels of either mode above made on the device from the block's own plane, in front of the
// mode's kernels on the block's stream.  A workgroup per source.  The row's keys (core::squelch_floor_key) go to LDS once — 16 KB at 4096 points —, and the
// key of rank N / 2 is selected by radix, the most significant byte first: four passes, each counting the keys that still share the selected prefix in a
// 256-entry LDS histogram (integer LDS adds: the counts do not depend on their order) and choosing the one bucket that holds the rank.  Every lane scans the
// histogram with wave-uniform reads, so the bucket needs no reduction; lane b owns bucket b.  The barriers: behind the keys and the zeroed histogram, behind
// the counts, and behind the choice (which is also in front of the next pass's zeroes).  One lane then applies core::squelch_floor and squelch_track to the
// source's carry F[s] — read and written in stream order like hold[] — and writes F[s] and out[4][S] = med | F' | open | close.  A block without a frame
// (J == 0) leaves F as it is.  Vector stores only, no float atomics, no global atomics.  64 points leave three quarters of the lanes without a key: they
// still zero, scan and meet every barrier.
constexpr int SQUELCH_FLOOR_THREADS = 256;
constexpr uint32_t SQUELCH_FLOOR_MAX_POINTS = 4096;

__global__ __launch_bounds__(SQUELCH_FLOOR_THREADS) void squelch_floor_kernel(const float* __restrict__ plane, uint32_t logn, uint32_t J, uint32_t B,
                                                                              float open_ratio, float close_ratio, float rise, float fall, float floor_min,
                                                                              float* __restrict__ carry, float* __restrict__ out, uint32_t S)
{
    __shared__ uint32_t keys[SQUELCH_FLOOR_MAX_POINTS];
    __shared__ uint32_t hist[SQUELCH_FLOOR_THREADS];
    __shared__ uint32_t sel[2];   // the selected prefix (in place, the bits below it 0) and the rank among the keys that share it
    const uint32_t s = blockIdx.x, t = threadIdx.x, N = 1u << logn;
    if (s >= S || N > SQUELCH_FLOOR_MAX_POINTS) return;   // (uniform over the workgroup)
    const float* row = plane + (size_t)s * N;
    for (uint32_t i = t; i < N; i += SQUELCH_FLOOR_THREADS) keys[i] = core::squelch_floor_key(row[i]);
    uint32_t prefix = 0, mask = 0, rank = N / 2;
    for (uint32_t shift = 24;; shift -= 8) {
        hist[t] = 0;
        __syncthreads();
        for (uint32_t i = t; i < N; i += SQUELCH_FLOOR_THREADS) {
            const uint32_t k = keys[i];
            if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        uint32_t below = 0, mine = 0;
        for (uint32_t b = 0; b < (uint32_t)SQUELCH_FLOOR_THREADS; ++b) {
            const uint32_t n = hist[b];
            below += b < t ? n : 0u;
            mine = b == t ? n : mine;
        }
        if (below <= rank && rank - below < mine) { sel[0] = prefix | (t << shift); sel[1] = rank - below; }   // (one lane: the buckets' counts sum to more than rank)
        __syncthreads();
        prefix = sel[0]; rank = sel[1]; mask |= 255u << shift;
        if (shift == 0) break;
    }
    if (t != 0) return;
    const float med = core::squelch_floor_value(prefix);
    float F = carry[s];
    if (J) F = core::squelch_track(F, core::squelch_floor(med, B, J, floor_min), rise, fall);
    carry[s] = F;
    out[s] = med;
    out[S + s] = F;
    out[2 * (size_t)S + s] = core::squelch_floor_level(F, open_ratio);
    out[3 * (size_t)S + s] = core::squelch_floor_level(F, close_ratio);
}

}  // namespace m17
