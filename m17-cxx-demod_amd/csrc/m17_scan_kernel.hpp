// K-1s: the carrier scan in front of the block squelch (m17hip_wide_scan): per block and source, the carriers of the block's own spectrum plane and the
// frequency words of the source's pool of channels (its SLOTS), so that a transmission is tuned in the block in which it first appears.  The words are
// core::scan_peak, scan_distance, scan_assign (scan_fcw and the open guarantee), scan_idle and scan_beats' beside the squelch's squelch_bin, squelch_band,
// squelch_level and squelch_step (detail/core.h: core::scan_source, the host form, gives the same words).  It runs on the block's stream between
// squelch_floor_kernel, whose plane holds the median and the levels it reads, and wide_squelch_kernel, which then reads the table THIS kernel writes — as
// the block's tuner does.  gfx950 / CDNA4, wave64.
#pragma once

#include "m17_common.hpp"

namespace m17 {

constexpr int SCAN_THREADS = 256;
constexpr uint32_t SCAN_MAX_POINTS = 4096;
constexpr uint32_t SCAN_MAX_PEAKS = SCAN_MAX_POINTS / 4;   // (two peaks are more than X >= 3 bins apart)
constexpr uint32_t SCAN_WAVES = SCAN_THREADS / 64;

// A workgroup per source s.  plane[S][N] is the block's spectrum of J frames; table[maxC | maxC] the host's channel table (source | fcw) in force for the
// block; pool[maxC] its slot marks; floor[4][S] the block's floor plane (median | floor | open | close); hold[maxC] the squelch's counts in front of the
// block (read only: wide_squelch_kernel steps them behind this kernel); carry[maxC] the slots' words in front of the block, or — `fresh` — the host's words,
// their seeds.  The steps, a barrier between each two:
//   1. the row to LDS (16 KB at 4096 points);  2. band[k] of every bin to LDS (16 KB);
//   3. the peak flags, a bin per lane and pass, and the peaks compacted in ascending bin order: a ballot per wave and pass, the waves' counts in LDS, every
//      lane sums the counts in front of its wave — no append by atomic, so the order is the bins';
//   4. the channel table scanned once, 256 channels a pass: the channels whose entry names s are copied to out[maxC | maxC] (a slot's source is the host's,
//      only its word is the device's), the source's slots among the block's C channels compacted in ascending channel order the same way; then a lane
//      per slot: its word, its bin, and whether it is HELD (squelch_step of the unchanged word has the open bit); the slots not held compacted likewise;
//   5. a lane per peak: covered iff a held slot's bin lies within X;  6. a lane per uncovered peak: its rank is the number of uncovered peaks that beat it
//      (O(P^2) LDS reads over at most 1024 peaks), and the rank-th slot not held takes scan_assign's word;  7. the slots' words, carry and flags are stored.
// A slot at C or above is no part of the block's pool: it keeps its word (on `fresh`: takes its seed).  A block that scan_idle names assigns nothing, holds
// nothing and leaves every word as it is.  Vector stores only, no float atomics, no global atomics (one integer LDS counter), no scratch; 41.3 KB of LDS.
__global__ __launch_bounds__(SCAN_THREADS) void wide_scan_kernel(const float* __restrict__ plane, uint32_t logn, uint32_t J, const uint32_t* __restrict__ table,
                                                                 uint32_t maxC, const uint32_t* __restrict__ pool, const float* __restrict__ floor, uint32_t S,
                                                                 uint32_t B, uint32_t X, uint32_t hang, const uint32_t* __restrict__ hold,
                                                                 uint32_t* __restrict__ carry, uint32_t fresh, uint32_t C, uint32_t* __restrict__ out,
                                                                 uint32_t* __restrict__ flags, uint32_t* __restrict__ missed)
{
    __shared__ float row[SCAN_MAX_POINTS], band[SCAN_MAX_POINTS];
    __shared__ uint32_t peaks[SCAN_MAX_PEAKS];   // bin | covered << 31
    __shared__ uint32_t slot_ch[core::SCAN_MAX_SLOTS], slot_word[core::SCAN_MAX_SLOTS], slot_bin[core::SCAN_MAX_SLOTS], slot_free[core::SCAN_MAX_SLOTS],
        slot_fl[core::SCAN_MAX_SLOTS];
    __shared__ uint32_t pcnt[(SCAN_MAX_POINTS / SCAN_THREADS) * SCAN_WAVES], scnt[2][SCAN_WAVES], fcnt[SCAN_WAVES], uncovered;
    const uint32_t s = blockIdx.x, t = threadIdx.x, N = 1u << logn, lane = t & 63u, wave = t >> 6;
    if (s >= S || N > SCAN_MAX_POINTS) return;   // (uniform over the workgroup)
    const unsigned long long below = (1ull << lane) - 1ull;
    const float* src = plane + (size_t)s * N;
    for (uint32_t i = t; i < N; i += SCAN_THREADS) row[i] = src[i];
    if (t == 0) uncovered = 0;
    const float med = floor[s], lo = floor[2 * (size_t)S + s], lc = floor[3 * (size_t)S + s];
    const bool idle = core::scan_idle(J, lo, med);
    const float to = core::squelch_level(lo, J), tc = core::squelch_level(lc, J);
    __syncthreads();
    for (uint32_t i = t; i < N; i += SCAN_THREADS) band[i] = core::squelch_band(row, N, i, B);
    __syncthreads();
    // 3. the peaks, ascending
    const uint32_t passes = N > (uint32_t)SCAN_THREADS ? N / SCAN_THREADS : 1u;
    uint32_t mine = 0;
    for (uint32_t it = 0; it < passes; ++it) {
        const uint32_t k = it * SCAN_THREADS + t;
        const bool f = !idle && k < N && core::scan_peak(band, N, k, X, to);
        mine |= (f ? 1u : 0u) << it;
        const unsigned long long m = __ballot(f);
        if (lane == 0) pcnt[it * SCAN_WAVES + wave] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    uint32_t P = 0;
    for (uint32_t it = 0; it < passes; ++it)
        for (uint32_t w = 0; w < SCAN_WAVES; ++w) {
            if (w == wave) {   // (uniform over the wave)
                const bool f = (mine >> it) & 1u;
                const unsigned long long m = __ballot(f);
                const uint32_t i = P + (uint32_t)__popcll(m & below);
                if (f && i < SCAN_MAX_PEAKS) peaks[i] = it * SCAN_THREADS + t;
            }
            P += pcnt[it * SCAN_WAVES + w];
        }
    P = P < SCAN_MAX_PEAKS ? P : SCAN_MAX_PEAKS;
    // 4. the table: the source's channels copied, its slots among the block's channels listed in ascending order
    uint32_t ns = 0;
    for (uint32_t base = 0, it = 0; base < maxC; base += SCAN_THREADS, ++it) {
        const uint32_t c = base + t;
        const bool own = c < maxC && table[c] == s;
        const bool slot = own && pool[c] != 0u, pooled = slot && c < C;
        if (own) {
            out[c] = s;
            if (!slot) { out[maxC + c] = table[maxC + c]; flags[c] = 0u; }
            else if (!pooled) {
                const uint32_t w = fresh ? table[maxC + c] : carry[c];
                out[maxC + c] = w; carry[c] = w; flags[c] = core::SCAN_SLOT;
            }
        }
        const unsigned long long m = __ballot(pooled);
        if (lane == 0) scnt[it & 1u][wave] = (uint32_t)__popcll(m);
        __syncthreads();   // (one a pass: the pass after next writes these counts again, behind the next pass's barrier)
        uint32_t off = ns;
        for (uint32_t w = 0; w < SCAN_WAVES; ++w) {
            const uint32_t n = scnt[it & 1u][w];
            off += w < wave ? n : 0u;
            ns += n;
        }
        const uint32_t i = off + (uint32_t)__popcll(m & below);
        if (pooled && i < core::SCAN_MAX_SLOTS) slot_ch[i] = c;
    }
    ns = ns < core::SCAN_MAX_SLOTS ? ns : core::SCAN_MAX_SLOTS;   // (the host refuses a block whose table gives a source more)
    __syncthreads();
    bool held = false;
    if (t < ns) {
        const uint32_t c = slot_ch[t];
        const uint32_t w = fresh ? table[maxC + c] : carry[c];
        const uint32_t kb = core::squelch_bin((int32_t)w, logn);
        held = !idle && (core::squelch_step(hold[c], band[kb], to, tc, hang, J) & core::SQUELCH_OPEN) != 0u;
        slot_word[t] = w;
        slot_bin[t] = held ? kb : 0xFFFFFFFFu;
        slot_fl[t] = core::SCAN_SLOT | (held ? core::SCAN_HELD : 0u);
    }
    const bool vacant = t < ns && !held;
    const unsigned long long mv = __ballot(vacant);
    if (lane == 0) fcnt[wave] = (uint32_t)__popcll(mv);
    __syncthreads();
    uint32_t voff = 0, nfree = 0;
    for (uint32_t w = 0; w < SCAN_WAVES; ++w) {
        const uint32_t n = fcnt[w];
        voff += w < wave ? n : 0u;
        nfree += n;
    }
    if (vacant) slot_free[voff + (uint32_t)__popcll(mv & below)] = t;
    __syncthreads();
    // 5. coverage
    for (uint32_t i = t; i < P; i += SCAN_THREADS) {
        const uint32_t k = peaks[i];
        bool cov = false;
        for (uint32_t j = 0; j < ns; ++j) {
            const uint32_t kb = slot_bin[j];
            cov = cov || (kb != 0xFFFFFFFFu && core::scan_distance(kb, k, N) <= X);
        }
        if (cov) peaks[i] = k | 0x80000000u;
        else atomicAdd(&uncovered, 1u);
    }
    __syncthreads();
    // 6. rank and assignment
    for (uint32_t i = t; i < P; i += SCAN_THREADS) {
        const uint32_t k = peaks[i];
        if (k >> 31) continue;
        const float bk = band[k];
        uint32_t r = 0;
        for (uint32_t j = 0; j < P; ++j) {
            const uint32_t q = peaks[j];
            r += (q >> 31) == 0u && core::scan_beats(band[q & (SCAN_MAX_POINTS - 1u)], q, bk, k) ? 1u : 0u;
        }
        if (r < nfree) {
            const uint32_t si = slot_free[r];   // (ranks are distinct: one writer a slot)
            slot_word[si] = (uint32_t)core::scan_assign(row, band, N, logn, k, B, med, to);
            slot_fl[si] |= core::SCAN_ASSIGNED;
        }
    }
    __syncthreads();
    // 7. the slots' words
    if (t < ns) {
        const uint32_t c = slot_ch[t], w = slot_word[t];
        out[maxC + c] = w;
        carry[c] = w;
        flags[c] = slot_fl[t];
    }
    if (t == 0) missed[s] = uncovered > nfree ? uncovered - nfree : 0u;
}

}  // namespace m17
