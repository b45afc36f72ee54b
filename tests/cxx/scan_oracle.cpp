// TEST INFRASTRUCTURE ONLY: the HOST form of the carrier scan of m17hip_wide_scan — m17cxx/detail/core.h's scan_peak, scan_distance, scan_fcw, scan_assign,
// scan_idle and scan_source, compiled by the host compiler.  Built and loaded by tests/scan_lib.py (g++ -O2 -ffp-contract=off).  The planes come from
// spectrum_lib, the floor plane from squelch_floor_lib; the table goes to squelch_lib's host form and the tuners' as a given table does.
#include "../../m17-cxx-demod_amd/include/m17cxx/detail/core.h"

#include <stddef.h>

#include <vector>

namespace core = mobilinkd::core;

extern "C" {

uint32_t sc_flag_bits(void) { return core::SCAN_SLOT | core::SCAN_ASSIGNED << 8 | core::SCAN_HELD << 16; }

uint32_t sc_max_slots(void) { return core::SCAN_MAX_SLOTS; }

void sc_bands(const float* row, uint32_t N, uint32_t B, float* band)
{
    for (uint32_t k = 0; k < N; ++k) band[k] = core::squelch_band(row, N, k, B);
}

int sc_peak(const float* band, uint32_t N, uint32_t k, uint32_t X, float to) { return core::scan_peak(band, N, k, X, to) ? 1 : 0; }

uint32_t sc_distance(uint32_t a, uint32_t b, uint32_t N) { return core::scan_distance(a, b, N); }

int32_t sc_fcw(const float* row, uint32_t N, uint32_t logn, uint32_t k, uint32_t B, float med) { return core::scan_fcw(row, N, logn, k, B, med); }

int32_t sc_assign(const float* row, const float* band, uint32_t N, uint32_t logn, uint32_t k, uint32_t B, float med, float to)
{
    return core::scan_assign(row, band, N, logn, k, B, med, to);
}

int sc_idle(uint32_t J, float open_level, float med) { return core::scan_idle(J, open_level, med) ? 1 : 0; }

// One block's scan for S sources, what wide_scan_kernel does, a source after the other: plane[S][N] of J frames, floor[4][S] the block's floor plane,
// src[C] / fcw[C] the table in front of the block (fcw rewritten for the assigned slots), pool[C] the slot marks, of which the first n channels are the
// block's; hold[C] the squelch's counts in front of the block.  flags[C] and missed[S] are written.
void sc_block(const float* plane, uint32_t logn, uint32_t J, uint32_t S, const float* floor, uint32_t B, uint32_t X, uint32_t hang, const uint32_t* src,
              int32_t* fcw, const uint8_t* pool, uint32_t C, uint32_t n, const uint32_t* hold, uint32_t* flags, uint32_t* missed)
{
    const uint32_t N = 1u << logn;
    std::vector<float> scratch(N);
    for (uint32_t c = 0; c < C; ++c) flags[c] = pool[c] ? core::SCAN_SLOT : 0u;
    for (uint32_t s = 0; s < S; ++s) {
        std::vector<uint32_t> slot;
        for (uint32_t c = 0; c < n; ++c) if (pool[c] && src[c] == s) slot.push_back(c);
        missed[s] = core::scan_source(plane + (size_t)s * N, N, logn, J, B, X, floor[2 * (size_t)S + s], floor[3 * (size_t)S + s], floor[s], hang,
                                      slot.data(), (uint32_t)slot.size(), hold, fcw, flags, scratch.data());
    }
}

}
