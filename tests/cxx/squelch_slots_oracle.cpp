// TEST INFRASTRUCTURE ONLY: the HOST form of the time-resolved squelch of m17hip_wide_squelch_slots — m17cxx/detail/core.h's squelch_slots,
// squelch_slot_frames, squelch_slot_of, squelch_tile_span and squelch_tile_open beside the four functions of the block squelch, compiled by the host compiler.
// Built and loaded by tests/squelch_slots_lib.py (g++ -O2 -ffp-contract=off).  The slots' rows come from spectrum_lib, the z and the y from the host forms of
// the three tuners (wide_lib, wide2_lib, resample_lib).
#include "../../m17-cxx-demod_amd/include/m17cxx/detail/core.h"

#include <stddef.h>

namespace core = mobilinkd::core;

extern "C" {

uint32_t ss_slots(uint32_t J) { return core::squelch_slots(J); }

uint32_t ss_slot_frames(uint32_t J, uint32_t g) { return core::squelch_slot_frames(J, g); }

uint32_t ss_slot_of(uint32_t x, uint32_t first, uint32_t hop, uint32_t G) { return core::squelch_slot_of(x, first, hop, G); }

void ss_tile_span(uint32_t t, uint32_t TO, uint32_t T, uint32_t W, uint32_t* a, uint32_t* e) { core::squelch_tile_span(t, TO, T, W, *a, *e); }

uint32_t ss_tile_open(const uint32_t* bits, uint32_t G, uint32_t first, uint32_t hop, uint32_t lead, uint32_t a, uint32_t e)
{
    return core::squelch_tile_open(bits, G, first, hop, lead, a, e) ? 1u : 0u;
}

// One block's decisions for C channels: rows[S][G][N] the slots' rows of a block of J frames whose first frame starts at block sample `first`, source[C],
// fcw[C], open_level[S], close_level[S]; the tuner makes T outputs from W block samples in `tiles` tiles of TO.  hold[C] is stepped in place through the
// slots; state[C] gets the last slot's word, band[C][G] the band powers, bits[C][SW] the slots' open flags (SW = max(ceil(G / 32), 1)) and mask[C][MW] the
// tile mask (MW = ceil(tiles / 32)) — what the three kernels do, a channel after the other.
void ss_block(const float* rows, uint32_t logn, uint32_t J, uint32_t first, uint32_t hop, const uint32_t* source, const int32_t* fcw, uint32_t C,
              const float* open_level, const float* close_level, uint32_t B, uint32_t hang, uint32_t lead, uint32_t TO, uint32_t T, uint32_t W, uint32_t tiles,
              uint32_t* hold, uint32_t* state, float* band, uint32_t* bits, uint32_t* mask)
{
    const uint32_t N = 1u << logn, G = core::squelch_slots(J), SW = G ? (G + 31u) / 32u : 1u, MW = (tiles + 31u) / 32u;
    for (uint32_t c = 0; c < C; ++c) {
        const uint32_t s = source[c], k = core::squelch_bin(fcw[c], logn);
        uint32_t* o = bits + (size_t)c * SW;
        for (uint32_t i = 0; i < SW; ++i) o[i] = 0;
        uint32_t w = core::squelch_step(hold[c], 0.0f, 0.0f, 0.0f, hang, 0), h = hold[c];
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t Jg = core::squelch_slot_frames(J, g);
            const float b = core::squelch_band(rows + (((size_t)s * G + g) << logn), N, k, B);
            band[(size_t)c * G + g] = b;
            w = core::squelch_step(h, b, core::squelch_level(open_level[s], Jg), core::squelch_level(close_level[s], Jg), hang, Jg);
            h = w & ~core::SQUELCH_OPEN;
            if (w & core::SQUELCH_OPEN) o[g >> 5] |= 1u << (g & 31u);
        }
        hold[c] = h;
        state[c] = w;
        for (uint32_t i = 0; i < MW; ++i) mask[(size_t)c * MW + i] = 0;
        for (uint32_t t = 0; t < tiles; ++t) {
            uint32_t a, e;
            core::squelch_tile_span(t, TO, T, W, a, e);
            if (core::squelch_tile_open(o, G, first, hop, lead, a, e)) mask[(size_t)c * MW + (t >> 5)] |= 1u << (t & 31u);
        }
    }
}

}
