// TEST INFRASTRUCTURE ONLY: the HOST form of the source spectrum of m17hip_wide_spectrum — m17cxx/detail/core.h's spec_frames, spec_window, spec_bitrev,
// spec_item1 (and spec_item2, the two-stage pass a device may take), chan_power and the two-level sum (CHAN_SURVEY_GROUP frames per group, both levels
// chains of plain float adds from +0 in ascending order), compiled by the host compiler.  Built and loaded by tests/spectrum_lib.py
// (g++ -O2 -ffp-contract=off; every fmaf is explicit).
#include "../../m17-cxx-demod_amd/include/m17cxx/detail/core.h"

#include <stddef.h>

#include <vector>

namespace core = mobilinkd::core;

extern "C" {

uint32_t sp_group(void) { return core::CHAN_SURVEY_GROUP; }

void sp_frames(uint64_t c0, uint32_t W, uint32_t N, uint32_t hop, uint32_t* first, uint32_t* J) { core::spec_frames(c0, W, N, hop, *first, *J); }

// v: [N][2], in natural order on entry; the DFT in place.  fused != 0: stage 1 alone where logn is odd, then two stages per pass (spec_item2).
void sp_fft(float* v, const float* tw, uint32_t logn, int fused)
{
    const uint32_t N = 1u << logn;
    std::vector<float> t(v, v + 2 * (size_t)N);
    for (uint32_t i = 0; i < N; ++i) { const uint32_t r = core::spec_bitrev(i, logn); v[2 * r] = t[2 * i]; v[2 * r + 1] = t[2 * i + 1]; }
    uint32_t s = 1;
    if (fused) {
        if (logn & 1u) { for (uint32_t j = 0; j < N / 2; ++j) core::spec_item1(v, tw, logn, 1, j); s = 2; }
        for (; s < logn; s += 2) for (uint32_t q = 0; q < N / 4; ++q) core::spec_item2(v, tw, logn, s, q);
    } else {
        for (; s <= logn; ++s) for (uint32_t j = 0; j < N / 2; ++j) core::spec_item1(v, tw, logn, s, j);
    }
}

// x: [W][2], one source block as floats; window[N]; tw[N / 2][2].  out[N]: the plane's words; *first and *J as spec_frames has them.
// What the definition is NOT, for the tests that show a mistake misses the bound: shift — added to every frame's start (the caller keeps it inside the
// block); wshift — the window index is (i + wshift) mod N; single != 0 — ONE ascending chain over all J frames in place of the two levels.
void sp_plane(const float* x, uint32_t W, uint64_t c0, const float* window, const float* tw, uint32_t logn, uint32_t hop, int shift, int wshift, int single,
              int fused, float* out, uint32_t* first, uint32_t* J)
{
    const uint32_t N = 1u << logn;
    core::spec_frames(c0, W, N, hop, *first, *J);
    std::vector<float> v(2 * (size_t)N), P(N, 0.0f), q(N, 0.0f);
    for (uint32_t f = 0; f < *J; ++f) {
        const size_t a = (size_t)((int64_t)*first + (int64_t)f * hop + shift);
        for (uint32_t i = 0; i < N; ++i)
            core::spec_window(window[(i + (uint32_t)(wshift + (int)N)) % N], x[2 * (a + i)], x[2 * (a + i) + 1], v[2 * i], v[2 * i + 1]);
        sp_fft(v.data(), tw, logn, fused);
        const bool last = single ? f + 1 == *J : (f + 1) % core::CHAN_SURVEY_GROUP == 0 || f + 1 == *J;
        for (uint32_t k = 0; k < N; ++k) {
            q[k] = q[k] + core::chan_power(v[2 * k], v[2 * k + 1]);
            if (last) { P[k] = single ? q[k] : P[k] + q[k]; q[k] = 0.0f; }
        }
    }
    for (uint32_t k = 0; k < N; ++k) out[k] = P[k];
}

}
