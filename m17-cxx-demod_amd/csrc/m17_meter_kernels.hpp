// K-1m: the channel meter behind the wideband kernels (m17hip_wide_meter): per channel and per piece of a window of the feed's outputs, the sums of
// p = chan_power(z) — which the metered instantiation of the configuration's kernel has left in the power scratch —, of the y that kernel has stored into
// the float input slab, and of e = y * y.  The words are core::meter_piece, meter_sq and meter_chain's (detail/core.h: meter_sum is the host form): first-level
// chains over 16 outputs, a second-level chain over those, all plain adds from +0 in ascending order.  gfx950 / CDNA4, wave64.
#pragma once

#include "m17_common.hpp"

namespace m17 {

constexpr int METER_THREADS = 256;          // four waves per workgroup
constexpr uint32_t METER_SLOTS = 1024;      // first-level sums of one quantity that the workgroup's LDS holds at a time (3 x 4 KB)
// G, the groups of a whole window, and PP, the pieces a workgroup takes: as many as give every lane a group while they fit (window 16: 256 pieces, a lane
// each), one where a window has more groups than the workgroup lanes (window 65 536: 4096 groups, sixteen per lane, in four passes over the LDS).
__host__ __device__ inline uint32_t meter_groups(uint32_t window) { return (window + core::CHAN_SURVEY_GROUP - 1) / core::CHAN_SURVEY_GROUP; }
__host__ __device__ inline uint32_t meter_pieces_per_wg(uint32_t window)
{
    const uint32_t G = meter_groups(window);
    return G >= (uint32_t)METER_THREADS ? 1u : (uint32_t)METER_THREADS / G;
}

// Grid (ceil(K / PP), channels).  The workgroup takes the pieces k0 .. k0 + PP - 1 of channel c; SLOT pl * G + g is group g of piece k0 + pl (a piece holds
// at most G groups; the block's first and last pieces may hold fewer, and their slots stay idle).
// 1. A lane per slot, METER_SLOTS slots at a time: the three first-level chains over the group's <= 16 outputs, read from the power scratch and from the
//    channel's slab row (which starts at XPRE: nothing beyond 4-byte alignment is assumed, so the loads are single floats; a lane reads 64 consecutive
//    bytes of either, its neighbours the 64 before and behind), into LDS.
// 2. A lane per piece: the three second-level chains over the piece's groups of this pass, carried in a register across the passes — one pass unless
//    the window has more than METER_SLOTS groups.
// 3. Three floats per piece into the plane [3][C][K].  Vector stores only, no atomics.
__global__ __launch_bounds__(METER_THREADS) void wide_meter_kernel(const float* __restrict__ power, size_t ppitch, const float* __restrict__ x, size_t xpitch,
                                                                   uint32_t a0, uint32_t T, uint32_t window, uint32_t K, uint32_t C,
                                                                   float* __restrict__ plane)
{
    __shared__ float q[3][METER_SLOTS];
    const uint32_t tid = threadIdx.x, c = blockIdx.y;
    const uint32_t G = meter_groups(window), PP = meter_pieces_per_wg(window), k0 = blockIdx.x * PP;
    const uint32_t NS = PP * G;   // <= METER_THREADS where PP > 1
    const float* pr = power + (size_t)c * ppitch;
    const float* yr = x + (size_t)c * xpitch + XPRE;
    // the lane's chains of step 2: the three quantities of piece k0 + tid (three independent chains in flight per lane)
    const uint32_t cpl = tid, ck = k0 + cpl;
    const bool chain = cpl < PP && ck < K;
    uint32_t clo = 0, cm = 0;
    if (chain) core::meter_piece(a0, T, window, ck, clo, cm);
    const uint32_t cng = (cm + core::CHAN_SURVEY_GROUP - 1) / core::CHAN_SURVEY_GROUP;
    float accp = 0.0f, accy = 0.0f, acce = 0.0f;
    for (uint32_t s0 = 0; s0 < NS; s0 += METER_SLOTS) {
        const uint32_t s1 = NS - s0 < METER_SLOTS ? NS : s0 + METER_SLOTS;
        for (uint32_t slot = s0 + tid; slot < s1; slot += METER_THREADS) {
            const uint32_t pl = slot / G, g = slot - pl * G, k = k0 + pl;
            if (k >= K) continue;
            uint32_t lo, m;
            core::meter_piece(a0, T, window, k, lo, m);
            const uint32_t o = g * core::CHAN_SURVEY_GROUP;
            if (o >= m) continue;
            const uint32_t n = m - o < core::CHAN_SURVEY_GROUP ? m - o : core::CHAN_SURVEY_GROUP;
            const float* pp = pr + lo + o;
            const float* yp = yr + lo + o;
            float sp, sy, se;
            if (n == core::CHAN_SURVEY_GROUP) {   // (a whole group: the loads go out together)
                float pv[core::CHAN_SURVEY_GROUP], yv[core::CHAN_SURVEY_GROUP], ev[core::CHAN_SURVEY_GROUP];
#pragma unroll
                for (uint32_t i = 0; i < core::CHAN_SURVEY_GROUP; ++i) { pv[i] = pp[i]; yv[i] = yp[i]; }
#pragma unroll
                for (uint32_t i = 0; i < core::CHAN_SURVEY_GROUP; ++i) ev[i] = core::meter_sq(yv[i]);
                sp = core::meter_chain(0.0f, pv, core::CHAN_SURVEY_GROUP);
                sy = core::meter_chain(0.0f, yv, core::CHAN_SURVEY_GROUP);
                se = core::meter_chain(0.0f, ev, core::CHAN_SURVEY_GROUP);
            } else {
                sp = sy = se = 0.0f;
                for (uint32_t i = 0; i < n; ++i) {
                    const float y = yp[i], e = core::meter_sq(y);
                    sp = core::meter_chain(sp, pp + i, 1);
                    sy = core::meter_chain(sy, &y, 1);
                    se = core::meter_chain(se, &e, 1);
                }
            }
            q[0][slot - s0] = sp; q[1][slot - s0] = sy; q[2][slot - s0] = se;
        }
        __syncthreads();
        if (chain) {   // the piece's groups that this pass holds: slots cpl G + g, g0 <= g < g1
            const uint32_t b = cpl * G;   // (PP == 1: 0, and the pass holds groups s0 .. s1 - 1; else s0 == 0 and the pass holds them all)
            const uint32_t g0 = s0 > b ? s0 - b : 0, gend = s1 - b < cng ? s1 - b : cng;
            for (uint32_t g = g0; g < gend; ++g) {
                accp = core::meter_chain(accp, &q[0][b + g - s0], 1);
                accy = core::meter_chain(accy, &q[1][b + g - s0], 1);
                acce = core::meter_chain(acce, &q[2][b + g - s0], 1);
            }
        }
        __syncthreads();   // (the next pass overwrites the sums)
    }
    if (chain) {
        plane[((size_t)0 * C + c) * K + ck] = accp;
        plane[((size_t)1 * C + c) * K + ck] = accy;
        plane[((size_t)2 * C + c) * K + ck] = acce;
    }
}

}  // namespace m17
