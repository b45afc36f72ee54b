// K-1: the tuner in front of the chain (wideband IQ input, m17hip_upload_wide): per channel, mix its source to the channel's offset, low-pass with the
// context's taps, keep every R-th sample and discriminate — z[n] = sum_i h[i] mixed[nR + R - 1 - i], y[n] = gain * arg(z[n] conj(z[n-1])) — into the rows of
// the context's FLOAT input slab: from there on the stream is a float stream like any other.  The arithmetic is core::ddc_mix, ddc_tap and fm_discriminate
// (detail/core.h: the host form gives the same words).  gfx950 / CDNA4, wave64.
#pragma once

#include "m17_common.hpp"
#include "m17_iq_kernels.hpp"

namespace m17 {

// a wideband sample as two floats (all exact): int16 and float32 as iq_float has them, uint8 in rtl_sdr's convention
__device__ __forceinline__ float2 iq_float(uchar2 v) { return make_float2(core::ddc_u8(v.x), core::ddc_u8(v.y)); }

// The power scratch of a metered launch (m17hip_wide_meter; csrc/m17_meter_kernels.hpp): [channels][pitch] floats, chan_power of the z of output n of
// channel c at p[c * pitch + n].  The metered instantiations of the four wideband kernels take one as their last argument; the others have no such argument.
struct MeterOut { float* p; size_t pitch; };
__device__ __forceinline__ void meter_put(uint32_t c, uint32_t n, float2 z, MeterOut m) { m.p[(size_t)c * m.pitch + n] = core::chan_power(z.x, z.y); }

constexpr int WIDE_THREADS = 64;                        // one wave per workgroup
constexpr int WIDE_PER_LANE = 4;                        // filter sums in flight per lane: lane l has z number l, l + 64, l + 128, l + 192 of the tile
constexpr int WIDE_Z = WIDE_THREADS * WIDE_PER_LANE;    // z per tile: the one in front of the tile's first output and one per output
constexpr int WIDE_TILE = WIDE_Z - 1;                   // outputs per tile
constexpr int WIDE_TAPS = 8;                            // taps fetched together
// the tile's LDS in float2: R planes of WIDE_TILE + J mixed samples, J = ceil(L / R), and the tile's z
__host__ __device__ inline uint32_t wide_plane(uint32_t L, uint32_t R) { return WIDE_TILE + (L + R - 1) / R; }
__host__ __device__ inline size_t wide_lds_bytes(uint32_t L, uint32_t R) { return ((size_t)R * wide_plane(L, R) + WIDE_Z) * sizeof(float2); }   // <= 42880 (R = 16, L = 1024)

// What a squelched launch of a tuner takes as its last argument (m17hip_wide_squelch; csrc/m17_squelch_kernels.hpp): the block's state words, [channels] of
// h' | open << 31.
struct SquelchIn { const uint32_t* state; };
// A tile-squelched launch (m17hip_wide_squelch_slots) takes the block's tile mask instead: [channels][words], bit t & 31 of word t >> 5 set where the
// channel's tile t is tuned.  SQUELCH stays one template flag: the type of the trailing argument says which decision a workgroup reads.
struct SquelchTilesIn { const uint32_t* mask; uint32_t words; };
__device__ __forceinline__ bool squelch_closed(uint32_t c, uint32_t, SquelchIn q) { return !(q.state[c] & core::SQUELCH_OPEN); }
__device__ __forceinline__ bool squelch_closed(uint32_t c, uint32_t tile, SquelchTilesIn q) { return !((q.mask[(size_t)c * q.words + (tile >> 5)] >> (tile & 31u)) & 1u); }
template <typename Q> __device__ __forceinline__ bool squelch_closed(uint32_t c, uint32_t tile, MeterOut, Q q) { return squelch_closed(c, tile, q); }
// (the metered and squelched instantiations carry both: the power goes where the meter's argument says)
__device__ __forceinline__ void meter_put(uint32_t c, uint32_t n, float2 z, MeterOut m, SquelchIn) { meter_put(c, n, z, m); }
__device__ __forceinline__ void meter_put(uint32_t c, uint32_t n, float2 z, MeterOut m, SquelchTilesIn) { meter_put(c, n, z, m); }
__device__ __forceinline__ void squelch_power(uint32_t, uint32_t, SquelchIn) {}
__device__ __forceinline__ void squelch_power(uint32_t, uint32_t, SquelchTilesIn) {}
__device__ __forceinline__ void squelch_power(uint32_t c, uint32_t n, MeterOut m, SquelchIn) { m.p[(size_t)c * m.pitch + n] = 0.0f; }
__device__ __forceinline__ void squelch_power(uint32_t c, uint32_t n, MeterOut m, SquelchTilesIn) { m.p[(size_t)c * m.pitch + n] = 0.0f; }

// A closed channel's workgroup: the outputs n0 .. n1 - 1 of the block (n1 <= T) get +0, the meter's power scratch likewise where there is one, and the
// workgroup that holds output T - 1 leaves (0, 0) as the channel's carry.  No LDS, no barrier.
template <typename... PW>
__device__ __forceinline__ void squelch_zero(uint32_t c, uint32_t n0, uint32_t n1, uint32_t T, float* __restrict__ d, float2* __restrict__ znew, PW... pw)
{
    for (uint32_t n = n0 + threadIdx.x; n < n1; n += WIDE_THREADS) {
        d[n] = 0.0f;
        squelch_power(c, n, pw...);
        if (n == T - 1) znew[c] = make_float2(0.0f, 0.0f);
    }
}

// Grid (tiles of WIDE_TILE outputs, channels).  Channel c listens to source table[c] at the frequency word table[maxC + c].
// 1. The workgroup mixes the (WIDE_TILE + J) R input samples under its tile ONCE into LDS (the oscillator costs as much as ten taps: never per output).
//    Sample k of the block (k < 0: the source's carried history of H = L - 1 converted samples; below that and behind the row's end: zero, which no stored
//    output reads) has the phase fcw * (count + k).  Layout: sample u of the tile (u = 0 is sample n0 R - J R of the block) lies in plane u % R at u / R —
//    the polyphase order — so that in step 2 all lanes read ONE plane at consecutive places, whatever R is: a lane-to-sample stride of R float2 would
//    conflict on the 64 banks for every even R.  A lane fills place a of every plane from R consecutive samples: no division, conflict-free stores.
// 2. Lane l runs the two fma chains of its WIDE_PER_LANE z over LDS, taps in the order i = 0 .. L - 1 (i = R j + rho reads plane R - 1 - rho at
//    w + J - 1 - j); the tap is a scalar load.  At L = 513 that is a long serial chain, hence four in flight.
// 3. The z go to LDS, and output n = n0 + w - 1 is z[w] against z[w - 1].  In front of the block's output 0 that is the channel's CARRY (the last z of the
//    block before; zero for a fresh feed); in front of a later tile's first output the z is recomputed (one in 256).  The block's last z goes to znew[c]:
//    tile 0 of this launch reads carry[c], so the carry itself is written by wide_carry_kernel behind this launch.
// Samples are read one by one (a sample is aligned to its own size, nothing more is asked of the rows); vector stores only, no atomics.
// METER (m17hip_wide_meter is on): the launch has one more argument, a MeterOut, and every output's chan_power(z) goes to it beside the output's y.
// SQUELCH (m17hip_wide_squelch is on): the launch's last argument is a SquelchIn, and the workgroups of a channel whose state word says closed store +0 for
// their tile's outputs (and powers), (0, 0) for the carry where they hold output T - 1, and return — before any LDS traffic, barrier or mixing.  The flag is
// the channel's, so the return is uniform for the workgroup.  Under m17hip_wide_squelch_slots the last argument is a SquelchTilesIn instead and the flag is
// the (channel, tile)'s — the workgroup's own bit of the block's tile mask —, read in the same place: SQUELCH stays one flag.
template <typename IQT, bool METER = false, bool SQUELCH = false, typename... PW>
__global__ __launch_bounds__(WIDE_THREADS) void tune_kernel(const IQT* __restrict__ src, size_t spitch, uint32_t W, const float2* __restrict__ hist,
                                                            const float* __restrict__ taps, uint32_t L, uint32_t R, const uint32_t* __restrict__ table,
                                                            uint32_t maxC, uint32_t count, float* __restrict__ dst, size_t dpitch, uint32_t T,
                                                            const float2* __restrict__ carry, float2* __restrict__ znew, float gain, PW... pw)
{
    extern __shared__ float2 wide_lds[];
    const uint32_t c = blockIdx.y, lane = threadIdx.x;
    const uint32_t n0 = blockIdx.x * WIDE_TILE;
    if constexpr (SQUELCH) {
        if (squelch_closed(c, blockIdx.x, pw...)) {
            squelch_zero(c, n0, T - n0 < (uint32_t)WIDE_TILE ? T : n0 + WIDE_TILE, T, dst + (size_t)c * dpitch + XPRE, znew, pw...);
            return;
        }
    }
    const uint32_t s = table[c], fcw = table[maxC + c];
    const uint32_t J = (L + R - 1) / R, P = WIDE_TILE + J, H = L - 1;
    float2* zbuf = wide_lds + (size_t)R * P;
    const IQT* row = src + (size_t)s * spitch;
    const float2* hs = hist + (size_t)s * H;
    const int64_t k0 = (int64_t)n0 * R - (int64_t)J * R;
    for (uint32_t a = lane; a < P; a += WIDE_THREADS) {
        int64_t k = k0 + (int64_t)a * R;
        for (uint32_t r = 0; r < R; ++r, ++k) {
            float2 v = make_float2(0.0f, 0.0f);
            if (k >= 0) { if (k < (int64_t)W) v = iq_float(row[k]); }
            else if (k >= -(int64_t)H) v = hs[(int64_t)H + k];
            float2 m;
            core::ddc_mix(v.x, v.y, fcw, count + (uint32_t)k, m.x, m.y);
            wide_lds[r * P + a] = m;
        }
    }
    __syncthreads();
    float2 z[WIDE_PER_LANE];
#pragma unroll
    for (int q = 0; q < WIDE_PER_LANE; ++q) z[q] = make_float2(0.0f, 0.0f);
    // tap i = R j + rho: plane R - 1 - rho, place w + J - 1 - j.  The place in the planes is a scalar that all lanes share; the taps come WIDE_TAPS at a
    // time, so one wait covers several steps of the chains.  (The compiler pairs the lane's four 8-byte reads into two ds_read2st64_b64.  Four separate
    // ds_read_b64 through offsets it cannot relate were measured: 11 % slower — three more address adds per tap — so the pairs stay.)
    const float2* base = wide_lds + lane;
    uint32_t off = (R - 1) * P + J - 1, rho = 0, jrow = J - 1;
    auto step = [&](float t) {
        const float2* p = base + off;
#pragma unroll
        for (int q = 0; q < WIDE_PER_LANE; ++q) {
            const float2 v = p[q * WIDE_THREADS];
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

// behind tune_kernel on its stream: the channels' carries of the next block, a lane per channel
__global__ void wide_carry_kernel(const float2* __restrict__ znew, float2* __restrict__ carry, uint32_t C)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) carry[c] = znew[c];
}

// beside it: the sources' histories of the next block — the last H converted samples of history and row together, from `hist` into `next` (the two take
// turns: a block shorter than the history moves it by less than its length); a lane per sample, sources on grid.y
template <typename IQT>
__global__ void wide_hist_kernel(const IQT* __restrict__ src, size_t spitch, uint32_t W, const float2* __restrict__ hist, float2* __restrict__ next, uint32_t H)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
    if (j >= H) return;
    const int64_t k = (int64_t)W - (int64_t)H + j;   // the block's sample that becomes history place j
    next[(size_t)s * H + j] = k >= 0 ? iq_float(src[(size_t)s * spitch + k]) : hist[(size_t)s * H + (int64_t)H + k];
}

}  // namespace m17
