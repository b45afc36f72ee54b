// K0: the FM discriminator in front of the chain (complex IQ input, m17hip_upload_iq): y[n] = gain * arg(x[n] * conj(x[n-1])) per channel, written
// into the rows of the context's FLOAT input slab — from there on the stream is a float stream like any other.  The arithmetic is core::fm_discriminate
// (detail/core.h: the host form gives the same words).  gfx950 / CDNA4, wave64.
#pragma once

#include "m17_common.hpp"

namespace m17 {

// an IQ sample as two floats: an int16 pair is converted (exact), a float pair is taken as it is
__device__ __forceinline__ float2 iq_float(short2 v) { return make_float2((float)v.x, (float)v.y); }
__device__ __forceinline__ float2 iq_float(float2 v) { return v; }

constexpr int IQ_THREADS = 256;   // lanes per workgroup
constexpr int IQ_LANE = 4;        // consecutive samples per lane: one 16-byte store, one (int16 IQ) or two (float IQ) 16-byte loads
template <typename IQT> struct alignas(16) IqQuad { IQT v[IQ_LANE]; };

// Rows of T interleaved I,Q samples (IQT = short2 / float2, row pitch `spitch` in complex samples) -> the data region of the float slab's rows (dpitch in
// floats, behind the XPRE prefix), channels on grid.y as copy_rows_xf32_kernel has them.  Bandwidth-shaped: 8 + 4 or 4 + 4 bytes and about 40 VALU
// operations per sample; no LDS, no atomics.  A lane takes IQ_LANE consecutive samples of one row, a wave a contiguous span of 256, a workgroup 1024.  The
// sample in front of a lane's first one is one overlapping load (the neighbouring lane's last sample, out of the cache); in front of a row's sample 0 it
// is the channel's CARRY: the last IQ sample of the previous IQ block as floats (zero for a fresh feed: core::fm_phase(+-0, +-0) = +0).
// The workgroup that reads carry[c] and the one that holds the row's last sample are different workgroups of this launch, so the new carry is NOT written
// here: iq_carry_kernel follows on the same stream (the way the copy_tail_* kernels follow a run), and a launch on the other stream goes behind its event.
// Rows whose address is not 16-byte aligned and the ragged end of a row go sample by sample.
template <typename IQT>
__global__ __launch_bounds__(IQ_THREADS) void discriminate_kernel(const IQT* __restrict__ src, size_t spitch, float* __restrict__ dst, size_t dpitch, uint32_t T,
                                                                  const float2* __restrict__ carry, float gain)
{
    const uint32_t c = blockIdx.y;
    const uint32_t t = (blockIdx.x * blockDim.x + threadIdx.x) * IQ_LANE;
    if (t >= T) return;
    const IQT* s = src + (size_t)c * spitch + t;
    float* d = dst + (size_t)c * dpitch + XPRE + t;
    float2 p = t ? iq_float(s[-1]) : carry[c];
    if (t + IQ_LANE <= T && (((uintptr_t)s) & 15) == 0) {
        const IqQuad<IQT> in = *reinterpret_cast<const IqQuad<IQT>*>(s);
        float o[IQ_LANE];
#pragma unroll
        for (int q = 0; q < IQ_LANE; ++q) {
            const float2 v = iq_float(in.v[q]);
            o[q] = core::fm_discriminate(v.x, v.y, p.x, p.y, gain);
            p = v;
        }
        *reinterpret_cast<float4*>(d) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
        for (uint32_t q = 0; q < IQ_LANE && t + q < T; ++q) {
            const float2 v = iq_float(s[q]);
            d[q] = core::fm_discriminate(v.x, v.y, p.x, p.y, gain);
            p = v;
        }
    }
}

// behind discriminate_kernel on its stream: the carry of the next IQ block, a lane per channel
template <typename IQT>
__global__ void iq_carry_kernel(const IQT* __restrict__ src, size_t spitch, uint32_t T, float2* __restrict__ carry, uint32_t C)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) carry[c] = iq_float(src[(size_t)c * spitch + T - 1]);
}

}  // namespace m17
