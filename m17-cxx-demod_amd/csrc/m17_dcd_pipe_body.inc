// The body of dcd_pipe_kernel<INVERT> and dcd_pipe_mixed_kernel (m17_frontend_kernels.hpp): included into both, inside the kernel's braces.
// The including kernel names: INVERT, MIXED (constants); pol (MIXED only: the polarity table; the producer's per-lane mask is its entry XOR bit 0 of flags);
// XT, the sample type of the input slab: int16_t, or float (a float stream: nothing is scaled, negation is a sign-bit XOR, under the lane's mask when MIXED).
    constexpr bool F32 = std::is_same<XT, float>::value;
    __shared__ __attribute__((aligned(16))) float dbuf[2][DP_CPB][DP_DPITCH];
    __shared__ __attribute__((aligned(16))) float4 xb[2][DP_BLK / 2][64];
    const int role = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int g = lane >> 1, bin = lane & 1;
    uint32_t c = blockIdx.x * DP_CPB + g;
    const bool live = c < C;   // lanes beyond the last channel shadow it and never store
    if (!live) c = C - 1;
    const XT* xr = x + (size_t)c * xpitch + XPRE;
    DcdState* st = state + c;
    const uint32_t NB = T / DP_BLK;       // blocks
    // every role runs NI hand-overs: NB + 2 for pipeline fill and drain, rounded up to a multiple of DP_PF so that the
    // producer's unrolled loop has no early exit (its registers stay in fixed slots and its waits stay partial)
    const uint32_t NI = (NB + 2u + DP_PF - 1u) / DP_PF * DP_PF;

    if (role == 0) {
        // ---- P: scaling and delta.  A block lasts ~0.5 us, an HBM round trip twice that: the loads of block b are issued DP_PF
        // blocks ahead (slot = b % DP_PF is a compile-time constant: the loop is unrolled DP_PF times and every body issues the
        // same loads — past the end the last block again — so the wait for a slot leaves the other slots in flight).
        int m = 0;             // MIXED: this lane's channel's polarity mask
        if constexpr (MIXED) m = pol_mask(pol, c, flags);
        constexpr int NV = F32 ? 4 : 2, SPV = F32 ? 4 : 8;   // 16-byte registers per sixteen samples; samples per register
        int4 pa[DP_PF][NV], pb[DP_PF][NV];
        auto issue = [&](uint32_t b, int slot) {   // lane (g, bin) converts samples [16 bin, 16 bin + 16) of its channel's block
            const XT* p = xr + (size_t)min(b, NB - 1u) * DP_BLK + 16 * bin;
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                pa[slot][q] = *reinterpret_cast<const int4*>(p + SPV * q);
                pb[slot][q] = *reinterpret_cast<const int4*>(p + SPV * q - 120);
            }
        };
#pragma unroll
        for (int j = 0; j < DP_PF; ++j) issue((uint32_t)j, j);
        auto lo = [](int w) { return (int)(int16_t)(w & 0xFFFF); };
        auto hi = [](int w) { return w >> 16; };
        for (uint32_t i0 = 0; i0 < NI; i0 += DP_PF) {
#pragma unroll
            for (int slot = 0; slot < DP_PF; ++slot) {
                const uint32_t i = i0 + (uint32_t)slot;
                {
                    float4 o[4];
                    if constexpr (F32) {
                        const int sm = MIXED ? (m & (int)0x80000000u) : (INVERT ? (int)0x80000000u : 0);
                        auto neg = [&](int w) { return __int_as_float(w ^ sm); };
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int4 a = pa[slot][q], d = pb[slot][q];
                            o[q] = make_float4(neg(a.x) - neg(d.x), neg(a.y) - neg(d.y), neg(a.z) - neg(d.z), neg(a.w) - neg(d.w));
                        }
                    } else
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        int4 a = pa[slot][q], d = pb[slot][q];
                        if constexpr (MIXED) { a = pol_word4(a, m); d = pol_word4(d, m); }
                        const v2f u0 = dcd_scale2<INVERT>(lo(a.x), hi(a.x)) - dcd_scale2<INVERT>(lo(d.x), hi(d.x));
                        const v2f u1 = dcd_scale2<INVERT>(lo(a.y), hi(a.y)) - dcd_scale2<INVERT>(lo(d.y), hi(d.y));
                        const v2f u2 = dcd_scale2<INVERT>(lo(a.z), hi(a.z)) - dcd_scale2<INVERT>(lo(d.z), hi(d.z));
                        const v2f u3 = dcd_scale2<INVERT>(lo(a.w), hi(a.w)) - dcd_scale2<INVERT>(lo(d.w), hi(d.w));
                        o[2 * q] = make_float4(u0.x, u0.y, u1.x, u1.y);
                        o[2 * q + 1] = make_float4(u2.x, u2.y, u3.x, u3.y);
                    }
                    issue(i + DP_PF, slot);   // this slot's registers are free again: block i + DP_PF goes in flight
                    if (i < NB && !(flags & 16u)) {
                        float* wrow = &dbuf[i & 1u][g][16 * bin];
#pragma unroll
                        for (int q = 0; q < 4; ++q) *reinterpret_cast<float4*>(wrow + 4 * q) = o[q];
                    }
                    dp_handover();
                }
            }
        }
    } else if (role == 1) {
        // ---- R: the recurrence and nothing else
        v2f X = v2f{st->xr[bin], st->xi[bin]};
        const v2f cc = bin ? v2f{k.c1r, k.c1i} : v2f{k.c0r, k.c0i};
        const v2f cs = v2f{-cc.y, cc.x};
        auto step = [&](float delta) {
            const float a = X.x + delta;
            const v2f m1 = v2f{a, a} * cc;          // (ac, ad)
            const v2f m2 = v2f{X.y, X.y} * cs;      // (-bd, bc)
            X = m1 + m2;                            // (ac - bd, ad + bc)
        };
        for (uint32_t i = 0; i < NI; ++i) {
            if (i >= 1u && i <= NB && !(flags & 32u)) {
                const uint32_t b = i - 1u;
                const float* drow = &dbuf[b & 1u][g][0];
                float4* out = &xb[b & 1u][0][lane];
                float d[DP_BLK];
#pragma unroll
                for (int u = 0; u < DP_BLK / 4; ++u) {
                    const float4 v = *reinterpret_cast<const float4*>(drow + 4 * u);
                    d[4 * u] = v.x; d[4 * u + 1] = v.y; d[4 * u + 2] = v.z; d[4 * u + 3] = v.w;
                }
#pragma unroll
                for (int u = 0; u < DP_BLK; u += 2) {
                    step(d[u]); const v2f x0 = X;
                    step(d[u + 1]);
                    out[(u / 2) * 64] = make_float4(x0.x, x0.y, X.x, X.y);
                }
            }
            dp_handover();
        }
        if (live) { st->xr[bin] = X.x; st->xi[bin] = X.y; }
    } else {
        // ---- A0 / A1: norms and running sums; A0 (role 2) owns the sums restarted at ticks = 0..3 (mod 5), A1 the one restarted
        // at ticks = 4 (mod 5) and the one that runs from the stream start
        const bool a0 = role == 2;
        v2f s01 = a0 ? v2f{st->acc[0][bin], st->acc[1][bin]} : v2f{st->acc[4][bin], st->acc[5][bin]};
        v2f s23 = a0 ? v2f{st->acc[2][bin], st->acc[3][bin]} : v2f{0.f, 0.f};
        uint32_t phase = (uint32_t)(pos0 % TICK);
        uint64_t tick = pos0 / TICK;
        uint32_t row = 0;
        float* tab = table + (size_t)c * ticks_cap * 12 + bin * 6;
        const bool skip = flags & (a0 ? 64u : 128u);
        for (uint32_t i = 0; i < NI; ++i) {
            if (i >= 2u && i < NB + 2u && !skip) {
                const uint32_t b = i - 2u;
                const float4* in = &xb[b & 1u][0][lane];
                if (phase == 0) {   // the sum that restarts with this tick
                    const uint32_t j = (uint32_t)(tick % 5);
                    if (a0) { if (j == 0) s01.x = 0.f; if (j == 1) s01.y = 0.f; if (j == 2) s23.x = 0.f; if (j == 3) s23.y = 0.f; }
                    else if (j == 4) s01.x = 0.f;
                }
                auto acc = [&](float re, float im) {
                    const v2f xx = {re, im};
                    const v2f p = xx * xx;
                    const float nrm = p.x + p.y;
                    const v2f nn = {nrm, nrm};
                    s01 = s01 + nn;
                    if (a0) s23 = s23 + nn;
                };
#pragma unroll
                for (int u = 0; u < DP_BLK / 2; ++u) {
                    const float4 v = in[u * 64];
                    acc(v.x, v.y);
                    acc(v.z, v.w);
                }
                phase += DP_BLK;
                if (phase == TICK) {
                    if (live) {
                        float* o = tab + (size_t)row * 12;
                        if (a0) {
                            *reinterpret_cast<float2*>(o) = make_float2(s01.x, s01.y);
                            *reinterpret_cast<float2*>(o + 2) = make_float2(s23.x, s23.y);
                        } else {
                            *reinterpret_cast<float2*>(o + 4) = make_float2(s01.x, s01.y);
                        }
                    }
                    phase = 0; ++tick; ++row;
                }
            }
            dp_handover();
        }
        if (live) {
            if (a0) { st->acc[0][bin] = s01.x; st->acc[1][bin] = s01.y; st->acc[2][bin] = s23.x; st->acc[3][bin] = s23.y; }
            else { st->acc[4][bin] = s01.x; st->acc[5][bin] = s01.y; }
        }
    }
