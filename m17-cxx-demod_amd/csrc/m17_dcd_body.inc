// The body of dcd_kernel<INVERT> and dcd_mixed_kernel (m17_frontend_kernels.hpp): included into both, inside the kernel's braces.
// The including kernel names: INVERT, MIXED (constants); pol (MIXED only: the polarity table; a channel's polarity is its entry XOR bit 0 of flags); XT, the
// sample type of the input slab: int16_t, or float (a float stream: nothing is scaled, negation is a sign-bit XOR, under the lane's mask in the mixed form).
    constexpr bool F32 = std::is_same<XT, float>::value;
    __shared__ __attribute__((aligned(16))) float dl_all[DCD_WPB][DCD_CPW][DCD_PITCH];
    float (*dl)[DCD_PITCH] = dl_all[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
    const int g = lane >> 1, bin = lane & 1;
    uint32_t c = (blockIdx.x * DCD_WPB + (threadIdx.x >> 6)) * DCD_CPW + g;
    const bool live = c < C;   // lanes beyond the last channel shadow it and never store
    if (!live) c = C - 1;
    const XT* xr = x + (size_t)c * xpitch + XPRE;
    DcdState* st = state + c;
    // MIXED: the channels' polarities as a LANE MASK in a scalar pair; the per-lane mask (0 / -1) is formed from it where samples are converted — a
    // register kept across the recurrence cost the kernel its seventh wave per SIMD (74 VGPRs against 72)
    uint64_t inv_lanes = 0;
    if constexpr (MIXED) inv_lanes = __ballot(pol_mask(pol, c, flags) != 0);
    auto lane_mask = [&]() -> int {
        uint64_t il = inv_lanes;
        asm volatile("" : "+s"(il));   // (formed anew at every use: not hoisted out of the block loop)
        return __builtin_amdgcn_inverse_ballot_w64(il) ? -1 : 0;
    };
    DcdLane s;
    s.X = v2f{st->xr[bin], st->xi[bin]};
    s.cc = bin ? v2f{k.c1r, k.c1i} : v2f{k.c0r, k.c0i};
    s.cs = v2f{-s.cc.y, s.cc.x};
    s.a01 = v2f{st->acc[0][bin], st->acc[1][bin]};
    s.a23 = v2f{st->acc[2][bin], st->acc[3][bin]};
    s.a45 = v2f{st->acc[4][bin], st->acc[5][bin]};
    float* tab = table + (size_t)c * ticks_cap * 12 + bin * 6;
    const float* mydl = dl[g];
    uint32_t phase = (uint32_t)(pos0 % TICK);  // position inside the current tick (wave-uniform)
    uint64_t tick = pos0 / TICK;
    uint32_t row = 0;
    auto lds_sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    };
    auto tick_begin = [&] {  // the sum that restarts with this tick
        const uint32_t j = (uint32_t)(tick % 5);
        if (j == 0) s.a01.x = 0.f;
        if (j == 1) s.a01.y = 0.f;
        if (j == 2) s.a23.x = 0.f;
        if (j == 3) s.a23.y = 0.f;
        if (j == 4) s.a45.x = 0.f;
    };
    auto tick_end = [&] {
        if (live) {
            float* o = tab + (size_t)row * 12;
            *reinterpret_cast<float2*>(o) = make_float2(s.a01.x, s.a01.y);
            *reinterpret_cast<float2*>(o + 2) = make_float2(s.a23.x, s.a23.y);
            *reinterpret_cast<float2*>(o + 4) = make_float2(s.a45.x, s.a45.y);
        }
        phase = 0; ++tick; ++row;
    };
    auto one_sample = [&](uint32_t t) {  // generic path: head / tail of a run; x[n] and x[n-120] are one packed pair
        if (phase == 0) tick_begin();
        if constexpr (F32) {
            int sm = INVERT ? (int)0x80000000u : 0;
            if constexpr (MIXED) sm = lane_mask() & (int)0x80000000u;
            const float fn = __int_as_float(__float_as_int(xr[t]) ^ sm), fd = __int_as_float(__float_as_int(xr[(int64_t)t - 120]) ^ sm);
            dcd_step(s, fn - fd);
        } else {
        int xn = (int)xr[t], xd = (int)xr[(int64_t)t - 120];
        if constexpr (MIXED) { const int m = lane_mask(); xn = pol_i16(xn, m); xd = pol_i16(xd, m); }
        const v2f f = dcd_scale2<INVERT>(xn, xd);
        dcd_step(s, f.x - f.y);
        }
        if (++phase == TICK) tick_end();
    };

    uint32_t t = 0;
    while (t < T && (phase % DCD_BLK) != 0) { one_sample(t); ++t; }   // head: up to a block boundary of the tick
    // whole blocks: lane (g, bin) converts samples [HALF bin, HALF bin + HALF) of its channel's block
    if (t + DCD_BLK <= T) {
        constexpr int HALF = DCD_BLK / 2, NQ = HALF / 8;
        constexpr int NV = F32 ? 2 * NQ : NQ;   // 16-byte registers per half block
        int4 pa[NV], pb[NV];
        auto issue = [&](uint32_t t0) {
            constexpr int SPV = F32 ? 4 : 8;    // samples per 16-byte register
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const XT* p = xr + (size_t)t0 + HALF * bin + SPV * q;
                pa[q] = *reinterpret_cast<const int4*>(p);
                pb[q] = *reinterpret_cast<const int4*>(p - 120);
            }
        };
        auto lo = [](int w) { return (int)(int16_t)(w & 0xFFFF); };
        auto hi = [](int w) { return w >> 16; };
        issue(t);
        for (; t + DCD_BLK <= T; t += DCD_BLK) {
            float* wrow = dl[g] + HALF * bin;
            int m = 0;
            if constexpr (MIXED) m = lane_mask();
            if constexpr (F32) {
                const int sm = MIXED ? (m & (int)0x80000000u) : (INVERT ? (int)0x80000000u : 0);
                auto neg = [&](int w) { return __int_as_float(w ^ sm); };
#pragma unroll
                for (int q = 0; q < NV; ++q) {
                    const int4 a = pa[q], d = pb[q];
                    *reinterpret_cast<float4*>(wrow + 4 * q) = make_float4(neg(a.x) - neg(d.x), neg(a.y) - neg(d.y), neg(a.z) - neg(d.z), neg(a.w) - neg(d.w));
                }
            } else
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                int4 a = pa[q], d = pb[q];
                if constexpr (MIXED) { a = pol_word4(a, m); d = pol_word4(d, m); }
                const v2f u0 = dcd_scale2<INVERT>(lo(a.x), hi(a.x)) - dcd_scale2<INVERT>(lo(d.x), hi(d.x));
                const v2f u1 = dcd_scale2<INVERT>(lo(a.y), hi(a.y)) - dcd_scale2<INVERT>(lo(d.y), hi(d.y));
                const v2f u2 = dcd_scale2<INVERT>(lo(a.z), hi(a.z)) - dcd_scale2<INVERT>(lo(d.z), hi(d.z));
                const v2f u3 = dcd_scale2<INVERT>(lo(a.w), hi(a.w)) - dcd_scale2<INVERT>(lo(d.w), hi(d.w));
                *reinterpret_cast<float4*>(wrow + 8 * q) = make_float4(u0.x, u0.y, u1.x, u1.y);
                *reinterpret_cast<float4*>(wrow + 8 * q + 4) = make_float4(u2.x, u2.y, u3.x, u3.y);
            }
            lds_sync();
            if (t + 2 * DCD_BLK <= T) issue(t + DCD_BLK);   // in flight while the recurrence below runs
            if (phase == 0) tick_begin();
            float d[DCD_BLK];
#pragma unroll
            for (int u = 0; u < DCD_BLK / 4; ++u) {
                const float4 v = *reinterpret_cast<const float4*>(mydl + 4 * u);
                d[4 * u] = v.x; d[4 * u + 1] = v.y; d[4 * u + 2] = v.z; d[4 * u + 3] = v.w;
            }
#pragma unroll
            for (int u = 0; u < DCD_BLK; ++u) dcd_step(s, d[u]);
            phase += DCD_BLK;
            if (phase == TICK) tick_end();
            lds_sync();
        }
    }
    for (; t < T; ++t) one_sample(t);  // tail
    if (live) {
        st->xr[bin] = s.X.x; st->xi[bin] = s.X.y;
        st->acc[0][bin] = s.a01.x; st->acc[1][bin] = s.a01.y; st->acc[2][bin] = s.a23.x;
        st->acc[3][bin] = s.a23.y; st->acc[4][bin] = s.a45.x; st->acc[5][bin] = s.a45.y;
    }
