// The body of fir_rrc150_skew_kernel<INVERT> and fir_rrc150_skew_mixed_kernel (m17_frontend_kernels.hpp): included into both, inside the kernel's braces.
// The including kernel names: INVERT, MIXED (constants); pol, flip (MIXED only: the polarity table and bit 0 of the call's flags); XT, the sample type of
// the input slab: int16_t, or float (a float stream: samples in the reference's units, 32 bytes per eight-sample chunk, staged as they are, negated by a
// sign-bit XOR — under the item's mask in the mixed form; no dcd_scale2).
    // first_needed (may be null): per channel, the first sample of this slab the carrier can be on for (gate_forecast_kernel): tiles that end
    // before it are skipped
    __shared__ __attribute__((aligned(16))) float win[FS_LDS_FLOATS];
    const int tid = threadIdx.x;
    typedef int v4i __attribute__((ext_vector_type(4)));
    constexpr int NCH = (FS_WIN + 7) / 8;             // 531 chunks of eight samples
    constexpr int CPT = (NCH + FS_THREADS - 1) / FS_THREADS;   // 3 per thread (the third for 19 threads only)
    constexpr bool F32 = std::is_same<XT, float>::value;
    // float rows: the two whole chunks of a lane are 32 bytes each; the last 152 samples of the window (chunks 512 .. 530, which the int16 form gives
    // to nineteen lanes as a third chunk) go one sample per lane — 17 registers in flight instead of 24, which the 128 of four workgroups per CU do not hold
    constexpr int FS_LAST = FS_WIN - 16 * FS_THREADS; // 152
    static_assert(FS_LAST > 0 && FS_LAST <= FS_THREADS && CPT == 3, "the float form's split of the window");
    v4i pre[F32 ? 4 : CPT];
    int pre_last = 0;
    int m = 0;                                        // MIXED: the polarity mask of the item being staged
    // the int16 input of an item: chunk k <-> window samples 8k .. 8k + 7 <-> times t0 - 152 + 8k ...; beyond the slab's end: zero
    auto fetch = [&](uint32_t item) {
        const uint32_t c = item / tiles, tile = item - c * tiles;
        const XT* xr = x + (size_t)c * xpitch + XPRE;
        const int64_t w0 = (int64_t)tile * FS_TILE - FS_WOFF;
#pragma unroll
        for (int q = 0; q < CPT; ++q) {
            const int k = tid + q * FS_THREADS;
            const int64_t t = w0 + 8 * k;
            v4i v = {0, 0, 0, 0};
            if constexpr (F32) {
                if (q < 2) {                          // (k < NCH for both)
                    v4i v2 = {0, 0, 0, 0};
                    if (t + 8 <= (int64_t)T) {
                        v = *reinterpret_cast<const v4i*>(xr + t);
                        v2 = *reinterpret_cast<const v4i*>(xr + t + 4);
                    } else {                          // the slab ends inside this chunk (once per channel at most): sample by sample
                        uint32_t w[8];
#pragma unroll
                        for (int h = 0; h < 8; ++h) w[h] = t + h < (int64_t)T ? __float_as_uint(xr[t + h]) : 0u;
                        v = v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
                        v2 = v4i{(int)w[4], (int)w[5], (int)w[6], (int)w[7]};
                    }
                    pre[2 * q] = v; pre[2 * q + 1] = v2;
                } else {
                    const int64_t tl = w0 + 16 * FS_THREADS + tid;
                    pre_last = (tid < FS_LAST && tl < (int64_t)T) ? (int)__float_as_uint(xr[tl]) : 0;
                }
            } else {
            if (k < NCH) {
                if (t + 8 <= (int64_t)T) v = *reinterpret_cast<const v4i*>(xr + t);
                else {                                // the slab ends inside this chunk (once per channel at most): sample by sample
                    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
                    for (int h = 0; h < 8; ++h)
                        if (t + h < (int64_t)T) w[h >> 1] |= (uint32_t)(uint16_t)xr[t + h] << (16 * (h & 1));
                    v = v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
                }
            }
            pre[q] = v;
            }
        }
    };
    auto stage = [&] {
#pragma unroll
        for (int q = 0; q < CPT; ++q) {
            const int k = tid + q * FS_THREADS;
            int sm = INVERT ? (int)0x80000000u : 0;   // (float rows) the sign bit where the sample is negated
            if constexpr (F32 && MIXED) sm = m & (int)0x80000000u;
            if constexpr (F32) if (q == 2) {          // the window's last 152 samples, one per lane
                const int j = 16 * FS_THREADS + tid;
                if (tid < FS_LAST) win[FS_PADF + j + 2 * (j >> 4)] = __int_as_float(pre_last ^ sm);
                continue;
            }
            if (k < NCH) {
                float* dst = win + FS_PADF + 8 * k + 2 * (k >> 1);   // sample j = 8k at word j + 2 (j >> 4)
                if constexpr (F32) {
#pragma unroll
                    for (int h = 0; h < 4; ++h) {
                        const v4i r = pre[2 * q + (h >> 1)];
                        const int a = ((h & 1) ? r[2] : r[0]) ^ sm, b = ((h & 1) ? r[3] : r[1]) ^ sm;
                        *reinterpret_cast<v2f*>(dst + 2 * h) = v2f{__int_as_float(a), __int_as_float(b)};
                    }
                } else
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    int w = pre[q][h];
                    if constexpr (MIXED) w = pol_word(w, m);
                    const v2f f = dcd_scale2<INVERT>((int)(int16_t)(w & 0xFFFF), w >> 16);
                    *reinterpret_cast<v2f*>(dst + 2 * h) = f;
                }
            }
        }
    };
    auto next_item = [&](uint32_t it) {               // the first item from `it` on (stride = the grid) that is not skipped
        if (first_needed) {
            while (it < items) {
                const uint32_t c = it / tiles, tile = it - c * tiles;
                if ((uint64_t)(tile + 1u) * FS_TILE > (uint64_t)first_needed[c]) break;
                it += gridDim.x;
            }
        }
        return it;
    };
    uint32_t item = next_item(blockIdx.x);
    if (item < items) fetch(item);
    const float* lbase = win + FS_PADF + 18 * tid;    // lane-relative element e at lbase[fs_off(e)]
    while (item < items) {
        const uint32_t c = item / tiles, tile = item - c * tiles;
        const uint32_t following = next_item(item + gridDim.x);
        // MIXED: consecutive items of a workgroup may differ in polarity.  The window is staged under the polarity of the item it is staged FOR — this
        // one, about to be computed; what goes in flight in `pre` during its tap loop is raw int16 and belongs to the item after.
        if constexpr (MIXED) m = pol_mask(pol, c, flip);
        stage();
        dp_handover();                                // (LDS only: no wait for the stores of the item before)
        if (following < items) fetch(following);      // in flight during the tap loop
        v2f acc[8], ring[16];
        v2f late = {0.0f, 0.0f};                      // pair 7's product of the step before (added one step late: +0 first, harmless)
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = v2f{0.0f, 0.0f};
        // the ring before step 0: the pairs that positions in front of the entry point would have loaded (elements 142 .. 167)
        static_for<0, 13>([&](auto kc) {
            constexpr int e = 142 + 2 * decltype(kc)::value;
            ring[(e & 31) >> 1] = *reinterpret_cast<const v2f*>(lbase + fs_off(e));
        });
        const float* lb = lbase + 36;                 // body b reads from lbase - 36 b: b = -1 first
#pragma unroll 1
        for (int bi = 0; bi < FS_NBODY; ++bi) {
            const float* tb = tab + bi * FS_TAB;      // wave-uniform: scalar loads
            auto half = [&](auto lo_c, auto hi_c) {
                static_for<decltype(lo_c)::value, decltype(hi_c)::value>([&](auto pc) {
                    constexpr int p = decltype(pc)::value;
                    // step s = 32 b + 22 + p; pair q reads element e = 153 + 2q - s = 131 - 32 b + 2q - p: slot (131 + 2q - p) mod 32
                    if constexpr ((p & 1) == 0) {     // the pair of elements first needed twelve steps from now
                        constexpr int e = 118 - p;    // (minus 32 b: folded into lb)
                        ring[(e & 31) >> 1] = *reinterpret_cast<const v2f*>(lb + fs_off(e));
                    }
                    const v2f tp = (p & 1) ? *reinterpret_cast<const v2f*>(tb + 32 + p - 1) : *reinterpret_cast<const v2f*>(tb + p);
                    v2f pr[8];                        // the eight products first, then the eight additions: no dependent neighbours
                    static_for<0, 8>([&](auto qc) {
                        constexpr int q = decltype(qc)::value;
                        constexpr int slot = (131 + 2 * q - p) & 31;
                        pr[q] = fs_tap_pair_times<slot & 1>(tp, ring[slot >> 1]);
                    });
                    // (the compiler counts an asm statement as no wait state at all and pads a reader of ANY asm result that follows a run of
                    //  them with an s_nop: pair 7's addition of the step before goes first — its product is eight real instructions old)
                    acc[7] = acc[7] + late;
#pragma unroll
                    for (int q = 0; q < 7; ++q) acc[q] = acc[q] + pr[q];
                    late = pr[7];
                });
            };
            if (bi > 0) half(std::integral_constant<int, 0>{}, std::integral_constant<int, FS_ENTRY>{});
            half(std::integral_constant<int, FS_ENTRY>{}, std::integral_constant<int, FS_BODY>{});
            lb -= 36;
        }
        acc[7] = acc[7] + late;
        // outputs 16 tid .. 16 tid + 15 of the tile, from the registers
        const uint32_t t = tile * FS_TILE + 16u * (uint32_t)tid;
        float* yo = y + (size_t)c * ypitch + YPRE + t;
        if (t + 16 <= T) {
#pragma unroll
            for (int g = 0; g < 4; ++g) *reinterpret_cast<float4*>(yo + 4 * g) = make_float4(acc[2 * g].x, acc[2 * g].y, acc[2 * g + 1].x, acc[2 * g + 1].y);
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (t + 2 * q < T) yo[2 * q] = acc[q].x;
                if (t + 2 * q + 1 < T) yo[2 * q + 1] = acc[q].y;
            }
        }
        dp_handover();                                // every wave is through with the window before the next item is staged
        item = following;
    }
