// K5: the per-channel sequential glue — reference a3, a5, a6, a8 (decision half), a9-a13, a19:
// Correlator::sample / SyncWord / outer_symbol_levels (Correlator.h), DataCarrierDetect::update,
// ClockRecovery + KalmanFilter, FreqDevEstimator, SymbolEvm, llr<float,4>, M17Framer and the
// M17Demodulator state machine (M17Demodulator.h:233-753) — plus K4 (frame decode, wave-cooperative).
//
// Mapping: ONE WAVE PER CHANNEL.  Everything here is a recurrence or a state machine per channel, so there is
// no data parallelism across time; what the hardware charges for is wave instructions (four waves share a SIMD's
// 1.85 ns per instruction, uniform "scalar" float work included) and divergence.  With one wave per channel 4096
// channels are 4096 waves = 4 per SIMD (the whole chip busy, latencies of one wave hidden by its three neighbours),
// the state machine is wave-uniform (every branch is taken by all lanes, untaken code is skipped), the channel's
// state (Hot, Cold) lives in LDS, and the 64 lanes cooperate where a stretch of the stream allows it:
//   * "bulk chunks" of up to 480 samples while nothing but feeding happens (initialisation, the 77 quiet samples
//     after a frame, SYNC_WAIT, the inside of a payload frame): samples come from a coalesced LDS window prefetched
//     512 samples ahead, the <= 48 payload symbols of the chunk are normalised / sliced by 64 lanes at once, the
//     running EVM is folded sequentially, the correlator ring is refilled from the chunk's tail;
//   * search chunks (UNLOCKED) and sync-window chunks (*_SYNC states): lane k evaluates the sync-word trigger of
//     sample k, ballots find the first sample that needs the single-sample path;
//   * the frame decode uses 16 lanes as the 16 trellis states (m17_decode_device.hpp, viterbi_decode_wave).
// The massively parallel work (K1 FIR), the state-machine-independent recurrence (K3 sliding DFT) and the
// correlator's limit filter (K2, speculatively: m17_gate_kernel.hpp) run as their own passes; this kernel consumes
//   ybuf[c][t]    the matched-filter output, valid wherever the last 149 FIR inputs were consecutive samples
//   dcd table     the sequential carrier-detect sums for every possible segment (see K3)
//   hbuf[c][t]    the limit-filter history after every fed sample — until this kernel forces an unlock K2 could not
//                 foresee; from there to the end of the segment it carries the filter itself
// The reference gates the FIR and the correlator with the carrier detect: their input is the
// concatenation of gated-on runs.  Runs start and end on tick boundaries and last >= 960 samples, so only the
// first 148 outputs of a run see samples of the previous run; for those the FIR is recomputed cooperatively from a
// 149-sample snapshot taken when the previous run ended and patched into ybuf in place (rare).
//
// All 64 lanes hold the same scalar state and execute the single-sample path redundantly; stores of state are
// issued by every lane with identical values (no cross-lane ordering is relied on).
#pragma once

#include "m17_common.hpp"
#include "m17_decode_device.hpp"
#include "m17_frontend_kernels.hpp"
#include "m17_state.hpp"

namespace m17 {

#ifndef M17_WAVE_MINW
#define M17_WAVE_MINW 5  // waves per SIMD the register budget is sized for: 96 VGPRs, so that four waves of this kernel (4096 channels
                         // resident at once) leave 128 registers of every SIMD to the kernels that run beside it (K2, K1)
#endif
constexpr int WV_WIN = 1024;                                            // LDS window of upcoming matched-filter samples (circular)
constexpr int WV_PF = 512;                                              // prefetch granule: 8 samples per lane in flight
constexpr int WV_YCH = 480;                                             // largest bulk chunk (<= WV_PF)
constexpr int WV_TAB_WORDS = 64;                                        // per block: llr edges (the decoder's source maps and the FIR taps stay in global memory)
constexpr int WV_WAVE_WORDS = 80 + 40 + 92 + 122 + 8 + 8 + WV_WIN + 488 + 64 + 48; // per wave: ring, sync samples, llr, hist, outb, lsf, sample window, decoder soft bits (+ EVM terms), hot state, cold state
constexpr int wave_lds_words(int waves_per_block) { return WV_TAB_WORDS + waves_per_block * WV_WAVE_WORDS; }

// M17FrameDecoder::operator() on the wave's completed frame; returns (viterbi_cost, decoder state)
__device__ __forceinline__ uint2 nf_decode_wave(const DecodeTables* tb, DecodeLds L, int wl, uint32_t sync_type, M17_LDS Cold* cd, uint32_t cost_in,
                                             FrameRec* rec_base, uint32_t rec_cap, uint32_t channel, uint64_t pos, uint32_t* overflow, uint32_t* defer)
{
    DecoderRegs D{cd->dec_state, cd->lich_segments, cd->stale401};
    RecSink S{rec_base, rec_cap, nullptr, nullptr, channel, pos, sync_type, overflow, defer};
    uint32_t n_run = cd->n_run, seq = cd->seq;
    const uint32_t cost = decode_frame<true>(tb, L, 0, sync_type, D, cost_in, S, n_run, seq, wl);
    cd->dec_state = D.state; cd->lich_segments = D.lich_segments; cd->stale401 = D.stale401;
    cd->n_run = n_run; cd->seq = seq;
    return make_uint2(cost, D.state);
}

// Correlator::sample x (to - from) for ONE channel as a tight pass (Correlator.h:43-49, IirFilter.h:26-42): the limit filter's
// history after every sample of [from, to) goes to the channel's hbuf row, exactly where K2 would have left it.  Used by a wave whose
// gate has left K2's replay (a forced dcd.unlock(), M17Demodulator.h:396-404, 470-478 ...): instead of carrying the recurrence sample
// by sample through every chunk of the state machine, the wave serves itself one stretch of certainly-fed samples at a time and
// then runs its usual hbuf-reading paths over it.  256-sample blocks staged in LDS (B, replaced in place by the history values),
// the next block's loads in flight during the recurrence.  h[3] = history after sample from - 1 on entry, after to - 1 on exit.
struct Hist3 { float h0, h1, h2; };
typedef float m17_v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ Hist3 nf_serve_limit(const float* yr, float* hr, M17_LDS float* B, uint32_t from, uint32_t to, float h0, float h1, float h2)
{
    const uint32_t l = threadIdx.x & 63u;
    // Both rows through buffer descriptors that end at `to`: a load beyond it returns 0, a store beyond it is dropped — three loads and three
    // stores per block on EVERY path, so that the wait for a block's samples can leave the previous block's stores in flight (with the
    // bounds as branches the wait-count insertion could only wait for everything: a store round trip per block).
    const __amdgpu_buffer_rsrc_t ysrc = __builtin_amdgcn_make_buffer_rsrc((void*)yr, 0, (int)(to * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t hdst = __builtin_amdgcn_make_buffer_rsrc((void*)hr, 0, (int)(to * 4u), 0x00020000);
    constexpr uint32_t BLK = TICK;   // one block = what iir_tick_in_place runs over (192 samples; B holds them + 16 bytes of padding + 32 readable)
    float nx[3];
    auto load = [&](uint32_t b) {
#pragma unroll
        for (int j = 0; j < 3; ++j) nx[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ysrc, (int)((b + l + 64u * j) * 4u), 0, 0));
    };
    load(from);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 3; ++j) __builtin_amdgcn_raw_buffer_store_b32(0, hdst, 0x7FFF0000 + 256 * j, 0, 0);   // (three dropped stores: the first block's wait sees what every later one sees)
    for (uint32_t b = from; b < to; b += BLK) {
        const uint32_t n = min(BLK, to - b);
#pragma unroll
        for (int j = 0; j < 3; ++j) B[l + 64u * j] = nx[j];
        wave_lds_sync();
        load(b + BLK);   // (beyond `to`: zeros, not used)
        if (l == 0u) {
            // The recurrence is one value per sample for the whole wave: ONE lane runs it.  A whole block as K2's tick does (m17_frontend_kernels.hpp,
            // iir_tick_in_place: one asm statement, three instructions per sample, the samples replaced by their history values in their registers, the
            // LDS reads two groups ahead, the writes left in flight) — a wave that serves itself is what its launch waits for (up to 2.2 ms of a launch
            // whose median wave needs 0.45: gpurun_out/r6/wave_times_*.txt), and the compiler's form of this loop (eight samples per pass, waits for its
            // own LDS writes) ran at 16 ns per sample alone and 33 in the crowd.
            if (n == BLK) {
                iir_tick_in_place((uint32_t)(uintptr_t)B, h0, h1, h2);
            } else {
                float m2 = IirCoef::a2 * h1;
                for (uint32_t i = 0; i < n; ++i) {
                    const float hn = iir_advance_pk(fabsf(B[i]), h0, m2);
                    h2 = h1; h1 = h0; h0 = hn;
                    B[i] = hn;
                }
            }
        }
        wave_lds_sync();
#pragma unroll
        for (int j = 0; j < 3; ++j) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, B[l + 64u * j]), hdst, (int)((b + l + 64u * j) * 4u), 0, 0);
        wave_lds_sync();
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // the history values are read back by this wave (other lanes, later loads)
    // (lane 0 holds the history: the caller's scalar registers take the first lane's values)
    return Hist3{__builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, h0))),
                 __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, h1))),
                 __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, h2)))};
}

// (the kernel itself, demod_wave_kernel<XT, WPB, PROF, TIMED, KORDER>: m17_wave_demod_kernel.hpp)

}  // namespace m17
