// Payload consumer of the STREAM branch (apps/m17-demod.cpp:178-205, 321-323: demodulate_audio): the codec2 payloads of a run's
// voice records next to each other per channel, a mark byte per slot, and a per-channel call log (include/m17hip.h, m17hip_tune key 34).
// codec2 itself is host work; what is done here is what a host would otherwise do record by record on one thread.
//
// One wave per channel, four channels per 256-lane workgroup, no workgroup barrier and no LDS: the wave takes 64 records per pass,
// lane i reads record i.  Everything a lane needs of its own record comes with three aligned 128-bit loads (bytes 0..47 of the 64);
// payload bytes 2..17 lie at byte 26 of the record — two bytes off a dword — so the 16 codec2 bytes are funnel-shifted out of five
// dwords and leave as ONE aligned 128-bit store.  Voice records are found by __ballot; a lane's slot is the popcount of the ballot
// below it plus the channel's running count.  What a voice lane must know of the records before it (is a call open, has it a voice
// frame, which frame number came last) is a property of its nearest predecessor among the LSF and voice lanes: one __shfl to the
// previous set bit of the ballot, the carried state for the first.  Calls open and close at the pass's few BOUNDARY lanes (LSF |
// accepted EOS | a voice lane that finds no call open), which one uniform loop walks in order; the sums of the voice lanes between two
// boundaries are differences of two wave-wide inclusive prefix sums (cost, lost) and popcounts of masked ballots (frames, blanked).
// The channel's state is read once and written once (lane 0).  Nothing orders the output but (channel, seq): a closed call goes to
// slot `calls closed by this channel in this run` of the channel's own row of the call store.
#pragma once

#include "m17_common.hpp"

namespace m17 {

constexpr uint32_t VOICE_CPB = 4;   // channels (waves) per workgroup

// A channel's open call and what the next voice frame is compared with; carried from run to run.
struct VoiceState {
    uint32_t open;       // bit 0: a call is open, bit 1: it began with an LSF record
    uint32_t seq;        // calls this channel has closed since its reset
    uint32_t prev_fn;    // frame number of the call's last voice frame (valid while frames > 0)
    uint32_t pad;
    uint32_t start_lo, start_hi, end_lo, end_hi;
    uint32_t cost_sum, frames, blanked, lost;
    uint32_t lsf[8];     // 30 bytes + 2 of padding (zero)
};
static_assert(sizeof(VoiceState) == 80, "VoiceState layout");

struct CallRec {         // = m17_call_rec
    uint32_t channel, seq;
    uint64_t start_pos, end_pos;
    uint32_t cost_sum, frames, blanked, lost;
    uint8_t has_lsf, close;
    uint8_t lsf[30];
};
static_assert(sizeof(CallRec) == 72, "m17_call_rec layout");

struct VoiceParams {
    const FrameRec* recs; uint32_t rec_cap; const uint32_t* rec_count;   // [C][rec_cap] records, rec_count[c] of them used (cut at rec_cap)
    VoiceState* state; uint32_t C;
    uint8_t* audio;      // [C][room][16]
    uint8_t* marks;      // [C][room]
    uint32_t* counts;    // [C] voice records of the channel in this run (may exceed room: the slots that fit are written)
    uint32_t room;
    CallRec* calls;      // [C][call_room]
    uint32_t* call_counts;   // [C] calls the channel closed in this run (may exceed call_room)
    uint32_t call_room;
    uint32_t channel_base;
};

__device__ __forceinline__ uint32_t voice_lane_u32(uint32_t v, uint32_t lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)__builtin_amdgcn_readfirstlane((int)lane)); }
__device__ __forceinline__ uint32_t voice_scan_add(uint32_t v, uint32_t lane)   // inclusive prefix sum over the wave's 64 lanes
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= (uint32_t)d) v += o;
    }
    return v;
}
__device__ __forceinline__ uint64_t voice_range(uint32_t lo, uint32_t hi)   // lanes lo .. hi - 1 (0 <= lo, hi <= 64)
{
    const uint64_t below_hi = hi >= 64u ? ~0ull : ((1ull << hi) - 1ull);
    const uint64_t below_lo = lo >= 64u ? ~0ull : ((1ull << lo) - 1ull);
    return below_hi & ~below_lo;
}

__global__ __launch_bounds__(64 * VOICE_CPB) void voice_log_kernel(const VoiceParams P)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * VOICE_CPB + (threadIdx.x >> 6)));
    if (c >= P.C) return;   // (a whole wave: there is no barrier below)
    const uint32_t n = min(P.rec_count[c], P.rec_cap);
    VoiceState S = P.state[c];   // (a wave-uniform address: every lane holds the same values)
    uint32_t run_voice = 0, run_calls = 0;
    const uint64_t lane_bit = 1ull << lane, below = lane_bit - 1ull;
    const FrameRec* row = P.recs + (size_t)c * P.rec_cap;
    CallRec* call_row = P.calls + (size_t)c * P.call_room;

    for (uint32_t base = 0; base < n; base += 64u) {
        const uint32_t r = base + lane;
        uint4 q0 = make_uint4(0, 0, 0, 0), q1 = make_uint4(0, 0xFFu, 0, 0), q2 = make_uint4(0, 0, 0, 0);
        if (r < n) {
            const uint4* w = reinterpret_cast<const uint4*>(row + r);   // (records are 64 bytes in a hipMalloc'ed store: 16-byte aligned)
            q0 = w[0];   // channel, seq, sample_pos
            q1 = w[1];   // cost, type | sync | len | flags, payload 0..7
            q2 = w[2];   // payload 8..23
        }
        const uint32_t type = q1.y & 0xFFu;
        const bool isV = type == 2u, isL = type == 0u;
        const int cost = (int)q1.x;
        const uint32_t fn = (((q1.z & 0xFFu) << 8) | ((q1.z >> 8) & 0xFFu)) & 0x7FFFu;
        const bool eos = isV && cost < 70 && (q1.z & 0x80u);
        const bool blank = isV && cost > 80;
        const uint64_t bV = __ballot(isV), bL = __ballot(isL), bE = __ballot(eos), bB = __ballot(blank);
        if ((bV | bL) == 0ull) continue;

        // ---- what each lane finds in front of it: its nearest predecessor among the LSF and voice lanes, or the carried state
        const uint64_t pm = (bV | bL) & below;
        const uint32_t j = pm ? 63u - (uint32_t)__clzll((long long)pm) : 0u;
        const uint32_t fn_j = (uint32_t)__shfl((int)fn, (int)j, 64);
        bool open_before, voice_before; uint32_t pfn;
        if (pm) {
            const bool pL = (bL >> j) & 1ull, pE = (bE >> j) & 1ull;
            open_before = pL || !pE;
            voice_before = !pL && !pE;
            pfn = fn_j;
        } else {
            open_before = (S.open & 1u) != 0u;
            voice_before = open_before && S.frames != 0u;
            pfn = S.prev_fn;
        }
        const bool first = isV && !voice_before;
        const bool disc = isV && voice_before && fn != ((pfn + 1u) & 0x7FFFu);
        const uint64_t bS = __ballot(isV && !open_before);   // voice lanes that open a call themselves
        const uint32_t lost_i = disc ? ((fn - pfn - 1u) & 0x7FFFu) : 0u;
        const uint32_t Pc = voice_scan_add(isV ? (uint32_t)cost : 0u, lane);
        const uint32_t Pl = voice_scan_add(lost_i, lane);

        // ---- the planes: 16 codec2 bytes (payload 2..17) and the mark byte of every voice lane whose slot exists
        if (isV) {
            const uint32_t slot = run_voice + (uint32_t)__popcll(bV & below);
            if (slot < P.room) {
                uint4 a;
                a.x = (q1.z >> 16) | (q1.w << 16);
                a.y = (q1.w >> 16) | (q2.x << 16);
                a.z = (q2.x >> 16) | (q2.y << 16);
                a.w = (q2.y >> 16) | (q2.z << 16);
                const size_t at = (size_t)c * P.room + slot;
                *reinterpret_cast<uint4*>(P.audio + at * 16u) = a;
                P.marks[at] = (uint8_t)((blank ? 1u : 0u) | (eos ? 2u : 0u) | (first ? 4u : 0u) | (disc ? 8u : 0u));
            }
        }
        run_voice += (uint32_t)__popcll(bV);

        // ---- the call log: a uniform walk over the boundary lanes; the voice lanes between two of them are summed at once
        auto account = [&](uint32_t lo, uint32_t hi) {   // the open call takes the voice lanes lo .. hi - 1
            const uint64_t m = bV & voice_range(lo, hi);
            if (!m) return;
            const uint32_t top = 63u - (uint32_t)__clzll((long long)m);
            S.frames += (uint32_t)__popcll(m);
            S.blanked += (uint32_t)__popcll(bB & m);
            S.cost_sum += voice_lane_u32(Pc, hi - 1u) - (lo ? voice_lane_u32(Pc, lo - 1u) : 0u);
            S.lost += voice_lane_u32(Pl, hi - 1u) - (lo ? voice_lane_u32(Pl, lo - 1u) : 0u);
            S.end_lo = voice_lane_u32(q0.z, top); S.end_hi = voice_lane_u32(q0.w, top);
            S.prev_fn = voice_lane_u32(fn, top);
        };
        auto close_call = [&](uint32_t how) {
            if (run_calls < P.call_room && lane == 0u) {
                CallRec* o = call_row + run_calls;
                o->channel = P.channel_base + c; o->seq = S.seq;
                o->start_pos = ((uint64_t)S.start_hi << 32) | S.start_lo; o->end_pos = ((uint64_t)S.end_hi << 32) | S.end_lo;
                o->cost_sum = S.cost_sum; o->frames = S.frames; o->blanked = S.blanked; o->lost = S.lost;
                o->has_lsf = (uint8_t)((S.open >> 1) & 1u); o->close = (uint8_t)how;
#pragma unroll
                for (int k = 0; k < 30; ++k) o->lsf[k] = (uint8_t)(S.lsf[k >> 2] >> (8 * (k & 3)));
            }
            ++run_calls; ++S.seq; S.open = 0u;
        };
        auto open_call = [&](uint32_t b, bool with_lsf) {
            S.open = with_lsf ? 3u : 1u;
            S.start_lo = S.end_lo = voice_lane_u32(q0.z, b); S.start_hi = S.end_hi = voice_lane_u32(q0.w, b);
            S.cost_sum = S.frames = S.blanked = S.lost = 0u; S.prev_fn = 0u;
#pragma unroll
            for (int k = 0; k < 8; ++k) S.lsf[k] = 0u;
        };
        uint64_t bnd = bL | bE | bS;
        uint32_t lo = 0;
        while (bnd) {
            const uint32_t b = (uint32_t)__builtin_ctzll(bnd);
            bnd &= bnd - 1ull;
            account(lo, b);
            lo = b;
            if ((bL >> b) & 1ull) {          // an LSF record: M17FrameDecoder.h:247-254 / an LSF frame; dump_lsf
                if (S.open & 1u) close_call(2u);
                open_call(b, true);
                // payload 0..29 of lane b: bytes 24..53 of its record (the last six come with one more load, LSF lanes only)
                uint32_t t6 = 0, t7 = 0;
                if (lane == b) { const uint2 t = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint8_t*>(row + base + b) + 48); t6 = t.x; t7 = t.y & 0xFFFFu; }
                S.lsf[0] = voice_lane_u32(q1.z, b); S.lsf[1] = voice_lane_u32(q1.w, b);
                S.lsf[2] = voice_lane_u32(q2.x, b); S.lsf[3] = voice_lane_u32(q2.y, b);
                S.lsf[4] = voice_lane_u32(q2.z, b); S.lsf[5] = voice_lane_u32(q2.w, b);
                S.lsf[6] = voice_lane_u32(t6, b); S.lsf[7] = voice_lane_u32(t7, b);
                continue;
            }
            if ((bS >> b) & 1ull) open_call(b, false);   // a voice frame with no call open: a late join, or what follows an end of stream
            if ((bE >> b) & 1ull) {          // an accepted end of stream: the frame belongs to the call it closes
                account(b, b + 1u);
                lo = b + 1u;
                close_call(1u);
            }
        }
        account(lo, 64u);
    }
    if (lane == 0u) {
        P.state[c] = S;
        P.counts[c] = run_voice;
        P.call_counts[c] = run_calls;
    }
}

__device__ __forceinline__ void fresh_voice_state(VoiceState* state, uint32_t c)
{
    uint32_t* w = reinterpret_cast<uint32_t*>(state + c);
    for (uint32_t k = 0; k < sizeof(VoiceState) / 4; ++k) w[k] = 0u;
}
__global__ void voice_reset_kernel(VoiceState* state, uint32_t C)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    fresh_voice_state(state, c);
}

}  // namespace m17
