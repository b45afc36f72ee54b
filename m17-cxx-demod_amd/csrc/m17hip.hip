// C-ABI implementation (include/m17hip.h) over the HIP kernels.  Host side: context, device slabs,
// constant tables, launches, record compaction, per-kernel HIP-event timing.  gfx950 only.
// Product code: no fallback path of any kind — if a HIP call fails the entry point returns M17HIP_EHIP.
#include "../../include/m17hip.h"

#include "m17_common.hpp"
#include "m17_decode_device.hpp"
#include "m17_frontend_kernels.hpp"
#include "m17_iq_kernels.hpp"
#include "m17_wide_kernels.hpp"
#include "m17_wide2_kernels.hpp"
#include "m17_resample_kernels.hpp"
#include "m17_chan_kernels.hpp"
#include "m17_chan_survey_kernels.hpp"
#include "m17_spectrum_kernels.hpp"
#include "m17_meter_kernels.hpp"
#include "m17_squelch_kernels.hpp"
#include "m17_scan_kernel.hpp"
#include "m17_wide_tx_kernels.hpp"
#include "m17_state.hpp"
#include "m17_wave_demod_kernel.hpp"
#include "m17_gate_kernel.hpp"
#include "m17_mod_kernels.hpp"
#include "m17_parity_kernels.hpp"
#include "m17_voice_kernel.hpp"
#include "m17_gather.hpp"

#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <mutex>
#include <new>
#include <vector>

using namespace m17;

namespace {

enum { KT_FIR = 0, KT_DCD, KT_SEQ, KT_DEC, KT_CORR, KT_COMPACT, KT_GATE, KT_VOICE, KT_IQ, KT_WIDE, KT_WIDE2, KT_CHAN, KT_SURVEY, KT_RESAMPLE, KT_SPECTRUM, KT_WIDE_TX, KT_METER, KT_SQUELCH, KT_SQUELCH_SLOTS, KT_SQUELCH_FLOOR, KT_SCAN, KT_N };

// Device memory (hipMalloc) that gives itself back: the member that names a buffer owns it.  Reads as the pointer it holds (nullptr while
// empty).  It never synchronises: a caller that regrows a buffer which queued work may still read waits for that work first.  A failed
// hipFree (a pointer the runtime does not know, a dead device) drops the pointer all the same — never reused, never freed twice — and is
// recorded in *last_hip where the caller passes one.
template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t size() const { return n_; }   // (elements)
    hipError_t alloc(size_t n)   // n elements in place of what it holds; empty when that fails
    {
        release();
        const hipError_t e = hipMalloc((void**)&p_, n * sizeof(T));
        if (e == hipSuccess) n_ = n; else p_ = nullptr;
        return e;
    }
    hipError_t grow(size_t n, int* last_hip)   // at least n elements: reallocated (its contents lost) only when it holds fewer
    {
        if (n <= n_) return hipSuccess;
        release(last_hip);
        return alloc(n);
    }
    void release(int* last_hip = nullptr)
    {
        if (!p_) return;
        const hipError_t e = hipFree((void*)p_);
        if (e != hipSuccess && last_hip) *last_hip = (int)e;
        p_ = nullptr;
        n_ = 0;
    }
private:
    T* p_ = nullptr;
    size_t n_ = 0;
};
// The half that segment k's parity names of a buffer doubled by segment parity: [2][maxC] entries of `per` elements
template <typename T> T* by_parity(const DevBuf<T>& b, uint32_t k, uint32_t maxC, size_t per = 1) { return b.get() + (size_t)(k & 1u) * maxC * per; }

// A HIP event that destroys itself; reads as the hipEvent_t it holds (nullptr until created).  Movable: the timing pool hands them round.
class Event {
public:
    Event() = default;
    Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event& operator=(Event&& o) noexcept { std::swap(e_, o.e_); return *this; }
    ~Event() { if (e_) (void)hipEventDestroy(e_); }
    operator hipEvent_t() const { return e_; }
    hipError_t create(unsigned flags = hipEventDisableTiming) { return hipEventCreateWithFlags(&e_, flags); }
private:
    hipEvent_t e_ = nullptr;
};

// A small table of words that the host writes and kernels on several streams read (the reset lists, the polarity table).  Two device copies take turns, so
// a write never touches the copy that queued work reads, and the host waits for nothing that is in flight:
//   begin_write   passes the turn to the other copy, waits ON THE HOST for the readers recorded for that one — those of two turns ago — and for its earlier
//                 upload, and hands out its pinned staging buffer; events and buffers (`cap` words) are made the first time a copy is written
//   publish       queues the upload of the first n words on `first`, the stream whose kernels read the table first, and records `ready` there
//   before_read   a kernel on `st` is about to read the table: `st` goes behind `ready` (on `first` that is stream order already)
//   after_read    a kernel of reader `which` has been queued on `st`: `used[which]` is recorded, what the write after next waits for
// An object that is never written owns nothing and waits for nothing.
enum Reader { RD_MAIN = 0, RD_DCD, RD_FIR, RD_REPLAY, RD_FRONT, RD_PAY, RD_N };   // main stream; K3's, K1's, the replay's; a reset list's first kernel; the payload stream
class TurnTable {
public:
    bool live() const { return t_[cur_].live; }                // the current copy holds a published table
    const uint32_t* dev() const { return t_[cur_].dev; }       // (the current copy, on the device)
    size_t words() const { return t_[0].dev.size() + t_[1].dev.size(); }   // device words held by both copies
    hipError_t begin_write(size_t cap, uint32_t** staging)
    {
        if (live()) cur_ ^= 1;   // (a write that failed half way is made again into the same copy)
        Copy& t = t_[cur_];
        t.live = false;
        for (int i = 0; i < RD_N; ++i) {
            if (!t.recorded[i]) continue;
            if (const hipError_t e = hipEventSynchronize(t.used[i])) return e;
            t.recorded[i] = false;
        }
        if (const hipError_t e = t.ready ? hipEventSynchronize(t.ready) : t.ready.create()) return e;   // (the staging buffer is the upload's source)
        if (!t.dev) if (const hipError_t e = t.dev.alloc(cap)) return e;
        if (!t.staging) if (const hipError_t e = hipHostMalloc((void**)&t.staging, cap * 4, hipHostMallocDefault)) return e;
        *staging = t.staging;
        return hipSuccess;
    }
    hipError_t publish(size_t n, hipStream_t first)
    {
        Copy& t = t_[cur_];
        if (const hipError_t e = hipMemcpyAsync(t.dev, t.staging, n * 4, hipMemcpyHostToDevice, first)) return e;
        if (const hipError_t e = hipEventRecord(t.ready, first)) return e;
        t.first = first;
        t.live = true;
        return hipSuccess;
    }
    hipError_t before_read(hipStream_t st) { return st == t_[cur_].first ? hipSuccess : hipStreamWaitEvent(st, t_[cur_].ready, 0); }
    hipError_t after_read(Reader which, hipStream_t st)
    {
        Copy& t = t_[cur_];
        if (!t.used[which]) if (const hipError_t e = t.used[which].create()) return e;
        if (const hipError_t e = hipEventRecord(t.used[which], st)) return e;
        t.recorded[which] = true;
        return hipSuccess;
    }
private:
    struct Copy {
        DevBuf<uint32_t> dev; uint32_t* staging = nullptr; hipStream_t first = nullptr; Event ready, used[RD_N]; bool recorded[RD_N] = {}; bool live = false;
        ~Copy() { if (staging) (void)hipHostFree(staging); }
    } t_[2];
    int cur_ = 0;
};

// The running EVM folded OUTSIDE K5, one lane per channel (m17_state.hpp, evm_fold_pass; m17hip_tune key 17).  K5 writes a run's operations into one row per
// channel and leaves its cursor at the end of every segment; the fold follows in passes.  Segment k's operations ride the limit-filter replay that runs ahead
// for segment k + 2 (ahead).  The LAST pass of a run, the operations of its last two segments, is OWED once the run is queued (end_run); whoever comes first
// takes it (take) and makes it: the next run's first replay (which K5 of that run waits for anyway), the run's own deferred decode, somebody who asks for
// m17_diag (flush_fold), or the end of the next run.  A run that begins while a pass is owed writes the other row buffer and leaves its end-of-run cursors
// in the other row of `cur_`: the owed pass keeps what it works on.  EvParams::last says which pass a kernel is making:
enum EvLast : uint32_t {
    EV_MORE = 0, EV_SETTLES = 1,   // not a run's last pass; its last pass, behind the run or in front of what K5 waits for: m17_diag is settled as always
    EV_BESIDE_K5 = 2   // its last pass beside K5 of the NEXT run's first segment: m17_diag is NOT settled by this pass — that K5 has the state in its hands meanwhile; found by the sweep: a run whose last segment fires no callback kept the value this pass had put over the first segment's mark (NOTES 6.3.4)
};
class EvmFold {
public:
    struct Pass { const float* ops = nullptr; uint32_t C = 0; const uint32_t* upto = nullptr; uint32_t blocks() const { return ev_fold_blocks(C); } };
    DevBuf<EvState> state;                                   // [maxC]
    hipError_t alloc(size_t maxC) { maxC_ = (uint32_t)maxC; return cur_.alloc(4 * maxC); }   // (the cursors; the rows come with the first run that needs them)
    float* ops() const { return ops_[par_]; } uint32_t pitch() const { return pitch_; }   // the rows of the current / latest run (nullptr: none yet), floats per row
    void set_pitch(uint32_t floats) { pitch_override_ = floats; }   // tuning knob 18 (tests): floats per row instead of ev_row_floats(maxT); for rows still to be allocated
    bool owed() const { return owed_.ops != nullptr; }       // the latest run's last pass is still to be made
    hipError_t begin_run(uint32_t maxT)                      // the run before keeps its rows while its last pass is owed; rows of 4 B per symbol of the longest run
    {
        if (owed()) par_ ^= 1;
        if (!ops_[par_]) pitch_ = pitch_override_ ? pitch_override_ : ev_row_floats(maxT);
        return ops_[par_] ? hipSuccess : ops_[par_].alloc((size_t)maxC_ * pitch_);
    }
    uint32_t* cursor_out(uint32_t k, uint32_t nseg) const { return k + 1u == nseg ? end_cursors() : by_parity(cur_, k, maxC_); }   // where K5 of segment k of nseg leaves its cursor
    Pass ahead(uint32_t k, uint32_t C) const { return Pass{ops_[par_], C, by_parity(cur_, k - 2u, maxC_)}; }   // beside the replay ahead for segment k: up to K5's cursor of segment k - 2
    Pass take() { const Pass f = owed_; owed_ = Pass{}; return f; }   // the owed pass (ops == nullptr: none), which is the caller's to launch now
    void end_run(uint32_t C, bool deferred) { owed_ = deferred ? Pass{ops_[par_], C, end_cursors()} : Pass{}; }   // the run's rows, channels and end cursors
    void forget() { owed_ = Pass{}; }                        // (the state the pass would have updated is reset)
    void release(int* last_hip) { ops_[0].release(last_hip); ops_[1].release(last_hip); forget(); }   // the rows; nothing queued may still use them
private:
    uint32_t* end_cursors() const { return cur_.get() + (2 + (size_t)par_) * maxC_; }
    DevBuf<float> ops_[2];     // [maxC][pitch_] operations of a run
    int par_ = 0;              // the buffer of the current / latest run
    Pass owed_; uint32_t pitch_ = 0, pitch_override_ = 0, maxC_ = 0;
    DevBuf<uint32_t> cur_;     // [4][maxC] K5's operation cursor at the end of a segment: [0], [1] by segment parity; [2], [3] at the end of a run's LAST segment, by the run's buffer (par_)
};

struct TimedLaunch { Event a, b; int which; };

struct BertState; struct ChanStat; struct PacketState; struct PacketRec;   // (with the host layer's kernels, below)

// THE PAYLOAD CONSUMERS and the diagnostic log: what works on a run's records behind K5, on the payload stream (flush_payload).  Each owns its buffers and
// its books.  A consumer's STATE goes from run to run (and through the feeds); what a run completes goes to the STORE of the run's record set (0 / 1), so a
// fetch of run k reads beside the consumer of run k + 1.  `room` == 0: off.  configure = the m17hip_tune key (quiesce_payload comes first: nothing queued
// uses the buffers); reset = the consumer's part of m17hip_demod_reset; consume = the consumer over C rows of records, into the store of `set`.  Whether a
// RUN feeds a consumer is the run's (RecSet::bert / pkt / voice: what was on when it was made).  The methods are defined beside flush_payload.
struct BertStats {   // PRBS9 statistics (m17hip_tune key 6; m17hip_bert_stats, m17hip_sweep_stats)
    DevBuf<BertState> state;          // [maxC], from the creation on
    bool on = false;                  // (the runs made so far keep the setting they were made with)
    int reset(m17hip_ctx* c, hipStream_t st);
};
struct Packets {     // packet reassembly (key 7; m17hip_packets_fetch, m17hip_packets_feed)
    uint32_t room = 0;                // completed packets a store holds
    bool fed = false;                 // m17hip_packets_feed has filled a store since the room was set.  m17hip_demod_reset does NOT clear it (the voice
                                      // consumer's is cleared): a fetch after feed + reset finds the store empty, not M17HIP_ESTATE.  Kept as it is.
    bool on() const { return room != 0; }
    PacketState* state_or_null() const { return on() ? state_.get() : nullptr; }
    const PacketRec* store(int set) const { return recs_[set]; }
    const uint32_t* count(int set) const { return count_.get() + set; }   // packets completed into the store (not cut at room)
    int configure(m17hip_ctx* c, uint32_t value);
    int reset(m17hip_ctx* c, hipStream_t st);
    int consume(m17hip_ctx* c, hipStream_t ps, const FrameRec* recs, uint32_t rec_cap, const uint32_t* rec_count, uint32_t C, int set);
private:
    int fresh(m17hip_ctx* c, hipStream_t st);   // no half-assembled packet, nothing completed (configure, reset)
    DevBuf<PacketState> state_;       // [maxC]
    DevBuf<PacketRec> recs_[2];       // [room]
    DevBuf<uint32_t> count_;          // [2]
};
struct Voice {       // codec2 payload planes and the call log (key 34; m17_voice_kernel.hpp; m17hip_voice_fetch, m17hip_calls_fetch, m17hip_voice_feed)
    uint32_t room = 0, call_room = 0; // voice slots / call slots per channel of a store (nothing but (channel, seq) orders the calls)
    uint32_t rows[2] = {0, 0};        // channels whose rows of a store the consumer has written (a run's, or m17hip_voice_feed's)
    bool fed = false;                 // m17hip_voice_feed has filled a store since the room was set or the reset
    bool on() const { return room != 0; }
    VoiceState* state_or_null() const { return on() ? state_.get() : nullptr; }
    const uint8_t* audio(int set) const { return audio_[set]; }                                  // [maxC][room][16]
    const uint8_t* marks(int set) const { return marks_[set]; }                                  // [maxC][room]
    const uint32_t* counts(int set) const { return counts_.get() + (size_t)set * maxC_; }        // [maxC] voice records of the run (not cut at room)
    const CallRec* calls(int set) const { return calls_[set]; }                                  // [maxC][call_room]
    const uint32_t* call_counts(int set) const { return call_counts_.get() + (size_t)set * maxC_; }   // [maxC] calls closed in the run (not cut at call_room)
    VoiceParams params(int set, const FrameRec* recs, uint32_t rec_cap, const uint32_t* rec_count, uint32_t C, uint32_t channel_base) const
    {
        return VoiceParams{recs, rec_cap, rec_count, state_, C, audio_[set], marks_[set], counts_.get() + (size_t)set * maxC_, room,
                           calls_[set], call_counts_.get() + (size_t)set * maxC_, call_room, channel_base};
    }
    int configure(m17hip_ctx* c, uint32_t value);
    int reset(m17hip_ctx* c, hipStream_t st);
    int consume(m17hip_ctx* c, hipStream_t ps, const FrameRec* recs, uint32_t rec_cap, const uint32_t* rec_count, uint32_t C, int set);
private:
    int fresh(m17hip_ctx* c, hipStream_t st);   // no open call, seq back to 0, nothing of the runs before left to fetch (configure, reset)
    DevBuf<VoiceState> state_;        // [maxC]
    DevBuf<uint8_t> audio_[2], marks_[2];
    DevBuf<CallRec> calls_[2];
    DevBuf<uint32_t> counts_, call_counts_;   // [2][maxC]
    uint32_t maxC_ = 0;
};
struct DiagLog {     // one entry per diagnostic callback of the LATEST run (key 9; m17hip_diag_log_fetch): one store, not one per record set
    uint32_t room = 0;                // entries per channel
    bool on() const { return room != 0; }
    Diag* entries() const { return on() ? log_.get() : nullptr; }   // [maxC][room]: with `room`, the pair the kernels' parameter blocks take
    uint32_t* count() const { return count_; }                      // [maxC] entries written this run
    int configure(m17hip_ctx* c, uint32_t value);
private:
    DevBuf<Diag> log_;
    DevBuf<uint32_t> count_;
};

// The context's eight overflow words on the host (m17hip_ctx::RecSet::ovf is the layout: four words per record set), for what is asked of BOTH sets — the
// runs of a stream alternate between them.  `read` queues the copy; the words are there once `st` has been synchronised.
struct OvfWords {
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    hipError_t read(const uint32_t* overflow, hipStream_t st) { return hipMemcpyAsync(w, overflow, 32, hipMemcpyDeviceToHost, st); }
    bool evm_ops_dropped() const { return (w[2] | w[6]) != 0; }        // a channel outran its row of deferred EVM operations (since the reset): m17_diag::evm is not right
    uint64_t replay_drops() const { return (uint64_t)w[1] + w[5]; }    // channels that left the limit-filter replay (since the reset)
};

// What a run looks like: decided once (plan_run) and handed to every launch of the run.  Between m17hip_demod_front and m17hip_demod_run the
// context keeps it (front_plan), and the run call uses it as it is.
struct RunPlan {
    uint32_t C = 0, T = 0, flags = 0, nseg = 0;
    std::vector<uint32_t> b;      // b[k] = first sample of segment k; b[nseg] = T (segment_bounds)
    bool staged = false, from_front = false;   // it works on freshly swapped slabs (prefixes still to be carried), not in place; m17hip_demod_front queued its front end
    uint32_t ramp = 0;            // first segment of its ramp (tuning knob 33), 0 = none
    bool dcd_latency = false, fir_latency = false;   // K3 as the four-wave latency pipeline (tuning knob 10); few items per K1 workgroup: the chain of K5 launches decides
    bool gate_run = false;        // it is gate-aware (tuning knob 26)
    uint32_t front_segs = 0;      // segments whose front end is queued at once (tuning knob 5)
    bool gate0_queued = false;    // m17hip_demod_front has queued the replay of its first segment (and the prefix copies in front of it)
    uint32_t n_reset = 0;         // channels that begin it with fresh demodulators (m17hip_demod_reset_channels): entries of the context's reset list in use
    // The polarity of its channels (m17hip_set_channel_polarity; resolve_polarity): uniform — bit 0 of kflags says it, pol == nullptr, the launches are those
    // of a context without a table — or mixed: pol = the device table the run reads to its end (entry XOR bit 0 of kflags), whatever is set meanwhile.
    uint32_t kflags = 0;          // `flags` as the kernels get them
    const uint32_t* pol = nullptr;
    uint32_t t0(uint32_t k) const { return b[std::min<size_t>(k, nseg)]; }
};

}  // namespace

struct m17hip_ctx {
    int device = 0;
    int last_hip = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_main = nullptr;   // the main stream the library created with the others (StreamSet); `stream` is this one until m17hip_set_stream names another
    int set_mode = 0;
    hipStream_t side = nullptr;        // K3 runs here, concurrently with K1 (side2) and with K2/K5 of earlier segments (stream)
    hipStream_t side2 = nullptr;       // K1 of the segments of a run
    hipStream_t side3 = nullptr;       // K2 of segment k+1 while K5 works on segment k
    Event ev_fork, ev_join;
    uint32_t front_ahead = 0;         // tuning knob 5: segments the front end (K1, K3) may run ahead of K5 (0 = unlimited, measured best)
    uint32_t maxC = 0, maxT = 0;
    size_t xpitch = 0, ypitch = 0;
    uint32_t ticks_cap = 0, rec_cap = 0, rec_cap_alloc = 0;   // rec_cap: record slots per channel and run in use (<= allocated)
    // The per-run slabs (the kernels' comments call them xbuf, ybuf, hbuf): input x (pitch xpitch), matched-filter output y and K2's
    // limit-filter history h (pitch ypitch), K3's table dcd (ticks_cap rows of 12 per channel).
    // Streaming: a second pair.  The input of the NEXT run is staged in other().x while the current run computes; that
    // run's front end (K1 -> other().y, K3 -> other().dcd) may start before the current run's K2/K5 chain has ended (m17hip_demod_front),
    // and K2 / K5 of the next run then work on other().y / .h.  The pairs change roles (slot ^= 1) when a staged run begins.
    struct SegEvents { Event fir, dcd, gate, redo, seq; };   // of one segment: K1 / K3 / K2 (ahead) done, K2 redo done, K5 done
    struct Slab {
        DevBuf<int16_t> x;
        DevBuf<float> y, h, dcd;
        uint32_t C = 0, T = 0;        // what the input slab holds (m17hip_input_alternate)
        Event end; bool used = false; // the last run on this pair is done with its slabs, if there has been one
        std::vector<SegEvents> seg;   // one set per slab pair (consecutive staged runs alternate)
        hipError_t wait_free(hipStream_t st) const { return used ? hipStreamWaitEvent(st, end, 0) : hipSuccess; }
        hipError_t ensure_seg_events(uint32_t nseg)
        {
            for (SegEvents s; seg.size() < nseg; seg.push_back(std::move(s)))   // (what an Event is moved out of is empty again)
                for (Event* e : {&s.fir, &s.dcd, &s.gate, &s.redo, &s.seq}) if (const hipError_t r = e->create()) return r;
            return hipSuccess;
        }
    } slab[2];                        // [1]: allocated the first time input is staged (stage_prepare)
    // A FLOAT STREAM (m17hip_upload_f32): its input rows are float32 in the reference's units, in a pair of their own — same pitch in samples, same
    // XPRE prefix, named by the same slot as the int16 pair.  Allocated lazily: a slab with the first float input that goes to its slot, and with the
    // first of them the float twins of the 149-sample histories (SeqState::hist -> hist_f; Boundary::hist -> bnd_hist_f, by segment parity).
    // A context that never sees a float holds none of it (m17hip_input_format reports the bytes) and its launches are what they always were.
    struct FloatSlab {
        DevBuf<float> x;
        size_t bytes() const { return x.size() * sizeof(float); }
    } fslab[2];
    DevBuf<float> hist_f, bnd_hist_f; // [maxC][HISTF_PITCH]; [2][maxC][HISTF_PITCH]
    // The sample format belongs to the stream: the first input after the creation or m17hip_demod_reset fixes it (synthesis is int16), input of the
    // other format is refused until the next reset.  Each slab pair remembers the format of the input it holds; a run takes its slab's.
    int stream_fmt = 0;               // M17HIP_FORMAT_*; 0: free
    int slab_fmt[2] = {0, 0};
    // COMPLEX IQ INPUT (m17hip_upload_iq): the discriminator writes the float pair's slabs, so behind it the stream is a float stream.  What it holds of its
    // own, allocated with the first IQ input: the carry — one float2 per channel, the last IQ sample of the previous IQ block, zero for a fresh feed — and,
    // for the host forms, a buffer for the raw IQ of one block (grown when a later block is larger).  In-place blocks run on the main stream and staged ones
    // on the copy stream: `ev_iq` follows every launch that reads or writes the carry (or reads iq_raw), a launch on the other stream goes behind it.
    DevBuf<float2> iq_carry;          // [maxC]
    DevBuf<char> iq_raw;              // rows of round_up(T, 4) samples of the latest host block's format
    Event ev_iq;
    hipStream_t iq_last = nullptr;    // the stream ev_iq was recorded on (nullptr: never)
    // WIDEBAND IQ INPUT (m17hip_wide_config, m17hip_upload_wide): S sources at 48 kSPS x decim, every channel tuned to one of them by tune_kernel, which
    // writes the float slabs as the discriminator does and keeps its last z in iq_carry.  Of its own: the taps, the sources' histories (the last ntaps - 1
    // converted samples each; two copies that take turns, wide_par names the one to read), the z a launch leaves for wide_carry_kernel, and the channel table
    // [source[maxC] | fcw[maxC]] — on the host here, on the device in a turn-taking table, so m17hip_wide_channels touches no stream and a queued
    // block keeps the table it was tuned with.  ev_iq orders these launches across the two streams like the discriminator's.
    struct Wide {
        uint32_t S = 0, R = 0, L = 0; int fmt = 0;   // S == 0: not configured
        uint32_t R2 = 0, L2 = 0;                     // R2 == 0: one stage (m17hip_wide_config); else R and L are stage 1's (m17hip_wide_config2: tune2_kernel)
        uint32_t U = 0, D = 0;                       // U != 0: the second stage resamples by U / D (m17hip_wide_resample: resample_kernel); R2 == 0, L2 its taps
        uint64_t row(uint32_t T) const { return U ? (uint64_t)(T / U) * D * R : (uint64_t)T * (R2 ? R * R2 : R); }   // wideband samples under T outputs
        uint32_t hlen() const { return U ? (wide2_j(L2, U) - 1) * R + L - 1 : R2 ? (L2 - 1) * R + L - 1 : L - 1; }   // converted samples a source carries
        uint32_t M = 0, M1 = 0, M2 = 0;              // M != 0: a raster of M bins (m17hip_wide_raster: chan_kernel); R and L are its decimation and taps, R2 == 0
        DevBuf<float> taps, taps2; DevBuf<float2> hist[2], znew, tw;
        int par = 0;
        uint64_t count = 0;               // wideband samples per source since the feed began
        std::vector<uint32_t> table;      // [2 * maxC]
        bool dirty = true;
        TurnTable dev;
        // Under a raster the table's second half holds bin mod M, and the device reads it sorted by source (chan_table_words; csrc/m17_chan_kernels.hpp), made
        // for the channels of the launch: a copy of its own, written when the table or the launch's channel count has changed.
        TurnTable rdev;
        uint32_t rdev_C = 0;
        // The raster survey (m17hip_wide_survey; csrc/m17_chan_survey_kernels.hpp): stride != 0 is on.  Two power planes [S][M] take turns like hist, each
        // with the event recorded behind the block's chan_survey_sum_kernel and the block's J and N0; `latest` names the one of the latest surveyed block.
        // The scratch [S][groups][M] is every block's: the blocks' launches are ordered by ev_iq.
        struct Survey {
            uint32_t stride = 0;
            DevBuf<float> scratch, plane[2];
            Event ev[2];
            bool valid[2] = {false, false};
            uint32_t times[2] = {0, 0};
            uint64_t first_output[2] = {0, 0};
            int latest = 0;
            hipStream_t fetch = nullptr;   // m17hip_wide_survey_fetch's copies: a stream of its own, behind nothing but the plane's event
            void forget() { valid[0] = valid[1] = false; }
            ~Survey() { if (fetch) (void)hipStreamDestroy(fetch); }
        } sv;
        // The source spectrum (m17hip_wide_spectrum; csrc/m17_spectrum_kernels.hpp), under every configuration: points != 0 is on.  Planes [S][points],
        // events and scratch [S][groups][points] as the survey's.  The window and the twiddles stay on the host until the next block brings them to the
        // device as one table [window[points] | tw[points / 2][2]] (`dirty`), in the copy no queued launch reads.
        struct Spectrum {
            uint32_t points = 0, logn = 0, hop = 0;
            std::vector<float> table;
            bool dirty = true;
            TurnTable dev;
            DevBuf<float> scratch, plane[2];
            Event ev[2];
            bool valid[2] = {false, false};
            uint32_t frames[2] = {0, 0};
            uint64_t first_sample[2] = {0, 0};
            int latest = 0;
            hipStream_t fetch = nullptr;   // m17hip_wide_spectrum_fetch's copies: a stream of its own, behind nothing but the plane's event
            void forget() { valid[0] = valid[1] = false; }
            ~Spectrum() { if (fetch) (void)hipStreamDestroy(fetch); }
        } sp;
        // The channel meter (m17hip_wide_meter; csrc/m17_meter_kernels.hpp), under every configuration: window != 0 is on.  `outputs` is the feed's output
        // count (N0 of the next block), kept whether the meter is on or off.  The power scratch [C][T] is written by the metered instantiation of the
        // block's kernel and read by wide_meter_kernel behind it on the same stream; it is every block's, like the survey's: the next block's kernel runs
        // behind ev_iq, which is recorded behind this block's meter kernel.  Two planes [3][C][K] take turns, each with its own shape, event and capacity:
        // only the plane whose turn it is is ever regrown, so the block before keeps its words.
        struct Meter {
            uint32_t window = 0;
            uint64_t outputs = 0;
            DevBuf<float> scratch, plane[2];
            Event ev[2];
            bool valid[2] = {false, false};
            uint32_t C[2] = {0, 0}, K[2] = {0, 0}, T[2] = {0, 0};
            uint64_t N0[2] = {0, 0};
            uint32_t win[2] = {0, 0};
            int latest = 0;
            hipStream_t fetch = nullptr;   // m17hip_wide_meter_fetch's copies: a stream of its own, behind nothing but the plane's event
            void forget() { valid[0] = valid[1] = false; }
            ~Meter() { if (fetch) (void)hipStreamDestroy(fetch); }
        } mt;
        // The spectrum squelch of the three tuners (m17hip_wide_squelch; csrc/m17_squelch_kernels.hpp): `on` needs the spectrum on and no raster.  The
        // levels [open[S] | close[S]] stay on the host until the next block brings them to the device in a turn-taking table (`dirty`).  The hold counts
        // [maxC] are the feed's, ordered across the two streams by ev_iq like the carries; `fresh` says that the next squelched block zeroes the whole
        // array on its own stream in front of its kernel, so neither m17hip_wide_squelch nor m17hip_demod_reset touches a stream for them.  Two planes of state words and band
        // powers [maxC] take turns, each with the event recorded behind the block's wide_squelch_kernel; the block's tuner reads its own state plane.
        struct Squelch {
            bool on = false, fresh = true;
            uint32_t B = 0, hang = 0;
            std::vector<float> levels;
            bool dirty = true;
            TurnTable dev;
            DevBuf<uint32_t> hold, state[2];
            DevBuf<float> band[2];
            Event ev[2];
            bool valid[2] = {false, false};
            uint32_t C[2] = {0, 0}, frames[2] = {0, 0};
            int latest = 0;
            hipStream_t fetch = nullptr;   // m17hip_wide_squelch_fetch's copies: a stream of its own, behind nothing but the plane's event
            // The time-resolved mode (m17hip_wide_squelch_slots; `slots`, exclusive with the block mode above): hold, state, levels, events and the fetch
            // stream serve as they do there.  Of its own: the slots' open flags of the block being queued (read by its tile kernel alone, on the same
            // stream), and two band planes [C][G] and two tile masks [C][ceil(tiles / 32)] that take turns with the state planes and grow with the
            // block's shape; the block's tuner reads its own mask.
            bool slots = false;
            uint32_t lead = 0;
            DevBuf<uint32_t> sbits, mask[2];
            DevBuf<float> sband[2];
            uint32_t G[2] = {0, 0}, tiles[2] = {0, 0};
            // The floor on the device (m17hip_wide_squelch_floor; `floor`, beside either mode above): squelch_floor_kernel in front of the mode's kernels makes
            // the block's levels from its plane, and those kernels read them from the floor plane whose turn it is in place of the table of given levels,
            // which is then neither uploaded nor read and keeps what it holds.  The carry [256] is the feed's, ordered by ev_iq like `hold`; `fresh` fills it
            // with NaNs where it zeroes `hold`.  Two planes [4][S] = med | floor | open | close take turns with the state planes and share their events;
            // has_floor says which of those blocks wrote one.  Only squelch_set turns `on` on, and it turns `floor` off: nothing else has to.
            bool floor = false;
            float f_open = 0.0f, f_close = 0.0f, f_rise = 1.0f, f_fall = 1.0f, f_min = 0.0f;
            DevBuf<float> fcarry, fplane[2];
            bool has_floor[2] = {false, false};
            void forget() { valid[0] = valid[1] = false; }
            ~Squelch() { if (fetch) (void)hipStreamDestroy(fetch); }
        } sq;
        // The carrier scan (m17hip_wide_scan; csrc/m17_scan_kernel.hpp): `on` needs the block squelch and its floor on (active()).  The pool marks [maxC]
        // stay on the host until the next block brings them to the device in a turn-taking table (`dirty`).  wide_scan_kernel goes between the block's
        // floor kernel and its squelch kernel and writes the block's COMPLETE channel table [source[maxC] | fcw[maxC]] into the plane whose turn it is: the
        // squelch kernel and the tuner of that block read it in place of the host's table.  Two planes, two flag planes [maxC] and two miss planes [256]
        // take turns with the squelch's state planes — the next writer of a plane, two blocks on, is behind this block's tuner through ev_iq —, each with
        // the event recorded behind the block's scan kernel.  The slots' words [maxC] are the feed's carry, ordered by ev_iq like `hold`; the squelch's
        // `fresh` says that the block's kernel takes the host's words, the seeds, in their place.
        struct Scan {
            bool on = false;
            uint32_t X = 0;
            std::vector<uint32_t> pool;   // [maxC] while on
            bool dirty = true;
            TurnTable dev;
            DevBuf<uint32_t> carry, plane[2], flags[2], missed[2];
            Event ev[2];
            bool valid[2] = {false, false};
            uint32_t C[2] = {0, 0}, frames[2] = {0, 0};
            int latest = 0;
            void forget() { valid[0] = valid[1] = false; }
        } sc;
        bool scanning() const { return sc.on && sq.on && !sq.slots && sq.floor; }
        size_t bytes() const
        {
            return (taps.size() + taps2.size() + sv.scratch.size() + sv.plane[0].size() + sv.plane[1].size() + sp.scratch.size() + sp.plane[0].size() +
                    sp.plane[1].size() + mt.scratch.size() + mt.plane[0].size() + mt.plane[1].size()) * sizeof(float) +
                   (hist[0].size() + hist[1].size() + znew.size() + tw.size()) * sizeof(float2) + (dev.words() + rdev.words() + sp.dev.words()) * 4 +
                   (sq.dev.words() + sq.hold.size() + sq.state[0].size() + sq.state[1].size() + sq.band[0].size() + sq.band[1].size() +
                    sq.sbits.size() + sq.mask[0].size() + sq.mask[1].size() + sq.sband[0].size() + sq.sband[1].size() + sq.fcarry.size() + sq.fplane[0].size() +
                    sq.fplane[1].size() + sc.dev.words() + sc.carry.size() + sc.plane[0].size() + sc.plane[1].size() + sc.flags[0].size() + sc.flags[1].size() +
                    sc.missed[0].size() + sc.missed[1].size()) * 4;
        }
    } wide;
    // THE WIDEBAND SIGNAL GENERATOR (m17hip_synth_wide_config, m17hip_synth_wide; csrc/m17_wide_tx_kernels.hpp): the int16 input slab's rows FM-modulated into
    // S wide streams at 48000 P / Q in the caller's memory.  Of its own: the channel table — on the host [maxC] entries, on the device a turn-taking copy of
    // the per-source lists made for the channels of a call —, the carries (A2 per channel; the last baseband sample in two copies that take turns, `par` names
    // the one to read), the scratch plane of phase bases (8 bytes per baseband sample of the largest block so far) and, for the host form, the block's
    // output before it is copied out.  Every call is complete when it returns, so nothing here is ever in flight between calls.
    struct WideTx {
        uint32_t S = 0, P = 0, Q = 0; int fmt = 0;   // S == 0: not configured
        uint64_t K = 0, seed = 0, first = 0, count = 0;
        float sigma = 0.0f;
        std::vector<m17_wide_tx> table;   // [maxC]
        bool dirty = true;
        TurnTable dev;
        uint32_t dev_C = 0;
        DevBuf<uint64_t> a2, plane;       // [maxC]; [channels][samples] of the largest block
        DevBuf<int32_t> last;             // [2][maxC]
        DevBuf<char> out;                 // the host form's block
        int par = 0;
        bool fresh = true;                // the carries are zeroed in front of the next block (a feed's start)
        size_t bytes() const { return (a2.size() + plane.size()) * 8 + last.size() * 4 + out.size() + dev.words() * 4; }
    } wtx;
    Slab& now() { return slab[slot]; }         // the current / latest run's
    Slab& other() { return slab[slot ^ 1]; }   // the staging pair (the run before the latest one's)
    bool foreign_streams[4] = {false, false, false, false};   // tools build, keys 40-43: side / side2 / side3 / copy belong to the experiment, not to the context
    hipStream_t copy = nullptr;       // host -> device copies of staged input only
    Event ev_copy;                    // the staged copy has left its source buffer
    Event ev_in_ready;                // the staged slab and its carried 152-sample prefix are complete
    Event ev_mark;                    // last main-stream operation a front end must not overtake (reset)
    bool inplace_after_run = false;   // the current input slab was overwritten in place after its last run: its data region no longer holds that run's tail
    int slot = 0;                     // the slab pair now() names (0 until the first staged run begins)
    bool staged = false;
    bool stage_inputs = false;        // tuning knob 16: the in-place producers write the staging slab
    DevBuf<char> synth_scratch;       // symbol staging of m17hip_synth_i16 (and the impairment grid of m17hip_synth_sweep_i16)
    uint32_t runT = 0;                // samples of the latest run
    Event ev_tail;                    // the latest run has carried its tails into its prefixes (K5 is done with its last segment)
    int gate0_early = 1;              // tuning knob 25: 1 = it does so
    DevBuf<Boundary> bnd;             // [2][maxC] boundary records (by segment parity, as every [2][maxC] below: by_parity): K5 -> the redo of K2 (m17_state.hpp)
    uint32_t front_k1_after = 0;      // tuning knob 21: the matched filter of a staged run starts after K5 of this segment (1-based) of the run before it; 0 = at once
    uint32_t last_nseg = 0;           // segments of the latest run
    bool wave_times = false;          // tuning knob 19: K5 writes each wave's working time per segment (m17hip_debug_counters)
    uint32_t stagedC = 0, stagedT = 0;
    bool front_queued = false;        // m17hip_demod_front has queued the front end of the run that must follow:
    RunPlan front_plan;               // that run, as m17hip_demod_run will make it
    uint32_t carryT = 0;              // length of the run whose tail those prefixes come from (0 = none since the reset)
    DevBuf<float> final_h;            // [2][maxC][4], by segment parity
    DevBuf<GateExport> gate_exp;      // [maxC] K2's own state at the end of a segment
    DevBuf<uint32_t> dropped;         // [2][maxC] K5: the segment dropped the speculation
    BertStats bert;                   // the payload consumers and the diagnostic log (tuning knobs 6, 7, 34, 9)
    Packets packets;
    Voice voice;
    DiagLog diag;
    DevBuf<ChanStat> chan_words;      // m17hip_sweep_stats' words on their way out / a rank's words on their way into m17hip_gather_sweep_stats (payload stream)
    uint32_t kalman_order = 3;        // evaluation order of the Kalman updates (m17hip_set_kalman_order)
    int gather_fault = 0;             // tuning knob 30 (tests): 1 = this rank's compaction (m17hip_gather_sweep_stats: its upload) fails inside the gather, 2 = the root's staging allocation fails, 3 = its word of exchange 2 is not written,
                                      // 4 = it cannot read exchange 1, 5 = it cannot read exchange 2
    uint32_t gather_timeout_ms = 120000;   // tuning knob 31: bound of every wait inside m17hip_gather_frames / m17hip_gather_sweep_stats (0 = none)
    uint32_t channel_base = 0;        // global id of channel 0 (m17hip_set_channel_base): records carry channel_base + c
    uint32_t front_first = 0;         // tuning knob 12: segments of K1 that must be complete before the first K5 starts (0 = its own only)
    int redo_form = 0;                // tuning knob 20: the replay's redo beside K5, state only (0, default), or in front of K5 with the history stored (1)
    int dcd_form = -1;                // tuning knob 10: K3 as one wave per 32 channels (0), as the four-wave latency pipeline (1), or chosen per run (-1: the pipeline for runs queued by m17hip_demod_front)
    uint64_t seen_overlap = 0;        // (run registry below) the overlap count this context's previous run saw
    hipEvent_t last_end = nullptr;    // Slab::end of the run queued last (not owned)
    uint32_t seg_len = 48000;         // tuning knob 3: samples per K2+K5 segment of a run (0 = the whole run)
    uint32_t seg0_len = 0;            // tuning knob 4: samples of the FIRST segment (a short one starts K5 early; 0 = like the others; measured neutral)
    int64_t seg_ramp = -1;            // tuning knob 33: first segment of a ramp r, 2 r, 4 r, ... up to seg_len (0 = none; -1 = per run: AUTO_RAMP when the run is the only thing in flight)
    DevBuf<DcdState> dcd_state;
    DevBuf<SeqState> seq_state;
    // Two RECORD SETS that alternate run by run (what a run writes for its consumers: record slots, counts, the deferred-frame store, the
    // run's overflow words).  The payload work of run k — deferred decode, consumers, compaction, the gather — runs on the PAYLOAD stream
    // beside the chain of run k + 1, which writes the other set; m17hip_frames_select says which run's records the fetch family names.
    struct RecSet {
        DevBuf<FrameRec> recs;            // [maxC][rec_cap_alloc]
        DevBuf<uint32_t> rec_count;       // [maxC]
        DevBuf<uint32_t> defer_llr;       // [maxC][rec_cap_alloc][46]: LLR frames (nibbles) K5 leaves for decode_deferred_kernel (tune 15), lazily
        uint32_t* ovf = nullptr;          // -> overflow + 4 * index: [0] record overflow of the run, [1] channels that left the replay (since reset, this set's runs),
                                          //    [2] deferred EVM operations dropped (since reset), [3] channel-segments of the run that ended with the carrier off
        Event chain;                      // the run that wrote this set has left the main stream (state settled): what its payload work waits for
        Event done;                       // the payload stream is through with the run that wrote this set
        uint32_t C = 0, rec_cap = 0, nseg = 0;
        bool valid = false;               // holds a finished run's records in the layout (rec_cap) they were written with
        bool pending = false;             // its payload work (deferred decode, consumers) is not queued yet (flush_payload)
        bool bert = false, pkt = false, voice = false;   // the consumers that were on when the run was made
    } sets[2];
    int cur = 0;                      // the set of the latest run
    uint32_t sel_back = 0;            // m17hip_frames_select: 0 = the latest run's records, 1 = the run's before it
    // The PAYLOAD stream (deferred decode, consumers, compaction, gather): the copy stream of a context that streams (it exists from the first
    // staged input on), the main stream otherwise.  Not a stream of its own: one more stream per context moved the continued-stream regime from
    // 24 to 27-37 ms whatever its place in the creation order (which streams share a hardware pipe: NOTES 4.14, 6.3).  The copy stream also
    // carries the next run's staged input and prefix copies, which must never wait for a FUTURE event: so a run's payload work is queued
    // when somebody asks for its results (or needs its record set back), not when the run is queued — flush_payload.
    bool streams() const { return copy && slab[1].x; }   // input has been staged (stage_prepare): the copy stream is at work (a parked set may bring one along — that alone changes nothing)
    hipStream_t pay() const { return streams() ? copy : stream; }
    Event ev_dst;                     // the caller's main-stream work on a device destination is done (a fetch of the LATEST run orders itself behind it)
    Event ev_switch;                  // m17hip_set_stream: what was queued before the switch (the new main stream waits for it)
    Event ev_fetch;                   // m17hip_sweep_stats: the main stream's last EVM fold (the payload stream waits for it)
    DevBuf<uint32_t> overflow;        // [8]: four words per record set
    DevBuf<uint64_t> rec_offsets;     // exclusive prefix of rec_count (+ total at [C]): scratch of a compaction (payload stream)
    DevBuf<FrameRec> compact;         // lazily sized
    DevBuf<DecodeTables> tables;
    DevBuf<float> taps;
    DevBuf<float> taps_skew;         // tap table of fir_rrc150_skew_kernel (fs_build_tap_table)
    int limit_form = 1;              // (tools build only, key 27) configs[1]'s limit filter: 1 = the chain relayed between two waves, 0 = round 4's one recurrence wave
    int fir_form = 1;                // (tools build, key 11) K1: 1 = skewed-pair form on a bounded grid, 0 = round 4's rolled R = 15 form, one workgroup per tile
    int gate_aware = -1;             // tuning knob 26: K1 skips what the carrier cannot be on for (1), never (0), or chosen per run from how much of the previous run's channel-segments ended with the carrier off (-1, default)
    DevBuf<GateTruth> truth;         // [2][maxC] by segment parity: K5's gate state at the end of a segment
    DevBuf<uint32_t> first_needed;   // [maxC] gate_forecast_kernel -> K1
    uint32_t off_segs_prev = 0, chan_segs_prev = 0;   // channel-segments of the last FETCHED run that ended with the carrier off / in all
    uint32_t fir_grid = 0;           // tuning knob 13: workgroups of K1's grid (0 = default: from the items per workgroup below)
    uint32_t n_cu = 256;
    DevBuf<uint32_t> defer_hist;     // [maxC][101][64]: decode_deferred_kernel's decision words (one launch at a time: payload stream)
    bool defer_decode = true;
    bool defer_evm = true;           // tuning knob 17: the running EVM folded outside K5 ...
    EvmFold evm;                     // ... its state, its operation rows and the pass that is still owed
    uint32_t seq_lds_bytes = 0; // tune 14: LDS bytes a workgroup of the sequential kernel asks for (0 = SEQ_LDS_BYTES_4 for four waves)
    DevBuf<float> llr_edges;
    DevBuf<core::Kalman2Gain> level_gain;   // [8 orders][LEVEL_SCHED_N] gain schedules of the level filters (core.h)
    DevBuf<char> scratch;             // per-operator staging (correlator outputs, viterbi io)
    DcdCoef coef{};
    uint64_t pos = 0;          // samples consumed since reset
    // m17hip_demod_reset_channels: the channels marked since the latest run was queued, each once (`marked`: [maxC], sized with the first mark).
    // The run that takes the marks puts them on the device as a list (TurnTable; take_marks); each kernel that reads it records its reader's event as it
    // is queued (front / carrier detect / main / payload).  A context that never marks never writes one.
    std::vector<uint32_t> marks;
    std::vector<uint8_t> marked;
    TurnTable reset_list;      // the list of the latest run that took marks
    // m17hip_set_channel_polarity: entry c = 1: channel c's samples are negated (XOR M17HIP_FLAG_INVERT of the call).  The table is the host's (`pol_host`,
    // [maxC], sized by the first call that sets a 1; `pol_ones` of its entries are 1); a launch whose channels are of one polarity never needs it on the
    // device.  One that does (resolve_polarity) finds it in a TurnTable, written when the host's has changed (`pol_dirty`).  Its readers are every launch of
    // every run queued until the next change: their events are recorded on all four reading streams (main, K3's, K1's, the replay's) when the turn passes
    // on — so a run in flight keeps the table it was queued with.  A context that never sets a 1 never writes one.
    std::vector<uint8_t> pol_host;
    uint32_t pol_ones = 0;
    bool pol_dirty = false;
    TurnTable pol_table;       // the table of the latest launch that read one
    uint32_t lastC = 0;
    bool have_run = false;     // a run has been made since the last reset (the stream continues)
    bool uploaded = false;
    bool timing = false;
    bool profile = false;      // K5 writes per-channel tick counters (tuning knob 1)
    DevBuf<unsigned long long> dbg;  // [maxC][8] diagnostic cycle counters of K5
    uint32_t dbg_waves = 0;
    std::vector<TimedLaunch> pending;
    std::vector<Event> pool;
    double acc_ms[KT_N] = {0};
    uint64_t acc_n[KT_N] = {0};
};

struct m17hip_comm {
    ncclComm_t comm = nullptr;
    int device = 0;                   // any context on this device may gather through the communicator (one call at a time)
    int rank = 0, nranks = 1;
    int last_rccl = 0;
    DevBuf<uint64_t> counts_dev;      // [2 * nranks] words of the status / count exchanges
    uint64_t* words_host = nullptr;   // pinned, [2 + 2 * nranks]: this rank's word pair on its way out, every rank's on the way in — no copy of an exchange ever
                                      // targets memory that a call which ran out of time has already given back
    uint32_t serial = 0;              // gather calls made through this communicator (every rank counts the same)
    DevBuf<char> gathered;            // root: every rank's contribution (frame records, sweep words), rank after rank
    bool dead = false;                // an exchange did not end in time or a collective call failed: given up, every later call returns M17HIP_ECOMM
};

namespace {

#define HIPCHK(ctx, expr)                                   \
    do {                                                    \
        hipError_t e_ = (expr);                             \
        if (e_ != hipSuccess) {                             \
            (ctx)->last_hip = (int)e_;                      \
            return M17HIP_EHIP;                             \
        }                                                   \
    } while (0)

size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

// The code of a failed allocation (or of a failed step of the gather): M17HIP_ENOMEM when the device is out of memory, M17HIP_EHIP
// otherwise; the error is kept in last_hip.  M17HIP_OK for hipSuccess.
int alloc_code(m17hip_ctx* c, hipError_t e)
{
    if (e == hipSuccess) return M17HIP_OK;
    c->last_hip = (int)e;
    return e == hipErrorOutOfMemory ? M17HIP_ENOMEM : M17HIP_EHIP;
}

// ---- constant tables ------------------------------------------------------------------------------------------
const uint8_t DC_SEQ[46] = {0xd6, 0xb5, 0xe2, 0x30, 0x82, 0xFF, 0x84, 0x62, 0xba, 0x4e, 0x96, 0x90, 0xd8, 0x98, 0xdd, 0x5d,
                            0x0c, 0xc8, 0x52, 0x43, 0x91, 0x1d, 0xf8, 0x6e, 0x68, 0x2F, 0x35, 0xda, 0x14, 0xea, 0xcd, 0x76,
                            0x19, 0x8d, 0xd5, 0x80, 0xd1, 0x33, 0x87, 0x13, 0x57, 0x18, 0x2d, 0x29, 0x78, 0xc3};  // M17 spec / M17Randomizer.h:16-22

uint16_t frame_source(size_t deinterleaved_index)
{
    const size_t i = deinterleaved_index;
    const size_t src = (45 * i + 92 * i * i) % 368;                       // PolynomialInterleaver.h:21-24
    const bool neg = (DC_SEQ[src >> 3] >> (7 - (src & 7))) & 1;           // M17Randomizer.h:30-49
    return (uint16_t)(src | (neg ? 0x200u : 0u));
}

void build_tables(DecodeTables& t)
{
    std::memset(&t, 0, sizeof(t));
    // puncture matrices Trellis.h:17-40
    std::vector<int> p1(61), p2(12, 1), p3(8, 1);
    for (size_t i = 0, j = 2; i != 61; ++i) { if (i == j) { p1[i] = 0; j += 4; } else p1[i] = 1; }
    p2[11] = 0;
    p3[7] = 0;
    struct Lay { int out, in, first; const std::vector<int>* p; };
    const Lay lay[4] = {{488, 368, 0, &p1}, {296, 272, 96, &p2}, {420, 368, 0, &p3}, {402, 368, 0, &p2}};
    for (int k = 0; k < 4; ++k) {
        size_t index = 0, pindex = 0;
        for (int i = 0; i < 488; ++i) t.src[k][i] = 0x8000;
        int i = 0;
        for (; i != lay[k].out && index < (size_t)lay[k].in; ++i) {     // depuncture, Util.h:169-190
            if (!(*lay[k].p)[pindex++]) t.src[k][i] = 0x8000;
            else t.src[k][i] = frame_source(lay[k].first + index++);
            if (pindex == lay[k].p->size()) pindex = 0;
        }
        for (; i < lay[k].out; ++i) t.src[k][i] = 0x4000;               // never written (BERT position 401)
        for (int q = 0; q < 488; ++q) t.src[4 + k][q] = (uint16_t)q;    // identity maps for already depunctured input
    }
    for (int i = 0; i < 96; ++i) t.lich_src[i] = frame_source(i);
    // Golay syndrome -> error pattern (weight <= 3 over 23 bits): Golay24.h:131-177
    auto syndrome = [](uint32_t cw) { cw &= 0xFFFFFFu; for (int i = 0; i != 12; ++i) { if (cw & 1u) cw ^= 0xC75u; cw >>= 1; } return cw; };
    std::vector<int> seen(2048, 0);
    auto put = [&](uint32_t v) { const uint32_t s = syndrome(v) & 0x7FF; t.golay_fix[s] = v; seen[s]++; };
    put(0);
    for (int i = 0; i < 23; ++i) put(1u << i);
    for (int i = 0; i < 22; ++i) for (int j = i + 1; j < 23; ++j) put((1u << i) | (1u << j));
    for (int i = 0; i < 21; ++i) for (int j = i + 1; j < 22; ++j) for (int k = j + 1; k < 23; ++k) put((1u << i) | (1u << j) | (1u << k));
}

void build_llr_edges(float* e)  // Util.h:63-104: edges accumulated in fp32
{
    const float inc = (float)(1.0 / (double)7.0f);
    float k = (float)(-3.0 + (double)inc);
    for (int n = 0; n < 43; ++n) { e[n] = k; k = k + inc; }
}

DcdCoef build_coef()  // SlidingDFT.h:85-95
{
    const std::complex<float> j{0, 1};
    const float pi2 = (float)(M_PI * 2.0);
    auto coeff = [&](size_t f) { const float k = float(f) / float(48000); return std::exp(-j * pi2 * k); };
    const auto c0 = coeff(2400), c1 = coeff(3600);
    return DcdCoef{c0.real(), c0.imag(), c1.real(), c1.imag()};
}

// ---- timing ---------------------------------------------------------------------------------------------------
Event get_event(m17hip_ctx* c)   // empty (and last_hip set) when the runtime cannot create one
{
    Event e;
    if (!c->pool.empty()) { e = std::move(c->pool.back()); c->pool.pop_back(); return e; }
    const hipError_t r = e.create(hipEventDefault);
    if (r != hipSuccess) c->last_hip = (int)r;
    return e;
}
// (a pair of timing events back to the pool: those of a launch that is not timed after all, or of one drain_timing has read)
void pool_events(m17hip_ctx* c, Event& a, Event& b)
{
    if (a) c->pool.push_back(std::move(a));
    if (b) c->pool.push_back(std::move(b));
}
struct Timed {  // HIP events on the stream the kernel is launched on; a launch whose events could not be had is not timed
    m17hip_ctx* c; int which; hipStream_t st; Event a, b;
    Timed(m17hip_ctx* ctx, int w, hipStream_t stream) : c(ctx), which(w), st(stream)
    {
        if (!c->timing) return;
        a = get_event(c); b = get_event(c);
        if (!a || !b || hipEventRecord(a, st) != hipSuccess) pool_events(c, a, b);
    }
    Timed(m17hip_ctx* ctx, int w) : Timed(ctx, w, ctx->stream) {}
    ~Timed()
    {
        if (!a) return;
        if (hipEventRecord(b, st) == hipSuccess) c->pending.push_back({std::move(a), std::move(b), which});
        else pool_events(c, a, b);
    }
};
// One kernel, timed by events BOUND to its launch (hipExtLaunchKernelGGL's start / stop events: the dispatch's own time stamps, what rocprofv3 reports) — nothing
// is put into the stream around it.  Two recorded events per launch (Timed above) cost a continued stream 0.65 ms of its 21.7 ms step (tools/stream_only.py,
// TIMING=1): for the five kernels of a run's chain that is the wrong price for being measured.
struct TimedK {
    m17hip_ctx* c; int which; Event a, b;
    TimedK(m17hip_ctx* ctx, int w) : c(ctx), which(w)
    {
        if (!c->timing) return;
        a = get_event(c); b = get_event(c);
        if (!a || !b) pool_events(c, a, b);
    }
    ~TimedK() { if (a) c->pending.push_back({std::move(a), std::move(b), which}); }
    template <typename... P, typename... A>
    void launch(void (*kernel)(P...), dim3 grid, dim3 block, uint32_t lds, hipStream_t st, const A&... args)
    {   // (the arguments converted to the kernel's own parameter types: hipExtLaunchKernelGGL copies them as they come)
        if (a) hipExtLaunchKernelGGL(kernel, grid, block, lds, st, a, b, 0, static_cast<P>(args)...);
        else hipLaunchKernelGGL(kernel, grid, block, lds, st, static_cast<P>(args)...);
    }
};
// Every entry point works on the context's own device whatever the calling thread's current device is (a host that also
// drives other GPUs, torch.cuda.set_device, ...): set it for the duration of the call and put the caller's back.
struct DeviceGuard {
    int prev = -1; bool ok = true;
    explicit DeviceGuard(m17hip_ctx* c)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != c->device) { const hipError_t e = hipSetDevice(c->device); if (e != hipSuccess) { c->last_hip = (int)e; ok = false; prev = -1; } }
        else prev = -1;
        (void)hipGetLastError();   // a stale error of an earlier call (ours or the host's) must not be blamed on this one's launches
    }
    ~DeviceGuard() { if (prev >= 0) hipSetDevice(prev); }
};
#define GUARD(ctx) DeviceGuard guard_(ctx); if (!guard_.ok) return M17HIP_EHIP

// ---- is this context the only one with a run in flight? ------------------------------------------------------------------------------
// The form of the carrier-detect kernel (m17hip_tune key 10 = -1) depends on it: with nothing else in flight on the device a step waits for
// that kernel's ten-launch chain and the four-wave latency form is 12 % faster; with other batches in flight the one-wave form is (the chip is
// full, the extra wave slots cost more than the chain saves).  A context cannot see the caller's intentions, only what happened: a run that is
// queued while another context's latest run has not finished counts as an overlap, and a context whose previous run was followed by one
// (its own launch or somebody's since) takes the process for one that overlaps batches.
// (Process-wide state: heap-allocated once and never destroyed — a context destroyed during static destruction at process exit still finds it;
//  every field of it, and every context's `last_end`, is read and written under `mu` only.)
struct RunRegistry { std::mutex mu; std::vector<m17hip_ctx*> ctxs; uint64_t overlaps = 0; };
RunRegistry& g_runs_ref() { static RunRegistry* r = new RunRegistry; return *r; }
#define g_runs (g_runs_ref())
bool runs_overlap(m17hip_ctx* c)   // at the launch of a run of c
{
    std::lock_guard<std::mutex> lk(g_runs.mu);
    bool other = false;
    for (m17hip_ctx* o : g_runs.ctxs)
        if (o != c && o->device == c->device && o->last_end && hipEventQuery(o->last_end) == hipErrorNotReady) other = true;
    (void)hipGetLastError();
    if (other) ++g_runs.overlaps;
    const bool overlapped = other || g_runs.overlaps != c->seen_overlap;
    c->seen_overlap = g_runs.overlaps;
    return overlapped;
}
void drain_timing(m17hip_ctx* c)
{
    for (auto& t : c->pending) {
        hipEventSynchronize(t.b);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) { c->acc_ms[t.which] += ms; c->acc_n[t.which]++; }
        pool_events(c, t.a, t.b);
    }
    c->pending.clear();
}

// ---- small device kernels owned by the host layer ----------------------------------------------------------------
// m17hip_tune key 17 changed: RunningStandardDeviation::S moves to where the new mode keeps it
__global__ void ev_move_kernel(SeqState* st, EvState* es, uint32_t C, int to_deferred)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    if (to_deferred) { es[c].S = st[c].hot.evm_S; es[c].pos = 0; } else st[c].hot.evm_S = es[c].S;
}

// A fresh channel = the zero-initialised object + the constructors' values (M17Demodulator.h:180-182), its stream beginning at
// the context's sample `pos` (a multiple of TICK: the carrier-detect ticks are the context's; 0 for m17hip_demod_reset).  The ONE definition
// of it: seq_reset_kernel (every channel) and the list kernels of m17hip_demod_reset_channels call these two.
__device__ __forceinline__ void fresh_demod_state(SeqState* st, EvState* es, uint32_t c, uint64_t pos)
{
    es[c] = EvState{1.0f, 0.f, 0u, 0u};   // RunningStandardDeviation::S{1.0}
    uint32_t* w = reinterpret_cast<uint32_t*>(st + c);
    for (size_t k = 0; k < sizeof(SeqState) / 4; ++k) w[k] = 0;
    Hot& s = st[c].hot;
    Cold& k = st[c].cold;
    s.run_pos = 148;              // the stream start is exact in ybuf (zero history)
    kal_reset(k.ck, 0.f);         // KalmanFilter() : reset(0.)
    // (the level filters: SymbolKalmanFilter() : reset(0.) = zero state, update count 0 — the zeroes above)
    k.dev_reset = 1;              // FreqDevEstimator::reset_ = true
    s.evm_S = 1.0f;               // RunningStandardDeviation::S{1.0}
    s.initializing = 1920;        // M17Demodulator.h:659 (per channel)
    s.st = ST_UNLOCKED;
    k.seg_start_tick = (uint32_t)(pos / TICK);   // the first carrier-detect segment begins with the channel's stream
    k.origin_lo = (uint32_t)pos; k.origin_hi = (uint32_t)(pos >> 32);   // records and log entries count from here
}
__device__ __forceinline__ void fresh_dcd_state(DcdState* ds, uint32_t c)
{
    uint32_t* d = reinterpret_cast<uint32_t*>(ds + c);
    for (size_t k = 0; k < sizeof(DcdState) / 4; ++k) d[k] = 0;
}

__global__ void seq_reset_kernel(SeqState* st, DcdState* ds, EvState* es, uint32_t C)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    fresh_demod_state(st, es, c, 0);
    fresh_dcd_state(ds, c);
}

// ---- m17hip_demod_reset_channels: the same over a LIST of n channels (each listed once, every entry < max_channels) -------------------------
// front end: the channel's 152-sample input prefix (FIR history, DFT delay) and / or its sliding-DFT state; a workgroup per listed channel
template <typename XT>
__global__ void front_reset_list_kernel(const uint32_t* list, uint32_t n, XT* x, size_t xpitch, DcdState* ds)
{
    if (blockIdx.x >= n) return;
    const uint32_t c = list[blockIdx.x];
    if (x) for (int k = threadIdx.x; k < XPRE; k += blockDim.x) x[(size_t)c * xpitch + k] = XT(0);
    if (ds && threadIdx.x == 0) fresh_dcd_state(ds, c);
}
// the 96-sample prefixes of the matched-filter output and of the limit-filter history; a workgroup per listed channel
__global__ void prefix_reset_list_kernel(const uint32_t* list, uint32_t n, float* y, float* h, size_t ypitch)
{
    if (blockIdx.x >= n) return;
    const uint32_t c = list[blockIdx.x];
    for (int k = threadIdx.x; k < YPRE; k += blockDim.x) { y[(size_t)c * ypitch + k] = 0.f; h[(size_t)c * ypitch + k] = 0.f; }
}
// the demodulator and EVM state; a lane per listed channel
__global__ void seq_reset_list_kernel(const uint32_t* list, uint32_t n, SeqState* st, EvState* es, uint64_t pos)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fresh_demod_state(st, es, list[i], pos);
}

// ---- the prefixes of the rows: ONE family for every element type and prefix length ------------------------------------------------------------
// XT, PRE = int16_t or float with XPRE for input rows (pitch and prefix in samples whatever the type), float with YPRE for the y and h rows.
// A workgroup per channel.  The forms over x AND y do in one launch what a run's end and the reset need of both.
template <typename XT, int PRE>
__global__ void zero_prefix_kernel(XT* x, size_t pitch)
{
    for (int k = threadIdx.x; k < PRE; k += blockDim.x) x[(size_t)blockIdx.x * pitch + k] = XT(0);
}
template <typename XT>
__global__ void zero_prefix_xy_kernel(XT* x, size_t xpitch, float* y, size_t ypitch)
{
    for (int k = threadIdx.x; k < XPRE; k += blockDim.x) x[(size_t)blockIdx.x * xpitch + k] = XT(0);
    for (int k = threadIdx.x; k < YPRE; k += blockDim.x) y[(size_t)blockIdx.x * ypitch + k] = 0.f;
}
// carry the last PRE samples of a run into the prefix of the next one
template <typename XT, int PRE>
__global__ void carry_tail_kernel(XT* x, size_t pitch, uint32_t T)
{
    __shared__ XT xs[PRE];
    XT* xr = x + (size_t)blockIdx.x * pitch;
    for (int k = threadIdx.x; k < PRE; k += blockDim.x) xs[k] = xr[(size_t)T + k];   // = row[PRE + T - PRE + k]
    __syncthreads();
    for (int k = threadIdx.x; k < PRE; k += blockDim.x) xr[k] = xs[k];
}
template <typename XT>
__global__ void carry_tail_xy_kernel(XT* x, size_t xpitch, float* y, size_t ypitch, uint32_t T)
{
    __shared__ XT xs[XPRE];
    __shared__ float ys[YPRE];
    XT* xr = x + (size_t)blockIdx.x * xpitch;
    float* yr = y + (size_t)blockIdx.x * ypitch;
    for (int k = threadIdx.x; k < XPRE; k += blockDim.x) xs[k] = xr[(size_t)T + k];
    for (int k = threadIdx.x; k < YPRE; k += blockDim.x) ys[k] = yr[(size_t)T + k];
    __syncthreads();
    for (int k = threadIdx.x; k < XPRE; k += blockDim.x) xr[k] = xs[k];
    for (int k = threadIdx.x; k < YPRE; k += blockDim.x) yr[k] = ys[k];
}
// staged runs: the other slab's prefix = the prefix of the previous run's rows (which that run's last kernel carried its tail into) ...
template <typename XT, int PRE>
__global__ void copy_prefix_kernel(const XT* src, XT* dst, size_t pitch)
{
    for (int k = threadIdx.x; k < PRE; k += blockDim.x) dst[(size_t)blockIdx.x * pitch + k] = src[(size_t)blockIdx.x * pitch + k];
}
// ... or the last PRE samples of the previous run's input, read where they lie: row[T .. T + PRE)
template <typename XT, int PRE>
__global__ void copy_tail_kernel(const XT* src, XT* dst, size_t pitch, uint32_t T)
{
    for (int k = threadIdx.x; k < PRE; k += blockDim.x) dst[(size_t)blockIdx.x * pitch + k] = src[(size_t)blockIdx.x * pitch + T + k];
}
// rows of T samples (pitch spitch) into the data region of the slab's rows: 16 bytes per lane where the source allows it
template <typename XT>
__global__ void copy_rows_kernel(const XT* src, size_t spitch, XT* dst, size_t dpitch, uint32_t T)
{
    constexpr uint32_t N = 16 / sizeof(XT);
    const uint32_t c = blockIdx.y;
    const uint32_t t = (blockIdx.x * blockDim.x + threadIdx.x) * N;
    if (t >= T) return;
    const XT* s = src + (size_t)c * spitch + t;
    XT* d = dst + (size_t)c * dpitch + XPRE + t;
    if (t + N <= T && (((uintptr_t)s) & 15) == 0) {
        *reinterpret_cast<int4*>(d) = *reinterpret_cast<const int4*>(s);
    } else {
        for (uint32_t q = 0; q < N && t + q < T; ++q) d[q] = s[q];
    }
}

// PRBS9 receiver state per channel (Util.h:320-441), carried between runs
struct BertState {
    uint32_t lfsr, synced, sync_count, bit_count, err_count, hist_count, hist_pos, frames;
    uint32_t hist[4];   // error flags of the last 128 validated bits
};
// decode_bert (apps/m17-demod.cpp:286-304) over the BERT records of the run just finished: one lane per channel
__global__ void bert_stats_kernel(const FrameRec* recs, uint32_t rec_cap, const uint32_t* rec_count, BertState* state, uint32_t C)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    BertState b = state[c];
    const uint32_t n = min(rec_count[c], rec_cap);
    for (uint32_t r = 0; r < n; ++r) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(recs + (size_t)c * rec_cap + r);
        if ((w[5] & 0xFFu) != 5u) continue;   // frame_type BERT
        ++b.frames;
        for (int i = 0; i < 197; ++i) {       // 24 bytes MSB first + the top 5 bits of byte 24
            const uint32_t byte = (w[6 + (i >> 5)] >> (8 * ((i >> 3) & 3))) & 0xFFu;
            const uint32_t bit = (byte >> (7 - (i & 7))) & 1u;
            if (!b.synced) {                  // PRBS9::syncronize
                const uint32_t res = (bit ^ (b.lfsr >> 8) ^ (b.lfsr >> 4)) & 1u;
                b.lfsr = ((b.lfsr << 1) | bit) & 0x1FFu;
                if (res) b.sync_count = 0;
                else if (++b.sync_count == 18u) {
                    b.synced = 1; b.bit_count += 18u;
                    b.hist[0] = b.hist[1] = b.hist[2] = b.hist[3] = 0; b.hist_count = 0; b.hist_pos = 0; b.sync_count = 0;
                }
            } else {                          // PRBS9::generate + count_errors
                const uint32_t g = ((b.lfsr >> 8) ^ (b.lfsr >> 4)) & 1u;
                b.lfsr = ((b.lfsr << 1) | g) & 0x1FFu;
                const uint32_t err = bit ^ g;
                b.bit_count += 1;
                const uint32_t wi = b.hist_pos >> 5, m = 1u << (b.hist_pos & 31u);
                uint32_t h = wi == 0 ? b.hist[0] : (wi == 1 ? b.hist[1] : (wi == 2 ? b.hist[2] : b.hist[3]));
                b.hist_count -= (h & m) ? 1u : 0u;
                if (err) { b.err_count += 1; b.hist_count += 1; h |= m; if (b.hist_count >= 25u) b.synced = 0; }
                else h &= ~m;
                if (wi == 0) b.hist[0] = h; else if (wi == 1) b.hist[1] = h; else if (wi == 2) b.hist[2] = h; else b.hist[3] = h;
                if (++b.hist_pos == 128u) b.hist_pos = 0;
            }
        }
    }
    state[c] = b;
}

// m17hip_sweep_stats: one packed word per channel (layout of m17_chan_stat) from the PRBS9 receiver's state and SymbolEvm's value; one lane per channel
struct ChanStat { uint32_t channel, point, bits, errors, synced, frames; float evm; uint32_t flags; };
__global__ void sweep_stats_kernel(const BertState* bert, const SeqState* seq, const uint32_t* ovf, uint32_t C, uint32_t channel_base, uint32_t n_points,
                                   ChanStat* out)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const BertState& b = bert[c];
    ChanStat w;
    w.channel = channel_base + c;
    w.point = w.channel % n_points;
    w.bits = b.bit_count; w.errors = b.err_count; w.synced = b.synced; w.frames = b.frames;
    w.evm = seq[c].cold.diag.evm;
    w.flags = (ovf[2] | ovf[6]) ? 0u : 1u;   // (deferred EVM operations were dropped: see m17hip_diag_fetch)
    out[c] = w;
}

// LinkSetupFrame::decode_callsign + type field + CRC of a batch of LSFs: one lane per frame
struct LsfInfo { char dst[10], src[10]; uint16_t type; uint8_t crc_ok; uint8_t reserved[9]; };
__global__ void lsf_info_kernel(const uint8_t* lsf, uint32_t n, LsfInfo* out)
{
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const uint8_t* b = lsf + (size_t)f * 30;
    LsfInfo o{};
    for (int which = 0; which < 2; ++which) {
        const uint8_t* e = b + 6 * which;
        char* dst = which ? o.src : o.dst;
        bool bc = true;
        uint64_t v = 0;
        for (int i = 0; i < 6; ++i) { bc = bc && e[i] == 0xFF; v = (v << 8) | e[i]; }
        if (bc) { const char t[10] = {'B', 'R', 'O', 'A', 'D', 'C', 'A', 'S', 'T', 0}; for (int i = 0; i < 10; ++i) dst[i] = t[i]; continue; }
        const char map[41] = "xABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-/.";
        int idx = 0;
        while (v) { dst[idx++] = map[v % 40u]; v /= 40u; }   // at most 9 digits below 2^48
    }
    o.type = (uint16_t)((b[12] << 8) | b[13]);
    uint8_t tmp[30];
    for (int i = 0; i < 30; ++i) tmp[i] = b[i];
    o.crc_ok = mod_crc16(tmp, 30) == 0u ? 1 : 0;
    out[f] = o;
}

// Packet reassembly per channel (apps/m17-demod.cpp:32-33,154-155,207-253), carried between runs
struct PacketState {
    uint32_t size, counter, seq_errors, frames, completed, pad[3];
    uint8_t data[832];   // 32 numbered frames x 25 bytes + a last frame of up to 25
};
struct PacketRec {       // = m17_packet_rec
    uint32_t channel, seq;
    uint64_t sample_pos;
    uint16_t size, checksum;
    uint8_t crc_ok, frames, seq_errors, reserved;
    uint8_t data[840];
};
// decode_packet over the packet records of the run just finished: one lane per channel.  An LSF callback starts a new packet
// (dump_lsf clears current_packet and the frame counter); numbered frames must arrive in order (a frame out of sequence is
// dropped, the counter stays); the frame with the EOF bit appends its last `n` bytes and closes the packet with the
// CRC-16/X.25 check (0x0f47 over contents + FCS).  Completed packets go to `out` in arrival order of the atomics;
// (channel, seq) orders them.
__global__ void packet_asm_kernel(const FrameRec* recs, uint32_t rec_cap, const uint32_t* rec_count, PacketState* state, uint32_t C,
                                  PacketRec* out, uint32_t out_cap, uint32_t* out_count, uint32_t channel_base)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    PacketState* st = state + c;
    uint32_t size = st->size, counter = st->counter, seq_errors = st->seq_errors, frames = st->frames, completed = st->completed;
    const uint32_t n = min(rec_count[c], rec_cap);
    for (uint32_t r = 0; r < n; ++r) {
        const FrameRec* rec = recs + (size_t)c * rec_cap + r;
        const uint32_t type = rec->frame_type;
        if (type == 0u) { size = 0; counter = 0; seq_errors = 0; frames = 0; continue; }   // FrameType::LSF -> dump_lsf
        if (type != 3u && type != 4u) continue;
        const uint8_t* p = rec->payload;
        const uint32_t tag = p[25];
        const uint32_t num = (tag & 0x7Fu) >> 2;
        if (!(tag & 0x80u)) {
            if (num != counter) { ++seq_errors; continue; }
            ++counter; ++frames;
            for (uint32_t i = 0; i < 25u; ++i) if (size + i < 832u) st->data[size + i] = p[i];
            size = min(size + 25u, 832u);
            continue;
        }
        const uint32_t take = min(num, 25u);
        ++frames;
        for (uint32_t i = 0; i < take; ++i) if (size + i < 832u) st->data[size + i] = p[i];
        size = min(size + take, 832u);
        uint32_t crc = 0xFFFFu;
        for (uint32_t i = 0; i < size; ++i) crc = mod_crc16_x25_update(crc, st->data[i]);
        crc = ~crc & 0xFFFFu;
        const uint32_t slot = atomicAdd(out_count, 1u);
        if (slot < out_cap) {
            PacketRec* o = out + slot;
            o->channel = channel_base + c; o->seq = completed; o->sample_pos = rec->sample_pos;
            o->size = (uint16_t)size; o->checksum = (uint16_t)crc;
            o->crc_ok = crc == 0x0F47u ? 1 : 0; o->frames = (uint8_t)frames; o->seq_errors = (uint8_t)min(seq_errors, 255u); o->reserved = 0;
            for (uint32_t i = 0; i < 840u; ++i) o->data[i] = i < size ? st->data[i] : (uint8_t)0;
        }
        ++completed;
    }
    st->size = size; st->counter = counter; st->seq_errors = seq_errors; st->frames = frames; st->completed = completed;
}
__device__ __forceinline__ void fresh_packet_state(PacketState* state, uint32_t c)
{
    state[c].size = 0; state[c].counter = 0; state[c].seq_errors = 0; state[c].frames = 0; state[c].completed = 0;
}
__global__ void packet_reset_kernel(PacketState* state, uint32_t C)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    fresh_packet_state(state, c);
}

__device__ __forceinline__ void fresh_bert_state(BertState* state, uint32_t c)
{
    BertState b{};
    b.lfsr = 1;
    state[c] = b;
}
__global__ void bert_reset_kernel(BertState* state, uint32_t C)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    fresh_bert_state(state, c);
}
// m17hip_demod_reset_channels: the payload consumers of the listed channels start over (pkt / voice == nullptr: that consumer is off); a lane per listed channel
__global__ void consumer_reset_list_kernel(const uint32_t* list, uint32_t n, BertState* bert, PacketState* pkt, VoiceState* voice)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fresh_bert_state(bert, list[i]);
    if (pkt) fresh_packet_state(pkt, list[i]);
    if (voice) fresh_voice_state(voice, list[i]);   // (an open call is abandoned, as a half-assembled packet is; its seq restarts)
}

// exclusive prefix sum of the per-channel record counts (single block; C <= a few 100k)
__global__ void rec_offsets_kernel(const uint32_t* counts, uint32_t rec_cap, uint64_t* offsets, uint32_t C)
{
    __shared__ uint64_t partial[256];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (C + 255) / 256;
    const uint32_t lo = tid * per, hi = min(C, lo + per);
    uint64_t sum = 0;
    for (uint32_t c = lo; c < hi; ++c) sum += min(counts[c], rec_cap);
    partial[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint64_t run = 0;
        for (int k = 0; k < 256; ++k) { const uint64_t v = partial[k]; partial[k] = run; run += v; }
        offsets[C] = run;
    }
    __syncthreads();
    uint64_t run = partial[tid];
    for (uint32_t c = lo; c < hi; ++c) { offsets[c] = run; run += min(counts[c], rec_cap); }
}

__global__ void compact_kernel(const FrameRec* recs, uint32_t rec_cap, const uint32_t* counts, const uint64_t* offsets,
                               FrameRec* out, uint64_t out_cap, uint32_t C)
{
    const uint32_t c = blockIdx.x;
    const uint32_t n = min(counts[c], rec_cap);
    const uint4* src = reinterpret_cast<const uint4*>(recs + (size_t)c * rec_cap);
    uint4* dst = reinterpret_cast<uint4*>(out + offsets[c]);
    for (uint32_t k = threadIdx.x; k < n * 4; k += blockDim.x)
        if (offsets[c] + k / 4 < out_cap) dst[k] = src[k];
}

// ---- the sample format of a slab pair's input rows (int16, or float32 in the reference's units): known HERE -----------------------------------
template <typename XT> constexpr int fmt_of() { return std::is_same<XT, float>::value ? M17HIP_FORMAT_F32 : M17HIP_FORMAT_I16; }
// the input rows of slab pair `slot` in that format (nullptr: not allocated)
template <typename XT> XT* slab_x(m17hip_ctx* c, int slot)
{
    if constexpr (std::is_same<XT, float>::value) return c->fslab[slot].x;
    else return c->slab[slot].x;
}
// f(the input rows of slab pair `slot` as what they hold — int16_t* or float*, slab_fmt[slot]); what f returns.  Whatever depends on the element type
// (a helper kernel's instantiation, the kernels below, the float histories) is written once, inside f.
template <typename F> auto with_x(m17hip_ctx* c, int slot, F&& f)
{
    return c->slab_fmt[slot] == M17HIP_FORMAT_F32 ? f(slab_x<float>(c, slot)) : f(slab_x<int16_t>(c, slot));
}
// The kernels that read input rows, chosen by the rows' pointer: K1 and K3 for channels of one polarity (INV) or of mixed ones, K2, K5 (KORDER as
// demod_wave_kernel has it).  The two forms of K3 take the same arguments.
template <bool INV, bool MIXED, typename XT> auto fir_kernel(XT*) { return fir_rrc150_skew_kernel<XT, INV, MIXED>; }
template <bool INV, bool MIXED, typename XT> auto dcd_kernel_of(XT*, bool one_wave) { return one_wave ? dcd_kernel<XT, INV, MIXED> : dcd_pipe_kernel<XT, INV, MIXED>; }
template <typename XT> auto gate_kernel(XT*) { return limit_track_kernel<XT>; }
template <int KORDER, typename XT> auto wave_kernel(XT*) { return demod_wave_kernel<XT, 4, false, false, KORDER>; }

// t0: first sample of the slab to process (segment of a run); the kernels see the slab from there on
constexpr size_t SEQ_LDS_BYTES_4 = 34816;   // see the K5 launch
// K1's grid.  A workgroup loops over (channel, tile) items; how many it takes decides how long it holds its place on a CU, i.e. how long a K5
// launch that becomes ready waits for room: 38 items per workgroup (five workgroups per CU) cost a continued stream 1.5 ms per step and one batch
// at a time 2 ms against 3 items per workgroup, while two batches in flight are 2 % faster with 6-12 than with 3 (NOTES 5.7).  So: about three
// items per workgroup for the runs that get the latency form of K3 (a continued stream, or nothing else in flight), eight for the others, and
// never fewer workgroups than a CU can hold of them five times over.
constexpr uint32_t FIR_GRID_PER_CU = 5, FIR_ITEMS_LATENCY = 3, FIR_ITEMS_THROUGHPUT = 8;
// `flags` / `pol`: the channels' polarity as resolve_polarity gave it (pol == nullptr: uniform, bit 0 of flags — today's two instantiations)
int launch_fir(m17hip_ctx* c, uint32_t C, uint32_t T, uint32_t flags, bool latency, hipStream_t st, uint32_t t0 = 0, const uint32_t* first_needed = nullptr,
               const uint32_t* pol = nullptr)
{
    TimedK tm(c, KT_FIR);
    return with_x(c, c->slot, [&](auto* x) -> int {
#ifdef M17_TOOLS
        if (c->fir_form == 0) {   // round 4's kernel: the measurement build keeps it for same-box comparisons (tools/k1_forms.py, the clk_k1 pass of tools/profile_round.sh)
            if constexpr (!std::is_same<decltype(x), int16_t*>::value) return M17HIP_ESTATE;   // (it reads int16 rows only: a float stream is refused, m17hip_tune key 11)
            else {
                if (pol) return M17HIP_EINVAL;   // (it has no per-channel form: refused, not computed under the flag alone)
                dim3 grid((T + FIR_TILE - 1) / FIR_TILE, C);
                tm.launch((fir_rrc150_rolled_kernel<FIR_R, 4>), grid, dim3(FIR_THREADS), 0, st, x + t0, c->xpitch, c->now().y + t0, c->ypitch, T, flags, c->taps);
                HIPCHK(c, hipGetLastError());
                return M17HIP_OK;
            }
        }
#endif
        const uint32_t tiles = (T + FS_TILE - 1) / FS_TILE;
        const uint64_t items64 = (uint64_t)tiles * C;
        if (items64 > 0xFFFFFFFFull) return M17HIP_EINVAL;
        const uint32_t items = (uint32_t)items64;
        const uint32_t per = latency ? FIR_ITEMS_LATENCY : FIR_ITEMS_THROUGHPUT;
        const uint32_t cap = c->fir_grid ? c->fir_grid : std::max(FIR_GRID_PER_CU * c->n_cu, (items + per - 1) / per);
        const dim3 grid(std::min(items, cap));
        const auto go = [&](auto kernel) {   // (pol, flip: read by the mixed form only)
            tm.launch(kernel, grid, dim3(FS_THREADS), 0, st, x + t0, c->xpitch, c->now().y + t0, c->ypitch, T, c->taps_skew, tiles, items, first_needed, pol, pol ? flags & 1u : 0u);
        };
        if (pol) go(fir_kernel<false, true>(x));
        else if (flags & 1u) go(fir_kernel<true, false>(x));
        else go(fir_kernel<false, false>(x));
        HIPCHK(c, hipGetLastError());
        return M17HIP_OK;
    });
}
// `pos`: the stream position of the slab's first sample (of the run, where t0 names a segment); `latency`: the four-wave pipeline where the piece allows it
int launch_dcd(m17hip_ctx* c, uint32_t C, uint32_t T, uint32_t flags, uint64_t pos, bool latency, hipStream_t st, uint32_t t0 = 0, const uint32_t* pol = nullptr)
{
    TimedK tm(c, KT_DCD);
    // table rows are numbered from the first tick of the RUN: a later segment continues where the previous one stopped
    const uint64_t row0 = (pos + t0) / TICK - pos / TICK;
    // (the pipeline needs whole 32-sample blocks that start on a block boundary of the stream: ragged pieces take the one-wave form)
    const bool one_wave = !latency || T % DP_BLK != 0 || (pos + t0) % DP_BLK != 0 || t0 % 8 != 0 || T < 4 * DP_BLK;
    const dim3 grid(one_wave ? (C + DCD_CPW * DCD_WPB - 1) / (DCD_CPW * DCD_WPB) : (C + DP_CPB - 1) / DP_CPB), block(one_wave ? 64 * DCD_WPB : 256);
    with_x(c, c->slot, [&](auto* x) {
        const auto go = [&](auto kernel) {   // (pol: read by the mixed form only)
            tm.launch(kernel, grid, block, 0, st, x + t0, c->xpitch, c->dcd_state, c->now().dcd + row0 * 12, c->ticks_cap, C, T, pos + t0, c->coef, flags, pol);
        };
        if (pol) go(dcd_kernel_of<false, true>(x, one_wave));
        else if (flags & 1u) go(dcd_kernel_of<true, false>(x, one_wave));
        else go(dcd_kernel_of<false, false>(x, one_wave));
    });
    HIPCHK(c, hipGetLastError());
    return M17HIP_OK;
}

// The polarity of channels [0, C) in a call made with `flags`: entry XOR bit 0 of flags (m17hip_set_channel_polarity).  Of one polarity (no table, all
// 0, all 1): kflags carries it in bit 0 and pol stays nullptr — what a context without a table passes.  Mixed: kflags = flags, pol = the device table,
// brought up to date first where the host's has changed: the copy goes to `first`, the stream whose kernels read it first (or that they are ordered behind).
int resolve_polarity(m17hip_ctx* c, uint32_t C, uint32_t flags, hipStream_t first, uint32_t& kflags, const uint32_t*& pol)
{
    kflags = flags; pol = nullptr;
    if (!c->pol_ones) return M17HIP_OK;
    const uint32_t ones = (uint32_t)std::count(c->pol_host.begin(), c->pol_host.begin() + C, (uint8_t)1);
    if (ones == 0) return M17HIP_OK;
    if (ones == C) { kflags = flags ^ 1u; return M17HIP_OK; }
    if (c->pol_dirty || !c->pol_table.live()) {
        const struct { Reader which; hipStream_t st; } readers[4] = {{RD_MAIN, c->stream}, {RD_DCD, c->side}, {RD_FIR, c->side2}, {RD_REPLAY, c->side3}};
        if (c->pol_table.live())   // the turn passes on: whatever reads the table in use has been queued by now
            for (const auto& rd : readers) HIPCHK(c, c->pol_table.after_read(rd.which, rd.st));
        uint32_t* staging;
        HIPCHK(c, c->pol_table.begin_write(c->maxC, &staging));
        for (uint32_t ch = 0; ch < c->maxC; ++ch) staging[ch] = c->pol_host[ch];
        HIPCHK(c, c->pol_table.publish(c->maxC, first));
        for (const auto& rd : readers) HIPCHK(c, c->pol_table.before_read(rd.st));
        c->pol_dirty = false;
    }
    pol = c->pol_table.dev();
    return M17HIP_OK;
}

}  // namespace

extern "C" {

const char* m17hip_strerror(int code)
{
    switch (code) {
    case M17HIP_OK: return "ok";
    case M17HIP_EINVAL: return "invalid argument";
    case M17HIP_EHIP: return "HIP runtime error";
    case M17HIP_ENOMEM: return "out of memory";
    case M17HIP_ESTATE: return "call sequence error";
    case M17HIP_EOVERFLOW: return "frame record buffer overflow";
    case M17HIP_ETRUNC: return "output truncated to the caller's capacity";
    case M17HIP_ECOMM: return "RCCL communication error";
    case M17HIP_ECONFIG: return "GPU_MAX_HW_QUEUES is unset or below 8: a context's streams would share hardware queues and serialise (export GPU_MAX_HW_QUEUES=16 before the process's first HIP call, or M17HIP_FEW_HW_QUEUES_OK=1 to go on regardless)";
    default: return "unknown error";
    }
}
int m17hip_last_hip_error(const m17hip_ctx* ctx) { return ctx ? ctx->last_hip : 0; }
// The streams of a context — main, carrier-detect (K3), matched filter (K1), replay (K2 ahead / redo), and the copy / payload stream once something is staged —
// are created by the library in ONE go in a fixed role order, and when a context goes they are parked as a SET: the next context of that device gets the same
// streams in the same roles.  Which role streams share a hardware pipe decides 10-40 % of a continued stream's step time (NOTES 4.14, 5.3, 5.10), the runtime maps
// streams to pipes in creation order, and a process that creates and destroys contexts beside a host's own streams walks through the bad layouts
// (tools/stream_history.py: 24.3 -> 26.2 -> 31.8 ms per step over three cycles with per-context streams and a host main stream; 22.1-22.5 in every cycle this way).
// M17HIP_STREAM_SETS=0 in the environment restores per-context streams on the default stream (tools/stream_history.py's A/B).
struct StreamSet { hipStream_t main, side, side2, side3, copy; int device; };
// (heap-allocated once and never destroyed, like the run registry: a context destroyed during static destruction at process exit still finds it)
struct StreamSets { std::mutex mu; std::vector<StreamSet> parked; };
static StreamSets& g_sets_ref() { static StreamSets* r = new StreamSets; return *r; }
#define g_sets (g_sets_ref())
static int stream_set_mode()
{
    const char* e = getenv("M17HIP_STREAM_SETS");
    return (e && atoi(e) == 0) ? 0 : 1;
}

static int hw_queues_env()   // what the process asked the HIP runtime for (the runtime's default is 4)
{
    const char* q = std::getenv("GPU_MAX_HW_QUEUES");
    return q ? std::atoi(q) : 4;
}
int m17hip_advice(const m17hip_ctx* ctx)
{
    if (!ctx) return 0;
    const int n = hw_queues_env();
    return (n < 8 ? M17HIP_ADVICE_HW_QUEUES : 0) | (n < 16 ? M17HIP_ADVICE_HW_QUEUES_16 : 0);
}
int m17hip_version(void) { return 622; }

// The two device tables every matched-filter form reads (c->taps: K5, K2, the rolled K1; c->taps_skew: the skew K1 forms), from taps149 or, for
// nullptr, the RRC taps.  Tap 150 (and the padding behind it) is zero.  Blocking copies: the caller has nothing in flight that reads them.
static hipError_t write_fir_taps(m17hip_ctx* c, const float* taps149)
{
    float taps[160] = {0};
    for (int i = 0; i < NTAPS; ++i) taps[i] = taps149 ? taps149[i] : rrc_tap(i);
    hipError_t e = hipMemcpy(c->taps, taps, sizeof(taps), hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
    float skew[FS_NBODY * FS_TAB];
    fs_build_tap_table(skew, taps149);
    return hipMemcpy(c->taps_skew, skew, sizeof(skew), hipMemcpyHostToDevice);
}

int m17hip_ctx_create(int device, uint32_t max_channels, uint32_t max_samples, m17hip_ctx** out)
{
    if (!out || max_channels == 0 || max_samples == 0 || max_samples > M17HIP_MAX_SAMPLES_PER_RUN) return M17HIP_EINVAL;   // (argument checks: before any HIP call)
    // The slow state is not entered silently: with the runtime's default of four hardware queues the five streams of a context share queues,
    // a kernel queued behind another stream's event wait waits with it, and a step takes 1.4-1.6 x as long (NOTES 4.14, 5.3).
    if (hw_queues_env() < 8) {
        const char* ok = std::getenv("M17HIP_FEW_HW_QUEUES_OK");
        if (!ok || std::atoi(ok) == 0) return M17HIP_ECONFIG;
    }
    m17hip_ctx* c = new (std::nothrow) m17hip_ctx();
    if (!c) return M17HIP_ENOMEM;
    c->device = device;
    c->maxC = max_channels;
    c->maxT = max_samples;
    auto fail = [&](int code) { m17hip_ctx_destroy(c); return code; };
    DeviceGuard guard_(c);
    if (!guard_.ok) return fail(M17HIP_EHIP);
    c->xpitch = round_up((size_t)XPRE + max_samples + 8, 8);
    c->ypitch = round_up((size_t)YPRE + max_samples + 4, 4);
    // K2 stores the limit-filter history of a workgroup's GT_CPW channel rows through ONE buffer descriptor with 32-bit byte offsets
    // (m17_gate_kernel.hpp, limit_track_pass): the rows of a workgroup must fit below the offset that stands for "no store"
    static_assert(M17HIP_MAX_SAMPLES_PER_RUN == (0x7FFF0000u / (4u * GT_CPW)) - 256u, "include/m17hip.h: M17HIP_MAX_SAMPLES_PER_RUN");
    if ((size_t)GT_CPW * c->ypitch * 4u > (size_t)0x7FFF0000u) return fail(M17HIP_EINVAL);
    c->ticks_cap = max_samples / TICK + 2;
    c->rec_cap = c->rec_cap_alloc = 2 * (max_samples / 1920 + 2) + 4;  // <= 2 callbacks per 1920-sample frame
    const size_t C = max_channels;
    int r = M17HIP_OK;   // (the first allocation that fails ends the creation)
    auto alloc = [&](auto& buf, size_t n) { if (!r) r = alloc_code(c, buf.alloc(n)); };
    m17hip_ctx::Slab& s = c->slab[0];   // (the second pair: the first time input is staged, stage_prepare)
    alloc(s.x, C * c->xpitch);
    alloc(s.y, C * c->ypitch);
    alloc(s.h, C * c->ypitch);
    alloc(c->final_h, 2 * C * 4);
    alloc(c->gate_exp, C);
    alloc(c->dropped, 2 * C);
    alloc(c->bert.state, C);
    alloc(s.dcd, C * c->ticks_cap * 12);
    alloc(c->dcd_state, C);
    alloc(c->seq_state, C);
    alloc(c->evm.state, C);
    alloc(c->evm, C);
    alloc(c->sets[0].recs, C * c->rec_cap);      // (the second set: with the second run, m17hip_demod_run)
    alloc(c->sets[0].rec_count, C);
    alloc(c->rec_offsets, C + 1);
    alloc(c->overflow, 8);
    alloc(c->tables, 1);
    alloc(c->taps, 160);
    alloc(c->taps_skew, FS_NBODY * FS_TAB);
    alloc(c->llr_edges, 64);
    alloc(c->level_gain, 8 * (size_t)core::LEVEL_SCHED_N);
    alloc(c->dbg, (C + 1) * DBG_SLOTS);   // (tools build: per-wave counters of K5)
    if (r) return fail(r);
    c->sets[0].ovf = c->overflow; c->sets[1].ovf = c->overflow + 4;
    // (a gate-aware K1 leaves tiles unwritten: what K2's replay may read there must be finite.  A memset is queued, not done, when it returns: wait —
    //  the first run's K1 is on a stream of its own that would not)
    if (hipMemset(s.y, 0, C * c->ypitch * sizeof(float)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(M17HIP_EHIP);
    if (c->bert.reset(c, 0)) return fail(M17HIP_EHIP);
    {
        DecodeTables* t = new DecodeTables;
        build_tables(*t);
        hipError_t e = hipMemcpy(c->tables, t, sizeof(DecodeTables), hipMemcpyHostToDevice);
        delete t;
        if (e != hipSuccess) { c->last_hip = (int)e; return fail(M17HIP_EHIP); }
        float edges[64] = {0};
        build_llr_edges(edges);
        if (write_fir_taps(c, nullptr) != hipSuccess) return fail(M17HIP_EHIP);
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu <= 0) return fail(M17HIP_EHIP);
        c->n_cu = (uint32_t)ncu;
        if (hipMemcpy(c->llr_edges, edges, sizeof(edges), hipMemcpyHostToDevice) != hipSuccess) return fail(M17HIP_EHIP);
        std::vector<core::Kalman2Gain> sched(8 * (size_t)core::LEVEL_SCHED_N);
        for (uint32_t o = 0; o < 8; ++o)   // (false = the covariance has not reached its fixed point inside the table: the scheduled update would be wrong)
            if (!core::level_schedule(sched.data() + (size_t)o * core::LEVEL_SCHED_N, o)) return fail(M17HIP_ESTATE);
        if (hipMemcpy(c->level_gain, sched.data(), sched.size() * sizeof(core::Kalman2Gain), hipMemcpyHostToDevice) != hipSuccess) return fail(M17HIP_EHIP);
    }
    c->coef = build_coef();
    c->set_mode = stream_set_mode();
    bool parked = false;
    if (c->set_mode) {
        std::lock_guard<std::mutex> lk(g_sets.mu);
        for (size_t i = g_sets.parked.size(); i-- > 0;)   // (the set parked last)
            if (g_sets.parked[i].device == device) {
                const StreamSet& ss = g_sets.parked[i];
                c->own_main = ss.main; c->side = ss.side; c->side2 = ss.side2; c->side3 = ss.side3; c->copy = ss.copy;
                g_sets.parked.erase(g_sets.parked.begin() + (long)i);
                parked = true;
                break;
            }
    }
    if (!parked) {
        // (the copy stream joins the set when something is staged — stage_prepare: created here with the others, two batches measured 21.5 against 21.1 ms)
        // (the ORDER of the four inside the set does not matter: all 24 measured, two batches 20.3-20.6, continued stream 21.3-21.7 ms on one box — NOTES 6.6)
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return fail(M17HIP_EHIP);
        auto make_set = [&](StreamSet& ss) -> bool {
            ss = StreamSet{nullptr, nullptr, nullptr, nullptr, nullptr, device};
            if (c->set_mode && hipStreamCreateWithFlags(&ss.main, hipStreamNonBlocking) != hipSuccess) return false;
            if (hipStreamCreateWithFlags(&ss.side, hipStreamNonBlocking) != hipSuccess) return false;
            if (hipStreamCreateWithFlags(&ss.side2, hipStreamNonBlocking) != hipSuccess) return false;
            // the replay stream outranks the others: its few workgroups must not queue behind K5's thousand.  (K1's stream at the LOWEST priority
            // was tried: a continued stream of 2 x 2048 channels 24.6 -> 22.8 ms in a process with history, but 2 x 1024 channels 11.5 -> 16.1 ms —
            // K1 starves behind the other group's kernels: NOTES 5.10.)
            return hipStreamCreateWithPriority(&ss.side3, hipStreamNonBlocking, greatest) == hipSuccess;
        };
        StreamSet mine;
        if (!make_set(mine)) return fail(M17HIP_EHIP);
        c->own_main = mine.main; c->side = mine.side; c->side2 = mine.side2; c->side3 = mine.side3;
        // (creating the sets two at a time — a spare right behind every new set, so that the sets of two contexts sit side by side whatever the host creates in
        //  between — was measured: two batches 20.6-20.9 ms in all four layouts of tools/bisect_bench.py against 20.7 / 21.6 / 20.7 / 21.3; but four more queues per
        //  process: four rank processes on one GPU, 32 + queues in all, ran tests/test_gpu_gather_ranks.py twice as long.  Not kept: NOTES 6.6)
    }
    if (c->own_main) c->stream = c->own_main;
    for (Event* e : {&c->ev_fork, &c->ev_join, &c->ev_mark, &c->ev_tail, &c->slab[0].end, &c->slab[1].end})
        if (e->create() != hipSuccess) return fail(M17HIP_EHIP);
    if (hipFuncSetAttribute((const void*)viterbi_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (122 + 122 + 16) * 64 * 4) != hipSuccess)
        return fail(M17HIP_EHIP);
    if (hipFuncSetAttribute((const void*)decode_deferred_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, DEFER_LDS_BYTES) != hipSuccess)
        return fail(M17HIP_EHIP);
    if (hipFuncSetAttribute((const void*)decode_frames_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (92 + 122 + 16) * 64 * 4) != hipSuccess)
        return fail(M17HIP_EHIP);
    if (hipFuncSetAttribute((const void*)decode_seq_lane_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (92 + 122 + 16) * 64 * 4) != hipSuccess)
        return fail(M17HIP_EHIP);
    if (hipMemset(c->overflow, 0, 32) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(M17HIP_EHIP);   // (default-stream work of the creation is through before the context's own streams start)
    for (Event* e : {&c->sets[0].done, &c->sets[1].done, &c->sets[0].chain, &c->sets[1].chain, &c->ev_dst, &c->ev_switch, &c->ev_fetch})
        if (e->create() != hipSuccess) return fail(M17HIP_EHIP);
    { std::lock_guard<std::mutex> lk(g_runs.mu); c->seen_overlap = g_runs.overlaps; g_runs.ctxs.push_back(c); }   // (a new context has seen no overlap yet)
    *out = c;
    if ((r = m17hip_demod_reset(c)) != M17HIP_OK) { *out = nullptr; return fail(r); }
    return M17HIP_OK;
}

void m17hip_ctx_destroy(m17hip_ctx* c)
{
    if (!c) return;
    {
        std::lock_guard<std::mutex> lk(g_runs.mu);
        for (size_t i = 0; i < g_runs.ctxs.size(); ++i)
            if (g_runs.ctxs[i] == c) { g_runs.ctxs.erase(g_runs.ctxs.begin() + (long)i); break; }
    }
    DeviceGuard guard_(c);
    drain_timing(c);
    const bool any_foreign = c->foreign_streams[0] || c->foreign_streams[1] || c->foreign_streams[2] || c->foreign_streams[3];
    if (c->set_mode && !any_foreign && c->own_main && c->side && c->side2 && c->side3) {
        // the set is parked as a SET: the next context of this device gets the same five streams in the same roles
        for (hipStream_t st : {c->own_main, c->side, c->side2, c->side3, c->copy})
            if (st) (void)hipStreamSynchronize(st);
        std::lock_guard<std::mutex> lk(g_sets.mu);
        g_sets.parked.push_back(StreamSet{c->own_main, c->side, c->side2, c->side3, c->copy, c->device});
    } else {
        if (c->own_main) hipStreamDestroy(c->own_main);
        if (c->side && !c->foreign_streams[0]) hipStreamDestroy(c->side);
        if (c->side2 && !c->foreign_streams[1]) hipStreamDestroy(c->side2);
        if (c->side3 && !c->foreign_streams[2]) hipStreamDestroy(c->side3);
        if (c->copy && !c->foreign_streams[3]) hipStreamDestroy(c->copy);
    }
    delete c;   // (its members give the device memory and the events back — on the context's device: the guard still holds it)
}

int m17hip_get_stream(m17hip_ctx* c, void** hip_stream)
{
    if (!c || !hip_stream) return M17HIP_EINVAL;
    *hip_stream = (void*)c->stream;
    return M17HIP_OK;
}

int m17hip_set_stream(m17hip_ctx* c, void* hip_stream)
{
    if (!c) return M17HIP_EINVAL;
    GUARD(c);
    // an ordered switch: the new stream starts behind everything queued so far on the old one (a run in flight, its payload work, the reset
    // kernels of m17hip_ctx_create) and on the payload stream where that is another (the copy stream of a context that streams)
    const hipStream_t to = (hipStream_t)hip_stream;
    if (to != c->stream) {
        HIPCHK(c, hipEventRecord(c->ev_switch, c->stream));
        HIPCHK(c, hipStreamWaitEvent(to, c->ev_switch, 0));
        if (c->pay() != c->stream) {
            HIPCHK(c, hipEventRecord(c->ev_switch, c->pay()));
            HIPCHK(c, hipStreamWaitEvent(to, c->ev_switch, 0));
        }
    }
    c->stream = to;
    return M17HIP_OK;
}

// ---- staged input (streaming) -------------------------------------------------------------------------------------------
// Second slab pair, streams and events: allocated the first time input is staged.  (slot is 0 until a staged run begins, and that needs
// staged input: the second pair is slab[1].)
static int stage_prepare(m17hip_ctx* c)
{
    m17hip_ctx::Slab& s = c->slab[1];
    if (s.x) return M17HIP_OK;
    int r;   // (a call that failed half way is picked up where it stopped: nothing is allocated twice)
    const bool fresh_y = !s.y;
    if (!s.y && (r = alloc_code(c, s.y.alloc((size_t)c->maxC * c->ypitch)))) return r;
    if (!s.h && (r = alloc_code(c, s.h.alloc((size_t)c->maxC * c->ypitch)))) return r;
    if (!s.dcd && (r = alloc_code(c, s.dcd.alloc((size_t)c->maxC * c->ticks_cap * 12)))) return r;
    if (!c->copy) HIPCHK(c, hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking));
    // (zeroed as slab[0].y is — ON the copy stream: the staged run's K1 waits for that stream's ev_in_ready, a memset on the default stream would
    //  sit behind the run in flight and land in the middle of the staged one)
    if (fresh_y) HIPCHK(c, hipMemsetAsync(s.y, 0, (size_t)c->maxC * c->ypitch * sizeof(float), c->copy));
    if (!c->ev_copy) HIPCHK(c, c->ev_copy.create());
    if (!c->ev_in_ready) HIPCHK(c, c->ev_in_ready.create());
    // (from here on the copy stream is the PAYLOAD stream: behind the last reset, as m17hip_demod_reset orders the payload stream it sees)
    HIPCHK(c, hipStreamWaitEvent(c->copy, c->ev_mark, 0));
    return alloc_code(c, s.x.alloc((size_t)c->maxC * c->xpitch));   // last: its presence says "all of it is there"
}

extern "C++" {   // (templates)
// The float pair's slab of `slot` and the float history arrays, the first time they are needed.  A fresh slab's prefix is zeroed on `st` (the stream
// its input is written on): what a stream that begins in it finds where an int16 stream finds the prefix m17hip_demod_reset cleared.
static int ensure_f32(m17hip_ctx* c, int slot, hipStream_t st)
{
    int r;
    if (!c->hist_f || !c->bnd_hist_f) {
        if (!c->hist_f && (r = alloc_code(c, c->hist_f.alloc((size_t)c->maxC * HISTF_PITCH)))) return r;
        if (!c->bnd_hist_f && (r = alloc_code(c, c->bnd_hist_f.alloc(2 * (size_t)c->maxC * HISTF_PITCH)))) return r;
        HIPCHK(c, hipMemsetAsync(c->hist_f, 0, c->hist_f.size() * sizeof(float), c->stream));
        HIPCHK(c, hipMemsetAsync(c->bnd_hist_f, 0, c->bnd_hist_f.size() * sizeof(float), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (once per context: the replay reads them on a stream of its own)
    }
    if (!c->fslab[slot].x) {
        if ((r = alloc_code(c, c->fslab[slot].x.alloc((size_t)c->maxC * c->xpitch)))) return r;
        HIPCHK(c, hipMemset2DAsync(c->fslab[slot].x, c->xpitch * sizeof(float), 0, XPRE * sizeof(float), c->maxC, st));
    }
    return M17HIP_OK;
}
// input of format `fmt` is about to be written: refused on a stream of the other format
static int claim_format(const m17hip_ctx* c, int fmt) { return (c->stream_fmt && c->stream_fmt != fmt) ? M17HIP_ESTATE : M17HIP_OK; }

// Where a way in writes its rows: the current input slab on the main stream, or the STAGING slab on the copy stream, as soon as the run before the
// latest one has released it — `staged`: an _async entry point; or any in-place producer (m17hip_upload_i16 / _f32, their _device forms, the IQ and
// wideband ones, m17hip_synth_i16) under tuning knob 16.
template <typename XT> struct InputTarget { XT* x = nullptr; hipStream_t st = nullptr; bool stage = false; int slot = 0; };
template <typename XT>
static int input_target(m17hip_ctx* c, InputTarget<XT>& t, bool staged = false)
{
    int r;
    if ((r = claim_format(c, fmt_of<XT>()))) return r;
    if (!staged && !c->stage_inputs) { t.slot = c->slot; t.st = c->stream; t.stage = false; }
    else {
        if ((r = stage_prepare(c))) return r;
        // the staging slab was the input of the run BEFORE the one now queued / running: free once that run is done with it
        HIPCHK(c, c->other().wait_free(c->copy));
        t.slot = c->slot ^ 1; t.st = c->copy; t.stage = true;
    }
    if constexpr (std::is_same<XT, float>::value) if ((r = ensure_f32(c, t.slot, t.st))) return r;
    t.x = slab_x<XT>(c, t.slot);
    return M17HIP_OK;
}
template <typename XT>
static void input_done(m17hip_ctx* c, const InputTarget<XT>& t, uint32_t C, uint32_t T)
{
    c->stream_fmt = c->slab_fmt[t.slot] = fmt_of<XT>();
    if (t.stage) {
        c->staged = true; c->stagedC = C; c->stagedT = T; c->other().C = C; c->other().T = T;
        return;
    }
    c->uploaded = true;
    c->now().C = C; c->now().T = T;
    c->lastC = C;
    if (c->have_run) c->inplace_after_run = true;
}

// The frame of every way in (host or device rows of either format, IQ through the discriminator, a wideband block through the tuner or the channeliser),
// in place or staged for the next run.  `p`: the caller's rows or raw block.  `own()`: the checks particular to the way in, made once the common
// arguments are good; what it refuses is the call's result.  `produce(x, st)`: queues on `st` whatever writes C rows of T samples behind the prefix of x.
template <typename XT, typename Own, typename Produce>
static int upload_frame(m17hip_ctx* c, const void* p, uint32_t C, uint32_t T, bool staged, Own&& own, Produce&& produce)
{
    if (!c || !p || C == 0 || T == 0 || C > c->maxC || T > c->maxT) return M17HIP_EINVAL;
    if (int r = own()) return r;
    GUARD(c);
    if (c->front_queued) return M17HIP_ESTATE;   // the slabs belong to the run m17hip_demod_front has started
    InputTarget<XT> in;
    int r = input_target(c, in, staged);
    if (r) return r;
    if ((r = produce(in.x, in.st))) return r;
    if (staged) HIPCHK(c, hipEventRecord(c->ev_copy, c->copy));
    else HIPCHK(c, hipStreamSynchronize(in.st));   // the caller's memory belongs to the caller again when this returns
    input_done(c, in, C, T);
    return M17HIP_OK;
}

// Rows from host or device memory, for either format (the C entry points below name the instantiations).
template <typename XT>
static int upload_host(m17hip_ctx* c, const XT* host, uint32_t C, uint32_t T, size_t pitch, bool staged)
{
    return upload_frame<XT>(c, host, C, T, staged, [&] { return pitch < T ? M17HIP_EINVAL : M17HIP_OK; }, [&](XT* x, hipStream_t st) -> int {
        HIPCHK(c, hipMemcpy2DAsync(x + XPRE, c->xpitch * sizeof(XT), host, pitch * sizeof(XT), (size_t)T * sizeof(XT), C, hipMemcpyHostToDevice, st));
        return M17HIP_OK;
    });
}
template <typename XT>
static int upload_dev(m17hip_ctx* c, const XT* dev, uint32_t C, uint32_t T, size_t pitch, bool staged)
{
    return upload_frame<XT>(c, dev, C, T, staged, [&] { return pitch < T ? M17HIP_EINVAL : M17HIP_OK; }, [&](XT* x, hipStream_t st) -> int {
        constexpr uint32_t N = 16 / sizeof(XT);   // (samples per lane: copy_rows_kernel)
        hipLaunchKernelGGL(copy_rows_kernel<XT>, dim3(((T + N - 1) / N + 255) / 256, C), dim3(256), 0, st, dev, pitch, x, c->xpitch, T);
        HIPCHK(c, hipGetLastError());
        return M17HIP_OK;
    });
}
template <typename XT>
static int download_host(m17hip_ctx* c, XT* host, uint32_t C, uint32_t T, size_t pitch)
{
    if (!c || !host || C == 0 || T == 0 || C > c->maxC || T > c->maxT || pitch < T) return M17HIP_EINVAL;
    GUARD(c);
    if (!c->uploaded || c->slab_fmt[c->slot] != fmt_of<XT>()) return M17HIP_ESTATE;   // (nothing there, or input of the other format)
    HIPCHK(c, hipMemcpy2DAsync(host, pitch * sizeof(XT), slab_x<XT>(c, c->slot) + XPRE, c->xpitch * sizeof(XT), (size_t)T * sizeof(XT), C, hipMemcpyDeviceToHost,
                               c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return M17HIP_OK;
}

// ---- complex IQ input (ABI 608): the FM discriminator in front of the float slab -----------------------------------------------------------
// `st` is about to read or write the IQ carry (or the raw-IQ buffer): behind the latest launch that did, where that was on the other stream
static int iq_order(m17hip_ctx* c, hipStream_t st)
{
    if (c->iq_last && c->iq_last != st) HIPCHK(c, hipStreamWaitEvent(st, c->ev_iq, 0));
    return M17HIP_OK;
}
static int iq_mark(m17hip_ctx* c, hipStream_t st)
{
    HIPCHK(c, hipEventRecord(c->ev_iq, st));
    c->iq_last = st;
    return M17HIP_OK;
}
// the carry, the first time an IQ block arrives: zeroed on the stream that block's discriminator runs on
static int ensure_iq(m17hip_ctx* c, hipStream_t st)
{
    if (c->iq_carry) return M17HIP_OK;
    if (!c->ev_iq) HIPCHK(c, c->ev_iq.create());
    if (int r = alloc_code(c, c->iq_carry.alloc(c->maxC))) return r;
    HIPCHK(c, hipMemsetAsync(c->iq_carry, 0, (size_t)c->maxC * sizeof(float2), st));
    return iq_mark(c, st);
}
// A fresh feed for every channel (m17hip_demod_reset) or for the listed ones (m17hip_demod_reset_channels: one memset per run of consecutive channels;
// nothing is copied to the device and the host waits for nothing).  On the stream of the latest IQ launch: IQ blocks uploaded from here on find the zeroes.
static int iq_fresh_feed(m17hip_ctx* c, const uint32_t* channels, uint32_t n)
{
    if (!c->iq_carry) return M17HIP_OK;
    const hipStream_t st = c->iq_last;
    if (!channels) {
        HIPCHK(c, hipMemsetAsync(c->iq_carry, 0, (size_t)c->maxC * sizeof(float2), st));
        if (c->wide.S) {   // (the wideband sources' feeds as well: histories and sample count; the listed form leaves them alone — they are not a channel's)
            for (auto& h : c->wide.hist) HIPCHK(c, hipMemsetAsync(h, 0, h.size() * sizeof(float2), st));
            c->wide.count = 0;
            c->wide.sv.forget();   // (the planes were blocks of the feed that ends here)
            c->wide.sp.forget();
            c->wide.mt.forget();   // (the meter stays on: its windows start over with the feed)
            c->wide.mt.outputs = 0;
            c->wide.sq.forget();   // (the squelch stays on: every channel's hold count starts over)
            c->wide.sq.fresh = true;
            c->wide.sc.forget();   // (the scan likewise: its slots take their seeds again)
        }
    } else {
        auto& sq = c->wide.sq;
        // the listed channels' hold counts as well.  Not while `fresh` is set: the next squelched block then zeroes the WHOLE array on its stream before its
        // kernel reads a count (launch_squelch), so nothing that stands in it now is ever read
        const bool hold = c->wide.S && sq.hold && !sq.fresh;
        std::vector<uint32_t> v(channels, channels + n);
        std::sort(v.begin(), v.end());
        for (size_t i = 0; i < v.size();) {
            size_t j = i + 1;
            while (j < v.size() && v[j] <= v[j - 1] + 1u) ++j;
            HIPCHK(c, hipMemsetAsync(c->iq_carry.get() + v[i], 0, (size_t)(v[j - 1] - v[i] + 1u) * sizeof(float2), st));
            if (hold) HIPCHK(c, hipMemsetAsync(sq.hold.get() + v[i], 0, (size_t)(v[j - 1] - v[i] + 1u) * sizeof(uint32_t), st));
            i = j;
        }
    }
    return iq_mark(c, st);
}
template <typename IQT>
static int launch_discriminate(m17hip_ctx* c, const void* dev, size_t pitch, float* x, uint32_t C, uint32_t T, float gain, hipStream_t st)
{
    const IQT* src = static_cast<const IQT*>(dev);
    {
        TimedK tm(c, KT_IQ);
        tm.launch(discriminate_kernel<IQT>, dim3(((T + IQ_LANE - 1) / IQ_LANE + IQ_THREADS - 1) / IQ_THREADS, C), dim3(IQ_THREADS), 0, st, src, pitch, x, c->xpitch, T,
                  c->iq_carry.get(), gain);
    }
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(iq_carry_kernel<IQT>, dim3((C + 63) / 64), dim3(64), 0, st, src, pitch, T, c->iq_carry.get(), C);   // (behind it: the next block's carry)
    HIPCHK(c, hipGetLastError());
    return iq_mark(c, st);
}
// f(a value of the type the IQ samples of format `fmt` have — short2, float2 or uchar2); what f returns
template <typename F> static auto with_iq_type(int fmt, F&& f)
{
    return fmt == M17HIP_IQ_I16 ? f(short2{}) : fmt == M17HIP_IQ_F32 ? f(float2{}) : f(uchar2{});
}
static size_t iq_sample_bytes(int fmt) { return with_iq_type(fmt, [](auto s) { return sizeof(s); }); }
// The raw block of a host form (IQ, wideband) into the context's own buffer first, on `st`: `rows` rows of `samples` samples of `sb` bytes from the caller's
// `dev` (pitch in samples), into rows of a multiple of four samples (16-byte loads).  Afterwards `dev` and `pitch` name the buffer.
static int stage_raw(m17hip_ctx* c, uint32_t rows, size_t samples, size_t sb, hipStream_t st, const void*& dev, size_t& pitch)
{
    const size_t rp = round_up(samples, IQ_LANE);
    if (c->iq_raw.size() < (size_t)rows * rp * sb) {
        HIPCHK(c, hipEventSynchronize(c->ev_iq));   // (the block before may still be read)
        if (int r = alloc_code(c, c->iq_raw.grow((size_t)rows * rp * sb, &c->last_hip))) return r;
    }
    HIPCHK(c, hipMemcpy2DAsync(c->iq_raw, rp * sb, dev, pitch * sb, samples * sb, rows, hipMemcpyHostToDevice, st));
    dev = c->iq_raw; pitch = rp;
    return M17HIP_OK;
}
// The four ways in (`how`: from host memory / staged for the next run) through the frame of all of them: the discriminator takes the place of the copy.
enum { IQ_FROM_HOST = 1, IQ_STAGED = 2 };
static int upload_iq(m17hip_ctx* c, const void* p, int iq_format, float gain, uint32_t C, uint32_t T, size_t pitch, int how)
{
    const auto own = [&] {
        if (pitch < T || (iq_format != M17HIP_IQ_I16 && iq_format != M17HIP_IQ_F32)) return M17HIP_EINVAL;   // (no discriminator reads 8-bit samples)
        return std::isfinite(gain) && gain > 0.0f ? M17HIP_OK : M17HIP_EINVAL;
    };
    return upload_frame<float>(c, p, C, T, (how & IQ_STAGED) != 0, own, [&](float* x, hipStream_t st) -> int {
        int r;
        if ((r = ensure_iq(c, st))) return r;
        if ((r = iq_order(c, st))) return r;
        const void* dev = p;
        if ((how & IQ_FROM_HOST) && (r = stage_raw(c, C, T, iq_sample_bytes(iq_format), st, dev, pitch))) return r;
        return with_iq_type(iq_format, [&](auto s) -> int {
            if constexpr (std::is_same<decltype(s), uchar2>::value) return M17HIP_EINVAL;   // (refused above)
            else return launch_discriminate<decltype(s)>(c, dev, pitch, x, C, T, gain, st);
        });
    });
}

// ---- wideband IQ input (ABI 609): the tuner in front of the float slab -----------------------------------------------------------------------
// Blackman-windowed sinc of L taps, cutoff fc (cycles per sample), in double; DC gain `gain` (1: the quotient as it is), then rounded to float
static void windowed_sinc(uint32_t L, double fc, float* taps, double gain = 1.0)
{
    const double pi = 3.14159265358979323846, mid = 0.5 * (L - 1);
    std::vector<double> h(L);
    double sum = 0.0;
    for (uint32_t i = 0; i < L; ++i) {
        const double t = (double)i - mid, x = 2.0 * pi * fc * t;
        const double sinc = t == 0.0 ? 2.0 * fc : std::sin(x) / (pi * t);
        const double w = 0.42 - 0.5 * std::cos(2.0 * pi * i / (L - 1)) + 0.08 * std::cos(4.0 * pi * i / (L - 1));
        h[i] = sinc * w;
        sum += h[i];
    }
    for (uint32_t i = 0; i < L; ++i) taps[i] = (float)(h[i] / sum * gain);
}
// The channel filter: cutoff 5500 Hz at 48000 * decim, 32 * decim + 1 taps
static void wide_default(uint32_t R, float* taps) { windowed_sinc(32 * R + 1, 5500.0 / (48000.0 * R), taps); }
// The first of two stages (ABI 610): all it has to do is keep what the first decimation folds onto the channel out of it.  Cutoff 24000 * R2 Hz at
// 48000 * R1 * R2 (half the rate it leaves), 8 * R1 + 1 taps.  R1 = 1: one tap of 1.
static void wide_default1(uint32_t R1, uint32_t R2, float* taps)
{
    if (R1 == 1) { taps[0] = 1.0f; return; }
    windowed_sinc(8 * R1 + 1, 24000.0 * R2 / (48000.0 * R1 * R2), taps);
}
// The survey of one block (m17hip_wide_survey is on), queued behind chan_kernel on the block's stream: it reads what chan_kernel read — src, w.hist[w.par],
// w.count — and writes the plane whose turn it is.  A block without a survey time (J = 0) queues the second kernel alone: its plane is all +0.
template <typename IQT>
static int launch_survey(m17hip_ctx* c, const IQT* src, size_t pitch, uint32_t W, uint32_t T, hipStream_t st)
{
    auto& w = c->wide;
    auto& sv = w.sv;
    const uint64_t N0 = w.count / w.R;
    const uint32_t first = (uint32_t)((sv.stride - (N0 + 1) % sv.stride) % sv.stride);
    const uint32_t J = first < T ? (T - 1 - first) / sv.stride + 1 : 0;
    const uint32_t G = (J + core::CHAN_SURVEY_GROUP - 1) / core::CHAN_SURVEY_GROUP;
    const int p = sv.latest ^ 1;
    int r;
    if (!sv.fetch) HIPCHK(c, hipStreamCreateWithFlags(&sv.fetch, hipStreamNonBlocking));
    for (auto& e : sv.ev) if (!e) HIPCHK(c, e.create());
    for (auto& b : sv.plane) if ((r = alloc_code(c, b.grow((size_t)w.S * w.M, &c->last_hip)))) return r;   // (released with every configuration: nothing reads them)
    if (sv.scratch.size() < (size_t)w.S * G * w.M) {
        HIPCHK(c, hipEventSynchronize(c->ev_iq));   // (the block before may still be surveyed)
        if ((r = alloc_code(c, sv.scratch.grow((size_t)w.S * G * w.M, &c->last_hip)))) return r;
    }
    sv.valid[p] = false;
    {
        Timed tm(c, KT_SURVEY, st);
        if (G) {
            const uint32_t WP = survey_wpitch(w.L, w.R, sv.stride), TS = survey_tile(w.L, WP, w.M);
            hipLaunchKernelGGL(chan_survey_kernel<IQT>, dim3(G, w.S), dim3(SURVEY_THREADS), survey_lds_bytes(w.L, WP, w.M, TS), st, src, pitch, W,
                               w.hist[w.par].get(), w.taps.get(), w.L, w.R, w.M1, w.M2, w.tw.get(), (uint32_t)(w.count % w.M), first, sv.stride, J, WP, TS,
                               sv.scratch.get());
            HIPCHK(c, hipGetLastError());
        }
        hipLaunchKernelGGL(chan_survey_sum_kernel, dim3((w.S * w.M + 255) / 256), dim3(256), 0, st, sv.scratch.get(), G, w.M, w.S, sv.plane[p].get());
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(sv.ev[p], st));
    sv.times[p] = J; sv.first_output[p] = N0; sv.valid[p] = true; sv.latest = p;
    return M17HIP_OK;
}
// The spectrum of one block (m17hip_wide_spectrum is on), on the block's stream: it reads src and w.count alone, and writes the plane whose turn it is.  A
// block without a frame (J = 0) queues the second kernel alone: its plane is all +0.
template <typename IQT>
static int launch_spectrum(m17hip_ctx* c, const IQT* src, size_t pitch, uint32_t W, hipStream_t st)
{
    auto& w = c->wide;
    auto& sp = w.sp;
    const uint32_t N = sp.points;
    uint32_t first, J;
    core::spec_frames(w.count, W, N, sp.hop, first, J);
    const uint32_t G = (J + core::CHAN_SURVEY_GROUP - 1) / core::CHAN_SURVEY_GROUP;
    const int p = sp.latest ^ 1;
    int r;
    if (!sp.fetch) HIPCHK(c, hipStreamCreateWithFlags(&sp.fetch, hipStreamNonBlocking));
    for (auto& e : sp.ev) if (!e) HIPCHK(c, e.create());
    // The planes are regrown where `points` has risen since they were made (m17hip_wide_spectrum never frees: its call waits for nothing).  The block before
    // may still be writing the old ones then — its sum kernel is the last but one of its chain, and `st` has only been put behind ev_iq, the host has not
    // waited.  What orders the release behind that writer is hipFree itself, which synchronises the device before it frees (documented in
    // hip_runtime_api.h): this upload then returns no earlier than the block before ends (tests/test_gpu_call_orders_spectrum.py: 9.3 - 9.7 ms with a
    // tuner of 7.5 ms in flight).  A release that does not wait (a pool, hipFreeAsync) needs hipEventSynchronize(c->ev_iq) here, as the scratch below has.
    for (auto& b : sp.plane) if ((r = alloc_code(c, b.grow((size_t)w.S * N, &c->last_hip)))) return r;
    if (sp.scratch.size() < (size_t)w.S * G * N) {
        HIPCHK(c, hipEventSynchronize(c->ev_iq));   // (the block before may still be transformed)
        if ((r = alloc_code(c, sp.scratch.grow((size_t)w.S * G * N, &c->last_hip)))) return r;
    }
    if (sp.dirty || !sp.dev.live()) {   // the window and the twiddles, into the copy no queued launch reads
        uint32_t* staging = nullptr;
        HIPCHK(c, sp.dev.begin_write(2 * 4096, &staging));
        std::memcpy(staging, sp.table.data(), sp.table.size() * 4);
        HIPCHK(c, sp.dev.publish(sp.table.size(), st));
        sp.dirty = false;
    }
    HIPCHK(c, sp.dev.before_read(st));
    sp.valid[p] = false;
    {
        Timed tm(c, KT_SPECTRUM, st);
        if (G) {
            const uint32_t F = spectrum_frames_per_pass(N);
            const float* tab = reinterpret_cast<const float*>(sp.dev.dev());
            hipLaunchKernelGGL(spectrum_kernel<IQT>, dim3(G, w.S), dim3(SPECTRUM_THREADS), spectrum_lds_bytes(N, F), st, src, pitch, tab,
                               reinterpret_cast<const float2*>(tab + N), sp.logn, sp.hop, first, J, F, sp.scratch.get());
            HIPCHK(c, hipGetLastError());
        }
        hipLaunchKernelGGL(chan_survey_sum_kernel, dim3((w.S * N + 255) / 256), dim3(256), 0, st, sp.scratch.get(), G, N, w.S, sp.plane[p].get());
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, sp.dev.after_read(st == c->stream ? RD_MAIN : RD_FRONT, st));
    HIPCHK(c, hipEventRecord(sp.ev[p], st));
    sp.frames[p] = J; sp.first_sample[p] = w.count + first; sp.valid[p] = true; sp.latest = p;
    return M17HIP_OK;
}
// What follows the tuner's or the channeliser's kernel on its stream `st`, for the next block: the channels' carries, the sources' histories (H converted
// samples each, into the copy whose turn it is), the feed's sample count.  In between the survey of a raster's block, which reads what that kernel read.
// The power scratch of a metered block, in front of the block's kernel: [C][T] floats.  Regrown behind everything that may still read the old one.
static int meter_scratch(m17hip_ctx* c, uint32_t C, uint32_t T)
{
    auto& mt = c->wide.mt;
    if (mt.scratch.size() >= (size_t)C * T) return M17HIP_OK;
    HIPCHK(c, hipEventSynchronize(c->ev_iq));   // (the block before may still be metered)
    return alloc_code(c, mt.scratch.grow((size_t)C * T, &c->last_hip));
}
// The meter of one block (m17hip_wide_meter is on), on the block's stream behind its kernel: it reads the power scratch and the rows of `x` that kernel
// wrote, and writes the plane whose turn it is.
static int launch_meter(m17hip_ctx* c, const float* x, uint32_t T, uint32_t C, hipStream_t st)
{
    auto& mt = c->wide.mt;
    uint32_t a0, K;
    core::meter_pieces(mt.outputs, T, mt.window, a0, K);
    const int p = mt.latest ^ 1;
    int r;
    if (!mt.fetch) HIPCHK(c, hipStreamCreateWithFlags(&mt.fetch, hipStreamNonBlocking));
    for (auto& e : mt.ev) if (!e) HIPCHK(c, e.create());
    mt.valid[p] = false;
    if (mt.plane[p].size() < (size_t)3 * C * K) {   // (this plane alone: the other one is the block before's, which keeps its words)
        HIPCHK(c, hipEventSynchronize(c->ev_iq));   // (its last writer, two blocks back, is in front of that)
        if ((r = alloc_code(c, mt.plane[p].grow((size_t)3 * C * K, &c->last_hip)))) return r;
    }
    {
        Timed tm(c, KT_METER, st);
        const uint32_t PP = meter_pieces_per_wg(mt.window);
        hipLaunchKernelGGL(wide_meter_kernel, dim3((K + PP - 1) / PP, C), dim3(METER_THREADS), 0, st, mt.scratch.get(), (size_t)T, x, c->xpitch, a0, T,
                           mt.window, K, C, mt.plane[p].get());
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(mt.ev[p], st));
    mt.C[p] = C; mt.K[p] = K; mt.T[p] = T; mt.N0[p] = mt.outputs; mt.win[p] = mt.window; mt.valid[p] = true; mt.latest = p;
    return M17HIP_OK;
}
// The levels of one squelched block, in front of its squelch kernels on its stream `st`: with m17hip_wide_squelch_floor on, squelch_floor_kernel makes them
// from the plane launch_spectrum has just queued (J frames) into floor plane `p`; otherwise the table of given levels is brought up to date.  `fresh` also
// starts the hold counts and the floor carry over here.  *levels is what the squelch kernel reads; squelch_levels_done follows that kernel.
static int squelch_levels(m17hip_ctx* c, int p, uint32_t J, hipStream_t st, const float** levels)
{
    auto& w = c->wide;
    auto& sq = w.sq;
    int r;
    if (sq.floor && !sq.fcarry) {   // ([256] and [4][256], once per configuration: never regrown)
        if ((r = alloc_code(c, sq.fcarry.alloc(256)))) return r;
        for (auto& b : sq.fplane) if ((r = alloc_code(c, b.alloc(4 * 256)))) return r;
        sq.fresh = true;
    }
    if (!sq.floor) {
        if (sq.dirty || !sq.dev.live()) {   // the levels, into the copy no queued launch reads
            uint32_t* staging = nullptr;
            HIPCHK(c, sq.dev.begin_write(2 * 256, &staging));
            std::memcpy(staging, sq.levels.data(), sq.levels.size() * 4);
            HIPCHK(c, sq.dev.publish(sq.levels.size(), st));
            sq.dirty = false;
        }
        HIPCHK(c, sq.dev.before_read(st));
    }
    // A fresh feed of decisions: every count of the array is 0, not only those of this block's channels — a later block may carry more channels than this
    // one — and every source's floor is forgotten.  On the block's stream, which iq_order has put behind whatever read or wrote the arrays last: nothing
    // is waited for.
    if (sq.fresh) {
        HIPCHK(c, hipMemsetAsync(sq.hold.get(), 0, (size_t)c->maxC * sizeof(uint32_t), st));
        if (sq.fcarry) HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(sq.fcarry.get()), (int)core::SQUELCH_FLOOR_NAN, 256, st));
    }
    sq.has_floor[p] = sq.floor;
    if (!sq.floor) { *levels = reinterpret_cast<const float*>(sq.dev.dev()); return M17HIP_OK; }
    {
        Timed tm(c, KT_SQUELCH_FLOOR, st);
        hipLaunchKernelGGL(squelch_floor_kernel, dim3(w.S), dim3(SQUELCH_FLOOR_THREADS), 0, st, w.sp.plane[w.sp.latest].get(), w.sp.logn, J, sq.B, sq.f_open,
                           sq.f_close, sq.f_rise, sq.f_fall, sq.f_min, sq.fcarry.get(), sq.fplane[p].get(), w.S);
        HIPCHK(c, hipGetLastError());
    }
    *levels = sq.fplane[p].get() + 2 * (size_t)w.S;
    return M17HIP_OK;
}
static int squelch_levels_done(m17hip_ctx* c, hipStream_t st)
{
    auto& sq = c->wide.sq;
    if (!sq.floor) HIPCHK(c, sq.dev.after_read(st == c->stream ? RD_MAIN : RD_FRONT, st));
    return M17HIP_OK;
}
// The carrier scan of one block (m17hip_wide_scan is on), on the block's stream between its floor kernel and its squelch kernel: it reads the plane
// launch_spectrum has just queued, the floor plane `p` squelch_levels has just queued, the host's channel table (launch_tune has put the stream behind its
// upload and records the read behind the tuner), the pool marks and the hold counts, and writes the scan's planes whose turn it is.  *table is what the
// block's squelch kernel and tuner read from here on.
static int launch_scan(m17hip_ctx* c, int p, uint32_t C, hipStream_t st, const uint32_t** table)
{
    auto& w = c->wide;
    auto& sq = w.sq;
    auto& sc = w.sc;
    const int ps = w.sp.latest;
    int r;
    for (auto& e : sc.ev) if (!e) HIPCHK(c, e.create());
    if (!sc.carry) {   // ([maxC], [2 maxC], [maxC] and [256], once per configuration: never regrown)
        if ((r = alloc_code(c, sc.carry.alloc(c->maxC)))) return r;
        for (auto& b : sc.plane) if ((r = alloc_code(c, b.alloc(2 * (size_t)c->maxC)))) return r;
        for (auto& b : sc.flags) if ((r = alloc_code(c, b.alloc(c->maxC)))) return r;
        for (auto& b : sc.missed) if ((r = alloc_code(c, b.alloc(256)))) return r;
        sq.fresh = true;
    }
    if (sc.dirty || !sc.dev.live()) {   // the pool marks, into the copy no queued launch reads
        uint32_t* staging = nullptr;
        HIPCHK(c, sc.dev.begin_write(c->maxC, &staging));
        std::memcpy(staging, sc.pool.data(), (size_t)c->maxC * 4);
        HIPCHK(c, sc.dev.publish(c->maxC, st));
        sc.dirty = false;
    }
    HIPCHK(c, sc.dev.before_read(st));
    sc.valid[p] = false;
    {
        Timed tm(c, KT_SCAN, st);
        hipLaunchKernelGGL(wide_scan_kernel, dim3(w.S), dim3(SCAN_THREADS), 0, st, w.sp.plane[ps].get(), w.sp.logn, w.sp.frames[ps], w.dev.dev(), c->maxC,
                           sc.dev.dev(), sq.fplane[p].get(), w.S, sq.B, sc.X, sq.hang, sq.hold.get(), sc.carry.get(), sq.fresh ? 1u : 0u, C, sc.plane[p].get(),
                           sc.flags[p].get(), sc.missed[p].get());
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, sc.dev.after_read(st == c->stream ? RD_MAIN : RD_FRONT, st));
    HIPCHK(c, hipEventRecord(sc.ev[p], st));
    sc.C[p] = C; sc.frames[p] = w.sp.frames[ps]; sc.valid[p] = true; sc.latest = p;
    *table = sc.plane[p].get();
    return M17HIP_OK;
}
// The squelch of one block (m17hip_wide_squelch is on), on the block's stream between its spectrum and its tuner: it reads the plane launch_spectrum has
// just queued, the channel table the tuner is about to read and the levels, steps the hold counts and writes the state and band planes whose turn it is.
// The state plane is what the block's tuner reads: its next writer, two blocks on, is behind that tuner through ev_iq.
static int launch_squelch(m17hip_ctx* c, uint32_t C, hipStream_t st)
{
    auto& w = c->wide;
    auto& sq = w.sq;
    const int p = sq.latest ^ 1, ps = w.sp.latest;
    int r;
    if (!sq.fetch) HIPCHK(c, hipStreamCreateWithFlags(&sq.fetch, hipStreamNonBlocking));
    for (auto& e : sq.ev) if (!e) HIPCHK(c, e.create());
    if (!sq.hold) {   // ([maxC] each, once per configuration: never regrown)
        if ((r = alloc_code(c, sq.hold.alloc(c->maxC)))) return r;
        for (auto& b : sq.state) if ((r = alloc_code(c, b.alloc(c->maxC)))) return r;
        for (auto& b : sq.band) if ((r = alloc_code(c, b.alloc(c->maxC)))) return r;
        sq.fresh = true;
    }
    sq.valid[p] = false;
    const float* levels = nullptr;
    if ((r = squelch_levels(c, p, w.sp.frames[ps], st, &levels))) return r;
    const uint32_t* table = w.dev.dev();
    if (w.scanning()) if ((r = launch_scan(c, p, C, st, &table))) return r;   // (m17hip_wide_scan: the block's table is the scan's from here on)
    {
        Timed tm(c, KT_SQUELCH, st);
        hipLaunchKernelGGL(wide_squelch_kernel, dim3((C + SQUELCH_THREADS - 1) / SQUELCH_THREADS), dim3(SQUELCH_THREADS), 0, st, w.sp.plane[ps].get(), w.sp.logn,
                           w.sp.frames[ps], table, c->maxC, levels, w.S, sq.B, sq.hang, sq.hold.get(), sq.state[p].get(), sq.band[p].get(), C);
        HIPCHK(c, hipGetLastError());
    }
    if ((r = squelch_levels_done(c, st))) return r;
    HIPCHK(c, hipEventRecord(sq.ev[p], st));
    sq.fresh = false;
    sq.C[p] = C; sq.frames[p] = w.sp.frames[ps]; sq.valid[p] = true; sq.latest = p;
    return M17HIP_OK;
}
// The time-resolved squelch of one block (m17hip_wide_squelch_slots is on), in launch_squelch's place: it reads the group sums spectrum_kernel has just left
// in the spectrum's scratch — the next writer of that scratch is the next block's spectrum_kernel, behind this stream through ev_iq, and a regrowth waits
// for ev_iq first —, the channel table and the levels, steps the hold counts through the block's slots and writes the band plane, the state plane and the
// tile mask whose turn it is.  TO: the outputs of a tile of the tuner that follows; tiles: their number.
static int launch_squelch_slots(m17hip_ctx* c, uint32_t C, uint32_t T, uint32_t W, uint32_t TO, uint32_t tiles, hipStream_t st)
{
    auto& w = c->wide;
    auto& sq = w.sq;
    const int p = sq.latest ^ 1;
    uint32_t first, J;
    core::spec_frames(w.count, W, w.sp.points, w.sp.hop, first, J);   // (what launch_spectrum has just transformed)
    const uint32_t G = core::squelch_slots(J), SW = squelch_slot_words(G), MW = squelch_tile_words(tiles);
    int r;
    if (!sq.fetch) HIPCHK(c, hipStreamCreateWithFlags(&sq.fetch, hipStreamNonBlocking));
    for (auto& e : sq.ev) if (!e) HIPCHK(c, e.create());
    if (!sq.hold) {   // ([maxC] each, once per configuration: never regrown)
        if ((r = alloc_code(c, sq.hold.alloc(c->maxC)))) return r;
        for (auto& b : sq.state) if ((r = alloc_code(c, b.alloc(c->maxC)))) return r;
        for (auto& b : sq.band) if ((r = alloc_code(c, b.alloc(c->maxC)))) return r;
        sq.fresh = true;
    }
    sq.valid[p] = false;
    if (sq.sbits.size() < (size_t)C * SW || sq.sband[p].size() < (size_t)C * G || sq.mask[p].size() < (size_t)C * MW) {   // (the block's shape has grown)
        HIPCHK(c, hipEventSynchronize(c->ev_iq));   // (the last reader of these — the tuner two blocks back, the tile kernel of the block before — is in front of that)
        if ((r = alloc_code(c, sq.sbits.grow((size_t)C * SW, &c->last_hip)))) return r;
        if ((r = alloc_code(c, sq.sband[p].grow((size_t)C * G, &c->last_hip)))) return r;
        if ((r = alloc_code(c, sq.mask[p].grow((size_t)C * MW, &c->last_hip)))) return r;
    }
    const float* levels = nullptr;
    if ((r = squelch_levels(c, p, J, st, &levels))) return r;   // (as launch_squelch does)
    {
        Timed tm(c, KT_SQUELCH_SLOTS, st);
        if (G) {
            hipLaunchKernelGGL(squelch_slots_band_kernel, dim3((uint32_t)(((uint64_t)C * G + SQUELCH_THREADS - 1) / SQUELCH_THREADS)), dim3(SQUELCH_THREADS), 0, st,
                               w.sp.scratch.get(), w.sp.logn, G, w.dev.dev(), c->maxC, sq.B, sq.sband[p].get(), C);
            HIPCHK(c, hipGetLastError());
        }
        hipLaunchKernelGGL(squelch_slots_step_kernel, dim3((C + SQUELCH_THREADS - 1) / SQUELCH_THREADS), dim3(SQUELCH_THREADS), 0, st, sq.sband[p].get(), G, J,
                           w.dev.dev(), levels, w.S, sq.hang, sq.hold.get(), sq.state[p].get(), sq.sbits.get(), C);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(squelch_slots_tile_kernel, dim3((uint32_t)(((uint64_t)C * MW + SQUELCH_THREADS - 1) / SQUELCH_THREADS)), dim3(SQUELCH_THREADS), 0, st,
                           sq.sbits.get(), G, first, w.sp.hop, sq.lead, TO, T, W, tiles, MW, sq.mask[p].get(), C);
        HIPCHK(c, hipGetLastError());
    }
    if ((r = squelch_levels_done(c, st))) return r;
    HIPCHK(c, hipEventRecord(sq.ev[p], st));
    sq.fresh = false;
    sq.C[p] = C; sq.frames[p] = J; sq.G[p] = G; sq.tiles[p] = tiles; sq.valid[p] = true; sq.latest = p;
    return M17HIP_OK;
}
template <typename IQT>
static int wide_after_block(m17hip_ctx* c, const IQT* src, size_t pitch, uint32_t W, uint32_t T, uint32_t H, uint32_t C, const float* x, hipStream_t st)
{
    auto& w = c->wide;
    hipLaunchKernelGGL(wide_carry_kernel, dim3((C + 63) / 64), dim3(64), 0, st, w.znew.get(), c->iq_carry.get(), C);
    HIPCHK(c, hipGetLastError());
    if (w.mt.window) if (int r = launch_meter(c, x, T, C, st)) return r;   // (m17hip_wide_meter: under every configuration)
    w.mt.outputs += T;
    if (w.sv.stride) if (int r = launch_survey<IQT>(c, src, pitch, W, T, st)) return r;   // (m17hip_wide_survey: on under a raster only)
    if (w.sp.points && !w.sq.on) if (int r = launch_spectrum<IQT>(c, src, pitch, W, st)) return r;   // (m17hip_wide_spectrum: under every configuration; a squelched block's went in front of its tuner)
    if (H) {
        hipLaunchKernelGGL(wide_hist_kernel<IQT>, dim3((H + 63) / 64, w.S), dim3(64), 0, st, src, pitch, W, w.hist[w.par].get(), w.hist[w.par ^ 1].get(), H);
        HIPCHK(c, hipGetLastError());
    }
    w.par ^= 1;
    w.count += W;
    return iq_mark(c, st);
}
template <typename IQT>
static int launch_tune(m17hip_ctx* c, const void* dev, size_t pitch, float* x, uint32_t C, uint32_t T, float gain, hipStream_t st)
{
    auto& w = c->wide;
    const IQT* src = static_cast<const IQT*>(dev);
    const uint32_t W = (uint32_t)w.row(T), H = w.hlen();   // (W fits: upload_wide has seen to it)
    if (w.dirty || !w.dev.live()) {   // the channel table, into the copy no queued launch reads
        uint32_t* staging = nullptr;
        HIPCHK(c, w.dev.begin_write(w.table.size(), &staging));
        std::memcpy(staging, w.table.data(), w.table.size() * 4);
        HIPCHK(c, w.dev.publish(w.table.size(), st));
        w.dirty = false;
    }
    HIPCHK(c, w.dev.before_read(st));
    const bool meter = w.mt.window != 0;   // (the metered instantiations: one more argument and one more store per output, otherwise the same launch)
    if (meter) if (int r = meter_scratch(c, C, T)) return r;
    const MeterOut mo{w.mt.scratch.get(), (size_t)T};
    // The squelched instantiations (m17hip_wide_squelch): the block's spectrum and the squelch kernel go IN FRONT of the tuner on its stream, and the tuner's
    // last argument is the state plane that kernel has written.  With the squelch off nothing moves: the spectrum follows in wide_after_block.
    // The tile-squelched instantiations (m17hip_wide_squelch_slots) take the block's tile mask in the state plane's place; everything else is the same.
    const bool slots = w.sq.on && w.sq.slots, squelch = w.sq.on && !slots;
    const uint32_t RG = w.U ? resample_groups(w.L, w.R, w.L2, w.U, w.D) : 0;
    const uint32_t tiles = w.U ? (T / w.U + RG - 1) / RG : (T + WIDE_TILE - 1) / WIDE_TILE;
    if (squelch || slots) {
        if (int r = launch_spectrum<IQT>(c, src, pitch, W, st)) return r;
        if (int r = slots ? launch_squelch_slots(c, C, T, W, w.U ? RG * w.U : (uint32_t)WIDE_TILE, tiles, st) : launch_squelch(c, C, st)) return r;
    }
    // the table the tuner reads: the host's, or — m17hip_wide_scan — the one the block's scan kernel has just written (launch_squelch)
    const uint32_t* table = squelch && w.scanning() ? w.sc.plane[w.sc.latest].get() : w.dev.dev();
    const SquelchIn qi{squelch ? w.sq.state[w.sq.latest].get() : nullptr};
    const SquelchTilesIn ti{slots ? w.sq.mask[w.sq.latest].get() : nullptr, squelch_tile_words(tiles)};
    if (w.U) {
        const uint32_t G = RG, Q = resample_q(w.L, w.R, w.L2, w.U, w.D, G);
        TimedK tm(c, KT_RESAMPLE);
        if (slots && meter)
            tm.launch(resample_kernel<IQT, true, true, MeterOut, SquelchTilesIn>, dim3((T / w.U + G - 1) / G, C), dim3(WIDE_THREADS),
                      resample_lds_bytes(w.L, w.R, w.L2, w.U, w.D, G, Q), st, src, pitch, W, w.hist[w.par].get(), w.taps.get(), w.L, w.R, w.taps2.get(), w.L2, w.U,
                      w.D, G, Q, table, c->maxC, (uint32_t)w.count, x, c->xpitch, T, c->iq_carry.get(), w.znew.get(), gain, mo, ti);
        else if (slots)
            tm.launch(resample_kernel<IQT, false, true, SquelchTilesIn>, dim3((T / w.U + G - 1) / G, C), dim3(WIDE_THREADS),
                      resample_lds_bytes(w.L, w.R, w.L2, w.U, w.D, G, Q), st, src, pitch, W, w.hist[w.par].get(), w.taps.get(), w.L, w.R, w.taps2.get(), w.L2, w.U,
                      w.D, G, Q, table, c->maxC, (uint32_t)w.count, x, c->xpitch, T, c->iq_carry.get(), w.znew.get(), gain, ti);
        else if (squelch && meter)
            tm.launch(resample_kernel<IQT, true, true, MeterOut, SquelchIn>, dim3((T / w.U + G - 1) / G, C), dim3(WIDE_THREADS),
                      resample_lds_bytes(w.L, w.R, w.L2, w.U, w.D, G, Q), st, src, pitch, W, w.hist[w.par].get(), w.taps.get(), w.L, w.R, w.taps2.get(), w.L2, w.U,
                      w.D, G, Q, table, c->maxC, (uint32_t)w.count, x, c->xpitch, T, c->iq_carry.get(), w.znew.get(), gain, mo, qi);
        else if (squelch)
            tm.launch(resample_kernel<IQT, false, true, SquelchIn>, dim3((T / w.U + G - 1) / G, C), dim3(WIDE_THREADS),
                      resample_lds_bytes(w.L, w.R, w.L2, w.U, w.D, G, Q), st, src, pitch, W, w.hist[w.par].get(), w.taps.get(), w.L, w.R, w.taps2.get(), w.L2, w.U,
                      w.D, G, Q, table, c->maxC, (uint32_t)w.count, x, c->xpitch, T, c->iq_carry.get(), w.znew.get(), gain, qi);
        else if (meter)
            tm.launch(resample_kernel<IQT, true, false, MeterOut>, dim3((T / w.U + G - 1) / G, C), dim3(WIDE_THREADS), resample_lds_bytes(w.L, w.R, w.L2, w.U, w.D, G, Q), st,
                      src, pitch, W, w.hist[w.par].get(), w.taps.get(), w.L, w.R, w.taps2.get(), w.L2, w.U, w.D, G, Q, table, c->maxC, (uint32_t)w.count,
                      x, c->xpitch, T, c->iq_carry.get(), w.znew.get(), gain, mo);
        else
        tm.launch(resample_kernel<IQT>, dim3((T / w.U + G - 1) / G, C), dim3(WIDE_THREADS), resample_lds_bytes(w.L, w.R, w.L2, w.U, w.D, G, Q), st, src, pitch,
                  W, w.hist[w.par].get(), w.taps.get(), w.L, w.R, w.taps2.get(), w.L2, w.U, w.D, G, Q, table, c->maxC, (uint32_t)w.count, x,
                  c->xpitch, T, c->iq_carry.get(), w.znew.get(), gain);
    } else if (w.R2) {
        TimedK tm(c, KT_WIDE2);
        if (slots && meter)
            tm.launch(tune2_kernel<IQT, true, true, MeterOut, SquelchTilesIn>, dim3((T + WIDE_TILE - 1) / WIDE_TILE, C), dim3(WIDE_THREADS),
                      wide2_lds_bytes(w.L, w.R, w.L2, w.R2), st, src, pitch, W, w.hist[w.par].get(), w.taps.get(), w.L, w.R, w.taps2.get(), w.L2, w.R2,
                      wide2_q(w.L, w.R, w.L2, w.R2), table, c->maxC, (uint32_t)w.count, x, c->xpitch, T, c->iq_carry.get(), w.znew.get(), gain, mo, ti);
        else if (slots)
            tm.launch(tune2_kernel<IQT, false, true, SquelchTilesIn>, dim3((T + WIDE_TILE - 1) / WIDE_TILE, C), dim3(WIDE_THREADS),
                      wide2_lds_bytes(w.L, w.R, w.L2, w.R2), st, src, pitch, W, w.hist[w.par].get(), w.taps.get(), w.L, w.R, w.taps2.get(), w.L2, w.R2,
                      wide2_q(w.L, w.R, w.L2, w.R2), table, c->maxC, (uint32_t)w.count, x, c->xpitch, T, c->iq_carry.get(), w.znew.get(), gain, ti);
        else if (squelch && meter)
            tm.launch(tune2_kernel<IQT, true, true, MeterOut, SquelchIn>, dim3((T + WIDE_TILE - 1) / WIDE_TILE, C), dim3(WIDE_THREADS),
                      wide2_lds_bytes(w.L, w.R, w.L2, w.R2), st, src, pitch, W, w.hist[w.par].get(), w.taps.get(), w.L, w.R, w.taps2.get(), w.L2, w.R2,
                      wide2_q(w.L, w.R, w.L2, w.R2), table, c->maxC, (uint32_t)w.count, x, c->xpitch, T, c->iq_carry.get(), w.znew.get(), gain, mo, qi);
        else if (squelch)
            tm.launch(tune2_kernel<IQT, false, true, SquelchIn>, dim3((T + WIDE_TILE - 1) / WIDE_TILE, C), dim3(WIDE_THREADS),
                      wide2_lds_bytes(w.L, w.R, w.L2, w.R2), st, src, pitch, W, w.hist[w.par].get(), w.taps.get(), w.L, w.R, w.taps2.get(), w.L2, w.R2,
                      wide2_q(w.L, w.R, w.L2, w.R2), table, c->maxC, (uint32_t)w.count, x, c->xpitch, T, c->iq_carry.get(), w.znew.get(), gain, qi);
        else if (meter)
            tm.launch(tune2_kernel<IQT, true, false, MeterOut>, dim3((T + WIDE_TILE - 1) / WIDE_TILE, C), dim3(WIDE_THREADS), wide2_lds_bytes(w.L, w.R, w.L2, w.R2), st, src,
                      pitch, W, w.hist[w.par].get(), w.taps.get(), w.L, w.R, w.taps2.get(), w.L2, w.R2, wide2_q(w.L, w.R, w.L2, w.R2), table, c->maxC,
                      (uint32_t)w.count, x, c->xpitch, T, c->iq_carry.get(), w.znew.get(), gain, mo);
        else
        tm.launch(tune2_kernel<IQT>, dim3((T + WIDE_TILE - 1) / WIDE_TILE, C), dim3(WIDE_THREADS), wide2_lds_bytes(w.L, w.R, w.L2, w.R2), st, src, pitch, W,
                  w.hist[w.par].get(), w.taps.get(), w.L, w.R, w.taps2.get(), w.L2, w.R2, wide2_q(w.L, w.R, w.L2, w.R2), table, c->maxC,
                  (uint32_t)w.count, x, c->xpitch, T, c->iq_carry.get(), w.znew.get(), gain);
    } else {
        TimedK tm(c, KT_WIDE);
        if (slots && meter)
            tm.launch(tune_kernel<IQT, true, true, MeterOut, SquelchTilesIn>, dim3((T + WIDE_TILE - 1) / WIDE_TILE, C), dim3(WIDE_THREADS), wide_lds_bytes(w.L, w.R), st,
                      src, pitch, W, w.hist[w.par].get(), w.taps.get(), w.L, w.R, table, c->maxC, (uint32_t)w.count, x, c->xpitch, T, c->iq_carry.get(),
                      w.znew.get(), gain, mo, ti);
        else if (slots)
            tm.launch(tune_kernel<IQT, false, true, SquelchTilesIn>, dim3((T + WIDE_TILE - 1) / WIDE_TILE, C), dim3(WIDE_THREADS), wide_lds_bytes(w.L, w.R), st, src,
                      pitch, W, w.hist[w.par].get(), w.taps.get(), w.L, w.R, table, c->maxC, (uint32_t)w.count, x, c->xpitch, T, c->iq_carry.get(),
                      w.znew.get(), gain, ti);
        else if (squelch && meter)
            tm.launch(tune_kernel<IQT, true, true, MeterOut, SquelchIn>, dim3((T + WIDE_TILE - 1) / WIDE_TILE, C), dim3(WIDE_THREADS), wide_lds_bytes(w.L, w.R), st,
                      src, pitch, W, w.hist[w.par].get(), w.taps.get(), w.L, w.R, table, c->maxC, (uint32_t)w.count, x, c->xpitch, T, c->iq_carry.get(),
                      w.znew.get(), gain, mo, qi);
        else if (squelch)
            tm.launch(tune_kernel<IQT, false, true, SquelchIn>, dim3((T + WIDE_TILE - 1) / WIDE_TILE, C), dim3(WIDE_THREADS), wide_lds_bytes(w.L, w.R), st, src,
                      pitch, W, w.hist[w.par].get(), w.taps.get(), w.L, w.R, table, c->maxC, (uint32_t)w.count, x, c->xpitch, T, c->iq_carry.get(),
                      w.znew.get(), gain, qi);
        else if (meter)
            tm.launch(tune_kernel<IQT, true, false, MeterOut>, dim3((T + WIDE_TILE - 1) / WIDE_TILE, C), dim3(WIDE_THREADS), wide_lds_bytes(w.L, w.R), st, src, pitch, W,
                      w.hist[w.par].get(), w.taps.get(), w.L, w.R, table, c->maxC, (uint32_t)w.count, x, c->xpitch, T, c->iq_carry.get(), w.znew.get(),
                      gain, mo);
        else
        tm.launch(tune_kernel<IQT>, dim3((T + WIDE_TILE - 1) / WIDE_TILE, C), dim3(WIDE_THREADS), wide_lds_bytes(w.L, w.R), st, src, pitch, W, w.hist[w.par].get(),
                  w.taps.get(), w.L, w.R, table, c->maxC, (uint32_t)w.count, x, c->xpitch, T, c->iq_carry.get(), w.znew.get(), gain);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, w.dev.after_read(st == c->stream ? RD_MAIN : RD_FRONT, st));   // (two readers: the main stream and the copy stream)
    return wide_after_block(c, src, pitch, W, T, H, C, x, st);
}
// The channeliser's launch (m17hip_wide_raster): the same frame, one workgroup per source and tile of output times.
template <typename IQT>
static int launch_chan(m17hip_ctx* c, const void* dev, size_t pitch, float* x, uint32_t C, uint32_t T, float gain, hipStream_t st)
{
    auto& w = c->wide;
    const IQT* src = static_cast<const IQT*>(dev);
    const uint32_t W = T * w.R, H = w.L - 1;   // (W fits: upload_wide has seen to it)
    if (w.dirty || !w.rdev.live() || w.rdev_C != C) {   // the channel table by source, into the copy no queued launch reads
        uint32_t* t = nullptr;
        HIPCHK(c, w.rdev.begin_write(chan_table_words(256, c->maxC), &t));
        const uint32_t S = w.S, maxC = c->maxC;
        uint32_t* first = t;                 // [S + 1]
        uint32_t* ufirst = t + S + 1;        // [S + 1]
        uint32_t* pairs = t + 2 * (S + 1);   // [C][2]
        uint32_t* ubins = pairs + 2 * (size_t)C;
        std::fill(t, t + 2 * (S + 1), 0u);
        for (uint32_t ch = 0; ch < C; ++ch) ++first[w.table[ch] + 1];
        for (uint32_t s = 0; s < S; ++s) first[s + 1] += first[s];
        std::vector<uint32_t> at(first, first + S);
        for (uint32_t ch = 0; ch < C; ++ch) { uint32_t& a = at[w.table[ch]]; pairs[2 * a] = w.table[maxC + ch]; pairs[2 * a + 1] = ch; ++a; }
        std::vector<uint8_t> seen(w.M);
        uint32_t U = 0;
        for (uint32_t s = 0; s < S; ++s) {
            std::fill(seen.begin(), seen.end(), 0);
            ufirst[s] = U;
            for (uint32_t a = first[s]; a < first[s + 1]; ++a) if (!seen[pairs[2 * a]]) { seen[pairs[2 * a]] = 1; ubins[U++] = pairs[2 * a]; }
        }
        ufirst[S] = U;
        HIPCHK(c, w.rdev.publish(chan_table_words(S, C), st));
        w.dirty = false; w.rdev_C = C;
    }
    HIPCHK(c, w.rdev.before_read(st));
    const bool meter = w.mt.window != 0;
    if (meter) if (int r = meter_scratch(c, C, T)) return r;
    {
        const uint32_t TT = chan_tile(w.L, w.R, w.M);
        TimedK tm(c, KT_CHAN);
        if (meter)
            tm.launch(chan_kernel<IQT, true, MeterOut>, dim3((T + TT - 1) / TT, w.S), dim3(CHAN_THREADS), chan_lds_bytes(w.L, w.R, w.M, TT), st, src, pitch, W,
                      w.hist[w.par].get(), w.taps.get(), w.L, w.R, w.M1, w.M2, w.tw.get(), w.rdev.dev(), w.S, (uint32_t)(w.count % w.M), TT, C, x, c->xpitch, T,
                      c->iq_carry.get(), w.znew.get(), gain, MeterOut{w.mt.scratch.get(), (size_t)T});
        else
        tm.launch(chan_kernel<IQT>, dim3((T + TT - 1) / TT, w.S), dim3(CHAN_THREADS), chan_lds_bytes(w.L, w.R, w.M, TT), st, src, pitch, W, w.hist[w.par].get(),
                  w.taps.get(), w.L, w.R, w.M1, w.M2, w.tw.get(), w.rdev.dev(), w.S, (uint32_t)(w.count % w.M), TT, C, x, c->xpitch, T, c->iq_carry.get(),
                  w.znew.get(), gain);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, w.rdev.after_read(st == c->stream ? RD_MAIN : RD_FRONT, st));
    return wide_after_block(c, src, pitch, W, T, H, C, x, st);
}
// The four ways in, as upload_iq has them: the tuner or the channeliser takes the place of the copy.  `p`: [sources][pitch] samples of the configured format.
static int upload_wide(m17hip_ctx* c, const void* p, float gain, uint32_t C, uint32_t T, size_t pitch, int how)
{
    uint64_t W = 0;
    const auto own = [&] {
        if (!std::isfinite(gain) || !(gain > 0.0f)) return M17HIP_EINVAL;
        if (!c->wide.S) return M17HIP_ESTATE;   // (m17hip_wide_config first)
        if (c->wide.U && T % c->wide.U) return M17HIP_EINVAL;   // (a block holds whole groups of `up` outputs: the phase never depends on the feed's history)
        W = c->wide.row(T);
        if (c->wide.scanning()) {   // (m17hip_wide_scan: at most 256 slots a source among the block's channels, by the table in force)
            uint32_t slots[256] = {0};
            for (uint32_t ch = 0; ch < C && ch < c->maxC; ++ch)
                if (c->wide.sc.pool[ch] && ++slots[c->wide.table[ch]] > core::SCAN_MAX_SLOTS) return M17HIP_ESTATE;
        }
        return pitch < W || W > 0xFFFFFFFFull ? M17HIP_EINVAL : M17HIP_OK;   // (the kernels count a row's samples in 32 bits)
    };
    return upload_frame<float>(c, p, C, T, (how & IQ_STAGED) != 0, own, [&](float* x, hipStream_t st) -> int {
        auto& w = c->wide;
        int r;
        if ((r = iq_order(c, st))) return r;
        const void* dev = p;
        if ((how & IQ_FROM_HOST) && (r = stage_raw(c, w.S, W, iq_sample_bytes(w.fmt), st, dev, pitch))) return r;
        return with_iq_type(w.fmt, [&](auto s) {
            return w.M ? launch_chan<decltype(s)>(c, dev, pitch, x, C, T, gain, st) : launch_tune<decltype(s)>(c, dev, pitch, x, C, T, gain, st);
        });
    });
}

}  // extern "C++"

int m17hip_upload_i16(m17hip_ctx* c, const int16_t* host, uint32_t C, uint32_t T, size_t pitch) { return upload_host(c, host, C, T, pitch, false); }
int m17hip_upload_f32(m17hip_ctx* c, const float* host, uint32_t C, uint32_t T, size_t pitch) { return upload_host(c, host, C, T, pitch, false); }
int m17hip_upload_i16_async(m17hip_ctx* c, const int16_t* host, uint32_t C, uint32_t T, size_t pitch) { return upload_host(c, host, C, T, pitch, true); }
int m17hip_upload_f32_async(m17hip_ctx* c, const float* host, uint32_t C, uint32_t T, size_t pitch) { return upload_host(c, host, C, T, pitch, true); }
int m17hip_upload_i16_device_async(m17hip_ctx* c, const int16_t* dev, uint32_t C, uint32_t T, size_t pitch) { return upload_dev(c, dev, C, T, pitch, true); }
int m17hip_upload_f32_device_async(m17hip_ctx* c, const float* dev, uint32_t C, uint32_t T, size_t pitch) { return upload_dev(c, dev, C, T, pitch, true); }
int m17hip_upload_i16_device(m17hip_ctx* c, const int16_t* dev, uint32_t C, uint32_t T, size_t pitch) { return upload_dev(c, dev, C, T, pitch, false); }
int m17hip_upload_f32_device(m17hip_ctx* c, const float* dev, uint32_t C, uint32_t T, size_t pitch) { return upload_dev(c, dev, C, T, pitch, false); }
int m17hip_download_i16(m17hip_ctx* c, int16_t* host, uint32_t C, uint32_t T, size_t pitch) { return download_host(c, host, C, T, pitch); }
int m17hip_download_f32(m17hip_ctx* c, float* host, uint32_t C, uint32_t T, size_t pitch) { return download_host(c, host, C, T, pitch); }

int m17hip_upload_iq(m17hip_ctx* c, const void* host, int iq_format, float gain, uint32_t C, uint32_t T, size_t pitch)
{
    return upload_iq(c, host, iq_format, gain, C, T, pitch, IQ_FROM_HOST);
}
int m17hip_upload_iq_device(m17hip_ctx* c, const void* dev, int iq_format, float gain, uint32_t C, uint32_t T, size_t pitch)
{
    return upload_iq(c, dev, iq_format, gain, C, T, pitch, 0);
}
int m17hip_upload_iq_async(m17hip_ctx* c, const void* host, int iq_format, float gain, uint32_t C, uint32_t T, size_t pitch)
{
    return upload_iq(c, host, iq_format, gain, C, T, pitch, IQ_FROM_HOST | IQ_STAGED);
}
int m17hip_upload_iq_device_async(m17hip_ctx* c, const void* dev, int iq_format, float gain, uint32_t C, uint32_t T, size_t pitch)
{
    return upload_iq(c, dev, iq_format, gain, C, T, pitch, IQ_STAGED);
}
int m17hip_iq_bytes(m17hip_ctx* c, uint64_t* bytes)
{
    if (!c || !bytes) return M17HIP_EINVAL;
    *bytes = c->iq_carry.size() * sizeof(float2) + c->iq_raw.size() + c->wide.bytes() + c->wtx.bytes();
    return M17HIP_OK;
}

int m17hip_wide_default_taps(uint32_t decim, float* taps, uint32_t capacity, uint32_t* ntaps)
{
    if (decim < 1 || decim > 16 || !ntaps) return M17HIP_EINVAL;
    *ntaps = 32 * decim + 1;
    if (!taps || capacity < *ntaps) return M17HIP_EINVAL;
    wide_default(decim, taps);
    return M17HIP_OK;
}
// the caller's taps of one stage checked and copied, or the default ones where there are none: false is M17HIP_EINVAL
static bool wide_stage_taps(const float* taps, uint32_t ntaps, uint32_t limit, std::vector<float>& h)
{
    if (!taps && ntaps == 0) return true;   // (h holds the default taps)
    if (!taps || ntaps < 1 || ntaps > limit) return false;
    for (uint32_t i = 0; i < ntaps; ++i) if (!std::isfinite(taps[i])) return false;
    h.assign(taps, taps + ntaps);
    return true;
}
// the channeliser's twiddles, tw[j] = exp(-2 pi j j / M) as (re, im): cos and sin in double for j <= M / 2, rounded to float, exactly 0 / +-1 where 4 j is a
// multiple of M; the upper half is the lower one's conjugate to the bit
static void chan_twiddles(uint32_t M, float* tw)
{
    const double pi = 3.14159265358979323846;
    for (uint32_t j = 0; j <= M / 2; ++j) {
        float re, im;
        if (4 * j % M == 0) { const uint32_t q = 4 * j / M; re = q == 0 ? 1.0f : q == 2 ? -1.0f : 0.0f; im = q == 1 ? 1.0f : 0.0f; }
        else { re = (float)std::cos(2.0 * pi * j / M); im = (float)std::sin(2.0 * pi * j / M); }
        tw[2 * j] = re; tw[2 * j + 1] = -im;
        if (j) { tw[2 * (M - j)] = re; tw[2 * (M - j) + 1] = im; }
    }
    if (M % 2 == 0) tw[M + 1] = 0.0f;   // (j = M / 2: -1, and its own conjugate)
}
// What the four configurations share, the arguments checked: h2 empty and decim2 == 0 is a single stage; bins != 0 the raster (a single stage, no oscillator);
// up != 0 the resampling tuner (h2 its second stage at up / down, decim2 == 0).
static int wide_setup(m17hip_ctx* c, uint32_t sources, int iq_format, uint32_t decim, const std::vector<float>& h, uint32_t decim2, const std::vector<float>& h2,
                      uint32_t bins = 0, uint32_t up = 0, uint32_t down = 0)
{
    GUARD(c);
    if (c->front_queued) return M17HIP_ESTATE;
    auto& w = c->wide;
    const hipStream_t st = c->iq_last ? c->iq_last : c->stream;
    int r;
    if ((r = ensure_iq(c, st))) return r;
    HIPCHK(c, hipEventSynchronize(c->ev_iq));   // (a block tuned with the configuration before may still be in flight: its buffers go)
    const uint32_t L = (uint32_t)h.size(), L2 = (uint32_t)h2.size();
    const size_t hn = (size_t)sources * std::max<uint32_t>(up ? (wide2_j(L2, up) - 1) * decim + L - 1 : decim2 ? (L2 - 1) * decim + L - 1 : L - 1, 1);
    w.S = 0;   // (not configured until all of it is there)
    w.sv.stride = 0; w.sv.forget();   // (the survey's plane has the configuration's shape: off, and its memory back)
    w.sv.scratch.release(&c->last_hip);
    for (auto& b : w.sv.plane) b.release(&c->last_hip);
    w.sp.points = 0; w.sp.forget();   // (the spectrum likewise: its plane has a row per source)
    w.sp.scratch.release(&c->last_hip);
    for (auto& b : w.sp.plane) b.release(&c->last_hip);
    w.sq.on = false; w.sq.forget();   // (the squelch goes with the spectrum)
    w.sq.hold.release(&c->last_hip);
    w.sq.fcarry.release(&c->last_hip);
    for (auto& b : w.sq.fplane) b.release(&c->last_hip);
    w.sc.on = false; w.sc.forget();   // (the scan goes with the squelch)
    w.sc.carry.release(&c->last_hip);
    for (auto& b : w.sc.plane) b.release(&c->last_hip);
    for (auto& b : w.sc.flags) b.release(&c->last_hip);
    for (auto& b : w.sc.missed) b.release(&c->last_hip);
    for (auto& b : w.sq.state) b.release(&c->last_hip);
    for (auto& b : w.sq.band) b.release(&c->last_hip);
    w.sq.sbits.release(&c->last_hip);
    for (auto& b : w.sq.mask) b.release(&c->last_hip);
    for (auto& b : w.sq.sband) b.release(&c->last_hip);
    w.mt.window = 0; w.mt.forget(); w.mt.outputs = 0;   // (the meter likewise: a new feed)
    w.mt.scratch.release(&c->last_hip);
    for (auto& b : w.mt.plane) b.release(&c->last_hip);
    if ((r = alloc_code(c, w.taps.alloc(L)))) return r;
    if (L2) { if ((r = alloc_code(c, w.taps2.alloc(L2)))) return r; }
    else w.taps2.release(&c->last_hip);
    for (auto& b : w.hist) if ((r = alloc_code(c, b.alloc(hn)))) return r;
    if (!w.znew && (r = alloc_code(c, w.znew.alloc(c->maxC)))) return r;
    HIPCHK(c, hipMemcpy(w.taps, h.data(), L * sizeof(float), hipMemcpyHostToDevice));
    if (L2) HIPCHK(c, hipMemcpy(w.taps2, h2.data(), L2 * sizeof(float), hipMemcpyHostToDevice));
    if (bins) {
        std::vector<float> tw(2 * (size_t)bins);
        chan_twiddles(bins, tw.data());
        if ((r = alloc_code(c, w.tw.alloc(bins)))) return r;
        HIPCHK(c, hipMemcpy(w.tw, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice));
    } else w.tw.release(&c->last_hip);
    for (auto& b : w.hist) HIPCHK(c, hipMemsetAsync(b, 0, hn * sizeof(float2), st));
    if ((r = iq_mark(c, st))) return r;
    if (w.table.empty() || w.M != bins) w.table.assign(2 * (size_t)c->maxC, 0u);   // (a frequency word is no bin, nor a bin of M one of another M: all fresh)
    for (uint32_t ch = 0; ch < c->maxC; ++ch)   // (a channel on a source that is no longer there goes back to the fresh entry)
        if (w.table[ch] >= sources) { w.table[ch] = 0; w.table[c->maxC + ch] = 0; }
    w.dirty = true;
    w.R = decim; w.L = L; w.R2 = decim2; w.L2 = L2; w.fmt = iq_format; w.par = 0; w.count = 0;
    w.M = bins; w.M1 = w.M2 = 0;
    w.U = up; w.D = down;
    if (bins) core::chan_factor(bins, w.M1, w.M2);
    w.S = sources;
    return M17HIP_OK;
}
int m17hip_wide_config(m17hip_ctx* c, uint32_t sources, uint32_t decim, int iq_format, const float* taps, uint32_t ntaps)
{
    if (!c || sources < 1 || sources > 256 || decim < 1 || decim > 16) return M17HIP_EINVAL;
    if (iq_format != M17HIP_IQ_I16 && iq_format != M17HIP_IQ_F32 && iq_format != M17HIP_IQ_U8) return M17HIP_EINVAL;
    std::vector<float> h(32 * decim + 1);
    wide_default(decim, h.data());
    if (!wide_stage_taps(taps, ntaps, 1024, h)) return M17HIP_EINVAL;
    return wide_setup(c, sources, iq_format, decim, h, 0, std::vector<float>());
}
int m17hip_wide_default_taps2(uint32_t decim1, uint32_t decim2, float* taps1, uint32_t cap1, uint32_t* ntaps1, float* taps2, uint32_t cap2, uint32_t* ntaps2)
{
    if (decim1 < 1 || decim1 > 16 || decim2 < 1 || decim2 > 16 || !ntaps1 || !ntaps2) return M17HIP_EINVAL;
    *ntaps1 = decim1 == 1 ? 1 : 8 * decim1 + 1;
    *ntaps2 = 32 * decim2 + 1;
    if (!taps1 || cap1 < *ntaps1 || !taps2 || cap2 < *ntaps2) return M17HIP_EINVAL;
    wide_default1(decim1, decim2, taps1);
    wide_default(decim2, taps2);
    return M17HIP_OK;
}
int m17hip_wide_config2(m17hip_ctx* c, uint32_t sources, uint32_t decim1, const float* taps1, uint32_t ntaps1, uint32_t decim2, const float* taps2,
                        uint32_t ntaps2, int iq_format)
{
    if (!c || sources < 1 || sources > 256 || decim1 < 1 || decim1 > 16 || decim2 < 1 || decim2 > 16) return M17HIP_EINVAL;
    if (iq_format != M17HIP_IQ_I16 && iq_format != M17HIP_IQ_F32 && iq_format != M17HIP_IQ_U8) return M17HIP_EINVAL;
    std::vector<float> h1(decim1 == 1 ? 1 : 8 * decim1 + 1), h2(32 * decim2 + 1);
    wide_default1(decim1, decim2, h1.data());
    wide_default(decim2, h2.data());
    if (!wide_stage_taps(taps1, ntaps1, 256, h1) || !wide_stage_taps(taps2, ntaps2, 1024, h2)) return M17HIP_EINVAL;
    return wide_setup(c, sources, iq_format, decim1, h1, decim2, h2);
}
// ---- a resampling second stage (ABI 615): sources at 48000 * decim1 * down / up ----------------------------------------------------------------
static uint32_t gcd_u32(uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; }
static bool resample_shape(uint32_t decim1, uint32_t up, uint32_t down)
{
    return decim1 >= 1 && decim1 <= 16 && up >= 1 && up <= 32 && down >= 1 && down <= 125 && up <= down && gcd_u32(up, down) == 1;
}
// Stage 2: the channel filter at 48000 * down — 32 * down + 1 taps, cutoff 5500 Hz — scaled in double to DC gain `up` (what the zero-stuffing takes), then
// rounded: at up == 1 wide_default(down) word for word.  Stage 1: cutoff at half the rate it leaves, as wide_default1 has it.
static void resample_default2(uint32_t up, uint32_t down, float* taps) { windowed_sinc(32 * down + 1, 5500.0 / (48000.0 * down), taps, (double)up); }
int m17hip_wide_resample_default_taps(uint32_t decim1, uint32_t up, uint32_t down, float* taps1, uint32_t cap1, uint32_t* ntaps1, float* taps2, uint32_t cap2,
                                      uint32_t* ntaps2)
{
    if (!resample_shape(decim1, up, down) || !ntaps1 || !ntaps2) return M17HIP_EINVAL;
    *ntaps1 = decim1 == 1 ? 1 : 8 * decim1 + 1;
    *ntaps2 = 32 * down + 1;
    if (!taps1 || cap1 < *ntaps1 || !taps2 || cap2 < *ntaps2) return M17HIP_EINVAL;
    wide_default1(decim1, 1, taps1);
    resample_default2(up, down, taps2);
    return M17HIP_OK;
}
int m17hip_wide_resample_ratio(uint32_t rate_hz, uint32_t* decim1, uint32_t* up, uint32_t* down)
{
    if (!rate_hz || !decim1 || !up || !down) return M17HIP_EINVAL;
    const uint32_t g = gcd_u32(rate_hz, 48000), N = rate_hz / g, U = 48000 / g;   // rate / 48000 = N / U in lowest terms
    if (U > 32) return M17HIP_EINVAL;
    uint32_t best = 0;
    for (uint32_t d = 16; d >= 1 && !best; --d) if (N % d == 0 && N / d <= 125 && N / d >= 2 * U) best = d;   // (the intermediate rate at or above 96 kSPS)
    for (uint32_t d = 16; d >= 1 && !best; --d) if (N % d == 0 && N / d <= 125 && N / d >= U) best = d;
    if (!best) return M17HIP_EINVAL;
    *decim1 = best; *up = U; *down = N / best;
    return M17HIP_OK;
}
int m17hip_wide_resample(m17hip_ctx* c, uint32_t sources, uint32_t decim1, const float* taps1, uint32_t ntaps1, uint32_t up, uint32_t down, const float* taps2,
                         uint32_t ntaps2, int iq_format)
{
    if (!c || sources < 1 || sources > 256 || !resample_shape(decim1, up, down)) return M17HIP_EINVAL;
    if (iq_format != M17HIP_IQ_I16 && iq_format != M17HIP_IQ_F32 && iq_format != M17HIP_IQ_U8) return M17HIP_EINVAL;
    std::vector<float> h1(decim1 == 1 ? 1 : 8 * decim1 + 1), h2(32 * down + 1);
    wide_default1(decim1, 1, h1.data());
    resample_default2(up, down, h2.data());
    if (!wide_stage_taps(taps1, ntaps1, 256, h1) || !wide_stage_taps(taps2, ntaps2, 4096, h2)) return M17HIP_EINVAL;
    return wide_setup(c, sources, iq_format, decim1, h1, 0, h2, 0, up, down);
}
int m17hip_wide_channels(m17hip_ctx* c, const uint32_t* source, const int32_t* fcw, uint32_t n)
{
    if (!c || n > c->maxC || (n > 0 && (!source || !fcw))) return M17HIP_EINVAL;
    auto& w = c->wide;
    if (!w.S || w.M) return M17HIP_ESTATE;   // (which sources exist is m17hip_wide_config's to say; under a raster the table is m17hip_wide_raster_channels')
    for (uint32_t ch = 0; ch < n; ++ch) if (source[ch] >= w.S) return M17HIP_EINVAL;
    if (w.scanning())   // (m17hip_wide_scan: a slot stays with its source; its word is its seed, read where the scan's feed starts over)
        for (uint32_t ch = 0; ch < n; ++ch) if (w.sc.pool[ch] && source[ch] != w.table[ch]) return M17HIP_ESTATE;
    for (uint32_t ch = 0; ch < n; ++ch) { w.table[ch] = source[ch]; w.table[c->maxC + ch] = (uint32_t)fcw[ch]; }
    w.dirty = true;   // (the next block uploaded brings it to the device: nothing is queued and nothing waited for here)
    return M17HIP_OK;
}
int m17hip_wide_raster_default_taps(uint32_t decim, float* taps, uint32_t capacity, uint32_t* ntaps)
{
    if (decim < 1 || decim > 64 || !ntaps) return M17HIP_EINVAL;
    *ntaps = 32 * decim + 1;
    if (!taps || capacity < *ntaps) return M17HIP_EINVAL;
    wide_default(decim, taps);
    return M17HIP_OK;
}
int m17hip_wide_raster_twiddles(uint32_t bins, float* out, uint32_t capacity)
{
    uint32_t m1, m2;
    if (!core::chan_factor(bins, m1, m2) || !out || capacity < 2 * bins) return M17HIP_EINVAL;
    chan_twiddles(bins, out);
    return M17HIP_OK;
}
int m17hip_wide_raster(m17hip_ctx* c, uint32_t sources, uint32_t decim, uint32_t bins, int iq_format, const float* taps, uint32_t ntaps)
{
    uint32_t m1, m2;
    if (!c || sources < 1 || sources > 256 || decim < 1 || decim > 64 || !core::chan_factor(bins, m1, m2)) return M17HIP_EINVAL;
    if (iq_format != M17HIP_IQ_I16 && iq_format != M17HIP_IQ_F32 && iq_format != M17HIP_IQ_U8) return M17HIP_EINVAL;
    std::vector<float> h(32 * decim + 1);
    wide_default(decim, h.data());
    if (!wide_stage_taps(taps, ntaps, 4096, h)) return M17HIP_EINVAL;
    return wide_setup(c, sources, iq_format, decim, h, 0, std::vector<float>(), bins);
}
int m17hip_wide_raster_channels(m17hip_ctx* c, const uint32_t* source, const int32_t* bin, uint32_t n)
{
    if (!c || n > c->maxC || (n > 0 && (!source || !bin))) return M17HIP_EINVAL;
    auto& w = c->wide;
    if (!w.S || !w.M) return M17HIP_ESTATE;   // (which sources and bins exist is m17hip_wide_raster's to say)
    const int32_t lo = -(int32_t)(w.M / 2), hi = (int32_t)((w.M - 1) / 2);
    for (uint32_t ch = 0; ch < n; ++ch) if (source[ch] >= w.S || bin[ch] < lo || bin[ch] > hi) return M17HIP_EINVAL;
    for (uint32_t ch = 0; ch < n; ++ch) { w.table[ch] = source[ch]; w.table[c->maxC + ch] = (uint32_t)(bin[ch] < 0 ? bin[ch] + (int32_t)w.M : bin[ch]); }
    w.dirty = true;   // (the next block uploaded brings it to the device: nothing is queued and nothing waited for here)
    return M17HIP_OK;
}
int m17hip_wide_survey(m17hip_ctx* c, uint32_t stride)
{
    if (!c || stride > 4096) return M17HIP_EINVAL;
    auto& w = c->wide;
    if (!w.S || !w.M || c->front_queued) return M17HIP_ESTATE;   // (a raster's bins are what is surveyed; the staged block belongs to the run being made)
    w.sv.stride = stride;   // (the next block uploaded is the first it holds for: nothing is queued and nothing waited for here)
    w.sv.forget();
    return M17HIP_OK;
}
int m17hip_wide_survey_fetch(m17hip_ctx* c, uint32_t back, float* power_host, uint64_t capacity, uint32_t* times, uint64_t* first_output)
{
    if (!c || back > 1 || !power_host) return M17HIP_EINVAL;
    auto& w = c->wide;
    auto& sv = w.sv;
    if (!w.S || !w.M || !sv.stride) return M17HIP_ESTATE;
    const size_t n = (size_t)w.S * w.M;
    if (capacity < n) return M17HIP_EINVAL;
    const int p = sv.latest ^ (int)back;
    if (!sv.valid[p]) return M17HIP_ESTATE;
    GUARD(c);
    HIPCHK(c, hipEventSynchronize(sv.ev[p]));   // (that block's survey and what its stream held in front of it: no run, no later block)
    HIPCHK(c, hipMemcpyAsync(power_host, sv.plane[p].get(), n * sizeof(float), hipMemcpyDeviceToHost, sv.fetch));
    HIPCHK(c, hipStreamSynchronize(sv.fetch));
    if (times) *times = sv.times[p];
    if (first_output) *first_output = sv.first_output[p];
    return M17HIP_OK;
}
// ---- the source spectrum (ABI 616): the averaged periodogram of every source, under every wideband configuration ------------------------------
// 0 for anything but a power of two in 64..4096
static uint32_t spectrum_logn(uint32_t points)
{
    for (uint32_t l = 6; l <= 12; ++l) if (points == 1u << l) return l;
    return 0;
}
// four-term Blackman-Harris (the minimum 92 dB one), periodic: the N-point DFT sees one whole period
static void spectrum_window(uint32_t N, float* w)
{
    const double pi = 3.14159265358979323846;
    for (uint32_t i = 0; i < N; ++i) {
        const double x = 2.0 * pi * i / N;
        w[i] = (float)(0.35875 - 0.48829 * std::cos(x) + 0.14128 * std::cos(2.0 * x) - 0.01168 * std::cos(3.0 * x));
    }
}
// tw[j] = exp(-2 pi j j / N) as (re, im), j < N / 2: cos and sin in double for j <= N / 4, rounded to float, exactly (1, 0) at 0 and (0, -1) at N / 4; the
// second quarter is the first one's mirror to the bit, tw[N / 2 - j] = (-re, im) of tw[j]
static void spectrum_twiddles(uint32_t N, float* tw)
{
    const double pi = 3.14159265358979323846;
    tw[0] = 1.0f; tw[1] = 0.0f;
    tw[2 * (N / 4)] = 0.0f; tw[2 * (N / 4) + 1] = -1.0f;
    for (uint32_t j = 1; j < N / 4; ++j) {
        const float re = (float)std::cos(2.0 * pi * j / N), im = (float)std::sin(2.0 * pi * j / N);
        tw[2 * j] = re; tw[2 * j + 1] = -im;
        tw[2 * (N / 2 - j)] = -re; tw[2 * (N / 2 - j) + 1] = -im;
    }
}
int m17hip_wide_spectrum_default_window(uint32_t points, float* out, uint32_t capacity)
{
    if (!spectrum_logn(points) || !out || capacity < points) return M17HIP_EINVAL;
    spectrum_window(points, out);
    return M17HIP_OK;
}
int m17hip_wide_spectrum_twiddles(uint32_t points, float* out, uint32_t capacity)
{
    if (!spectrum_logn(points) || !out || capacity < points) return M17HIP_EINVAL;
    spectrum_twiddles(points, out);
    return M17HIP_OK;
}
int m17hip_wide_spectrum(m17hip_ctx* c, uint32_t points, uint32_t hop, const float* window, uint32_t nwindow)
{
    if (!c) return M17HIP_EINVAL;
    auto& w = c->wide;
    auto& sp = w.sp;
    if (points) {
        if (!spectrum_logn(points) || hop < 1 || hop > (1u << 24)) return M17HIP_EINVAL;
        if (window ? nwindow != points : nwindow != 0) return M17HIP_EINVAL;
        for (uint32_t i = 0; window && i < points; ++i) if (!std::isfinite(window[i])) return M17HIP_EINVAL;
    }
    if (!w.S || c->front_queued) return M17HIP_ESTATE;   // (the planes have a row per source; the staged block belongs to the run being made)
    sp.forget();   // (the next block uploaded is the first it holds for: nothing is queued and nothing waited for here)
    w.sq.on = false; w.sq.forget();   // (the squelch's bins are this call's to redefine: off until m17hip_wide_squelch is called again)
    w.sc.on = false; w.sc.forget();   // (and the scan with it)
    sp.points = points;
    if (!points) return M17HIP_OK;
    sp.logn = spectrum_logn(points); sp.hop = hop;
    sp.table.resize(2 * (size_t)points);
    if (window) std::copy(window, window + points, sp.table.begin());
    else spectrum_window(points, sp.table.data());
    spectrum_twiddles(points, sp.table.data() + points);
    sp.dirty = true;
    return M17HIP_OK;
}
int m17hip_wide_spectrum_fetch(m17hip_ctx* c, uint32_t back, float* power_host, uint64_t capacity, uint32_t* frames, uint64_t* first_sample)
{
    if (!c || back > 1 || !power_host) return M17HIP_EINVAL;
    auto& w = c->wide;
    auto& sp = w.sp;
    if (!w.S || !sp.points) return M17HIP_ESTATE;
    const size_t n = (size_t)w.S * sp.points;
    if (capacity < n) return M17HIP_EINVAL;
    const int p = sp.latest ^ (int)back;
    if (!sp.valid[p]) return M17HIP_ESTATE;
    GUARD(c);
    HIPCHK(c, hipEventSynchronize(sp.ev[p]));   // (that block's spectrum and what its stream held in front of it: no run, no later block)
    HIPCHK(c, hipMemcpyAsync(power_host, sp.plane[p].get(), n * sizeof(float), hipMemcpyDeviceToHost, sp.fetch));
    HIPCHK(c, hipStreamSynchronize(sp.fetch));
    if (frames) *frames = sp.frames[p];
    if (first_sample) *first_sample = sp.first_sample[p];
    return M17HIP_OK;
}
// ---- the channel meter (ABI 618): level, offset and deviation sums per channel and window, under every wideband configuration --------------------
int m17hip_wide_meter(m17hip_ctx* c, uint32_t window)
{
    if (!c || (window && (window < 16 || window > 65536))) return M17HIP_EINVAL;
    auto& w = c->wide;
    if (!w.S || c->front_queued) return M17HIP_ESTATE;   // (the staged block belongs to the run being made)
    w.mt.forget();   // (the next block uploaded is the first it holds for: nothing is queued and nothing waited for here)
    w.mt.window = window;
    return M17HIP_OK;
}
// the plane `back` names, or -1
static int meter_plane(const m17hip_ctx* c, uint32_t back)
{
    const auto& mt = c->wide.mt;
    if (!c->wide.S || !mt.window) return -1;
    const int p = mt.latest ^ (int)back;
    return mt.valid[p] ? p : -1;
}
int m17hip_wide_meter_shape(m17hip_ctx* c, uint32_t back, uint32_t* channels, uint32_t* pieces, uint64_t* first_window, uint64_t* first_output, uint32_t* outputs)
{
    if (!c || back > 1) return M17HIP_EINVAL;
    const int p = meter_plane(c, back);
    if (p < 0) return M17HIP_ESTATE;
    const auto& mt = c->wide.mt;
    if (channels) *channels = mt.C[p];
    if (pieces) *pieces = mt.K[p];
    if (first_window) *first_window = mt.N0[p] / mt.win[p];
    if (first_output) *first_output = mt.N0[p];
    if (outputs) *outputs = mt.T[p];
    return M17HIP_OK;
}
int m17hip_wide_meter_fetch(m17hip_ctx* c, uint32_t back, float* planes_host, uint64_t capacity)
{
    if (!c || back > 1 || !planes_host) return M17HIP_EINVAL;
    const int p = meter_plane(c, back);
    if (p < 0) return M17HIP_ESTATE;
    auto& mt = c->wide.mt;
    const size_t n = (size_t)3 * mt.C[p] * mt.K[p];
    if (capacity < n) return M17HIP_EINVAL;
    GUARD(c);
    HIPCHK(c, hipEventSynchronize(mt.ev[p]));   // (that block's meter kernel and what its stream held in front of it: no run, no later block)
    HIPCHK(c, hipMemcpyAsync(planes_host, mt.plane[p].get(), n * sizeof(float), hipMemcpyDeviceToHost, mt.fetch));
    HIPCHK(c, hipStreamSynchronize(mt.fetch));
    return M17HIP_OK;
}
// ---- the spectrum squelch (ABI 619): the three tuners skip the channels whose band of the block's spectrum holds no carrier ----------------------------
// Both modes' call: `slots` says which one the levels turn on (m17hip_wide_squelch: hang in blocks, lead 0; m17hip_wide_squelch_slots: hang in slots).
static int squelch_set(m17hip_ctx* c, uint32_t half_bins, const float* open_level, const float* close_level, uint32_t nlevels, uint32_t hang, bool slots,
                       uint32_t lead)
{
    if (!c) return M17HIP_EINVAL;
    auto& w = c->wide;
    auto& sq = w.sq;
    const bool off = !open_level && nlevels == 0;
    if (!off) {
        if (!open_level || !close_level || nlevels < 1 || nlevels > 256 || half_bins > 64 || hang > 65535 || lead > 255) return M17HIP_EINVAL;
        for (uint32_t s = 0; s < nlevels; ++s)
            if (!std::isfinite(open_level[s]) || !std::isfinite(close_level[s]) || !(close_level[s] > 0.0f) || !(close_level[s] <= open_level[s])) return M17HIP_EINVAL;
    }
    if (!w.S || c->front_queued) return M17HIP_ESTATE;   // (the staged block belongs to the run being made)
    if (!off) {
        if (w.M || !w.sp.points) return M17HIP_ESTATE;   // (a raster's channels share their work; the decision is read from the block's spectrum)
        if (nlevels != w.S || half_bins >= w.sp.points / 2) return M17HIP_EINVAL;
    }
    sq.forget();   // (the next block uploaded is the first it holds for: nothing is queued and nothing waited for here)
    sq.fresh = true;
    sq.on = !off;
    sq.floor = false;   // (the levels this call carries serve; m17hip_wide_squelch_floor comes after it)
    w.sc.on = false; w.sc.forget();   // (the scan needs the floor: m17hip_wide_scan comes after that)
    if (off) return M17HIP_OK;
    sq.B = half_bins; sq.hang = hang; sq.slots = slots; sq.lead = lead;
    sq.levels.assign(open_level, open_level + nlevels);
    sq.levels.insert(sq.levels.end(), close_level, close_level + nlevels);
    sq.dirty = true;
    return M17HIP_OK;
}
int m17hip_wide_squelch(m17hip_ctx* c, uint32_t half_bins, const float* open_level, const float* close_level, uint32_t nlevels, uint32_t hang)
{
    return squelch_set(c, half_bins, open_level, close_level, nlevels, hang, false, 0);
}
// ---- the time-resolved squelch (ABI 620): a decision per slot of 16 frames, a skip per tile of the tuner's outputs --------------------------------------
int m17hip_wide_squelch_slots(m17hip_ctx* c, uint32_t half_bins, const float* open_level, const float* close_level, uint32_t nlevels, uint32_t hang, uint32_t lead)
{
    return squelch_set(c, half_bins, open_level, close_level, nlevels, hang, true, lead);
}
int m17hip_wide_squelch_slots_fetch(m17hip_ctx* c, uint32_t back, uint32_t* state_host, float* bands_host, uint32_t* mask_host, uint64_t cap_channels,
                                    uint64_t cap_bands, uint64_t cap_mask_words, uint32_t* channels, uint32_t* slots, uint32_t* tiles, uint32_t* frames)
{
    if (!c || back > 1 || !state_host || !bands_host || !mask_host) return M17HIP_EINVAL;
    auto& sq = c->wide.sq;
    if (!c->wide.S || !sq.on || !sq.slots) return M17HIP_ESTATE;
    const int p = sq.latest ^ (int)back;
    if (!sq.valid[p]) return M17HIP_ESTATE;
    const size_t n = sq.C[p], nb = n * sq.G[p], nm = n * squelch_tile_words(sq.tiles[p]);
    if (cap_channels < n || cap_bands < nb || cap_mask_words < nm) return M17HIP_EINVAL;
    GUARD(c);
    HIPCHK(c, hipEventSynchronize(sq.ev[p]));   // (that block's squelch kernels and what its stream held in front of them: not its tuner, no run, no later block)
    HIPCHK(c, hipMemcpyAsync(state_host, sq.state[p].get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost, sq.fetch));
    if (nb) HIPCHK(c, hipMemcpyAsync(bands_host, sq.sband[p].get(), nb * sizeof(float), hipMemcpyDeviceToHost, sq.fetch));
    HIPCHK(c, hipMemcpyAsync(mask_host, sq.mask[p].get(), nm * sizeof(uint32_t), hipMemcpyDeviceToHost, sq.fetch));
    HIPCHK(c, hipStreamSynchronize(sq.fetch));
    if (channels) *channels = (uint32_t)n;
    if (slots) *slots = sq.G[p];
    if (tiles) *tiles = sq.tiles[p];
    if (frames) *frames = sq.frames[p];
    return M17HIP_OK;
}
int m17hip_wide_squelch_fetch(m17hip_ctx* c, uint32_t back, uint32_t* state_host, float* band_host, uint64_t capacity, uint32_t* channels, uint32_t* frames)
{
    if (!c || back > 1 || !state_host || !band_host) return M17HIP_EINVAL;
    auto& sq = c->wide.sq;
    if (!c->wide.S || !sq.on || sq.slots) return M17HIP_ESTATE;   // (the slot mode's planes are m17hip_wide_squelch_slots_fetch's)
    const int p = sq.latest ^ (int)back;
    if (!sq.valid[p]) return M17HIP_ESTATE;
    const size_t n = sq.C[p];
    if (capacity < n) return M17HIP_EINVAL;
    GUARD(c);
    HIPCHK(c, hipEventSynchronize(sq.ev[p]));   // (that block's squelch kernel and what its stream held in front of it: not its tuner, no run, no later block)
    HIPCHK(c, hipMemcpyAsync(state_host, sq.state[p].get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost, sq.fetch));
    HIPCHK(c, hipMemcpyAsync(band_host, sq.band[p].get(), n * sizeof(float), hipMemcpyDeviceToHost, sq.fetch));
    HIPCHK(c, hipStreamSynchronize(sq.fetch));
    if (channels) *channels = (uint32_t)n;
    if (frames) *frames = sq.frames[p];
    return M17HIP_OK;
}
// ---- the floor on the device (ABI 621): the levels of either mode from the block's own plane ------------------------------------------------------------
int m17hip_wide_squelch_floor(m17hip_ctx* c, float open_ratio, float close_ratio, float rise, float fall, float floor_min)
{
    if (!c) return M17HIP_EINVAL;
    auto& sq = c->wide.sq;
    if (!std::isfinite(open_ratio) || !std::isfinite(close_ratio) || !std::isfinite(rise) || !std::isfinite(fall) || !std::isfinite(floor_min)) return M17HIP_EINVAL;
    const bool off = open_ratio == 0.0f && close_ratio == 0.0f;
    if (!off && (!(close_ratio > 0.0f) || !(close_ratio <= open_ratio))) return M17HIP_EINVAL;
    if (!(rise > 0.0f) || !(rise <= 1.0f) || !(fall > 0.0f) || !(fall <= 1.0f) || floor_min < 0.0f) return M17HIP_EINVAL;
    if (!c->wide.S || c->front_queued) return M17HIP_ESTATE;   // (the staged block belongs to the run being made)
    if (!off && !sq.on) return M17HIP_ESTATE;
    sq.forget();   // (as either squelch call: the next block uploaded is the first it holds for, hold counts zeroed and floor forgotten; nothing is queued here)
    sq.fresh = true;
    sq.floor = !off && sq.on;
    c->wide.sc.forget();   // (the scan's feed starts over with the squelch's)
    if (off) { c->wide.sc.on = false; return M17HIP_OK; }   // (the scan reads the floor plane: off with it)
    sq.f_open = open_ratio; sq.f_close = close_ratio; sq.f_rise = rise; sq.f_fall = fall; sq.f_min = floor_min;
    return M17HIP_OK;
}
int m17hip_wide_squelch_floor_fetch(m17hip_ctx* c, uint32_t back, float* plane_host, uint64_t capacity, uint32_t* sources, uint32_t* frames)
{
    if (!c || back > 1 || !plane_host) return M17HIP_EINVAL;
    auto& sq = c->wide.sq;
    if (!c->wide.S || !sq.on || !sq.floor) return M17HIP_ESTATE;
    const int p = sq.latest ^ (int)back;
    if (!sq.valid[p] || !sq.has_floor[p]) return M17HIP_ESTATE;
    const size_t n = (size_t)4 * c->wide.S;
    if (capacity < n) return M17HIP_EINVAL;
    GUARD(c);
    HIPCHK(c, hipEventSynchronize(sq.ev[p]));   // (that block's floor and squelch kernels and what its stream held in front of them: not its tuner, no run, no later block)
    HIPCHK(c, hipMemcpyAsync(plane_host, sq.fplane[p].get(), n * sizeof(float), hipMemcpyDeviceToHost, sq.fetch));
    HIPCHK(c, hipStreamSynchronize(sq.fetch));
    if (sources) *sources = c->wide.S;
    if (frames) *frames = sq.frames[p];
    return M17HIP_OK;
}
// ---- the carrier scan (ABI 622): the block's carriers found and a pool of channels tuned to them on the device, in front of the block squelch -----------
int m17hip_wide_scan(m17hip_ctx* c, const uint8_t* pool, uint32_t n, uint32_t guard_bins)
{
    if (!c) return M17HIP_EINVAL;
    auto& w = c->wide;
    auto& sc = w.sc;
    const bool off = !pool && n == 0;
    if (!off && (!pool || n < 1 || n > c->maxC || guard_bins < 3)) return M17HIP_EINVAL;
    if (!w.S || c->front_queued) return M17HIP_ESTATE;   // (the staged block belongs to the run being made)
    if (!off) {
        if (w.M || !w.sp.points || w.sp.points > SCAN_MAX_POINTS || !w.sq.on || w.sq.slots || !w.sq.floor) return M17HIP_ESTATE;
        if (guard_bins > w.sp.points / 4) return M17HIP_EINVAL;
    }
    if (off && !sc.on) return M17HIP_OK;   // (off stays off: the squelch's feed is not touched)
    // as either squelch call and the floor call: the next block uploaded is the first it holds for, the hold counts and the floor start over and the slots
    // take their seeds; nothing is queued and nothing waited for here
    w.sq.forget();
    w.sq.fresh = true;
    sc.forget();
    sc.on = !off;
    if (off) return M17HIP_OK;
    sc.X = guard_bins;
    sc.pool.assign(c->maxC, 0u);
    for (uint32_t ch = 0; ch < n; ++ch) sc.pool[ch] = pool[ch] ? 1u : 0u;
    sc.dirty = true;
    return M17HIP_OK;
}
int m17hip_wide_scan_fetch(m17hip_ctx* c, uint32_t back, int32_t* fcw_host, uint32_t* flags_host, uint32_t* missed_host, uint64_t cap_channels,
                           uint32_t* channels, uint32_t* sources, uint32_t* frames)
{
    if (!c || back > 1 || !fcw_host || !flags_host || !missed_host) return M17HIP_EINVAL;
    auto& w = c->wide;
    auto& sc = w.sc;
    if (!w.S || !w.scanning()) return M17HIP_ESTATE;
    const int p = sc.latest ^ (int)back;
    if (!sc.valid[p]) return M17HIP_ESTATE;
    const size_t C = sc.C[p], n = cap_channels < C ? (size_t)cap_channels : C;
    GUARD(c);
    HIPCHK(c, hipEventSynchronize(sc.ev[p]));   // (that block's scan kernel and what its stream held in front of it: not its squelch kernel, not its tuner, no run, no later block)
    if (n) {
        HIPCHK(c, hipMemcpyAsync(fcw_host, sc.plane[p].get() + c->maxC, n * sizeof(uint32_t), hipMemcpyDeviceToHost, w.sq.fetch));
        HIPCHK(c, hipMemcpyAsync(flags_host, sc.flags[p].get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost, w.sq.fetch));
    }
    HIPCHK(c, hipMemcpyAsync(missed_host, sc.missed[p].get(), (size_t)w.S * sizeof(uint32_t), hipMemcpyDeviceToHost, w.sq.fetch));
    HIPCHK(c, hipStreamSynchronize(w.sq.fetch));
    if (channels) *channels = (uint32_t)C;
    if (sources) *sources = w.S;
    if (frames) *frames = sc.frames[p];
    return n < C ? M17HIP_ETRUNC : M17HIP_OK;
}
int m17hip_upload_wide(m17hip_ctx* c, const void* host, float gain, uint32_t C, uint32_t T, size_t pitch) { return upload_wide(c, host, gain, C, T, pitch, IQ_FROM_HOST); }
int m17hip_upload_wide_device(m17hip_ctx* c, const void* dev, float gain, uint32_t C, uint32_t T, size_t pitch) { return upload_wide(c, dev, gain, C, T, pitch, 0); }
int m17hip_upload_wide_async(m17hip_ctx* c, const void* host, float gain, uint32_t C, uint32_t T, size_t pitch)
{
    return upload_wide(c, host, gain, C, T, pitch, IQ_FROM_HOST | IQ_STAGED);
}
int m17hip_upload_wide_device_async(m17hip_ctx* c, const void* dev, float gain, uint32_t C, uint32_t T, size_t pitch)
{
    return upload_wide(c, dev, gain, C, T, pitch, IQ_STAGED);
}

int m17hip_input_format(m17hip_ctx* c, int* stream_format, uint64_t* f32_bytes)
{
    if (!c) return M17HIP_EINVAL;
    if (stream_format) *stream_format = c->stream_fmt;
    if (f32_bytes) *f32_bytes = c->fslab[0].bytes() + c->fslab[1].bytes() + (c->hist_f.size() + c->bnd_hist_f.size()) * sizeof(float);
    return M17HIP_OK;
}

int m17hip_input_alternate(m17hip_ctx* c, uint32_t C, uint32_t T)
{
    if (!c || C == 0 || T == 0 || C > c->maxC || T > c->maxT) return M17HIP_EINVAL;
    GUARD(c);
    if (c->front_queued) return M17HIP_ESTATE;
    if (!c->other().x || c->other().C != C || c->other().T != T) return M17HIP_ESTATE;   // the other slab does not hold such an input
    if (!c->slab_fmt[c->slot ^ 1] || (c->stream_fmt && c->slab_fmt[c->slot ^ 1] != c->stream_fmt)) return M17HIP_ESTATE;   // (... of the stream's format)
    c->staged = true; c->stagedC = C; c->stagedT = T;
    return M17HIP_OK;
}

// m17hip_synth_i16 (points == nullptr: the impairments of `params`) and m17hip_synth_sweep_i16 (channel c under points[(chan0 + c) % n_points])
static int synth_impl(m17hip_ctx* c, const m17_synth_params* params, const m17_impairment* points, uint32_t n_points, uint32_t C, uint32_t T,
                      uint32_t chan0)
{
    if (!c || !params || C == 0 || T == 0 || C > c->maxC || T > c->maxT || params->n_frames < 0 || params->kind > 4) return M17HIP_EINVAL;
    GUARD(c);
    if (c->front_queued) return M17HIP_ESTATE;   // the slabs belong to the run m17hip_demod_front has started
    if (params->kind == 4 && (params->n_frames < 1 || params->n_frames > 33)) return M17HIP_EINVAL;   // 5-bit frame numbers
    static_assert(sizeof(ModParams) == sizeof(m17_synth_params), "parameter block layout");
    static_assert(sizeof(ModImpair) == sizeof(m17_impairment) && sizeof(ModImpair) == 32, "m17_impairment layout");
    ModParams mp;
    std::memcpy(&mp, params, sizeof(mp));
    const size_t sym_pitch = round_up((size_t)mod_max_symbols(mp.n_frames, mp.n_preamble), 16);
    const size_t sym_bytes = round_up((size_t)C * sym_pitch, 256);
    const size_t pts_at = sym_bytes + round_up((size_t)C * 4, 256);
    const size_t need = points ? pts_at + (size_t)n_points * sizeof(ModImpair) : sym_bytes + (size_t)C * 4;
    InputTarget<int16_t> in;
    int r = input_target(c, in);
    if (r) return r;
    // the symbol staging lives in its own allocation: the per-operator scratch may be in use by work queued on the main stream
    if (need > c->synth_scratch.size() && c->synth_scratch) HIPCHK(c, hipDeviceSynchronize());   // (nothing still reads the one it outgrew)
    HIPCHK(c, c->synth_scratch.grow(need, &c->last_hip));
    int8_t* sym = reinterpret_cast<int8_t*>(c->synth_scratch.get());
    uint32_t* nsym = reinterpret_cast<uint32_t*>(c->synth_scratch + sym_bytes);
    hipLaunchKernelGGL(mod_symbols_kernel, dim3((C + 63) / 64), dim3(64), 0, in.st, mp, C, chan0, sym, sym_pitch, nsym);
    HIPCHK(c, hipGetLastError());
    if (points) {
        ModImpair* pts = reinterpret_cast<ModImpair*>(c->synth_scratch + pts_at);
        HIPCHK(c, hipMemcpyAsync(pts, points, (size_t)n_points * sizeof(ModImpair), hipMemcpyHostToDevice, in.st));
        hipLaunchKernelGGL(mod_shape_grid_kernel, dim3((T + 255) / 256, C), dim3(256), 0, in.st, mp, pts, n_points, C, T, chan0, sym, sym_pitch, nsym, in.x,
                           c->xpitch);
    } else {
        hipLaunchKernelGGL(mod_shape_kernel, dim3((T + 255) / 256, C), dim3(256), 0, in.st, mp, C, T, chan0, sym, sym_pitch, nsym, in.x, c->xpitch);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(in.st));
    input_done(c, in, C, T);
    return M17HIP_OK;
}

int m17hip_synth_i16(m17hip_ctx* c, const m17_synth_params* params, uint32_t C, uint32_t T, uint32_t chan0)
{
    return synth_impl(c, params, nullptr, 0, C, T, chan0);
}

int m17hip_synth_sweep_i16(m17hip_ctx* c, const m17_synth_params* base, const m17_impairment* points, uint32_t n_points, uint32_t C, uint32_t T,
                           uint32_t chan0)
{
    if (!points || n_points == 0 || n_points > M17HIP_MAX_SWEEP_POINTS) return M17HIP_EINVAL;
    for (uint32_t i = 0; i < n_points; ++i) {
        const m17_impairment& p = points[i];
        if (!std::isfinite(p.noise_sigma) || !std::isfinite(p.tail_sigma) || p.noise_sigma < 0.0 || p.tail_sigma < 0.0) return M17HIP_EINVAL;
        if (!std::isfinite(p.dc_offset) || !std::isfinite(p.gain)) return M17HIP_EINVAL;
    }
    return synth_impl(c, base, points, n_points, C, T, chan0);
}

// Caller-supplied transmissions: mod_symbols_tx_kernel fills the symbol staging mod_symbols_kernel would have filled, mod_shape_kernel runs as
// for m17hip_synth_i16.  Every index the symbols kernel forms is bounded HERE (it re-checks nothing).
int m17hip_synth_tx_i16(m17hip_ctx* c, const m17_synth_params* base, const m17_tx* tx, const uint8_t* lsf30, const uint8_t* rows, uint32_t n_rows,
                        uint32_t C, uint32_t T, uint32_t chan0)
{
    if (!c || !base || !tx || !rows || C == 0 || T == 0 || C > c->maxC || T > c->maxT) return M17HIP_EINVAL;
    static_assert(sizeof(ModTx) == sizeof(m17_tx) && sizeof(ModTx) == 16, "m17_tx layout");
    uint32_t max_frames = 0, max_slots = 0;
    for (uint32_t i = 0; i < C; ++i) {
        const m17_tx& t = tx[i];
        if (t.kind > 2u || t.reserved != 0u || (t.kind != 0u && !lsf30)) return M17HIP_EINVAL;
        if (t.n_frames > T / 1920u + 1u || (uint64_t)t.first_row + t.n_frames > n_rows) return M17HIP_EINVAL;
        max_frames = std::max(max_frames, t.n_frames);
        max_slots = std::max(max_slots, t.n_frames + (t.kind != 0u ? 1u : 0u));
    }
    GUARD(c);
    if (c->front_queued) return M17HIP_ESTATE;   // the slabs belong to the run m17hip_demod_front has started
    ModParams mp;
    std::memcpy(&mp, base, sizeof(mp));
    mp.kind = 1;        // (the shaper asks only whether this is 3)
    mp.n_frames = 0;
    // preambles past the end of the slab are cut off whatever their number: bounding it bounds the staging
    const uint32_t n_pre = mp.n_preamble > 0 ? std::min((uint32_t)mp.n_preamble, T / 1920u + 2u) : 0u;
    const size_t sym_pitch = round_up((size_t)mod_max_symbols((int)max_frames, (int)n_pre), 16);
    const size_t sym_bytes = round_up((size_t)C * sym_pitch, 256);
    const size_t tx_at = sym_bytes + round_up((size_t)C * 4, 256);
    const size_t lsf_at = tx_at + round_up((size_t)C * sizeof(ModTx), 256);
    const size_t rows_at = lsf_at + round_up((size_t)C * 30, 256);
    const size_t need = rows_at + std::max<size_t>((size_t)n_rows * 32, 32);
    InputTarget<int16_t> in;
    int r = input_target(c, in);
    if (r) return r;
    if (need > c->synth_scratch.size() && c->synth_scratch) HIPCHK(c, hipDeviceSynchronize());   // (nothing still reads the one it outgrew)
    HIPCHK(c, c->synth_scratch.grow(need, &c->last_hip));
    int8_t* sym = reinterpret_cast<int8_t*>(c->synth_scratch.get());
    uint32_t* nsym = reinterpret_cast<uint32_t*>(c->synth_scratch + sym_bytes);
    ModTx* dtx = reinterpret_cast<ModTx*>(c->synth_scratch + tx_at);
    uint8_t* dlsf = reinterpret_cast<uint8_t*>(c->synth_scratch + lsf_at);
    uint8_t* drows = reinterpret_cast<uint8_t*>(c->synth_scratch + rows_at);
    HIPCHK(c, hipMemcpyAsync(dtx, tx, (size_t)C * sizeof(ModTx), hipMemcpyHostToDevice, in.st));
    if (lsf30) HIPCHK(c, hipMemcpyAsync(dlsf, lsf30, (size_t)C * 30, hipMemcpyHostToDevice, in.st));
    if (n_rows) HIPCHK(c, hipMemcpyAsync(drows, rows, (size_t)n_rows * 32, hipMemcpyHostToDevice, in.st));
    hipLaunchKernelGGL(mod_symbols_tx_kernel, dim3(1 + max_slots, C), dim3(64), 0, in.st, dtx, dlsf, drows, n_pre, sym, sym_pitch, nsym);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(mod_shape_kernel, dim3((T + 255) / 256, C), dim3(256), 0, in.st, mp, C, T, chan0, sym, sym_pitch, nsym, in.x, c->xpitch);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(in.st));
    input_done(c, in, C, T);
    return M17HIP_OK;
}

// ---- the wideband signal generator (ABI 617): FM-multiplex basebands of the int16 input slab ---------------------------------------------------
static uint32_t wtx_gcd(uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; }
// K = 2^63 hz_per_unit / (48000 p^2), rounded half up, in integers: hz_per_unit is mant 2^(e - 53) exactly (frexp), the default 2400 / 21504 a quotient of
// integers.  Refused: a K of 0 or of 2^63 and more, a numerator that does not fit 128 bits.
int m17hip_synth_wide_k(double hz_per_unit, uint32_t p, uint64_t* k)
{
    if (!k || p < 1 || p > 2000 || !std::isfinite(hz_per_unit) || hz_per_unit < 0.0) return M17HIP_EINVAL;
    typedef unsigned __int128 u128;
    u128 num, den = (u128)48000u * p * p;
    if (hz_per_unit == 0.0) { num = (u128)2400u << 63; den *= 21504u; }
    else {
        int e = 0;
        const double f = std::frexp(hz_per_unit, &e);   // hz_per_unit = f 2^e, 0.5 <= f < 1
        const uint64_t mant = (uint64_t)std::ldexp(f, 53);
        const int sh = e + 10;   // 2^63 mant 2^(e - 53) = mant 2^(e + 10)
        if (sh > 74) return M17HIP_EINVAL;
        if (sh >= 0) num = (u128)mant << sh;
        else { if (-sh > 64) return M17HIP_EINVAL; num = mant; den <<= -sh; }
    }
    const u128 q = (num + den / 2) / den;
    if (q == 0 || q >= ((u128)1 << 63)) return M17HIP_EINVAL;
    *k = (uint64_t)q;
    return M17HIP_OK;
}
int m17hip_synth_wide_config(m17hip_ctx* c, uint32_t sources, uint32_t p, uint32_t q, int iq_format, uint64_t k, float noise_sigma, uint64_t seed,
                             uint64_t first_sample)
{
    if (!c || sources < 1 || sources > 256 || p < 1 || p > 2000 || q < 1 || q > 32 || p < q || wtx_gcd(p, q) != 1) return M17HIP_EINVAL;
    if (iq_format != M17HIP_IQ_I16 && iq_format != M17HIP_IQ_F32 && iq_format != M17HIP_IQ_U8) return M17HIP_EINVAL;
    if (!std::isfinite(noise_sigma) || noise_sigma < 0.0f || first_sample % p) return M17HIP_EINVAL;
    if (c->front_queued) return M17HIP_ESTATE;
    auto& w = c->wtx;
    w.S = sources; w.P = p; w.Q = q; w.fmt = iq_format; w.K = k; w.sigma = noise_sigma; w.seed = seed; w.first = w.count = first_sample;
    w.table.assign(c->maxC, m17_wide_tx{0u, 0, 0u, 0.0f});   // (a fresh table: nobody transmits)
    w.dirty = true; w.fresh = true;
    return M17HIP_OK;
}
int m17hip_synth_wide_channels(m17hip_ctx* c, const m17_wide_tx* tx, uint32_t n)
{
    if (!c || !tx || n > c->maxC) return M17HIP_EINVAL;
    auto& w = c->wtx;
    if (!w.S || c->front_queued) return M17HIP_ESTATE;
    for (uint32_t i = 0; i < n; ++i)
        if (tx[i].source >= w.S || !std::isfinite(tx[i].amplitude) || tx[i].amplitude < 0.0f) return M17HIP_EINVAL;
    std::copy(tx, tx + n, w.table.begin());
    w.dirty = true;
    return M17HIP_OK;
}
static int synth_wide(m17hip_ctx* c, void* dst, uint32_t C, uint32_t T, size_t pitch, bool host)
{
    if (!c || !dst || C == 0 || T == 0 || C > c->maxC || T > c->maxT) return M17HIP_EINVAL;
    auto& w = c->wtx;
    if (!w.S || c->front_queued || c->stream_fmt == M17HIP_FORMAT_F32) return M17HIP_ESTATE;
    if (!c->uploaded || c->slab_fmt[c->slot] != M17HIP_FORMAT_I16 || c->now().C != C || c->now().T != T) return M17HIP_ESTATE;   // (no such int16 input there)
    if (T % w.Q) return M17HIP_EINVAL;
    const uint64_t W64 = (uint64_t)(T / w.Q) * w.P;
    if (W64 > 0xFFFFFFFFull || pitch < W64) return M17HIP_EINVAL;
    const uint32_t W = (uint32_t)W64;
    GUARD(c);
    const hipStream_t st = c->stream;
    const size_t sb = iq_sample_bytes(w.fmt);
    int r;
    if (!w.a2 && (r = alloc_code(c, w.a2.alloc(c->maxC)))) return r;
    if (!w.last && (r = alloc_code(c, w.last.alloc(2 * (size_t)c->maxC)))) return r;
    if ((r = alloc_code(c, w.plane.grow((size_t)C * T, &c->last_hip)))) return r;   // (every earlier block is complete: nothing reads the one it outgrew)
    if (host && (r = alloc_code(c, w.out.grow((size_t)w.S * W * sb, &c->last_hip)))) return r;
    if (w.fresh) {
        HIPCHK(c, hipMemsetAsync(w.a2, 0, w.a2.size() * 8, st));
        HIPCHK(c, hipMemsetAsync(w.last, 0, w.last.size() * 4, st));
        w.fresh = false;
    }
    if (w.dirty || !w.dev.live() || w.dev_C != C) {   // the lists by source of the channels < C that transmit, into the copy no queued launch reads
        uint32_t* t = nullptr;
        HIPCHK(c, w.dev.begin_write(wtx_table_words(256, c->maxC), &t));
        uint32_t* first = t;
        std::fill(first, first + w.S + 1, 0u);
        for (uint32_t ch = 0; ch < C; ++ch) if (w.table[ch].amplitude > 0.0f) ++first[w.table[ch].source + 1];   // (a term of amplitude 0 is a zero: +0 + -0 = +0)
        for (uint32_t s = 0; s < w.S; ++s) first[s + 1] += first[s];
        std::vector<uint32_t> at(first, first + w.S);
        uint32_t* ent = t + w.S + 1;
        for (uint32_t ch = 0; ch < C; ++ch) {
            const m17_wide_tx& e = w.table[ch];
            if (!(e.amplitude > 0.0f)) continue;
            uint32_t* o = ent + WTX_ENTRY * (size_t)at[e.source]++;
            o[0] = ch; o[1] = (uint32_t)e.fcw; o[2] = e.phase0;
            std::memcpy(o + 3, &e.amplitude, 4);
        }
        HIPCHK(c, w.dev.publish(wtx_table_words(w.S, first[w.S]), st));
        w.dirty = false; w.dev_C = C;
    }
    HIPCHK(c, w.dev.before_read(st));
    const int32_t* last_in = w.last.get() + (size_t)w.par * c->maxC;
    int32_t* last_out = w.last.get() + (size_t)(w.par ^ 1) * c->maxC;
    const uint32_t NK = wtx_span(w.P, w.Q), CH = wtx_chunk(NK);
    void* out = host ? (void*)w.out.get() : dst;
    const size_t opitch = host ? (size_t)W : pitch;
    {
        Timed tm(c, KT_WIDE_TX, st);
        hipLaunchKernelGGL(wide_tx_prefix_kernel, dim3(c->maxC), dim3(64), 0, st, c->now().x.get(), c->xpitch, C, T, w.K * w.P * w.P, w.a2.get(), last_in,
                           last_out, w.plane.get(), (size_t)T);
        HIPCHK(c, hipGetLastError());
        r = with_iq_type(w.fmt, [&](auto s) -> int {
            hipLaunchKernelGGL(wide_tx_mux_kernel<decltype(s)>, dim3((W + WTX_TILE - 1) / WTX_TILE, w.S), dim3(WTX_THREADS), wtx_lds_bytes(NK, CH), st,
                               c->now().x.get(), c->xpitch, w.plane.get(), (size_t)T, last_in, w.dev.dev(), w.S, w.P, w.Q, w.K, W, w.count, NK, CH, w.sigma,
                               w.seed, static_cast<decltype(s)*>(out), opitch);
            HIPCHK(c, hipGetLastError());
            return M17HIP_OK;
        });
        if (r) return r;
    }
    HIPCHK(c, w.dev.after_read(RD_MAIN, st));
    if (host) HIPCHK(c, hipMemcpy2DAsync(dst, pitch * sb, out, opitch * sb, (size_t)W * sb, w.S, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));   // complete when it returns: what m17hip_upload_wide_device asks of its producer
    w.par ^= 1;
    w.count += W;
    return M17HIP_OK;
}
int m17hip_synth_wide(m17hip_ctx* c, void* dst_host, uint32_t C, uint32_t T, size_t pitch) { return synth_wide(c, dst_host, C, T, pitch, true); }
int m17hip_synth_wide_device(m17hip_ctx* c, void* dst_dev, uint32_t C, uint32_t T, size_t pitch) { return synth_wide(c, dst_dev, C, T, pitch, false); }

int m17hip_fir_rrc150(m17hip_ctx* c, uint32_t C, uint32_t T, uint32_t flags, float* out_host)
{
    if (!c || C == 0 || T == 0 || C > c->maxC || T > c->maxT || (flags & ~M17HIP_FLAG_INVERT)) return M17HIP_EINVAL;
    GUARD(c);
    if (c->front_queued) return M17HIP_ESTATE;
    if (!c->uploaded) return M17HIP_ESTATE;
    uint32_t kflags; const uint32_t* pol;
    if (int r = resolve_polarity(c, C, flags, c->stream, kflags, pol)) return r;
    if (int r = launch_fir(c, C, T, kflags, false, c->stream, 0, nullptr, pol)) return r;   // (an operator call: the whole chip is its own)
    if (out_host) {
        HIPCHK(c, hipMemcpy2DAsync(out_host, (size_t)T * sizeof(float), c->now().y + YPRE, c->ypitch * sizeof(float), (size_t)T * sizeof(float), C,
                                   hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return M17HIP_OK;
}

int m17hip_correlator(m17hip_ctx* c, uint32_t C, uint32_t T, float* limit_host, float* corr_host)
{
    if (!c || C == 0 || T == 0 || C > c->maxC || T > c->maxT) return M17HIP_EINVAL;
    GUARD(c);
    if (c->front_queued) return M17HIP_ESTATE;
    const size_t n = (size_t)C * T;
    HIPCHK(c, c->scratch.grow(5 * n * sizeof(float), &c->last_hip));
    float* limit = (float*)c->scratch.get();
    float* corr = limit + n;
    {   // the limit filter is a handful of latency-bound workgroups, the correlations an HBM-bound elementwise pass: side by side
        Timed tm(c, KT_CORR);
        HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
        if (T % 4 == 0) hipLaunchKernelGGL(correlate4_kernel, dim3((T / 4 + 255) / 256, C), dim3(256), 0, c->side, c->now().y, c->ypitch, corr, C, T, 0u, T);
        else hipLaunchKernelGGL(correlate_kernel, dim3((T + 255) / 256, C), dim3(256), 0, c->side, c->now().y, c->ypitch, corr, C, T, 0u, T);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->ev_join, c->side));
#ifdef M17_TOOLS
        if (c->limit_form == 0 && T % LP_TILE == 0 && T >= 4 * LP_TILE && (((size_t)C * T) & 3) == 0)
            hipLaunchKernelGGL(limit_pipe_kernel, dim3((C + LP_CH - 1) / LP_CH), dim3(320), 0, c->stream, c->now().y, c->ypitch, limit, (size_t)T, C, T, (const float*)nullptr, (float*)nullptr);
        else
#endif
        if (T % LR_TILE == 0 && (((size_t)C * T) & 3) == 0)
            hipLaunchKernelGGL(limit_relay_kernel, dim3((C + LR_CH - 1) / LR_CH), dim3(320), 0, c->stream, c->now().y, c->ypitch, limit, (size_t)T, C, T, (const float*)nullptr, (float*)nullptr);
        else
            hipLaunchKernelGGL(limit_kernel, dim3((C + 63) / 64), dim3(64), 0, c->stream, c->now().y, c->ypitch, limit, C, T);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    }
    HIPCHK(c, hipGetLastError());
    if (limit_host) HIPCHK(c, hipMemcpyAsync(limit_host, limit, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (corr_host) HIPCHK(c, hipMemcpyAsync(corr_host, corr, 4 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return M17HIP_OK;
}

int m17hip_dcd(m17hip_ctx* c, uint32_t C, uint32_t T, uint32_t flags, float* sums_host, uint32_t* ticks_out)
{
    if (!c || C == 0 || T == 0 || C > c->maxC || T > c->maxT) return M17HIP_EINVAL;
    if (flags & ~M17HIP_FLAG_INVERT) return M17HIP_EINVAL;
    GUARD(c);
    if (c->front_queued) return M17HIP_ESTATE;
    if (!c->uploaded) return M17HIP_ESTATE;
    // operator-level call: always from a fresh DFT state at stream position 0
    HIPCHK(c, hipMemsetAsync(c->dcd_state, 0, (size_t)C * sizeof(DcdState), c->stream));
    uint32_t kflags; const uint32_t* pol;
    if (int r = resolve_polarity(c, C, flags, c->stream, kflags, pol)) return r;
    if (int r = launch_dcd(c, C, T, kflags, 0, c->dcd_form == 1, c->stream, 0, pol)) return r;
    const uint32_t ticks = T / TICK;
    if (ticks_out) *ticks_out = ticks;
    if (sums_host && ticks)
        HIPCHK(c, hipMemcpy2DAsync(sums_host, (size_t)ticks * 12 * sizeof(float), c->now().dcd, (size_t)c->ticks_cap * 12 * sizeof(float),
                                   (size_t)ticks * 12 * sizeof(float), C, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return M17HIP_OK;
}

int m17hip_viterbi(m17hip_ctx* c, const int8_t* soft_host, uint32_t n, int kind, uint8_t* bits_host, int32_t* cost_host)
{
    if (!c || !soft_host || n == 0 || kind < 0 || kind > 3) return M17HIP_EINVAL;
    GUARD(c);
    static const int IN[4] = {488, 296, 420, 402}, OUT[4] = {240, 144, 206, 197};
    const size_t in_b = (size_t)n * IN[kind], out_b = (size_t)n * OUT[kind];
    const size_t o1 = round_up(in_b, 256), o2 = o1 + round_up(out_b, 256);
    HIPCHK(c, c->scratch.grow(o2 + (size_t)n * 4, &c->last_hip));
    char* base = c->scratch;
    HIPCHK(c, hipMemcpyAsync(base, soft_host, in_b, hipMemcpyHostToDevice, c->stream));
    {
        Timed tm(c, KT_DEC);
        hipLaunchKernelGGL(viterbi_kernel, dim3((n + 63) / 64), dim3(64), (122 + 122 + 16) * 64 * 4, c->stream, (const int8_t*)base, n, kind,
                           (uint8_t*)(base + o1), (int32_t*)(base + o2), c->tables);
    }
    HIPCHK(c, hipGetLastError());
    if (bits_host) HIPCHK(c, hipMemcpyAsync(bits_host, base + o1, out_b, hipMemcpyDeviceToHost, c->stream));
    if (cost_host) HIPCHK(c, hipMemcpyAsync(cost_host, base + o2, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return M17HIP_OK;
}

int m17hip_slice_llr(m17hip_ctx* c, const float* sym_host, uint32_t rows, uint32_t n, int8_t* llr_host, float* evm_host)
{
    if (!c || !sym_host || rows == 0 || n == 0) return M17HIP_EINVAL;
    GUARD(c);
    const size_t cnt = (size_t)rows * n;
    const size_t o1 = round_up(cnt * 4, 256), o2 = o1 + round_up(cnt * 2, 256);
    HIPCHK(c, c->scratch.grow(o2 + cnt * 4, &c->last_hip));
    char* b = c->scratch;
    HIPCHK(c, hipMemcpyAsync(b, sym_host, cnt * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(slice_kernel, dim3((rows + 63) / 64), dim3(64), 0, c->stream, (const float*)b, rows, n, (int8_t*)(b + o1),
                       (float*)(b + o2), c->llr_edges);
    HIPCHK(c, hipGetLastError());
    if (llr_host) HIPCHK(c, hipMemcpyAsync(llr_host, b + o1, cnt * 2, hipMemcpyDeviceToHost, c->stream));
    if (evm_host) HIPCHK(c, hipMemcpyAsync(evm_host, b + o2, cnt * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return M17HIP_OK;
}

int m17hip_decode_frames(m17hip_ctx* c, const int8_t* llr368_host, uint32_t n, const uint8_t* sync_type, uint8_t* state_io,
                         uint8_t* lich_io, uint8_t* lsf_io, int8_t* dep401_io, int64_t* cost_io, m17_frame_rec* recs, uint8_t* nrec)
{
    if (!c || !llr368_host || !sync_type || !state_io || !lich_io || !lsf_io || !dep401_io || !cost_io || !recs || !nrec || n == 0)
        return M17HIP_EINVAL;
    GUARD(c);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += round_up(bytes, 256); return o; };
    const size_t o_llr = take((size_t)n * 368), o_st = take(n), o_state = take(n), o_lich = take(n), o_lsf = take((size_t)n * 30),
                 o_dep = take(n), o_cost = take((size_t)n * 8), o_rec = take((size_t)n * 2 * sizeof(FrameRec)), o_nrec = take(n);
    HIPCHK(c, c->scratch.grow(off, &c->last_hip));
    char* b = c->scratch;
    HIPCHK(c, hipMemcpyAsync(b + o_llr, llr368_host, (size_t)n * 368, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b + o_st, sync_type, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b + o_state, state_io, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b + o_lich, lich_io, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b + o_lsf, lsf_io, (size_t)n * 30, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b + o_dep, dep401_io, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b + o_cost, cost_io, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(b + o_rec, 0, (size_t)n * 2 * sizeof(FrameRec), c->stream));
    DecodeFramesParams P{(const int8_t*)(b + o_llr), (const uint8_t*)(b + o_st), (uint8_t*)(b + o_state), (uint8_t*)(b + o_lich),
                         (uint8_t*)(b + o_lsf), (int8_t*)(b + o_dep), (int64_t*)(b + o_cost), (FrameRec*)(b + o_rec),
                         (uint8_t*)(b + o_nrec), n, c->tables, c->overflow};
    {
        Timed tm(c, KT_DEC);
        hipLaunchKernelGGL(decode_frames_kernel, dim3((n + 63) / 64), dim3(64), (92 + 122 + 16) * 64 * 4, c->stream, P);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(state_io, b + o_state, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(lich_io, b + o_lich, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(lsf_io, b + o_lsf, (size_t)n * 30, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(dep401_io, b + o_dep, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cost_io, b + o_cost, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(recs, b + o_rec, (size_t)n * 2 * sizeof(FrameRec), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(nrec, b + o_nrec, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return M17HIP_OK;
}

// TEST HOOK (include/m17hip.h): other matched-filter taps for every form that reads the context's two tap tables.  No kernel knows of it.
int m17hip_set_fir_taps(m17hip_ctx* c, const float* taps149)
{
    if (!c) return M17HIP_EINVAL;
    if (taps149)
        for (int i = 0; i < NTAPS; ++i)
            if (!std::isfinite(taps149[i])) return M17HIP_EINVAL;
    if (c->front_queued) return M17HIP_ESTATE;   // the run m17hip_demod_front began would get its K1 from one table and its K2 / K5 from another
    GUARD(c);
    HIPCHK(c, hipDeviceSynchronize());   // (everything queued has read the tables it was queued with)
    HIPCHK(c, write_fir_taps(c, taps149));
    return M17HIP_OK;
}

// TEST HOOK (include/m17hip.h): the frame decoder in each of its device forms on caller-chosen LLRs.  Everything lives in the operator scratch — the
// context's record sets, demodulator state, diagnostic log and overflow words are not touched.
int m17hip_decode_sequences(m17hip_ctx* c, int form, const int8_t* llr368_host, const uint8_t* sync_type, uint32_t C, uint32_t F, uint32_t rec_cap,
                            uint8_t* state_io, uint8_t* lich_io, uint8_t* lsf_io, int8_t* dep401_io, int64_t* cost_io, m17_frame_rec* recs,
                            uint32_t* nrec, uint32_t* overflow_out, int32_t* cost_trace)
{
    if (!llr368_host || !sync_type || !state_io || !lich_io || !lsf_io || !dep401_io || !cost_io || !recs || !nrec || !overflow_out || !cost_trace)
        return M17HIP_EINVAL;
    if (form < 0 || form > 2 || C == 0 || F == 0 || rec_cap == 0) return M17HIP_EINVAL;
    if (rec_cap > 0x7FFFFFFFu || (uint64_t)C * F > 0x7FFFFFFFull / 368u || (uint64_t)C * rec_cap > 0x7FFFFFFFull / 184u) return M17HIP_EINVAL;   // (a slot is a tag's low 31 bits; sizes within 2 GB)
    // the domain: what the slicer produces and the nibble forms can hold
    const size_t nf = (size_t)C * F;
    for (size_t i = 0; i < nf * 368; ++i)
        if (llr368_host[i] < -7 || llr368_host[i] > 7) return M17HIP_EINVAL;
    for (size_t i = 0; i < nf; ++i)
        if (sync_type[i] > 3) return M17HIP_EINVAL;
    for (uint32_t i = 0; i < C; ++i)
        if (dep401_io[i] < -7 || dep401_io[i] > 7 || state_io[i] > 4 || cost_io[i] < -1 || cost_io[i] > 0x7FFFFFFF) return M17HIP_EINVAL;   // (no tag comes in as a cost)
    if (!c) return M17HIP_EINVAL;
    GUARD(c);
    const bool store = form == 2;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += round_up(bytes, 256); return o; };
    const size_t rec_b = (size_t)C * rec_cap * sizeof(FrameRec);
    const size_t o_llr = take(nf * 368), o_st = take(nf), o_state = take(C), o_lich = take(C), o_lsf = take((size_t)C * 30), o_dep = take(C),
                 o_cost = take((size_t)C * 8), o_rec = take(rec_b), o_nrec = take((size_t)C * 4), o_trace = take(nf * 4), o_ovf = take(4),
                 o_defer = take(store ? (size_t)C * rec_cap * 46 * 4 : 0), o_seq = take(store ? (size_t)C * sizeof(SeqState) : 0),
                 o_diag = take(store ? nf * sizeof(Diag) : 0), o_dcnt = take(store ? (size_t)C * 4 : 0),
                 o_hist = take(store ? (size_t)C * DEFER_HIST_WORDS * 64 * 4 : 0);
    HIPCHK(c, c->scratch.grow(off, &c->last_hip));
    char* b = c->scratch;
    HIPCHK(c, hipMemcpyAsync(b + o_llr, llr368_host, nf * 368, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b + o_st, sync_type, nf, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b + o_state, state_io, C, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b + o_lich, lich_io, C, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b + o_lsf, lsf_io, (size_t)C * 30, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b + o_dep, dep401_io, C, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b + o_cost, cost_io, (size_t)C * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(b + o_rec, 0, rec_b, c->stream));
    HIPCHK(c, hipMemsetAsync(b + o_ovf, 0, 4, c->stream));
    DecodeSeqParams P{};
    P.llr = (const int8_t*)(b + o_llr); P.sync_type = (const uint8_t*)(b + o_st); P.state_io = (uint8_t*)(b + o_state); P.lich_io = (uint8_t*)(b + o_lich);
    P.lsf_io = (uint8_t*)(b + o_lsf); P.dep401_io = (int8_t*)(b + o_dep); P.cost_io = (int64_t*)(b + o_cost); P.recs = (FrameRec*)(b + o_rec);
    P.rec_cap = rec_cap; P.nrec = (uint32_t*)(b + o_nrec); P.cost_trace = (int32_t*)(b + o_trace); P.C = C; P.F = F; P.tables = c->tables;
    P.overflow = (uint32_t*)(b + o_ovf);
    std::vector<Diag> diag;
    std::vector<SeqState> seq;
    const EvParams no_fold{nullptr, 0, nullptr, nullptr, 0, nullptr, C, nullptr, 0u};   // (no EVM operations: neither kernel gets fold blocks)
    if (form == 0) {
        hipLaunchKernelGGL(decode_seq_lane_kernel, dim3((C + 63) / 64), dim3(64), (92 + 122 + 16) * 64 * 4, c->stream, P);
        HIPCHK(c, hipGetLastError());
    } else if (!store) {
        hipLaunchKernelGGL(decode_seq_wave_kernel, dim3(C), dim3(64), 0, c->stream, P);
        HIPCHK(c, hipGetLastError());
    } else {
        // K5's part, then the production kernels as they stand and in production order: settle_tail_kernel (the one or two costs the state still names), then
        // decode_deferred_kernel (every other deferred frame; its tag replacement over the diagnostic rows is what fills cost_trace)
        P.defer = (uint32_t*)(b + o_defer); P.state = (SeqState*)(b + o_seq); P.diag = (Diag*)(b + o_diag);
        HIPCHK(c, hipMemsetAsync(b + o_seq, 0, (size_t)C * sizeof(SeqState), c->stream));
        HIPCHK(c, hipMemsetAsync(b + o_diag, 0, nf * sizeof(Diag), c->stream));
        std::vector<uint32_t> dcnt(C, F);
        HIPCHK(c, hipMemcpyAsync(b + o_dcnt, dcnt.data(), (size_t)C * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (dcnt is a local)
        hipLaunchKernelGGL(decode_seq_wave_kernel, dim3(C), dim3(64), 0, c->stream, P);
        HIPCHK(c, hipGetLastError());
        SettleParams S{P.recs, rec_cap, P.defer, c->tables, P.state, C, no_fold};
        hipLaunchKernelGGL(settle_tail_kernel, dim3(C), dim3(64), SETTLE_LDS_BYTES, c->stream, S);
        HIPCHK(c, hipGetLastError());
        DeferParams D{};
        D.recs = P.recs; D.rec_cap = rec_cap; D.rec_count = P.nrec; D.defer = P.defer; D.hist = (uint32_t*)(b + o_hist); D.tables = c->tables;
        D.state = P.state; D.diag_log = P.diag; D.diag_cap = F; D.diag_count = (const uint32_t*)(b + o_dcnt); D.C = C;
        D.ev = no_fold;
        hipLaunchKernelGGL(decode_deferred_kernel, dim3(defer_blocks(C)), dim3(64 * DEFER_CPB), DEFER_LDS_BYTES, c->stream, D);
        HIPCHK(c, hipGetLastError());
        diag.resize(nf);
        seq.resize(C);
        HIPCHK(c, hipMemcpyAsync(diag.data(), b + o_diag, nf * sizeof(Diag), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(seq.data(), b + o_seq, (size_t)C * sizeof(SeqState), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(state_io, b + o_state, C, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(lich_io, b + o_lich, C, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(lsf_io, b + o_lsf, (size_t)C * 30, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(dep401_io, b + o_dep, C, hipMemcpyDeviceToHost, c->stream));
    if (!store) {
        HIPCHK(c, hipMemcpyAsync(cost_io, b + o_cost, (size_t)C * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(cost_trace, b + o_trace, nf * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(recs, b + o_rec, rec_b, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(nrec, b + o_nrec, (size_t)C * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(overflow_out, b + o_ovf, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (store) {
        for (size_t i = 0; i < nf; ++i) cost_trace[i] = diag[i].viterbi_cost;
        for (uint32_t i = 0; i < C; ++i) {
            const uint32_t v = seq[i].hot.viterbi_cost;
            cost_io[i] = v == 0xFFFFFFFFu ? (int64_t)-1 : (int64_t)v;
        }
    }
    return M17HIP_OK;
}

int m17hip_demod_reset(m17hip_ctx* c)
{
    if (!c) return M17HIP_EINVAL;
    GUARD(c);
    if (c->front_queued) {   // a front end queued by m17hip_demod_front is abandoned: let it drain, its results are not used
        HIPCHK(c, hipStreamSynchronize(c->side));
        HIPCHK(c, hipStreamSynchronize(c->side2));
        HIPCHK(c, hipStreamSynchronize(c->side3));
        c->front_queued = false;
    }
    // the payload work of the runs before (deferred decode, consumers: their state is reset below) is waited for ON the device
    // (payload work that was never asked for goes with the stream it belonged to: the consumers' state is reset below)
    for (auto& rs : c->sets) {
        HIPCHK(c, hipStreamWaitEvent(c->stream, rs.done, 0));   // (never recorded: no wait)
        rs.pending = false;
    }
    c->evm.forget();   // (the EVM state the owed pass would have updated is reset below)
    for (uint32_t ch : c->marks) c->marked[ch] = 0;   // (m17hip_demod_reset_channels: every channel starts over anyway)
    c->marks.clear();
    hipLaunchKernelGGL(seq_reset_kernel, dim3((c->maxC + 63) / 64), dim3(64), 0, c->stream, c->seq_state, c->dcd_state, c->evm.state, c->maxC);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(zero_prefix_xy_kernel<int16_t>, dim3(c->maxC), dim3(64), 0, c->stream, c->now().x.get(), c->xpitch, c->now().y.get(), c->ypitch);
    HIPCHK(c, hipGetLastError());
    // (a context that has seen a float stream: the float pair's prefix and the float histories as well — whatever format the slab pair holds NOW: the
    //  next stream may be of either)
    if (c->fslab[c->slot].x) {
        hipLaunchKernelGGL((zero_prefix_kernel<float, XPRE>), dim3(c->maxC), dim3(64), 0, c->stream, c->fslab[c->slot].x.get(), c->xpitch);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemsetAsync(c->hist_f, 0, c->hist_f.size() * sizeof(float), c->stream));
    }
    if (int r = iq_fresh_feed(c, nullptr, 0)) return r;   // (a context that has seen IQ input: every channel's feed starts over)
    c->wtx.count = c->wtx.first; c->wtx.fresh = true;   // (a generator's feed likewise: count and carries as m17hip_synth_wide_config left them)
    HIPCHK(c, hipMemset2DAsync(c->now().h, c->ypitch * sizeof(float), 0, YPRE * sizeof(float), c->maxC, c->stream));
    if (int r = c->bert.reset(c, c->stream)) return r;
    if (int r = c->packets.reset(c, c->stream)) return r;
    if (int r = c->voice.reset(c, c->stream)) return r;
    for (auto& rs : c->sets) {
        if (rs.rec_count) HIPCHK(c, hipMemsetAsync(rs.rec_count, 0, (size_t)c->maxC * 4, c->stream));
        rs.valid = false;
    }
    HIPCHK(c, hipMemsetAsync(c->overflow, 0, 32, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_mark, c->stream));   // the front end of a staged run starts on its own streams: not before this
    HIPCHK(c, hipStreamWaitEvent(c->pay(), c->ev_mark, 0));   // (nor anything a fetch queues on the payload stream)
    c->pos = 0;
    c->have_run = false;
    c->inplace_after_run = false;
    c->sel_back = 0;
    c->stream_fmt = 0;   // the next input chooses the stream's sample format again (what the slabs hold keeps its own)
    return M17HIP_OK;
}

// the marks of m17hip_demod_reset_channels (and of a polarity change of a channel that has run): every entry < maxC
static void mark_channels(m17hip_ctx* c, const uint32_t* channels, uint32_t n)
{
    if (c->marked.empty()) c->marked.assign(c->maxC, 0);
    for (uint32_t i = 0; i < n; ++i)
        if (!c->marked[channels[i]]) { c->marked[channels[i]] = 1; c->marks.push_back(channels[i]); }
}

int m17hip_demod_reset_channels(m17hip_ctx* c, const uint32_t* channels, uint32_t n)
{
    if (!c || (n && !channels)) return M17HIP_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
        if (channels[i] >= c->maxC) return M17HIP_EINVAL;   // (before anything is marked)
    if (c->front_queued) return M17HIP_ESTATE;   // the run m17hip_demod_front began has taken its marks
    if (n == 0) return M17HIP_OK;
    // The carrier-detect tick grid is the context's: K3's table rows, K2's replay, K5 and the gate forecast all find a tick as position / 192.  A fresh
    // demodulator's update points fall on ITS tick ends, so its stream can only begin where a tick of the context does.
    if (c->pos % TICK != 0) return M17HIP_ESTATE;
    if (c->iq_carry) {   // (a context that has seen IQ input: the listed channels' feeds start over with the next IQ block uploaded)
        GUARD(c);
        if (int r = iq_fresh_feed(c, channels, n)) return r;
    }
    mark_channels(c, channels, n);
    return M17HIP_OK;
}

int m17hip_set_channel_polarity(m17hip_ctx* c, const uint8_t* invert, uint32_t n)
{
    if (!c || n > c->maxC || (invert == nullptr) != (n == 0)) return M17HIP_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
        if (invert[i] > 1) return M17HIP_EINVAL;   // (before anything changes)
    if (c->front_queued) return M17HIP_ESTATE;   // the run m17hip_demod_front began has its table
    // the entries that change: [0, n) against the call's values, or every 1 when the table is cleared
    std::vector<uint32_t> changed;
    const uint32_t span = c->pol_host.empty() ? 0u : (n ? n : c->maxC);
    for (uint32_t i = 0; i < span; ++i)
        if (c->pol_host[i] != (n ? invert[i] : 0)) changed.push_back(i);
    if (c->pol_host.empty())
        for (uint32_t i = 0; i < n; ++i)
            if (invert[i]) changed.push_back(i);
    if (changed.empty()) return M17HIP_OK;
    // A channel that has run carries state formed under its old polarity (the raw input prefix, the sliding DFT, the demodulator): it starts over, as
    // m17hip_demod_reset_channels starts it — and where that call can (the tick grid is the context's).  The channels of a continued stream are [0, lastC).
    std::vector<uint32_t> restart;
    if (c->have_run)
        for (uint32_t ch : changed)
            if (ch < c->lastC) restart.push_back(ch);
    if (!restart.empty() && c->pos % TICK != 0) return M17HIP_ESTATE;
    if (c->pol_host.empty()) c->pol_host.assign(c->maxC, 0);
    for (uint32_t ch : changed) { c->pol_host[ch] ^= 1u; if (c->pol_host[ch]) ++c->pol_ones; else --c->pol_ones; }
    c->pol_dirty = true;
    if (!restart.empty()) mark_channels(c, restart.data(), (uint32_t)restart.size());
    return M17HIP_OK;
}

namespace {

// How a run of T samples is cut into segments (tuning knobs 3, 4, 33): segment k covers [t0(k), t0(k + 1)).  Equal ones of seg_len samples;
// optionally a short first one (key 4), or a RAMP (key 33): segments of r, 2 r, 4 r, ... samples until seg_len is reached.  The ramp is for
// where channels leave the limit-filter replay — at the start of a transmission, while sync is being acquired: a channel that leaves it in
// segment k carries the filter itself to the end of segment k + 1, so what a drop costs the launches it falls into is twice the segment's length.
constexpr uint32_t AUTO_RAMP = 9600;   // (2400 ... 24 000 measured: NOTES 6.5)
static std::vector<uint32_t> segment_bounds(const m17hip_ctx* c, uint32_t T, uint32_t ramp)   // b[k] = first sample of segment k; the last entry = T
{
    const uint32_t seg_len = (!c->profile && c->seg_len) ? c->seg_len : T;
    std::vector<uint32_t> b(1, 0u);
    uint32_t pos = 0;
    if (seg_len < T && !c->profile) {
        if (ramp && ramp < seg_len) {
            for (uint32_t len = ramp; len < seg_len && pos + len < T; len *= 2) { pos += len; b.push_back(pos); }
        } else if (c->seg0_len && c->seg0_len < seg_len) {
            pos = c->seg0_len; b.push_back(pos);
        }
    }
    while (pos + seg_len < T) { pos += seg_len; b.push_back(pos); }
    // Segment starts are multiples of eight samples: the matched filter loads its input sixteen bytes at a time and stores float4s from a
    // segment's first sample on (an odd start made those accesses misaligned — the hardware splits them, C++ calls it undefined)
    for (size_t k = 1; k < b.size(); ++k) b[k] &= ~7u;
    b.erase(std::unique(b.begin(), b.end()), b.end());
    b.push_back(T);
    return b;
}

// The one place where a run is decided.  `kind`: on input uploaded in place; on staged input, begun by the run call or — a continued stream — by m17hip_demod_front.
// Is the run the only thing in flight on the device?  (What a context can know of it: runs_overlap — which counts what it is asked: once per run at most, and only
// where the answer is used.)  Then a step lasts what its chain of launches lasts: K3 and K1 take their latency forms, and a run in place starts with a ramp of short
// segments (key 33) — one batch at a time 23.65 -> 22.8 ms per 4096 x 480 000; with batches in flight or a continued stream both cost more than they save.
enum RunKind { RUN_IN_PLACE, RUN_STAGED, RUN_STAGED_FRONT };
static RunPlan plan_run(m17hip_ctx* c, uint32_t C, uint32_t T, uint32_t flags, RunKind kind)
{
    RunPlan p;
    p.C = C; p.T = T; p.flags = p.kflags = flags; p.staged = kind != RUN_IN_PLACE; p.from_front = kind == RUN_STAGED_FRONT;
    // kind              runs_overlap is asked                    ramp where key 33 = -1
    // in place          always                                   AUTO_RAMP when chain-bound
    // staged (run)      where key 10 = -1 leaves K3 to the run   none: as a rule a continued stream, where the extra launches of a ramp
    // staged (front)    never: a continued stream, chain-bound   none  cost the chain more than the shorter drops save
    const bool ask = kind == RUN_IN_PLACE || (kind == RUN_STAGED && c->dcd_form < 0);
    const bool chain_bound = !ask || !runs_overlap(c);   // what key 10 = -1 goes by
    p.ramp = c->seg_ramp > 0 ? (uint32_t)c->seg_ramp : (c->seg_ramp < 0 && kind == RUN_IN_PLACE && chain_bound) ? AUTO_RAMP : 0u;
    p.b = segment_bounds(c, T, p.ramp); p.nseg = (uint32_t)p.b.size() - 1u;
    p.front_segs = std::min(c->front_ahead ? c->front_ahead : p.nseg, p.nseg);
    // Gate-aware (m17hip_tune key 26)?  -1: yes when more than a quarter of the channel-segments of the last fetched run ended with the carrier
    // off (K5 counts them: overflow[3], read with every fetch) — an always-on load keeps K1 running ahead freely.
    // Needs at least three segments and the default front-end schedule.
    const bool want = c->gate_aware == 1 || (c->gate_aware < 0 && c->chan_segs_prev && 4ull * c->off_segs_prev > (uint64_t)c->chan_segs_prev);
    p.gate_run = want && p.nseg >= 3u && !c->front_ahead && !c->profile;
    p.fir_latency = c->dcd_form < 0 ? chain_bound : c->dcd_form == 1;
    // A gate-aware run is a run on mostly idle channels: K1 skips most of its work, K5's waves jump from update point to update point — what is left of the step
    // is K3's chain, which sees every sample whatever the gate does.  Its latency form then (four waves per 32 channels, 1.1-1.9 ms per launch against
    // 2.2-3.7): the wave slots it takes are free on such input.
    p.dcd_latency = p.fir_latency || (p.gate_run && c->dcd_form < 0);
    return p;
}

// K3 and K1 of segment k of the run being queued (slab pair c->slot), on the two side streams.
// The front end of segment k may be held back until K5 of segment k - front_ahead is done (tuning knob 5), to spread it over
// the step; measured, letting it run ahead freely is faster (K3 is a latency chain of 1.7 ms per segment: held back, it is
// what K5 ends up waiting for).
// (A gate-aware run queues K1 of segment k >= 2 later, behind K5 of segment k - 2: launch_gated_fir.)
static int launch_front_seg(m17hip_ctx* c, const RunPlan& p, uint32_t k)
{
    if (k >= p.nseg) return M17HIP_OK;
    auto& seg = c->now().seg;
    const uint32_t ahead = p.front_segs, t0 = p.t0(k), len = p.t0(k + 1) - t0;
    if (k >= ahead) {   // (tuning knob 5 is set)
        HIPCHK(c, hipStreamWaitEvent(c->side, seg[k - ahead].seq, 0));
        HIPCHK(c, hipStreamWaitEvent(c->side2, seg[k - ahead].seq, 0));
    }
    if (k == 1) HIPCHK(c, hipStreamWaitEvent(c->side, seg[0].fir, 0));   // segment 0's front end first: K2/K5 wait for it
    if (int r = launch_dcd(c, p.C, len, p.kflags, c->pos, p.dcd_latency, c->side, t0, p.pol)) return r;
    HIPCHK(c, hipEventRecord(seg[k].dcd, c->side));
    if (p.gate_run && k >= 2u) return M17HIP_OK;
    if (int r = launch_fir(c, p.C, len, p.kflags, p.fir_latency, c->side2, t0, nullptr, p.pol)) return r;
    HIPCHK(c, hipEventRecord(seg[k].fir, c->side2));
    return M17HIP_OK;
}

// The whole front end of a run as far as it can be queued at once: K3 and K1 of every segment — or, for a gate-aware run, K3 of every segment
// and K1 of the first two (K1 of segment k >= 2 follows K5 of segment k - 2 and its forecast: launch_gated_fir, from the K5 loop).
// A run in place: behind what the main stream holds so far (its input); a staged one is ordered by begin_staged.
static int launch_front_all(m17hip_ctx* c, const RunPlan& p)
{
    HIPCHK(c, c->now().ensure_seg_events(p.nseg));
    if (!p.staged) {
        HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
        HIPCHK(c, hipStreamWaitEvent(c->side2, c->ev_fork, 0));
    }
    for (uint32_t k = 0; k < p.front_segs; ++k)
        if (int r = launch_front_seg(c, p, k)) return r;
    return M17HIP_OK;
}

// Gate-aware run, after K5 of segment k has been queued (ev_seq[k] recorded): the forecast for segment k + 2 from K5's gate state at the
// end of segment k and the table rows of segments k + 1 and k + 2, then K1 of segment k + 2 over what the carrier can be on for.
static int launch_gated_fir(m17hip_ctx* c, const RunPlan& p, uint32_t k)
{
    if (k + 2u >= p.nseg) return M17HIP_OK;
    auto& seg = c->now().seg;
    const uint32_t C = p.C, t1 = p.t0(k + 1u), t2 = p.t0(k + 2u), t3 = p.t0(k + 3u);
    HIPCHK(c, hipStreamWaitEvent(c->side2, seg[k].seq, 0));
    HIPCHK(c, hipStreamWaitEvent(c->side2, seg[k + 2u].dcd, 0));
    hipLaunchKernelGGL(gate_forecast_kernel, dim3((C + 63) / 64), dim3(64), 0, c->side2, by_parity(c->truth, k, c->maxC), c->now().dcd, c->ticks_cap,
                       (uint64_t)(c->pos / TICK), (uint64_t)(c->pos + t1), t2 - t1, t3 - t1, c->first_needed, C);
    HIPCHK(c, hipGetLastError());
    if (int r = launch_fir(c, C, t3 - t2, p.kflags, p.fir_latency, c->side2, t2, c->first_needed, p.pol)) return r;
    HIPCHK(c, hipEventRecord(seg[k + 2u].fir, c->side2));
    return M17HIP_OK;
}

// A fold pass of the deferred EVM (EvmFold) as a kernel gets it; and none — what a kernel that can take a pass along is given when there is nothing to fold.
static EvParams ev_fold(const m17hip_ctx* c, const EvmFold::Pass& f, EvLast last) { return EvParams{f.ops, c->evm.pitch(), c->evm.state, c->diag.entries(), c->diag.room, c->seq_state, f.C, f.upto, last}; }
static EvParams ev_no_fold(uint32_t C) { return EvParams{nullptr, 0, nullptr, nullptr, 0, nullptr, C, nullptr, 0u}; }

// The parameter blocks of K2 and K5 (GateParams::x, SeqParams::x: filled in launch_gate_seg and seq_params, below) name the input rows as const void*;
// limit_track_kernel<XT> and demod_wave_kernel<XT, ...> read them as rows of XT.  The kernel a block is launched with comes from the same typed pointer
// the block is filled from (gate_kernel, wave_kernel), so the two cannot disagree.

// One launch of K2 over segment k of the run whose slabs the context names: the whole segment from K5's state (first segment), ahead of
// K5 from K2's own state, or the redo of the channels K5 flagged in the previous segment.
static int launch_gate_seg(m17hip_ctx* c, const RunPlan& p, uint32_t k, hipStream_t st, bool ahead, bool redo, bool redo_stores = false)
{
    if (k == 0 && p.gate0_queued) {   // m17hip_demod_front has queued this one on the replay stream, behind the prefix copies
        HIPCHK(c, hipStreamWaitEvent(st, c->now().seg[0].gate, 0));
        return M17HIP_OK;
    }
    const uint32_t C = p.C, t0 = p.t0(k), len = p.t0(k + 1) - t0;
    TimedK tm(c, KT_GATE);
    GateParams G{};
    G.xpitch = c->xpitch; G.y = c->now().y + t0; G.ypitch = c->ypitch; G.h = c->now().h + t0;
    G.dcd_table = c->now().dcd; G.ticks_cap = c->ticks_cap; G.state = c->seq_state;
    G.final_h = by_parity(c->final_h, k, c->maxC, 4);
    G.chain_in = ahead ? c->gate_exp : nullptr; G.chain_out = c->gate_exp;
    G.only = redo ? by_parity(c->dropped, k - 1u, c->maxC) : nullptr;   // (flags by segment parity)
    G.bnd = redo ? by_parity(c->bnd, k, c->maxC) : nullptr;   // (written by K5 of segment k - 1)
    G.taps = c->taps; G.C = C; G.T = len; G.pos0 = c->pos + t0; G.tick_row0 = c->pos / TICK; G.flags = p.kflags | ((redo && !redo_stores) ? 2u : 0u); G.pol = p.pol;
    G.nblk = (C + GT_CPW - 1) / GT_CPW;
    uint32_t fold_blocks = 0;
    if (ahead && k >= 2 && c->defer_evm && c->evm.ops()) {   // (K5 of segment k - 2 is through: its EVM operations ride along, sixteen channels per block)
        G.ev = ev_fold(c, c->evm.ahead(k, C), EV_MORE);
        fold_blocks = ev_fold_blocks(C);
    }
    // The LAST pass of the run before (its buffer is not this run's): beside K5 of this run's first segment, with the replay that runs ahead for the
    // second one — or, for a run of one segment, with this replay, which K5 waits for (that K5 is the one that moves the end-of-run cursors on)
    if (!redo && c->evm.owed() && ((p.nseg >= 2 && ahead && k == 1) || (p.nseg < 2 && k == 0))) {
        const EvmFold::Pass f = c->evm.take();
        G.ev = ev_fold(c, f, k == 0 ? EV_SETTLES : EV_BESIDE_K5);   // (in front of segment 0, which K5 waits for: settled; beside the replay ahead: not)
        fold_blocks = f.blocks();
    }
    with_x(c, c->slot, [&](auto* x) {
        G.x = x + t0;
        if constexpr (std::is_same<decltype(x), float*>::value) { G.hist_f = c->hist_f; G.bnd_hist_f = redo ? by_parity(c->bnd_hist_f, k, c->maxC, HISTF_PITCH) : nullptr; }
        tm.launch(gate_kernel(x), dim3(G.nblk + fold_blocks), dim3(64), GT_LDS_FLOATS * sizeof(float), st, G);
    });
    HIPCHK(c, hipGetLastError());
    return M17HIP_OK;
}

// ---- m17hip_demod_reset_channels: the marked channels begin the run being queued with fresh demodulators ---------------------------------------
// The marks become a list on the device (n entries; 0: nothing is marked — the caller then queues nothing for them).
// `first`: the stream whose kernel reads the list first (TurnTable::publish).
// The marks themselves stay until the run's front end is queued (commit_marks): a call that fails before that leaves them for the caller's next attempt.
static int take_marks(m17hip_ctx* c, uint32_t& n, hipStream_t first)
{
    n = (uint32_t)c->marks.size();
    if (!n) return M17HIP_OK;
    uint32_t* staging;
    HIPCHK(c, c->reset_list.begin_write(c->maxC, &staging));
    std::memcpy(staging, c->marks.data(), (size_t)n * 4);
    HIPCHK(c, c->reset_list.publish(n, first));
    return M17HIP_OK;
}
static void commit_marks(m17hip_ctx* c)
{
    for (uint32_t ch : c->marks) c->marked[ch] = 0;
    c->marks.clear();
}
// The FRONT-END state of the listed channels — `x`: the input prefix (K1's FIR history, K3's 120-sample delay), on a stream that has carried the previous
// input's tail into the prefixes; `dcd`: the sliding-DFT state, on a stream that is behind the previous run's K3 — before K1 / K3 of the run start.
static int reset_marked_front(m17hip_ctx* c, uint32_t n, hipStream_t st, Reader which, bool x, bool dcd)
{
    HIPCHK(c, c->reset_list.before_read(st));
    with_x(c, c->slot, [&](auto* rows) {
        hipLaunchKernelGGL(front_reset_list_kernel<std::remove_pointer_t<decltype(rows)>>, dim3(n), dim3(64), 0, st, c->reset_list.dev(), n, x ? rows : nullptr, c->xpitch,
                           dcd ? c->dcd_state.get() : (DcdState*)nullptr);
    });
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, c->reset_list.after_read(which, st));
    return M17HIP_OK;
}

// A run is about to read the input slab pair `slot` holds: its format must be the stream's (it becomes the stream's where a reset has freed the
// choice since the input was written), and the kernels a tuning key selects must exist for it — the tools-only instantiations of the
// sequential kernel (keys 1, 19) and round 4's matched filter (key 11 = 0) read int16 rows only: refused, never launched on float memory.
static int run_format_check(m17hip_ctx* c, int slot)
{
    const int fmt = c->slab_fmt[slot];
    if (c->stream_fmt && fmt && fmt != c->stream_fmt) return M17HIP_ESTATE;
    if (fmt == M17HIP_FORMAT_F32 && (c->profile || c->wave_times || c->fir_form == 0)) return M17HIP_ESTATE;
    if (fmt) c->stream_fmt = fmt;
    return M17HIP_OK;
}

// A staged run begins: the slab pairs swap, the 152-sample tail of the previous input is carried into the new slab's prefix, and the
// front end (K1, K3: nothing in them depends on the outcome of the run before) is queued on the side streams — NOT ordered behind
// the main stream, where K2 / K5 of the previous run may still have a long way to go.  `p`: the run, decided here.
static int begin_staged(m17hip_ctx* c, RunPlan& p, uint32_t C, uint32_t T, uint32_t flags, RunKind kind)
{
    if (C != c->stagedC || T != c->stagedT) return M17HIP_EINVAL;
    if (c->have_run && C != c->lastC) return M17HIP_EINVAL;  // a continued stream keeps its channel count
    if (int r = run_format_check(c, c->slot ^ 1)) return r;
    c->slot ^= 1;   // (the staged input's pair becomes now(), the previous run's other())
    c->staged = false; c->uploaded = true;
    c->carryT = c->have_run ? c->runT : 0;
    // the new slab's prefix, behind the staged copy on the copy stream; the slab pair itself is free since now().end (the copy
    // stream waited for it when the input was staged — m17hip_input_alternate stages without a copy, so wait here as well)
    HIPCHK(c, c->now().wait_free(c->copy));
    const int carried = with_x(c, c->slot, [&](auto* x) -> int {
        using XT = std::remove_pointer_t<decltype(x)>;
        const XT* xprev = slab_x<XT>(c, c->slot ^ 1);   // the previous run's rows: of the stream's format, as these are
        if (c->carryT && !xprev) return M17HIP_ESTATE;   // (cannot be: a continued stream has run on a slab of its format)
        if (c->carryT >= (uint32_t)XPRE && !c->inplace_after_run)   // the tail of the previous input, where it lies (that slab is only read while its run is in flight)
            hipLaunchKernelGGL((copy_tail_kernel<XT, XPRE>), dim3(C), dim3(64), 0, c->copy, xprev, x, c->xpitch, c->carryT);
        else if (c->carryT) {
            // a run shorter than the prefix: its tail reaches into its own prefix, which its last kernel rewrites — wait for that, and copy the prefix
            // (or its data region was overwritten in place since: the tail its last kernel carried into its prefix)
            HIPCHK(c, hipStreamWaitEvent(c->copy, c->other().end, 0));
            hipLaunchKernelGGL((copy_prefix_kernel<XT, XPRE>), dim3(C), dim3(64), 0, c->copy, xprev, x, c->xpitch);
        } else HIPCHK(c, hipMemset2DAsync(x, c->xpitch * sizeof(XT), 0, XPRE * sizeof(XT), C, c->copy));   // a fresh stream
        HIPCHK(c, hipGetLastError());
        return M17HIP_OK;
    });
    if (carried) return carried;
    uint32_t n_reset = 0;   // (m17hip_demod_reset_channels: the marked channels' input prefixes, behind the tail copy)
    if (!c->marks.empty()) {
        if (int r = take_marks(c, n_reset, c->copy)) return r;
        if (int r = reset_marked_front(c, n_reset, c->copy, RD_FRONT, true, false)) return r;
    }
    uint32_t kflags; const uint32_t* pol;   // (m17hip_set_channel_polarity: a changed table goes up behind the staged input, in front of everything that reads it)
    if (int r = resolve_polarity(c, C, flags, c->copy, kflags, pol)) return r;
    HIPCHK(c, hipEventRecord(c->ev_in_ready, c->copy));
    for (hipStream_t st : {c->side, c->side2}) {
        HIPCHK(c, hipStreamWaitEvent(st, c->ev_in_ready, 0));
        HIPCHK(c, hipStreamWaitEvent(st, c->ev_mark, 0));
    }
    if (n_reset) {   // (... and their sliding-DFT state, on K3's stream: behind the previous run's K3, in front of this run's)
        if (int r = reset_marked_front(c, n_reset, c->side, RD_DCD, false, true)) return r;
    }
    if (c->front_k1_after && c->have_run && c->last_nseg) {   // K1 out of the way of the previous run's first (heaviest) K5 launches
        const uint32_t j = std::min(c->front_k1_after, c->last_nseg) - 1u;
        HIPCHK(c, hipStreamWaitEvent(c->side2, c->other().seg[j].seq, 0));
    }
    p = plan_run(c, C, T, flags, kind);
    p.n_reset = n_reset; p.kflags = kflags; p.pol = pol;
    if (int r = launch_front_all(c, p)) return r;
    if (n_reset) commit_marks(c);
    return M17HIP_OK;
}

}  // namespace

// The latest run's last EVM fold pass on the main stream (behind that run), if nothing has taken it along yet.
static int flush_fold(m17hip_ctx* c)
{
    const EvmFold::Pass f = c->evm.take();
    if (!f.ops) return M17HIP_OK;
    hipLaunchKernelGGL(evm_deferred_kernel, dim3(f.blocks()), dim3(64), 0, c->stream, ev_fold(c, f, EV_SETTLES));
    HIPCHK(c, hipGetLastError());
    return M17HIP_OK;
}

// ---- the payload consumers and the diagnostic log (BertStats, Packets, Voice, DiagLog, above) ----
int BertStats::reset(m17hip_ctx* c, hipStream_t st)
{
    hipLaunchKernelGGL(bert_reset_kernel, dim3((c->maxC + 63) / 64), dim3(64), 0, st, state, c->maxC);
    HIPCHK(c, hipGetLastError());
    return M17HIP_OK;
}

int Packets::fresh(m17hip_ctx* c, hipStream_t st)
{
    hipLaunchKernelGGL(packet_reset_kernel, dim3((c->maxC + 63) / 64), dim3(64), 0, st, state_, c->maxC);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemsetAsync(count_, 0, 8, st));
    return M17HIP_OK;
}
int Packets::reset(m17hip_ctx* c, hipStream_t st) { return on() ? fresh(c, st) : M17HIP_OK; }   // (`fed` stays: see its comment)
int Packets::configure(m17hip_ctx* c, uint32_t value)
{
    recs_[0].release(&c->last_hip); recs_[1].release(&c->last_hip); room = 0; fed = false;
    if (value == 0) return M17HIP_OK;
    if (!state_) {   // (the state and the counts survive a change of the room)
        HIPCHK(c, state_.alloc(c->maxC));
        HIPCHK(c, count_.alloc(2));
    }
    HIPCHK(c, recs_[0].alloc(value));
    HIPCHK(c, recs_[1].alloc(value));
    room = value;   // (a failed allocation has left the consumer off)
    return fresh(c, c->stream);
}
int Packets::consume(m17hip_ctx* c, hipStream_t ps, const FrameRec* recs, uint32_t rec_cap, const uint32_t* rec_count, uint32_t C, int set)
{
    HIPCHK(c, hipMemsetAsync(count_.get() + set, 0, 4, ps));
    hipLaunchKernelGGL(packet_asm_kernel, dim3((C + 63) / 64), dim3(64), 0, ps, recs, rec_cap, rec_count, state_, C, recs_[set], room, count_.get() + set, c->channel_base);
    HIPCHK(c, hipGetLastError());
    return M17HIP_OK;
}

int Voice::fresh(m17hip_ctx* c, hipStream_t st)
{
    hipLaunchKernelGGL(voice_reset_kernel, dim3((c->maxC + 63) / 64), dim3(64), 0, st, state_, c->maxC);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemsetAsync(counts_, 0, (size_t)2 * c->maxC * 4, st));
    HIPCHK(c, hipMemsetAsync(call_counts_, 0, (size_t)2 * c->maxC * 4, st));
    return M17HIP_OK;
}
int Voice::reset(m17hip_ctx* c, hipStream_t st)
{
    if (!on()) return M17HIP_OK;
    if (int r = fresh(c, st)) return r;
    fed = false;
    return M17HIP_OK;
}
int Voice::configure(m17hip_ctx* c, uint32_t value)
{
    for (int i = 0; i < 2; ++i) {
        audio_[i].release(&c->last_hip); marks_[i].release(&c->last_hip); calls_[i].release(&c->last_hip);
        rows[i] = 0;
    }
    room = 0; call_room = 0; fed = false;
    if (value == 0) return M17HIP_OK;
    const uint32_t calls = M17HIP_CALLS_PER_CHANNEL(value);
    maxC_ = c->maxC;
    if (!state_) {   // (the state and the counts survive a change of the room)
        HIPCHK(c, state_.alloc(maxC_));
        HIPCHK(c, counts_.alloc((size_t)2 * maxC_));
        HIPCHK(c, call_counts_.alloc((size_t)2 * maxC_));
    }
    for (int i = 0; i < 2; ++i) {
        HIPCHK(c, audio_[i].alloc((size_t)maxC_ * value * 16));
        HIPCHK(c, marks_[i].alloc((size_t)maxC_ * value));
        HIPCHK(c, calls_[i].alloc((size_t)maxC_ * calls));
    }
    if (int r = fresh(c, c->stream)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (the payload stream, where the consumer works, may be another one)
    room = value; call_room = calls;   // (a step that failed has left the consumer off)
    return M17HIP_OK;
}
// (the payload stream: the state goes from run to run)
int Voice::consume(m17hip_ctx* c, hipStream_t ps, const FrameRec* recs, uint32_t rec_cap, const uint32_t* rec_count, uint32_t C, int set)
{
    TimedK tm(c, KT_VOICE);
    tm.launch(voice_log_kernel, dim3((C + VOICE_CPB - 1) / VOICE_CPB), dim3(64 * VOICE_CPB), 0, ps, params(set, recs, rec_cap, rec_count, C, c->channel_base));
    rows[set] = C;
    HIPCHK(c, hipGetLastError());
    return M17HIP_OK;
}

int DiagLog::configure(m17hip_ctx* c, uint32_t value)
{
    log_.release(&c->last_hip); room = 0;
    if (value == 0) return M17HIP_OK;
    if (!count_) HIPCHK(c, count_.alloc(c->maxC));
    HIPCHK(c, hipMemsetAsync(count_, 0, (size_t)c->maxC * 4, c->stream));   // (on the stream the kernels that count into it run on)
    HIPCHK(c, log_.alloc((size_t)c->maxC * (size_t)value));
    room = value;
    return M17HIP_OK;
}

// Queue the payload work of the runs whose results nobody has asked for yet, in run order, on the payload stream: the frames K5 left to
// decode_deferred_kernel (one lane per frame), then the consumers (their state goes from run to run), then `done`.
// `selected_only`: up to the run the fetch family names (m17hip_frames_select) — a fetch of run k must not queue the work of run k + 1, whose
// chain may have just begun: everything behind it on the payload stream would wait for that run's end.
// `older_only`: the run before the latest alone (its record set is about to be written again).
// `fold_beside_decode`: the latest run's pending last fold pass rides its deferred decode (m17hip_demod_run, where that is queued behind the run at once).
static int flush_payload(m17hip_ctx* c, bool selected_only = false, bool older_only = false, bool fold_beside_decode = false)
{
    for (int j = 0; j < 2; ++j) {
        const int i = j == 0 ? (c->cur ^ 1) : c->cur;   // the older run first
        if (j == 1 && (older_only || (selected_only && (c->sel_back & 1u)))) break;
        m17hip_ctx::RecSet& rs = c->sets[i];
        if (!rs.valid || !rs.pending) continue;
        const hipStream_t ps = c->pay();
        HIPCHK(c, hipStreamWaitEvent(ps, c->sets[i ^ 1].done, 0));   // (the run before it, whichever stream did its work; never recorded: no wait)
        HIPCHK(c, hipStreamWaitEvent(ps, rs.chain, 0));
        const uint32_t C = rs.C;
        if (rs.defer_llr && c->defer_hist) {   // (frames are deferred only while both stores exist: m17hip_tune key 15)
            DeferParams D{};
            D.recs = rs.recs; D.rec_cap = rs.rec_cap; D.rec_count = rs.rec_count; D.defer = rs.defer_llr; D.hist = c->defer_hist; D.tables = c->tables;
            D.state = c->seq_state; D.diag_log = c->diag.entries(); D.diag_cap = c->diag.room; D.diag_count = c->diag.count(); D.C = C;
            D.ev = ev_no_fold(C);
            uint32_t fold_blocks = 0;
            if (fold_beside_decode && c->evm.owed() && i == c->cur) {   // (the latest run's last fold pass, beside its decode on the main stream)
                const EvmFold::Pass f = c->evm.take();
                D.ev = ev_fold(c, f, EV_SETTLES);
                fold_blocks = f.blocks();
            }
            TimedK tm(c, KT_DEC);
            tm.launch(decode_deferred_kernel, dim3(defer_blocks(C) + fold_blocks), dim3(64 * DEFER_CPB), DEFER_LDS_BYTES, ps, D);
            HIPCHK(c, hipGetLastError());
        }
        // the consumers that were on when the run was made (and still are): PRBS9 statistics over its BERT records, packet reassembly over its packet
        // records, codec2 payload planes and the call log over its stream records (behind their deferred decode)
        if (rs.bert && c->bert.state) {
            hipLaunchKernelGGL(bert_stats_kernel, dim3((C + 63) / 64), dim3(64), 0, ps, rs.recs, rs.rec_cap, rs.rec_count, c->bert.state, C);
            HIPCHK(c, hipGetLastError());
        }
        if (rs.pkt && c->packets.on())
            if (int r = c->packets.consume(c, ps, rs.recs, rs.rec_cap, rs.rec_count, C, i)) return r;
        if (rs.voice && c->voice.on())
            if (int r = c->voice.consume(c, ps, rs.recs, rs.rec_cap, rs.rec_count, C, i)) return r;
        HIPCHK(c, hipEventRecord(rs.done, ps));
        rs.pending = false;
    }
    return M17HIP_OK;
}

// A fetch reads what a run and its payload work wrote, on the payload stream of NOW — which need not be the stream that work went to: a
// context that ran in place made it on the main stream, its first staged input moves the payload stream to the copy stream, and
// m17hip_set_stream moves the main one.  So the fetch orders the payload stream behind the run itself: its `done`, or its `chain` while
// its payload work is still to be queued (flush_payload queues it behind `chain`).  (An event that was never recorded: no wait.)
// The two forms below are the whole rule; whatever reads a consumer's state or a run's store on the payload stream calls one of them first.
static int pay_after(m17hip_ctx* c, const m17hip_ctx::RecSet& rs)
{
    HIPCHK(c, hipStreamWaitEvent(c->pay(), rs.pending ? rs.chain : rs.done, 0));
    return M17HIP_OK;
}
// Behind EVERY run: for what reads or changes a consumer's state, which every run's consumer adds to.  The payload work of both runs is queued first.
static int behind_all_runs(m17hip_ctx* c)
{
    if (int r = flush_payload(c)) return r;
    for (const auto& rs : c->sets)
        if (rs.valid)
            if (int r = pay_after(c, rs)) return r;
    return M17HIP_OK;
}
// Behind the SELECTED run (m17hip_frames_select; `set`: its record set and its stores), for what reads that run's results: its payload work is queued
// first, the later run's is not.  M17HIP_ESTATE when the run before the latest is named and its records are not there; an invalid LATEST set passes and
// is waited for nothing (a store that a feed has filled).
static int behind_selected(m17hip_ctx* c, int& set)
{
    set = c->cur ^ (int)(c->sel_back & 1u);
    if (c->sel_back && !c->sets[set].valid) return M17HIP_ESTATE;
    if (int r = flush_payload(c, true)) return r;
    return c->sets[set].valid ? pay_after(c, c->sets[set]) : M17HIP_OK;
}
// The payload stream and the main stream idle, the payload work that was owed made (m17hip_tune: in front of a change of what that work uses);
// `fold_first`: the latest run's last EVM fold pass as well (it writes the diagnostic log)
static int quiesce_payload(m17hip_ctx* c, bool fold_first)
{
    if (fold_first) if (int r = flush_fold(c)) return r;
    if (int r = flush_payload(c)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->pay()));
    return M17HIP_OK;
}

// BASELINE configs[1] as ONE call: matched filter, limit filter and the four correlations of `samples` samples per channel, pipelined in time.
// The limit filter is one dependent chain per channel over the whole run (12 ns per sample) and is what the call lasts; the matched filter
// (K1) of piece k + 1 and the correlations of piece k run beside the chain's piece k on two side streams, the chain's state (four history
// values per channel) carried from piece to piece.  Results identical to m17hip_fir_rrc150 followed by m17hip_correlator.
int m17hip_fir_correlator(m17hip_ctx* c, uint32_t C, uint32_t T, uint32_t flags, float* y_host, float* limit_host, float* corr_host)
{
    if (!c || C == 0 || T == 0 || C > c->maxC || T > c->maxT || (flags & ~M17HIP_FLAG_INVERT)) return M17HIP_EINVAL;
    GUARD(c);
    if (c->front_queued) return M17HIP_ESTATE;
    if (!c->uploaded) return M17HIP_ESTATE;
    const size_t n = (size_t)C * T;
    HIPCHK(c, c->scratch.grow(5 * n * sizeof(float) + (size_t)C * 4 * sizeof(float), &c->last_hip));
    float* limit = (float*)c->scratch.get();
    float* corr = limit + n;
    float* lstate = corr + 4 * n;
    // pieces of whole 256-sample tiles (the limit pipeline's granule), about a tenth of the run each; anything else: one piece, the plain kernels
    const bool tiled = T % LP_TILE == 0 && T >= 8 * LP_TILE && (n & 3) == 0;
    const uint32_t piece = tiled ? std::max<uint32_t>((uint32_t)round_up((T + 9) / 10, LP_TILE), 4 * LP_TILE) : T;
    uint32_t npieces = (T + piece - 1) / piece;
    if (tiled && npieces > 1 && T - (npieces - 1) * piece < 4 * LP_TILE) --npieces;   // (a last piece of fewer than four tiles joins the one before it)
    HIPCHK(c, c->now().ensure_seg_events(npieces));   // (it borrows the current pair's `fir` events)
    int r;
    uint32_t kflags; const uint32_t* pol;
    if ((r = resolve_polarity(c, C, flags, c->stream, kflags, pol))) return r;
    auto& seg = c->now().seg;
    // (Tried: the chain on compute units of its own — hipExtStreamCreateWithCUMask, a quarter of the chip — with the two throughput kernels on
    //  the rest: the chain's pieces 0.79 -> 0.74 ms, the call 8.2 -> 9.0 ms.  What stretches the chain beside them is not its SIMD: NOTES 5.4.)
    const hipStream_t st_chain = c->stream, st_fir = c->side2, st_corr = c->side;
    const uint32_t chain_wgs = (C + LP_CH - 1) / LP_CH;
    HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
    for (hipStream_t st : {st_chain, st_fir, st_corr})
        if (st != c->stream) HIPCHK(c, hipStreamWaitEvent(st, c->ev_fork, 0));
    if (tiled) HIPCHK(c, hipMemsetAsync(lstate, 0, (size_t)C * 4 * sizeof(float), st_chain));
    for (uint32_t k = 0; k < npieces; ++k) {
        const uint32_t t0 = k * piece, len = k + 1 < npieces ? piece : T - t0;
        if ((r = launch_fir(c, C, len, kflags, false, st_fir, t0, nullptr, pol))) return r;
        HIPCHK(c, hipEventRecord(seg[k].fir, st_fir));
        HIPCHK(c, hipStreamWaitEvent(st_corr, seg[k].fir, 0));
        HIPCHK(c, hipStreamWaitEvent(st_chain, seg[k].fir, 0));
        {   // each kernel timed on the stream it runs on, under its own key: the correlations as "correlator", the limit chain as "limit_track"
            Timed tc(c, KT_CORR, st_corr);
            if (T % 4 == 0 && t0 % 4 == 0 && len % 4 == 0)
                hipLaunchKernelGGL(correlate4_kernel, dim3((len / 4 + 255) / 256, C), dim3(256), 0, st_corr, c->now().y, c->ypitch, corr, C, len, t0, T);
            else
                hipLaunchKernelGGL(correlate_kernel, dim3((len + 255) / 256, C), dim3(256), 0, st_corr, c->now().y, c->ypitch, corr, C, len, t0, T);
        }
        Timed tm(c, KT_GATE, st_chain);
#ifdef M17_TOOLS
        if (tiled && c->limit_form == 0)
            hipLaunchKernelGGL(limit_pipe_kernel, dim3(chain_wgs), dim3(320), 0, st_chain, c->now().y + t0, c->ypitch, limit + t0, (size_t)T, C, len,
                               (const float*)lstate, lstate);
        else
#endif
        if (tiled)
            hipLaunchKernelGGL(limit_relay_kernel, dim3(chain_wgs), dim3(320), 0, st_chain, c->now().y + t0, c->ypitch, limit + t0, (size_t)T, C, len,
                               (const float*)lstate, lstate);
        else
            hipLaunchKernelGGL(limit_kernel, dim3((C + 63) / 64), dim3(64), 0, st_chain, c->now().y, c->ypitch, limit, C, T);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(c->ev_join, st_corr));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    if (y_host) HIPCHK(c, hipMemcpy2DAsync(y_host, (size_t)T * sizeof(float), c->now().y + YPRE, c->ypitch * sizeof(float), (size_t)T * sizeof(float), C, hipMemcpyDeviceToHost, c->stream));
    if (limit_host) HIPCHK(c, hipMemcpyAsync(limit_host, limit, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (corr_host) HIPCHK(c, hipMemcpyAsync(corr_host, corr, 4 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return M17HIP_OK;
}

// The steps of a run (m17hip_demod_run), each on the context, the run's plan and its record set.  First: a staged run's y / h prefixes, on the main stream.
static int carry_staged_prefixes(m17hip_ctx* c, const RunPlan& p)
{
    // K2 / K5 read the input slab too (snapshots, spliced-history FIR outputs); the y / h prefixes (the correlator ring and the limit
    // filter's history reach back into the previous run) come from the previous run's slabs, final now that its K5 is done
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_in_ready, 0));
    if (p.gate0_queued) return M17HIP_OK;   // (m17hip_demod_front has queued these copies on the replay stream, in front of the first segment's replay)
    if (c->carryT) {   // (the previous run ended by carrying its tails into its own prefixes: copy those)
        hipLaunchKernelGGL((copy_prefix_kernel<float, YPRE>), dim3(p.C), dim3(64), 0, c->stream, c->other().y, c->now().y, c->ypitch);
        hipLaunchKernelGGL((copy_prefix_kernel<float, YPRE>), dim3(p.C), dim3(64), 0, c->stream, c->other().h, c->now().h, c->ypitch);
        HIPCHK(c, hipGetLastError());
    } else {
        HIPCHK(c, hipMemset2DAsync(c->now().y, c->ypitch * sizeof(float), 0, YPRE * sizeof(float), p.C, c->stream));
        HIPCHK(c, hipMemset2DAsync(c->now().h, c->ypitch * sizeof(float), 0, YPRE * sizeof(float), p.C, c->stream));
    }
    return M17HIP_OK;
}

// The run's record set `rs` is made free, and what the run needs beside the slabs is allocated the first time it is needed.
static int prepare_run(m17hip_ctx* c, const RunPlan& p, m17hip_ctx::RecSet& rs)
{
    int r;
    if (!rs.recs) {   // the second set appears with the second run
        HIPCHK(c, rs.recs.alloc((size_t)c->maxC * c->rec_cap_alloc));
        HIPCHK(c, rs.rec_count.alloc(c->maxC));
        HIPCHK(c, hipMemsetAsync(rs.rec_count, 0, (size_t)c->maxC * 4, c->stream));
    }
    if (c->defer_decode && !rs.defer_llr)   // the deferred-frame stores exist only where that mode is used (184 B per record slot)
        HIPCHK(c, rs.defer_llr.alloc((size_t)c->maxC * c->rec_cap_alloc * 46));
    if (c->defer_decode && !c->defer_hist)
        HIPCHK(c, c->defer_hist.alloc((size_t)c->maxC * DEFER_HIST_WORDS * 64));
    if (rs.valid) {   // the run that wrote it last: its payload work must be through (queued now if nobody asked for it)
        if (rs.pending && (r = flush_payload(c, false, true))) return r;
        HIPCHK(c, hipStreamWaitEvent(c->stream, rs.done, 0));
    }
    rs.valid = false;
    if (c->defer_evm) HIPCHK(c, c->evm.begin_run(c->maxT));   // (the operation rows of the deferred EVM)
    c->dbg_waves = (c->profile || c->wave_times) ? p.C : 0;
    if (!c->bnd) {
        HIPCHK(c, c->bnd.alloc(2 * (size_t)c->maxC));
        HIPCHK(c, hipMemsetAsync(c->bnd, 0, 2 * (size_t)c->maxC * sizeof(Boundary), c->stream));
    }
    if (!c->truth) {   // (K5 leaves the gate state and counts the closed gates in every mode: the next run's choice comes from it)
        HIPCHK(c, c->truth.alloc(2 * (size_t)c->maxC));
        HIPCHK(c, c->first_needed.alloc(c->maxC));
    }
    return M17HIP_OK;
}

// K5's parameters for segment k; `x`: the run's input rows (with_x)
extern "C++" {   // (a template inside the C ABI's extern "C" block)
template <typename XT>
static SeqParams seq_params(m17hip_ctx* c, const RunPlan& p, const m17hip_ctx::RecSet& rs, uint32_t k, const XT* x)
{
    const uint32_t t0 = p.t0(k), len = p.t0(k + 1) - t0;
    SeqParams P{};
    P.h = c->now().h + t0; P.final_h = by_parity(c->final_h, k, c->maxC, 4);
    P.dropped = by_parity(c->dropped, k, c->maxC);
    P.x = x + t0; P.xpitch = c->xpitch; P.y = c->now().y + t0; P.ypitch = c->ypitch;
    if constexpr (std::is_same<XT, float>::value) { P.hist_f = c->hist_f; P.bnd_hist_f = by_parity(c->bnd_hist_f, k + 1u, c->maxC, HISTF_PITCH); }
    P.dcd_table = c->now().dcd; P.ticks_cap = c->ticks_cap; P.state = c->seq_state;
    P.recs = rs.recs; P.rec_cap = c->rec_cap; P.rec_count = rs.rec_count; P.overflow = rs.ovf;
    P.tables = c->tables; P.taps = c->taps; P.llr_edges = c->llr_edges;
    P.C = p.C; P.T = len; P.pos0 = c->pos + t0; P.tick_row0 = c->pos / TICK; P.flags = (p.kflags & 1u) | (t0 ? 2u : 0u) | (std::min(k, 23u) << 8); P.pol = p.pol;
    P.kalman_order = c->kalman_order; P.channel_base = c->channel_base;
    P.level_gain = c->level_gain + (size_t)(c->kalman_order & 7u) * core::LEVEL_SCHED_N;
    P.diag_log = c->diag.entries(); P.diag_cap = c->diag.room; P.diag_count = c->diag.count();
    P.defer = c->defer_decode ? rs.defer_llr : nullptr;
    if (c->defer_evm) { P.ev_ops = c->evm.ops(); P.ev_pitch = c->evm.pitch(); P.ev_cursor_out = c->evm.cursor_out(k, p.nseg); }
    P.bnd_out = by_parity(c->bnd, k + 1u, c->maxC);
    P.truth_out = c->truth ? by_parity(c->truth, k, c->maxC) : nullptr;
    P.dbg = (c->profile || c->wave_times) ? c->dbg : nullptr;
    P.dropped_in = (k > 0 && c->redo_form != 1) ? by_parity(c->dropped, k - 1u, c->maxC) : nullptr;   // (redo in front: nobody starts a segment off the replay)
    return P;
}
}  // extern "C++"

// The chain of the run: K2 -> K5 per segment on the main stream, the replay on its stream, and what of the front end follows K5 (tuning knob 5; a gate-aware run's K1).
// K2 launches: the whole first segment from K5's state; every later segment AHEAD of K5 from the replay's own end state (replay
// stream); and the REDO: for the channels that left the replay in segment k - 1 (a forced dcd.unlock()), the replay's state at the
// end of segment k is re-derived from K5's boundary record, beside K5 of segment k on the replay stream.  It stores nothing — those
// channels serve themselves in segment k (m17_wave_kernel.hpp) — and makes the replay of segment k + 1 good for them again; K5 never
// waits for it.
static int queue_chain(m17hip_ctx* c, const RunPlan& p, const m17hip_ctx::RecSet& rs)
{
    int r;
    const uint32_t nseg = p.nseg, ahead = p.front_segs;   // (ahead < nseg: tuning knob 5 is set)
    auto& seg = c->now().seg;
    // Redo policy (m17hip_tune key 20).  IN FRONT of K5: the redo stores the history of segment k for the channels that left the replay in
    // k - 1 before K5(k) starts — sixteen channels per instruction instead of one wave each carrying the filter itself through segment k
    // (3 dependent instructions per sample): fewer instructions, but 1-2 ms of replay latency on the K5 chain of every segment that follows
    // a drop.  BESIDE K5: the redo re-derives the replay's end state only, the channels concerned serve themselves through segment k, K5
    // never waits.  Measured: wherever the chain of K5 launches is what a step lasts — a continued stream, one batch at a time — the redo
    // beside K5 wins (24.7 against 28.0 ms, 26.3 against 28.9); with round 4's matched filter several independent batches in flight were
    // 1.4 % faster with the redo in front (NOTES 4.11), with round 5's they are 5 % slower (22.6 against 21.4: NOTES 5.5).  Default: beside.
    const bool redo_front = c->redo_form == 1;
    constexpr uint32_t wpb = 4;   // one wave per channel, four waves per workgroup
    const dim3 grid((p.C + wpb - 1) / wpb), block(64 * wpb);
    // LDS: what the workgroup needs (31.8 KB for four waves), padded so that a CU holds FOUR of them and not five — the rest of
    // the CU (24 KB, 128 VGPRs per SIMD) is where a K2 wave or a K1 workgroup runs beside them without taking a K5 slot
    const size_t lds = std::max((size_t)wave_lds_words((int)wpb) * 4, c->seq_lds_bytes ? (size_t)c->seq_lds_bytes : (size_t)SEQ_LDS_BYTES_4);
    HIPCHK(c, hipMemsetAsync(rs.ovf, 0, 4, c->stream));       // record overflow of THIS run
    HIPCHK(c, hipMemsetAsync(rs.ovf + 3, 0, 4, c->stream));   // channel-segments of THIS run that end with the carrier off (K5 counts)
    for (uint32_t k = 0; k < nseg; ++k) {
        HIPCHK(c, hipStreamWaitEvent(c->stream, seg[k].fir, 0));
        HIPCHK(c, hipStreamWaitEvent(c->stream, seg[k].dcd, 0));
        if (k == 0 && c->front_first > 1 && ahead >= nseg) {   // the matched filter of the first `front_first` segments has the chip to itself
            const uint32_t last = std::min(c->front_first, nseg) - 1u;
            HIPCHK(c, hipStreamWaitEvent(c->stream, seg[last].fir, 0));
        }
        // replay stream: ahead(k) -> redo(k) [after K5(k - 1): its flags and its state] -> ahead(k + 1) -> ...; the main stream only
        // ever waits for an `ahead`
        if (k > 0) HIPCHK(c, hipStreamWaitEvent(c->stream, seg[k].gate, 0));
        if (k == 0 || redo_front) {   // the first segment whole; a redo in front: flagged channels only, from their boundary records, history stored
            if ((r = launch_gate_seg(c, p, k, c->stream, false, k > 0, k > 0))) return r;
            HIPCHK(c, hipEventRecord(seg[k].redo, c->stream));
            HIPCHK(c, hipStreamWaitEvent(c->side3, seg[k].redo, 0));
        } else if (k + 1 < nseg) {
            HIPCHK(c, hipStreamWaitEvent(c->side3, seg[k - 1].seq, 0));
            if ((r = launch_gate_seg(c, p, k, c->side3, false, true))) return r;
        }
        if (k + 1 < nseg) {
            HIPCHK(c, hipStreamWaitEvent(c->side3, seg[k + 1].fir, 0));
            HIPCHK(c, hipStreamWaitEvent(c->side3, seg[k + 1].dcd, 0));
            if ((r = launch_gate_seg(c, p, k + 1, c->side3, true, false))) return r;
            HIPCHK(c, hipEventRecord(seg[k + 1].gate, c->side3));
        }
        TimedK tm(c, KT_SEQ);
        with_x(c, c->slot, [&](auto* x) {
            const SeqParams P = seq_params(c, p, rs, k, x);
#ifdef M17_TOOLS   // (int16 rows only: run_format_check has refused these instantiations on a float stream)
            if (c->profile) tm.launch((demod_wave_kernel<int16_t, 4, true>), grid, block, lds, c->stream, P);
            else if (c->wave_times) tm.launch((demod_wave_kernel<int16_t, 4, false, true>), grid, block, lds, c->stream, P);
            else
#endif
            if (c->kalman_order == 3u) tm.launch(wave_kernel<3>(x), grid, block, lds, c->stream, P);   // (the default order: no call in the kernel)
            else tm.launch(wave_kernel<-1>(x), grid, block, lds, c->stream, P);
        });
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(seg[k].seq, c->stream));
        if (k + ahead < nseg && (r = launch_front_seg(c, p, k + ahead))) return r;
        if (p.gate_run && (r = launch_gated_fir(c, p, k))) return r;
    }
    HIPCHK(c, hipGetLastError());
    return M17HIP_OK;
}

// The end of the run on the main stream, and the context's books: `rs` holds the latest run.
static int end_run(m17hip_ctx* c, const RunPlan& p, m17hip_ctx::RecSet& rs)
{
    int r;
    const uint32_t C = p.C, T = p.T;
    // the tails a run that continues in THESE slabs (input uploaded in place) will find as its prefixes; a staged run takes them from
    // here into the other slab pair itself.  (Before the deferred decode: the next staged run's first replay waits for these, not for that.)
    with_x(c, c->slot, [&](auto* x) {
        hipLaunchKernelGGL(carry_tail_xy_kernel<std::remove_pointer_t<decltype(x)>>, dim3(C), dim3(64), 0, c->stream, x, c->xpitch, c->now().y.get(), c->ypitch, T);
    });
    hipLaunchKernelGGL((carry_tail_kernel<float, YPRE>), dim3(C), dim3(64), 0, c->stream, c->now().h.get(), c->ypitch, T);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_tail, c->stream));
    // ---- the end of the run on the MAIN stream: what the next run's chain needs of this one — the one or two deferred costs the state still
    //      names (settle_tail_kernel).  The rest of the run's EVM fold (the operations of its last two segments: 0.8 ms of one dependent chain
    //      per channel that nothing in the demodulator reads) is NOT made here: it is owed (EvmFold)
    if (c->defer_decode) {
        SettleParams S{rs.recs, c->rec_cap, rs.defer_llr, c->tables, c->seq_state, C, ev_no_fold(C)};
        hipLaunchKernelGGL(settle_tail_kernel, dim3(C), dim3(64), SETTLE_LDS_BYTES, c->stream, S);
        HIPCHK(c, hipGetLastError());
    }
    if ((r = flush_fold(c))) return r;   // (the run before: nothing of this run took its last pass along — one segment, no replay ahead)
    c->evm.end_run(C, c->defer_evm);
    HIPCHK(c, hipEventRecord(rs.chain, c->stream));
    HIPCHK(c, hipEventRecord(c->now().end, c->stream));
    { std::lock_guard<std::mutex> lk(g_runs.mu); c->last_end = c->now().end; }
    c->now().used = true; c->pos += T; c->inplace_after_run = false; c->have_run = true;
    c->lastC = C; c->runT = T; c->last_nseg = p.nseg;
    rs.valid = true; rs.C = C; rs.rec_cap = c->rec_cap; rs.nseg = p.nseg;
    rs.pending = true; rs.bert = c->bert.on; rs.pkt = c->packets.on(); rs.voice = c->voice.on();
    c->cur = (int)(&rs - c->sets); c->sel_back = 0;
    return M17HIP_OK;
}

// The run's payload work — the frames K5 did not decode itself, then the consumers — is queued when its results are asked for.  At once
// where that costs nothing or is needed: a context that does not stream (the work goes to the main stream, behind the run, as up to round 5),
// and with the diagnostic log on (ONE store, which the deferred decode patches: the next run waits for it).
static int flush_after_run(m17hip_ctx* c, const m17hip_ctx::RecSet& rs)
{
    if (c->streams() && !c->diag.on()) return M17HIP_OK;
    const int r = flush_payload(c, false, false, c->evm.owed() && c->defer_decode && c->pay() == c->stream);   // (the fold beside the decode, as up to round 5)
    if (r || !c->diag.on()) return r;
    HIPCHK(c, hipStreamWaitEvent(c->stream, rs.done, 0));
    return flush_fold(c);
}

// m17hip_demod_reset_channels, the part of a run that begins with marked channels which waits for the run before it: everything the STATE-MACHINE half
// reads.  On the main stream, behind the previous run's settle_tail_kernel and the carried / copied y and h prefixes, in front of this run's first replay:
// the listed channels' SeqState (from the context's position: their tick and their origin) and their 96-sample y / h prefixes; EvState only after the
// previous run's LAST fold pass has been through them (made here, as m17hip_diag_fetch makes it); the consumers' state on the payload stream, behind the
// payload work of every earlier run — queued now where it was still to come (flush_payload), so that those runs' statistics and packets are complete.
static int reset_marked_state(m17hip_ctx* c, const RunPlan& p)
{
    const uint32_t n = p.n_reset;
    const uint32_t* list = c->reset_list.dev();
    if (int r = flush_fold(c)) return r;
    if (int r = behind_all_runs(c)) return r;
    HIPCHK(c, c->reset_list.before_read(c->pay()));
    hipLaunchKernelGGL(consumer_reset_list_kernel, dim3((n + 63) / 64), dim3(64), 0, c->pay(), list, n, c->bert.state.get(), c->packets.state_or_null(), c->voice.state_or_null());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, c->reset_list.after_read(RD_PAY, c->pay()));
    HIPCHK(c, c->reset_list.before_read(c->stream));
    hipLaunchKernelGGL(prefix_reset_list_kernel, dim3(n), dim3(64), 0, c->stream, list, n, c->now().y.get(), c->now().h.get(), c->ypitch);
    hipLaunchKernelGGL(seq_reset_list_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, list, n, c->seq_state.get(), c->evm.state.get(), (uint64_t)c->pos);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, c->reset_list.after_read(RD_MAIN, c->stream));
    return M17HIP_OK;
}

int m17hip_demod_front(m17hip_ctx* c, uint32_t C, uint32_t T, uint32_t flags)
{
    if (!c || C == 0 || T == 0 || C > c->maxC || T > c->maxT || (flags & ~M17HIP_FLAG_INVERT)) return M17HIP_EINVAL;
    GUARD(c);
    if (c->front_queued || !c->staged) return M17HIP_ESTATE;
    RunPlan& p = c->front_plan;
    if (int r = begin_staged(c, p, C, T, flags, RUN_STAGED_FRONT)) return r;
    c->front_queued = true;
    // The replay of the staged run's first segment (K2 from K5's state) needs the run in flight only up to its last K5 launch and its
    // carried tails — not its deferred decode, its consumers, the caller's fetch of its records or the launch of the next run from the
    // host: queued here, on the replay stream, it runs beside all of those.
    // (not for a run that begins with marked channels, m17hip_demod_reset_channels: their state is reset by the run call, and this replay reads it)
    if (c->gate0_early && c->have_run && c->carryT && !c->profile && !p.n_reset) {
        m17hip_ctx::SegEvents& seg0 = c->now().seg[0];
        for (const Event* e : {&c->ev_tail, &c->ev_in_ready, &seg0.fir, &seg0.dcd}) HIPCHK(c, hipStreamWaitEvent(c->side3, *e, 0));
        hipLaunchKernelGGL((copy_prefix_kernel<float, YPRE>), dim3(C), dim3(64), 0, c->side3, c->other().y, c->now().y, c->ypitch);
        hipLaunchKernelGGL((copy_prefix_kernel<float, YPRE>), dim3(C), dim3(64), 0, c->side3, c->other().h, c->now().h, c->ypitch);
        HIPCHK(c, hipGetLastError());
        if (int r = launch_gate_seg(c, p, 0, c->side3, false, false)) return r;
        HIPCHK(c, hipEventRecord(seg0.gate, c->side3));
        p.gate0_queued = true;
    }
    return M17HIP_OK;
}

// The run is processed in segments.  K1 (throughput-bound, the whole chip) and K3 (latency-bound lone waves) of ALL segments
// are queued on two side streams; the main stream runs K2 -> K5 per segment as soon as that segment's K1 and K3 are done,
// so the front end of segment k+1 fills the issue slots K5 of segment k leaves idle (its tail above all).
// Every K2 starts a fresh speculation from K5's own state, so a channel that had to drop it (forced unlock) carries the
// limit filter itself only until the end of its segment.
int m17hip_demod_run(m17hip_ctx* c, uint32_t C, uint32_t T, uint32_t flags)
{
    if (!c || C == 0 || T == 0 || C > c->maxC || T > c->maxT || (flags & ~M17HIP_FLAG_INVERT)) return M17HIP_EINVAL;
    GUARD(c);
    int r;
    RunPlan p;
    if (c->front_queued) {   // the front end is already on its way (m17hip_demod_front): this call must be the run it was queued for
        if (C != c->front_plan.C || T != c->front_plan.T || flags != c->front_plan.flags) return M17HIP_ESTATE;
        c->front_queued = false;
        p = std::move(c->front_plan);
    } else if (c->staged) {   // input staged by m17hip_upload_i16_async and friends: swap the slabs, queue the front end
        if ((r = begin_staged(c, p, C, T, flags, RUN_STAGED))) return r;
    }
    if (!c->uploaded) return M17HIP_ESTATE;
    if (c->have_run && C != c->lastC) return M17HIP_EINVAL;  // a continued stream keeps its channel count
    if (!p.staged) {
        if ((r = run_format_check(c, c->slot))) return r;
        p = plan_run(c, C, T, flags, RUN_IN_PLACE);
        if ((r = resolve_polarity(c, C, flags, c->stream, p.kflags, p.pol))) return r;
        if (!c->marks.empty()) {   // (m17hip_demod_reset_channels; in place the main stream is behind the previous run's carried tails and its K3)
            if ((r = take_marks(c, p.n_reset, c->stream))) return r;
            if ((r = reset_marked_front(c, p.n_reset, c->stream, RD_FRONT, true, true))) return r;
        }
    }
    if ((r = p.staged ? carry_staged_prefixes(c, p) : launch_front_all(c, p))) return r;
    if (!p.staged && p.n_reset) commit_marks(c);
    if (p.n_reset && (r = reset_marked_state(c, p))) return r;
    // this run's record set: the one the run before the previous one wrote (its payload work is long through; waited for on the device)
    m17hip_ctx::RecSet& rs = c->sets[(c->sets[0].valid || c->sets[1].valid || c->have_run) ? (c->cur ^ 1) : c->cur];
    if ((r = prepare_run(c, p, rs))) return r;
    if ((r = queue_chain(c, p, rs))) return r;
    if ((r = end_run(c, p, rs))) return r;
    return flush_after_run(c, rs);
}

// The record set the fetch family names (m17hip_frames_select): the latest run's, or the run's before it; nullptr when that run's
// records are not there (no such run since the reset, or the layout was changed under them: m17hip_tune key 8).
static m17hip_ctx::RecSet* selected_set(m17hip_ctx* c)
{
    m17hip_ctx::RecSet& rs = c->sets[c->cur ^ (int)(c->sel_back & 1u)];
    return rs.valid ? &rs : nullptr;
}

// Offsets + (optionally) the dense copy in one pass and ONE stream synchronisation — of the PAYLOAD stream: behind the deferred decode
// and the consumers of the run concerned, beside whatever the main stream has been given since.  *count = records the run produced;
// at most `cap` of them are written.  M17HIP_EOVERFLOW: a channel outran its record slots during the run;
// M17HIP_ETRUNC: more records than `cap`.
static int compact_into(m17hip_ctx* c, FrameRec* dev_out, uint64_t cap, uint64_t* count)
{
    m17hip_ctx::RecSet* rs = selected_set(c);
    if (!rs) return M17HIP_ESTATE;
    int set = 0;
    if (int fr = behind_selected(c, set)) return fr;   // (`set` is rs's; behind that run wherever its payload work was queued)
    const uint32_t C = rs->C;
    if (dev_out && dev_out != c->compact && c->sel_back == 0 && c->pay() != c->stream) {
        // a device destination of the caller's: whatever the caller queued on the main stream for it (a fill, its previous consumer) comes first —
        // for the LATEST run that costs nothing (the payload work waits for that run's end on the main stream anyway); with a newer run queued
        // (m17hip_frames_select(ctx, 1)) the destination must be ready when the call is made (include/m17hip.h)
        HIPCHK(c, hipEventRecord(c->ev_dst, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->pay(), c->ev_dst, 0));
    }
    {
        Timed tm(c, KT_COMPACT, c->pay());
        hipLaunchKernelGGL(rec_offsets_kernel, dim3(1), dim3(256), 0, c->pay(), rs->rec_count, rs->rec_cap, c->rec_offsets, C);
        HIPCHK(c, hipGetLastError());
        if (dev_out) {
            hipLaunchKernelGGL(compact_kernel, dim3(C), dim3(64), 0, c->pay(), rs->recs, rs->rec_cap, rs->rec_count, c->rec_offsets, dev_out, cap, C);
            HIPCHK(c, hipGetLastError());
        }
    }
    uint64_t total = 0;
    uint32_t ovf[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(&total, c->rec_offsets + C, 8, hipMemcpyDeviceToHost, c->pay()));
    HIPCHK(c, hipMemcpyAsync(ovf, rs->ovf, 16, hipMemcpyDeviceToHost, c->pay()));
    HIPCHK(c, hipStreamSynchronize(c->pay()));
    if (count) *count = total;
    c->off_segs_prev = ovf[3]; c->chan_segs_prev = rs->C * std::max(1u, rs->nseg);   // (what the next run's gate-aware choice looks at)
    if (ovf[0]) return M17HIP_EOVERFLOW;
    if (dev_out && total > cap) return M17HIP_ETRUNC;
    return M17HIP_OK;
}

int m17hip_frames_select(m17hip_ctx* c, uint32_t back)
{
    if (!c || back > 1) return M17HIP_EINVAL;
    if (!c->sets[c->cur ^ (int)back].valid) return M17HIP_ESTATE;
    c->sel_back = back;
    return M17HIP_OK;
}

int m17hip_frames_count(m17hip_ctx* c, uint64_t* total)
{
    if (!c || !total) return M17HIP_EINVAL;
    GUARD(c);
    return compact_into(c, nullptr, 0, total);
}

int m17hip_frames_compact_device(m17hip_ctx* c, m17_frame_rec* recs_dev, uint64_t capacity, uint64_t* count)
{
    if (!c || !recs_dev) return M17HIP_EINVAL;
    GUARD(c);
    return compact_into(c, (FrameRec*)recs_dev, capacity, count);
}

int m17hip_frames_fetch(m17hip_ctx* c, m17_frame_rec* recs_host, uint64_t capacity, uint64_t* count)
{
    if (!c || !recs_host) return M17HIP_EINVAL;
    GUARD(c);
    const m17hip_ctx::RecSet* rs = selected_set(c);
    if (!rs) return M17HIP_ESTATE;
    // one compaction into the context's dense buffer; it is sized for the caller's capacity (records beyond it are not
    // wanted anyway), so a second pass is never needed
    const uint64_t want = std::max<uint64_t>(std::min<uint64_t>(capacity, (uint64_t)rs->C * rs->rec_cap), 1024);
    if (want > c->compact.size()) HIPCHK(c, hipStreamSynchronize(c->pay()));   // (nothing still reads the one it outgrew)
    HIPCHK(c, c->compact.grow(want, &c->last_hip));
    uint64_t total = 0;
    const int r = compact_into(c, c->compact, std::min<uint64_t>(capacity, c->compact.size()), &total);
    if (r && r != M17HIP_EOVERFLOW && r != M17HIP_ETRUNC) return r;
    const uint64_t n = std::min(total, capacity);
    if (n) HIPCHK(c, hipMemcpy(recs_host, c->compact, (size_t)n * sizeof(FrameRec), hipMemcpyDeviceToHost));
    if (count) *count = total;
    return r;
}

int m17hip_diag_fetch(m17hip_ctx* c, m17_diag* diag_host, uint32_t C)
{
    if (!c || !diag_host || C == 0 || C > c->maxC) return M17HIP_EINVAL;
    GUARD(c);
    if (int fr = flush_fold(c)) return fr;        // m17_diag::evm of the latest run: its last fold pass, if nothing has made it yet
    if (c->front_queued && c->front_plan.gate0_queued)   // (... or the replay m17hip_demod_front queued for the next run is making it: wait for that launch)
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->now().seg[0].gate, 0));
    HIPCHK(c, hipMemcpy2DAsync(diag_host, sizeof(Diag), &c->seq_state[0].cold.diag, sizeof(SeqState), sizeof(Diag), C, hipMemcpyDeviceToHost,
                               c->stream));
    OvfWords ovf;
    HIPCHK(c, ovf.read(c->overflow, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ovf.evm_ops_dropped() ? M17HIP_EOVERFLOW : M17HIP_OK;   // (every field but `evm` is right)
}

int m17hip_diag_log_fetch(m17hip_ctx* c, m17_diag* log_host, uint32_t* counts_host, uint32_t C, uint32_t capacity)
{
    if (!c || !log_host || !counts_host || C == 0 || C > c->maxC || capacity == 0) return M17HIP_EINVAL;
    GUARD(c);
    if (!c->diag.on() || !c->sets[c->cur].valid) return M17HIP_ESTATE;
    if (int fr = flush_fold(c)) return fr;
    // Neither behind_all_runs nor behind_selected: there is ONE log, the latest run's whatever m17hip_frames_select names, and it is read on the main
    // stream, where K5 and the fold wrote it.  So all payload work is queued and the HOST waits for the payload stream; payload work that went to the
    // main stream (before the payload stream moved) is in front of the copies below in stream order.
    if (int fr = flush_payload(c)) return fr;
    HIPCHK(c, hipStreamSynchronize(c->pay()));   // (the deferred decode has put the costs into the log's entries)
    HIPCHK(c, hipMemcpyAsync(counts_host, c->diag.count(), (size_t)C * 4, hipMemcpyDeviceToHost, c->stream));
    const uint32_t n = std::min(capacity, c->diag.room);
    HIPCHK(c, hipMemcpy2DAsync(log_host, (size_t)capacity * sizeof(Diag), c->diag.entries(), (size_t)c->diag.room * sizeof(Diag), (size_t)n * sizeof(Diag), C,
                               hipMemcpyDeviceToHost, c->stream));
    OvfWords ovf;
    HIPCHK(c, ovf.read(c->overflow, c->stream));   // (on the stream of the two copies above: one synchronisation for the three)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (ovf.evm_ops_dropped()) return M17HIP_EOVERFLOW;   // (see m17hip_diag_fetch)
    bool trunc = false;
    for (uint32_t i = 0; i < C; ++i) trunc = trunc || counts_host[i] > n;
    return trunc ? M17HIP_ETRUNC : M17HIP_OK;
}

int m17hip_lsf_info(m17hip_ctx* c, const uint8_t* lsf30_host, uint32_t n, m17_lsf_info* out_host)
{
    if (!c || !lsf30_host || !out_host || n == 0) return M17HIP_EINVAL;
    GUARD(c);
    static_assert(sizeof(LsfInfo) == sizeof(m17_lsf_info) && sizeof(LsfInfo) == 32, "m17_lsf_info layout");
    const size_t in_b = round_up((size_t)n * 30, 256);
    HIPCHK(c, c->scratch.grow(in_b + (size_t)n * sizeof(LsfInfo), &c->last_hip));
    uint8_t* din = reinterpret_cast<uint8_t*>(c->scratch.get());
    LsfInfo* dout = reinterpret_cast<LsfInfo*>(din + in_b);
    HIPCHK(c, hipMemcpyAsync(din, lsf30_host, (size_t)n * 30, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(lsf_info_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, din, n, dout);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out_host, dout, (size_t)n * sizeof(LsfInfo), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return M17HIP_OK;
}

int m17hip_bert_stats(m17hip_ctx* c, m17_bert_stat* stats_host, uint32_t C)
{
    if (!c || !stats_host || C == 0 || C > c->maxC) return M17HIP_EINVAL;
    GUARD(c);
    if (!c->bert.on) return M17HIP_ESTATE;
    if (int fr = behind_all_runs(c)) return fr;
    std::vector<BertState> tmp(C);
    HIPCHK(c, hipMemcpyAsync(tmp.data(), c->bert.state, (size_t)C * sizeof(BertState), hipMemcpyDeviceToHost, c->pay()));   // (behind the consumers of the runs queued so far)
    HIPCHK(c, hipStreamSynchronize(c->pay()));
    for (uint32_t i = 0; i < C; ++i) {
        stats_host[i].bits = tmp[i].bit_count; stats_host[i].errors = tmp[i].err_count;
        stats_host[i].synced = tmp[i].synced; stats_host[i].frames = tmp[i].frames;
    }
    return M17HIP_OK;
}

// The payload stream's buffer of sweep words holds at least n (nothing on that stream still uses the old one: the callers wait for it)
static int ensure_chan_words(m17hip_ctx* c, uint64_t n)
{
    if (n > c->chan_words.size()) HIPCHK(c, hipStreamSynchronize(c->pay()));
    HIPCHK(c, c->chan_words.grow(n, &c->last_hip));
    return M17HIP_OK;
}

int m17hip_sweep_stats(m17hip_ctx* c, uint32_t n_points, m17_chan_stat* host, uint32_t C)
{
    if (!c || !host || n_points == 0 || C == 0 || C > c->maxC) return M17HIP_EINVAL;
    GUARD(c);
    static_assert(sizeof(ChanStat) == sizeof(m17_chan_stat) && sizeof(ChanStat) == 32, "m17_chan_stat layout");
    if (!c->bert.on || !c->have_run) return M17HIP_ESTATE;
    // m17hip_diag_fetch's order for `evm`: the latest run's last fold pass on the main stream (or the replay m17hip_demod_front queued is making it)
    if (int fr = flush_fold(c)) return fr;
    if (c->front_queued && c->front_plan.gate0_queued) HIPCHK(c, hipStreamWaitEvent(c->stream, c->now().seg[0].gate, 0));
    // ... m17hip_bert_stats' order for the PRBS9 state: the payload work of both runs, wherever it was queued
    if (int fr = behind_all_runs(c)) return fr;
    // ... and the words are made and copied on the payload stream, behind the main stream's work so far
    if (c->pay() != c->stream) {
        HIPCHK(c, hipEventRecord(c->ev_fetch, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->pay(), c->ev_fetch, 0));
    }
    if (int r = ensure_chan_words(c, c->maxC)) return r;
    hipLaunchKernelGGL(sweep_stats_kernel, dim3((C + 63) / 64), dim3(64), 0, c->pay(), c->bert.state, c->seq_state, c->overflow, C,
                       c->channel_base, n_points, c->chan_words);
    HIPCHK(c, hipGetLastError());
    OvfWords ovf;
    HIPCHK(c, hipMemcpyAsync(host, c->chan_words, (size_t)C * sizeof(ChanStat), hipMemcpyDeviceToHost, c->pay()));
    HIPCHK(c, ovf.read(c->overflow, c->pay()));
    HIPCHK(c, hipStreamSynchronize(c->pay()));
    return ovf.evm_ops_dropped() ? M17HIP_EOVERFLOW : M17HIP_OK;
}

// m17hip_packets_feed, m17hip_voice_feed: the caller's records [C][pitch] and counts [C] copied to the scratch buffer on the payload stream, where the
// runs' own consumer works on the same state — behind the payload work of every run (the state goes from run to run)
static int stage_feed(m17hip_ctx* c, const m17_frame_rec* recs_host, const uint32_t* counts_host, uint32_t C, uint32_t pitch, FrameRec*& drec, uint32_t*& dcnt)
{
    if (int fr = behind_all_runs(c)) return fr;
    const size_t rec_b = round_up((size_t)C * pitch * sizeof(FrameRec), 256);
    HIPCHK(c, c->scratch.grow(rec_b + (size_t)C * 4, &c->last_hip));
    drec = reinterpret_cast<FrameRec*>(c->scratch.get());
    dcnt = reinterpret_cast<uint32_t*>(c->scratch + rec_b);
    HIPCHK(c, hipMemcpyAsync(drec, recs_host, (size_t)C * pitch * sizeof(FrameRec), hipMemcpyHostToDevice, c->pay()));
    HIPCHK(c, hipMemcpyAsync(dcnt, counts_host, (size_t)C * 4, hipMemcpyHostToDevice, c->pay()));
    return M17HIP_OK;
}

int m17hip_packets_feed(m17hip_ctx* c, const m17_frame_rec* recs_host, const uint32_t* counts_host, uint32_t C, uint32_t pitch)
{
    if (!c || !recs_host || !counts_host || C == 0 || C > c->maxC || pitch == 0) return M17HIP_EINVAL;
    GUARD(c);
    if (!c->packets.on()) return M17HIP_ESTATE;   // (not refused between m17hip_demod_front and m17hip_demod_run, as m17hip_voice_feed is: kept)
    FrameRec* drec; uint32_t* dcnt;
    if (int r = stage_feed(c, recs_host, counts_host, C, pitch, drec, dcnt)) return r;
    // (the store of the latest run's set: what m17hip_packets_fetch names unless m17hip_frames_select says otherwise)
    if (int r = c->packets.consume(c, c->pay(), drec, pitch, dcnt, C, c->cur)) return r;
    HIPCHK(c, hipStreamSynchronize(c->pay()));   // the host buffers may go away
    c->packets.fed = true;
    return M17HIP_OK;
}

int m17hip_packets_fetch(m17hip_ctx* c, m17_packet_rec* recs_host, uint32_t capacity, uint32_t* count)
{
    if (!c || !count || (capacity && !recs_host)) return M17HIP_EINVAL;
    GUARD(c);
    static_assert(sizeof(PacketRec) == sizeof(m17_packet_rec) && sizeof(PacketRec) == 864, "m17_packet_rec layout");
    const Packets& pk = c->packets;
    if (!pk.on() || !(c->have_run || pk.fed)) return M17HIP_ESTATE;
    int ps = 0;   // the packets completed by the SELECTED run (m17hip_frames_select)
    if (int r = behind_selected(c, ps)) return r;
    uint32_t total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, pk.count(ps), 4, hipMemcpyDeviceToHost, c->pay()));
    HIPCHK(c, hipStreamSynchronize(c->pay()));
    *count = total;
    const uint32_t stored = std::min(total, pk.room);
    std::vector<PacketRec> tmp(stored);
    if (stored) HIPCHK(c, hipMemcpy(tmp.data(), pk.store(ps), (size_t)stored * sizeof(PacketRec), hipMemcpyDeviceToHost));
    std::sort(tmp.begin(), tmp.end(), [](const PacketRec& a, const PacketRec& b) { return a.channel != b.channel ? a.channel < b.channel : a.seq < b.seq; });
    const uint32_t n = std::min(stored, capacity);
    if (n) std::memcpy(recs_host, tmp.data(), (size_t)n * sizeof(PacketRec));
    return total > pk.room ? M17HIP_EOVERFLOW : M17HIP_OK;
}

// The store of the run the fetch family names (m17hip_frames_select), ordered behind that run's payload work wherever it was queued
static int voice_select(m17hip_ctx* c, int& ps)
{
    if (!c->voice.on() || !(c->have_run || c->voice.fed)) return M17HIP_ESTATE;
    return behind_selected(c, ps);
}

int m17hip_voice_fetch(m17hip_ctx* c, uint8_t* audio_host, uint8_t* marks_host, uint32_t* counts_host, uint32_t C, uint32_t slots)
{
    if (!c || !counts_host || C == 0 || C > c->maxC || (slots && (!audio_host || !marks_host))) return M17HIP_EINVAL;
    GUARD(c);
    int ps = 0;
    if (int r = voice_select(c, ps)) return r;
    const Voice& v = c->voice;
    if (C > v.rows[ps]) return M17HIP_EINVAL;   // (rows the consumer has not written)
    const uint32_t room = v.room, w = std::min(slots, room);
    HIPCHK(c, hipMemcpyAsync(counts_host, v.counts(ps), (size_t)C * 4, hipMemcpyDeviceToHost, c->pay()));
    if (w) {   // rows cut at `slots` (slots beyond the room are not written)
        HIPCHK(c, hipMemcpy2DAsync(audio_host, (size_t)slots * 16, v.audio(ps), (size_t)room * 16, (size_t)w * 16, C, hipMemcpyDeviceToHost, c->pay()));
        HIPCHK(c, hipMemcpy2DAsync(marks_host, slots, v.marks(ps), room, w, C, hipMemcpyDeviceToHost, c->pay()));
    }
    HIPCHK(c, hipStreamSynchronize(c->pay()));
    bool over = false, trunc = false;
    for (uint32_t i = 0; i < C; ++i) { over = over || counts_host[i] > room; trunc = trunc || counts_host[i] > slots; }
    return over ? M17HIP_EOVERFLOW : (trunc ? M17HIP_ETRUNC : M17HIP_OK);
}

int m17hip_voice_device(m17hip_ctx* c, const uint8_t** audio_dev, const uint8_t** marks_dev, const uint32_t** counts_dev, uint32_t* pitch_slots)
{
    if (!c || !audio_dev || !marks_dev || !counts_dev || !pitch_slots) return M17HIP_EINVAL;
    GUARD(c);
    int ps = 0;
    if (int r = voice_select(c, ps)) return r;
    HIPCHK(c, hipStreamSynchronize(c->pay()));
    *audio_dev = c->voice.audio(ps); *marks_dev = c->voice.marks(ps); *counts_dev = c->voice.counts(ps);
    *pitch_slots = c->voice.room;
    return M17HIP_OK;
}

int m17hip_calls_fetch(m17hip_ctx* c, m17_call_rec* host, uint32_t capacity, uint32_t* count)
{
    if (!c || !count || (capacity && !host)) return M17HIP_EINVAL;
    GUARD(c);
    static_assert(sizeof(CallRec) == sizeof(m17_call_rec) && sizeof(CallRec) == 72, "m17_call_rec layout");
    int ps = 0;
    if (int r = voice_select(c, ps)) return r;
    const uint32_t C = c->voice.rows[ps], room = c->voice.call_room;
    std::vector<uint32_t> cnt(C);
    if (C) HIPCHK(c, hipMemcpyAsync(cnt.data(), c->voice.call_counts(ps), (size_t)C * 4, hipMemcpyDeviceToHost, c->pay()));
    HIPCHK(c, hipStreamSynchronize(c->pay()));
    uint64_t total = 0; uint32_t most = 0; bool over = false;
    for (uint32_t n : cnt) { total += n; most = std::max(most, std::min(n, room)); over = over || n > room; }
    *count = (uint32_t)std::min<uint64_t>(total, 0xFFFFFFFFu);
    if (most && capacity) {   // the columns in use of every channel's row, then row after row: (channel, seq) order
        std::vector<CallRec> tmp((size_t)C * most);
        HIPCHK(c, hipMemcpy2D(tmp.data(), (size_t)most * sizeof(CallRec), c->voice.calls(ps), (size_t)room * sizeof(CallRec), (size_t)most * sizeof(CallRec), C,
                              hipMemcpyDeviceToHost));
        uint32_t written = 0;
        for (uint32_t ch = 0; ch < C && written < capacity; ++ch) {
            const uint32_t k = std::min(std::min(cnt[ch], room), capacity - written);
            if (k) std::memcpy(host + written, tmp.data() + (size_t)ch * most, (size_t)k * sizeof(CallRec));
            written += k;
        }
    }
    return over ? M17HIP_EOVERFLOW : M17HIP_OK;
}

int m17hip_voice_feed(m17hip_ctx* c, const m17_frame_rec* recs_host, const uint32_t* counts_host, uint32_t C, uint32_t pitch)
{
    if (!c || !recs_host || !counts_host || C == 0 || C > c->maxC || pitch == 0) return M17HIP_EINVAL;
    GUARD(c);
    if (c->front_queued || !c->voice.on()) return M17HIP_ESTATE;
    FrameRec* drec; uint32_t* dcnt;
    if (int r = stage_feed(c, recs_host, counts_host, C, pitch, drec, dcnt)) return r;
    if (int r = c->voice.consume(c, c->pay(), drec, pitch, dcnt, C, c->cur)) return r;   // (the store of the latest run's set, as m17hip_packets_feed)
    HIPCHK(c, hipStreamSynchronize(c->pay()));   // the host buffers may go away
    c->voice.fed = true;
    return M17HIP_OK;
}

int m17hip_set_kalman_order(m17hip_ctx* c, int order)
{
    if (!c || order < 0 || order > 7) return M17HIP_EINVAL;
    c->kalman_order = (uint32_t)order;
    return M17HIP_OK;
}

int m17hip_set_channel_base(m17hip_ctx* c, uint32_t channel_base)
{
    if (!c) return M17HIP_EINVAL;
    c->channel_base = channel_base;
    return M17HIP_OK;
}

int m17hip_kalman_trace(m17hip_ctx* c, const float* z_host, const uint32_t* dt_host, uint32_t rows, uint32_t n, int wrap, float z0, int order,
                        float* out_host)
{
    if (!c || !z_host || !dt_host || !out_host || rows == 0 || n == 0 || order < 0 || order > 7 || (wrap != 0 && wrap != 10 && wrap != -1)) return M17HIP_EINVAL;
    GUARD(c);
    const size_t cnt = (size_t)rows * n;
    const size_t o1 = round_up(cnt * 4, 256), o2 = o1 + round_up(cnt * 4, 256);
    HIPCHK(c, c->scratch.grow(o2 + cnt * 24, &c->last_hip));
    char* b = c->scratch;
    HIPCHK(c, hipMemcpyAsync(b, z_host, cnt * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b + o1, dt_host, cnt * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(kalman_kernel, dim3((rows + 63) / 64), dim3(64), 0, c->stream, (const float*)b, (const uint32_t*)(b + o1), rows, n, wrap, z0,
                       (uint32_t)order, (float*)(b + o2), c->level_gain + (size_t)order * core::LEVEL_SCHED_N);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out_host, b + o2, cnt * 24, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return M17HIP_OK;
}

int m17hip_upload_wait(m17hip_ctx* c)
{
    if (!c) return M17HIP_EINVAL;
    GUARD(c);
    if (c->ev_copy) HIPCHK(c, hipEventSynchronize(c->ev_copy));
    return M17HIP_OK;
}

// ---- multi-GPU: gather of the frame records over RCCL ------------------------------------------------------------------
int m17hip_comm_get_id(void* id128)
{
    if (!id128) return M17HIP_EINVAL;
    const Rccl& R = rccl();
    if (!R.ok) return M17HIP_ECOMM;
    static_assert(sizeof(ncclUniqueId) == M17HIP_COMM_ID_BYTES, "RCCL unique id size");
    ncclUniqueId id;
    if (R.GetUniqueId(&id) != ncclSuccess) return M17HIP_ECOMM;
    std::memcpy(id128, &id, sizeof(id));
    return M17HIP_OK;
}

int m17hip_comm_create(m17hip_ctx* c, const void* id128, int rank, int nranks, m17hip_comm** out)
{
    if (!c || !id128 || !out || nranks < 1 || rank < 0 || rank >= nranks) return M17HIP_EINVAL;
    GUARD(c);
    const Rccl& R = rccl();
    if (!R.ok) return M17HIP_ECOMM;
    m17hip_comm* m = new (std::nothrow) m17hip_comm();
    if (!m) return M17HIP_ENOMEM;
    m->device = c->device; m->rank = rank; m->nranks = nranks;
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    const ncclResult_t r = R.CommInitRank(&m->comm, nranks, id, rank);
    if (r != ncclSuccess) { c->last_hip = 0x10000 | (int)r; delete m; return M17HIP_ECOMM; }   // (no communicator to ask: the ncclResult_t is left in m17hip_last_hip_error, | 0x10000)
    hipError_t e = m->counts_dev.alloc(2 * (size_t)nranks);
    // (no slot looks like a word of call 1.  ON the stream the gather works on, and waited for: a plain hipMemset runs on the default stream and is not waited
    //  for — with the library's own non-blocking streams it could land behind the first exchange's words: one first gather in a few hundred then read 0xFF..
    //  where a peer's word had been and answered ECOMM.  Found by tests/test_gpu_gather_ranks.py, four ranks, 2 of 25 suite runs)
    if (e == hipSuccess) e = hipMemsetAsync(m->counts_dev, 0xFF, 2 * (size_t)nranks * sizeof(uint64_t), c->pay());
    if (e == hipSuccess) e = hipStreamSynchronize(c->pay());
    if (e == hipSuccess) e = hipHostMalloc((void**)&m->words_host, (2 + 2 * (size_t)nranks) * sizeof(uint64_t), hipHostMallocDefault);
    if (e != hipSuccess) { c->last_hip = (int)e; m17hip_comm_destroy(m); return M17HIP_ENOMEM; }
    *out = m;
    return M17HIP_OK;
}

void m17hip_comm_destroy(m17hip_comm* m)
{
    if (!m) return;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    hipSetDevice(m->device);
    const ncclComm_t comm = m->dead ? nullptr : m->comm;   // (a communicator that was given up is not waited for)
    if (m->words_host) (void)hipHostFree(m->words_host);
    delete m;   // (its device memory goes before the communicator)
    if (comm) rccl().CommDestroy(comm);
    if (prev >= 0) hipSetDevice(prev);
}

// Every rank makes the same sequence of collective calls whatever goes wrong locally: a failure travels as a status inside the words
// that are exchanged anyway, and all ranks return together (a rank that left early would leave its peers waiting inside RCCL).
//   exchange 1 (all-gather, two words per rank):  [0] = record count (40 bits) | call serial (16 bits) | status (8 bits: -code)
//                                                 [1] = the ROOT's staging capacity in records (0 from the other ranks)
//       the serial makes a stale word recognisable: a rank whose own word could not be written to the device (its HIP calls fail)
//       still joins the all-gather, and what its peers then read in its slot is a word of an EARLIER exchange
//   exchange 2 (all-gather, one word per rank), ALWAYS: "I have read exchange 1 and am ready for the records" — the root grows its
//       staging first when the gathered set does not fit and says whether that worked; a rank that could NOT read exchange 1 (it does
//       not know the counts and cannot take part in exchange 3) says so here, where up to round 5 it returned and left its peers
//       waiting in exchange 3.  The words carry a phase tag in the status byte's place (0xA5: no status of exchange 1 looks like it,
//       and read as one it is an error) and the serial again; EVERY rank looks at EVERY slot — a slot without the tag and this call's
//       serial is a word that could not be written, whoever's it is — so that all ranks leave together or go on together
//   exchange 3: grouped ncclSend / ncclRecv of the exact record sets, rank after rank = global (channel, seq) order; ranks without
//       records are skipped on both sides
// What no exchange of words can close (a rank that reads exchange 1 but not exchange 2; a peer process that died) is bounded in TIME:
// every wait of this function is a bounded one (m17hip_tune key 31, default 120 s); a wait that runs out gives the communicator up
// (ncclCommAbort where the library has it) and the call — and every later call through that communicator — returns M17HIP_ECOMM.
static void comm_give_up(m17hip_comm* m, int code)
{
    m->last_rccl = code;
    if (m->dead) return;
    m->dead = true;
    const Rccl& R = rccl();
    if (m->comm && R.CommAbort) { R.CommAbort(m->comm); m->comm = nullptr; }   // (without it the communicator is left alone: destroying it would wait for the exchange)
}
// hipStreamSynchronize with a deadline: 0 = done, M17HIP_ECOMM = not in time (communicator given up), M17HIP_EHIP = the stream reports an error
static int comm_wait(m17hip_ctx* c, m17hip_comm* m)
{
    if (c->gather_timeout_ms == 0) {
        const hipError_t e = hipStreamSynchronize(c->pay());
        if (e != hipSuccess) { c->last_hip = (int)e; return M17HIP_EHIP; }
        return M17HIP_OK;
    }
    timespec t0;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (uint64_t spins = 0;; ++spins) {
        const hipError_t e = hipStreamQuery(c->pay());
        if (e == hipSuccess) return M17HIP_OK;
        if (e != hipErrorNotReady) { c->last_hip = (int)e; return M17HIP_EHIP; }
        (void)hipGetLastError();
        if ((spins & 63) == 63) {
            timespec t;
            clock_gettime(CLOCK_MONOTONIC, &t);
            const double ms = (t.tv_sec - t0.tv_sec) * 1e3 + (t.tv_nsec - t0.tv_nsec) * 1e-6;
            if (ms > (double)c->gather_timeout_ms) { comm_give_up(m, (int)ncclSystemError); return M17HIP_ECOMM; }
            if (ms > 2.0) { timespec nap{0, 50000}; nanosleep(&nap, nullptr); }   // (a gather is through in well under that: only a stuck one gets here)
        }
    }
}

// The gather protocol above over what a rank contributes: `elem` bytes per element; prepare(src, mine, overflow) puts this rank's elements
// dense on the device (the payload stream's work) and returns its local status.  m17hip_gather_frames[_device]: the selected run's frame
// records, compacted; m17hip_gather_sweep_stats: the caller's sweep words, uploaded.
extern "C++" {   // (a template inside the C ABI's extern "C" block)
template <class Prepare>
static int gather_impl(m17hip_ctx* c, m17hip_comm* m, int root, size_t elem, Prepare&& prepare, void* recs_host, uint64_t capacity, uint64_t* counts_host,
                       uint64_t* total_out, bool dest_is_device)
{
    if (!c || !m || m->device != c->device || root < 0 || root >= m->nranks || (m->rank == root && capacity && !recs_host)) return M17HIP_EINVAL;
    GUARD(c);
    if (m->dead) return M17HIP_ECOMM;
    const Rccl& R = rccl();
    const bool is_root = m->rank == root;
    auto hip_code = [&](hipError_t e) { return alloc_code(c, e); };
    auto comm_failed = [&](ncclResult_t q) { comm_give_up(m, (int)q); return M17HIP_ECOMM; };   // a collective call itself failed: nothing more can be agreed on
    // 1. this rank's elements, dense on the device
    const void* src = nullptr;
    uint64_t mine = 0;
    bool overflow = false;
    int local = prepare(src, mine, overflow);
    if (is_root && !m->gathered && local == M17HIP_OK && c->gather_fault != 2)   // a first staging buffer (grown below when a gathered set outgrows it)
        (void)m->gathered.alloc((size_t)std::max<uint64_t>(2 * mine * (uint64_t)m->nranks, 1024) * elem);
    const uint64_t gathered_cap = m->gathered.size() / elem;   // (in elements of this call)
    // 2. exchange 1
    const uint64_t serial = (uint64_t)(++m->serial & 0xFFFFu);
    constexpr uint64_t COUNT_MASK = (1ull << 40) - 1;
    if (mine > COUNT_MASK && !local) { local = M17HIP_EINVAL; mine = 0; }   // (2^40 records: not a real case, but the word has no room for more)
    uint64_t* const word = m->words_host;        // (pinned, owned by the communicator: see there)
    uint64_t* const words = m->words_host + 2;
    word[0] = (mine & COUNT_MASK) | (serial << 40) | ((uint64_t)(uint8_t)(-local) << 56);
    word[1] = is_root ? gathered_cap : 0ull;
    const size_t words_n = 2 * (size_t)m->nranks;
    int unread = M17HIP_OK;   // this rank could not read exchange 1
    {
        hipError_t e = hipMemcpyAsync(m->counts_dev + 2 * m->rank, word, 16, hipMemcpyHostToDevice, c->pay());
        if (e != hipSuccess && !local) local = hip_code(e);     // (our slot keeps the previous call's word: its serial gives it away)
        const ncclResult_t q = R.AllGather(m->counts_dev + 2 * m->rank, m->counts_dev, 2, ncclUint64, m->comm, c->pay());
        if (q != ncclSuccess) return comm_failed(q);
        e = c->gather_fault == 4 ? hipErrorUnknown : hipMemcpyAsync(words, m->counts_dev, words_n * 8, hipMemcpyDeviceToHost, c->pay());
        if (e != hipSuccess) unread = hip_code(e);
        const int w = comm_wait(c, m);
        if (w == M17HIP_ECOMM) return w;     // not in time: the communicator is given up
        if (w && !unread) unread = w;
    }
    std::vector<uint64_t> counts((size_t)m->nranks, 0);
    uint64_t total = 0;
    int remote = M17HIP_OK;
    if (!unread) {
        for (int k = 0; k < m->nranks; ++k) {
            const uint64_t w = words[2 * (size_t)k];
            int code = -(int)(w >> 56);
            if (((w >> 40) & 0xFFFFu) != serial) code = M17HIP_ECOMM;   // a stale word: that rank could not deliver this call's
            counts[k] = code ? 0 : (w & COUNT_MASK);
            total += counts[k];
            if (code && !remote) remote = code;
        }
        if (counts_host) std::memcpy(counts_host, counts.data(), counts.size() * 8);
        if (total_out) *total_out = total;
    }
    // 3. exchange 2: every rank, whatever it knows by now.  The root grows its staging when the gathered set does not fit it
    //    (only when the records are going to travel: every rank that read exchange 1 comes to the same conclusion about that)
    int rc = unread;
    if (!unread && !local && !remote && is_root && (total > gathered_cap || c->gather_fault == 3)) {   // (fault 3 on the root: grown in any case)
        m->gathered.release(&c->last_hip);
        const uint64_t want = std::max<uint64_t>(total + total / 8, 1024);
        const hipError_t e = c->gather_fault == 2 ? hipErrorOutOfMemory : m->gathered.alloc((size_t)want * elem);
        if (e != hipSuccess) rc = hip_code(e);
    }
    constexpr uint64_t PHASE2 = 0xA5ull << 56;
    {
        word[0] = PHASE2 | (serial << 40) | (uint64_t)(uint8_t)(-rc);
        const hipError_t ew = c->gather_fault == 3 ? hipErrorUnknown : hipMemcpyAsync(m->counts_dev + 2 * m->rank, word, 8, hipMemcpyHostToDevice, c->pay());
        if (ew != hipSuccess && !rc) rc = hip_code(ew);          // (our slot keeps a word of exchange 1: no tag — every rank sees that)
        const ncclResult_t q = R.AllGather(m->counts_dev + 2 * m->rank, m->counts_dev, 2, ncclUint64, m->comm, c->pay());
        if (q != ncclSuccess) return comm_failed(q);
        hipError_t e = c->gather_fault == 5 ? hipErrorUnknown : hipMemcpyAsync(words, m->counts_dev, words_n * 8, hipMemcpyDeviceToHost, c->pay());
        const int w = comm_wait(c, m);
        if (w == M17HIP_ECOMM) return w;
        // this rank cannot read what was agreed on: it cannot know whether the records travel, so it takes no part in exchange 3.  If they
        // do, its peers' waits run out (comm_wait) — the one case that costs them the communicator
        if (e != hipSuccess) return hip_code(e);
        if (w) return w;
    }
    if (unread) return unread;
    if (local) return local;
    if (remote) return M17HIP_ECOMM;   // some other rank could not deliver its records: nobody sends, everybody returns
    bool all_ok = true;
    for (int k = 0; k < m->nranks; ++k) {
        const uint64_t w = words[2 * (size_t)k];
        if ((w & (0xFFull << 56)) != PHASE2 || ((w >> 40) & 0xFFFFu) != serial || (w & 0xFFu)) all_ok = false;
    }
    if (rc) return rc;
    if (!all_ok) return M17HIP_ECOMM;   // the root has no room for the gathered set, a rank could not read the counts, or some rank's word did not arrive: nobody sends
    // 4. the records travel to the root with their exact sizes, rank after rank = global channel order
    if (is_root) {
        ncclResult_t q = R.GroupStart();
        uint64_t off = 0;
        for (int k = 0; k < m->nranks && q == ncclSuccess; ++k) {
            if (k != root && counts[k]) q = R.Recv(m->gathered + off * elem, (size_t)counts[k] * elem, ncclUint8, k, m->comm, c->pay());
            off += counts[k];
        }
        const ncclResult_t qe = R.GroupEnd();   // the group is closed whatever happened inside it
        if (q == ncclSuccess) q = qe;
        if (q != ncclSuccess) return comm_failed(q);
        off = 0;
        hipError_t he = hipSuccess;
        for (int k = 0; k < m->nranks; ++k) {   // the root's own share: a plain copy, outside the group
            if (k == root && mine) he = hipMemcpyAsync(m->gathered + off * elem, src, (size_t)mine * elem, hipMemcpyDeviceToDevice, c->pay());
            off += counts[k];
        }
        if (he != hipSuccess) return hip_code(he);
        if (const int w = comm_wait(c, m)) return w;
        // the caller's buffer is written only now, when nothing on the stream depends on a peer any more: a call that ran out of time
        // never leaves a copy into the caller's memory behind
        const uint64_t n = std::min(total, capacity);
        if (n) {
            if (dest_is_device && c->sel_back == 0 && c->pay() != c->stream) {   // (a device destination: behind the caller's main-stream work on it, as in compact_into)
                HIPCHK(c, hipEventRecord(c->ev_dst, c->stream));
                HIPCHK(c, hipStreamWaitEvent(c->pay(), c->ev_dst, 0));
            }
            HIPCHK(c, hipMemcpyAsync(recs_host, m->gathered, (size_t)n * elem, dest_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->pay()));
            HIPCHK(c, hipStreamSynchronize(c->pay()));
        }
        if (overflow) return M17HIP_EOVERFLOW;
        return total > capacity ? M17HIP_ETRUNC : M17HIP_OK;
    }
    if (mine) {
        ncclResult_t q = R.GroupStart();
        if (q == ncclSuccess) q = R.Send(src, (size_t)mine * elem, ncclUint8, root, m->comm, c->pay());
        const ncclResult_t qe = R.GroupEnd();
        if (q == ncclSuccess) q = qe;
        if (q != ncclSuccess) return comm_failed(q);
    }
    if (const int w = comm_wait(c, m)) return w;
    return overflow ? M17HIP_EOVERFLOW : M17HIP_OK;
}
}   // extern "C++"

// m17hip_gather_frames[_device]: the selected run's records, dense and (channel, seq)-ordered, in the context's compaction buffer
// (compact_into orders the payload stream behind the selected run: every transfer of the records is queued behind that)
static int gather_frames_impl(m17hip_ctx* c, m17hip_comm* m, int root, m17_frame_rec* recs, uint64_t capacity, uint64_t* counts_host, uint64_t* total_out,
                              bool dest_is_device)
{
    auto prepare = [c](const void*& src, uint64_t& mine, bool& overflow) {
        mine = 0;
        int local = selected_set(c) ? M17HIP_OK : M17HIP_ESTATE;
        overflow = false;
        if (local == M17HIP_OK) {
            int r = c->gather_fault == 1 ? M17HIP_EHIP : compact_into(c, c->compact, c->compact.size(), &mine);
            // the dense buffer must hold ALL of this rank's records before anything is sent from it, whatever the first pass said
            // (an overflowed run reports EOVERFLOW before the truncation is looked at)
            if ((r == M17HIP_OK || r == M17HIP_ETRUNC || r == M17HIP_EOVERFLOW) && mine > c->compact.size()) {
                const hipError_t e = c->compact.grow(std::max<uint64_t>(mine + mine / 8, 1024), &c->last_hip);
                r = e != hipSuccess ? alloc_code(c, e) : compact_into(c, c->compact, c->compact.size(), &mine);
            }
            overflow = r == M17HIP_EOVERFLOW;
            if (r && !overflow) { local = r; mine = 0; }
        }
        src = c->compact;
        return local;
    };
    return gather_impl(c, m, root, sizeof(FrameRec), prepare, recs, capacity, counts_host, total_out, dest_is_device);
}

int m17hip_gather_frames(m17hip_ctx* c, m17hip_comm* m, int root, m17_frame_rec* recs_host, uint64_t capacity, uint64_t* counts_host, uint64_t* total_out)
{
    return gather_frames_impl(c, m, root, recs_host, capacity, counts_host, total_out, false);
}
int m17hip_gather_frames_device(m17hip_ctx* c, m17hip_comm* m, int root, m17_frame_rec* recs_dev, uint64_t capacity, uint64_t* counts_host, uint64_t* total_out)
{
    return gather_frames_impl(c, m, root, recs_dev, capacity, counts_host, total_out, true);
}


int m17hip_gather_sweep_stats(m17hip_ctx* c, m17hip_comm* m, int root, const m17_chan_stat* mine_host, uint64_t n_mine, m17_chan_stat* out_host,
                              uint64_t capacity, uint64_t* counts_host, uint64_t* total_out)
{
    if (n_mine && !mine_host) return M17HIP_EINVAL;
    // this rank's words (the caller's: a rank may have processed its shard in several runs), uploaded to the payload stream's buffer
    auto prepare = [c, mine_host, n_mine](const void*& src, uint64_t& mine, bool& overflow) {
        overflow = false;
        mine = 0;
        src = nullptr;
        if (c->gather_fault == 1) return (int)M17HIP_EHIP;
        if (n_mine) {
            if (int r = ensure_chan_words(c, n_mine)) return r;
            hipError_t e = hipMemcpyAsync(c->chan_words, mine_host, (size_t)n_mine * sizeof(ChanStat), hipMemcpyHostToDevice, c->pay());
            if (e == hipSuccess) e = hipStreamSynchronize(c->pay());   // (the caller's memory is not read once the call has returned, whatever happens in it)
            if (e != hipSuccess) return alloc_code(c, e);
        }
        src = c->chan_words;
        mine = n_mine;
        return (int)M17HIP_OK;
    };
    return gather_impl(c, m, root, sizeof(ChanStat), prepare, out_host, capacity, counts_host, total_out, false);
}

int m17hip_comm_last_error(const m17hip_comm* m) { return m ? m->last_rccl : 0; }

int m17hip_replay_drops(m17hip_ctx* c, uint64_t* count)
{
    if (!c || !count) return M17HIP_EINVAL;
    GUARD(c);
    OvfWords ovf;
    HIPCHK(c, ovf.read(c->overflow, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *count = ovf.replay_drops();
    return M17HIP_OK;
}

int m17hip_tune(m17hip_ctx* c, int key, int64_t value)
{
    if (!c) return M17HIP_EINVAL;
    GUARD(c);
    if (c->front_queued) return M17HIP_ESTATE;
    switch (key) {
    // ---- deployment knobs (include/m17hip.h) ----------------------------------------------------------------------------------
    case 3:  // samples per K2+K5 segment of a run (0 = whole run)
        if (value < 0 || value > 0x7FFFFFFF) return M17HIP_EINVAL;
        c->seg_len = (uint32_t)value;
        return M17HIP_OK;
    case 6:  // BERT statistics (m17hip_bert_stats) on/off (the runs made so far keep the setting they were made with)
        c->bert.on = value != 0;
        return M17HIP_OK;
    case 7:  // packet reassembly (m17hip_packets_fetch): room for `value` completed packets per run, 0 = off
        if (value < 0 || value > (1 << 24)) return M17HIP_EINVAL;
        if (int r = quiesce_payload(c, false)) return r;
        return c->packets.configure(c, (uint32_t)value);
    case 34:  // voice consumer (m17hip_voice_fetch, m17hip_calls_fetch): `value` voice slots per channel and run, 0 = off
        if (value < 0 || value > 65536) return M17HIP_EINVAL;
        if (int r = quiesce_payload(c, false)) return r;
        return c->voice.configure(c, (uint32_t)value);
    case 8:  // record slots per channel and run actually used (0 = all that were allocated): exercises M17HIP_EOVERFLOW
        if (value < 0 || value > (int64_t)c->rec_cap_alloc) return M17HIP_EINVAL;
        c->rec_cap = value ? (uint32_t)value : c->rec_cap_alloc;   // (the sets keep the layout they were written with: a finished run's records stay fetchable)
        return M17HIP_OK;
    case 9:  // diagnostic log: room for `value` diagnostic callbacks per channel and run, 0 = off (m17hip_diag_log_fetch)
        if (value < 0 || value > (1 << 20)) return M17HIP_EINVAL;
        if (int r = quiesce_payload(c, true)) return r;
        return c->diag.configure(c, (uint32_t)value);
    case 10:  // K3 form: 0 = one wave per 32 channels (throughput), 1 = four-wave pipeline (latency), -1 (default) = the pipeline for the runs m17hip_demod_front queues
        if (value < -1 || value > 1) return M17HIP_EINVAL;
        c->dcd_form = (int)value;
        return M17HIP_OK;
    case 20:  // redo policy of the limit-filter replay: 0 (default) = beside K5, state only; 1 = in front of K5, history stored
        if (value < 0 || value > 1) return M17HIP_EINVAL;
        c->redo_form = (int)value;
        return M17HIP_OK;
    case 17:  // RunningStandardDeviation (the EVM of the diagnostic callback) folded outside K5, one lane per channel (1, default), or inside K5 (0)
        if ((value != 0) != c->defer_evm) {
            if (int fr = flush_fold(c)) return fr;
            HIPCHK(c, hipStreamSynchronize(c->stream));
            c->defer_evm = value != 0;
            hipLaunchKernelGGL(ev_move_kernel, dim3((c->maxC + 63) / 64), dim3(64), 0, c->stream, c->seq_state, c->evm.state, c->maxC, c->defer_evm ? 1 : 0);
            HIPCHK(c, hipGetLastError());
            if (!c->defer_evm) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->evm.release(&c->last_hip); }
        }
        return M17HIP_OK;
    case 18:  // (tests) floats per channel row of deferred EVM operations, 0 = what a run of max_samples can produce: a smaller value makes the overflow flag reachable
        if (value < 0 || value > (1 << 28) || (value & 3)) return M17HIP_EINVAL;
        if (int fr = flush_fold(c)) return fr;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->evm.release(&c->last_hip); c->evm.set_pitch((uint32_t)value);
        return M17HIP_OK;
    case 15:  // payload frames of running stream / BERT transmissions decoded after the run, one lane per frame (1, default), or in K5 (0)
        c->defer_decode = value != 0;
        if (!c->defer_decode && c->defer_hist) {   // give the stores back (a run in flight may still use them: wait for it)
            if (int r = quiesce_payload(c, false)) return r;
            for (auto& rs_ : c->sets) rs_.defer_llr.release(&c->last_hip);
            c->defer_hist.release(&c->last_hip);
        }
        return M17HIP_OK;
    case 30:  // fault injection for m17hip_gather_frames (tests): 0 = none, 1 = this rank's compaction fails, 2 = the root's staging allocation fails,
              // 3 = this rank's word of exchange 2 cannot be written (its slot keeps the word of exchange 1) and the root's staging is grown,
              // 4 = this rank cannot read exchange 1, 5 = this rank cannot read exchange 2
        if (value < 0 || value > 5) return M17HIP_EINVAL;
        c->gather_fault = (int)value;
        return M17HIP_OK;
    case 31:  // bound, in milliseconds, of every wait inside m17hip_gather_frames[_device] (default 120000; 0 = wait for ever): a wait that runs out
              // gives the communicator up (ncclCommAbort) and the call returns M17HIP_ECOMM, as does every later call through that communicator
        if (value < 0 || value > 0x7FFFFFFF) return M17HIP_EINVAL;
        c->gather_timeout_ms = (uint32_t)value;
        return M17HIP_OK;
    case 16:  // the in-place producers (m17hip_upload_i16, m17hip_upload_i16_device, m17hip_synth_i16) write the STAGING slab instead
        c->stage_inputs = value != 0;
        return M17HIP_OK;
    case 26:  // gate-aware front end: 1 = K1 of segment k >= 2 skips what the carrier cannot be on for, 0 = never, -1 (default) = per run from the previous run's share of closed gates
        if (value < -1 || value > 1) return M17HIP_EINVAL;
        c->gate_aware = (int)value;
        return M17HIP_OK;
    case 33:  // ramp of segment lengths at the start of a run: value, 2 x value, 4 x value, ... samples, then seg_len (0 = none, -1 = per run)
        if (value < -1 || value > 0x7FFFFFFF) return M17HIP_EINVAL;
        c->seg_ramp = value;
        return M17HIP_OK;
    case 13:  // workgroups of K1's bounded grid (0 = default)
        if (value < 0 || value > (1 << 20)) return M17HIP_EINVAL;
        c->fir_grid = (uint32_t)value;
        return M17HIP_OK;
#ifdef M17_TOOLS
    case 27:  // configs[1]'s limit filter: 1 (default) = limit_relay_kernel, 0 = round 4's limit_pipe_kernel
        if (value < 0 || value > 1) return M17HIP_EINVAL;
        c->limit_form = (int)value;
        return M17HIP_OK;
    case 11:  // K1 form: 1 (default) = skewed pairs on a bounded grid, 0 = round 4's rolled R = 15 form with one workgroup per tile
        if (value < 0 || value > 1) return M17HIP_EINVAL;
        c->fir_form = (int)value;
        return M17HIP_OK;
    // ---- measurement / experiment knobs: only in the tools build (make -C csrc tools -> libm17hip_tools.so), used by tools/*.py ------
    case 1:  // section timers and counters of the sequential kernel (PROF instantiation; one segment per run) -> m17hip_debug_counters
        c->profile = value != 0;
        return M17HIP_OK;
    case 19:  // per-wave working time of the sequential kernel, per segment (TIMED instantiation): m17hip_debug_counters slot = segment
        c->wave_times = value != 0;
        return M17HIP_OK;
    case 4:  // samples of the first segment of a run (0 = like the others)
        if (value < 0 || value > 0x7FFFFFFF) return M17HIP_EINVAL;
        c->seg0_len = (uint32_t)value;
        return M17HIP_OK;
    case 5:  // segments the front end may run ahead of K5 (0 = unlimited)
        if (value < 0 || value > 1000) return M17HIP_EINVAL;
        c->front_ahead = (uint32_t)value;
        return M17HIP_OK;
    case 12:  // segments of K1 complete before the first K5 (0 / 1 = its own only)
        if (value < 0 || value > 1000) return M17HIP_EINVAL;
        c->front_first = (uint32_t)value;
        return M17HIP_OK;
    case 14:  // LDS bytes per workgroup of the sequential kernel (at least its need: decides how many of them share a CU), 0 = default
        if (value < 0 || value > 65536) return M17HIP_EINVAL;
        c->seq_lds_bytes = (uint32_t)value;
        return M17HIP_OK;
    case 21:  // the matched filter of a staged run waits for K5 of this segment (1-based) of the run before it (0 = starts at once)
        if (value < 0 || value > 1000) return M17HIP_EINVAL;
        c->front_k1_after = (uint32_t)value;
        return M17HIP_OK;
    case 40: case 41: case 42: case 43: {   // pipe-layout experiments (tools/pipe_layout.py): the K3 / K1 / replay / copy stream replaced by the caller's (value = hipStream_t)
        hipStream_t* slot[4] = {&c->side, &c->side2, &c->side3, &c->copy};
        const int r = key - 40;
        HIPCHK(c, hipDeviceSynchronize());
        if (*slot[r] && !c->foreign_streams[r]) hipStreamDestroy(*slot[r]);
        *slot[r] = (hipStream_t)(uintptr_t)value;
        c->foreign_streams[r] = true;
        return M17HIP_OK;
    }
    case 25:  // 1 (default) = m17hip_demod_front also queues the replay of the staged run's first segment (beside the current run's deferred decode)
        if (value != 0 && value != 1) return M17HIP_EINVAL;
        c->gate0_early = (int)value;
        return M17HIP_OK;
#endif
    default: return M17HIP_EINVAL;
    }
}

int m17hip_debug_counters(m17hip_ctx* c, uint64_t* host, uint32_t max_waves, uint32_t* waves)
{
    if (!c || !host || !waves) return M17HIP_EINVAL;
    GUARD(c);
    const uint32_t n = std::min(max_waves, c->dbg_waves);
    HIPCHK(c, hipMemcpy(host, c->dbg, (size_t)n * DBG_SLOTS * sizeof(uint64_t), hipMemcpyDeviceToHost));
    *waves = n;
    return M17HIP_OK;
}

int m17hip_timing_enable(m17hip_ctx* c, int on)
{
    if (!c) return M17HIP_EINVAL;
    GUARD(c);
    drain_timing(c);
    c->timing = on != 0;
    return M17HIP_OK;
}
int m17hip_timing_get(m17hip_ctx* c, int which, double* total_ms, uint64_t* launches)
{
    if (!c || which < 0 || which >= KT_N) return M17HIP_EINVAL;
    GUARD(c);
    drain_timing(c);
    if (total_ms) *total_ms = c->acc_ms[which];
    if (launches) *launches = c->acc_n[which];
    return M17HIP_OK;
}
int m17hip_timing_reset(m17hip_ctx* c)
{
    if (!c) return M17HIP_EINVAL;
    GUARD(c);
    drain_timing(c);
    for (int k = 0; k < KT_N; ++k) { c->acc_ms[k] = 0; c->acc_n[k] = 0; }
    return M17HIP_OK;
}

}  // extern "C"
