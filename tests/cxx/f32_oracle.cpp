// TEST INFRASTRUCTURE ONLY: the oracle's demodulator (oracle/m17_oracle_demod.hpp, DemodulatorT<OracleOps>) stepped on FLOAT samples — what the
// reference's M17Demodulator<float>::operator()(float) receives — instead of on int16 through scale_sample.  Records, the last m17_diag and the diagnostic
// log of one channel and of a batch, laid out like the oracle's C entry points (run_channel_t / diag_log_t are the models); under invert the sample is
// negated, which is exact.  Built and loaded by tests/f32_lib.py (g++ -O2 -ffp-contract=off).
#include "../../oracle/m17_oracle_demod.hpp"

#include <atomic>
#include <thread>

using namespace m17o;

extern "C" {

struct f32o_frame_rec {   // include/m17hip.h `m17_frame_rec`
    uint32_t channel, seq;
    uint64_t sample_pos;
    int32_t cost;
    uint8_t frame_type, sync_type, len, flags;
    uint8_t payload[32];
    uint8_t pad[8];
};
static_assert(sizeof(f32o_frame_rec) == 64, "record must be 64 bytes");
struct f32o_diag {        // include/m17hip.h `m17_diag`
    int32_t dcd;
    float evm, deviation, offset;
    int32_t locked;
    float clock;
    int32_t sample_index, sync_index, clock_index, viterbi_cost;
    float dcd_level;
    uint32_t n_diag, demod_state, n_frames;
    uint32_t pad[2];
};
static_assert(sizeof(f32o_diag) == 64, "diag must be 64 bytes");

}

static void put_diag(f32o_diag& o, const Diag& g, uint32_t state, uint32_t n_frames)
{
    std::memset(&o, 0, sizeof(o));
    o.dcd = g.dcd; o.evm = g.evm; o.deviation = g.deviation; o.offset = g.offset; o.locked = g.locked; o.clock = g.clock;
    o.sample_index = g.sample_index; o.sync_index = g.sync_index; o.clock_index = g.clock_index; o.viterbi_cost = g.viterbi_cost;
    o.dcd_level = g.dcd_level; o.n_diag = g.n_diag; o.demod_state = state; o.n_frames = n_frames;
}

static void feed(Demodulator& d, const float* x, size_t n, bool invert)
{
    for (size_t i = 0; i < n; ++i) { d.step(invert ? -x[i] : x[i]); d.pos++; }
}

// one channel: records (at most cap written; the count is returned), the last diagnostic callback, optionally every diagnostic callback
static size_t run_f32(const float* x, size_t n, int invert, uint32_t channel, f32o_frame_rec* recs, size_t cap, f32o_diag* diag, f32o_diag* log, size_t log_cap,
                      size_t* n_log)
{
    std::vector<FrameRecord> out;
    auto d = std::make_unique<Demodulator>();
    d->out = &out;
    size_t nl = 0;
    Demodulator* dp = d.get();
    if (log || n_log)
        d->on_diag = [&](uint64_t pos, const Diag& g) {
            if (log && nl < log_cap) {
                put_diag(log[nl], g, (uint32_t)dp->st, (uint32_t)out.size());
                log[nl].pad[0] = (uint32_t)pos; log[nl].pad[1] = (uint32_t)(pos >> 32);
            }
            ++nl;
        };
    feed(*d, x, n, invert != 0);
    size_t cnt = 0;
    for (auto& f : out) {
        if (recs && cnt < cap) {
            f32o_frame_rec& r = recs[cnt];
            std::memset(&r, 0, sizeof(r));
            r.channel = channel; r.seq = (uint32_t)cnt; r.sample_pos = f.sample_pos; r.cost = f.cost;
            r.frame_type = f.frame_type; r.sync_type = f.sync_type; r.len = f.len;
            std::memcpy(r.payload, f.data, 30);
        }
        cnt++;
    }
    if (diag) {
        put_diag(*diag, d->diag, (uint32_t)d->st, (uint32_t)cnt);
        diag->pad[0] = (uint32_t)d->clock.count;   // live counters at the end of the run, as the oracle's and the HIP path's
        diag->pad[1] = ((uint32_t)d->sync_count & 0xFFFFu) | ((uint32_t)d->missing_sync_count << 16);
    }
    if (n_log) *n_log = nl;
    return cnt;
}

extern "C" {

// evaluation order of the Kalman updates (m17_oracle_dsp.hpp; process-wide in THIS library: set it before a batch, put 3 back after)
void f32o_set_kalman_order(int order) { kalman_order() = order & 7; }

size_t f32o_demod(const float* x, size_t n, int invert, f32o_frame_rec* recs, size_t cap, f32o_diag* diag)
{
    return run_f32(x, n, invert, 0, recs, cap, diag, nullptr, 0, nullptr);
}
size_t f32o_diag_log(const float* x, size_t n, int invert, f32o_diag* log, size_t cap)
{
    size_t nl = 0;
    run_f32(x, n, invert, 0, nullptr, 0, nullptr, log, cap, &nl);
    return nl;
}
// Batch: x[C][T] (row pitch in samples); invert[C] per channel (nullptr: none); recs[C][cap], counts[C], diags[C]; logs[C][log_cap], log_counts[C]
// (both may be nullptr).
void f32o_demod_batch(const float* x, size_t C, size_t T, size_t pitch, const uint8_t* invert, int threads, f32o_frame_rec* recs, size_t cap, uint32_t* counts,
                      f32o_diag* diags, f32o_diag* logs, size_t log_cap, uint32_t* log_counts)
{
    std::atomic<size_t> next{0};
    auto worker = [&]() {
        for (;;) {
            const size_t c = next.fetch_add(1);
            if (c >= C) break;
            size_t nl = 0;
            const size_t n = run_f32(x + c * pitch, T, invert ? invert[c] : 0, (uint32_t)c, recs ? recs + c * cap : nullptr, recs ? cap : 0,
                                     diags ? diags + c : nullptr, logs ? logs + c * log_cap : nullptr, log_cap, logs ? &nl : nullptr);
            if (counts) counts[c] = (uint32_t)n;
            if (log_counts) log_counts[c] = (uint32_t)nl;
        }
    };
    if (threads <= 1) { worker(); return; }
    std::vector<std::thread> th;
    for (int i = 0; i < threads; ++i) th.emplace_back(worker);
    for (auto& t : th) t.join();
}

}
