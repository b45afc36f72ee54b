// TEST INFRASTRUCTURE ONLY: the oracle's demodulator (oracle/m17_oracle_demod.hpp, DemodulatorT<OracleOps>) with CALLER-CHOSEN matched-filter taps — Fir150
// holds its taps as a member — stepped on float32 samples (what M17Demodulator<float>::operator()(float) receives) or on int16 samples through scale_sample.
// What m17hip_set_fir_taps (include/m17hip.h, a test hook) makes the device compute.  Records, the last m17_diag and the diagnostic log of every channel of a
// batch, laid out like the oracle's C entry points, and — for the premises tests/test_crafted.py asserts — taps into the machine: every symbol, every call of
// update_values, and per input sample the state the sample met, the limit filter and the four sync words' triggered() values.
// Built and loaded by tests/crafted_lib.py (g++ -O2 -ffp-contract=off).
#include "../../oracle/m17_oracle_demod.hpp"

#include <atomic>
#include <thread>

using namespace m17o;

extern "C" {

struct cro_frame_rec {   // include/m17hip.h `m17_frame_rec`
    uint32_t channel, seq;
    uint64_t sample_pos;
    int32_t cost;
    uint8_t frame_type, sync_type, len, flags;
    uint8_t payload[32];
    uint8_t pad[8];
};
static_assert(sizeof(cro_frame_rec) == 64, "record must be 64 bytes");
struct cro_diag {        // include/m17hip.h `m17_diag`
    int32_t dcd;
    float evm, deviation, offset;
    int32_t locked;
    float clock;
    int32_t sample_index, sync_index, clock_index, viterbi_cost;
    float dcd_level;
    uint32_t n_diag, demod_state, n_frames;
    uint32_t pad[2];
};
static_assert(sizeof(cro_diag) == 64, "diag must be 64 bytes");

// Everything one channel can hand back; any pointer may be null.  Per-sample planes are T long, the lists hold at most their capacity (counts go on).
struct cro_out {
    cro_frame_rec* recs; size_t cap; uint32_t* count;
    cro_diag* diag;
    cro_diag* log; size_t log_cap; uint32_t* log_count;
    uint32_t* sym_pos; float* sym; /* [sym_cap][2]: normalised, filtered */ size_t sym_cap; uint32_t* sym_count;
    uint32_t* lev_pos; float* lev; /* [lev_cap][4]: mn, mx, idev and offset after the update */ size_t lev_cap; uint32_t* lev_count;
    uint8_t* state;     // [T] what sample n met: bits 0-2 the state, 3 dcd_, 4 missing_sync_count >= 1920 (do_unlocked's second half), 5 sync_count >= 77
                        //     (a *_SYNC state then searches: its nine-sample window), 6 the sample went through the matched filter and the correlator
    uint8_t* cidx;      // [T] Correlator::index() after the sample
    float* limit;       // [T] Correlator::limit() after the sample
    float* trig;        // [T][4] SyncWord::triggered of preamble, LSF, packet, EOT after the sample (0 where bit 6 is clear)
    float* y;           // [T] the matched filter's output (0 where bit 6 is clear)
};

}

static void put_diag(cro_diag& o, const Diag& g, uint32_t state, uint32_t n_frames)
{
    std::memset(&o, 0, sizeof(o));
    o.dcd = g.dcd; o.evm = g.evm; o.deviation = g.deviation; o.offset = g.offset; o.locked = g.locked; o.clock = g.clock;
    o.sample_index = g.sample_index; o.sync_index = g.sync_index; o.clock_index = g.clock_index; o.viterbi_cost = g.viterbi_cost;
    o.dcd_level = g.dcd_level; o.n_diag = g.n_diag; o.demod_state = state; o.n_frames = n_frames;
}

// The demodulator with a window on the filter's output: Fir150 with the taps of the caller, remembering what it last returned.
struct TapFir : Fir150 {
    float last = 0.f;
    float step(float in) { last = Fir150::step(in); return last; }
};
struct TapOps : OracleOps { using Fir = TapFir; };
using TapDemod = DemodulatorT<TapOps>;

static void run_one(const float* xf, const int16_t* xi, size_t n, const float* taps150, int invert, uint32_t channel, const cro_out& o)
{
    std::vector<FrameRecord> out;
    auto d = std::make_unique<TapDemod>();
    if (taps150) for (int i = 0; i < 150; ++i) d->fir.taps[i] = taps150[i];
    d->out = &out;
    TapDemod* dp = d.get();
    size_t nl = 0, ns = 0, nv = 0;
    if (o.log || o.log_count)
        d->on_diag = [&](uint64_t pos, const Diag& g) {
            if (o.log && nl < o.log_cap) {
                put_diag(o.log[nl], g, (uint32_t)dp->st, (uint32_t)out.size());
                o.log[nl].pad[0] = (uint32_t)pos; o.log[nl].pad[1] = (uint32_t)(pos >> 32);
            }
            ++nl;
        };
    if (o.sym || o.sym_count)
        d->on_symbol = [&](uint64_t pos, float s, float f) {
            if (o.sym && ns < o.sym_cap) { o.sym_pos[ns] = (uint32_t)pos; o.sym[2 * ns] = s; o.sym[2 * ns + 1] = f; }
            ++ns;
        };
    size_t nv_done = 0;
    if (o.lev || o.lev_count)
        d->on_levels = [&](uint64_t pos, float mn, float mx) {
            if (o.lev && nv < o.lev_cap) { o.lev_pos[nv] = (uint32_t)pos; o.lev[4 * nv] = mn; o.lev[4 * nv + 1] = mx; }
            ++nv;
        };
    for (size_t i = 0; i < n; ++i) {
        const bool through = d->initializing != 0 || d->dcd_;
        if (o.state)
            o.state[i] = (uint8_t)((uint8_t)d->st | (d->dcd_ ? 8 : 0) | (d->missing_sync_count >= 1920 ? 16 : 0) | (d->sync_count >= 77 ? 32 : 0) |
                                   (through ? 64 : 0));
        d->step(xf ? (invert ? -xf[i] : xf[i]) : scale_sample(xi[i], invert != 0));
        for (; nv_done < nv; ++nv_done)   // (what the estimator made of the levels this sample handed it)
            if (o.lev && nv_done < o.lev_cap) { o.lev[4 * nv_done + 2] = d->dev.idev(); o.lev[4 * nv_done + 3] = d->dev.offset(); }
        if (o.cidx) o.cidx[i] = (uint8_t)d->corr.index();
        if (o.limit) o.limit[i] = d->corr.limit();
        if (o.y) o.y[i] = through ? d->fir.last : 0.f;
        if (o.trig) {
            float* t = o.trig + 4 * i;
            t[0] = through ? d->preamble_sync.triggered(d->corr) : 0.f;
            t[1] = through ? d->lsf_sync.triggered(d->corr) : 0.f;
            t[2] = through ? d->packet_sync.triggered(d->corr) : 0.f;
            t[3] = through ? d->eot_sync.triggered(d->corr) : 0.f;
        }
        d->pos++;
    }
    size_t cnt = 0;
    for (auto& f : out) {
        if (o.recs && cnt < o.cap) {
            cro_frame_rec& r = o.recs[cnt];
            std::memset(&r, 0, sizeof(r));
            r.channel = channel; r.seq = (uint32_t)cnt; r.sample_pos = f.sample_pos; r.cost = f.cost;
            r.frame_type = f.frame_type; r.sync_type = f.sync_type; r.len = f.len;
            std::memcpy(r.payload, f.data, 30);
        }
        cnt++;
    }
    if (o.diag) {
        put_diag(*o.diag, d->diag, (uint32_t)d->st, (uint32_t)cnt);
        o.diag->pad[0] = (uint32_t)d->clock.count;   // live counters at the end of the run, as the oracle's and the HIP path's
        o.diag->pad[1] = ((uint32_t)d->sync_count & 0xFFFFu) | ((uint32_t)d->missing_sync_count << 16);
    }
    if (o.count) *o.count = (uint32_t)cnt;
    if (o.log_count) *o.log_count = (uint32_t)nl;
    if (o.sym_count) *o.sym_count = (uint32_t)ns;
    if (o.lev_count) *o.lev_count = (uint32_t)nv;
}

extern "C" {

// The ungated filter with the caller's taps over float rows (state starts at zero): y[C][T].  Under invert the sample is negated.
void cro_fir(const float* x, size_t C, size_t T, const float* taps150, const uint8_t* invert, float* y)
{
    for (size_t c = 0; c < C; ++c) {
        Fir150 f;
        for (int i = 0; i < 150; ++i) f.taps[i] = taps150[i];
        const bool inv = invert && invert[c];
        for (size_t i = 0; i < T; ++i) y[c * T + i] = f.step(inv ? -x[c * T + i] : x[c * T + i]);
    }
}
// the float an int16 sample becomes (apps/m17-demod.cpp:489), for the int16 rows of cro_fir's callers
void cro_scale(const int16_t* s, size_t n, float* out)
{
    for (size_t i = 0; i < n; ++i) out[i] = scale_sample(s[i], false);
}

// Batch: x[C][T] float32 (is_i16 = 0) or int16 (is_i16 = 1), taps150 (nullptr: the RRC taps), invert[C] (nullptr: none); `base` describes channel 0's
// outputs and `step[k]` is the distance in ELEMENTS from one channel's k-th array to the next one's, in the order of cro_out's pointers:
// recs, count, diag, log, log_count, sym_pos, sym, sym_count, lev_pos, lev, lev_count, state, cidx, limit, trig, y.
void cro_demod_batch(const void* x, int is_i16, size_t C, size_t T, const float* taps150, const uint8_t* invert, int threads, const cro_out* base,
                     const size_t* step)
{
    std::atomic<size_t> next{0};
    auto worker = [&]() {
        for (;;) {
            const size_t c = next.fetch_add(1);
            if (c >= C) break;
            cro_out o = *base;
            auto at = [c](auto* p, size_t s) { return p ? p + c * s : p; };
            o.recs = at(o.recs, step[0]); o.count = at(o.count, step[1]); o.diag = at(o.diag, step[2]); o.log = at(o.log, step[3]);
            o.log_count = at(o.log_count, step[4]); o.sym_pos = at(o.sym_pos, step[5]); o.sym = at(o.sym, step[6]); o.sym_count = at(o.sym_count, step[7]);
            o.lev_pos = at(o.lev_pos, step[8]); o.lev = at(o.lev, step[9]); o.lev_count = at(o.lev_count, step[10]); o.state = at(o.state, step[11]);
            o.cidx = at(o.cidx, step[12]); o.limit = at(o.limit, step[13]); o.trig = at(o.trig, step[14]); o.y = at(o.y, step[15]);
            run_one(is_i16 ? nullptr : (const float*)x + c * T, is_i16 ? (const int16_t*)x + c * T : nullptr, T, taps150, invert ? invert[c] : 0, (uint32_t)c, o);
        }
    };
    if (threads <= 1) { worker(); return; }
    std::vector<std::thread> th;
    for (int i = 0; i < threads; ++i) th.emplace_back(worker);
    for (auto& t : th) t.join();
}

// Census of ClockRecovery's roundings (ClockRecovery.h: std::round in update(index) and update()) over a batch: per channel out[c][0] = calls,
// out[c][1] = calls whose argument's fraction is exactly 0.5, out[c][2] = the smallest | fraction - 0.5 | seen (1 if none).
void cro_clock_census(const void* x, int is_i16, size_t C, size_t T, const float* taps150, int threads, double* out)
{
    std::atomic<size_t> next{0};
    auto worker = [&]() {
        for (;;) {
            const size_t c = next.fetch_add(1);
            if (c >= C) break;
            auto d = std::make_unique<TapDemod>();
            if (taps150) for (int i = 0; i < 150; ++i) d->fir.taps[i] = taps150[i];
            size_t seen = 0, exact = 0;
            double best = 1.0;
            for (size_t i = 0; i < T; ++i) {
                d->step(is_i16 ? scale_sample(((const int16_t*)x)[c * T + i], false) : ((const float*)x)[c * T + i]);
                d->pos++;
                if (d->clock.n_round != seen) {   // (at most one rounding per sample)
                    seen = d->clock.n_round;
                    const double a = d->clock.round_arg, dist = std::fabs((a - std::floor(a)) - 0.5);
                    if (dist == 0.0) ++exact;
                    if (dist < best) best = dist;
                }
            }
            out[3 * c] = (double)seen; out[3 * c + 1] = (double)exact; out[3 * c + 2] = best;
        }
    };
    std::vector<std::thread> th;
    for (int i = 0; i < std::max(threads, 1); ++i) th.emplace_back(worker);
    for (auto& t : th) t.join();
}

}
