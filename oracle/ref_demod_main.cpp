// ORACLE — TEST INFRASTRUCTURE ONLY.
// The REFERENCE's own demodulator, mobilinkd::M17Demodulator<float>, compiled from its headers where they lie over this project's
// blaze stand-in (oracle/blaze_min, -DBLAZE_MIN_ORDER=k) into oracle/_ref/m17ref_demod_o<k> by oracle/Makefile.  No reference
// source is copied into this repository.
//
//   m17ref_demod_o<k> <samples.i16> <invert 0|1> <out.bin>
//
// ONE CHANNEL PER PROCESS: `initializing` and the EOT flag of the reference are function statics.  The object is
// placement-new'ed into zero-filled storage (Q4), <stdlib.h> comes before the reference's headers (Q5), and the samples are fed
// as the reference's application feeds them (m17o::scale_sample): negated as int16 when inverted, then float(double(s) / 41067.0).
//
// out.bin: uint64 n_frames, uint64 n_diag, then n_frames 64-byte frame records, then n_diag 64-byte diagnostic records
// (tests/oracle_lib.py FRAME_REC and DIAG).  sample_pos / pad = index of the sample being processed when the callback ran; n_diag
// counts from 1; sync_type, dcd_level, demod_state and n_frames are no arguments of the reference's callbacks and stay 0.
#include <stdlib.h>
#include <math.h>

#include "M17Demodulator.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

bool display_lsf = false;  // M17FrameDecoder.h declares it extern

static_assert(std::is_same<decltype(abs(1.0f)), float>::value, "abs(float) must be the float overload (Q5)");

using namespace mobilinkd;

namespace {

struct frame_rec {
    uint32_t channel, seq;
    uint64_t sample_pos;
    int32_t cost;
    uint8_t frame_type, sync_type, len, flags;
    uint8_t payload[32];
    uint8_t pad[8];
};
struct diag_rec {
    int32_t dcd; float evm, deviation, offset; int32_t locked; float clock; int32_t sample_index, sync_index, clock_index, viterbi_cost;
    float dcd_level; uint32_t n_diag, demod_state, n_frames, pad[2];
};
static_assert(sizeof(frame_rec) == 64 && sizeof(diag_rec) == 64, "record layouts");

using Demod = M17Demodulator<float>;
alignas(64) unsigned char g_storage[sizeof(Demod)];

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: %s samples.i16 invert out.bin\n", argv[0]); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    std::vector<int16_t> s;
    int16_t buf[4096];
    for (size_t n; (n = std::fread(buf, 2, 4096, in)) != 0;) s.insert(s.end(), buf, buf + n);
    std::fclose(in);
    const bool invert = std::atoi(argv[2]) != 0;

    std::vector<frame_rec> frames;
    std::vector<diag_rec> diags;
    uint64_t pos = 0;

    std::memset(g_storage, 0, sizeof(g_storage));
    Demod* d = new (g_storage) Demod([&](const M17FrameDecoder::output_buffer_t& ob, int cost) {
        frame_rec r;
        std::memset(&r, 0, sizeof(r));
        r.seq = (uint32_t)frames.size(); r.sample_pos = pos; r.cost = cost; r.frame_type = (uint8_t)ob.type;
        switch (ob.type) {
        case M17FrameDecoder::FrameType::LSF: r.len = 30; std::memcpy(r.payload, ob.lsf.data(), 30); break;
        case M17FrameDecoder::FrameType::LICH: r.len = 6; std::memcpy(r.payload, ob.lich.data(), 6); break;
        case M17FrameDecoder::FrameType::STREAM: r.len = 18; std::memcpy(r.payload, ob.stream.data(), 18); break;
        case M17FrameDecoder::FrameType::BERT: r.len = 25; std::memcpy(r.payload, ob.bert.data(), 25); break;
        default: r.len = 26; std::memcpy(r.payload, ob.packet.data(), 26); break;
        }
        frames.push_back(r);
        return true;
    });
    d->diagnostics([&](bool dcd, float evm, float deviation, float offset, bool locked, float clock, int sample_index, int sync_index,
                       int clock_index, int viterbi_cost) {
        diag_rec g;
        std::memset(&g, 0, sizeof(g));
        g.dcd = dcd; g.evm = evm; g.deviation = deviation; g.offset = offset; g.locked = locked; g.clock = clock;
        g.sample_index = sample_index; g.sync_index = sync_index; g.clock_index = clock_index; g.viterbi_cost = viterbi_cost;
        g.n_diag = (uint32_t)diags.size() + 1;
        g.pad[0] = (uint32_t)pos; g.pad[1] = (uint32_t)(pos >> 32);
        diags.push_back(g);
    });

    for (pos = 0; pos < s.size(); ++pos) {
        const int16_t v = invert ? (int16_t)(s[pos] * -1) : s[pos];
        (*d)((float)((double)v / 41067.0));
    }
    d->~Demod();

    std::FILE* out = std::fopen(argv[3], "wb");
    if (!out) { std::perror(argv[3]); return 2; }
    const uint64_t head[2] = {frames.size(), diags.size()};
    bool ok = std::fwrite(head, 8, 2, out) == 2;
    ok = ok && std::fwrite(frames.data(), 64, frames.size(), out) == frames.size();
    ok = ok && std::fwrite(diags.data(), 64, diags.size(), out) == diags.size();
    ok = (std::fclose(out) == 0) && ok;
    return ok ? 0 : 1;
}
