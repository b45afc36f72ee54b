// Test driver of BatchedDemodulator::enable_voice / voice / calls (tests/test_voice_log.py builds it, tests/test_gpu_voice.py runs it):
//   voice_check <in.i16> <channels> <samples> <room>
// in: [channels][samples] int16.  One run with the voice consumer on; stdout: per channel its slot count, the marks in hex and the first audio
// frame in hex (or "-"), then one line per closed call: channel seq start end frames blanked lost cost_sum has_lsf close.
#include "BatchedDemodulator.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 5) return 2;
    const uint32_t C = (uint32_t)std::atoi(argv[2]), T = (uint32_t)std::atoi(argv[3]);
    const int room = std::atoi(argv[4]);
    if (C == 0 || T == 0 || room <= 0 || room > 65536) return 2;
    std::vector<int16_t> x((size_t)C * T);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(x.data(), 2, x.size(), f) != x.size()) return 3;
    std::fclose(f);
    try {
        mobilinkd::BatchedDemodulator d(C, T);
        d.enable_voice((uint32_t)room);
        d.upload(x.data(), C, T, (size_t)T);
        d.run();
        const mobilinkd::BatchedDemodulator::Voice v = d.voice();
        for (uint32_t c = 0; c < C; ++c) {
            std::printf("%u %u ", c, v.counts[c]);
            for (uint32_t s = 0; s < v.counts[c]; ++s) std::printf("%02x", v.mark(c, s));
            std::printf(v.counts[c] ? " " : "- ");
            if (!v.counts[c]) std::printf("-");
            else for (unsigned k = 0; k < 16; ++k) std::printf("%02x", v.frame(c, 0)[k]);
            std::printf("\n");
        }
        for (const m17_call_rec& r : d.calls())
            std::printf("call %u %u %llu %llu %u %u %u %u %u %u\n", r.channel, r.seq, (unsigned long long)r.start_pos, (unsigned long long)r.end_pos, r.frames,
                        r.blanked, r.lost, r.cost_sum, (unsigned)r.has_lsf, (unsigned)r.close);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
