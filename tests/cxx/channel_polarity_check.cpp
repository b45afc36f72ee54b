// Test driver of BatchedDemodulator::set_channel_polarity (tests/test_channel_polarity_args.py builds it, tests/test_gpu_channel_polarity.py runs it):
//   channel_polarity_check <in.i16> <channels> <samples> <pattern>
// in: [channels][samples] int16; pattern: one character 0 / 1 per channel.  One run under that table; stdout: the record count, then per channel
// the number of its records and the payload of its first one in hex (or "-").
#include "BatchedDemodulator.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 5) return 2;
    const uint32_t C = (uint32_t)std::atoi(argv[2]), T = (uint32_t)std::atoi(argv[3]);
    if (C == 0 || T == 0 || std::strlen(argv[4]) != C) return 2;
    std::vector<uint8_t> pol(C);
    for (uint32_t c = 0; c < C; ++c) {
        if (argv[4][c] != '0' && argv[4][c] != '1') return 2;
        pol[c] = (uint8_t)(argv[4][c] - '0');
    }
    std::vector<int16_t> x((size_t)C * T);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(x.data(), 2, x.size(), f) != x.size()) return 3;
    std::fclose(f);
    try {
        mobilinkd::BatchedDemodulator d(C, T);
        d.set_channel_polarity(pol.data(), C);
        d.upload(x.data(), C, T, (size_t)T);
        d.run();
        const std::vector<m17_frame_rec> recs = d.frames();
        std::printf("%zu\n", recs.size());
        for (uint32_t c = 0; c < C; ++c) {
            size_t n = 0;
            const m17_frame_rec* first = nullptr;
            for (const m17_frame_rec& r : recs)
                if (r.channel == c) { if (!first) first = &r; ++n; }
            std::printf("%u %zu ", c, n);
            if (!first) std::printf("-");
            else for (unsigned k = 0; k < first->len; ++k) std::printf("%02x", first->payload[k]);
            std::printf("\n");
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
