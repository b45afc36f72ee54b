// Test driver of BatchedDemodulator::reset_channels (tests/test_channel_reset_args.py builds it, tests/test_gpu_channel_reset.py runs it):
//   reset_channels_check <in.i16> <channels> <samples per run> <out.recs> <channel> [<channel> ...]
// in: [channels][2 x samples] int16.  Run 0 over the first half, the listed channels reset, run 1 over the second half;
// out: the 64-byte records of run 0, then those of run 1; the two counts go to stdout.
#include "BatchedDemodulator.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const uint32_t C = (uint32_t)std::atoi(argv[2]), T = (uint32_t)std::atoi(argv[3]);
    std::vector<int16_t> x((size_t)C * 2 * T);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(x.data(), 2, x.size(), f) != x.size()) return 3;
    std::fclose(f);
    std::vector<uint32_t> list;
    for (int i = 5; i < argc; ++i) list.push_back((uint32_t)std::atoi(argv[i]));
    try {
        mobilinkd::BatchedDemodulator d(C, T);
        FILE* o = std::fopen(argv[4], "wb");
        if (!o) return 4;
        size_t n[2];
        for (int r = 0; r < 2; ++r) {
            if (r == 1) d.reset_channels(list.data(), (uint32_t)list.size());
            d.upload(x.data() + (size_t)r * T, C, T, 2 * (size_t)T);
            d.run();
            const std::vector<m17_frame_rec> recs = d.frames();
            n[r] = recs.size();
            if (n[r] && std::fwrite(recs.data(), sizeof(m17_frame_rec), n[r], o) != n[r]) return 5;
        }
        std::fclose(o);
        std::printf("%zu %zu\n", n[0], n[1]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
