// f32_mirror_check in.f32 [block]: the GPU-backed M17Demodulator<float> and its scalar_cpu form fed the SAME float samples, one per call; every callback
// of both (frame type, cost, payload; the diagnostic arguments with their floats as bit patterns) in order.  Exit status 0 and "ok <frames> <diagnostics>"
// when the two sequences are equal, 1 and the first difference otherwise.  (tests/test_gpu_f32_input.py)
#include "M17Demodulator.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

bool display_lsf = false;
using namespace mobilinkd;

static std::vector<std::string> run(const std::vector<float>& in, bool on_gpu, uint32_t block, size_t& n_frames, size_t& n_diag)
{
    std::vector<std::string> out;
    n_frames = n_diag = 0;
    {
        auto on_frame = [&](M17FrameDecoder::output_buffer_t const& f, int cost) {
            const uint8_t* p = nullptr; size_t n = 0;
            switch (f.type) {
            case M17FrameDecoder::FrameType::LSF: p = f.lsf.data(); n = 30; break;
            case M17FrameDecoder::FrameType::LICH: p = f.lich.data(); n = 6; break;
            case M17FrameDecoder::FrameType::STREAM: p = f.stream.data(); n = 18; break;
            case M17FrameDecoder::FrameType::BERT: p = f.bert.data(); n = 25; break;
            default: p = f.packet.data(); n = 26; break;
            }
            char head[64];
            std::snprintf(head, sizeof head, "F %d %d ", (int)f.type, cost);
            std::string line = head;
            for (size_t i = 0; i < n; ++i) { char b[4]; std::snprintf(b, sizeof b, "%02x", p[i]); line += b; }
            out.push_back(line);
            ++n_frames;
            return true;
        };
        std::unique_ptr<M17Demodulator<float>> dp;
        if (on_gpu) dp = std::make_unique<M17Demodulator<float>>(on_frame, block);
        else dp = std::make_unique<M17Demodulator<float>>(on_frame, scalar_cpu);
        dp->diagnostics([&](bool dcd, float evm, float dev, float off, bool locked, float clock, int si, int sy, int ci, int vc) {
            uint32_t w[4]; std::memcpy(&w[0], &evm, 4); std::memcpy(&w[1], &dev, 4); std::memcpy(&w[2], &off, 4); std::memcpy(&w[3], &clock, 4);
            char line[160];
            std::snprintf(line, sizeof line, "D %d %08x %08x %08x %d %08x %d %d %d %d", (int)dcd, w[0], w[1], w[2], (int)locked, w[3], si, sy, ci, vc);
            out.push_back(line);
            ++n_diag;
        });
        for (float x : in) (*dp)(x);
    }   // the destructor flushes the last partial block
    return out;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: f32_mirror_check in.f32 [block]\n"); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<float> in(raw.size() / sizeof(float));
    std::memcpy(in.data(), raw.data(), in.size() * sizeof(float));
    const uint32_t block = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 1920u;
    size_t cf, cd, gf, gd;
    const auto cpu = run(in, false, block, cf, cd);
    const auto gpu = run(in, true, block, gf, gd);
    for (size_t i = 0; i < cpu.size() || i < gpu.size(); ++i) {
        const std::string a = i < cpu.size() ? cpu[i] : "(none)", b = i < gpu.size() ? gpu[i] : "(none)";
        if (a != b) {
            std::printf("callback %zu differs\n  scalar_cpu: %s\n  gpu:        %s\n", i, a.c_str(), b.c_str());
            return 1;
        }
    }
    std::printf("ok %zu %zu\n", gf, gd);
    return 0;
}
