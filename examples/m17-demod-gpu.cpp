// A reference-style demodulator front end on the GPU path: 48 kSPS s16le mono on stdin (with -f / --float32: raw float32 in the
// reference's units — a discriminator's output, taken as it is: a float stream, nothing rounded; with --iq-i16 / --iq-f32: interleaved
// I,Q of the narrowband FM channel, int16 or float32, discriminated on the device with --iq-gain G, default 1; with --wide-i16 / --wide-f32 / --wide-u8
// --decim R --offset-hz F: interleaved I,Q of a WIDEBAND feed at 48000 R samples per second, the channel F Hz from its centre tuned, filtered, decimated and
// discriminated on the device — rtl_sdr -s 240000 ... | m17-demod-gpu --wide-u8 --decim 5 --offset-hz 12500; with --decim2 R2 as well the feed is at
// 48000 R R2 and decimated in two stages — rtl_sdr -s 2400000 ... | m17-demod-gpu --wide-u8 --decim 10 --decim2 5 --offset-hz 12500; with --rate HZ in place of
// --decim the feed runs at HZ samples per second, any rate m17hip_wide_resample_ratio has a shape for, and the second stage resamples —
// rtl_sdr -s 2048000 ... | m17-demod-gpu --wide-u8 --rate 2048000 --offset-hz 12500 (--rate excludes --decim, --decim2 and --raster); with --raster M --bin B in place of --offset-hz
// the feed at 48000 R (R up to 64) is split into M channels by the polyphase channeliser and bin B of them demodulated — rtl_sdr -s 2400000 ... |
// m17-demod-gpu --wide-u8 --decim 50 --raster 192 --bin 1; with --scan STRIDE beside --raster every STRIDE-th output of the feed is surveyed on the device
// and after each block the occupied bins — more than --scan-margin dB, default 20, over the median of the 192 — are printed to stderr: bin, Hz from the
// centre, dB over the floor), one line per frame callback on
// stdout.  It is written the way apps/m17-demod.cpp drives the reference (construct M17Demodulator<float> with a
// handle_frame callback, push sample / 41067.0 per sample) — audio (codec2) and the CLI options are out of scope.
//   g++ -std=c++20 -O2 examples/m17-demod-gpu.cpp -I m17-cxx-demod_amd/include -L m17-cxx-demod_amd -lm17hip -Wl,-rpath,... -o m17-demod-gpu
#include "m17cxx/M17Demodulator.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

bool display_lsf = false;  // the reference's M17FrameDecoder.h:19 expects the application to define this

static bool handle_frame(mobilinkd::M17FrameDecoder::output_buffer_t const& frame, int viterbi_cost)
{
    using FrameType = mobilinkd::M17FrameDecoder::FrameType;
    const uint8_t* p = nullptr;
    size_t n = 0;
    switch (frame.type) {
    case FrameType::LSF: p = frame.lsf.data(); n = 30; break;
    case FrameType::LICH: p = frame.lich.data(); n = 6; break;
    case FrameType::STREAM: p = frame.stream.data(); n = 18; break;
    case FrameType::BERT: p = frame.bert.data(); n = 25; break;
    default: p = frame.packet.data(); n = 26; break;
    }
    std::printf("%d %d ", (int)frame.type, viterbi_cost);
    for (size_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
    std::printf("\n");
    return true;
}

int main(int argc, char** argv)
{
    using namespace mobilinkd;
    bool float_input = false;
    int iq = 0;   // 1: int16 I,Q; 2: float32 I,Q
    int wide = 0;   // M17HIP_IQ_I16 / _F32 / _U8: a wideband feed of that format
    uint32_t decim = 1, decim2 = 0;   // (decim2 == 0: one stage)
    bool decim_given = false;
    unsigned long long rate = 0;      // (0: integer decimations)
    double offset_hz = 0.0;
    uint32_t raster = 0;   // (0: a tuner)
    long bin = 0;
    float iq_gain = 1.0f;
    uint32_t scan = 0;   // (0: no survey)
    double scan_margin = 20.0;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "-f") || !std::strcmp(argv[i], "--float32")) float_input = true;
        else if (!std::strcmp(argv[i], "--iq-i16")) iq = 1;
        else if (!std::strcmp(argv[i], "--iq-f32")) iq = 2;
        else if (!std::strcmp(argv[i], "--iq-gain") && i + 1 < argc) iq_gain = std::strtof(argv[++i], nullptr);
        else if (!std::strcmp(argv[i], "--wide-i16")) wide = M17HIP_IQ_I16;
        else if (!std::strcmp(argv[i], "--wide-f32")) wide = M17HIP_IQ_F32;
        else if (!std::strcmp(argv[i], "--wide-u8")) wide = M17HIP_IQ_U8;
        else if (!std::strcmp(argv[i], "--decim") && i + 1 < argc) { decim = (uint32_t)std::strtoul(argv[++i], nullptr, 10); decim_given = true; }
        else if (!std::strcmp(argv[i], "--rate") && i + 1 < argc) { rate = std::strtoull(argv[++i], nullptr, 10); if (!rate) rate = ~0ull; }
        else if (!std::strcmp(argv[i], "--decim2") && i + 1 < argc) { decim2 = (uint32_t)std::strtoul(argv[++i], nullptr, 10); if (!decim2) decim2 = 17; }
        else if (!std::strcmp(argv[i], "--offset-hz") && i + 1 < argc) offset_hz = std::strtod(argv[++i], nullptr);
        else if (!std::strcmp(argv[i], "--raster") && i + 1 < argc) { raster = (uint32_t)std::strtoul(argv[++i], nullptr, 10); if (!raster) raster = 257; }
        else if (!std::strcmp(argv[i], "--bin") && i + 1 < argc) bin = std::strtol(argv[++i], nullptr, 10);
        else if (!std::strcmp(argv[i], "--scan") && i + 1 < argc) { scan = (uint32_t)std::strtoul(argv[++i], nullptr, 10); if (!scan) scan = 4097; }
        else if (!std::strcmp(argv[i], "--scan-margin") && i + 1 < argc) scan_margin = std::strtod(argv[++i], nullptr);
        else {
            std::fprintf(stderr, "usage: m17-demod-gpu [-f | --float32 | --iq-i16 | --iq-f32 | --wide-i16 | --wide-f32 | --wide-u8] [--decim R [--decim2 R2] | --rate HZ] [--offset-hz F | --raster M --bin B [--scan STRIDE [--scan-margin DB]]] [--iq-gain G] < samples\n");
            return 2;
        }
    }
    if (((iq || wide) && float_input) || (iq && wide) || !(iq_gain > 0.0f) || !std::isfinite(iq_gain)) { std::fprintf(stderr, "m17-demod-gpu: one input format, and a finite gain > 0\n"); return 2; }
    const double half_hz = rate ? 0.5 * (double)rate : 24000.0 * decim * (decim2 ? decim2 : 1);
    if (rate) {
        uint32_t d1, up, down;
        if (!wide || decim_given || decim2 || raster || rate > 0xFFFFFFFFull || m17hip_wide_resample_ratio((uint32_t)rate, &d1, &up, &down) != M17HIP_OK ||
            !(std::fabs(offset_hz) <= half_hz)) {
            std::fprintf(stderr, "m17-demod-gpu: --rate HZ goes with a wideband format and without --decim, --decim2 and --raster; a rate of 48000 * decim1 * down / up "
                                 "(decim1 to 16, up to 32, down to 125) and an offset inside the feed\n");
            return 2;
        }
    } else if (wide && raster) {
        uint32_t m1, m2;
        if (decim < 1 || decim > 64 || decim2 || !core::chan_factor(raster, m1, m2) || bin < -(long)(raster / 2) || bin > (long)((raster - 1) / 2)) {
            std::fprintf(stderr, "m17-demod-gpu: a decimation of 1 to 64 in one stage, a raster that factors into two numbers up to 16, and a bin inside it\n");
            return 2;
        }
    } else if (wide && (decim < 1 || decim > 16 || decim2 > 16 || !(std::fabs(offset_hz) <= half_hz))) {
        std::fprintf(stderr, "m17-demod-gpu: decimations of 1 to 16, and an offset inside the +-%g Hz the feed covers\n", half_hz);
        return 2;
    }
    if (scan && (!(wide && raster) || scan > 4096)) { std::fprintf(stderr, "m17-demod-gpu: --scan STRIDE (1 to 4096) goes with --raster\n"); return 2; }
    M17Demodulator<float> demod(handle_frame);
    demod.diagnostics([](bool, float, float, float, bool, float, int, int, int, int) {});
    demod.iq_gain(iq_gain);
    while (iq == 1 && std::cin) {   // interleaved int16 I,Q at 48 kSPS: the discriminator runs on the device
        int16_t s[2];
        std::cin.read(reinterpret_cast<char*>(s), 4);
        if (!std::cin) break;
        demod.iq((float)s[0], (float)s[1]);
    }
    while (iq == 2 && std::cin) {
        float s[2];
        std::cin.read(reinterpret_cast<char*>(s), 8);
        if (!std::cin) break;
        demod.iq(s[0], s[1]);
    }
    if (iq) return 0;
    if (wide) {   // a wideband feed: the tuner runs on the device
        if (rate) demod.wide_rate((uint32_t)rate, offset_hz);
        else if (raster) demod.wide_raster(decim, raster, (int32_t)bin);
        else if (decim2) demod.wide_config(decim, decim2, offset_hz);
        else demod.wide_config(decim, offset_hz);
        if (scan) {   // the occupied bins of the one source after each block: the floor is the median of the plane
            const double spacing = 48000.0 * decim / raster;
            const bool on = demod.wide_survey(scan, [=](const std::vector<float>& power, uint32_t times, uint64_t first_output) {
                std::vector<float> sorted(power);
                std::sort(sorted.begin(), sorted.end());
                const size_t M = sorted.size();
                const double floor = M % 2 ? sorted[M / 2] : 0.5 * ((double)sorted[M / 2 - 1] + (double)sorted[M / 2]);
                std::fprintf(stderr, "scan: outputs from %llu, %u survey times\n", (unsigned long long)first_output, times);
                if (!(floor > 0.0) || !std::isfinite(floor)) return;
                for (size_t k = 0; k < M; ++k) {
                    const double db = 10.0 * std::log10((double)power[k] / floor);
                    const long b = k <= (M - 1) / 2 ? (long)k : (long)k - (long)M;
                    if (db > scan_margin) std::fprintf(stderr, "scan: bin %ld %+.1f Hz %.2f dB\n", b, b * spacing, db);
                }
            });
            if (!on) std::fprintf(stderr, "m17-demod-gpu: --scan needs the GPU path (the survey runs on the device); not surveying\n");
        }
        while (std::cin) {
            if (wide == M17HIP_IQ_I16) { int16_t s[2]; std::cin.read(reinterpret_cast<char*>(s), 4); if (std::cin) demod.wide((float)s[0], (float)s[1]); }
            else if (wide == M17HIP_IQ_F32) { float s[2]; std::cin.read(reinterpret_cast<char*>(s), 8); if (std::cin) demod.wide(s[0], s[1]); }
            else { uint8_t s[2]; std::cin.read(reinterpret_cast<char*>(s), 2); if (std::cin) demod.wide(core::ddc_u8(s[0]), core::ddc_u8(s[1])); }
        }
        return 0;
    }
    while (float_input && std::cin) {   // raw float32, native byte order: the value IS the demodulator's sample
        float sample;
        std::cin.read(reinterpret_cast<char*>(&sample), 4);
        if (!std::cin) break;
        demod(sample);
    }
    while (!float_input && std::cin) {
        int16_t sample;
        std::cin.read(reinterpret_cast<char*>(&sample), 2);
        if (!std::cin) break;
        demod(sample / 41067.0);
    }
    return 0;   // ~M17Demodulator() demodulates what is still buffered
}
