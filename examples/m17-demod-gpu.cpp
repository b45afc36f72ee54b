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
// centre, dB over the floor); with --spectrum N [--hop H, default N] under ANY wideband option the averaged N-point periodogram of each block is
// computed on the device and the carriers it shows — the rule of m17hip's Python wide_spectrum_carriers: 9 kHz bands, more than --scan-margin dB over the
// median floor — are printed to stderr with the offset in Hz that --offset-hz takes: rtl_sdr -s 2048000 ... | m17-demod-gpu --wide-u8 --rate 2048000
// --spectrum 2048; with --meter W (16 to 65536 outputs; 1920 is one M17 frame) under ANY wideband option the channel's level, its carrier's offset from
// the tuned frequency and its deviation are measured on the device per window of W outputs and printed to stderr after each block; with --squelch DB
// [--hang N] beside --spectrum and a tuner (not --raster) the first block runs unsquelched, its plane's median sets the floor of a 9 kHz band, and from
// the second block on the channel is tuned only while its band stands DB dB over that floor (it stays open down to DB - 3 dB and for N more blocks), and
// is fed zeros otherwise; each decision is printed to stderr; with --slots [--lead N] beside --squelch the decision is taken per slot of 16 frames of the
// block's spectrum and the tuner skips per tile of its outputs (--hang then counts slots, --lead N opens the tiles up to N slots in front of an opening),
// so a transmission that begins inside a block is kept from its start; the tiles tuned are printed per block; with --auto-floor [--rise A] [--fall A]
// beside --squelch the floor is taken on the device from every block's own plane and tracked (towards a higher floor by A, towards a lower one by A, each
// in (0, 1], default 1), so the first block is squelched too and a floor that moves is followed; the floor is printed in dB per block; with --scan-pool N
// beside --rate, --squelch and --auto-floor a pool of N channels is tuned by the carrier scan on the device, each transmission from the block in which it
// first appears (rtl_sdr -s 2048000 ... | m17-demod-gpu --wide-u8 --rate 2048000 --spectrum 2048 --squelch 10 --auto-floor --scan-pool 8): the
// assignments and misses are printed per block, the frames with their channel in front.  One line per frame callback on
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

// The carriers of one source's spectrum plane at `rate` samples per second, as m17hip.wide_spectrum_carriers finds them (m17hip/__init__.py): band power
// over `width` Hz, the floor the median times the band's bins, peaks greedily, strongest first, each excluding +-width around itself and a taken peak's
// shoulders passed over, the offset refined to the centroid over the median.  (offset Hz, dB over the floor), strongest first.
static std::vector<std::pair<double, double>> carriers(const std::vector<float>& power, double rate, double width, double margin_db)
{
    const long N = (long)power.size();
    std::vector<std::pair<double, double>> out;
    std::vector<double> sorted(power.begin(), power.end());
    std::sort(sorted.begin(), sorted.end());
    const double med = 0.5 * (sorted[(N - 1) / 2] + sorted[N / 2]);
    if (!(med > 0.0) || !std::isfinite(med)) return out;
    const double df = rate / N;
    const long h = std::min<long>(std::lround(width / 2.0 / df), (N - 1) / 2), excl = (long)std::ceil(width / df);
    const auto at = [&](long k) { return (double)power[(size_t)(((k % N) + N) % N)]; };
    std::vector<double> band(N);
    for (long k = 0; k < N; ++k) { double b = 0.0; for (long d = -h; d <= h; ++d) b += at(k + d); band[k] = b; }
    const double floor = med * (2 * h + 1), need = floor * std::pow(10.0, margin_db / 10.0);
    std::vector<char> free_(N);
    for (long k = 0; k < N; ++k) free_[k] = std::isfinite(band[k]);
    for (;;) {
        long k = -1;
        for (long i = 0; i < N; ++i) if (free_[i] && (k < 0 || band[i] > band[k])) k = i;
        if (k < 0 || !(band[k] > need)) break;
        long j = k;
        for (;;) {   // uphill, half a band at a time
            long m = j;
            for (long d = -h; d <= h; ++d) { const long i = (((j + d) % N) + N) % N; if (band[i] > band[m]) m = i; }
            if (m == j) break;
            j = m;
        }
        if (j != k) { free_[k] = 0; continue; }
        double sw = 0.0, sdw = 0.0;
        for (long d = -h; d <= h; ++d) { const double w = std::max(at(k + d) - med, 0.0); sw += w; sdw += d * w; }
        const double c = (double)(k < N / 2 ? k : k - N) + (sw > 0.0 ? sdw / sw : 0.0);
        double hz = std::fmod(c * df + rate / 2.0, rate);
        if (hz < 0.0) hz += rate;
        out.emplace_back(hz - rate / 2.0, 10.0 * std::log10(band[k] / floor));
        for (long d = -excl; d <= excl; ++d) free_[(size_t)((((k + d) % N) + N) % N)] = 0;
    }
    std::sort(out.begin(), out.end(), [](const auto& a, const auto& b) { return a.second > b.second; });
    return out;
}

// --scan-pool N beside --rate HZ --spectrum P --squelch DB --auto-floor: a pool of N channels on the one source, all seeded at --offset-hz, tuned by the
// carrier scan on the device (m17hip_wide_scan) in blocks of 4800 outputs (100 ms).  Per block the assignments and the misses are printed to stderr, the
// assigned channels are reset before the block's run (the reset rule of include/m17hip.h), and every frame is printed with its channel in front.
static int scan_pool_main(int wide, uint32_t rate, double offset_hz, uint32_t points, uint32_t hop, double squelch_db, uint32_t hang, float rise, float fall,
                          uint32_t pool, float iq_gain)
{
    using namespace mobilinkd;
    uint32_t d1, up, down;
    BatchedDemodulator::wide_resample_ratio(rate, d1, up, down);
    const uint32_t block = 4800 / (192 * up) * (192 * up);   // (whole groups of `up` outputs and whole ticks of 192: the listed reset's rule)
    const size_t W = (size_t)block / up * down * d1, bytes = wide == M17HIP_IQ_F32 ? 8 : wide == M17HIP_IQ_I16 ? 4 : 2;
    BatchedDemodulator gpu(pool, block);
    gpu.wide_resample(1, d1, up, down, wide);
    const int32_t seed = (int32_t)(uint32_t)std::llround(offset_hz / (double)rate * 4294967296.0);
    std::vector<uint32_t> src(pool, 0u);
    std::vector<int32_t> words(pool, seed);
    gpu.wide_channels(src.data(), words.data(), pool);
    gpu.reset();
    gpu.wide_spectrum(points, hop);
    const double df = (double)rate / points;
    const uint32_t half = std::min<uint32_t>((uint32_t)std::lrint(9000.0 / 2.0 / df), std::min<uint32_t>(64u, points / 2 - 1));
    const uint32_t guard = std::max<uint32_t>(3u, std::min<uint32_t>((uint32_t)std::ceil(9000.0 / df), points / 4));
    gpu.wide_squelch(half, {1.0f}, {1.0f}, hang);
    gpu.wide_squelch_floor((float)std::pow(10.0, squelch_db / 10.0), (float)std::pow(10.0, (squelch_db - 3.0) / 10.0), rise, fall);
    gpu.wide_scan(std::vector<uint8_t>(pool, 1), guard);
    std::vector<char> buf(W * bytes);
    std::vector<uint32_t> flags, missed, assigned;
    for (uint64_t b = 0;; ++b) {
        std::cin.read(buf.data(), (std::streamsize)buf.size());
        const size_t got = (size_t)std::cin.gcount() / bytes / ((size_t)down * d1) * ((size_t)down * d1);   // (whole groups; what is left over at the end is dropped)
        if (!got) break;
        gpu.upload_wide(buf.data(), pool, (uint32_t)(got / ((size_t)down * d1) * up), got, iq_gain);
        gpu.wide_scan_fetch(0, words, flags, missed, &assigned);   // (waits for the block's scan kernel, not for its tuner)
        for (const uint32_t c : assigned)
            std::fprintf(stderr, "scan: block %llu, channel %u assigned %.1f Hz\n", (unsigned long long)b, c, (double)words[c] * (double)rate / 4294967296.0);
        if (missed[0]) std::fprintf(stderr, "scan: block %llu, %u carriers found no free slot\n", (unsigned long long)b, missed[0]);
        if (!assigned.empty()) gpu.reset_channels(assigned.data(), (uint32_t)assigned.size());
        gpu.run();
        for (const auto& r : gpu.frames()) {
            static const size_t len[] = {30, 6, 18, 26, 26, 25};
            std::printf("%u %d %d ", r.channel, (int)r.frame_type, (int)r.cost);
            for (size_t i = 0; i < (r.frame_type < 6 ? len[r.frame_type] : 26); ++i) std::printf("%02x", r.payload[i]);
            std::printf("\n");
        }
        if (!std::cin) break;
    }
    return 0;
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
    bool margin_given = false;
    uint32_t spectrum = 0, hop = 0;   // (spectrum == 0: none; hop == 0: the points)
    uint32_t meter = 0;               // (0: no meter)
    double squelch_db = 0.0;          // (--squelch: dB over the floor; hang in blocks)
    bool squelch = false;
    uint32_t hang = 0;
    bool slots = false;               // (--slots: per slot and tile; --lead in slots)
    uint32_t lead = 0;
    bool auto_floor = false;          // (--auto-floor: the floor from each block's plane, on the device; --rise and --fall track it)
    float rise = 1.0f, fall = 1.0f;
    bool track_given = false;
    uint32_t scan_pool = 0;           // (--scan-pool N: N channels tuned by the carrier scan on the device)
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
        else if (!std::strcmp(argv[i], "--scan-margin") && i + 1 < argc) { scan_margin = std::strtod(argv[++i], nullptr); margin_given = true; }
        else if (!std::strcmp(argv[i], "--spectrum") && i + 1 < argc) { spectrum = (uint32_t)std::strtoul(argv[++i], nullptr, 10); if (!spectrum) spectrum = 1; }
        else if (!std::strcmp(argv[i], "--meter") && i + 1 < argc) { meter = (uint32_t)std::strtoul(argv[++i], nullptr, 10); if (!meter) meter = 1; }
        else if (!std::strcmp(argv[i], "--squelch") && i + 1 < argc) { squelch_db = std::strtod(argv[++i], nullptr); squelch = true; }
        else if (!std::strcmp(argv[i], "--hang") && i + 1 < argc) hang = (uint32_t)std::strtoul(argv[++i], nullptr, 10);
        else if (!std::strcmp(argv[i], "--slots")) slots = true;
        else if (!std::strcmp(argv[i], "--lead") && i + 1 < argc) { lead = (uint32_t)std::strtoul(argv[++i], nullptr, 10); if (!lead) lead = ~0u; }
        else if (!std::strcmp(argv[i], "--auto-floor")) auto_floor = true;
        else if (!std::strcmp(argv[i], "--scan-pool") && i + 1 < argc) { scan_pool = (uint32_t)std::strtoul(argv[++i], nullptr, 10); if (!scan_pool) scan_pool = ~0u; }
        else if (!std::strcmp(argv[i], "--rise") && i + 1 < argc) { rise = std::strtof(argv[++i], nullptr); track_given = true; }
        else if (!std::strcmp(argv[i], "--fall") && i + 1 < argc) { fall = std::strtof(argv[++i], nullptr); track_given = true; }
        else if (!std::strcmp(argv[i], "--hop") && i + 1 < argc) { hop = (uint32_t)std::strtoul(argv[++i], nullptr, 10); if (!hop) hop = ~0u; }
        else {
            std::fprintf(stderr, "usage: m17-demod-gpu [-f | --float32 | --iq-i16 | --iq-f32 | --wide-i16 | --wide-f32 | --wide-u8] [--decim R [--decim2 R2] | --rate HZ] [--offset-hz F | --raster M --bin B [--scan STRIDE [--scan-margin DB]]] [--spectrum N [--hop H] [--squelch DB [--hang N] [--slots [--lead N]] [--auto-floor [--rise A] [--fall A] [--scan-pool N]]]] [--meter W] [--iq-gain G] < samples\n");
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
    if (meter && (!wide || meter < 16 || meter > 65536)) { std::fprintf(stderr, "m17-demod-gpu: --meter W (16 to 65536 outputs) goes with a wideband format\n"); return 2; }
    if ((squelch || hang) && (!squelch || !spectrum || raster || !(squelch_db > 0.0) || hang > 65535)) {
        std::fprintf(stderr, "m17-demod-gpu: --squelch DB (above 0) [--hang N (0 to 65535 blocks)] goes with --spectrum and a tuner, not with --raster\n");
        return 2;
    }
    if ((slots || lead) && (!squelch || !slots || (lead && lead > 255))) {
        std::fprintf(stderr, "m17-demod-gpu: --slots [--lead N (1 to 255 slots)] goes with --squelch\n");
        return 2;
    }
    if ((auto_floor || track_given) && (!squelch || !auto_floor || !(rise > 0.0f) || !(rise <= 1.0f) || !(fall > 0.0f) || !(fall <= 1.0f))) {
        std::fprintf(stderr, "m17-demod-gpu: --auto-floor [--rise A] [--fall A] (each above 0, 1 at the most) goes with --squelch\n");
        return 2;
    }
    if (spectrum || hop) {
        if (!hop) hop = spectrum;
        if (!wide || spectrum < 64 || spectrum > 4096 || (spectrum & (spectrum - 1)) || hop > (1u << 24)) {
            std::fprintf(stderr, "m17-demod-gpu: --spectrum N (a power of two, 64 to 4096) [--hop H (1 to 16777216)] goes with a wideband format\n");
            return 2;
        }
    }
    if (scan_pool) {
        if (!rate || !auto_floor || slots || meter || scan_pool > 256) {
            std::fprintf(stderr, "m17-demod-gpu: --scan-pool N (1 to 256 channels) goes with --rate, --spectrum, --squelch and --auto-floor, without --slots and --meter\n");
            return 2;
        }
        return scan_pool_main(wide, (uint32_t)rate, offset_hz, spectrum, hop, squelch_db, hang, rise, fall, scan_pool, iq_gain);
    }
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
        if (spectrum) {   // the carriers of the one source after each block
            const double fs = 2.0 * half_hz, margin = margin_given ? scan_margin : 10.0;
            const bool on = demod.wide_spectrum(spectrum, hop, [=](const std::vector<float>& power, uint32_t frames, uint64_t first_sample) {
                std::fprintf(stderr, "spectrum: samples from %llu, %u frames\n", (unsigned long long)first_sample, frames);
                for (const auto& c : carriers(power, fs, 9000.0, margin)) std::fprintf(stderr, "spectrum: carrier %+.1f Hz %.2f dB\n", c.first, c.second);
            });
            if (!on) std::fprintf(stderr, "m17-demod-gpu: --spectrum needs the GPU path (it runs on the device); no spectrum\n");
        }
        if (squelch) {   // the first block unsquelched: its plane sets the levels (--auto-floor: none is, the device takes every block's floor)
            const double fs = 2.0 * half_hz;
            const uint32_t h = std::min<uint32_t>((uint32_t)std::lrint(9000.0 / 2.0 / (fs / spectrum)), std::min<uint32_t>(64u, spectrum / 2 - 1));
            const bool on = slots ? demod.wide_squelch_slots(h, squelch_db, squelch_db - 3.0, hang, lead, [](uint32_t open_tiles, uint32_t tiles, uint32_t nslots, uint32_t frames) {
                std::fprintf(stderr, "squelch: %u of %u tiles open, %u slots over %u frames\n", open_tiles, tiles, nslots, frames);
            }) : demod.wide_squelch(h, squelch_db, squelch_db - 3.0, hang, [](bool open, uint32_t hold, float band, uint32_t frames) {
                std::fprintf(stderr, "squelch: %s, hold %u, band %.6g over %u frames\n", open ? "open" : "closed", hold, (double)band, frames);
            });
            if (!on) std::fprintf(stderr, "m17-demod-gpu: --squelch needs the GPU path (it runs on the device); no squelch\n");
            if (on && auto_floor)   // the floor of every block on the device: the first block is squelched too
                demod.wide_squelch_floor(squelch_db, squelch_db - 3.0, rise, fall, [](float floor, float open_level, float, uint32_t frames) {
                    std::fprintf(stderr, "floor: %.2f dB per frame and band, open at %.2f dB, %u frames\n", 10.0 * std::log10((double)floor),
                                 10.0 * std::log10((double)open_level), frames);
                });
        }
        if (meter) {   // level, offset and deviation of the one channel per window of the feed (a window a block cuts comes in two pieces)
            const bool on = demod.wide_meter(meter, [](uint64_t window, uint32_t outputs, double level_db, double offset_hz, double deviation_hz) {
                std::fprintf(stderr, "meter: window %llu, %u outputs: level %.2f dB, offset %+.1f Hz, deviation %.1f Hz\n", (unsigned long long)window, outputs,
                             level_db, offset_hz, deviation_hz);
            });
            if (!on) std::fprintf(stderr, "m17-demod-gpu: --meter needs the GPU path (it runs on the device); no meter\n");
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
