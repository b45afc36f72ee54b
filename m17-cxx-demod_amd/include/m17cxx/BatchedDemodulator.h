// C++ RAII face of the C ABI (include/m17hip.h) for C independent channels on one GPU.  What the reference does with
// one M17Demodulator<float> object per channel and one operator() call per sample (apps/m17-demod.cpp:455,484-490),
// this does with one context and one run() per block of samples.  Errors become std::runtime_error.
#pragma once

#include "../../../include/m17hip.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

namespace mobilinkd
{

class BatchedDemodulator
{
    m17hip_ctx* ctx_ = nullptr;
    uint32_t channels_ = 0, samples_ = 0, room_ = 0, diag_room_ = 0, voice_room_ = 0;
    uint64_t last_frames_ = 0;

    static void check(int code, const char* what)
    {
        if (code != M17HIP_OK) throw std::runtime_error(std::string(what) + ": " + m17hip_strerror(code));
    }

public:
    BatchedDemodulator(uint32_t max_channels, uint32_t max_samples, int device = 0)
    {
        // The HIP runtime reads GPU_MAX_HW_QUEUES when it initialises (a context's five streams must not share hardware queues,
        // include/m17hip.h m17hip_advice): ask for 16 unless the host has decided otherwise.  Effective when this is the process's
        // first contact with the GPU — the case of a host like apps/m17-demod.cpp; a host that has already used HIP sets it itself.
        ::setenv("GPU_MAX_HW_QUEUES", "16", /*overwrite*/0);
        check(m17hip_ctx_create(device, max_channels, max_samples, &ctx_), "m17hip_ctx_create");
        static bool warned = false;
        if ((m17hip_advice(ctx_) & M17HIP_ADVICE_HW_QUEUES) && !warned) {
            warned = true;
            std::fprintf(stderr, "m17hip: GPU_MAX_HW_QUEUES is below 8 (M17HIP_FEW_HW_QUEUES_OK was given): the context's streams will share hardware queues and serialise; "
                                 "export GPU_MAX_HW_QUEUES=16 before the process touches the GPU (include/m17hip.h)\n");
        }
    }
    ~BatchedDemodulator() { m17hip_ctx_destroy(ctx_); }
    BatchedDemodulator(const BatchedDemodulator&) = delete;
    BatchedDemodulator& operator=(const BatchedDemodulator&) = delete;

    m17hip_ctx* handle() const { return ctx_; }
    // the context's main stream (a hipStream_t; the library's own, non-blocking): what a host orders its own device work against
    void* stream() const { void* s = nullptr; check(m17hip_get_stream(ctx_, &s), "m17hip_get_stream"); return s; }

    // [channels][samples] int16, row pitch in samples
    void upload(const int16_t* host, uint32_t channels, uint32_t samples, size_t pitch)
    {
        check(m17hip_upload_i16(ctx_, host, channels, samples, pitch), "m17hip_upload_i16");
        channels_ = channels; samples_ = samples;
    }
    // float32 input in the reference's units (what M17Demodulator<float>::operator() receives), taken as it is: a float stream
    // (m17hip_upload_f32; the format belongs to the stream until the next reset())
    void upload(const float* host, uint32_t channels, uint32_t samples, size_t pitch)
    {
        check(m17hip_upload_f32(ctx_, host, channels, samples, pitch), "m17hip_upload_f32");
        channels_ = channels; samples_ = samples;
    }
    // Complex IQ input, one narrowband 48 kSPS stream per channel (m17hip_upload_iq): gain * arg(x[n] conj(x[n-1])) is computed on the device into
    // the float input slab — a float stream from there on.  [channels][samples] interleaved I,Q as complex<float> or as int16 pairs, row pitch in
    // complex samples.  IQ blocks continue one another per channel in call order; reset() / reset_channels() start a feed over.
    void upload_iq(const std::complex<float>* host, uint32_t channels, uint32_t samples, size_t pitch, float gain = 1.0f)
    {
        check(m17hip_upload_iq(ctx_, host, M17HIP_IQ_F32, gain, channels, samples, pitch), "m17hip_upload_iq");
        channels_ = channels; samples_ = samples;
    }
    void upload_iq(const int16_t (*host)[2], uint32_t channels, uint32_t samples, size_t pitch, float gain = 1.0f)
    {
        check(m17hip_upload_iq(ctx_, host, M17HIP_IQ_I16, gain, channels, samples, pitch), "m17hip_upload_iq");
        channels_ = channels; samples_ = samples;
    }
    // Wideband IQ input (m17hip_wide_config, m17hip_wide_channels, m17hip_upload_wide): `sources` wide streams at 48000 * decim, every channel tuned to
    // one of them on the device — mixed to its offset, low-passed with `taps` (none: the default taps), decimated and discriminated into the float input
    // slab.  A block is [sources][pitch] interleaved I,Q of the configured format with samples * decim complex samples per row; `samples` counts outputs.
    void wide_config(uint32_t sources, uint32_t decim, int iq_format = M17HIP_IQ_I16, const float* taps = nullptr, uint32_t ntaps = 0)
    {
        check(m17hip_wide_config(ctx_, sources, decim, iq_format, taps, ntaps), "m17hip_wide_config");
    }
    // The same in two stages, for sources above 16 x 48 kSPS (m17hip_wide_config2): 48000 * decim1 * decim2 samples per second, every row
    // samples * decim1 * decim2 complex samples; frequency words are wide_fcw(offset_hz, decim1 * decim2).  It and wide_config replace one another.
    void wide_config2(uint32_t sources, uint32_t decim1, uint32_t decim2, int iq_format = M17HIP_IQ_I16, const float* taps1 = nullptr, uint32_t ntaps1 = 0,
                      const float* taps2 = nullptr, uint32_t ntaps2 = 0)
    {
        check(m17hip_wide_config2(ctx_, sources, decim1, taps1, ntaps1, decim2, taps2, ntaps2, iq_format), "m17hip_wide_config2");
    }
    // The same with a second stage that resamples by up / down, for sources whose rate is no integer multiple of 48 kSPS (m17hip_wide_resample):
    // 48000 * decim1 * down / up samples per second (wide_resample_ratio finds the three for a rate), `samples` a multiple of `up`, every row
    // samples / up * down * decim1 complex samples; frequency words are wide_fcw_rate(offset_hz, rate_hz).  It and the other configurations replace one another.
    void wide_resample(uint32_t sources, uint32_t decim1, uint32_t up, uint32_t down, int iq_format = M17HIP_IQ_I16, const float* taps1 = nullptr,
                       uint32_t ntaps1 = 0, const float* taps2 = nullptr, uint32_t ntaps2 = 0)
    {
        check(m17hip_wide_resample(ctx_, sources, decim1, taps1, ntaps1, up, down, taps2, ntaps2, iq_format), "m17hip_wide_resample");
    }
    static void wide_resample_ratio(uint32_t rate_hz, uint32_t& decim1, uint32_t& up, uint32_t& down)
    {
        if (m17hip_wide_resample_ratio(rate_hz, &decim1, &up, &down) != M17HIP_OK) throw std::invalid_argument("wide_resample_ratio: no configuration has this rate");
    }
    // S sources split into `bins` channels each on a raster of 48000 * decim / bins Hz by the polyphase channeliser (m17hip_wide_raster; decim 1..64, every
    // row samples * decim complex samples); channels are named by wide_raster_channels(source, bin), wide_bin gives the bin of an offset.  It replaces
    // wide_config and wide_config2 and is replaced by them.
    void wide_raster(uint32_t sources, uint32_t decim, uint32_t bins, int iq_format = M17HIP_IQ_I16, const float* taps = nullptr, uint32_t ntaps = 0)
    {
        check(m17hip_wide_raster(ctx_, sources, decim, bins, iq_format, taps, ntaps), "m17hip_wide_raster");
    }
    void wide_raster_channels(const uint32_t* source, const int32_t* bin, uint32_t n)
    {
        check(m17hip_wide_raster_channels(ctx_, source, bin, n), "m17hip_wide_raster_channels");
    }
    // The raster survey (m17hip_wide_survey): from the blocks uploaded after the call every stride-th output of the feed (1..4096; 0: off) adds the power of
    // every bin of every source to the block's plane.  wide_survey_fetch: the plane [sources][bins] (indexed by bin mod bins) of the latest surveyed block
    // (back = 0) or the one before (back = 1), its survey times and the feed's output index at its start; it waits for that block's survey kernels only.
    void wide_survey(uint32_t stride) { check(m17hip_wide_survey(ctx_, stride), "m17hip_wide_survey"); }
    void wide_survey_fetch(uint32_t back, float* power, uint64_t capacity, uint32_t* times = nullptr, uint64_t* first_output = nullptr)
    {
        check(m17hip_wide_survey_fetch(ctx_, back, power, capacity, times, first_output), "m17hip_wide_survey_fetch");
    }
    // The source spectrum (m17hip_wide_spectrum), under every wideband configuration: from the blocks uploaded after the call the frames of `points` samples
    // (a power of two in 64..4096; 0: off) that begin where the feed's sample index is a multiple of `hop` (1..2^24) are windowed (nullptr with 0: the
    // default window), transformed and their powers summed per source.  wide_spectrum_fetch: the plane [sources][points] of the latest such block (back = 0)
    // or the one before (back = 1), its frames and the feed's sample index at its first frame; it waits for that block's spectrum kernels only.
    void wide_spectrum(uint32_t points, uint32_t hop, const float* window = nullptr, uint32_t nwindow = 0)
    {
        check(m17hip_wide_spectrum(ctx_, points, hop, window, nwindow), "m17hip_wide_spectrum");
    }
    void wide_spectrum_fetch(uint32_t back, float* power, uint64_t capacity, uint32_t* frames = nullptr, uint64_t* first_sample = nullptr)
    {
        check(m17hip_wide_spectrum_fetch(ctx_, back, power, capacity, frames, first_sample), "m17hip_wide_spectrum_fetch");
    }
    // The channel meter (m17hip_wide_meter), under every wideband configuration: from the blocks uploaded after the call the sums of chan_power(z), of the
    // discriminator's y and of y * y per channel and per window of `window` outputs of the feed (16..65536; 0: off).  wide_meter_fetch: the planes
    // [3][channels][pieces] of the latest such block (back = 0) or the one before (back = 1), resized to fit, with the block's shape — piece k belongs to
    // window first_window + k of the feed; it waits for that block's meter kernel only.
    void wide_meter(uint32_t window) { check(m17hip_wide_meter(ctx_, window), "m17hip_wide_meter"); }
    void wide_meter_fetch(uint32_t back, std::vector<float>& planes, uint32_t* channels = nullptr, uint32_t* pieces = nullptr, uint64_t* first_window = nullptr,
                          uint64_t* first_output = nullptr, uint32_t* outputs = nullptr)
    {
        uint32_t c = 0, k = 0;
        check(m17hip_wide_meter_shape(ctx_, back, &c, &k, first_window, first_output, outputs), "m17hip_wide_meter_shape");
        planes.resize((size_t)3 * c * k);
        check(m17hip_wide_meter_fetch(ctx_, back, planes.data(), planes.size()), "m17hip_wide_meter_fetch");
        if (channels) *channels = c;
        if (pieces) *pieces = k;
    }
    // The spectrum squelch of the three tuners (m17hip_wide_squelch; the spectrum must be on): from the blocks uploaded after the call a channel whose band
    // of 2 half_bins + 1 bins of the block's spectrum lies below open_level[source] x frames is not tuned (its floats are +0); an open one stays open down
    // to close_level[source] x frames and for `hang` blocks behind that.  One level pair per source; wide_squelch_off turns it off.  wide_squelch_fetch:
    // per channel of the latest such block (back = 0) or the one before (back = 1) the word h' | open << 31 and the band power, resized to fit; it waits for
    // that block's squelch kernel only.
    void wide_squelch(uint32_t half_bins, const std::vector<float>& open_level, const std::vector<float>& close_level, uint32_t hang = 0)
    {
        if (open_level.size() != close_level.size()) throw std::invalid_argument("wide_squelch: one open and one close level per source");
        check(m17hip_wide_squelch(ctx_, half_bins, open_level.data(), close_level.data(), (uint32_t)open_level.size(), hang), "m17hip_wide_squelch");
    }
    void wide_squelch_off() { check(m17hip_wide_squelch(ctx_, 0, nullptr, nullptr, 0, 0), "m17hip_wide_squelch"); }
    void wide_squelch_fetch(uint32_t back, std::vector<uint32_t>& state, std::vector<float>& band, uint32_t* frames = nullptr)
    {
        state.resize(channels_);
        band.resize(channels_);
        uint32_t n = 0;
        check(m17hip_wide_squelch_fetch(ctx_, back, state.data(), band.data(), state.size(), &n, frames), "m17hip_wide_squelch_fetch");
        state.resize(n);
        band.resize(n);
    }
    // The time-resolved mode of the squelch (m17hip_wide_squelch_slots), exclusive with wide_squelch's: a decision per slot of 16 frames of the block's
    // spectrum, `hang` in slots, and the tuners skip per tile of outputs; `lead` (0..255) opens the tiles in front of an opening within the block.
    // wide_squelch_off turns either mode off.  wide_squelch_slots_fetch: per channel the state word behind the block, the slots' band powers [channels][slots]
    // and the tile mask [channels][ceil(tiles / 32)] of the latest such block (back = 0) or the one before; it waits for that block's squelch kernels only.
    // The planes' sizes are the block's: the vectors are grown while the library refuses their capacity.
    void wide_squelch_slots(uint32_t half_bins, const std::vector<float>& open_level, const std::vector<float>& close_level, uint32_t hang = 0, uint32_t lead = 0)
    {
        if (open_level.size() != close_level.size()) throw std::invalid_argument("wide_squelch_slots: one open and one close level per source");
        check(m17hip_wide_squelch_slots(ctx_, half_bins, open_level.data(), close_level.data(), (uint32_t)open_level.size(), hang, lead), "m17hip_wide_squelch_slots");
    }
    void wide_squelch_slots_fetch(uint32_t back, std::vector<uint32_t>& state, std::vector<float>& bands, std::vector<uint32_t>& mask, uint32_t* slots = nullptr,
                                  uint32_t* tiles = nullptr, uint32_t* frames = nullptr)
    {
        state.resize(channels_);
        uint32_t n = 0, g = 0, t = 0, j = 0;
        int rc = M17HIP_EINVAL;
        for (size_t per = 64; per <= ((size_t)1 << 22); per *= 8) {
            bands.resize(channels_ * per);
            mask.resize(channels_ * per);
            rc = m17hip_wide_squelch_slots_fetch(ctx_, back, state.data(), bands.data(), mask.data(), state.size(), bands.size(), mask.size(), &n, &g, &t, &j);
            if (rc != M17HIP_EINVAL || back > 1) break;
        }
        check(rc, "m17hip_wide_squelch_slots_fetch");
        state.resize(n);
        bands.resize((size_t)n * g);
        mask.resize((size_t)n * ((t + 31) / 32));
        if (slots) *slots = g;
        if (tiles) *tiles = t;
        if (frames) *frames = j;
    }
    // The sources' noise floor on the device (m17hip_wide_squelch_floor), beside whichever squelch mode is on: from the blocks uploaded after the call each
    // source's levels are its tracked floor — the upper median of the block's own plane times 2 half_bins + 1 over the frames, at least floor_min, moved
    // by `rise` towards a higher floor and by `fall` towards a lower one (both in (0, 1]) — times open_ratio and close_ratio; the mode's given levels are
    // set aside.  wide_squelch_floor_off gives them back; every wide_squelch and wide_squelch_slots call turns it off as well.  wide_squelch_floor_fetch:
    // plane[4][sources] = median | floor | open level | close level of the latest such block (back = 0) or the one before; it waits for that block's floor
    // and squelch kernels only.
    void wide_squelch_floor(float open_ratio, float close_ratio, float rise = 1.0f, float fall = 1.0f, float floor_min = 0.0f)
    {
        check(m17hip_wide_squelch_floor(ctx_, open_ratio, close_ratio, rise, fall, floor_min), "m17hip_wide_squelch_floor");
    }
    void wide_squelch_floor_off() { check(m17hip_wide_squelch_floor(ctx_, 0.0f, 0.0f, 1.0f, 1.0f, 0.0f), "m17hip_wide_squelch_floor"); }
    void wide_squelch_floor_fetch(uint32_t back, std::vector<float>& plane, uint32_t* sources = nullptr, uint32_t* frames = nullptr)
    {
        plane.resize(4 * 256);
        uint32_t n = 0;
        check(m17hip_wide_squelch_floor_fetch(ctx_, back, plane.data(), plane.size(), &n, frames), "m17hip_wide_squelch_floor_fetch");
        plane.resize((size_t)4 * n);
        if (sources) *sources = n;
    }
    // The carrier scan (m17hip_wide_scan), beside wide_spectrum (at most 4096 points), wide_squelch and wide_squelch_floor: pool[c] != 0 makes channel c a
    // slot of the source its wide_channels entry names; from the blocks uploaded after the call a kernel in front of the squelch finds each source's
    // carriers in the block's own plane and tunes the source's slots that no carrier holds to them (guard_bins, 3 .. points / 4: the least distance of two
    // carriers).  wide_scan_off turns it off; so does everything that turns off what it needs.  wide_scan_fetch: the table the latest scanned block (back =
    // 0) or the one before was tuned with, per channel the flags 1 = slot, 2 = assigned in this block, 4 = held over, per source the carriers that found no
    // free slot; `assigned`, if given, gets the channels with flag 2 — THE CALLER LISTS THEM IN reset_channels BEFORE THE BLOCK'S run() (a freshly assigned
    // slot starts a transmission on a demodulator fed zeros).  It waits for that block's scan kernel only.
    void wide_scan(const std::vector<uint8_t>& pool, uint32_t guard_bins)
    {
        check(m17hip_wide_scan(ctx_, pool.data(), (uint32_t)pool.size(), guard_bins), "m17hip_wide_scan");
    }
    void wide_scan_off() { check(m17hip_wide_scan(ctx_, nullptr, 0, 0), "m17hip_wide_scan"); }
    void wide_scan_fetch(uint32_t back, std::vector<int32_t>& fcw, std::vector<uint32_t>& flags, std::vector<uint32_t>& missed,
                         std::vector<uint32_t>* assigned = nullptr, uint32_t* frames = nullptr)
    {
        fcw.resize(channels_); flags.resize(channels_); missed.resize(256);
        uint32_t n = 0, s = 0;
        check(m17hip_wide_scan_fetch(ctx_, back, fcw.data(), flags.data(), missed.data(), fcw.size(), &n, &s, frames), "m17hip_wide_scan_fetch");
        fcw.resize(n); flags.resize(n); missed.resize(s);
        if (assigned) {
            assigned->clear();
            for (uint32_t c = 0; c < n; ++c) if (flags[c] & 2u) assigned->push_back(c);
        }
    }
    // The wideband signal generator (m17hip_synth_wide_config): the int16 input slab's basebands FM-modulated into `sources` wide IQ streams at
    // 48000 * p / q samples per second.  k = 0: M17's deviation (wide_tx_k).  synth_wide_channels: channel c transmits as tx[c] says from the next block.
    // synth_wide: one block, W = samples / q * p complex samples per source into dst[sources][pitch] — host memory, or device memory with device = true —,
    // complete on return: an RX object's upload_wide_device may take it at once.
    static uint64_t wide_tx_k(uint32_t p, double hz_per_unit = 0.0)
    {
        uint64_t k = 0;
        if (m17hip_synth_wide_k(hz_per_unit, p, &k) != M17HIP_OK) throw std::invalid_argument("m17hip_synth_wide_k: no such deviation word");
        return k;
    }
    void synth_wide_config(uint32_t sources, uint32_t p, uint32_t q, int iq_format, uint64_t k = 0, float noise_sigma = 0.0f, uint64_t seed = 0,
                           uint64_t first_sample = 0)
    {
        check(m17hip_synth_wide_config(ctx_, sources, p, q, iq_format, k ? k : wide_tx_k(p), noise_sigma, seed, first_sample), "m17hip_synth_wide_config");
    }
    void synth_wide_channels(const m17_wide_tx* tx, uint32_t n) { check(m17hip_synth_wide_channels(ctx_, tx, n), "m17hip_synth_wide_channels"); }
    void synth_wide(void* dst, uint32_t channels, uint32_t samples, size_t pitch, bool device = false)
    {
        check(device ? m17hip_synth_wide_device(ctx_, dst, channels, samples, pitch) : m17hip_synth_wide(ctx_, dst, channels, samples, pitch),
              "m17hip_synth_wide");
    }
    // the bin of an offset in Hz from the source's centre; throws where the offset is not on the raster or outside it
    static int32_t wide_bin(double offset_hz, uint32_t decim, uint32_t bins)
    {
        const double b = offset_hz * bins / (48000.0 * decim);
        const double k = std::nearbyint(b);
        if (std::fabs(b - k) > 1e-9 * std::max(1.0, std::fabs(b)) || k < -(double)(bins / 2) || k > (double)((bins - 1) / 2))
            throw std::invalid_argument("wide_bin: the offset is not a channel of the raster");
        return (int32_t)k;
    }
    // ... at any rate: under wide_resample the source runs at 48000 * decim1 * down / up
    static int32_t wide_fcw_rate(double offset_hz, double rate_hz)
    {
        const double w = std::nearbyint(offset_hz / rate_hz * 4294967296.0);
        return (int32_t)(uint32_t)(int64_t)w;
    }
    void wide_channels(const uint32_t* source, const int32_t* fcw, uint32_t n) { check(m17hip_wide_channels(ctx_, source, fcw, n), "m17hip_wide_channels"); }
    // the frequency word of an offset in Hz from the source's centre, rounded to the nearest word
    static int32_t wide_fcw(double offset_hz, uint32_t decim)
    {
        const double w = std::nearbyint(offset_hz / (48000.0 * decim) * 4294967296.0);
        return (int32_t)(uint32_t)(int64_t)w;
    }
    void upload_wide(const void* host, uint32_t channels, uint32_t samples, size_t pitch, float gain = 1.0f)
    {
        check(m17hip_upload_wide(ctx_, host, gain, channels, samples, pitch), "m17hip_upload_wide");
        channels_ = channels; samples_ = samples;
    }
    // The input generated on the device from the caller's own transmissions, one per channel (m17hip_synth_tx_i16: the framing of
    // apps/m17-mod.cpp:264-504, 509-564 around lsf30[channels][30] and rows[n_rows][32]; impairments and seeding from `base`)
    void synth_tx(const m17_synth_params& base, const m17_tx* tx, const uint8_t* lsf30, const uint8_t* rows, uint32_t n_rows, uint32_t channels,
                  uint32_t samples, uint32_t chan0 = 0)
    {
        check(m17hip_synth_tx_i16(ctx_, &base, tx, lsf30, rows, n_rows, channels, samples, chan0), "m17hip_synth_tx_i16");
        channels_ = channels; samples_ = samples;
    }
    void reset() { check(m17hip_demod_reset(ctx_), "m17hip_demod_reset"); }
    // Fresh demodulators for the listed channels only (local indices), from the start of the NEXT run queued; the others go on
    // (m17hip_demod_reset_channels: between runs whose lengths are multiples of 192 samples, not between front() and run()).
    void reset_channels(const uint32_t* channels, uint32_t n) { check(m17hip_demod_reset_channels(ctx_, channels, n), "m17hip_demod_reset_channels"); }
    // Per-channel input polarity (the reference's -i, per receiver): invert[n] of 0 / 1 for local channels 0 .. n - 1, nullptr with n == 0 clears;
    // XOR the flags of run() (m17hip_set_channel_polarity: changing a channel that has run restarts it, as reset_channels does).
    void set_channel_polarity(const uint8_t* invert, uint32_t n) { check(m17hip_set_channel_polarity(ctx_, invert, n), "m17hip_set_channel_polarity"); }
    void run(uint32_t flags = 0) { check(m17hip_demod_run(ctx_, channels_, samples_, flags), "m17hip_demod_run"); }

    // records of the last run, ordered by (channel, seq): one compaction and one synchronisation when the guessed capacity suffices
    // (M17HIP_ETRUNC reports the real count; the fetch is then repeated once)
    std::vector<m17_frame_rec> frames()
    {
        std::vector<m17_frame_rec> out(last_frames_ + last_frames_ / 4 + 1024);
        uint64_t got = 0;
        int code = m17hip_frames_fetch(ctx_, out.data(), out.size(), &got);
        if (code == M17HIP_ETRUNC && got > out.size()) {
            out.resize(got);
            code = m17hip_frames_fetch(ctx_, out.data(), out.size(), &got);
        }
        check(code, "m17hip_frames_fetch");
        out.resize(got);
        last_frames_ = got;
        return out;
    }
    // Which run's records frames() / packets() / voice() / calls() name: 0 = the latest run (every run() selects it again), 1 = the run before it — what a live
    // feed asks for after it has queued the next run (m17hip_frames_select).
    void select(uint32_t back) { check(m17hip_frames_select(ctx_, back), "m17hip_frames_select"); }
    // Streaming (include/m17hip.h, m17hip_demod_front): stage the next run's input from pinned host memory while the current run
    // computes, start its front end beside the current run's state-machine half, queue its run() behind the current one, then select(1) and
    // collect the current run's frames() (or, as up to round 5: frames() first, then run()).
    void stage(const int16_t* pinned_host, uint32_t channels, uint32_t samples, size_t pitch)
    {
        check(m17hip_upload_i16_async(ctx_, pinned_host, channels, samples, pitch), "m17hip_upload_i16_async");
        channels_ = channels; samples_ = samples;
    }
    void stage(const float* pinned_host, uint32_t channels, uint32_t samples, size_t pitch)
    {
        check(m17hip_upload_f32_async(ctx_, pinned_host, channels, samples, pitch), "m17hip_upload_f32_async");
        channels_ = channels; samples_ = samples;
    }
    void stage_iq(const std::complex<float>* pinned_host, uint32_t channels, uint32_t samples, size_t pitch, float gain = 1.0f)
    {
        check(m17hip_upload_iq_async(ctx_, pinned_host, M17HIP_IQ_F32, gain, channels, samples, pitch), "m17hip_upload_iq_async");
        channels_ = channels; samples_ = samples;
    }
    void stage_iq(const int16_t (*pinned_host)[2], uint32_t channels, uint32_t samples, size_t pitch, float gain = 1.0f)
    {
        check(m17hip_upload_iq_async(ctx_, pinned_host, M17HIP_IQ_I16, gain, channels, samples, pitch), "m17hip_upload_iq_async");
        channels_ = channels; samples_ = samples;
    }
    void stage_wide(const void* pinned_host, uint32_t channels, uint32_t samples, size_t pitch, float gain = 1.0f)
    {
        check(m17hip_upload_wide_async(ctx_, pinned_host, gain, channels, samples, pitch), "m17hip_upload_wide_async");
        channels_ = channels; samples_ = samples;
    }
    void front(uint32_t flags = 0) { check(m17hip_demod_front(ctx_, channels_, samples_, flags), "m17hip_demod_front"); }
    void stage_wait() { check(m17hip_upload_wait(ctx_), "m17hip_upload_wait"); }
    // BERT statistics per channel (apps/m17-demod.cpp:286-304 + PRBS9): counted over the runs made after enable_bert(true)
    void enable_bert(bool on) { check(m17hip_tune(ctx_, 6, on ? 1 : 0), "m17hip_tune"); }
    std::vector<m17_bert_stat> bert_stats()
    {
        std::vector<m17_bert_stat> st(channels_);
        check(m17hip_bert_stats(ctx_, st.data(), channels_), "m17hip_bert_stats");
        return st;
    }
    // Packet reassembly per channel (decode_packet, apps/m17-demod.cpp:207-253): enable with room for `room` packets per run (0 = off),
    // then packets() returns what the last run completed, ordered by (channel, seq)
    void enable_packets(uint32_t room) { check(m17hip_tune(ctx_, 7, room), "m17hip_tune"); room_ = room; }
    std::vector<m17_packet_rec> packets()
    {
        std::vector<m17_packet_rec> out(room_);
        uint32_t n = 0;
        check(m17hip_packets_fetch(ctx_, out.data(), room_, &n), "m17hip_packets_fetch");
        out.resize(n < room_ ? n : room_);
        return out;
    }
    // The voice of stream transmissions (demodulate_audio, apps/m17-demod.cpp:178-205, without codec2): enable with room for `room` voice
    // frames per channel and run (0 = off; samples / 1920 + 1 is always enough), then voice() returns the 16 payload bytes (two codec2 3200
    // frames) of every stream frame of the selected run per channel, in arrival order, with one mark byte each (M17HIP_MARK_*: bit 0 = what
    // -b would silence), and calls() the calls that run closed, ordered by (channel, seq).
    struct Voice {
        uint32_t slots = 0;              // row pitch of audio / marks
        std::vector<uint8_t> audio;      // [channels][slots][16]
        std::vector<uint8_t> marks;      // [channels][slots]
        std::vector<uint32_t> counts;    // [channels] slots in use
        const uint8_t* frame(uint32_t channel, uint32_t slot) const { return audio.data() + ((size_t)channel * slots + slot) * 16; }
        uint8_t mark(uint32_t channel, uint32_t slot) const { return marks[(size_t)channel * slots + slot]; }
    };
    void enable_voice(uint32_t room) { check(m17hip_tune(ctx_, 34, room), "m17hip_tune"); voice_room_ = room; }
    Voice voice()
    {
        Voice v;
        v.slots = voice_room_;
        v.audio.resize((size_t)channels_ * voice_room_ * 16);
        v.marks.resize((size_t)channels_ * voice_room_);
        v.counts.resize(channels_);
        check(m17hip_voice_fetch(ctx_, v.audio.data(), v.marks.data(), v.counts.data(), channels_, voice_room_), "m17hip_voice_fetch");
        return v;
    }
    std::vector<m17_call_rec> calls()
    {
        std::vector<m17_call_rec> out((size_t)channels_ * M17HIP_CALLS_PER_CHANNEL(voice_room_));
        uint32_t n = 0;
        check(m17hip_calls_fetch(ctx_, out.data(), (uint32_t)out.size(), &n), "m17hip_calls_fetch");
        out.resize(n < out.size() ? n : out.size());
        return out;
    }
    std::vector<m17_diag> diagnostics()
    {
        std::vector<m17_diag> d(channels_);
        check(m17hip_diag_fetch(ctx_, d.data(), channels_), "m17hip_diag_fetch");
        return d;
    }
    // Every diagnostic callback of a run, not only the last: enable with room for `room` callbacks per channel and run
    // (samples / 384 + 2 is always enough), then diag_log(channel) returns them in stream order; entry.pad[0] | pad[1] << 32
    // is the sample that fired it.
    void enable_diag_log(uint32_t room) { check(m17hip_tune(ctx_, 9, room), "m17hip_tune"); diag_room_ = room; }
    std::vector<m17_diag> diag_log(uint32_t channel = 0)
    {
        std::vector<m17_diag> all((size_t)channels_ * diag_room_);
        std::vector<uint32_t> counts(channels_);
        check(m17hip_diag_log_fetch(ctx_, all.data(), counts.data(), channels_, diag_room_), "m17hip_diag_log_fetch");
        const auto first = all.begin() + (size_t)channel * diag_room_;
        return std::vector<m17_diag>(first, first + counts[channel]);
    }
    // Multi-GPU (one BatchedDemodulator = one shard = one rank): records carry channel = base + local index
    void set_channel_base(uint32_t base) { check(m17hip_set_channel_base(ctx_, base), "m17hip_set_channel_base"); }
    // Evaluation order of the Kalman updates (include/m17hip.h); default 3
    void set_kalman_order(int order) { check(m17hip_set_kalman_order(ctx_, order), "m17hip_set_kalman_order"); }

    // batched counterparts of the reference's operators (parity API)
    std::vector<float> fir(uint32_t flags = 0)  // BaseFirFilter<float,150> with the RRC taps: FirFilter.h:28-43
    {
        std::vector<float> y((size_t)channels_ * samples_);
        check(m17hip_fir_rrc150(ctx_, channels_, samples_, flags, y.data()), "m17hip_fir_rrc150");
        return y;
    }
    void correlator(std::vector<float>& limit, std::vector<float>& corr)  // Correlator::sample/correlate: Correlator.h:43-64
    {
        limit.resize((size_t)channels_ * samples_);
        corr.resize((size_t)4 * channels_ * samples_);
        check(m17hip_correlator(ctx_, channels_, samples_, limit.data(), corr.data()), "m17hip_correlator");
    }
    std::vector<float> dcd_sums(uint32_t flags = 0)  // NSlidingDFT + DataCarrierDetect accumulation: DataCarrierDetect.h:53-58
    {
        std::vector<float> s((size_t)channels_ * (samples_ / 192) * 12);
        uint32_t ticks = 0;
        check(m17hip_dcd(ctx_, channels_, samples_, flags, s.data(), &ticks), "m17hip_dcd");
        return s;
    }
    // Viterbi<Trellis<4,2>,4>::decode<IN,OUT>: kind 0 = <488,240>, 1 = <296,144>, 2 = <420,206>, 3 = <402,197> (Viterbi.h:162-239)
    void viterbi(const int8_t* soft, uint32_t n_frames, int kind, uint8_t* bits, int32_t* cost)
    {
        check(m17hip_viterbi(ctx_, soft, n_frames, kind, bits, cost), "m17hip_viterbi");
    }
};

} // mobilinkd
