// mobilinkd::M17Demodulator<FloatType> — the reference's demodulator object (include/m17cxx/M17Demodulator.h:123-217) as
// apps/m17-demod.cpp drives it: construct with the frame callback (:455), install a diagnostic callback (:478), push one scaled
// sample per call (:484-490).  This one runs on the MI355X: samples are collected into blocks (default 1920 = one M17 frame,
// 40 ms), every full block goes through the GPU chain (include/m17hip.h; matched filter, carrier detect, correlator / clock
// recovery state machine, Viterbi) with the demodulator state carried from block to block, and the callbacks are then
// delivered in exactly the reference's order: every frame callback and every diagnostic callback (one per 960 samples while
// the carrier is on, one per 384 while it is off), ordered by the sample that fired them, frame callbacks of a sample first.
// What a caller can observe beyond that: callbacks arrive up to one block late, and the end of the input needs flush() —
// the destructor calls it, so a stock read loop loses nothing.  There is no silent CPU fallback: without libm17hip.so / a GPU the
// constructor throws.  For thousands of channels at once use BatchedDemodulator.h (this class is the 1-channel case of it).
//
// The same object can be told to stay on the HOST (BASELINE configs[0]: one stream, no GPU): construct it with the tag
// `mobilinkd::scalar_cpu`, or — for an application that is not to be touched, like the stock apps/m17-demod.cpp — export
// M17_DEMOD_DEVICE=cpu (M17_DEMOD_DEVICE=<n> picks GPU n; unset = GPU 0).  It then runs detail/scalar_demod.h: the operator classes
// of this directory, i.e. the arithmetic cores the kernels are built from, one sample per call, callbacks delivered at once.
//
// Like the reference's header this one pulls in the whole operator surface (Correlator, FirFilter, DataCarrierDetect,
// ClockRecovery, FreqDevEstimator, M17FrameDecoder with LinkSetupFrame / CRC16 / Viterbi / Trellis, M17Framer, SymbolEvm,
// Util with PRBS9 and llr), so an application written against the reference compiles unchanged.
#pragma once

#include "BatchedDemodulator.h"
#include "ClockRecovery.h"
#include "Correlator.h"
#include "DataCarrierDetect.h"
#include "FirFilter.h"
#include "FreqDevEstimator.h"
#include "M17FrameDecoder.h"
#include "M17Framer.h"
#include "SymbolEvm.h"
#include "Util.h"
#include "detail/scalar_demod.h"

#include <algorithm>
#include <cstdlib>
#include <memory>
#include <array>
#include <cmath>
#include <cstring>
#include <functional>
#include <optional>
#include <stdexcept>
#include <tuple>
#include <vector>

namespace mobilinkd
{

namespace detail
{

// The demodulator's matched filter: root-raised-cosine, alpha = 0.5, 10 samples per symbol, 150 taps (the last one 0.0).
// Reference M17Demodulator.h:29-118; the values live in detail/rrc_half_taps.inc (75 distinct ones, the filter is symmetric).
template <typename FloatType>
struct Taps
{
    static constexpr std::array<FloatType, 150> make()
    {
        std::array<FloatType, 150> t{};
        for (size_t i = 0; i != 149; ++i) t[i] = FloatType(i <= 74 ? core::RRC_HALF[i] : core::RRC_HALF[148 - i]);
        return t;
    }
    static constexpr auto rrc_taps = make();
};

} // detail

struct scalar_cpu_t { explicit scalar_cpu_t() = default; };
inline constexpr scalar_cpu_t scalar_cpu{};   // M17Demodulator<float> demod(callback, scalar_cpu): the host form, no GPU involved

template <typename FloatType>
struct M17Demodulator
{
    static constexpr uint16_t SAMPLE_RATE = 48000;
    static constexpr uint16_t SYMBOL_RATE = 4800;
    static constexpr uint16_t SAMPLES_PER_SYMBOL = SAMPLE_RATE / SYMBOL_RATE;
    static constexpr uint16_t BLOCK_SIZE = 192;

    static constexpr FloatType sample_rate = SAMPLE_RATE;
    static constexpr FloatType symbol_rate = SYMBOL_RATE;

    static constexpr size_t STREAM_COST_LIMIT = 80;
    static constexpr size_t PACKET_COST_LIMIT = 60;
    static constexpr uint8_t MAX_MISSING_SYNC = 10;
    static constexpr uint8_t MIN_SYNC_COUNT = 78;
    static constexpr uint8_t MAX_SYNC_COUNT = 86;
    static constexpr FloatType EOT_TRIGGER_LEVEL = 0.1;

    using collelator_t = Correlator<FloatType>;
    using sync_word_t = SyncWord<collelator_t>;
    using callback_t = M17FrameDecoder::callback_t;
    using diagnostic_callback_t = std::function<void(bool, FloatType, FloatType, FloatType, bool, FloatType, int, int, int, int)>;

    enum class DemodState { UNLOCKED, LSF_SYNC, STREAM_SYNC, PACKET_SYNC, BERT_SYNC, SYNC_WAIT, FRAME };

    DemodState demodState = DemodState::UNLOCKED;   // state at the end of the last block

    // the reference's constructor (M17Demodulator.h:180-182): where it runs is the environment's choice (see the header comment)
    explicit M17Demodulator(callback_t callback) : callback_(std::move(callback)), block_(1920)
    {
        const char* where = std::getenv("M17_DEMOD_DEVICE");
        if (where && std::string(where) == "cpu") start_cpu();
        else start_gpu(where && *where ? std::atoi(where) : 0);
    }
    M17Demodulator(callback_t callback, uint32_t block_samples, int device = 0) : callback_(std::move(callback)), block_(block_samples)
    {
        start_gpu(device);
    }
    M17Demodulator(callback_t callback, scalar_cpu_t) : callback_(std::move(callback)), block_(1920) { start_cpu(); }

    virtual ~M17Demodulator()
    {
        try { flush(); } catch (...) {}
    }

    // The sample is what the reference's operator() receives (apps/m17-demod.cpp:489 makes it sample / 41067.0; a discriminator delivers it as it
    // is): the GPU path buffers it as float32 and uploads it as a float stream (m17hip_upload_f32) — nothing is rounded, nothing is clipped, and the
    // callbacks are those of the host form on the same samples.
    void operator()(const FloatType input)
    {
        if (cpu_) {   // the host form: this very sample, callbacks before the call returns
            cpu_->step(input);
            demodState = (DemodState)cpu_->state();
            return;
        }
        if (!iq_buffer_.empty()) run_iq_block();   // (IQ pushed before this sample comes before it)
        if (wide_decim_ && wide_buffer_.size() >= wide_decim_) run_wide_block();
        buffer_.push_back((float)input);
        if (buffer_.size() == block_) run_block();
    }

    // One complex IQ sample of a narrowband FM channel at 48 kSPS in front of the demodulator: gain * arg(x[n] conj(x[n-1])) is the sample the
    // demodulator receives (detail/core.h fm_discriminate; an int16 pair converts exactly).  The GPU path buffers the IQ and discriminates it on the device
    // (m17hip_upload_iq); the host form computes the same words here.  The feed begins from a zero sample: the first output is +0.
    void iq(float i, float q)
    {
        if (cpu_) {
            const float y = core::fm_discriminate(i, q, iq_prev_[0], iq_prev_[1], iq_gain_);
            iq_prev_[0] = i; iq_prev_[1] = q;
            cpu_->step((FloatType)y);
            demodState = (DemodState)cpu_->state();
            return;
        }
        if (!buffer_.empty()) run_block();
        if (wide_decim_ && wide_buffer_.size() >= wide_decim_) run_wide_block();
        iq_buffer_.push_back({i, q});
        if (iq_buffer_.size() == block_) run_iq_block();
    }
    void iq_gain(float gain) { iq_gain_ = gain; }   // finite and > 0; 1 = radians per sample (the demodulator normalises by its own deviation estimate)

    // One channel out of one WIDEBAND feed at 48000 * decim samples per second, offset_hz from its centre: the feed is mixed to the offset, low-passed
    // with `taps` (empty: the default taps, m17hip_wide_default_taps), every decim-th sample kept and discriminated with iq_gain() — the stage the
    // reference's users run rtl_fm for.  Starts the feed over.  On the GPU path it is m17hip_wide_config / m17hip_wide_channels; the host form computes the
    // same words from detail/core.h (nco, ddc_mix, ddc_fir).  An int16 sample converts exactly, a uint8 one is core::ddc_u8.
    void wide_config(uint32_t decim, double offset_hz, std::vector<float> taps = {})
    {
        if (taps.empty()) {
            uint32_t n = 0;
            taps.resize(32 * 16 + 1);
            if (m17hip_wide_default_taps(decim, taps.data(), (uint32_t)taps.size(), &n) != M17HIP_OK) throw std::runtime_error("m17hip_wide_default_taps");
            taps.resize(n);
        }
        wide_decim_ = decim;
        spectrum_points_ = 0; scan_ = false;   // (every configuration turns the spectrum off, and the scan with it)
        meter_window_ = 0;      // (and the meter)
        squelch_mode_ = 0;      // (and the squelch)
        wide_r1_ = 0;
        wide_up_ = 1; wide_down_ = 0;
        raster_m_ = 0;
        wide_fcw_ = (uint32_t)BatchedDemodulator::wide_fcw(offset_hz, decim);
        if (gpu_) {
            flush();
            const uint32_t source = 0;
            const int32_t fcw = (int32_t)wide_fcw_;
            gpu_->wide_config(1, decim, M17HIP_IQ_F32, taps.data(), (uint32_t)taps.size());
            gpu_->wide_channels(&source, &fcw, 1);
            wide_buffer_.clear();
            return;
        }
        wide_taps_ = std::move(taps);
        wide_m_ = 0;
        wide_mixed_.clear();   // the mixed feed as (re, im): the zero history of ntaps - 1 samples first, at the phases it would have had
        for (size_t k = wide_taps_.size() - 1; k > 0; --k) {
            float re, im;
            core::ddc_mix(0.0f, 0.0f, wide_fcw_, (uint32_t)(0 - k), re, im);
            wide_mixed_.push_back(re); wide_mixed_.push_back(im);
        }
    }
    // The same out of a feed at 48000 * decim1 * decim2 samples per second, decimated in two stages (m17hip_wide_config2: a 2.4 MSPS dongle is 10 x 5):
    // low-passed with taps1 and every decim1-th sample kept, then with taps2 and every decim2-th; empty: that stage's default taps
    // (m17hip_wide_default_taps2).  The host form is core::ddc_fir2.
    void wide_config(uint32_t decim1, uint32_t decim2, double offset_hz, std::vector<float> taps1 = {}, std::vector<float> taps2 = {})
    {
        if (taps1.empty() || taps2.empty()) {
            uint32_t n1 = 0, n2 = 0;
            std::vector<float> d1(8 * 16 + 1), d2(32 * 16 + 1);
            if (m17hip_wide_default_taps2(decim1, decim2, d1.data(), (uint32_t)d1.size(), &n1, d2.data(), (uint32_t)d2.size(), &n2) != M17HIP_OK)
                throw std::runtime_error("m17hip_wide_default_taps2");
            if (taps1.empty()) taps1.assign(d1.begin(), d1.begin() + n1);
            if (taps2.empty()) taps2.assign(d2.begin(), d2.begin() + n2);
        }
        wide_decim_ = decim1 * decim2;
        spectrum_points_ = 0; scan_ = false;   // (every configuration turns the spectrum off, and the scan with it)
        meter_window_ = 0;      // (and the meter)
        squelch_mode_ = 0;      // (and the squelch)
        wide_r1_ = decim1;
        wide_up_ = 1; wide_down_ = 0;
        raster_m_ = 0;
        wide_fcw_ = (uint32_t)BatchedDemodulator::wide_fcw(offset_hz, wide_decim_);
        if (gpu_) {
            flush();
            const uint32_t source = 0;
            const int32_t fcw = (int32_t)wide_fcw_;
            gpu_->wide_config2(1, decim1, decim2, M17HIP_IQ_F32, taps1.data(), (uint32_t)taps1.size(), taps2.data(), (uint32_t)taps2.size());
            gpu_->wide_channels(&source, &fcw, 1);
            wide_buffer_.clear();
            return;
        }
        wide_taps_ = std::move(taps1);
        wide_taps2_ = std::move(taps2);
        wide_m_ = 0;
        wide_mixed_.clear();   // the zero history of (ntaps2 - 1) decim1 + ntaps1 - 1 samples first, at the phases it would have had
        for (size_t k = (wide_taps2_.size() - 1) * decim1 + wide_taps_.size() - 1; k > 0; --k) {
            float re, im;
            core::ddc_mix(0.0f, 0.0f, wide_fcw_, (uint32_t)(0 - k), re, im);
            wide_mixed_.push_back(re); wide_mixed_.push_back(im);
        }
        wide_u_.assign(2 * (wide_taps2_.size() - 1), 0.0f);   // (the u in front of the feed: made from that history with the first output)
    }
    // The same out of a feed at ANY rate m17hip_wide_resample_ratio has a shape for (2.048 MSPS is 16 x 3 / 8): the second stage resamples by up / down
    // (m17hip_wide_resample); empty taps: that stage's default taps (m17hip_wide_resample_default_taps).  Whole groups of down * decim1 samples — `up`
    // outputs each — are buffered.  The host form is core::ddc_resample, a group at a time.  Throws std::invalid_argument for a rate without a shape.
    void wide_rate(uint32_t rate_hz, double offset_hz, std::vector<float> taps1 = {}, std::vector<float> taps2 = {})
    {
        uint32_t decim1 = 0, up = 0, down = 0;
        BatchedDemodulator::wide_resample_ratio(rate_hz, decim1, up, down);
        if (taps1.empty() || taps2.empty()) {
            uint32_t n1 = 0, n2 = 0;
            std::vector<float> d1(8 * 16 + 1), d2(32 * 125 + 1);
            if (m17hip_wide_resample_default_taps(decim1, up, down, d1.data(), (uint32_t)d1.size(), &n1, d2.data(), (uint32_t)d2.size(), &n2) != M17HIP_OK)
                throw std::runtime_error("m17hip_wide_resample_default_taps");
            if (taps1.empty()) taps1.assign(d1.begin(), d1.begin() + n1);
            if (taps2.empty()) taps2.assign(d2.begin(), d2.begin() + n2);
        }
        wide_decim_ = decim1 * down;   // (the samples of a group)
        spectrum_points_ = 0; scan_ = false;   // (every configuration turns the spectrum off, and the scan with it)
        meter_window_ = 0;      // (and the meter)
        squelch_mode_ = 0;      // (and the squelch)
        wide_r1_ = decim1;
        wide_up_ = up; wide_down_ = down;
        raster_m_ = 0;
        wide_fcw_ = (uint32_t)BatchedDemodulator::wide_fcw_rate(offset_hz, (double)rate_hz);
        if (gpu_) {
            flush();
            const uint32_t source = 0;
            const int32_t fcw = (int32_t)wide_fcw_;
            gpu_->wide_resample(1, decim1, up, down, M17HIP_IQ_F32, taps1.data(), (uint32_t)taps1.size(), taps2.data(), (uint32_t)taps2.size());
            gpu_->wide_channels(&source, &fcw, 1);
            wide_buffer_.clear();
            return;
        }
        wide_taps_ = std::move(taps1);
        wide_taps2_ = std::move(taps2);
        wide_m_ = 0;
        const size_t J2 = (wide_taps2_.size() + up - 1) / up, H = (J2 - 1) * decim1 + wide_taps_.size() - 1;
        wide_mixed_.assign(2 * H, 0.0f);   // the feed itself as (re, im) — ddc_resample mixes it — behind its zero history
        wide_scratch_.resize(2 * (H + wide_decim_));
        wide_u_.resize(2 * (J2 - 1 + down));
    }
    // The same for a channel ON A RASTER of `bins` channels spaced 48000 * decim / bins Hz (decim 1..64; m17hip_wide_raster: the polyphase channeliser):
    // bin `bin`, -bins/2 <= bin < bins/2, of the feed; taps empty: the default taps (m17hip_wide_raster_default_taps).  The host form computes the same
    // words from detail/core.h (chan_fold, chan_pass1, chan_pass2) over the library's twiddle table.
    void wide_raster(uint32_t decim, uint32_t bins, int32_t bin, std::vector<float> taps = {})
    {
        uint32_t m1 = 0, m2 = 0;
        if (!core::chan_factor(bins, m1, m2) || bin < -(int32_t)(bins / 2) || bin > (int32_t)((bins - 1) / 2)) throw std::invalid_argument("M17Demodulator::wide_raster");
        if (taps.empty()) {
            uint32_t n = 0;
            taps.resize(32 * 64 + 1);
            if (m17hip_wide_raster_default_taps(decim, taps.data(), (uint32_t)taps.size(), &n) != M17HIP_OK) throw std::runtime_error("m17hip_wide_raster_default_taps");
            taps.resize(n);
        }
        wide_decim_ = decim;
        spectrum_points_ = 0; scan_ = false;   // (every configuration turns the spectrum off, and the scan with it)
        meter_window_ = 0;      // (and the meter)
        squelch_mode_ = 0;      // (and the squelch)
        wide_r1_ = 0;
        wide_up_ = 1; wide_down_ = 0;
        if (gpu_) {
            flush();
            const uint32_t source = 0;
            gpu_->wide_raster(1, decim, bins, M17HIP_IQ_F32, taps.data(), (uint32_t)taps.size());
            gpu_->wide_raster_channels(&source, &bin, 1);
            wide_buffer_.clear();
            raster_m_ = bins;
            return;
        }
        raster_tw_.resize(2 * (size_t)bins);
        if (m17hip_wide_raster_twiddles(bins, raster_tw_.data(), (uint32_t)raster_tw_.size()) != M17HIP_OK) throw std::runtime_error("m17hip_wide_raster_twiddles");
        raster_m_ = bins; raster_m1_ = m1; raster_m2_ = m2;
        raster_k_ = (uint32_t)(bin < 0 ? bin + (int32_t)bins : bin);
        raster_w_.resize(4 * (size_t)bins);
        wide_taps_ = std::move(taps);
        wide_m_ = 0;
        wide_mixed_.assign(2 * (wide_taps_.size() - 1), 0.0f);   // the feed itself as (re, im) — nothing is mixed — behind its zero history of ntaps - 1 samples
    }
    // The raster survey beside wide_raster on the GPU path (m17hip_wide_survey): every stride-th output of the feed adds the power of EVERY bin to the
    // block's plane, and after each block `report` gets the plane (indexed by bin mod bins), the block's survey times and the feed's output index at its
    // start.  stride 0 turns it off.  Returns false, with nothing changed, on the host form: the survey is a device feature.
    using survey_callback_t = std::function<void(const std::vector<float>& power, uint32_t times, uint64_t first_output)>;
    bool wide_survey(uint32_t stride, survey_callback_t report)
    {
        if (!gpu_) return false;
        if (!raster_m_) throw std::logic_error("M17Demodulator::wide_survey before wide_raster");
        flush();
        gpu_->wide_survey(stride);
        survey_stride_ = stride;
        survey_report_ = std::move(report);
        return true;
    }
    // The source spectrum beside any wideband configuration on the GPU path (m17hip_wide_spectrum): the frames of `points` samples (a power of two in
    // 64..4096; 0 turns it off) that begin where the feed's sample index is a multiple of `hop` are windowed (empty: the default Blackman-Harris window),
    // transformed and their powers summed, and after each block `report` gets the plane — bin k at k rate / points below points / 2, (k - points) rate /
    // points from there on —, the block's frames and the feed's sample index at its first frame.  Returns false, with nothing changed, on the host form: the
    // spectrum is a device feature.  Any wide_config / wide_rate / wide_raster call turns it off.
    using spectrum_callback_t = std::function<void(const std::vector<float>& power, uint32_t frames, uint64_t first_sample)>;
    bool wide_spectrum(uint32_t points, uint32_t hop, spectrum_callback_t report, const std::vector<float>& window = {})
    {
        if (!gpu_) return false;
        if (!wide_decim_) throw std::logic_error("M17Demodulator::wide_spectrum before wide_config");
        flush();
        gpu_->wide_spectrum(points, hop, window.empty() ? nullptr : window.data(), (uint32_t)window.size());
        spectrum_points_ = points;
        spectrum_report_ = std::move(report);
        squelch_mode_ = 0; scan_ = false;   // (every wide_spectrum call turns the squelch off, and the scan with it)
        return true;
    }
    // The spectrum squelch beside wide_config / wide_rate on the GPU path (m17hip_wide_squelch; wide_spectrum first): the NEXT block runs unsquelched, and
    // its plane gives the levels — the median of the plane times 2 half_bins + 1, per frame, times 10^(open_db / 10) and 10^(close_db / 10), the rule of
    // m17hip's Python wide_squelch_levels —; from the block after it the channel is tuned only while its band of the block's spectrum holds a carrier (and
    // for `hang` blocks behind that), and gets +0 otherwise.  After each squelched block `report`, if any, gets the decision: open, the hold count, the band
    // power and the block's frames.  Returns false, with nothing changed, on the host form.  Any wide_config / wide_rate / wide_raster / wide_spectrum
    // call turns it off.
    using squelch_callback_t = std::function<void(bool open, uint32_t hold, float band, uint32_t frames)>;
    bool wide_squelch(uint32_t half_bins, double open_db, double close_db, uint32_t hang = 0, squelch_callback_t report = {})
    {
        if (!gpu_) return false;
        if (!wide_decim_ || raster_m_ || !spectrum_points_) throw std::logic_error("M17Demodulator::wide_squelch needs wide_config or wide_rate, and wide_spectrum");
        if (half_bins > 64 || half_bins >= spectrum_points_ / 2 || hang > 65535 || !(close_db <= open_db)) throw std::invalid_argument("M17Demodulator::wide_squelch");
        flush();
        gpu_->wide_squelch_off();
        squelch_half_ = half_bins; squelch_open_db_ = open_db; squelch_close_db_ = close_db; squelch_hang_ = hang;
        squelch_report_ = std::move(report);
        squelch_slots_ = false;
        squelch_floor_ = false;
        scan_ = false;
        squelch_mode_ = 1;   // (armed: the next block's plane sets the levels)
        return true;
    }
    // The time-resolved mode of the same (m17hip_wide_squelch_slots), in wide_squelch's place: armed and levelled in the same way, but the decision is taken per
    // slot of 16 frames of the block's spectrum (`hang` counts slots) and the tuner skips per tile of its outputs; `lead` opens the tiles in front of an
    // opening within the block, so a transmission that begins inside a block keeps its start.  After each squelched block `report`, if any, gets the tiles
    // tuned, the block's tiles, its slots and its frames.
    using squelch_slots_callback_t = std::function<void(uint32_t open_tiles, uint32_t tiles, uint32_t slots, uint32_t frames)>;
    bool wide_squelch_slots(uint32_t half_bins, double open_db, double close_db, uint32_t hang = 0, uint32_t lead = 0, squelch_slots_callback_t report = {})
    {
        if (!gpu_) return false;
        if (!wide_decim_ || raster_m_ || !spectrum_points_) throw std::logic_error("M17Demodulator::wide_squelch_slots needs wide_config or wide_rate, and wide_spectrum");
        if (half_bins > 64 || half_bins >= spectrum_points_ / 2 || hang > 65535 || lead > 255 || !(close_db <= open_db))
            throw std::invalid_argument("M17Demodulator::wide_squelch_slots");
        flush();
        gpu_->wide_squelch_off();
        squelch_half_ = half_bins; squelch_open_db_ = open_db; squelch_close_db_ = close_db; squelch_hang_ = hang; squelch_lead_ = lead;
        squelch_slots_report_ = std::move(report);
        squelch_slots_ = true;
        squelch_floor_ = false;
        scan_ = false;
        squelch_mode_ = 1;   // (armed: the next block's plane sets the levels)
        return true;
    }
    // The floor on the device (m17hip_wide_squelch_floor), behind wide_squelch or wide_squelch_slots, whose half_bins, hang, lead and report stay and whose
    // own open_db / close_db are set aside: no block runs unsquelched and the host takes no median — every block, the next one included, is squelched at
    // open_db / close_db over the floor the device takes from that very block's plane (its upper median), tracked by `rise` towards a higher floor and by
    // `fall` towards a lower one (each in (0, 1]; 1 follows at once).  After each block `report`, if any, gets the tracked floor, the two levels (per frame)
    // and the block's frames.  Returns false, with nothing changed, on the host form.  Whatever turns the squelch off, and each of the two squelch calls,
    // turns it off.
    using squelch_floor_callback_t = std::function<void(float floor, float open_level, float close_level, uint32_t frames)>;
    bool wide_squelch_floor(double open_db, double close_db, float rise = 1.0f, float fall = 1.0f, squelch_floor_callback_t report = {})
    {
        if (!gpu_) return false;
        if (!squelch_mode_) throw std::logic_error("M17Demodulator::wide_squelch_floor needs wide_squelch or wide_squelch_slots");
        if (!(close_db <= open_db) || !(rise > 0.0f) || !(rise <= 1.0f) || !(fall > 0.0f) || !(fall <= 1.0f)) throw std::invalid_argument("M17Demodulator::wide_squelch_floor");
        flush();
        if (squelch_slots_) gpu_->wide_squelch_slots(squelch_half_, {1.0f}, {1.0f}, squelch_hang_, squelch_lead_);   // (the mode on; its levels are never read)
        else gpu_->wide_squelch(squelch_half_, {1.0f}, {1.0f}, squelch_hang_);
        gpu_->wide_squelch_floor((float)std::pow(10.0, open_db / 10.0), (float)std::pow(10.0, close_db / 10.0), rise, fall);
        squelch_floor_report_ = std::move(report);
        squelch_floor_ = true;
        squelch_mode_ = 2;
        return true;
    }
    // The carrier scan (m17hip_wide_scan), behind wide_squelch_floor: a pool of the one channel, so the demodulator follows the strongest carrier of its
    // source — where no carrier holds it, the block's scan tunes it to the strongest one, from the very block in which that carrier appears — and is reset
    // before the run of a block that retunes it (a new transmission on a demodulator fed zeros).  The offset given at construction is the seed.  guard_bins 0:
    // 9 kHz at the source's rate.  After each block `report`, if any, gets the frequency word the block was tuned with, whether it was assigned in this
    // block, whether a carrier held it, and the carriers that found it taken.  Returns false, with nothing changed, on the host form.
    using scan_callback_t = std::function<void(int32_t fcw, bool assigned, bool held, uint32_t missed)>;
    bool wide_scan(uint32_t guard_bins = 0, scan_callback_t report = {})
    {
        if (!gpu_) return false;
        if (!squelch_floor_ || squelch_slots_) throw std::logic_error("M17Demodulator::wide_scan needs wide_squelch and wide_squelch_floor");
        flush();
        if (!guard_bins) {
            const double rate = 48000.0 * (double)wide_decim_ / (double)wide_up_;
            guard_bins = std::max<uint32_t>(3u, std::min<uint32_t>((uint32_t)std::ceil(9000.0 / (rate / spectrum_points_)), spectrum_points_ / 4));
        }
        gpu_->wide_scan({1}, guard_bins);
        scan_report_ = std::move(report);
        scan_ = true;
        return true;
    }
    // The channel meter beside any wideband configuration on the GPU path (m17hip_wide_meter): per window of `window` outputs of the feed (16..65536; 0
    // turns it off; 1920 is one M17 frame) the channel's level, its carrier's offset from the channel's frequency and its deviation, and after each block
    // `report` gets them for every piece of a window the block holds: the feed's window number, the piece's outputs, 10 log10 of the mean power of z (dB
    // over an amplitude of 1 in the source's units), the mean of the discriminator's output in Hz and its standard deviation in Hz.  Returns false, with
    // nothing changed, on the host form: the meter is a device feature.  Any wide_config / wide_rate / wide_raster call turns it off.
    using meter_callback_t = std::function<void(uint64_t window, uint32_t outputs, double level_db, double offset_hz, double deviation_hz)>;
    bool wide_meter(uint32_t window, meter_callback_t report)
    {
        if (!gpu_) return false;
        if (!wide_decim_) throw std::logic_error("M17Demodulator::wide_meter before wide_config");
        flush();
        gpu_->wide_meter(window);
        meter_window_ = window;
        meter_report_ = std::move(report);
        return true;
    }
    // one wideband sample (wide_config or wide_raster first)
    void wide(float i, float q)
    {
        if (!wide_decim_) throw std::logic_error("M17Demodulator::wide before wide_config");
        if (cpu_ && raster_m_) {
            wide_mixed_.push_back(i); wide_mixed_.push_back(q);
            if (++wide_m_ % wide_decim_ != 0) return;
            const uint32_t M = raster_m_, L = (uint32_t)wide_taps_.size(), mm = (uint32_t)((wide_m_ - 1) % M);   // (the newest sample is number wide_m_ - 1)
            float* w = raster_w_.data();
            float* a = w + 2 * (size_t)M;
            for (uint32_t r = 0; r < M; ++r) core::chan_fold(wide_taps_.data(), L, M, (mm + M - r) % M, wide_mixed_.data() + wide_mixed_.size() - 2, w[2 * r], w[2 * r + 1]);
            for (uint32_t r1 = 0; r1 < raster_m1_; ++r1)
                for (uint32_t k2 = 0; k2 < raster_m2_; ++k2)
                    core::chan_pass1(w, raster_m1_, raster_m2_, raster_tw_.data(), r1, k2, a[2 * (r1 * raster_m2_ + k2)], a[2 * (r1 * raster_m2_ + k2) + 1]);
            float re, im;
            core::chan_pass2(a, raster_m1_, raster_m2_, raster_tw_.data(), raster_k_, re, im);
            const float y = core::fm_discriminate(re, im, iq_prev_[0], iq_prev_[1], iq_gain_);
            iq_prev_[0] = re; iq_prev_[1] = im;
            if (wide_mixed_.size() > 2 * ((size_t)L + 65536)) wide_mixed_.erase(wide_mixed_.begin(), wide_mixed_.end() - 2 * ((size_t)L - 1));
            cpu_->step((FloatType)y);
            demodState = (DemodState)cpu_->state();
            return;
        }
        if (cpu_ && wide_down_) {   // a whole group of down * decim1 samples makes `up` outputs
            wide_mixed_.push_back(i); wide_mixed_.push_back(q);
            if (++wide_m_ % wide_decim_ != 0) return;
            const uint32_t L1 = (uint32_t)wide_taps_.size(), L2 = (uint32_t)wide_taps2_.size();
            const size_t H = (size_t)((L2 + wide_up_ - 1) / wide_up_ - 1) * wide_r1_ + L1 - 1;
            float z[2 * 32], y[32];
            core::ddc_resample(wide_taps_.data(), L1, wide_r1_, wide_taps2_.data(), L2, wide_up_, wide_down_, wide_mixed_.data() + wide_mixed_.size() - 2 * (size_t)wide_decim_,
                               wide_fcw_, (uint32_t)(wide_m_ - wide_decim_), wide_up_, wide_scratch_.data(), wide_u_.data(), z, iq_prev_, iq_gain_, y);
            if (wide_mixed_.size() > 2 * (H + 65536)) wide_mixed_.erase(wide_mixed_.begin(), wide_mixed_.end() - 2 * H);
            for (uint32_t k = 0; k < wide_up_; ++k) cpu_->step((FloatType)y[k]);
            demodState = (DemodState)cpu_->state();
            return;
        }
        if (cpu_) {
            float re, im;
            core::ddc_mix(i, q, wide_fcw_, (uint32_t)wide_m_, re, im);
            wide_mixed_.push_back(re); wide_mixed_.push_back(im);
            if (++wide_m_ % wide_decim_ != 0) return;
            if (wide_r1_) {   // two stages: the decim2 new u and the z over them (the u in front are kept: they are a function of the mixed feed alone)
                const uint32_t L2 = (uint32_t)wide_taps2_.size(), R2 = wide_decim_ / wide_r1_;
                const size_t H = (size_t)(L2 - 1) * wide_r1_ + wide_taps_.size() - 1;
                wide_u_.resize(wide_u_.size() + 2 * R2);
                float z[2];
                core::ddc_fir2(wide_taps_.data(), (uint32_t)wide_taps_.size(), wide_r1_, wide_taps2_.data(), L2, R2,
                               wide_mixed_.data() + wide_mixed_.size() - 2 * (size_t)wide_decim_, 1, wide_m_ == wide_decim_ ? L2 - 1 : 0,
                               wide_u_.data() + wide_u_.size() - 2 * R2, z);
                const float y2 = core::fm_discriminate(z[0], z[1], iq_prev_[0], iq_prev_[1], iq_gain_);
                iq_prev_[0] = z[0]; iq_prev_[1] = z[1];
                if (wide_mixed_.size() > 2 * (H + 65536)) {
                    wide_mixed_.erase(wide_mixed_.begin(), wide_mixed_.end() - 2 * H);
                    wide_u_.erase(wide_u_.begin(), wide_u_.end() - 2 * (size_t)(L2 - 1));
                }
                cpu_->step((FloatType)y2);
                demodState = (DemodState)cpu_->state();
                return;
            }
            core::ddc_fir(wide_taps_.data(), (uint32_t)wide_taps_.size(), wide_mixed_.data() + wide_mixed_.size() - 2, re, im);
            const float y = core::fm_discriminate(re, im, iq_prev_[0], iq_prev_[1], iq_gain_);   // (the carry the discriminator's own feed uses: the last z)
            iq_prev_[0] = re; iq_prev_[1] = im;
            if (wide_mixed_.size() > 2 * (wide_taps_.size() + 8192)) wide_mixed_.erase(wide_mixed_.begin(), wide_mixed_.end() - 2 * (wide_taps_.size() - 1));
            cpu_->step((FloatType)y);
            demodState = (DemodState)cpu_->state();
            return;
        }
        if (!buffer_.empty()) run_block();
        if (!iq_buffer_.empty()) run_iq_block();
        wide_buffer_.push_back({i, q});
        if (wide_buffer_.size() == (size_t)(block_ / wide_up_) * wide_decim_) run_wide_block();
    }

    // demodulate what is buffered (end of input); safe to call at any time (wideband samples short of one output stay buffered)
    void flush()
    {
        if (gpu_ && !buffer_.empty()) run_block();
        if (gpu_ && !iq_buffer_.empty()) run_iq_block();
        if (gpu_ && wide_decim_ && wide_buffer_.size() >= wide_decim_) run_wide_block();
    }
    bool on_gpu() const { return gpu_ != nullptr; }

    bool locked() const { return dcd_; }
    void passall(bool enabled) { passall_ = enabled; }
    void diagnostics(diagnostic_callback_t callback) { diagnostic_callback = std::move(callback); }

    diagnostic_callback_t diagnostic_callback;

private:
    void deliver(const m17_frame_rec& r)
    {
        M17FrameDecoder::output_buffer_t ob;
        std::memset(&ob, 0, sizeof(ob));
        ob.type = (M17FrameDecoder::FrameType)r.frame_type;
        switch (ob.type) {
        case M17FrameDecoder::FrameType::LSF: std::memcpy(ob.lsf.data(), r.payload, 30); break;
        case M17FrameDecoder::FrameType::LICH: std::memcpy(ob.lich.data(), r.payload, 6); break;
        case M17FrameDecoder::FrameType::STREAM: std::memcpy(ob.stream.data(), r.payload, 18); break;
        case M17FrameDecoder::FrameType::BERT: std::memcpy(ob.bert.data(), r.payload, 25); break;
        default: std::memcpy(ob.packet.data(), r.payload, 26); break;
        }
        if (callback_) callback_(ob, r.cost);
    }
    void deliver(const m17_diag& d)
    {
        dcd_ = d.dcd != 0;
        if (diagnostic_callback)
            diagnostic_callback(d.dcd != 0, (FloatType)d.evm, (FloatType)d.deviation, (FloatType)d.offset, d.locked != 0, (FloatType)d.clock,
                                d.sample_index, d.sync_index, d.clock_index, d.viterbi_cost);
    }
    void start_gpu(int device)
    {
        gpu_ = std::make_unique<BatchedDemodulator>(1, block_, device);
        buffer_.reserve(block_);
        gpu_->enable_diag_log(block_ / 384 + 2);
        gpu_->reset();
    }
    void start_cpu()
    {
        cpu_ = std::make_unique<detail::ScalarDemodulator<FloatType>>(detail::Taps<FloatType>::rrc_taps,
            [this](const M17FrameDecoder::output_buffer_t& f, int cost) { return callback_ ? callback_(f, cost) : true; });
        cpu_->on_diagnostics = [this](bool dcd, FloatType evm, FloatType dev, FloatType off, bool locked, FloatType clock, int si, int sy, int ci, int vc) {
            dcd_ = dcd;
            if (diagnostic_callback) diagnostic_callback(dcd, evm, dev, off, locked, clock, si, sy, ci, vc);
        };
    }
    void run_block()
    {
        gpu_->upload(buffer_.data(), 1, (uint32_t)buffer_.size(), buffer_.size());
        buffer_.clear();
        run_uploaded();
    }
    void run_iq_block()
    {
        gpu_->upload_iq(iq_buffer_.data(), 1, (uint32_t)iq_buffer_.size(), iq_buffer_.size(), iq_gain_);
        iq_buffer_.clear();
        run_uploaded();
    }
    void run_wide_block()
    {
        const size_t n = wide_buffer_.size() / wide_decim_;
        gpu_->upload_wide(wide_buffer_.data(), 1, (uint32_t)(n * wide_up_), n * wide_decim_, iq_gain_);
        wide_buffer_.erase(wide_buffer_.begin(), wide_buffer_.begin() + n * wide_decim_);
        if (survey_stride_ && survey_report_) {   // (the plane of the block just uploaded: the fetch waits for its survey kernels, not for the run)
            survey_power_.resize(raster_m_);
            uint32_t times = 0;
            uint64_t first = 0;
            gpu_->wide_survey_fetch(0, survey_power_.data(), survey_power_.size(), &times, &first);
            survey_report_(survey_power_, times, first);
        }
        const bool squelched = squelch_mode_ == 2;   // (this block was uploaded with the squelch on)
        if (spectrum_points_ && (spectrum_report_ || squelch_mode_ == 1)) {   // (likewise: the fetch waits for the block's spectrum kernels)
            spectrum_power_.resize(spectrum_points_);
            uint32_t frames = 0;
            uint64_t first = 0;
            gpu_->wide_spectrum_fetch(0, spectrum_power_.data(), spectrum_power_.size(), &frames, &first);
            if (spectrum_report_) spectrum_report_(spectrum_power_, frames, first);
            if (squelch_mode_ == 1 && frames) {   // (the levels from this block's plane; the squelch holds from the next block on)
                std::vector<float> v(spectrum_power_);
                std::sort(v.begin(), v.end());
                const double floor = 0.5 * ((double)v[v.size() / 2 - 1] + (double)v[v.size() / 2]) * (2.0 * squelch_half_ + 1.0) / (double)frames;
                const float open = (float)(floor * std::pow(10.0, squelch_open_db_ / 10.0)), close = (float)(floor * std::pow(10.0, squelch_close_db_ / 10.0));
                if (std::isfinite(open) && close > 0.0f) {   // (a plane of zeros sets nothing: the next block tries again)
                    if (squelch_slots_) gpu_->wide_squelch_slots(squelch_half_, {open}, {close}, squelch_hang_, squelch_lead_);
                    else gpu_->wide_squelch(squelch_half_, {open}, {close}, squelch_hang_);
                    squelch_mode_ = 2;
                }
            }
        }
        if (squelched && squelch_slots_ && squelch_slots_report_) {   // (likewise: the fetch waits for the block's squelch kernels)
            uint32_t slots = 0, tiles = 0, frames = 0, open_tiles = 0;
            gpu_->wide_squelch_slots_fetch(0, squelch_state_, squelch_band_, squelch_mask_, &slots, &tiles, &frames);
            for (uint32_t t = 0; t < tiles; ++t) open_tiles += (squelch_mask_[t >> 5] >> (t & 31u)) & 1u;
            squelch_slots_report_(open_tiles, tiles, slots, frames);
        }
        if (squelched && !squelch_slots_ && squelch_report_) {   // (likewise: the fetch waits for the block's squelch kernel)
            uint32_t frames = 0;
            gpu_->wide_squelch_fetch(0, squelch_state_, squelch_band_, &frames);
            squelch_report_((squelch_state_[0] >> 31) != 0, squelch_state_[0] & 0x7FFFFFFFu, squelch_band_[0], frames);
        }
        if (squelched && squelch_floor_ && squelch_floor_report_) {   // (likewise: the fetch waits for the block's floor and squelch kernels)
            uint32_t frames = 0;
            gpu_->wide_squelch_floor_fetch(0, squelch_floor_plane_, nullptr, &frames);
            squelch_floor_report_(squelch_floor_plane_[1], squelch_floor_plane_[2], squelch_floor_plane_[3], frames);
        }
        if (squelched && squelch_floor_ && scan_) {   // (the reset rule: the fetch waits for the block's scan kernel, not for its tuner)
            gpu_->wide_scan_fetch(0, scan_fcw_, scan_flags_, scan_missed_, &scan_assigned_);
            if (!scan_assigned_.empty()) gpu_->reset_channels(scan_assigned_.data(), (uint32_t)scan_assigned_.size());
            if (scan_report_) scan_report_(scan_fcw_[0], (scan_flags_[0] & 2u) != 0, (scan_flags_[0] & 4u) != 0, scan_missed_[0]);
        }
        if (meter_window_ && meter_report_) {   // (likewise: the fetch waits for the block's meter kernel)
            uint32_t pieces = 0, outputs = 0;
            uint64_t first_window = 0, first_output = 0;
            gpu_->wide_meter_fetch(0, meter_planes_, nullptr, &pieces, &first_window, &first_output, &outputs);
            const double hz = 48000.0 / (2.0 * 3.14159265358979323846 * (double)iq_gain_);
            const uint64_t a0 = first_output % meter_window_;
            for (uint32_t k = 0; k < pieces; ++k) {   // (one channel: planes [3][1][pieces])
                const uint64_t lo = (uint64_t)k * meter_window_ > a0 ? (uint64_t)k * meter_window_ - a0 : 0;
                const uint64_t hi = std::min<uint64_t>((uint64_t)(k + 1) * meter_window_ - a0, outputs);
                const double m = (double)(hi - lo), mean = meter_planes_[pieces + k] / m;
                meter_report_(first_window + k, (uint32_t)(hi - lo), 10.0 * std::log10(meter_planes_[k] / m), mean * hz,
                              std::sqrt(std::max(meter_planes_[2 * pieces + k] / m - mean * mean, 0.0)) * hz);
            }
        }
        run_uploaded();
    }
    void run_uploaded()
    {
        auto& gpu_ = *this->gpu_;
        gpu_.run();
        const auto frames = gpu_.frames();
        const auto diags = gpu_.diag_log();
        // merge by the sample that fired the callback; within one sample the reference calls the frame callback(s) first
        size_t f = 0, g = 0;
        while (f < frames.size() || g < diags.size()) {
            const uint64_t fp = f < frames.size() ? frames[f].sample_pos : ~0ull;
            const uint64_t gp = g < diags.size() ? (uint64_t)diags[g].pad[0] | ((uint64_t)diags[g].pad[1] << 32) : ~0ull;
            if (f < frames.size() && fp <= gp) deliver(frames[f++]);
            else deliver(diags[g++]);
        }
        demodState = (DemodState)gpu_.diagnostics()[0].demod_state;
    }

    std::unique_ptr<BatchedDemodulator> gpu_;                        // one of the two
    std::unique_ptr<detail::ScalarDemodulator<FloatType>> cpu_;
    callback_t callback_;
    std::vector<float> buffer_;
    std::vector<std::complex<float>> iq_buffer_;   // (one of the two holds samples at a time)
    float iq_gain_ = 1.0f, iq_prev_[2] = {0.0f, 0.0f};
    std::vector<std::complex<float>> wide_buffer_;   // the GPU path's wideband samples short of a block
    std::vector<float> wide_taps_, wide_mixed_;      // the host form's filter and mixed feed
    std::vector<float> wide_taps2_, wide_u_;         // two stages: the second filter and the feed between the two
    uint32_t wide_decim_ = 0, wide_fcw_ = 0;         // (0: wide_config has not been called); wideband samples per output
    uint32_t wide_r1_ = 0;                           // the first stage's decimation (0: one stage)
    uint32_t wide_up_ = 1, wide_down_ = 0;           // wide_rate: outputs per group of wide_decim_ samples, and the second stage's `down` (0: integer stages)
    std::vector<float> wide_scratch_;                // wide_rate's host form: the mixed samples of one call
    uint32_t raster_m_ = 0, raster_m1_ = 0, raster_m2_ = 0, raster_k_ = 0;   // wide_raster: the bins (0: a tuner), their factors and the bin mod M
    uint32_t survey_stride_ = 0;                     // wide_survey: 0 = off
    survey_callback_t survey_report_;
    std::vector<float> survey_power_;
    uint32_t spectrum_points_ = 0;                   // wide_spectrum: 0 = off
    spectrum_callback_t spectrum_report_;
    std::vector<float> spectrum_power_;
    uint32_t meter_window_ = 0;                      // wide_meter: 0 = off
    meter_callback_t meter_report_;
    std::vector<float> meter_planes_;
    int squelch_mode_ = 0;                           // wide_squelch: 0 = off, 1 = armed (the next block's plane sets the levels), 2 = on
    bool squelch_slots_ = false;                     // wide_squelch_slots in wide_squelch's place
    bool squelch_floor_ = false;                     // wide_squelch_floor: the levels are the device's
    bool scan_ = false;                              // wide_scan: the one channel is a slot
    scan_callback_t scan_report_;
    std::vector<int32_t> scan_fcw_;
    std::vector<uint32_t> scan_flags_, scan_missed_, scan_assigned_;
    squelch_floor_callback_t squelch_floor_report_;
    std::vector<float> squelch_floor_plane_;
    uint32_t squelch_half_ = 0, squelch_hang_ = 0, squelch_lead_ = 0;
    squelch_slots_callback_t squelch_slots_report_;
    std::vector<uint32_t> squelch_mask_;
    double squelch_open_db_ = 0.0, squelch_close_db_ = 0.0;
    squelch_callback_t squelch_report_;
    std::vector<uint32_t> squelch_state_;
    std::vector<float> squelch_band_;
    std::vector<float> raster_tw_, raster_w_;        // the twiddle table; the partial sums and the first pass's sums of one output
    uint64_t wide_m_ = 0;
    uint32_t block_;
    bool dcd_ = false;
    bool passall_ = false;
};

} // mobilinkd
