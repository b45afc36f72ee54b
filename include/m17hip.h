/* m17hip.h — C ABI of the MI355X-native M17 4-FSK demodulation hot path.
 *
 * The reference (mobilinkd/m17-cxx-demod) has no FFI layer: its hot path is the header-only
 * operator surface in include/m17cxx driven one sample at a time by apps/m17-demod.cpp:484-490.
 * This library is what a batched replacement of that path binds to: plain pointers and sizes,
 * no C++ or torch types, every function returns 0 on success or a negative M17HIP_E* code
 * (m17hip_strerror), no exceptions cross the boundary.  One context per (host thread, GPU).
 * All channels of a context advance together: a "run" consumes T new samples of each of C
 * independent 48 kSPS int16 baseband channels and continues from the state the previous run left
 * (m17hip_demod_reset starts over), exactly as C fresh reference processes would.
 *
 * Each entry point names the reference interface it replaces (file:line in /root/reference).
 */
#ifndef M17HIP_H
#define M17HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M17HIP_OK 0
#define M17HIP_EINVAL (-1)   /* bad argument / size beyond what the context was created for */
#define M17HIP_EHIP (-2)     /* a HIP runtime call failed (m17hip_last_hip_error) */
#define M17HIP_ENOMEM (-3)
#define M17HIP_ESTATE (-4)   /* call sequence error (e.g. fetch before run) */
#define M17HIP_EOVERFLOW (-5) /* a per-channel frame-record buffer overflowed */
#define M17HIP_ETRUNC (-6)   /* more results than the caller's capacity: *count says how many exist, `capacity` were written */
#define M17HIP_ECOMM (-7)    /* an RCCL call failed (m17hip_gather_*) */
#define M17HIP_ECONFIG (-8)  /* m17hip_ctx_create: the process runs with fewer than 8 hardware queues (GPU_MAX_HW_QUEUES; see m17hip_advice) */
/* (-8 was M17HIP_ETIMEOUT of ABI 301's persistent kernel form, removed in ABI 400) */

/* Frame-type / sync-type codes = the reference enums M17FrameDecoder.h:52-55. */
enum { M17_FRAME_LSF = 0, M17_FRAME_LICH = 1, M17_FRAME_STREAM = 2, M17_FRAME_BASIC_PACKET = 3, M17_FRAME_FULL_PACKET = 4, M17_FRAME_BERT = 5 };
enum { M17_SYNC_LSF = 0, M17_SYNC_STREAM = 1, M17_SYNC_PACKET = 2, M17_SYNC_BERT = 3 };

/* One record per invocation of the reference's frame callback
 * `bool(const output_buffer_t&, int viterbi_cost)` (M17FrameDecoder.h:98, called at :171,221,253,271,286,306).
 * payload = lsf[30] | lich[6] | stream[18] | packet[26] | bert[25] according to frame_type. */
typedef struct m17_frame_rec {
    uint32_t channel;
    uint32_t seq;        /* per-channel callback counter since the last reset */
    uint64_t sample_pos; /* 0-based index (since reset) of the input sample whose processing fired the callback */
    int32_t cost;        /* the callback's viterbi_cost argument */
    uint8_t frame_type;  /* M17_FRAME_* */
    uint8_t sync_type;   /* M17_SYNC_* that selected the decode */
    uint8_t len;         /* valid payload bytes */
    uint8_t flags;
    uint8_t payload[32];
    uint8_t pad[8];
} m17_frame_rec; /* 64 bytes */

/* Arguments of the most recent diagnostic callback (M17Demodulator.h:144, fired at :681-685 and :746-750),
 * plus the demodulator state at the end of the run. */
typedef struct m17_diag {
    int32_t dcd;
    float evm, deviation, offset;
    int32_t locked;
    float clock;
    int32_t sample_index, sync_index, clock_index, viterbi_cost;
    float dcd_level;
    uint32_t n_diag;
    uint32_t demod_state; /* M17Demodulator.h:146 DemodState */
    uint32_t n_frames;    /* frame callbacks since reset */
    uint32_t pad[2];
} m17_diag; /* 64 bytes */

typedef struct m17hip_ctx m17hip_ctx;

#define M17HIP_FLAG_INVERT 1u /* apps/m17-demod.cpp:488 `if (invert_input) sample *= -1`; the only flag: any other bit is M17HIP_EINVAL */

const char* m17hip_strerror(int code);
int m17hip_last_hip_error(const m17hip_ctx* ctx);
int m17hip_version(void);

/* Context: device slabs for `max_channels` x `max_samples` (per run).  Replaces constructing one
 * M17Demodulator<float> per channel (apps/m17-demod.cpp:455, M17Demodulator.h:180-182).
 * max_samples <= M17HIP_MAX_SAMPLES_PER_RUN (11.6 minutes of 48 kSPS in ONE run; a stream of any length is continued run after run):
 * the kernels address a channel row — sixteen rows in the limit-filter replay — with 32-bit byte offsets.  Beyond it: M17HIP_EINVAL. */
#define M17HIP_MAX_SAMPLES_PER_RUN 33553152u
int m17hip_ctx_create(int device, uint32_t max_channels, uint32_t max_samples, m17hip_ctx** out);
void m17hip_ctx_destroy(m17hip_ctx* ctx);
/* Hardware queues.  A context uses five streams (main, matched filter, carrier detect, limit-filter replay, copy); with streams
 * sharing a hardware queue a kernel queued behind another stream's event wait waits with it, and the overlap the streams exist for
 * is lost (measured: two contexts 42 instead of 26 ms per step).  The HIP runtime reads GPU_MAX_HW_QUEUES when it initialises (its
 * default is 4): export GPU_MAX_HW_QUEUES=16 before the first HIP call of the process (the Python binding and the C++ host classes
 * set it at load time when it is unset — effective when that is before the process's first contact with the GPU).
 * The slow state is never entered silently: with the variable unset or below 8 m17hip_ctx_create returns M17HIP_ECONFIG, unless the
 * host says it accepts that (environment variable M17HIP_FEW_HW_QUEUES_OK=1).
 * m17hip_advice (bit set; 0 = nothing to say): bit 0 (M17HIP_ADVICE_HW_QUEUES) fewer than 8 queues were asked for, bit 1
 * (M17HIP_ADVICE_HW_QUEUES_16) fewer than 16 — enough for one context, not for two batches in flight or a stream in two groups. */
#define M17HIP_ADVICE_HW_QUEUES 1
#define M17HIP_ADVICE_HW_QUEUES_16 2
int m17hip_advice(const m17hip_ctx* ctx);
/* Operational statistic: how many times since the last m17hip_demod_reset a channel left the limit-filter replay (the demodulator
 * forced dcd.unlock() after losing sync, M17Demodulator.h:396-404, 470-478: the one gate event the replay cannot foresee) and computed
 * its own limit-filter history up to the end of the next segment — the slow path of the sequential kernel.  Waits for the queued work. */
int m17hip_replay_drops(m17hip_ctx* ctx, uint64_t* count);
/* The context's main stream (a hipStream_t).  From round 6 on the library creates it — together with the context's other streams, in one go and in a
 * fixed role order; a destroyed context's streams are parked as a set and handed to the next context of that device — because which streams share a
 * hardware pipe decides 10-40 % of a continued stream's step time and the runtime maps streams to pipes in creation order: a process that creates and
 * destroys contexts around a host's own main streams walks through the slow layouts (24 -> 26 -> 32 ms per step over three create / use / destroy
 * cycles, tools/stream_history.py; 22.1-22.5 ms in every cycle with the library's own).  It is a NON-BLOCKING stream: it does not synchronise with the
 * default stream.  A host that produces input on, or consumes device-side results from, a stream of its own orders the two with events (or, in
 * PyTorch, wraps this one: torch.cuda.ExternalStream(handle)); results fetched into host memory are complete when the fetch returns, as ever. */
int m17hip_get_stream(m17hip_ctx* ctx, void** hip_stream);
/* For hosts that insist: launch all work of this context on `hip_stream` instead (a hipStream_t; NULL = the default stream — what a context ran on
 * up to round 5 when this was not called).  The library's main stream stays with the context, idle.  The switch is ordered: what the context queues
 * on `hip_stream` afterwards starts behind everything it had queued before (a run still in flight, its payload work, the reset kernels of
 * m17hip_ctx_create), so it may be called at any time between calls.  M17HIP_STREAM_SETS=0 in the environment restores
 * the older behaviour altogether (streams per context, destroyed with it, main = the default stream): a diagnostic, not a deployment mode. */
int m17hip_set_stream(m17hip_ctx* ctx, void* hip_stream);

/* Input: [C][T] int16, row pitch in samples.  Replaces the stdin read loop apps/m17-demod.cpp:484-488. */
int m17hip_upload_i16(m17hip_ctx* ctx, const int16_t* host, uint32_t channels, uint32_t samples, size_t pitch);
/* Same, from a DEVICE pointer (e.g. a tensor that already lives in HBM); the copy is complete when the call returns, so
 * `dev` may be freed or refilled at once. */
int m17hip_upload_i16_device(m17hip_ctx* ctx, const int16_t* dev, uint32_t channels, uint32_t samples, size_t pitch);
/* Streaming ingest: stage the input of the NEXT m17hip_demod_run in a second slab while the current run is
 * computing.  The copy is queued on the context's own copy stream and starts as soon as the run before the current one has
 * released that slab; it should come from pinned memory (hipHostMalloc / hipHostRegister) to overlap.  The next
 * m17hip_demod_run (same channel / sample counts) makes the device wait for the copy, swaps the slabs (the carried 152-sample
 * tail is moved over) and runs on the staged input.  (The first staging call of a context allocates the second set of per-run
 * slabs: input, matched-filter output, limit-filter history, carrier-detect table.)  m17hip_demod_run does NOT wait on the host: the copy may still be in
 * flight when it returns.  The host buffer must stay valid AND unmodified until m17hip_upload_wait has returned (or until a
 * frames / diag fetch of the run that consumed it has returned — those synchronise with the run, which waited for the copy). */
int m17hip_upload_i16_async(m17hip_ctx* ctx, const int16_t* host, uint32_t channels, uint32_t samples, size_t pitch);
/* Block until the copy queued by the last m17hip_upload_i16_async / m17hip_upload_i16_device_async has left its source buffer. */
int m17hip_upload_wait(m17hip_ctx* ctx);
/* The same staging from DEVICE memory (a producer on the GPU hands a chunk over): a device-to-device copy on the context's copy
 * stream, NOT complete when the call returns — `dev` must stay valid and unmodified until m17hip_upload_wait has returned.  The copy
 * stream does not wait for the producer's stream: `dev` must be COMPLETE when the call is made (the producer synchronised, or the hand-over
 * ordered by the caller). */
int m17hip_upload_i16_device_async(m17hip_ctx* ctx, const int16_t* dev, uint32_t channels, uint32_t samples, size_t pitch);
/* Staging without a copy: declares that the context's second input slab — the one the run BEFORE the latest run consumed, or
 * that an earlier m17hip_upload_i16_async filled — already holds the next run's `channels` x `samples` input (two resident slabs
 * that alternate, e.g. a replayed capture).  M17HIP_ESTATE if that slab holds no input of this shape. */
int m17hip_input_alternate(m17hip_ctx* ctx, uint32_t channels, uint32_t samples);

/* ---- float32 input (ABI 607) ---------------------------------------------------------------------
 * A second sample format for a context's input: IEEE float32 IN THE REFERENCE'S UNITS — a value is what M17Demodulator<float>::operator()
 * receives (apps/m17-demod.cpp:489 makes it from an int16 as sample / 41067.0; a discriminator or a channeliser delivers it as it is).
 * Nothing is scaled and nothing is rounded; under M17HIP_FLAG_INVERT / m17hip_set_channel_polarity the float is negated, which is exact (there is
 * no -32768 wrap); values beyond +-1 are samples like any other.  Every kernel that reads the input has a float form, and records, m17_diag
 * and the diagnostic log are bit-identical to the reference algorithm stepped on those floats (tests/test_gpu_f32_input.py); on floats of
 * the form float(s / 41067.0) they are what the int16 path gives on s.
 * The four entry points are the int16 ones with `const float*` (pitch in samples; the same staging-pair semantics, m17hip_input_alternate,
 * m17hip_demod_front and m17hip_upload_wait).  The float slabs are allocated with the first float input: a context that never sees one holds
 * nothing more than before (m17hip_input_format).
 * THE FORMAT BELONGS TO THE STREAM: the first upload or synthesis after m17hip_ctx_create or m17hip_demod_reset fixes it (synthesis is int16);
 * an upload of the other format, m17hip_synth_* on a float stream and a run on a slab that holds the other format return M17HIP_ESTATE, with
 * nothing changed; m17hip_demod_reset frees the choice again.  m17hip_download_i16 / m17hip_download_f32 return M17HIP_ESTATE when the current
 * slab holds the other format.  Everything else — m17hip_demod_run / _front, m17hip_frames_*, m17hip_diag_*, the consumers and gathers,
 * m17hip_demod_reset_channels, the polarity table, the gate-aware front end, both carrier-detect forms, m17hip_fir_rrc150,
 * m17hip_fir_correlator and m17hip_dcd — works on a float stream exactly as on an int16 one.
 * m17hip_tune keys that select among kernels reading the input: 10, 13, 20 and 26 are honoured; the measurement build's keys 1, 19 (the
 * instrumented sequential kernels) and 11 = 0 (round 4's matched filter) have no float form: a float run under them returns M17HIP_ESTATE
 * (no int16 kernel is ever launched on float memory).
 * Non-finite samples are legal input: a NaN or an infinity stays in its channel (whose results from there on are whatever IEEE arithmetic
 * makes of it); the other channels and the call are not affected. */
#define M17HIP_FORMAT_I16 1
#define M17HIP_FORMAT_F32 2
int m17hip_upload_f32(m17hip_ctx* ctx, const float* host, uint32_t channels, uint32_t samples, size_t pitch);
int m17hip_upload_f32_device(m17hip_ctx* ctx, const float* dev, uint32_t channels, uint32_t samples, size_t pitch);
int m17hip_upload_f32_async(m17hip_ctx* ctx, const float* host, uint32_t channels, uint32_t samples, size_t pitch);
int m17hip_upload_f32_device_async(m17hip_ctx* ctx, const float* dev, uint32_t channels, uint32_t samples, size_t pitch);
/* Read the float input slab back: out[channels][samples] (row pitch in samples), byte for byte what was uploaded. */
int m17hip_download_f32(m17hip_ctx* ctx, float* host, uint32_t channels, uint32_t samples, size_t pitch);
/* *stream_format: the sample format the stream is fixed to (M17HIP_FORMAT_I16 / M17HIP_FORMAT_F32; 0 = free: nothing uploaded or synthesised
 * since the creation or the last m17hip_demod_reset).  *f32_bytes: device memory the context holds for float input (slabs and history
 * arrays): 0 for a context that has never seen a float.  Either pointer may be NULL. */
int m17hip_input_format(m17hip_ctx* ctx, int* stream_format, uint64_t* f32_bytes);

/* ---- complex IQ input: the FM discriminator on the device (ABI 608) -----------------------------------
 * The radios that deliver thousands of channels deliver complex IQ, one narrowband stream per channel at 48 kSPS.  These entry points take it and put
 *     y[n] = gain * arg(x[n] * conj(x[n-1]))        (radians per sample at gain 1)
 * into the context's float input slab, where m17hip_upload_f32 would have put the caller's floats: behind them the stream is a FLOAT STREAM and nothing
 * else in the chain knows the difference (m17hip_download_f32 returns the discriminated floats, m17hip_input_format says M17HIP_FORMAT_F32; on an int16
 * stream they return M17HIP_ESTATE with nothing changed; m17hip_synth_* on the stream they made returns M17HIP_ESTATE).  The arithmetic is the project's
 * own, defined once for host and device (m17cxx/detail/core.h: fm_cross, fm_phase, fm_discriminate — a float32 four-quadrant arctangent within 2^-20 rad
 * of atan2, odd in Q to the bit, +0 for a zero product), so a host can compute the very words the device computes.  The demodulator normalises by its own
 * deviation estimate: any finite gain > 0 decodes.  A spectrum-flipped (conjugated) input is the exact negation: M17HIP_FLAG_INVERT / the polarity table.
 * iq_format: M17HIP_IQ_I16 — interleaved int16 I,Q (converted to float, exact) — or M17HIP_IQ_F32 — interleaved float32 I,Q; no scaling in either, and
 * the format may change from one call to the next.  `samples` counts COMPLEX samples (= float baseband samples produced), and so does `pitch`.
 * The four functions are the four m17hip_upload_f32 ways in, with the same staging-pair semantics (m17hip_input_alternate, m17hip_demod_front and
 * m17hip_upload_wait work as for floats).  The device forms read the caller's memory directly (a sample aligned to its own size; rows that are 16-byte
 * aligned take the 16-byte loads, others go sample by sample).  As for m17hip_upload_i16_device_async, `dev` must be COMPLETE when the call is made: the
 * context's streams are non-blocking and do not wait for the producer's stream (the producer synchronised, or the hand-over ordered by the caller);
 * the _async form's memory stays valid and unmodified until m17hip_upload_wait has returned.  The host forms copy the raw IQ into a device buffer the
 * context owns (allocated with the first host IQ block, grown when a later one is larger), then discriminate on the same stream.
 * THE FEED: IQ blocks continue one another in call order, per channel, whether or not a run consumed the slab in between: the sample in front of a
 * block's first one is the last sample of the IQ block uploaded before it (one float2 per channel, kept on the device).  It is zero — the first output is
 * +0 — after m17hip_ctx_create, after m17hip_demod_reset, and for the listed channels after m17hip_demod_reset_channels: a channel reset applies to the IQ
 * blocks uploaded AFTER it (not to a block already staged).
 * M17HIP_EINVAL: a NULL context or pointer, channels or samples of 0 or beyond the context's limits, pitch < samples, an unknown iq_format, a gain that is
 * not finite and > 0.  M17HIP_ESTATE: while a front end queued by m17hip_demod_front is waiting for its run, as for every upload.
 * Non-finite IQ samples stay in their channel (and reach the following block's first output through the carry).
 * m17hip_timing_get index 8 is the discriminator kernel.
 * Out of scope: de-emphasis and squelch (tuning channels out of wideband IQ by an integer decimation, 8-bit IQ included: ABI 609, below). */
#define M17HIP_IQ_I16 1   /* interleaved int16 I,Q */
#define M17HIP_IQ_F32 2   /* interleaved float32 I,Q */
int m17hip_upload_iq(m17hip_ctx* ctx, const void* host, int iq_format, float gain, uint32_t channels, uint32_t samples, size_t pitch);
int m17hip_upload_iq_device(m17hip_ctx* ctx, const void* dev, int iq_format, float gain, uint32_t channels, uint32_t samples, size_t pitch);
int m17hip_upload_iq_async(m17hip_ctx* ctx, const void* host, int iq_format, float gain, uint32_t channels, uint32_t samples, size_t pitch);
int m17hip_upload_iq_device_async(m17hip_ctx* ctx, const void* dev, int iq_format, float gain, uint32_t channels, uint32_t samples, size_t pitch);
/* Device memory the context holds for IQ input: the carry and the host forms' raw-IQ buffer, and for wideband input (m17hip_wide_config) the taps, the
 * sources' histories and the channel tables.  0 for a context that has never seen IQ. */
int m17hip_iq_bytes(m17hip_ctx* ctx, uint64_t* bytes);

/* ---- wideband IQ input: tune and decimate channels on the device (ABI 609) ----------------------------
 * A receiver that covers thousands of channels delivers a few WIDE IQ streams at a multiple of 48 kSPS.  These entry points take S such sources at
 * 48000 * decim samples per second; each of the context's channels names a source and a frequency offset, and one kernel (csrc/m17_wide_kernels.hpp) mixes,
 * low-pass filters, keeps every decim-th sample and discriminates straight into the float input slab:
 *     mixed[m] = x[m] * conj(nco(fcw * m))                             (m counts the source's samples since the feed began; the product is taken mod 2^32)
 *     z[n]     = sum_{i < ntaps} taps[i] * mixed[n decim + decim - 1 - i]
 *     y[n]     = gain * arg(z[n] * conj(z[n-1]))
 * Behind it the stream is a FLOAT STREAM exactly as after m17hip_upload_iq.  There is no reference file to cite: this is the stage the reference's users run
 * rtl_fm or a channeliser for, the half of that job in front of the discriminator of ABI 608.  The arithmetic is the project's own, defined once for host
 * and device (m17cxx/detail/core.h: nco — a float32 oscillator within 2^-21 of cos / sin, exactly on the axes at the four quarter phases —, ddc_mix, ddc_tap:
 * two fma chains from +0 in the order i = 0 .. ntaps - 1), so a host can compute the very words the device computes.
 * Out of scope, for a later pull request: per-source sample counts, squelching the demodulator (per-channel level of a tuner's own z: the channel meter, ABI 618, below; per bin of a raster:
 * the survey, ABI 613, below; which offsets of a source carry anything, under any configuration: the source spectrum, ABI 616, below).  (Sources above 16 x 48 kSPS: two stages,
 * ABI 610, below.  Channels on a raster: the polyphase channeliser, ABI 611, below.  Rates that are no integer multiple of 48 kSPS: the resampling tuner,
 * ABI 615, below.) */
#define M17HIP_IQ_U8 3    /* interleaved uint8 I,Q around 127.5 (rtl_sdr): (float)u - 127.5, exact.  Wideband input only: m17hip_upload_iq* refuses it */
/* The filter m17hip_wide_config takes by default — what a user of rtl_fm leaves to its built-in low-pass: ntaps = 32 * decim + 1, a Blackman-windowed
 * sinc with its cutoff at 5500 Hz of 48000 * decim, computed in double, scaled to unit DC gain and rounded to float.  No context is needed.  *ntaps is set
 * whenever decim is valid (1..16); M17HIP_EINVAL if it is not, if ntaps is NULL, or if taps is NULL or capacity < *ntaps (nothing written to taps). */
int m17hip_wide_default_taps(uint32_t decim, float* taps, uint32_t capacity, uint32_t* ntaps);
/* What the command line of rtl_sdr / rtl_fm says once per receiver: `sources` wide streams (1..256) at 48000 * decim (decim 1..16) in iq_format
 * (M17HIP_IQ_I16, M17HIP_IQ_F32 or M17HIP_IQ_U8), low-passed with taps[ntaps] (1..1024, finite; taps == NULL with ntaps == 0: the default taps).  It starts
 * every source's feed over (history zero, sample count 0) and may be called again to reconfigure (it waits for the tuner's launches in flight, not for a
 * demodulation run; a channel whose source no longer exists goes back to source 0, offset 0).  The channels' carries are left as they are.
 * M17HIP_EINVAL outside those limits; M17HIP_ESTATE between m17hip_demod_front and its run. */
int m17hip_wide_config(m17hip_ctx* ctx, uint32_t sources, uint32_t decim, int iq_format, const float* taps, uint32_t ntaps);
/* What rtl_fm's -f says per process: local channel c < n listens to source[c] at fcw[c] / 2^32 * 48000 * decim Hz from that source's centre (a signed
 * 32-bit frequency word).  Entries at n and above keep their value; a fresh table is all (0, 0).  It applies to the blocks uploaded AFTER the call — a
 * block already staged keeps the table it was tuned with — and it never waits for anything in flight (two device copies take turns, as for
 * m17hip_set_channel_polarity).  A retuned channel's carry (the last z) belongs to its OLD frequency: the first output behind a retune is one sample of
 * that mismatch; m17hip_demod_reset_channels is the clean cut.
 * M17HIP_EINVAL, with nothing changed: n > max_channels, a source at or above `sources`, NULL with n > 0.  M17HIP_ESTATE before m17hip_wide_config. */
int m17hip_wide_channels(m17hip_ctx* ctx, const uint32_t* source, const int32_t* fcw, uint32_t n);
/* The input of `channels` channels from one block of every source: what the pipe from rtl_sdr delivers.  p: [sources][pitch] interleaved I,Q of the
 * configured format; `samples` counts OUTPUTS per channel at 48 kSPS, every source row holds samples * decim complex samples, and pitch counts complex
 * samples (>= samples * decim).  The four functions are the four ways in of m17hip_upload_iq with its staging-pair semantics (m17hip_input_alternate,
 * m17hip_demod_front and m17hip_upload_wait work as for floats); the device forms read the caller's memory directly (a sample aligned to its own size),
 * under the completeness rule stated for m17hip_upload_iq_device*; the host forms copy the raw block into the buffer m17hip_upload_iq's host forms use.
 * They make a float stream: on an int16 stream M17HIP_ESTATE, as for m17hip_upload_iq; M17HIP_ESTATE also before m17hip_wide_config and between
 * m17hip_demod_front and its run.  M17HIP_EINVAL as for m17hip_upload_iq, the gain rule included.
 * THE FEED: blocks continue one another in call order.  Per source the last ntaps - 1 converted samples are carried on the device, and the context keeps
 * ONE running sample count: all sources advance together.  Per channel the carry is the float2 of ABI 608, here the last z (zero: the first output is +0).
 * m17hip_demod_reset zeroes histories, count and carries; m17hip_demod_reset_channels zeroes the listed channels' carries at once and leaves the sources
 * alone — they are not the channel's.  A context may use this family and m17hip_upload_iq* on one stream: the carry is then whatever the last block left.
 * Non-finite samples stay in the channels that listen to their source.  m17hip_timing_get index 9 is the tuner; m17hip_iq_bytes counts its memory. */
int m17hip_upload_wide(m17hip_ctx* ctx, const void* host, float gain, uint32_t channels, uint32_t samples, size_t pitch);
int m17hip_upload_wide_device(m17hip_ctx* ctx, const void* dev, float gain, uint32_t channels, uint32_t samples, size_t pitch);
int m17hip_upload_wide_async(m17hip_ctx* ctx, const void* host, float gain, uint32_t channels, uint32_t samples, size_t pitch);
int m17hip_upload_wide_device_async(m17hip_ctx* ctx, const void* dev, float gain, uint32_t channels, uint32_t samples, size_t pitch);

/* ---- wideband IQ input above 16 x: two decimation stages (ABI 610) -------------------------------------
 * m17hip_wide_config stops at 48000 * 16 = 768 kSPS, and the rates a dongle is run at to cover many channels lie above it (rtl_sdr: 0.96, 1.44, 1.92, 2.4,
 * 2.88 MSPS; at 2.4 MSPS one source holds 192 channels of 12.5 kHz).  Two integer stages, decim1 then decim2, each 1..16: the source's rate is
 * 48000 * decim1 * decim2.  Per channel, one kernel (csrc/m17_wide2_kernels.hpp):
 *     mixed[m] = x[m] * conj(nco(fcw * m))                             (as above; mixed[m] = 0 for m < 0)
 *     u[p]     = sum_{i < ntaps1} taps1[i] * mixed[p decim1 + decim1 - 1 - i]
 *     z[n]     = sum_{i < ntaps2} taps2[i] * u[n decim2 + decim2 - 1 - i]
 *     y[n]     = gain * arg(z[n] * conj(z[n-1]))
 * with the arithmetic of ABI 609 in both stages (ddc_mix per input sample, ddc_tap chains from +0 in tap order, fm_discriminate; core::ddc_fir2 is the host
 * form of these words).  The frequency word means fcw / 2^32 * 48000 * decim1 * decim2 Hz.  The first filter is short: all it has to do is keep what the first
 * decimation folds onto the channel out of it; the channel's own filter is the second, at 48000 * decim2.
 * Out of scope: more than two stages, and folding the oscillator into per-channel complex first-stage taps (other arithmetic, other words). */
/* The default taps of both stages.  Stage 2: m17hip_wide_default_taps(decim2) word for word (32 * decim2 + 1 taps).  Stage 1: 8 * decim1 + 1 taps, a
 * Blackman-windowed sinc with its cutoff at 24000 * decim2 Hz of 48000 * decim1 * decim2, in double, unit DC gain, rounded to float (decim1 == 1: one tap
 * of 1).  For decim1 and decim2 in 2..16 it is within 0.003 dB of unity over +-6 kHz and at least 69 dB down on every band k * 48000 * decim2 +- 12 kHz that
 * the first decimation folds onto the channel; no claim is made for decim2 == 1.  No context is needed.  *ntaps1 and *ntaps2 are set whenever both
 * decimations are valid; M17HIP_EINVAL if one is not, if ntaps1 or ntaps2 is NULL, or if a taps pointer is NULL or its capacity too small (nothing written). */
int m17hip_wide_default_taps2(uint32_t decim1, uint32_t decim2, float* taps1, uint32_t cap1, uint32_t* ntaps1, float* taps2, uint32_t cap2, uint32_t* ntaps2);
/* m17hip_wide_config in two stages: `sources` (1..256) at 48000 * decim1 * decim2 (each 1..16), taps1[ntaps1] (1..256) and taps2[ntaps2] (1..1024), all
 * finite; a NULL pointer with a count of 0 selects that stage's default taps.  In every other respect it is m17hip_wide_config: it starts the feeds over, may
 * be called again, waits for tuner launches in flight and never for a run, clears channels of sources that are gone, and returns M17HIP_ESTATE between
 * m17hip_demod_front and its run.  The two calls replace one another: whichever was made last decides which kernel the next upload launches.
 * m17hip_wide_channels and m17hip_upload_wide* serve both: under a two-stage configuration every source row holds samples * decim1 * decim2 complex
 * samples and pitch is at least that; a row of more than 2^32 - 1 complex samples is M17HIP_EINVAL.
 * THE FEED is the one described above.  Per source the last (ntaps2 - 1) * decim1 + ntaps1 - 1 converted samples are carried (the u in front of a block
 * are recomputed from them); per channel nothing but the float2 carry (the last z), so resets, retunes and the staged-block rule read as above.
 * m17hip_timing_get index 10 is this tuner (index 9 stays the single-stage one); m17hip_iq_bytes counts its memory. */
int m17hip_wide_config2(m17hip_ctx* ctx, uint32_t sources, uint32_t decim1, const float* taps1, uint32_t ntaps1, uint32_t decim2, const float* taps2,
                        uint32_t ntaps2, int iq_format);

/* ---- wideband IQ input on a channel raster: the polyphase channeliser (ABI 611) ---------------------------
 * The tuners pay for every channel separately: each mixes all its source's samples with its own oscillator and filters them once more.  Where the channels
 * of a source sit on a RASTER — `bins` = M channels spaced 48000 * decim / M Hz, as the 192 channels of 12.5 kHz in a 2.4 MSPS source do — mixing and
 * filtering are shared.  Bin b, -M/2 <= b < M/2, is centred b spacings from the source's centre; k = b mod M; m is the absolute index of a source sample
 * since the feed began (x[m] = 0 for m < 0), and output n of a block that began at sample count c0 has its newest sample at m_n = c0 + n decim + decim - 1,
 * the tuner's convention:
 *     z_b[n] = sum_{i < ntaps} taps[i] * x[m_n - i] * exp(-2 pi j k (m_n - i) / M)
 *     y_b[n] = gain * arg(z_b[n] * conj(z_b[n-1]))
 * — the single-stage tuner's z with the oscillator exactly on the raster — computed, per source and output, as a fold and one M-point DFT:
 *     w_n[r] = sum over i = i0, i0 + M, i0 + 2M, ... < ntaps of taps[i] * x[m_n - i],   i0 = (m_n - r) mod M,   r = 0 .. M-1
 *     z_b[n] = sum_{r < M} w_n[r] * exp(-2 pi j k r / M)
 * The phase of tap i depends on (m_n - i) mod M = r alone, so no correction factor remains and only c0 mod M enters (taken from all 64 bits of the count).
 * One kernel (csrc/m17_chan_kernels.hpp), a workgroup per source and tile of outputs.  The arithmetic is defined once for host and device
 * (m17cxx/detail/core.h): chan_fold — the two fma chains of ddc_tap from +0 in ascending i, zero history like any sample —; the DFT as two passes of small
 * direct DFTs over M = M1 x M2 (chan_factor: M2 the largest divisor of M whose square is at most M; accepted when M1 <= 16 — which covers 48, 64, 96, 120,
 * 128, 144, 192, 240 and 256, the 10, 12.5, 20 and 25 kHz rasters of the rates a dongle runs at; every other M is M17HIP_EINVAL), chan_pass1 and chan_pass2:
 * chains of chan_mac, four fma per step in a fixed order, from +0; the second pass is evaluated for the bins some channel listens to only.  fm_discriminate
 * is unchanged.  The twiddles exp(-2 pi j j / M) are DATA: made in one place, on the host, in double, rounded to float, exactly 0 / +-1 on the axes, and
 * tw[M - j] the conjugate of tw[j] to the bit; m17hip_wide_raster_twiddles returns the table the device is given, so a host computes the device's words
 * whatever its libm.
 * Out of scope, for a later pull request: a raster shifted by a fraction of a spacing, a raster in a source at a rational rate (the tuner for those: ABI 615, below), per-source sample counts.  (Which bins carry
 * anything — RSSI per bin: the raster survey, ABI 613, below.) */
/* The default taps of m17hip_wide_raster: the formula of m17hip_wide_default_taps (32 * decim + 1 taps, Blackman-windowed sinc, cutoff 5500 Hz) for
 * decim 1..64, word for word that function's for decim <= 16.  No context is needed.  *ntaps is set whenever decim is valid; M17HIP_EINVAL if it is not, if
 * ntaps is NULL, or if taps is NULL or capacity < *ntaps (nothing written to taps). */
int m17hip_wide_raster_default_taps(uint32_t decim, float* taps, uint32_t capacity, uint32_t* ntaps);
/* The twiddle table of a raster of `bins`: out[2 j], out[2 j + 1] = re, im of exp(-2 pi j j / bins), j < bins; capacity counts floats (>= 2 * bins).  No
 * context is needed.  M17HIP_EINVAL for a `bins` m17hip_wide_raster refuses, a NULL pointer or too small a capacity (nothing written). */
int m17hip_wide_raster_twiddles(uint32_t bins, float* out, uint32_t capacity);
/* m17hip_wide_config for a raster: `sources` (1..256) at 48000 * decim (decim 1..64) in iq_format, split into `bins` channels (see above for the values
 * accepted), low-passed with taps[ntaps] (1..4096, finite; NULL with 0: the default taps).  In every other respect it is m17hip_wide_config: it starts the
 * feeds over, may be called again, waits for tuner launches in flight and never for a run, leaves the carries, and returns M17HIP_ESTATE between
 * m17hip_demod_front and its run.  The three configurations replace one another: whichever call was made last decides which kernel the next upload
 * launches.  The channel table is kept across a call that leaves `bins` as it was (a channel whose source is gone goes back to source 0, bin 0); a call that
 * changes the kind of configuration or `bins` starts the table over — a frequency word is no bin, nor is a bin of one raster a bin of another.
 * m17hip_upload_wide* serve it as they serve the tuners: rows hold samples * decim complex samples.  THE FEED is the one described above: per source the
 * last ntaps - 1 converted samples, per channel the float2 carry (the last z); m17hip_demod_reset and m17hip_demod_reset_channels as for the tuners.
 * m17hip_timing_get index 11 is the channeliser; m17hip_iq_bytes counts its memory. */
int m17hip_wide_raster(m17hip_ctx* ctx, uint32_t sources, uint32_t decim, uint32_t bins, int iq_format, const float* taps, uint32_t ntaps);
/* m17hip_wide_channels for a raster: local channel c < n listens to bin[c] of source[c]; several channels may name the same (source, bin).  Entries at n
 * and above keep their value; a fresh table is all (0, 0).  It applies to the blocks uploaded AFTER the call — a block already staged keeps the table it was
 * tuned with — and never waits for anything in flight (two device tables take turns).  The retune and carry rules are m17hip_wide_channels'.
 * M17HIP_EINVAL, with nothing changed: n > max_channels, a source at or above `sources`, a bin outside [-bins/2, bins/2), NULL with n > 0.
 * TABLE OWNERSHIP: each table call returns M17HIP_ESTATE under a configuration that is not its own — this one before m17hip_wide_raster or under a tuner,
 * m17hip_wide_channels under a raster. */
int m17hip_wide_raster_channels(m17hip_ctx* ctx, const uint32_t* source, const int32_t* bin, uint32_t n);

/* ---- the raster survey: per-bin power of every source beside the channeliser (ABI 613) -----------------------
 * m17hip_wide_raster_channels takes (source, bin) pairs; this says which bins carry anything, without a demodulator channel on them: survey, pick, assign,
 * demodulate.  With the survey on at `stride`, every wideband block uploaded under a raster is surveyed beside its channeliser:
 *     c0 = the feed's 64-bit sample count at the block's start (a multiple of decim), N0 = c0 / decim;
 *     output n of the block is a SURVEY TIME iff (N0 + n + 1) % stride == 0 — a property of the feed, not of how it is cut into blocks; the block's
 *     survey times are t_0 < ... < t_{J-1}, and J may be 0;
 *     for every source s and every k < bins, z_k[t_j] is the word the channeliser computes for bin k at output t_j (chan_fold, chan_pass1, chan_pass2 over
 *     the same history, the same count mod bins and the same twiddle table), whether or not any channel listens to s or k;
 *     p_j = chan_power(z.re, z.im) = fmaf(re, re, im * im);
 *     q_g = the chain from +0 of plain float adds of p_j, j = 16 g .. min(16 g + 15, J - 1), ascending (CHAN_SURVEY_GROUP = 16);
 *     P[s][k] = the chain from +0 of plain float adds of q_g, g ascending.  With J = 0 every P is +0.
 * The two-level order is part of the definition (m17cxx/detail/core.h has chan_power and the group size, so a host computes the device's words): a grid of
 * (group, source) workgroups does the first level and a fixed-order kernel the second — no atomics, no serial chain over a long block.  Two kernels
 * (csrc/m17_chan_survey_kernels.hpp) on the block's own stream behind the channeliser: m17hip_upload_wait and the in-place forms' synchronisation cover
 * them, the floats the channels get are untouched, and with the survey off a block queues exactly what it queued under ABI 611.  m17hip_timing_get index 12
 * is the survey (both kernels, one entry per block); m17hip_iq_bytes counts its scratch and planes.
 * Out of scope, for a later pull request: a waterfall of per-time spectra, channel assignment on the device, squelching the demodulator itself.  (Under
 * the tuners, which share no z: the spectrum of the source block itself, ABI 616, below.) */
/* stride 0 turns the survey off (the default); 1..4096 turns it on for the blocks uploaded AFTER the call — a block already staged is not surveyed
 * retroactively.  It never waits for anything in flight.  Planes of blocks surveyed before the call are no longer fetched.  M17HIP_ESTATE unless the last
 * wideband configuration is a raster, and between m17hip_demod_front and its run; M17HIP_EINVAL for a stride above 4096 or a NULL context.  Every
 * m17hip_wide_config, m17hip_wide_config2 or m17hip_wide_raster call turns the survey off: the plane's shape belongs to the configuration. */
int m17hip_wide_survey(m17hip_ctx* ctx, uint32_t stride);
/* The plane of the latest block uploaded with the survey on (back = 0) or of the block before it (back = 1; two planes and two events take turns):
 * power_host[sources][bins] floats, indexed by k = bin mod bins; *times = J and *first_output = N0 of that block (either may be NULL).  It waits for that
 * block's survey kernels only, on an event recorded behind the second of them — never for a demodulation run or a later block.  M17HIP_ESTATE if no such
 * plane exists: the survey is off, no block (or, for back = 1, one block) since it was turned on, or none since m17hip_demod_reset, which starts the feeds
 * over.  M17HIP_EINVAL for back > 1, a NULL power_host or capacity (in floats) < sources * bins; nothing is written then. */
int m17hip_wide_survey_fetch(m17hip_ctx* ctx, uint32_t back, float* power_host, uint64_t capacity, uint32_t* times, uint64_t* first_output);

/* ---- the source spectrum: averaged periodogram of every wideband source, under every configuration (ABI 616) ---
 * The three tuners take frequency words, and a user had to know every carrier's offset before m17hip_wide_channels was of any use: they share no z, so no
 * survey serves them.  What every configuration shares is the source block.  With the spectrum on at N = `points` and `hop`, every wideband block uploaded
 * is transformed beside whichever kernel the configuration launches:
 *     c0 = the feed's 64-bit sample count at the block's start, W = the block's complex samples per source row, x = its samples as floats (int16 and float32
 *     as they are, uint8 minus 127.5);
 *     FRAME f starts at block sample a_f = first + f * hop, first = (hop - c0 mod hop) mod hop from all 64 bits of the count — where the feed's absolute
 *     sample index is a multiple of hop: a property of the feed, not of how it is cut into blocks; J = the number of f with a_f + N <= W.  A frame that would
 *     straddle a block's end is not taken (no history, no carried state), and J may be 0;
 *     v[i] = (w[i] * re x[a_f + i], w[i] * im x[a_f + i]), two plain multiplies, w the window;
 *     X = the N-point DFT of v, X[k] = sum_i v[i] exp(-2 pi j k i / N), evaluated as a radix-2 decimation-in-time FFT: v is loaded in bit-reversed order,
 *     then stages s = 1 .. log2 N in ascending order; butterfly j < N / 2 of stage s pairs the elements i and i + h, h = 2^(s-1), i = 2 h (j div h) + j mod
 *     h, with t = tw[(j mod h) * N / 2^s] as
 *         (a, b) <- (a + b t, a - b t):   re' = fmaf(-b.im, t.im, fmaf(b.re, t.re, a.re)),  im' = fmaf(b.im, t.re, fmaf(b.re, t.im, a.im))
 *     — core::chan_mac onto a, for the difference with (-t.re, -t.im) in t's place — ONE formula for every butterfly of every stage, the twiddles on the axes
 *     included, so a non-finite sample gives the same words on host and device (it reaches every bin of its frame and of no other);
 *     p = chan_power(X[k].re, X[k].im) = fmaf(re, re, im * im);
 *     q_g = the chain from +0 of plain float adds of frame j's p, j = 16 g .. min(16 g + 15, J - 1), ascending (CHAN_SURVEY_GROUP = 16);
 *     P[s][k] = the chain from +0 of plain float adds of q_g, g ascending.  With J = 0 every P is +0.
 * P[s][k], k < N, belongs to the frequency k * Fs / N for k < N / 2 and (k - N) * Fs / N otherwise, measured from the source's centre at its sample rate Fs
 * — the survey's index rule.  The twiddles tw[j] = exp(-2 pi j j / N), j < N / 2, are DATA: made on the host in double and rounded to float, exactly (1, 0)
 * at j = 0 and (0, -1) at j = N / 4, and tw[N / 2 - j] = (-re, im) of tw[j] to the bit; m17hip_wide_spectrum_twiddles returns the table the device is
 * given.  m17cxx/detail/core.h has spec_frames, spec_window, spec_bitrev, spec_butterfly and spec_item1 (and spec_item2: two stages in one pass, the same
 * words), so a host computes the device's words.  Two kernels on the block's own stream (csrc/m17_spectrum_kernels.hpp; the second is the survey's
 * chan_survey_sum_kernel) behind the configuration's kernel: they read the source block only, m17hip_upload_wait and the in-place forms' synchronisation
 * cover them, the floats the channels get are untouched, and with the spectrum off a block queues exactly what it queued under ABI 615.
 * m17hip_timing_get index 14 is the spectrum (both kernels, one entry per block); m17hip_iq_bytes counts its table, scratch and planes.  The scratch is
 * sources * ceil(J / 16) * N floats: a hop far below N over a long block asks for as much memory as that says, and a block whose scratch cannot be had
 * fails with M17HIP_ENOMEM.
 * Out of scope, for a later pull request: a waterfall of per-frame spectra, frames that straddle blocks, squelching
 * the demodulator, assigning channels on the device. */
/* points = 0 turns the spectrum off (the default).  Otherwise points is a power of two in 64..4096, hop is in 1..2^24 and window[nwindow] holds `points`
 * finite floats; NULL with a count of 0 selects m17hip_wide_spectrum_default_window's.  It holds for the blocks uploaded AFTER the call and never waits for
 * anything in flight: window and twiddles travel with the next block.  (What a change can cost is paid by that NEXT upload, not by this call: where
 * `points` has risen the upload regrows the two planes, and where the block needs more scratch than any before it the scratch; either waits on the host
 * for the blocks still in flight.)  Planes of blocks transformed before the call are no longer fetched.  Legal under
 * EVERY wideband configuration, the raster included, and independent of m17hip_wide_survey.  M17HIP_EINVAL outside the limits (a NULL context included),
 * with nothing changed; M17HIP_ESTATE before any wideband configuration and between m17hip_demod_front and its run.  Every m17hip_wide_config,
 * m17hip_wide_config2, m17hip_wide_raster or m17hip_wide_resample call turns it off: the plane has a row per source. */
int m17hip_wide_spectrum(m17hip_ctx* ctx, uint32_t points, uint32_t hop, const float* window, uint32_t nwindow);
/* The default window: the four-term minimum Blackman-Harris window in its periodic form, w[i] = 0.35875 - 0.48829 cos(2 pi i / N) + 0.14128 cos(4 pi i / N)
 * - 0.01168 cos(6 pi i / N), computed in double and rounded to float.  No context is needed.  M17HIP_EINVAL for points that m17hip_wide_spectrum refuses
 * (0 included), a NULL out or capacity (in floats) < points; nothing is written then. */
int m17hip_wide_spectrum_default_window(uint32_t points, float* out, uint32_t capacity);
/* The twiddle table as described above: points / 2 pairs (re, im), `points` floats.  No context is needed.  M17HIP_EINVAL as for the default window. */
int m17hip_wide_spectrum_twiddles(uint32_t points, float* out, uint32_t capacity);
/* The plane of the latest block uploaded with the spectrum on (back = 0) or of the block before it (back = 1; two planes and two events take turns):
 * power_host[sources][points] floats; *frames = J and *first_sample = c0 + first of that block (either may be NULL).  It waits for that block's spectrum
 * kernels only, on an event recorded behind the second of them, and copies on a stream of its own — never for a demodulation run or a later block.
 * M17HIP_ESTATE if no such plane exists: the spectrum is off, no block (or, for back = 1, one block) since it was turned on, or none since
 * m17hip_demod_reset, which starts the feeds over.  M17HIP_EINVAL for back > 1, a NULL power_host or capacity (in floats) < sources * points; nothing is
 * written then. */
int m17hip_wide_spectrum_fetch(m17hip_ctx* ctx, uint32_t back, float* power_host, uint64_t capacity, uint32_t* frames, uint64_t* first_sample);

/* ---- the channel meter: level, offset and deviation sums per wideband channel, under every configuration (ABI 618) ---
 * The discriminator keeps arg(z[n] conj z[n-1]) and throws |z| away; the survey and the spectrum describe the SOURCE.  With the meter on at `window` (in
 * outputs, 16..65536) every wideband block uploaded under m17hip_wide_config, _config2, _wide_raster or _wide_resample leaves three sums per channel and per
 * stretch of time, taken where z and y already exist:
 *     T = the block's outputs per channel; N0 = the 64-bit number of outputs the feed produced before the block (0 after m17hip_demod_reset or a
 *     configuration); a0 = N0 mod window, taken on the host from all 64 bits; K = (a0 + T - 1) div window + 1;
 *     PIECE k < K of the block holds the outputs n with (a0 + n) div window == k: m_k outputs, lo_k .. lo_k + m_k - 1.  Windows are a property of the feed,
 *     not of its blocks: a window that a block boundary cuts is reported in two pieces, one per block, and nothing is carried;
 *     for channel c and output n: p = chan_power(z.re, z.im) = fmaf(re, re, im * im) of the very z[n] the configuration's kernel discriminates; y = the float
 *     that kernel stores into the input slab (before any polarity, with the gain of the upload call); e = y * y, one rounded multiply, not contracted;
 *     for each quantity v in (p, y, e) and each piece: q_g = the chain from +0 of plain float adds of v over the outputs lo_k + 16 g .. min(lo_k + 16 g + 15,
 *     lo_k + m_k - 1), ascending; V[c][k] = the chain from +0 of plain adds of q_g, g ascending — the survey's two levels and CHAN_SURVEY_GROUP; the order
 *     is part of the definition.
 * The plane of a block is [3][C][K] floats (sum p, sum y, sum e), C the upload call's channel count.  m17cxx/detail/core.h has meter_pieces, meter_piece,
 * meter_sq and meter_sum, so a host computes the device's words.  sum p / m is the channel's power (amplitude^2 in the units of the source's samples, through
 * the configuration's filter); (sum y / m) * 48000 / (2 pi gain) is the carrier's offset in Hz from the channel's frequency word; the variance of y, by the
 * same factor, is the deviation (an M17 carrier: its +-2400 Hz; an empty FM channel: discriminator noise several times wider — the classic noise squelch).
 * On the device the configuration's kernel runs in a metered instantiation that stores p beside y (one more float per output, into a scratch [C][T]), and
 * wide_meter_kernel (csrc/m17_meter_kernels.hpp) follows on the block's own stream: m17hip_upload_wait and the in-place forms' synchronisation cover it,
 * the floats the channels get are untouched, and with the meter off a block queues exactly what it queued under ABI 617.  m17hip_timing_get index 16 is the
 * meter kernel (one entry per block; the metered tuner keeps its own index); m17hip_iq_bytes counts the scratch and the planes.  A block whose scratch
 * cannot be had fails with M17HIP_ENOMEM.
 * Out of scope, for a later pull request: squelching the demodulator or the gate-aware front end from the meter, retuning a channel on the device from its
 * offset, a level per call in the call log, a peak-hold or a histogram, windows carried across blocks; tests of the meter under other calls in flight beyond one
 * staged and one in-place block. */
/* window = 0 turns the meter off (the default); 16..65536 turns it on for the blocks uploaded AFTER the call.  It never waits for anything in flight.
 * Planes of blocks measured before the call are no longer fetched.  M17HIP_EINVAL for 1..15, above 65536 or a NULL context; M17HIP_ESTATE before any
 * wideband configuration and between m17hip_demod_front and its run.  Every m17hip_wide_config, m17hip_wide_config2, m17hip_wide_raster or
 * m17hip_wide_resample call turns it off; m17hip_demod_reset keeps it on and starts N0 over; m17hip_demod_reset_channels does not touch it. */
int m17hip_wide_meter(m17hip_ctx* ctx, uint32_t window);
/* The shape of the latest block uploaded with the meter on (back = 0) or of the one before it (back = 1): C, K, N0 div window (the feed's window that piece
 * 0 belongs to), N0 and T.  Any pointer may be NULL.  It does not wait.  M17HIP_ESTATE if no such plane exists: the meter is off, no block (or, for
 * back = 1, one block) since it was turned on, or none since m17hip_demod_reset.  M17HIP_EINVAL for back > 1 or a NULL context; nothing is written then. */
int m17hip_wide_meter_shape(m17hip_ctx* ctx, uint32_t back, uint32_t* channels, uint32_t* pieces, uint64_t* first_window, uint64_t* first_output,
                            uint32_t* outputs);
/* The plane of that block: planes_host[3][C][K] floats.  It waits for that block's meter kernel only, on an event recorded behind it, and copies on a stream
 * of its own — never for a demodulation run or a later block.  M17HIP_ESTATE as for the shape; M17HIP_EINVAL for back > 1, a NULL context or planes_host,
 * or capacity (in floats) < 3 C K; nothing is written then. */
int m17hip_wide_meter_fetch(m17hip_ctx* ctx, uint32_t back, float* planes_host, uint64_t capacity);

/* ---- the spectrum squelch: the three tuners skip the channels whose band holds no carrier (ABI 619) -------------
 * m17hip_wide_config, _config2 and _wide_resample tune every channel of every block, transmitting or not.  What can say beforehand that a channel is silent
 * is the source spectrum (ABI 616): it reads the source block alone and costs a hundredth of a tuner.  With the squelch on, per block uploaded:
 *     N = the spectrum's points, J = the spectrum's frame count of THIS block, P = its plane [sources][N], B = half_bins;
 *     for channel c with source s and frequency word fcw (signed 32 bit):
 *     k_c = (((int64)fcw + 2^(31 - log2 N)) >> (32 - log2 N)) & (N - 1), the shift arithmetic (a floor): the spectrum's index rule — bin k belongs to
 *     k Fs / N — in integers, to the nearest bin; it holds for all three tuners, because the word is relative to the source's own rate;
 *     b_c = the chain from +0 of plain float adds of P[s][(k_c + d) & (N - 1)], d = -B .. B ascending;
 *     to = open_level[s] * (float)J and tc = close_level[s] * (float)J, one rounded multiply each.  The levels are per SOURCE: dongles differ in gain;
 *     h = the channel's hold count before the block: 0 after a configuration, after m17hip_wide_squelch, after m17hip_demod_reset and, for the listed
 *     channels, after m17hip_demod_reset_channels; a retune by m17hip_wide_channels keeps it;
 *     J == 0: the channel is OPEN and h' = h (a block too short for a frame is never silenced for want of a measurement);
 *     else !(b_c < to): h' = hang + 1; else h > 0 and !(b_c < tc): h' = hang + 1; else h' = h > 0 ? h - 1 : 0; the channel is open iff h' > 0.
 *     The comparisons are negated so that a NaN band opens the channel as well.
 * m17cxx/detail/core.h has squelch_bin, squelch_band, squelch_level and squelch_step, so a host computes the device's words.
 * An OPEN channel gets exactly the words the unsquelched kernel gives it from the same carry.  A CLOSED channel gets y = +0.0f for all T outputs of the
 * block, +0 in the meter's power scratch where the meter is on, and (0, 0) as its carry for the next block: the first output after a reopening is
 * fm_discriminate against a zero z, +0 (the zero-product rule), and every later output is the unsquelched word, since the sources' histories are kept
 * regardless.
 * On the device the block's spectrum moves IN FRONT of the tuner on the block's stream, wide_squelch_kernel (csrc/m17_squelch_kernels.hpp, a lane per
 * channel) follows it, and the tuner runs in a squelched instantiation whose workgroups read the channel's state word first: a closed workgroup stores its
 * tile's zeros and returns before it mixes a sample.  What m17hip_wide_spectrum_fetch returns and waits for does not change.  With the squelch off a block
 * queues exactly what it queued under ABI 618.  m17hip_timing_get index 17 is the squelch kernel (the spectrum and the tuner keep theirs); m17hip_iq_bytes
 * counts the levels, the hold counts and the fetch planes.
 * A transmission that begins in a block's last moments — behind the last frame the spectrum takes, or too short in it to lift the band over the level — is
 * not heard until the next block: its start is lost.  The loss is bounded by one block, so a receiver that must keep a transmission's link setup frame
 * (40 ms) uploads blocks no longer than the preamble it can count on, covers the block with frames (hop <= points), and sets the open level low enough
 * that a carrier present for one frame in J lifts the band over it: open_level * J below floor * (J - 1) + carrier.
 * Out of scope here: a floor estimated on the device (the median: m17hip_wide_squelch_floor below, ABI 621); squelch under the raster; driving the demodulator's gate-aware front
 * end or its frame cycle from the squelch; a look-back ACROSS a block boundary that re-tunes the block before an opening (within a block,
 * m17hip_wide_squelch_slots below decides per slot and has a lead); compacting the grid to open channels; AFC; tests of the squelch under deep in-flight call
 * orders beyond one staged and one in-place block. */
/* open_level == NULL with nlevels == 0 turns the squelch off (the default).  Otherwise half_bins is in 0..64 and below points / 2, the levels are finite
 * with 0 < close_level[s] <= open_level[s], nlevels == sources and hang is in 0..65535 (blocks a channel stays open behind the last block whose band held
 * it open).  It holds for the blocks uploaded AFTER the call and never waits for anything in flight: the levels travel to the device with the next block, in
 * a copy that no queued launch reads.  M17HIP_EINVAL outside the limits or for a NULL context, with nothing changed.  M17HIP_ESTATE, with nothing changed:
 * before any wideband configuration; between m17hip_demod_front and its run; and, when turning it on, with the spectrum off or under m17hip_wide_raster
 * (the channeliser's work is shared by a source's channels: there is nothing per channel to save, and the raster survey serves that case).  Every
 * m17hip_wide_spectrum call and every m17hip_wide_config, m17hip_wide_config2, m17hip_wide_raster or m17hip_wide_resample call turns it off. */
int m17hip_wide_squelch(m17hip_ctx* ctx, uint32_t half_bins, const float* open_level, const float* close_level, uint32_t nlevels, uint32_t hang);
/* The decision of the latest block uploaded with the squelch on (back = 0) or of the one before it (back = 1): state_host[c] = h' | open << 31 and
 * band_host[c] = b_c for the block's channels; *channels their number, *frames the block's J (either may be NULL).  Two planes and two events take turns.  It
 * waits for that block's squelch kernel only — not for its tuner, a run or a later block — and copies on a stream of its own.  M17HIP_ESTATE if no such
 * plane exists: the squelch is off, no block (or, for back = 1, one block) since it was turned on, or none since m17hip_demod_reset.  M17HIP_EINVAL for
 * back > 1, a NULL context, state_host or band_host, or capacity (in channels) below the block's channel count; nothing is written then. */
int m17hip_wide_squelch_fetch(m17hip_ctx* ctx, uint32_t back, uint32_t* state_host, float* band_host, uint64_t capacity, uint32_t* channels, uint32_t* frames);

/* ---- the time-resolved squelch: a decision per SLOT of a block, a skip per TILE of the tuner's outputs (ABI 620) --------------------------------------
 * m17hip_wide_squelch takes one decision per channel and block, so a carrier keyed for part of a block is diluted by the silent part (12 dB over the floor
 * for a fifth of the block lifts the block's band by 6 dB), and a strong one opens the whole block.  This second mode, exclusive with that one, decides per
 * group of 16 frames of the block's spectrum and lets the tuners skip per tile.  Per block uploaded with it on, N, hop, first and J as for the spectrum:
 *     SLOTS.  G = ceil(J / 16); slot g holds J_g = min(16, J - 16 g) frames; its row Q[s][g][.] is the spectrum's first-level sum for source s: the chain from
 *     +0 of chan_power over the slot's frames, ascending (what spectrum_kernel leaves in its scratch).  The plane m17hip_wide_spectrum_fetch returns is the same.
 *     BAND AND THRESHOLDS.  For channel c with source s: k_c = squelch_bin(fcw, log2 N), b_{c,g} = squelch_band(Q[s][g], N, k_c, B), and the thresholds are
 *     squelch_level(open_level[s], J_g) and squelch_level(close_level[s], J_g): the four functions of ABI 619, unchanged.
 *     RECURRENCE.  w_g = squelch_step(h_{g-1}, b_{c,g}, to_g, tc_g, hang, J_g), g = 0 .. G - 1; h_g is the low 31 bits of w_g, open_g its top bit; h_{-1} is the
 *     channel's hold count carried from the block before: 0 after a configuration, after either squelch call, after m17hip_demod_reset and, for the listed
 *     channels, after m17hip_demod_reset_channels; a retune keeps it.  hang counts SLOTS.  The block leaves h_{G-1} as the hold count and w_{G-1} as the
 *     channel's state word.  J == 0: every tile of the block is open, the hold count stays and the state word is h | 1 << 31.
 *     TILES.  TO = the tuner's outputs per workgroup: 255 under m17hip_wide_config and _config2, groups x up under m17hip_wide_resample.  Tile t holds the
 *     outputs [t TO, min((t + 1) TO, T)) of the block's T and spans the block samples [a_t, e_t), a_t = floor(t TO W / T), e_t = floor(min((t + 1) TO, T) W / T)
 *     of the block's W, in 64 bits.  slot(x) = 0 for x < first, else min((x - first) / (16 hop), G - 1).  Tile t is OPEN iff open_g holds for some g in
 *     slot(a_t) .. min(slot(e_t - 1) + lead, G - 1).  `lead` opens the tiles in front of an opening WITHIN the block: it cannot reach back into the block
 *     before, which has left the device's hands.
 * m17cxx/detail/core.h has squelch_slots, squelch_slot_frames, squelch_slot_of, squelch_tile_span and squelch_tile_open: one text for host and device.
 * An OPEN tile gets exactly the words the unsquelched kernel gives it from the same carry; a tile behind a closed one recomputes the z in front of its first
 * output as every tile does, so its first output is the unsquelched word.  A CLOSED tile gets +0 for its outputs, +0 in the meter's power scratch where the
 * meter is on, and (0, 0) as the carry where it holds output T - 1: the zero-product rule shows only at output 0 of a block whose predecessor's last tile
 * was closed.
 * On the device the block's spectrum goes in front of the tuner as under ABI 619; three kernels follow it (csrc/m17_squelch_kernels.hpp: the bands, a lane per
 * channel and slot; the recurrence, a lane per channel; the tile mask, a lane per channel and 32 tiles) and the tuner runs in a tile-squelched
 * instantiation.  m17hip_timing_get index 18 is the three kernels, one entry per block; m17hip_iq_bytes counts the planes, which grow with the block's shape
 * (M17HIP_ENOMEM from the upload when they cannot be had).
 * Arguments, limits, refusals and what turns it off are m17hip_wide_squelch's, plus lead in 0..255.  NULL / 0 levels turn the squelch off whichever mode was
 * on; each of the two calls replaces the other's mode and starts the hold counts over. */
int m17hip_wide_squelch_slots(m17hip_ctx* ctx, uint32_t half_bins, const float* open_level, const float* close_level, uint32_t nlevels, uint32_t hang,
                              uint32_t lead);
/* The decisions of the latest block uploaded in slot mode (back = 0) or of the one before it (back = 1): state_host[c] = w_{G-1}, bands_host[c * G + g] =
 * b_{c,g}, mask_host[c * ceil(tiles / 32) + (t >> 5)] bit t & 31 = tile t open; *channels, *slots = G, *tiles and *frames = J (each may be NULL).  Two plane
 * sets and two events take turns.  It waits for that block's squelch kernels only and copies on the fetch stream.  M17HIP_ESTATE if no such plane exists
 * (as m17hip_wide_squelch_fetch, or the block mode is on; m17hip_wide_squelch_fetch returns it under slot mode).  M17HIP_EINVAL for back > 1, a NULL
 * context, state_host, bands_host or mask_host, cap_channels < C, cap_bands < C G or cap_mask_words < C ceil(tiles / 32); nothing is written then. */
int m17hip_wide_squelch_slots_fetch(m17hip_ctx* ctx, uint32_t back, uint32_t* state_host, float* bands_host, uint32_t* mask_host, uint64_t cap_channels,
                                    uint64_t cap_bands, uint64_t cap_mask_words, uint32_t* channels, uint32_t* slots, uint32_t* tiles, uint32_t* frames);

/* ---- the sources' noise floor on the device: both squelch modes' levels from the block's own plane (ABI 621) ------------------------------------------
 * Both modes above compare against levels the caller supplies, which a receiver gets by fetching a plane, taking its median on the host and calling the
 * squelch again: a round trip, and levels that are wrong as soon as the floor moves (a rise by more than the open margin opens every channel of the source
 * in every block; a fall loses the weak carriers).  With this mode on, a kernel in front of the squelch kernels makes the block's levels from the block's
 * plane, so the floor applies to the very block it was measured on and no host takes part.  Per block uploaded with it on: N the spectrum's points, J the
 * block's frames, P[s][N] the block's plane (what m17hip_wide_spectrum_fetch returns; under the slot mode the same second-level sum, not a slot's row),
 * B = half_bins of the squelch mode that is on:
 *     KEY.  squelch_floor_key(x) = x != x ? 0xFFFFFFFF : bits(x).  Powers are sums of chan_power from +0, so no non-NaN value has its sign bit set: ascending
 *     key order is ascending value order, every NaN last.
 *     MEDIAN.  med_s = the row's UPPER MEDIAN: the element whose key has rank N / 2 (0-based) among the row's N keys in ascending order; where that key is
 *     0xFFFFFFFF, the quiet NaN 0x7FC00000.  A selection, not an average of two: every correct algorithm gives the same word.  It is deliberately NOT
 *     np.median's mean of the two middle values in float64 (m17hip.wide_squelch_levels takes that one).  With N / 2 - 1 bins raised by carriers the median
 *     is still a floor bin; with N / 2 or more it is a raised one.
 *     FLOOR.  f = squelch_floor(med, B, J) = (med * (float)(2 B + 1)) / (float)J, two rounded operations, then f = f < floor_min ? floor_min : f; a NaN
 *     stays a NaN.  Only taken for J >= 1.
 *     TRACK.  F = the source's carried floor, a NaN in front of the first block.  squelch_track(F, f, rise, fall): F is a NaN -> f, whatever it is; else f
 *     not finite -> F; else a = f > F ? rise : fall and a >= 1 ? f : fmaf(a, f - F, F).  A block with J == 0 leaves F as it is.
 *     LEVELS.  open_level[s] = F' * open_ratio, close_level[s] = F' * close_ratio, one rounded multiply each; they are per frame, and squelch_level(level, J)
 *     and squelch_level(level, J_g) of the two modes take them as they take given levels.  A NaN level opens every channel of the source (squelch_step's
 *     comparisons are negated: the fail-open rule): the state in front of the first block with a frame.
 * m17cxx/detail/core.h has squelch_floor_key, squelch_floor_median, squelch_floor, squelch_track and squelch_floor_level: one text for host and device.
 * On the device squelch_floor_kernel (csrc/m17_squelch_kernels.hpp; a workgroup per source, the keys in LDS, a radix select in four 8-bit passes over an LDS
 * histogram of integer counts) goes between the block's spectrum and the mode's kernels, which are unchanged and read the open | close rows of the floor
 * plane in place of the table of given levels; that table is neither uploaded nor read while the mode is on and serves again when it is turned off.  The
 * carry F[sources] is the feed's, ordered across the two streams like the hold counts, and starts over (NaN) wherever those are zeroed: after a
 * configuration, either squelch call, this call and m17hip_demod_reset.  m17hip_demod_reset_channels zeroes the listed hold counts and leaves the floor; a
 * retune keeps both.  m17hip_timing_get index 19 is the kernel, one entry per block; m17hip_iq_bytes counts the carry and the two floor planes.
 * The call needs one of the two squelch modes on; half_bins, hang and lead stay that mode's and its given levels are set aside.  It holds for the blocks
 * uploaded after it and never waits for anything in flight; it starts the hold counts and the floor over, as either squelch call does.  open_ratio == 0 &&
 * close_ratio == 0 turns it off: the given levels serve again from the next block.  Every m17hip_wide_squelch and _squelch_slots call (they carry levels)
 * turns it off, and so does everything that turns the squelch itself off.  m17hip.wide_squelch_ratio(dB) = 10^(dB / 10).
 * M17HIP_EINVAL, nothing changed: a NULL context; a non-finite argument; ratios outside 0 < close_ratio <= open_ratio, the off pair excepted; rise or fall
 * outside (0, 1]; floor_min < 0.  M17HIP_ESTATE, nothing changed: no wideband configuration; between m17hip_demod_front and its run; turning it on with no
 * squelch mode on.
 * OUT OF SCOPE: a floor per slot, or one that ignores bins already known to hold carriers; percentiles other than the median; per-source ratios; the
 * carrier list (wide_spectrum_carriers) and channel assignment on the device (m17hip_wide_scan below, ABI 622); the raster; the demodulator's behaviour on long runs of exact zeros
 * (NOTES.md; unchanged here); compacting the grid; AFC. */
int m17hip_wide_squelch_floor(m17hip_ctx* ctx, float open_ratio, float close_ratio, float rise, float fall, float floor_min);
/* The floor plane of the latest block uploaded with the mode on (back = 0) or of the one before it (back = 1): plane_host[4][sources] = med | F' | open_level |
 * close_level; *sources and *frames = J (each may be NULL).  Two planes take turns with the squelch's state planes and share their events: a plane whose
 * turn it is not keeps its words.  It waits for that block's floor and squelch kernels only — not for its tuner, a run or a later block — and copies on the
 * squelch's fetch stream.  M17HIP_ESTATE if no such plane exists: the mode is off, not enough blocks since it was turned on, or none since
 * m17hip_demod_reset.  M17HIP_EINVAL for back > 1, a NULL context or plane_host, or capacity (in floats) below 4 x sources; nothing is written then. */
int m17hip_wide_squelch_floor_fetch(m17hip_ctx* ctx, uint32_t back, float* plane_host, uint64_t capacity, uint32_t* sources, uint32_t* frames);

/* ---- the carrier scan: the block's carriers found and a pool of channels tuned to them on the device (ABI 622) ------------------------------------------
 * Who transmits where was the host's to decide: m17hip.wide_spectrum_carriers is numpy on a fetched plane (a wait for the device; nothing for C and C++),
 * and a carrier it finds is tuned a block late at the earliest, because m17hip_wide_channels holds for the blocks uploaded after it — an M17 transmission
 * has then lost its link setup frame and the receiver waits for the LICH to come round.  With this mode on, a kernel between the block's floor kernel and its
 * squelch kernel finds the carriers of the block in its own plane and writes the frequency words of a pool of channels, so a transmission is tuned in the
 * block in which it first appears.  It needs m17hip_wide_spectrum at no more than 4096 points, m17hip_wide_squelch (the block mode) and
 * m17hip_wide_squelch_floor, under one of the three tuners.
 * pool[c] != 0 makes local channel c < n a SLOT; channels at n and above are none.  A slot belongs to the source its m17hip_wide_channels entry names; the
 * slots of source s among the block's channels, in ascending channel order, are that source's pool in that block (a slot at or above the block's channel
 * count keeps its word).  At most 256 slots per source, checked per block against the table in force: the upload returns M17HIP_ESTATE, nothing queued.
 * guard_bins = X, 3 .. points / 4: the least distance of two reported carriers, and the distance within which a held slot covers a peak
 * (m17hip.wide_scan_guard_bins: ceil(9000 / (rate / points))).  Per block and source, N the points, J the block's frames, B the squelch's half_bins,
 * row = the source's row of the plane, med | . | open | close the source's column of the block's floor plane, to = squelch_level(open, J), tc likewise:
 *     BAND.  band[k] = squelch_band(row, N, k, B) of EVERY bin, unchanged.
 *     PEAK.  scan_peak(band, N, k, X, to): bin k is a peak iff band[k] >= to — a true comparison: a NaN band is no peak — and no bin j within circular
 *     distance X beats it; j beats k iff band[j] > band[k], or band[j] == band[k] && j < k (a NaN neighbour beats nothing).  A local maximum, deliberately
 *     not wide_spectrum_carriers' greedy pick with shoulders: it does not depend on the order of evaluation, so it is parallel, and a monotone skirt is
 *     never a peak (its inner neighbour beats it).  A row flat to the bit has exactly one candidate, bin 0.
 *     WORD.  scan_fcw(row, N, logn, k, B, med): w_d = max(row[(k + d) & (N - 1)] - med, +0) for d = -B .. B ascending (a NaN difference counts +0); two
 *     chains from +0 in that order, sum w_d and sum (float)d * w_d (the product rounded, then the add); delta their quotient, or 0 where the sum of weights
 *     is not positive or the quotient is not finite; the word is (int32)(k << (32 - logn)) + (int32)rint(delta * 2^(32 - logn)), wrapping.  delta is NOT
 *     clamped: a peak on the edge of a plateau of the band lies up to B bins from the carrier, and the centroid is what brings the word back.
 *     THE OPEN GUARANTEE.  scan_assign: where band[squelch_bin(word)] < to, the bin-centre word of k serves instead, whose band is not below `to`.  The
 *     unchanged wide_squelch_kernel therefore opens every slot in the block that assigns it.
 *     HELD.  A slot is held iff squelch_step(hold[c], band[squelch_bin(fcw_c)], to, tc, hang, J) has the open bit: exactly what the squelch kernel will
 *     compute from the unchanged word.  A held slot covers the peaks within circular distance X of its bin and is never retuned (no jitter; AFC is out of
 *     scope).
 *     ASSIGN.  The uncovered peaks are ranked by band descending, then bin ascending; the peak of rank r goes to the r-th slot of the source that is not
 *     held, in ascending channel order; the peaks left over are counted in missed[s].  A slot neither held nor assigned keeps its word and the squelch
 *     closes it by its own rule.
 *     IDLE.  A block without a frame (J == 0), and a source whose open level or median is not finite, assign nothing, hold nothing and leave every word.
 * m17cxx/detail/core.h has scan_peak, scan_beats, scan_distance, scan_fcw, scan_assign, scan_idle and scan_source (a source's block, the host form): one
 * text for host and device.  On the device wide_scan_kernel (csrc/m17_scan_kernel.hpp; a workgroup of 256 per source; row and bands in LDS, the peaks and the
 * slots compacted in ascending order by ballots and prefix counts, a rank by counting) writes the block's COMPLETE table [source | fcw] into a plane of the
 * scan's own: the entries of the channels that are no slots, and every source, are the host's; only a slot's word is the device's.  That block's squelch
 * kernel and tuner read this plane in place of the host's table; none of them is changed.
 * With the scan on m17hip_wide_channels keeps working for every channel, except that a call which would change a slot's SOURCE returns M17HIP_ESTATE with
 * nothing changed.  A slot's fcw entry is its SEED: it is read where the scan's feed starts over — the first block after this call, after either squelch
 * call or the floor call that leaves the scan on, after m17hip_demod_reset — and ignored otherwise.  This call starts the hold counts and the floor over as
 * either squelch call does, holds for the blocks uploaded after it and never waits for anything in flight.  pool == NULL with n == 0 turns the scan off (the
 * host's table serves again, the slots' seeds included); so does everything that turns off one of the three things it needs: every m17hip_wide_squelch and
 * _squelch_slots call, m17hip_wide_squelch_floor with both ratios 0, m17hip_wide_spectrum, a configuration.  With the scan off a block queues exactly what
 * it queued before.  m17hip_demod_reset_channels and m17hip_set_channel_polarity behave as they do.
 * THE RESET RULE.  A freshly assigned slot starts a new transmission on a demodulator that has been fed zeros — the false-lock case recorded under ABI 620.
 * The caller reads bit 1 of the flags from m17hip_wide_scan_fetch and lists those channels in m17hip_demod_reset_channels before the block's
 * m17hip_demod_run; by stream order the fetch waits for about a spectrum's worth of work, not for the tuner (when it returns in practice: NOTES.md).  (The listed reset also zeroes those channels' hold counts: the
 * next block holds them on their band alone.)  The Python layer (Context.run), M17Demodulator<float> and the example do this by themselves.
 * M17HIP_EINVAL, nothing changed: a NULL context; pool NULL with n != 0 or the reverse; n above the context's channels; guard_bins outside 3 .. points / 4.
 * M17HIP_ESTATE, nothing changed: no wideband configuration; a raster; between m17hip_demod_front and its run; turning it on without the spectrum (or with
 * more than 4096 points), without the block squelch (the slot mode is none) or without the floor.  m17hip_timing_get index 20 is the kernel, one entry per
 * scanned block; m17hip_iq_bytes counts the pool marks, the carry and the planes.
 * OUT OF SCOPE: the scan under the slot squelch or the raster; a reset list made on the device, so that the run needs no fetch; AFC of held slots from the
 * meter; bins to ignore — a dongle's DC spike is a carrier to the scan, which spends a slot on it; slots that move between sources; compacting the tuner's
 * grid to open channels. */
int m17hip_wide_scan(m17hip_ctx* ctx, const uint8_t* pool, uint32_t n, uint32_t guard_bins);
/* The scan of the latest block uploaded with it on (back = 0) or of the one before it (back = 1): fcw_host[C] the table the block was tuned with (every
 * channel's word, slot or not), flags_host[C] bit 0 = is a slot, bit 1 = assigned in this block, bit 2 = held over, missed_host[S] the peaks that found no
 * free slot (room for 256 serves every configuration); *channels = C, *sources = S, *frames = J (each may be NULL).  It waits for that block's scan kernel
 * only — not for its squelch kernel, its tuner, a run or a later block — and copies on the squelch's fetch stream.  cap_channels < C: the first
 * cap_channels entries and all of missed are written and M17HIP_ETRUNC returned, *channels = C.  M17HIP_ESTATE if no such block exists: the scan is off,
 * not enough blocks since it was turned on, or none since m17hip_demod_reset.  M17HIP_EINVAL for back > 1, a NULL context or a NULL array; nothing is
 * written then. */
int m17hip_wide_scan_fetch(m17hip_ctx* ctx, uint32_t back, int32_t* fcw_host, uint32_t* flags_host, uint32_t* missed_host, uint64_t cap_channels,
                           uint32_t* channels, uint32_t* sources, uint32_t* frames);

/* ---- the wideband signal generator: FM-multiplex basebands on the device (ABI 617) -----------------------------
 * Everything above is the receive side.  The project owns the transmit side up to baseband (m17hip_synth_tx_i16); what the reference's users attach behind
 * it, an FM exciter — as rtl_fm is attached in front of the receiver —, is this family: every int16 baseband of a context's input slab (uploaded, or made
 * by m17hip_synth_i16 / _tx_i16 / _sweep_i16: what m17hip_download_i16 would return) is FM-modulated and put at an offset into one of a few wide IQ streams,
 * at the rates the receive side accepts, in memory the CALLER supplies.  A TX context makes the multiplex; an RX context takes it through
 * m17hip_upload_wide_device.  The TX context's stream stays an int16 stream; no existing kernel, launch, stream rule or format rule changes.
 * THE DEFINITION (ring arithmetic in uint64 and uint32, wrapping):
 *     RATE AND BLOCK: a source runs at 48000 P / Q samples per second, P in 1..2000, Q in 1..32, gcd(P, Q) = 1, P >= Q — under m17hip_wide_config P = decim,
 *     under m17hip_wide_config2 P = decim1 decim2, under m17hip_wide_resample P = decim1 down and Q = up.  A block of `samples` baseband samples (a multiple
 *     of Q) gives W = samples / Q * P wideband samples per source.
 *     INDICES: c0 = the feed's 64-bit sample count at the block's start (a multiple of P; it begins at the configuration's first_sample); block sample m has
 *     the absolute index M = c0 + m; k = (m Q) div P and r = (m Q) mod P in 64 bits; b[k] = sample k of the channel's baseband row, b[-1] = the last
 *     baseband sample of the block before, 0 at the feed's start.
 *     PHASE: the exact integral of the baseband interpolated linearly between b[k-1] and b[k] — the baseband is delayed by one sample, so no block needs
 *     its successor:
 *         A2[k] = A2_carry + sum_{i<k} (b[i-1] + b[i]),   E(m) = A2[k] P^2 + 2 b[k-1] r P + (b[k] - b[k-1]) r^2,   theta(m) = K E(m) mod 2^64.
 *     K is the configuration's deviation word: 2^64 turns per unit of E, times the deviation per int16 unit and baseband sample, divided by 2 P^2
 *     (m17hip_synth_wide_k).  Every operation is an integer ring operation: any summation order, scan or tiling gives the same theta, and nothing per
 *     wideband sample is carried.
 *     CARRIER AND SUM: p = (uint32)(theta(m) >> 32) + fcw_c (uint32)M + phase0_c; (cos, sin) = core::nco(p); a channel's term is (amplitude_c cos,
 *     amplitude_c sin), two plain multiplies; x_s[m] = the chain of plain float adds from +0 over the channels of source s among the call's `channels`, in
 *     ascending channel index (a term of amplitude 0 is a zero of either sign and leaves the chain's words as they are); a source nobody transmits on is
 *     +0.  fcw means what m17hip_wide_channels means by it at the same rate, and the count enters as in core::ddc_mix: a receiver fed from count 0 sees a
 *     constant carrier phase.
 *     NOISE, with sigma > 0: re += (float)(unit_noise(ns_s, 2 M) * (double)sigma), im += the same with 2 M + 1; unit_noise = core::mod_unit_noise, the
 *     modulator's, M from all 64 bits; ns_s = mod_splitmix64(seed ^ mod_splitmix64(s * 0x9E3779B97F4A7C15 + 0x57494445)) (core::wtx_noise_stream).
 *     OUTPUT: M17HIP_IQ_F32 the floats as they are; M17HIP_IQ_I16 rintf, clamped to [-32768, 32767]; M17HIP_IQ_U8 rintf(fmaf(v, 1/128, 127.5)), clamped to
 *     [0, 255]; interleaved I,Q, the row pitch in complex samples — exactly what m17hip_upload_wide* reads.
 *     CARRIES: per channel A2 (uint64) and the last baseband sample; the context keeps one sample count.  m17hip_synth_wide_config starts count and
 *     carries over, and so does m17hip_demod_reset on the TX context (the count at the configuration's first_sample again).
 * m17cxx/detail/core.h has wtx_index, wtx_step, wtx_within, wtx_theta, wtx_phase, wtx_add, wtx_noise, wtx_i16 and wtx_u8, so a host computes the device's
 * words.  Two kernels on the context's main stream (csrc/m17_wide_tx_kernels.hpp): wide_tx_prefix_kernel writes K P^2 A2[k] per baseband sample to a scratch
 * plane and advances the carries, wide_tx_mux_kernel makes the streams.  The SCRATCH is 8 bytes per baseband sample of the block, channels * samples * 8
 * bytes (1.5 GB at 4096 channels of one second): allocated with the first call and grown on demand, M17HIP_ENOMEM where it cannot be had — like the
 * spectrum's scratch above, it is as large as that says.  The host form keeps the block's output on the device as well (sources * W samples).
 * m17hip_timing_get index 15 is the generator (both kernels, one entry per block); m17hip_iq_bytes counts its tables, carries and scratch.
 * Out of scope, for a later pull request: pre-emphasis, interpolation better than linear, per-channel deviation, an async device form, more than one
 * rate per context. */
typedef struct m17_wide_tx { uint32_t source; int32_t fcw; uint32_t phase0; float amplitude; } m17_wide_tx; /* 16 bytes */
/* The deviation word K = 2^63 hz_per_unit / (48000 p^2) for a deviation of hz_per_unit Hz per int16 unit of the baseband; hz_per_unit 0 selects M17's,
 * 2400 / (3 * 7168) (the outer symbols +-3 x 7168 deviate +-2400 Hz).  Computed in integers and rounded half up: a nonzero hz_per_unit is taken as the
 * exact binary fraction the double holds, the default as the quotient of integers it is.  No context is needed.  M17HIP_EINVAL for p outside 1..2000, a
 * NULL k, a negative or non-finite hz_per_unit, or a K that would be 0 or 2^63 and more (half a turn per unit of E); nothing is written then. */
int m17hip_synth_wide_k(double hz_per_unit, uint32_t p, uint64_t* k);
/* Configures the generator: sources 1..256 at 48000 p / q (p 1..2000, q 1..32, coprime, p >= q), output of iq_format (M17HIP_IQ_I16, _F32 or _U8), the
 * deviation word k, noise of noise_sigma (finite, >= 0; 0: none) from `seed`, the feed's count beginning at first_sample (a multiple of p).  The table
 * is fresh afterwards (every amplitude 0), the carries zero.  It never waits.  M17HIP_EINVAL outside the limits, with nothing changed; M17HIP_ESTATE
 * between m17hip_demod_front and its run. */
int m17hip_synth_wide_config(m17hip_ctx* ctx, uint32_t sources, uint32_t p, uint32_t q, int iq_format, uint64_t k, float noise_sigma, uint64_t seed,
                             uint64_t first_sample);
/* Channel c < n transmits on tx[c].source at the frequency word tx[c].fcw with the start phase tx[c].phase0 and the amplitude tx[c].amplitude (in output
 * units: int16 units for M17HIP_IQ_I16 and _U8, which scales by 1/128); entries >= n keep theirs.  It holds from the next m17hip_synth_wide call and
 * never waits: the table takes turns in two device copies.  M17HIP_EINVAL for n above the context's channels, a NULL tx, a source at or above
 * `sources`, an amplitude that is negative or not finite — nothing is changed then; M17HIP_ESTATE before the configuration and between
 * m17hip_demod_front and its run. */
int m17hip_synth_wide_channels(m17hip_ctx* ctx, const m17_wide_tx* tx, uint32_t n);
/* One block: the `channels` x `samples` int16 input the slab holds becomes dst[sources][pitch] complex samples of the configured format, W = samples / q * p
 * of them written per row; dst is host memory (m17hip_synth_wide) or device memory (m17hip_synth_wide_device).  Both are complete when they return — the
 * completeness m17hip_upload_wide_device asks of its producer.  M17HIP_EINVAL for a NULL pointer, channels or samples of 0 or above the context's,
 * samples not a multiple of q, W above 2^32 - 1, pitch < W; M17HIP_ESTATE before the configuration, on a float stream, where the slab holds no int16
 * input of channels x samples, and between m17hip_demod_front and its run; M17HIP_ENOMEM if the scratch cannot be had.  Nothing is written and no
 * carry moves on a refusal. */
int m17hip_synth_wide(m17hip_ctx* ctx, void* dst_host, uint32_t channels, uint32_t samples, size_t pitch);
int m17hip_synth_wide_device(m17hip_ctx* ctx, void* dst_dev, uint32_t channels, uint32_t samples, size_t pitch);

/* ---- wideband IQ input at rational sample rates: a resampling tuner (ABI 615) -------------------------------
 * Every configuration above wants a source at an INTEGER multiple of 48 kSPS, and the rates receivers run at by default are not: rtl_sdr's 2.048 MSPS is
 * 128/3 of it (1.024: 64/3, 2.56: 160/3), an Airspy's 2.5, 3, 6 and 10 MSPS 625/12, 125/2, 125 and 625/3, a HackRF's 8 and 20 MSPS 500/3 and 1250/3.  This
 * is the two-stage tuner with a second stage that resamples by up / down: the source runs at 48000 * decim1 * down / up, decim1 1..16, up 1..32, down
 * 1..125, up <= down and gcd(up, down) == 1.  With U = up, D = down, R1 = decim1, per channel, one kernel (csrc/m17_resample_kernels.hpp):
 *     mixed[m] = x[m] * conj(nco(fcw * m))                             (as above; mixed[m] = 0 for m < 0)
 *     u[p]     = sum_{i < ntaps1} taps1[i] * mixed[p R1 + R1 - 1 - i]  (the two-stage tuner's first stage, unchanged)
 *     N_n      = n D + D - 1,   i0_n = N_n mod U,   b_n = N_n div U    (in 64 bits)
 *     z[n]     = sum_{j : i0_n + U j < ntaps2} taps2[i0_n + U j] * u[b_n - j]
 *     y[n]     = gain * arg(z[n] * conj(z[n-1]))
 * — the u zero-stuffed by U, filtered with taps2 at 48000 * D, the sample at n D + D - 1 kept, with the products of the stuffed zeroes left out — in the
 * arithmetic of ABI 609 (ddc_mix per input sample, ddc_tap chains from +0 with j ascending, fm_discriminate; core::ddc_resample is the host form of these
 * words).  At U = 1 it is m17hip_wide_config2's definition, and the words are that tuner's.  n is counted WITHIN A BLOCK: every block holds a multiple of U
 * outputs, so the phase i0 never depends on the feed's history.  The frequency word means fcw / 2^32 * 48000 * decim1 * down / up Hz.
 * Out of scope: a rational-rate channeliser (a raster in a 2.048 MSPS source), sources of different rates in one context, interpolation (up > down), more
 * than two stages, squelching the demodulator.  (Which offsets carry anything: the source spectrum, ABI 616, below; a channel's own level, offset and deviation: the
 * channel meter, ABI 618, above.) */
/* The default taps of both stages.  Stage 1: 8 * decim1 + 1 taps of the Blackman-windowed sinc of m17hip_wide_default_taps2 with its cutoff at half the
 * rate the stage leaves (0.5 / decim1 of the source's rate); one tap of 1 at decim1 == 1.  Stage 2: 32 * down + 1 taps of the same formula with the cutoff
 * at 5500 Hz of 48000 * down, scaled in double to DC gain `up` — every one of the `up` branches taps2[r], taps2[r + up], ... then has unit gain within
 * 1e-6 — and rounded; at up == 1 m17hip_wide_raster_default_taps(down) word for word where that exists.  No context is needed.  *ntaps1 and *ntaps2 are set
 * whenever decim1, up and down are valid; M17HIP_EINVAL if they are not (up > down and a common factor included), if ntaps1 or ntaps2 is NULL, or if a taps
 * pointer is NULL or its capacity too small (nothing written). */
int m17hip_wide_resample_default_taps(uint32_t decim1, uint32_t up, uint32_t down, float* taps1, uint32_t cap1, uint32_t* ntaps1, float* taps2, uint32_t cap2,
                                      uint32_t* ntaps2);
/* What a user knows is the rate.  rate_hz / 48000 reduced to N / up; M17HIP_EINVAL if up > 32.  decim1 is the largest divisor of N that is <= 16 with
 * N / decim1 <= 125 and N / decim1 >= 2 * up (the rate between the stages at or above 96 kSPS); failing that the largest with N / decim1 >= up; failing
 * that M17HIP_EINVAL.  down = N / decim1.  2 048 000 -> 16, 3, 8;  2 400 000 -> 10, 1, 5;  2 500 000 -> 5, 12, 125;  3 000 000 -> 5, 2, 25;
 * 6 000 000 -> 5, 1, 25;  10 000 000 -> 5, 3, 125;  250 000 -> 1, 24, 125;  48 000 -> 1, 1, 1.  No context is needed; nothing is written by a refused call. */
int m17hip_wide_resample_ratio(uint32_t rate_hz, uint32_t* decim1, uint32_t* up, uint32_t* down);
/* m17hip_wide_config2 with a resampling second stage: `sources` (1..256) at 48000 * decim1 * down / up, taps1[ntaps1] (1..256) and taps2[ntaps2] (1..4096),
 * all finite; a NULL pointer with a count of 0 selects that stage's default taps.  M17HIP_EINVAL outside the limits, for up > down and for a common factor of
 * the two.  In every other respect it is m17hip_wide_config2: it starts the feeds over, may be called again, waits for tuner launches in flight and never
 * for a run, clears channels of sources that are gone, leaves the carries, returns M17HIP_ESTATE between m17hip_demod_front and its run, and turns the
 * survey off.  The four configurations replace one another: whichever call was made last decides which kernel the next upload launches.
 * m17hip_wide_channels serves it (it is a tuner: m17hip_wide_raster_channels and m17hip_wide_survey return M17HIP_ESTATE under it).
 * m17hip_upload_wide*, all four ways in: `samples` must be a multiple of `up`, else M17HIP_EINVAL; every source row holds samples / up * down * decim1
 * complex samples and pitch is at least that; a row of more than 2^32 - 1 complex samples is M17HIP_EINVAL on the arguments alone.
 * THE FEED is the one described above.  Per source the last (ceil(ntaps2 / up) - 1) * decim1 + ntaps1 - 1 converted samples are carried; per channel the
 * float2 carry (the last z); ONE running sample count; resets, retunes and the staged-block rule read as under the tuners.
 * m17hip_timing_get index 13 is this tuner; m17hip_iq_bytes counts its memory by the two-stage tuner's rule with that history. */
int m17hip_wide_resample(m17hip_ctx* ctx, uint32_t sources, uint32_t decim1, const float* taps1, uint32_t ntaps1, uint32_t up, uint32_t down, const float* taps2,
                         uint32_t ntaps2, int iq_format);

/* ---- per-operator batched entry points (config 2 parity) ---------------------------------------- */
/* K1: sample scaling + BaseFirFilter<float,150> with the RRC taps, ungated, over the uploaded slab
 * (apps/m17-demod.cpp:489 scaling; FirFilter.h:28-43; taps M17Demodulator.h:79-118).
 * out_host may be NULL (result stays on the device for the next operator). out: [C][T] float. */
int m17hip_fir_rrc150(m17hip_ctx* ctx, uint32_t channels, uint32_t samples, uint32_t flags, float* out_host);
/* K2: Correlator::sample (limit_ = IIR LPF of |y|) and Correlator::correlate against the four M17 sync words
 * (preamble, LSF, packet, EOT — M17Demodulator.h:154-157) for every sample of the FIR output left on the
 * device by m17hip_fir_rrc150 (Correlator.h:43-64, IirFilter.h:26-42).  limit: [C][T]; corr: [4][C][T]. */
int m17hip_correlator(m17hip_ctx* ctx, uint32_t channels, uint32_t samples, float* limit_host, float* corr_host);
/* K1 + K2 in one call (BASELINE configs[1]: "FIR + Correlator only"): the matched filter, the limit filter and the four correlations over
 * the uploaded slab, pipelined in time — the limit filter is one dependent chain per channel over the whole run and is what the call
 * lasts; the matched filter of the next piece and the correlations of this one run beside it.  Results are identical to
 * m17hip_fir_rrc150 followed by m17hip_correlator (FirFilter.h:28-43, Correlator.h:38-64, IirFilter.h:26-42).
 * y: [C][T], limit: [C][T], corr: [4][C][T]; any of the host pointers may be NULL (the result stays on the device). */
int m17hip_fir_correlator(m17hip_ctx* ctx, uint32_t channels, uint32_t samples, uint32_t flags, float* y_host, float* limit_host, float* corr_host);
/* K3: NSlidingDFT<float,48000,120,2> + DataCarrierDetect accumulation (SlidingDFT.h:118-132,
 * DataCarrierDetect.h:53-58) over the uploaded slab.  For every 192-sample tick k the table holds the
 * sequential sums of norm(X0) (bin 0) and norm(X1) (bin 1) for segments that started 1..5 ticks ago (index a%5,
 * a = start tick) and since the stream start (index 5): sums[C][ticks][2][6]. */
int m17hip_dcd(m17hip_ctx* ctx, uint32_t channels, uint32_t samples, uint32_t flags, float* sums_host, uint32_t* ticks_out);
/* K4: Viterbi<Trellis<4,2>,4>::decode (Viterbi.h:162-239) on n depunctured soft-bit frames.
 * kind: 0 = LSF 488->240, 1 = stream 296->144, 2 = packet 420->206, 3 = BERT 402->197.
 * soft: [n][IN] int8 (0 = erasure); bits: [n][OUT] uint8; cost: [n]. */
int m17hip_viterbi(m17hip_ctx* ctx, const int8_t* soft_host, uint32_t n_frames, int kind, uint8_t* bits_host, int32_t* cost_host);
/* a11/a12: llr<float,4> (Util.h:63-104,128-145) and SymbolEvm::update (SymbolEvm.h:31-51, after reset()) on `rows`
 * independent sequences of n normalised symbols.  llr: [rows][n][2] int8; evm: [rows][n] running evm(). */
int m17hip_slice_llr(m17hip_ctx* ctx, const float* sym_host, uint32_t rows, uint32_t n, int8_t* llr_host, float* evm_host);
/* K4': M17FrameDecoder::operator() (M17FrameDecoder.h:353-392: derandomize, deinterleave, depuncture,
 * Viterbi / Golay, CRC, frame-type state machine) on n independent 368-LLR frames, each with its own decoder
 * state in/out.  sync_type[n]; state_io[n] (State enum), lich_io[n], lsf_io[n][30], dep401_io[n], cost_io[n];
 * recs: [n][2] records, nrec[n] callbacks per frame. */
int m17hip_decode_frames(m17hip_ctx* ctx, const int8_t* llr368_host, uint32_t n_frames, const uint8_t* sync_type,
                         uint8_t* state_io, uint8_t* lich_io, uint8_t* lsf_io, int8_t* dep401_io, int64_t* cost_io,
                         m17_frame_rec* recs, uint8_t* nrec);
/* TEST HOOK (ABI 612; no product path calls it): M17FrameDecoder::operator() over `channels` independent sequences of `frames` 368-LLR frames
 * each, in the form of the decoder the caller names — the forms the full chain runs are otherwise reached through m17hip_demod_run alone, on
 * whatever LLRs a signal produces.
 *   form 0  one lane per channel, the lane-per-frame decoder with 32-bit metrics (the arithmetic of m17hip_decode_frames, frame after frame);
 *   form 1  one wave per channel, the wave decoder (sixteen lanes = sixteen states), every frame decoded where it completes: what the
 *           sequential kernel runs under m17hip_tune key 15 = 0, and for every LSF, LICH and packet frame under any setting;
 *   form 2  one wave per channel with a deferred-frame store: stream and BERT payload frames are left in the store, then the kernel that
 *           settles the end of a run and the deferred decode (one lane per frame, packed 16-bit metrics) run as m17hip_demod_run queues them.
 * llr368[channels][frames][368], sync_type[channels][frames] (0 LSF, 1 stream, 2 packet, 3 BERT); per channel in and out, as
 * m17hip_decode_frames: state_io (State enum, 0..4), lich_io, lsf_io[30], dep401_io, cost_io (-1 = size_t(-1)).  Out: recs[channels][rec_cap]
 * (slots beyond a channel's callbacks stay zero; `channel` = the sequence, `seq` = the callback's index, `sample_pos` = the frame's index),
 * nrec[channels] (callbacks, those that found the store full included), *overflow_out (1 if any did), cost_trace[channels][frames]: the
 * viterbi_cost as it stands after each frame, -1 for size_t(-1).  The three forms give the same results.
 * M17HIP_EINVAL — before anything is launched — for a NULL pointer, another form, channels, frames or rec_cap of 0, an LLR or a dep401
 * outside [-7, 7] (the slicer produces nothing else and the store's nibbles hold nothing else), a state above 4, a sync type above 3, a
 * cost below -1 or above INT32_MAX.  The context's runs, records and demodulator state are not touched. */
int m17hip_decode_sequences(m17hip_ctx* ctx, int form, const int8_t* llr368_host, const uint8_t* sync_type, uint32_t channels, uint32_t frames,
                            uint32_t rec_cap, uint8_t* state_io, uint8_t* lich_io, uint8_t* lsf_io, int8_t* dep401_io, int64_t* cost_io,
                            m17_frame_rec* recs, uint32_t* nrec, uint32_t* overflow_out, int32_t* cost_trace);

/* TEST HOOK (ABI 614; no product path calls it): other taps for the matched filter.  The 149 non-zero taps of BaseFirFilter<float,150> are not
 * compiled into any kernel: every form of the matched filter — K1 rolled and skewed, int16 and float32 input, uniform and per-channel polarity,
 * K2's patch window and the sequential kernel's own filter at a gate reopening — reads them from two host-built tables of the context.  The
 * call waits for everything the context has queued, then rewrites both from taps149[0..148] (taps149[i] multiplies the sample i steps back,
 * FirFilter.h:36-40); tap 150 stays the zero it is.  taps149 == NULL restores the RRC taps (M17Demodulator.h:79-118).  The taps stay in force
 * until the next call or m17hip_ctx_destroy — across m17hip_demod_reset and m17hip_demod_reset_channels — for the operator entry points above
 * and the full chain alike.  What it is for: the RRC taps are symmetric, so a mirrored tap index computes the same words; asymmetric taps make
 * it a value error.  And with the identity (taps149[0] = 1, the rest 0) on a float32 stream the matched filter's output IS the input, so a test
 * writes what the correlator, the sync search, the level estimator and the slicer see, sample by sample.
 * M17HIP_EINVAL for a NULL context or a tap that is not finite; M17HIP_ESTATE between m17hip_demod_front and its m17hip_demod_run (the run's
 * matched filter is queued with the tables as they are); nothing is changed then. */
int m17hip_set_fir_taps(m17hip_ctx* ctx, const float* taps149);

/* ---- the full chain ------------------------------------------------------------------------------- */
/* Fresh demodulators for every channel (M17Demodulator ctor + zero-initialised storage). */
int m17hip_demod_reset(m17hip_ctx* ctx);
/* Fresh demodulators for the listed channels only (M17Demodulator ctor, M17Demodulator.h:180-182, + zero-initialised storage, as
 * m17hip_demod_reset): what the reference does by starting a new m17-demod process for ONE stream — a receiver was retuned, a source
 * came back, a channel slot goes to another stream — while every other channel of the context keeps its sync, its clock and level
 * filters and its half-assembled LICH / packets.
 * channels[n]: LOCAL indices < max_channels (not offset by m17hip_set_channel_base); duplicates are allowed; n == 0 is a successful
 * no-op.  M17HIP_EINVAL for an index out of range or a NULL list with n > 0 — then nothing is marked.
 * The call MARKS the channels.  The resets take effect at the start of the NEXT run queued — by m17hip_demod_run, or by the
 * m17hip_demod_front that begins it — after the previous run's tails have been carried into that run's slab prefixes: from sample 0 of
 * that run each marked channel behaves as a reference process started there.  Several calls before one run add up;
 * m17hip_demod_reset clears the marks; so does the run that takes them, once its front end is queued — a m17hip_demod_front / m17hip_demod_run that
 * fails before that (bad arguments, M17HIP_ESTATE) leaves them pending, one that fails later with M17HIP_EHIP has dropped them.  Between m17hip_demod_front and its m17hip_demod_run: M17HIP_ESTATE, like the other
 * state-changing calls.  Before the first run after m17hip_demod_reset the call succeeds and changes nothing observable.
 * Everything the run BEFORE the resets produced stays intact for every channel, the reset ones included: its records in both fetch
 * orders of a live feed (m17hip_frames_select(ctx, 1) after the next run was queued), its deferred payload frames, its packets and
 * BERT statistics; its last EVM fold and its m17_diag when they are fetched before the next run is queued (m17hip_demod_run: the
 * front end m17hip_demod_front queues leaves them alone).
 * For a reset channel m17_frame_rec.seq and .sample_pos, m17_diag.n_frames / n_diag and the diagnostic log's sample index count
 * from the channel's own reset, not the context's; its BERT statistics (key 6) and its packet reassembly (key 7) start over — a
 * half-assembled packet is abandoned, m17_packet_rec.seq restarts.
 * LIMIT of this version: the carrier-detect tick grid (192 samples) belongs to the context — the carrier-detect table, the
 * limit-filter replay, the sequential kernel and the gate forecast all find a tick as position / 192 — and a fresh demodulator's
 * carrier-detect updates fall on the tick ends of ITS stream.  A reset can therefore only take effect where the context's sample
 * position (the samples run since m17hip_demod_reset) is a multiple of 192: otherwise M17HIP_ESTATE, and nothing is marked.
 * Cost: list-driven kernels over the marked channels only, O(n); a run with no mark pending queues exactly what it did before.
 * Complex IQ input (m17hip_upload_iq*): the listed channels' IQ feeds start over as well — AT ONCE, not with the next run: the reset applies to the IQ
 * blocks uploaded after this call (their first discriminated sample is +0), not to a block that is already staged. */
int m17hip_demod_reset_channels(m17hip_ctx* ctx, const uint32_t* channels, uint32_t n);
/* Per-channel input polarity (ABI 604): the reference's -i (apps/m17-demod.cpp:488, sample *= -1 in int16) is a property of ONE receiver — its
 * discriminator, its sound card, the side of the IF — and each reference process has its own command line.  invert[n], n in 1..max_channels:
 * entry c is 0 or 1 for LOCAL channel c (not offset by m17hip_set_channel_base); entries >= n keep their value; invert == NULL with n == 0 clears
 * the whole table.  M17HIP_EINVAL for a NULL context, n > max_channels, NULL with n > 0, non-NULL with n == 0, or an entry other than 0 / 1 —
 * then nothing changes.
 * The EFFECTIVE polarity of channel c in a call is table[c] XOR (flags & M17HIP_FLAG_INVERT): in m17hip_demod_run / m17hip_demod_front and in
 * the per-operator entries that take flags (m17hip_fir_rrc150, m17hip_dcd, m17hip_fir_correlator).
 * The table belongs to the context and describes the receivers, not the streams: m17hip_demod_reset keeps it; a fresh context has all zeros.
 * A channel that has RUN since m17hip_demod_reset carries state formed under its old polarity (the raw input prefix, the carrier detect's
 * sliding DFT, the demodulator), and no reference process corresponds to its continuation: changing its entry marks it exactly as
 * m17hip_demod_reset_channels does — from the next run queued it is a fresh demodulator under the new polarity, with everything that call
 * says about records, positions and consumers — and under that call's rule: if the context's position is not a multiple of 192 samples and
 * at least one CHANGED channel has run, M17HIP_ESTATE, and nothing changes, neither table nor marks.  Entries written with the value they
 * have mark nothing; before the first run after m17hip_demod_reset any change is free.
 * Between m17hip_demod_front and its m17hip_demod_run: M17HIP_ESTATE, like the other state-changing calls.  The call waits for no run in
 * flight and alters none: a run keeps the table it was queued with.
 * Cost: launches whose channels are of one effective polarity (no table, all 0, all 1) are those of a context without a table; mixed ones
 * take the per-channel forms of the matched filter and the carrier detect (NOTES.md has their instruction counts).  The call itself never
 * waits; the wait it saves is paid, if at all, where a mixed run is queued: two device tables take turns, and before one is written again the
 * host waits for the runs that read it, so m17hip_demod_run / m17hip_demod_front queued after a change may wait for the run before last
 * (as a marked run does for the reset lists). */
int m17hip_set_channel_polarity(m17hip_ctx* ctx, const uint8_t* invert, uint32_t n);
/* M17Demodulator<float>::operator() (M17Demodulator.h:657-753) for `samples` new samples of each channel of
 * the uploaded slab; frame callbacks become records, the last diagnostic callback becomes m17_diag. */
int m17hip_demod_run(m17hip_ctx* ctx, uint32_t channels, uint32_t samples, uint32_t flags);
/* Streaming: pipelining of consecutive runs of the SAME channels.  apps/m17-demod.cpp:484-490 is one endless
 * stream per channel; here the stream arrives in runs, and most of a run's arithmetic does not depend on how the run before it
 * ended: the matched filter (FirFilter.h:28-43) needs only the carried 152-sample input tail, the sliding DFT
 * (SlidingDFT.h:118-132) only its own end state.  With the next run's input STAGED (m17hip_upload_i16_async,
 * m17hip_upload_i16_device_async or m17hip_input_alternate), m17hip_demod_front swaps the context's two sets of per-run slabs
 * and queues that front end at once, on the context's side streams — while the state-machine half of the latest run (limit
 * filter, clock recovery, slicer, Viterbi: everything that waits for M17Demodulator's state) is still at work.  The call
 * sequence of a live feed:
 *     stage(k + 1); m17hip_demod_front(k + 1); m17hip_demod_run(k + 1);
 *     m17hip_frames_select(ctx, 1); m17hip_frames_fetch / _compact_device / m17hip_gather_frames (run k);  ...
 * i.e. the state-machine half of run k + 1 is queued BEFORE the host collects run k's records: nothing of run k + 1 waits for what only
 * run k's consumers need.  A run ends, on the context's main stream, with its demodulator state settled (M17Demodulator.h:146-176:
 * everything operator() reads the next time); the payload frames whose Viterbi decode K5 deferred, the payload consumers (BERT
 * statistics, packet reassembly), the compaction of the records and the gather work on the context's PAYLOAD stream, beside the next
 * run, on the record set of their own run — two record sets alternate run by run, so a run's records stay fetchable until the run
 * after the next is queued.  (The older order — fetch run k between m17hip_demod_front(k + 1) and m17hip_demod_run(k + 1) — works as
 * before; the next run's chain then starts a host round trip and the deferred decode, 2 ms per 4096 x 480 000, later.)
 * The m17hip_demod_run that follows m17hip_demod_front must name the same channels / samples / flags (M17HIP_ESTATE otherwise) and
 * queues the rest.  Between the two calls the context's results are still those of run k; in-place uploads, per-operator entry points and
 * m17hip_tune return M17HIP_ESTATE; m17hip_demod_reset abandons the queued front end.  Results are bit-identical to the same runs
 * made one after the other (tests/test_gpu_streaming.py).  M17HIP_ESTATE if nothing is staged.
 * (m17hip_demod_run on staged input without this call queues the same front end itself — then nothing is gained unless the host
 * calls it before it has fetched the previous run's records, which it thereby gives up.) */
int m17hip_demod_front(m17hip_ctx* ctx, uint32_t channels, uint32_t samples, uint32_t flags);
/* Which run's records m17hip_frames_count / _fetch / _compact_device and m17hip_gather_frames[_device] name: back = 0 the latest run
 * (the default; every m17hip_demod_run selects it again), back = 1 the run before it — what a live feed asks for after it has queued
 * the next run (above).  M17HIP_ESTATE if that run's records are not there (no such run since the last reset). */
int m17hip_frames_select(m17hip_ctx* ctx, uint32_t back);
/* Number of records produced by the selected run (all channels).  The calls of this family wait for the run's payload work only —
 * not for anything queued after it. */
int m17hip_frames_count(m17hip_ctx* ctx, uint64_t* total);
/* Records of the last run, ordered by (channel, seq).  Host destination.  *count = records the run produced; when that is
 * more than `capacity` only `capacity` are written and M17HIP_ETRUNC is returned. */
int m17hip_frames_fetch(m17hip_ctx* ctx, m17_frame_rec* recs_host, uint64_t capacity, uint64_t* count);
/* Same, compacted into caller-provided DEVICE memory (so a collective can ship it without a host hop); same
 * truncation rule.  The copy is made on the context's payload stream and is complete when the call returns.  For the latest run it is
 * ordered behind whatever the caller has queued on the context's main stream so far (a fill of the destination, say); with a newer run
 * queued (m17hip_frames_select(ctx, 1)) it waits for nothing but the selected run: the destination must be ready when the call is made.
 * The same holds for the device destination of m17hip_gather_frames_device. */
int m17hip_frames_compact_device(m17hip_ctx* ctx, m17_frame_rec* recs_dev, uint64_t capacity, uint64_t* count);
/* Per-channel diagnostics after the last run: diag_host[C]. */
int m17hip_diag_fetch(m17hip_ctx* ctx, m17_diag* diag_host, uint32_t channels);

/* Every diagnostic callback of the last run, not only the last one: after m17hip_tune(ctx, 9, room) each invocation of the
 * reference's diagnostic callback (every 960 samples while the carrier is on, every 384 while it is off) appends its
 * arguments to the channel's log: log_host[channels][capacity], counts_host[channels] entries valid per row, in stream order.
 * In a log entry demod_state / n_frames are the values at that moment and pad[0] | pad[1] << 32 is the index (since reset) of
 * the sample whose processing fired the callback — frame callbacks of the same sample come first (M17Demodulator.h:729-752).
 * M17HIP_ETRUNC if a channel fired more than min(capacity, room) callbacks. */
int m17hip_diag_log_fetch(m17hip_ctx* ctx, m17_diag* log_host, uint32_t* counts_host, uint32_t channels, uint32_t capacity);

/* Synthetic input on the device: the framing of the reference's modulator CLI (apps/m17-mod.cpp:164-504,
 * 628-677: preamble, LSF, stream / BERT / packet frames, EOT), its pulse shaping (one symbol per 10 samples through the 150-tap
 * RRC in double, x 7168, truncation to int16, :204-224) and the impairments of BASELINE config 5, written straight into the
 * context's input slab: [channels][samples], ready for m17hip_demod_run (no upload).  Channel c of the batch uses
 * seed ^ splitmix64((chan0 + c) * 0x9E3779B97F4A7C15 + 1); kind < 0 = even channels BERT, odd channels voice-like streams.
 * Reproducible bit for bit (integer-hash noise); the parity tests compare every int16 with the test generator. */
typedef struct m17_synth_params {
    uint64_t seed;
    int32_t kind;          /* 0 BERT, 1 voice-like stream, 2 RAW packet, 3 noise only, 4 RAW packet closed by a CRC-16/X.25 FCS (1..33 frames), < 0 mixed */
    int32_t n_frames;      /* payload frames */
    int32_t lead_in;       /* samples of lead-in noise (sigma lead_sigma) before the burst */
    int32_t phase;         /* extra delay 0..9 samples, < 0 = derived from the seed */
    int32_t tail, total;   /* unused here (the slab length is `samples`) */
    int32_t invert;        /* transmit inverted polarity */
    int32_t n_preamble;    /* 0 = as m17-mod does (2 for BERT, else 1) */
    double lead_sigma, noise_sigma, dc_offset, gain, tail_sigma;   /* LSB */
} m17_synth_params;
int m17hip_synth_i16(m17hip_ctx* ctx, const m17_synth_params* params, uint32_t channels, uint32_t samples, uint32_t chan0);
/* An impairment SWEEP in one synthesis (BASELINE config 5, SURVEY §8(d): AWGN, DC offset = FM frequency offset, gain): channel c
 * takes point p = (chan0 + c) % n_points of `points` — interleaved, so that every contiguous shard carries every point.  Row c is,
 * int16 for int16, row c of m17hip_synth_i16(ctx, base', channels, samples, chan0) with base' = *base and its noise_sigma, tail_sigma,
 * dc_offset and gain replaced by points[p]; every other field (kind < 0 mixed, phase, lead_in, invert, n_preamble, lead_sigma) and the
 * per-channel seeding come from `base`, so a shard synthesised with its global chan0 is bitwise the matching rows of the whole set.
 * Tuning knob 16 (staging) applies as to m17hip_synth_i16.  M17HIP_EINVAL for n_points == 0 or above M17HIP_MAX_SWEEP_POINTS, points
 * == NULL, a non-finite or negative sigma, a non-finite dc_offset or gain, and whatever m17hip_synth_i16 refuses. */
typedef struct m17_impairment {   /* one point of a sweep grid */
    double noise_sigma, tail_sigma, dc_offset, gain;   /* LSB, LSB, LSB, x */
} m17_impairment;                 /* 32 bytes */
#define M17HIP_MAX_SWEEP_POINTS 4096u
int m17hip_synth_sweep_i16(m17hip_ctx* ctx, const m17_synth_params* base, const m17_impairment* points, uint32_t n_points,
                           uint32_t channels, uint32_t samples, uint32_t chan0);
/* Caller-supplied transmissions (ABI 605): the same framing (apps/m17-mod.cpp:264-504, 509-564), shaping and impairments as
 * m17hip_synth_i16, with the CONTENT given by the caller — channel c sends transmission tx[c]:
 *   kind 1 (stream)  preamble(s), the LSF, n_frames stream frames, EOT + 40 zero symbols;
 *   kind 2 (packet)  preamble(s), the LSF, n_frames packet frames, EOT + 40 zero symbols;
 *   kind 0 (BERT)    preambles, n_frames BERT frames.
 * lsf30[c] is channel c's 30-byte LSF, sent as given: its CRC is NOT recomputed, so a broken one can be sent.  Payload frame i of
 * channel c is rows[tx[c].first_row + i], 32 bytes laid out as the frame records' payloads are: a stream frame takes bytes 0..17 (frame
 * number, with the caller's end-of-stream bit, and 16 payload bytes) and carries segment i % 6 of the channel's LSF as its LICH; a packet
 * frame takes bytes 0..25 of which 206 bits are carried; a BERT frame takes bytes 0..24 of which 197 bits are carried.  The rest of a row
 * is ignored and nothing outside rows[first_row .. first_row + n_frames) is read.
 * From `base`: seed (noise, the derived phase; per channel with chan0 as for m17hip_synth_i16), lead_in, phase, invert, n_preamble (0 = as
 * m17-mod does for the channel's kind), the sigmas, dc_offset and gain; base->kind and base->n_frames are ignored.  With the content the
 * built-in generator would have chosen, every int16 equals m17hip_synth_i16's.  A burst longer than `samples` is cut off.  Tuning knob 16
 * (staging) applies; M17HIP_ESTATE between m17hip_demod_front and its run; complete when it returns.
 * M17HIP_EINVAL, with nothing written: ctx, base, tx or rows NULL; lsf30 NULL with a kind other than 0; a kind > 2; reserved != 0;
 * first_row + n_frames > n_rows; n_frames > samples / 1920 + 1; and whatever m17hip_synth_i16 refuses for channels / samples. */
typedef struct m17_tx {      /* one transmission = one channel; 16 bytes */
    uint32_t kind;           /* 0 BERT, 1 stream, 2 packet */
    uint32_t n_frames;       /* payload frames */
    uint32_t first_row;      /* index of its first row in `rows` */
    uint32_t reserved;       /* 0 */
} m17_tx;
int m17hip_synth_tx_i16(m17hip_ctx* ctx, const m17_synth_params* base, const m17_tx* tx,
                        const uint8_t* lsf30,   /* [channels][30], NULL allowed when every kind is 0 */
                        const uint8_t* rows,    /* [n_rows][32] */
                        uint32_t n_rows, uint32_t channels, uint32_t samples, uint32_t chan0);
/* Read the input slab back: out[channels][samples] (row pitch in samples).  M17HIP_ESTATE when the slab holds float input (m17hip_download_f32). */
int m17hip_download_i16(m17hip_ctx* ctx, int16_t* host, uint32_t channels, uint32_t samples, size_t pitch);

/* Payload consumer: BERT statistics — decode_bert + PRBS9::validate (apps/m17-demod.cpp:286-304,
 * Util.h:320-441: LFSR x^9 + x^5 + 1, lock after 18 good bits, unlock at 25 errors in the last 128 bits) over the BERT
 * frame records of every run since the last m17hip_demod_reset, per channel.  Enabled with m17hip_tune(ctx, 6, 1) BEFORE the
 * runs to be counted (the records of a run are accounted at its end); M17HIP_ESTATE otherwise. */
typedef struct m17_bert_stat {
    uint32_t bits;    /* PRBS9::bits()   */
    uint32_t errors;  /* PRBS9::errors() */
    uint32_t synced;  /* PRBS9::sync()   */
    uint32_t frames;  /* BERT frames seen */
} m17_bert_stat;
int m17hip_bert_stats(m17hip_ctx* ctx, m17_bert_stat* stats_host, uint32_t channels);

/* One 32-byte word per channel for an impairment sweep (m17hip_synth_sweep_i16): m17hip_bert_stats and the `evm` field of
 * m17hip_diag_fetch in one pass on the device and ONE copy.  Replaces, per channel, PRBS9::bits() / errors() / sync() (Util.h:320-413),
 * the count of BERT frames and SymbolEvm::evm() (SymbolEvm.h:31-51).  Ordered as those two calls are: behind the latest run's last EVM
 * fold and the payload work of every run whose record set is still there (wherever it was queued), whatever the caller has queued
 * since.  M17HIP_ESTATE if BERT statistics are off (m17hip_tune key 6) or no run has been made since the last m17hip_demod_reset;
 * M17HIP_EOVERFLOW when m17hip_diag_fetch would return it — every word is still written, with flag bit 0 cleared. */
typedef struct m17_chan_stat {
    uint32_t channel;   /* channel_base + local index (m17hip_set_channel_base) */
    uint32_t point;     /* channel % n_points */
    uint32_t bits, errors, synced, frames;   /* = m17_bert_stat */
    float    evm;       /* = m17_diag.evm */
    uint32_t flags;     /* bit 0: evm is valid (no deferred-EVM overflow, m17hip_tune key 18); other bits 0 */
} m17_chan_stat;        /* 32 bytes */
int m17hip_sweep_stats(m17hip_ctx* ctx, uint32_t n_points, m17_chan_stat* host, uint32_t channels);

/* Payload consumer: packet reassembly — decode_packet (apps/m17-demod.cpp:207-253) with the per-transmission
 * reset of dump_lsf (:154-155), per channel, over the packet frame records of every run since the last m17hip_demod_reset:
 * an LSF record starts a new packet; numbered frames (payload[25] = frame number << 2) must arrive in sequence, one that does
 * not is dropped and counted; the frame with the EOF bit (payload[25] & 0x80) contributes its first min(count, 25) bytes and
 * closes the packet, whose CRC-16/X.25 over contents + FCS must leave 0x0f47 (boost::crc_optimal<16, 0x1021, 0xFFFF, 0xFFFF,
 * true, true>, :218-222).  dump_lsf's ENCAPSULATED branch reads lsf[109..111] of a 30-byte array (:157-171, out of bounds);
 * that prefix is not reproduced — every packet is assembled as RAW.  Enabled with m17hip_tune(ctx, 7, capacity) BEFORE the
 * runs; m17hip_packets_fetch returns the packets the LAST run completed, ordered by (channel, seq); *count = how many
 * there were (M17HIP_EOVERFLOW if more than the capacity set by m17hip_tune). */
typedef struct m17_packet_rec {
    uint32_t channel;
    uint32_t seq;          /* packets this channel completed before this one, since reset */
    uint64_t sample_pos;   /* of the closing frame's callback */
    uint16_t size;         /* bytes in data, FCS included */
    uint16_t checksum;     /* CRC-16/X.25 of data[0..size): 0x0f47 for an intact packet */
    uint8_t crc_ok;
    uint8_t frames;        /* packet frames accepted, the closing one included */
    uint8_t seq_errors;    /* frames dropped by the sequence check since the LSF */
    uint8_t reserved;
    uint8_t data[840];     /* at most 32 x 25 + 25 bytes are ever used */
} m17_packet_rec; /* 864 bytes */
int m17hip_packets_fetch(m17hip_ctx* ctx, m17_packet_rec* recs_host, uint32_t capacity, uint32_t* count);
/* The same consumer over frame records supplied by the caller (fetched earlier, or gathered from other GPUs) instead of the
 * last run's: recs_host[channels][pitch] with counts_host[c] records used in row c.  The per-channel assembly state advances
 * exactly as it does at the end of a run; the packets completed are then returned by m17hip_packets_fetch. */
int m17hip_packets_feed(m17hip_ctx* ctx, const m17_frame_rec* recs_host, const uint32_t* counts_host, uint32_t channels, uint32_t pitch);

/* Payload consumer (ABI 606): the voice of stream transmissions — FrameType::STREAM -> demodulate_audio
 * (apps/m17-demod.cpp:178-205, 321-323) — without codec2, which stays host work: per channel and run the 16 payload bytes of every
 * stream record (payload[2..17]: two codec2 3200 frames, :198-200) next to each other in arrival order, one MARK byte per slot, and a
 * log of the CALLS the run closed.  Enabled with m17hip_tune(ctx, 34, room) BEFORE the runs to be consumed: room = voice slots per
 * channel and run (a run of T samples carries at most T / 1920 + 1 stream frames per channel).  The consumer is defined on the frame
 * records of a run in (channel, seq) order, with per-channel state carried from run to run:
 *   1. a record with frame_type == M17_FRAME_LSF (an LSF frame, or one assembled from LICH, M17FrameDecoder.h:247-254) closes the
 *      channel's open call, if any (close = 2), and opens a new one: has_lsf = 1, lsf = payload[0..29], start_pos = its sample_pos
 *      (dump_lsf, :316);
 *   2. a record with frame_type == M17_FRAME_STREAM opens a call if none is open (has_lsf = 0, lsf all zero, start_pos = its sample_pos:
 *      a late join, or the frames that follow an end of stream) and takes the channel's next voice slot of the run: the payload is ALWAYS
 *      copied — blanking is the host's decision — with the mark bits
 *          bit 0 (M17HIP_MARK_BLANK)  cost > 80: what -b would silence (:190)
 *          bit 1 (M17HIP_MARK_EOS)    cost < 70 && (payload[0] & 0x80): an accepted end of stream (:184)
 *          bit 2 (M17HIP_MARK_FIRST)  the first voice frame of its call
 *          bit 3 (M17HIP_MARK_GAP)    its frame number ((payload[0] << 8 | payload[1]) & 0x7fff) is not the call's previous frame number
 *                                     + 1 mod 0x8000 (never set together with bit 2: a first frame has no predecessor)
 *      and the call's frames, blanked (bit 0), cost_sum (mod 2^32) and end_pos (= its sample_pos) advance; with bit 3 set `lost` grows by
 *      (frame number - previous frame number - 1) mod 0x8000.  Mark bit 1 closes the call (close = 1);
 *   3. every other record is ignored.
 * m17hip_demod_reset starts every channel over (no open call, seq 0); m17hip_demod_reset_channels, or a polarity change that marks a
 * channel, does so for the marked channels — an open call is abandoned, as a half-assembled packet is.
 * A call is reported ONCE, by the run that closes it.  Room for call records: M17HIP_CALLS_PER_CHANNEL(room) per channel and run (one
 * row per channel in the store, max_channels x that in all — nothing but (channel, seq) ever orders it); a channel that closes more in
 * one run keeps the first ones and m17hip_calls_fetch returns M17HIP_EOVERFLOW.  A channel with more stream records than `room` in one
 * run: the slots that fit are written, the call accounting goes on over every record, m17hip_voice_fetch returns M17HIP_EOVERFLOW. */
#define M17HIP_MARK_BLANK 1u
#define M17HIP_MARK_EOS 2u
#define M17HIP_MARK_FIRST 4u
#define M17HIP_MARK_GAP 8u
#define M17HIP_CALLS_PER_CHANNEL(room) ((room) / 8u + 2u)
typedef struct m17_call_rec {   /* 72 bytes */
    uint32_t channel;           /* channel_base + local index */
    uint32_t seq;               /* calls this channel closed before this one, since reset */
    uint64_t start_pos, end_pos;/* sample_pos of the opening record / of the last voice frame (= start_pos when there was none) */
    uint32_t cost_sum, frames, blanked, lost;
    uint8_t  has_lsf, close;    /* close: 1 accepted EOS, 2 the next LSF record */
    uint8_t  lsf[30];
} m17_call_rec;
/* The planes of the selected run (m17hip_frames_select; ordered as the fetch family is: behind that run's payload work, whatever was
 * queued since): audio_host[channels][slots][16], marks_host[channels][slots], counts_host[channels] = stream records of the channel in
 * that run.  slots < room is allowed: rows are cut (slots beyond the room are not written; slots == 0 fetches the counts alone, the two
 * plane pointers may then be NULL).  M17HIP_EOVERFLOW if a count exceeds room, else M17HIP_ETRUNC if one exceeds `slots` — the rows are
 * written as far as they go either way.  M17HIP_ESTATE with the key off or with no run made (nor m17hip_voice_feed) since the reset;
 * M17HIP_EINVAL for NULL where a pointer is needed, channels == 0 or more channels than the run had.
 * Replaces the loop a host runs over the fetched records: apps/m17-demod.cpp:178-205. */
int m17hip_voice_fetch(m17hip_ctx* ctx, uint8_t* audio_host, uint8_t* marks_host, uint32_t* counts_host, uint32_t channels, uint32_t slots);
/* The same planes where they lie, for a consumer on the GPU (a torch tensor view): DEVICE pointers of the selected run's
 * audio[max_channels][*pitch_slots][16], marks[max_channels][*pitch_slots], counts[max_channels] (*pitch_slots = room).  The call waits
 * for the payload work of that run; the memory is valid until the run after the next is queued (as the record sets are), or key 34 is
 * set again.  Replaces apps/m17-demod.cpp:198-200 (the payload handed to codec2). */
int m17hip_voice_device(m17hip_ctx* ctx, const uint8_t** audio_dev, const uint8_t** marks_dev, const uint32_t** counts_dev, uint32_t* pitch_slots);
/* The calls the selected run closed, ordered by (channel, seq): *count = how many there were, min(*count, capacity) are written
 * (the truncation rule of m17hip_packets_fetch); M17HIP_EOVERFLOW if a channel closed more than M17HIP_CALLS_PER_CHANNEL(room).
 * Replaces what an operator reads off dump_lsf's and demodulate_audio's output (apps/m17-demod.cpp:124-205, 316). */
int m17hip_calls_fetch(m17hip_ctx* ctx, m17_call_rec* host, uint32_t capacity, uint32_t* count);
/* The same consumer over frame records supplied by the caller (fetched earlier, gathered from other GPUs, or made by a test) instead of
 * a run's: recs_host[channels][pitch] with counts_host[c] records used in row c (cut at pitch).  The per-channel state advances exactly
 * as at the end of a run; the results are then what the three calls above return (they take the place of the latest run's).
 * M17HIP_ESTATE with the key off and between m17hip_demod_front and its run.  (apps/m17-demod.cpp:321-323 over a record list.) */
int m17hip_voice_feed(m17hip_ctx* ctx, const m17_frame_rec* recs_host, const uint32_t* counts_host, uint32_t channels, uint32_t pitch);

/* Payload consumer: link setup frames as text — LinkSetupFrame::decode_callsign (LinkSetupFrame.h:95-121: 6 bytes
 * big-endian base 40 -> up to 9 characters, all ones = "BROADCAST"), the 16-bit type field and the CRC check of dump_lsf
 * (apps/m17-demod.cpp:124-200), for a batch of n 30-byte LSFs (e.g. the payloads of the frame_type 0 records). */
typedef struct m17_lsf_info {
    char dst[10], src[10];   /* NUL-padded callsigns */
    uint16_t type;           /* LSF bytes 12..13 */
    uint8_t crc_ok;          /* CRC16 over the 30 bytes == 0 */
    uint8_t reserved[9];
} m17_lsf_info;
int m17hip_lsf_info(m17hip_ctx* ctx, const uint8_t* lsf30_host, uint32_t n, m17_lsf_info* out_host);

/* ---- numerics switch: evaluation order of the Kalman updates --------------------------------------------------------- */
/* KalmanFilter.h:41-65,91-107 (used by ClockRecovery.h:54-67 and FreqDevEstimator.h:31-48) keeps the innovation covariance and
 * the gain as lazy expressions of the blaze library (`auto S`, `auto K`), so the association and rounding of `x += K*y` and
 * `P = P - K*H*P` are decided by blaze's restructuring operators.  blaze is not part of the reference tree (empty submodule),
 * so the order is selectable: bit 0: x += double(fl32(P(:,0)*y)) * (1/S) instead of x += (double(P(:,0))/S) * y;
 * bit 1: P -= double(fl32(P(i,0)*P(0,j))) * (1/S) instead of P -= (double(P(i,0))/S) * P(0,j); bit 2: F*(P*F^T) instead of
 * (F*P)*F^T.  Default 3 (blaze's documented restructuring rules; DESIGN.md §4.4 has the measured sensitivity).  Applies to the
 * runs that follow. */
int m17hip_set_kalman_order(m17hip_ctx* ctx, int order);
/* a9/a10 per-operator parity entry: `rows` independent filters reset to z0, n updates each with measurement z[r][i] after
 * dt[r][i] samples; wrap = 10: KalmanFilter<float,10> (KalmanFilter.h:41-65), 0: SymbolKalmanFilter (:91-107).
 * out[rows][n][6] = x[0], x[1], P(0,0), P(0,1), P(1,0), P(1,1) after each update. */
int m17hip_kalman_trace(m17hip_ctx* ctx, const float* z_host, const uint32_t* dt_host, uint32_t rows, uint32_t n, int wrap, float z0, int order,
                        float* out_host);

/* ---- multi-GPU: contiguous channel shards, one context (rank) per GPU, no data-path collective ------------ */
/* Records of this context carry channel = channel_base + local channel index (default 0), so the union of the shards'
 * record sets is the record set of one big run.  Applies to the runs that follow (also to m17hip_packets_fetch). */
int m17hip_set_channel_base(m17hip_ctx* ctx, uint32_t channel_base);
/* The one exchange of the path: the gather of the frame records of the last run to `root` over RCCL (xGMI inside a node).
 * Rank 0 obtains an id (ncclGetUniqueId) and hands its 128 bytes to the other ranks by any host-side channel; every rank then
 * creates its communicator (ncclCommInitRank; collective; any context of the same device may then gather through it, one call
 * at a time).  m17hip_gather_frames is collective: every rank compacts its
 * records on the device, the counts are all-gathered, the records travel to `root` with their exact sizes (grouped
 * ncclSend / ncclRecv) and land in recs_host[capacity] rank after rank — with contiguous shards and channel bases set that is
 * global (channel, seq) order.  counts[nranks] (optional) and *total are filled on every rank; recs_host is only used on
 * `root`.  M17HIP_ETRUNC if total > capacity, M17HIP_ECOMM if RCCL is missing or fails (m17hip_comm_last_error).
 * Failure behaviour: a rank-local failure (its compaction, an allocation, a word it cannot write or read) travels inside the two
 * all-gathers every call makes before any record moves — the failing rank returns its own code, every other rank M17HIP_ECOMM, all of
 * them from the same call, and the communicator stays usable.  What words cannot settle (a peer that died, a rank that lost its device
 * between the second all-gather and the records) is bounded in time: every wait of the call has a deadline (m17hip_tune key 31, default
 * 120 s); when it passes the communicator is given up (ncclCommAbort), the call and every later call through it return M17HIP_ECOMM,
 * and the ranks create a new communicator to go on. */
typedef struct m17hip_comm m17hip_comm;
#define M17HIP_COMM_ID_BYTES 128
int m17hip_comm_get_id(void* id128);
int m17hip_comm_create(m17hip_ctx* ctx, const void* id128, int rank, int nranks, m17hip_comm** out);
void m17hip_comm_destroy(m17hip_comm* comm);
int m17hip_comm_last_error(const m17hip_comm* comm);
int m17hip_gather_frames(m17hip_ctx* ctx, m17hip_comm* comm, int root, m17_frame_rec* recs_host, uint64_t capacity, uint64_t* counts,
                         uint64_t* total);
/* Same, with the root's destination in DEVICE memory on the root's GPU (the gathered set stays in HBM for a device-side consumer). */
int m17hip_gather_frames_device(m17hip_ctx* ctx, m17hip_comm* comm, int root, m17_frame_rec* recs_dev, uint64_t capacity, uint64_t* counts,
                                uint64_t* total);
/* The per-channel sweep words of every rank (m17hip_sweep_stats: words the CALLER supplies — a rank may have processed its shard in
 * several runs) gathered to `root`: mine[n_mine] of each rank land in out_host[capacity] rank after rank — with contiguous shards, global
 * channel order.  The protocol of m17hip_gather_frames, the same code: counts[nranks] (optional) and *total on every rank, the two
 * all-gathers and their failure agreement, the root's staging growth, M17HIP_ETRUNC, the deadlines (key 31) and fault injection (key 30;
 * here 1 = this rank's upload of its words fails). */
int m17hip_gather_sweep_stats(m17hip_ctx* ctx, m17hip_comm* comm, int root, const m17_chan_stat* mine, uint64_t n_mine,
                              m17_chan_stat* out_host, uint64_t capacity, uint64_t* counts, uint64_t* total);

/* Knobs of a context (never results).  M17HIP_EINVAL for a key the library does not have.
 * key 3: samples per segment a run is processed in (default 48000; 0 = one segment): the granule of the K2 / K5 alternation — shorter
 *        segments bound how long a channel that lost sync computes its own limit-filter history, longer ones mean fewer launches.
 * key 6: BERT statistics on/off (m17hip_bert_stats; default off).
 * key 7: packet reassembly, value = packets of room per run (m17hip_packets_fetch; default 0 = off).
 * key 34: voice consumer, value = voice slots of room per channel and run (m17hip_voice_fetch, m17hip_calls_fetch; default 0 = off;
 *        at most 65536).  Set before the runs to be consumed, like keys 6 and 7; it allocates the per-channel call state, two sets of planes
 *        (max_channels x room x 17 bytes each) that alternate with the record sets, and max_channels x M17HIP_CALLS_PER_CHANNEL(room)
 *        call records per set.  With the key off a run queues exactly what it queues without it.
 * key 8: record slots per channel and run actually used, 0 = all that were allocated (2 per 1920 samples + 8, which a run cannot
 *        outgrow) — a smaller value makes M17HIP_EOVERFLOW reachable for tests.
 * key 9: diagnostic log, value = diagnostic callbacks of room per channel and run (m17hip_diag_log_fetch; default 0 = off).
 * key 10: form of the carrier-detect kernel K3: 0 = one wave per 32 channels (least wave slots: batch throughput), 1 = four-wave pipeline per
 *        32 channels (1.8x shorter chain, four times the wave slots: stream latency), -1 (default) = the pipeline for runs whose front end
 *        was queued by m17hip_demod_front (a continued stream waits for K3's chain) and for runs of a process that has not overlapped runs
 *        of different contexts on this device lately (one batch at a time: 29 -> 26 ms per 4096 x 480 000), the one-wave form while it does.
 *        Same table either way.  NOTE: -1 consults PROCESS-WIDE state (a registry of the process's contexts on the device and their last
 *        end-of-run events): the form, and with it a run's latency, depends on what other contexts of the process did lately — never a
 *        result.  A host that needs the same latency whatever else the process runs pins 0 or 1.
 * key 13: workgroups of the matched filter's grid (a K1 workgroup loops over (channel, tile) items), 0 (default) = about three items per workgroup
 *        for runs that get K3's latency form (key 10), eight for the others, at least five workgroups per compute unit.
 * key 26: gate-aware front end.  The reference runs neither the matched filter nor the correlator while its carrier detect is off
 *        (M17Demodulator.h:675-689).  1 = the matched filter of segment k >= 2 of a run skips what the carrier cannot be on for: the sequential
 *        kernel leaves the TRUE gate state at the end of every segment, a forecast walks the carrier-off update points of the next two segments
 *        from it (a closed gate reopens only when an update finds level > 4.0: a function of the table and the off state alone) and K1 follows
 *        K5 of segment k - 2 instead of running ahead — on input that is idle most of the time 1.35 x the throughput, on always-on input 5 %
 *        less (K1 on the chain); 0 = never; -1 (default) = per run: on when more than a quarter of the channel-segments of the last FETCHED run
 *        ended with the carrier off.  Same results either way.  NOTE: -1 consults the context's HISTORY (what the last fetched run looked like):
 *        the schedule of a run, and with it its latency, depends on the runs before — never a result.  A host that needs the same latency
 *        whatever came before pins 0 or 1.
 * key 33: a RAMP of segment lengths at the start of a run: value, 2 x value, 4 x value, ... samples until key 3's length is reached (0 = none).
 *        A channel that leaves the limit-filter replay in a segment carries the filter itself to the end of the NEXT one, and channels leave
 *        it mostly while sync is being acquired: short first segments bound what that costs the launches concerned.  One batch at a time
 *        23.65 -> 22.8 ms per 4096 x 480 000 with 9600; with batches in flight or a continued stream the extra launches cost 1-3 % (NOTES 6.5).
 *        -1 (default) = per run: 9600 when the run is the only thing in flight on the device as far as the library can see (no other context's
 *        run unfinished when this one is queued, none since this context's previous run — the rule key 10 = -1 uses) and was not staged, else none.
 *        NOTE: like keys 10 and 26, -1 consults process HISTORY: the schedule of a run, and with it its latency, depends on what was in flight
 *        before it — never a result.  A host that needs the same latency whatever came before pins a value.
 * key 20: what happens after a forced dcd.unlock() took a channel off the limit-filter replay: 0 (default) = the replay's state is re-derived
 *        beside the sequential kernel and the channel computes its own filter history through the next segment (the sequential kernel never
 *        waits: best wherever its chain of launches is what a step lasts — a continued stream, one batch at a time); 1 = the replay of the next
 *        segment is redone for those channels, history stored, IN FRONT of the sequential kernel (1-2 ms of replay latency on that chain, fewer
 *        instructions in all).  With round 4's matched filter 1 was 1.4 % faster when several independent batches were in flight; with
 *        round 5's it is slower in every regime (two batches 22.6 against 21.4 ms per 4096 x 480 000, a continued stream 28.0 against 24.7,
 *        one batch at a time 28.9 against 26.3: NOTES 5.5) and stays only as the other side of that comparison.
 * key 15: 1 (default) = the sequential kernel leaves the payload frames of running stream / BERT transmissions undecoded (LLRs to a
 *        store, the record reserved) and a lane-per-frame kernel decodes them after the run; 0 = every frame is decoded where it completes.
 * key 17: 1 (default) = the running EVM of the diagnostic callback (RunningStandardDeviation: three dependent operations per payload symbol
 *        that nothing in the demodulator reads) is folded OUTSIDE the sequential kernel: that kernel writes one 4-byte operation per symbol
 *        (4 B x samples / 10 per channel of device memory), one lane per channel folds them in the reference's order as extra workgroups of
 *        the limit-filter replay / the deferred decode, and m17_diag::evm and the diagnostic log carry the same values as with 0 = folded in
 *        the sequential kernel, symbol by symbol.  Can be changed between runs.
 * key 18 (tests): floats per channel row of deferred EVM operations (key 17), 0 (default) = what a run of max_samples can produce; with a
 *        smaller row a channel outruns it, the operations beyond are dropped and m17hip_diag_fetch / m17hip_diag_log_fetch return
 *        M17HIP_EOVERFLOW (every diagnostic field but `evm` is still right; the frame records are not affected).
 * key 16: 1 = m17hip_upload_i16, m17hip_upload_i16_device, m17hip_synth_i16, m17hip_synth_sweep_i16 and m17hip_synth_tx_i16 write the context's STAGING slab (as
 *        m17hip_upload_i16_async does, but complete when they return) and stage it for the next run; 0 (default) = the current slab.
 * key 30 (tests): fault injection for m17hip_gather_frames* and m17hip_gather_sweep_stats: 1 = this rank's compaction (its upload of
 *        the words) fails inside the call, 2 = the root's staging
 *        allocation fails, 3 = this rank's word of the second exchange cannot be written (and, on the root, the staging is grown whether
 *        it has to be or not), 4 = this rank cannot read the first exchange, 5 = this rank cannot read the second exchange; 0 = none.
 *        Under 1-4 every rank makes all its collective calls and all return from the same call; 5 is the case key 31 bounds.
 * key 31: deadline in milliseconds of every wait inside m17hip_gather_frames* and m17hip_gather_sweep_stats (default 120000, 0 = none).
 * The measurement build of the library (make -C m17-cxx-demod_amd/csrc tools -> libm17hip_tools.so, -DM17_TOOLS; tools/ only) adds
 * key 1 / key 19 (section timers / per-wave working times of the sequential kernel -> m17hip_debug_counters) and the schedule
 * experiments 4, 5, 12, 14, 21, 25 (csrc/m17hip.hip, m17hip_tune). */
int m17hip_tune(m17hip_ctx* ctx, int key, int64_t value);

/* Measurement build only (otherwise *waves = 0).  Diagnostic counters of the last sequential-kernel launch (after m17hip_tune(ctx, 1, 1)): host[channels][40] =
 * {total, bulk chunks, single-sample steps, frame decodes} in 10 ns ticks, {#chunks, #single steps, samples in chunks,
 * #chunks cut by a clock move | #decodes << 32}, then [8..14] ticks and [16..22] counts of single-sample steps per
 * DemodState. */
int m17hip_debug_counters(m17hip_ctx* ctx, uint64_t* host, uint32_t max_waves, uint32_t* waves);

/* ---- measurement ----------------------------------------------------------------------------------- */
/* When enabled, every kernel launch of the context is timed by HIP events: the five kernels of a run's chain (matched filter, carrier detect, limit filter,
 * sequential kernel, deferred decode) by events BOUND to the launch (hipExtLaunchKernelGGL: the dispatch's own time stamps, what rocprofv3 reports), the others by
 * a pair recorded around them on the stream they run on.  Not free on a chain of dependent launches: a continued stream 0.45 ms of a 21.7 ms step, two batches in
 * flight 1.5 % (tools/stream_only.py, tools/stream_history.py: TIMING=1). */
int m17hip_timing_enable(m17hip_ctx* ctx, int on);
/* Accumulated device time (ms) and launch count per kernel since the last m17hip_timing_reset:
 * which: 0 = fir_rrc150, 1 = dcd, 2 = demod_seq, 3 = viterbi/decode_frames, 4 = correlator, 5 = compaction,
 * 6 = limit_track (the limit filter run ahead of demod_seq; in m17hip_fir_correlator the limit filter's chain, 4 = its correlations),
 * 7 = voice (the voice consumer, m17hip_tune key 34: one launch per run, on the payload stream behind the deferred decode),
 * 8 = discriminate (the FM discriminator of m17hip_upload_iq*: one launch per IQ block),
 * 9 = tune (the tuner of m17hip_upload_wide* under m17hip_wide_config: one launch per wideband block),
 * 10 = tune2 (the two-stage tuner of m17hip_upload_wide* under m17hip_wide_config2: likewise),
 * 11 = channelise (the channeliser of m17hip_upload_wide* under m17hip_wide_raster: likewise), 12 = survey (the two kernels of m17hip_wide_survey, one
 * entry per surveyed block), 13 = resample (the resampling tuner of m17hip_upload_wide* under m17hip_wide_resample: one launch per wideband block), 14 = spectrum (the two
 * kernels of m17hip_wide_spectrum, one entry per transformed block), 15 = synth_wide (the two kernels of m17hip_synth_wide*, one entry per block),
 * 16 = meter (wide_meter_kernel of m17hip_wide_meter, one entry per metered block; the metered tuner keeps its own index),
 * 17 = squelch (wide_squelch_kernel of m17hip_wide_squelch, one entry per squelched block; its spectrum and its tuner keep their own indices),
 * 18 = squelch_slots (the three kernels of m17hip_wide_squelch_slots, one entry per squelched block; likewise),
 * 19 = squelch_floor (squelch_floor_kernel of m17hip_wide_squelch_floor, one entry per block uploaded with that mode on; none with it off),
 * 20 = scan (wide_scan_kernel of m17hip_wide_scan, one entry per scanned block; none with it off). */
int m17hip_timing_get(m17hip_ctx* ctx, int which, double* total_ms, uint64_t* launches);
int m17hip_timing_reset(m17hip_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* M17HIP_H */
