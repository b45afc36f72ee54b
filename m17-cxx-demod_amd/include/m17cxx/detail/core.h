// Arithmetic cores of the M17 demodulation path, written ONCE and compiled for both sides of the boundary: the HIP kernels
// (csrc/, under hipcc these are __host__ __device__) and the scalar operator classes of this directory (any C++17/20 host
// compiler).  Every rounding step of the path that decides a decoded bit is defined here and nowhere else, so the scalar
// classes and the kernels cannot drift apart.  Reference file:line is cited per function
// (/root/reference/include/m17cxx unless stated).  No dependency on the oracle, on HIP or on the C ABI.
//
// Build contract: -ffp-contract=off (every fp32 multiply and add rounds separately, as in the reference's default x86-64
// build; the few fused operations below are written as explicit fma calls and are exact by construction).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define M17_HD __host__ __device__ __forceinline__
#else
#define M17_HD inline
#endif

namespace mobilinkd
{
namespace core
{

// ---- a1: sample scaling (apps/m17-demod.cpp:486-489) ---------------------------------------------------------------
// x = float(double(s16) / 41067.0), optionally s16 *= -1 first (in int16: -(-32768) wraps to -32768).
// (float)s / 41067.0f is bit-identical for all 65536 inputs (41067 is odd and < 2^16: s / 41067 is never within 2^-40 of a
// float midpoint, so the double rounding is harmless), and so is one Newton step on q = s * RN(1/41067):
// r = fma(-q, 41067, s) is the exact remainder, fma(r, 1/41067, q) the correctly rounded quotient.
M17_HD float scale_i16(int s, bool invert)
{
    if (invert) s = (int)(int16_t)(-s);
    const float rcp = 1.0f / 41067.0f;
    const float fs = (float)s;
    const float q = fs * rcp;
    const float r = __builtin_fmaf(-q, 41067.0f, fs);
    return __builtin_fmaf(r, rcp, q);
}
// The float twin: a float32 input sample is already what the reference's M17Demodulator<float>::operator() receives — nothing is scaled.
// Under invert it is negated, which is exact (a sign-bit flip, NaNs and zeroes included); there is no -32768 wrap.
M17_HD float scale_f32(float v, bool invert) { return invert ? -v : v; }

// ---- a0: FM discriminator in front of a1 (complex IQ input, m17hip_upload_iq): y[n] = gain * arg(x[n] * conj(x[n-1])) ----------------------
// No reference file: the reference's users put rtl_fm in front of it.  Written here, once, so that the kernel and the host form give the same words.
// x[n] * conj(x[n-1]) of (i, q) and the sample before it (pi, pq): four float32 products and two sums, each rounded apart (the build contract).
// Nothing is scaled: an int16 sample is converted to float first, which is exact, so both IQ formats share this body.
M17_HD void fm_cross(float i, float q, float pi, float pq, float& re, float& im)
{
    const float a = i * pi, b = q * pq, c = q * pi, d = i * pq;
    re = a + b;
    im = c - d;
}
// The project's own four-quadrant arctangent of (im, re), float32, radians — NOT atan2f: the device library's and glibc's disagree in the last bits, and
// this project compares words.  z = min(|re|,|im|) / max(|re|,|im|), one correctly rounded divide; atan z = z * P(z^2), P of degree 7 in Horner form
// (a weighted least-squares fit over [0, 1], its error equalised; multiply and add rounded apart); then pi/2 - r above the diagonal, pi - r in the left half
// plane, and the sign of im.  Absolute error against double-precision atan2 of the same two floats: 3.2e-7 rad measured over 5e6 points, near-axis and
// near-diagonal ones included (bound asserted: 2^-20; tests/test_iq_input.py).
// fm_phase(+-0, +-0) = +0: the first sample behind a zero carry is silence, not pi.  Everything runs on the magnitudes and the sign of im is put on last, so
// fm_phase(re, -im) == -fm_phase(re, im) to the bit for every im != 0: a conjugated (spectrum-flipped) input is the exact negation.
// Non-finite inputs: whatever IEEE arithmetic makes of them below (inf / inf is a NaN; a lone infinity is an axis).
M17_HD float fm_phase(float re, float im)
{
    const float are = __builtin_fabsf(re), aim = __builtin_fabsf(im);
    const bool steep = aim > are;
    const float mx = steep ? aim : are, mn = steep ? are : aim;
    if (mx == 0.0f && mn == 0.0f) return 0.0f;
    const float z = mn / mx;
    const float s = z * z;
    float p = -0.00405456498f;
    p = p * s; p = p + 0.0218629558f;
    p = p * s; p = p + -0.0559123345f;
    p = p * s; p = p + 0.0964219868f;
    p = p * s; p = p + -0.139086306f;
    p = p * s; p = p + 0.199465662f;
    p = p * s; p = p + -0.333298594f;
    p = p * s; p = p + 0.999999344f;
    float r = z * p;
    if (steep) r = 1.57079637f - r;
    if (re < 0.0f) r = 3.14159274f - r;
    return __builtin_copysignf(r, im);
}
// one more rounded multiply: at gain 1 the output is radians per sample (the demodulator normalises by its own deviation estimate: any positive gain decodes)
M17_HD float fm_discriminate(float i, float q, float pi, float pq, float gain)
{
    float re, im;
    fm_cross(i, q, pi, pq, re, im);
    return gain * fm_phase(re, im);
}

// ---- a-1: the tuner in front of a0 (wideband IQ input, m17hip_upload_wide): mix to the channel's offset, low-pass, keep every R-th sample ----
// No reference file: the reference's users run rtl_fm or a channeliser for it.  Written here, once, so that the kernel and the host form give the same words.
// The oscillator: cos and sin of 2 pi p / 2^32 — the project's own, NOT sincosf (the device library's and glibc's disagree in the last bits).  The quadrant is
// p >> 30; inside it t = bits 29..6 of p as a fraction (24 bits: the conversion and the scaling are exact, the low 6 bits of p are not looked at), and
// sin(pi/2 t) = t S(t^2), cos(pi/2 t) = C(t^2): least-squares fits of degree 4 in t^2 over [0, 1], Horner form, multiply and add rounded apart; C's constant
// term is 1, so t = 0 gives (1, 0) exactly and the four axis phases p = 0, 2^30, 2^31, 3 2^30 give (1,0), (0,1), (-1,0), (0,-1) with zeroes of either sign:
// the quadrant's rotation is a swap and sign flips.  Absolute error of either component against float64, measured over all 2^26 distinct inputs: 2.8e-7
// (bound asserted: 2^-21; tests/test_wide_input.py) — far below 2^-17, half an LSB of a full-scale int16 sample.
M17_HD void nco(uint32_t p, float& c, float& s)
{
    const uint32_t q = p >> 30;
    const float t = (float)((p >> 6) & 0xFFFFFFu) * 5.9604644775390625e-08f;
    const float u = t * t;
    float a = 0.000151263870f;
    a = a * u; a = a + -0.00467313733f;
    a = a * u; a = a + 0.0796890929f;
    a = a * u; a = a + -0.645963490f;
    a = a * u; a = a + 1.57079625f;
    const float sn = t * a;
    float b = 0.000862553774f;
    b = b * u; b = b + -0.0208188817f;
    b = b * u; b = b + 0.253655702f;
    b = b * u; b = b + -1.23369920f;
    b = b * u; b = b + 1.0f;
    const float x = (q & 1u) ? sn : b, y = (q & 1u) ? b : sn;   // (cos, sin) of quadrant 0 or, swapped, (-cos, sin) of quadrant 1
    c = (q == 1u || q == 2u) ? -x : x;
    s = (q >= 2u) ? -y : y;
}
// Mixing is fm_cross(i, q, c, s): x * conj(nco), four products and two sums rounded apart.  The phase of wideband sample m of a feed is fcw * (uint32_t)m in
// uint32 — exact modulo 2^32, no accumulator, so a block boundary cannot shift it.
M17_HD void ddc_mix(float i, float q, uint32_t fcw, uint32_t m, float& re, float& im)
{
    float c, s;
    nco(fcw * m, c, s);
    fm_cross(i, q, c, s, re, im);
}
// One step of the low-pass filter's two chains, real and imaginary apart: acc = fma(h, v, acc).  z[n] = sum_{i=0}^{L-1} h[i] mixed[nR + R - 1 - i] is these
// steps from (+0, +0) in the order i = 0, 1, ..., L - 1 and in no other; the fused form is exact by construction on both sides (as in scale_i16), and on the
// device one packed fma does both chains.
M17_HD void ddc_tap(float h, float vre, float vim, float& re, float& im)
{
    re = __builtin_fmaf(h, vre, re);
    im = __builtin_fmaf(h, vim, im);
}
// the whole sum over a linear array: newest[0] is mixed[nR + R - 1] as (re, im), newest[-2 i] the sample i taps back
M17_HD void ddc_fir(const float* h, uint32_t L, const float* newest, float& re, float& im)
{
    re = 0.0f; im = 0.0f;
    for (uint32_t i = 0; i < L; ++i) ddc_tap(h[i], newest[-2 * (int64_t)i], newest[-2 * (int64_t)i + 1], re, im);
}
// an 8-bit IQ component in rtl_sdr's convention: unsigned around 127.5 (exact)
M17_HD float ddc_u8(uint8_t u) { return (float)u - 127.5f; }
// Two stages (m17hip_wide_config2), R1 then R2: u[p] = sum_i h1[i] mixed[p R1 + R1 - 1 - i], z[n] = sum_i h2[i] u[n R2 + R2 - 1 - i] — ddc_fir over the mixed
// feed, then ddc_fir over the u, nothing else.  One block of n outputs over linear arrays of (re, im): `mixed` points at the block's sample 0 and `u` at its
// u 0 (n R2 of them follow).  The u from -fresh on are computed here: fresh = L2 - 1 makes all the u the block reads from the (L2 - 1) R1 + L1 - 1 mixed
// samples in front of it, as the kernel does (a u is a function of the mixed feed alone, so a caller that kept the u of the block before passes 0 and gets the
// same words).  z: [n][2].
M17_HD void ddc_fir2(const float* h1, uint32_t L1, uint32_t R1, const float* h2, uint32_t L2, uint32_t R2, const float* mixed, uint32_t n, uint32_t fresh,
                     float* u, float* z)
{
    for (int64_t p = -(int64_t)fresh; p < (int64_t)n * R2; ++p) ddc_fir(h1, L1, mixed + 2 * (p * R1 + R1 - 1), u[2 * p], u[2 * p + 1]);
    for (uint32_t m = 0; m < n; ++m) ddc_fir(h2, L2, u + 2 * ((int64_t)m * R2 + R2 - 1), z[2 * m], z[2 * m + 1]);
}
// A second stage that RESAMPLES by U / D (m17hip_wide_resample; U <= D, coprime): the u zero-stuffed by U, low-passed with h2 at 48000 D, the sample at
// n D + D - 1 kept — with the products of the stuffed zeroes left out:
//   N_n = n D + D - 1 (64 bits),  i0 = N_n mod U,  b = N_n div U,  z[n] = sum_{j : i0 + U j < L2} h2[i0 + U j] u[b - j]
// the two chains of ddc_tap from +0, j ascending.  At U = 1 that is ddc_fir2's z word for word (i0 = 0, b = n D + D - 1).  n is counted within a block and a
// block holds a multiple of U outputs — (n / U) D u —, so the phase never depends on the feed's history.
// The whole host form of one block, composed of ddc_mix, ddc_tap and fm_discriminate and nothing else.  x: the block's converted samples (re, im), x[0] its
// sample 0, with the H = (J2 - 1) R1 + L1 - 1 samples in front of it (J2 = ceil(L2 / U)), (n / U) D R1 behind; `count` the feed's index of sample 0.
// Scratch: mixed [H + (n / U) D R1][2] and u [J2 - 1 + (n / U) D][2].  carry[2]: the z in front of output 0, on return the block's last z.  y[n]; z [n][2].
M17_HD void ddc_resample(const float* h1, uint32_t L1, uint32_t R1, const float* h2, uint32_t L2, uint32_t U, uint32_t D, const float* x, uint32_t fcw,
                         uint32_t count, uint32_t n, float* mixed, float* u, float* z, float* carry, float gain, float* y)
{
    const int64_t J2 = (L2 + U - 1) / U, H = (J2 - 1) * R1 + L1 - 1, NU = (int64_t)(n / U) * D;
    float* mx = mixed + 2 * H;
    float* uu = u + 2 * (J2 - 1);
    for (int64_t k = -H; k < NU * R1; ++k) ddc_mix(x[2 * k], x[2 * k + 1], fcw, count + (uint32_t)k, mx[2 * k], mx[2 * k + 1]);
    for (int64_t p = 1 - J2; p < NU; ++p) {
        float re = 0.0f, im = 0.0f;
        const float* newest = mx + 2 * (p * R1 + R1 - 1);
        for (uint32_t i = 0; i < L1; ++i) ddc_tap(h1[i], newest[-2 * (int64_t)i], newest[-2 * (int64_t)i + 1], re, im);
        uu[2 * p] = re; uu[2 * p + 1] = im;
    }
    float pre = carry[0], pim = carry[1];
    for (uint32_t m = 0; m < n; ++m) {
        const uint64_t N = (uint64_t)m * D + D - 1;
        const int64_t b = (int64_t)(N / U);
        float re = 0.0f, im = 0.0f;
        int64_t j = 0;
        for (uint32_t i = (uint32_t)(N % U); i < L2; i += U, ++j) ddc_tap(h2[i], uu[2 * (b - j)], uu[2 * (b - j) + 1], re, im);
        z[2 * m] = re; z[2 * m + 1] = im;
        y[m] = fm_discriminate(re, im, pre, pim, gain);
        pre = re; pim = im;
    }
    carry[0] = pre; carry[1] = pim;
}

// ---- a-1c: the channeliser (m17hip_wide_raster): M channels on a raster, spaced rate / M.  The single-stage tuner's z with the oscillator exactly on the
// raster, z_k[n] = sum_i h[i] x[m_n - i] exp(-2 pi j k (m_n - i) / M), computed as a FOLD of the taps into M partial sums — the phase of tap i depends on
// (m_n - i) mod M alone — and one M-point DFT over a table of M twiddles, tw[j] = exp(-2 pi j j / M) as (re, im) floats.  The table is data: made once, on the
// host, in double (m17hip_wide_raster_twiddles), so no libm enters the words.
// The fold of residue r at an output whose newest sample is m_n: the two chains of ddc_tap from +0 over the taps i = i0, i0 + M, i0 + 2M, ... < L in that
// order, i0 = (m_n - r) mod M.  `newest` as in ddc_fir; a residue no tap falls on (i0 >= L) is (+0, +0).
M17_HD void chan_fold(const float* h, uint32_t L, uint32_t M, uint32_t i0, const float* newest, float& re, float& im)
{
    re = 0.0f; im = 0.0f;
    uint32_t i = i0;
    // (eight taps and samples fetched together, then their eight steps in order: the same chain — on the device the loads' latencies are paid once, not
    // once per step)
    for (; L > 7 * M && i < L - 7 * M; i += 8 * M) {
        float t[8], vre[8], vim[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int64_t j = (int64_t)i + (int64_t)k * M;
            t[k] = h[j]; vre[k] = newest[-2 * j]; vim[k] = newest[-2 * j + 1];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) ddc_tap(t[k], vre[k], vim[k], re, im);
    }
    for (; i < L; i += M) ddc_tap(h[i], newest[-2 * (int64_t)i], newest[-2 * (int64_t)i + 1], re, im);
}
// One step of a DFT sum: acc += a * t, complex, as four fma in this order (the real chain takes a.re t.re then -a.im t.im, the imaginary one a.re t.im then
// a.im t.re).  A twiddle on an axis (0 / +-1) adds its term exactly.
M17_HD void chan_mac(float are, float aim, float tre, float tim, float& re, float& im)
{
    re = __builtin_fmaf(are, tre, re);
    re = __builtin_fmaf(-aim, tim, re);
    im = __builtin_fmaf(are, tim, im);
    im = __builtin_fmaf(aim, tre, im);
}
// M = M1 x M2 with M2 the largest divisor of M whose square is at most M (so M2 <= M1, and M1 is the smallest cofactor any factorisation offers): accepted
// when M1 <= 16.  6 = 3 x 2, 12 = 4 x 3, 192 = 16 x 12, 256 = 16 x 16; a prime p <= 16 is p x 1; 34 = 17 x 2 is refused.
M17_HD bool chan_factor(uint32_t M, uint32_t& M1, uint32_t& M2)
{
    M1 = 0; M2 = 1;
    if (M < 1 || M > 256) return false;
    for (uint32_t d = 1; d * d <= M; ++d) if (M % d == 0) M2 = d;
    M1 = M / M2;
    return M1 <= 16;
}
// With r = r1 + M1 r2 and k = M2 k1 + k2 (r1, k1 < M1; r2, k2 < M2):  z_k = sum_{r1} tw[(k r1) mod M] * a[r1][k2],  a[r1][k2] = sum_{r2} tw[M1 ((k2 r2) mod M2)]
// * w[r1 + M1 r2].  Pass 1, one element: r2 ascending from (+0, +0).  w: [M][2].
M17_HD void chan_pass1(const float* w, uint32_t M1, uint32_t M2, const float* tw, uint32_t r1, uint32_t k2, float& re, float& im)
{
    const uint32_t M = M1 * M2, dt = M1 * k2;
    re = 0.0f; im = 0.0f;
    for (uint32_t r2 = 0, t = 0; r2 < M2; ++r2) {
        const uint32_t r = r1 + M1 * r2;
        chan_mac(w[2 * r], w[2 * r + 1], tw[2 * t], tw[2 * t + 1], re, im);
        t += dt; if (t >= M) t -= M;
    }
}
// Pass 2, one bin k < M: r1 ascending from (+0, +0).  a: [M1][M2][2].
M17_HD void chan_pass2(const float* a, uint32_t M1, uint32_t M2, const float* tw, uint32_t k, float& re, float& im)
{
    const uint32_t M = M1 * M2, k2 = k % M2;
    re = 0.0f; im = 0.0f;
    for (uint32_t r1 = 0, t = 0; r1 < M1; ++r1) {
        const uint32_t e = r1 * M2 + k2;
        chan_mac(a[2 * e], a[2 * e + 1], tw[2 * t], tw[2 * t + 1], re, im);
        t += k; if (t >= M) t -= M;
    }
}
// The raster survey (m17hip_wide_survey): the power of one z, and how many powers a first-level sum holds.  A bin's power over a block's survey times
// p_0 .. p_{J-1} is a sum on two levels, both chains of plain float adds from +0 in ascending order: q_g over p_j, j = 16 g .. min(16 g + 15, J - 1), then
// the q_g.  The order is part of the definition (a workgroup per group on the device, a fixed-order second step, no atomics).
constexpr uint32_t CHAN_SURVEY_GROUP = 16;
M17_HD float chan_power(float re, float im) { return __builtin_fmaf(re, re, im * im); }

// ---- a-1d: the source spectrum (m17hip_wide_spectrum): the averaged periodogram of a source block, whatever tunes or channelises it.  Frames of N = 2^logn
// samples begin where the FEED's sample index is a multiple of `hop`; each is windowed (two plain multiplies per sample), transformed by a radix-2
// decimation-in-time FFT over a bit-reversed load, and chan_power of every bin is summed over the block's frames on the survey's two levels
// (CHAN_SURVEY_GROUP frames per group).  The twiddles tw[j] = exp(-2 pi j j / N), j < N / 2, are data (m17hip_wide_spectrum_twiddles).
// The frames of a block of W samples that begins at sample c0 of the feed: frame f starts at block sample first + f hop, first = (hop - c0 mod hop) mod hop
// from all 64 bits of the count, and J counts the f with first + f hop + N <= W — a frame that would straddle the block's end is not taken.
M17_HD void spec_frames(uint64_t c0, uint32_t W, uint32_t N, uint32_t hop, uint32_t& first, uint32_t& J)
{
    first = (uint32_t)((hop - c0 % hop) % hop);
    J = W >= N && first <= W - N ? (W - N - first) / hop + 1 : 0;
}
// the logn low bits of i in reverse order (logn 1..32)
M17_HD uint32_t spec_bitrev(uint32_t i, uint32_t logn)
{
    i = (i >> 16) | (i << 16);
    i = ((i & 0xFF00FF00u) >> 8) | ((i & 0x00FF00FFu) << 8);
    i = ((i & 0xF0F0F0F0u) >> 4) | ((i & 0x0F0F0F0Fu) << 4);
    i = ((i & 0xCCCCCCCCu) >> 2) | ((i & 0x33333333u) << 2);
    i = ((i & 0xAAAAAAAAu) >> 1) | ((i & 0x55555555u) << 1);
    return i >> (32 - logn);
}
// THE butterfly, one formula for every one of every stage, the twiddles on the axes included: (a, b) <- (a + b t, a - b t), each a chan_mac onto a — the
// sum with t, the difference with -t (a negation is exact) — so a component is rounded twice.  A non-finite b reaches both outputs through the same four
// fma on either side.  a, b, t: (re, im).
M17_HD void spec_butterfly(float* a, float* b, const float* t)
{
    float pre = a[0], pim = a[1], mre = a[0], mim = a[1];
    chan_mac(b[0], b[1], t[0], t[1], pre, pim);
    chan_mac(b[0], b[1], -t[0], -t[1], mre, mim);
    a[0] = pre; a[1] = pim; b[0] = mre; b[1] = mim;
}
// Stage s = 1 .. logn of the FFT over v[N][2] (bit-reversed on entry, in place), taken in ascending order of s; butterfly j < N / 2 of stage s pairs
// v[i] and v[i + h], h = 2^(s-1), i = 2 h (j div h) + j mod h, with the twiddle tw[(j mod h) 2^(logn-s)].  The butterflies of a stage share no element.
M17_HD void spec_item1(float* v, const float* tw, uint32_t logn, uint32_t s, uint32_t j)
{
    const uint32_t h = 1u << (s - 1), pos = j & (h - 1), i = ((j >> (s - 1)) << s) + pos;
    spec_butterfly(v + 2 * i, v + 2 * (i + h), tw + 2 * (pos << (logn - s)));
}
// Stages s and s + 1 in one pass: item q < N / 4 takes the four butterflies among v[i], v[i + h], v[i + 2h], v[i + 3h], i = 4 h (q div h) + q mod h, that
// spec_item1 takes in those two stages, stage s first — the same words, with the four elements in registers in between.
M17_HD void spec_item2(float* v, const float* tw, uint32_t logn, uint32_t s, uint32_t q)
{
    const uint32_t h = 1u << (s - 1), pos = q & (h - 1), i = ((q >> (s - 1)) << (s + 1)) + pos;
    float e0[2] = {v[2 * i], v[2 * i + 1]}, e1[2] = {v[2 * (i + h)], v[2 * (i + h) + 1]};
    float e2[2] = {v[2 * (i + 2 * h)], v[2 * (i + 2 * h) + 1]}, e3[2] = {v[2 * (i + 3 * h)], v[2 * (i + 3 * h) + 1]};
    const float* t = tw + 2 * (pos << (logn - s));
    spec_butterfly(e0, e1, t);
    spec_butterfly(e2, e3, t);
    spec_butterfly(e0, e2, tw + 2 * (pos << (logn - s - 1)));
    spec_butterfly(e1, e3, tw + 2 * ((pos + h) << (logn - s - 1)));
    v[2 * i] = e0[0]; v[2 * i + 1] = e0[1]; v[2 * (i + h)] = e1[0]; v[2 * (i + h) + 1] = e1[1];
    v[2 * (i + 2 * h)] = e2[0]; v[2 * (i + 2 * h) + 1] = e2[1]; v[2 * (i + 3 * h)] = e3[0]; v[2 * (i + 3 * h) + 1] = e3[1];
}
// One windowed sample on its way into the FFT: two plain multiplies.
M17_HD void spec_window(float w, float xre, float xim, float& re, float& im) { re = w * xre; im = w * xim; }

// ---- a-1e: the channel meter (m17hip_wide_meter): per channel and per WINDOW of `window` outputs of the feed, the sums of p = chan_power(z), of the
// discriminator's y and of e = y * y (meter_sq: one rounded multiply), under every wideband configuration.  Windows are a property of the FEED: with N0 the
// 64-bit number of outputs in front of a block of T outputs, a0 = N0 mod window (from all 64 bits) and PIECE k of the block holds the outputs n with
// (a0 + n) div window == k, k < K = (a0 + T - 1) div window + 1 — a window that a block boundary cuts is reported in two pieces, and nothing is carried.
// A piece's sum is the survey's sum on two levels: q_g over the piece's outputs 16 g .. min(16 g + 15, m - 1), then the q_g, all chains of plain adds from +0.
M17_HD void meter_pieces(uint64_t N0, uint32_t T, uint32_t window, uint32_t& a0, uint32_t& K)
{
    a0 = (uint32_t)(N0 % window);
    K = (uint32_t)(((uint64_t)a0 + T - 1) / window) + 1;
}
// piece k < K of a block of T >= 1 outputs: its first output lo and its count m >= 1
M17_HD void meter_piece(uint32_t a0, uint32_t T, uint32_t window, uint32_t k, uint32_t& lo, uint32_t& m)
{
    const uint64_t b = (uint64_t)k * window, e = b + window - a0;   // the window's first output and the one behind its last, counted from the block's output -a0 / 0
    lo = b > a0 ? (uint32_t)(b - a0) : 0u;
    m = (e < T ? (uint32_t)e : T) - lo;
}
M17_HD float meter_sq(float y) { return y * y; }
// the chain of plain float adds of v[0 .. n - 1] onto acc, ascending: both levels are this
M17_HD float meter_chain(float acc, const float* v, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i) acc = acc + v[i];
    return acc;
}
// a piece's sum over v[0 .. n - 1]: first-level chains from +0 over CHAN_SURVEY_GROUP values each, the second-level chain from +0 over those
M17_HD float meter_sum(const float* v, uint32_t n)
{
    float acc = 0.0f;
    for (uint32_t g = 0; g < n; g += CHAN_SURVEY_GROUP) {
        const float q = meter_chain(0.0f, v + g, n - g < CHAN_SURVEY_GROUP ? n - g : CHAN_SURVEY_GROUP);
        acc = acc + q;
    }
    return acc;
}

// ---- a-1f: the spectrum squelch (m17hip_wide_squelch): per block and channel of the three tuners, whether the channel's workgroups tune the block at all,
// decided from the block's own spectrum plane P[source][N] of J frames.  The channel's bin is the spectrum's index rule in integers — bin k belongs to
// k Fs / N, the frequency word to fcw Fs / 2^32 —, rounded to the nearest bin, a word half way between two bins to the upper one, circular.
M17_HD uint32_t squelch_bin(int32_t fcw, uint32_t logn)
{
    const int64_t v = ((int64_t)fcw + ((int64_t)1 << (31 - logn))) >> (32 - logn);   // (arithmetic: the floor)
    return (uint32_t)v & ((1u << logn) - 1u);
}
// the band power: the chain from +0 of plain float adds of row[(k + d) & (N - 1)], d = -B .. B ascending (B < N / 2)
M17_HD float squelch_band(const float* row, uint32_t N, uint32_t k, uint32_t B)
{
    float acc = 0.0f;
    for (uint32_t i = 0; i <= 2 * B; ++i) acc = acc + row[(k + N - B + i) & (N - 1)];
    return acc;
}
// a threshold of the block: the source's level per frame times the block's frames, one rounded multiply
M17_HD float squelch_level(float level, uint32_t J) { return level * (float)J; }
// One block's step of a channel: h the hold count in front of it, b its band power, to / tc the open and close thresholds, J the block's frames.  Returns
// h' | open << 31.  A block without a frame leaves the channel open and h as it is; the comparisons are negated so that a NaN band opens as well.
constexpr uint32_t SQUELCH_OPEN = 0x80000000u;
M17_HD uint32_t squelch_step(uint32_t h, float b, float to, float tc, uint32_t hang, uint32_t J)
{
    if (J == 0) return h | SQUELCH_OPEN;
    uint32_t hn;
    if (!(b < to)) hn = hang + 1u;
    else if (h > 0u && !(b < tc)) hn = hang + 1u;
    else hn = h > 0u ? h - 1u : 0u;
    return hn | (hn > 0u ? SQUELCH_OPEN : 0u);
}
// ---- a-1h: the sources' noise floor (m17hip_wide_squelch_floor): the levels of both squelch modes made from the block's own plane P[source][N] of J frames.
// The floor of a row is its UPPER MEDIAN by key: squelch_floor_key orders the powers — sums of chan_power from +0, so no non-NaN value has its sign bit set —
// as unsigned words, every NaN last.  The median is the element whose key has rank N / 2 (0-based) among the row's N keys in ascending order: a selection,
// so every correct algorithm gives the same word.  It is NOT np.median, which takes the mean of the two middle values in float64.
constexpr uint32_t SQUELCH_FLOOR_NAN = 0x7FC00000u;   // the carry in front of the first block, and the median of a row with more than N / 2 NaNs
M17_HD uint32_t squelch_floor_key(float x) { return x != x ? 0xFFFFFFFFu : __builtin_bit_cast(uint32_t, x); }
M17_HD float squelch_floor_value(uint32_t key) { return __builtin_bit_cast(float, key == 0xFFFFFFFFu ? SQUELCH_FLOOR_NAN : key); }
// the row's upper median, stated as plainly as possible (the host form; the kernel selects the same key by radix): the key with exactly N / 2 keys in
// front of it when ties are broken by index
M17_HD float squelch_floor_median(const float* row, uint32_t N)
{
    for (uint32_t i = 0; i < N; ++i) {
        const uint32_t k = squelch_floor_key(row[i]);
        uint32_t below = 0;
        for (uint32_t j = 0; j < N; ++j) {
            const uint32_t q = squelch_floor_key(row[j]);
            below += (q < k || (q == k && j < i)) ? 1u : 0u;
        }
        if (below == N / 2) return squelch_floor_value(k);
    }
    return squelch_floor_value(0xFFFFFFFFu);   // (N == 0: not reached)
}
// the block's floor per frame and band: the median times the band's bins over the block's frames, two rounded operations, not below floor_min.  A NaN
// stays a NaN.  J >= 1.
M17_HD float squelch_floor(float med, uint32_t B, uint32_t J, float floor_min)
{
    const float f = (med * (float)(2u * B + 1u)) / (float)J;
    return f < floor_min ? floor_min : f;
}
// the source's carried floor F behind a block whose floor is f: the first block sets it whatever it is (the carry starts as a NaN); a non-finite f leaves
// it; otherwise F moves towards f by `rise` or `fall`, and a factor of 1 or more returns f to the bit (fmaf(1, f - F, F) need not)
M17_HD float squelch_track(float F, float f, float rise, float fall)
{
    if (!(F == F)) return f;
    if (!(f - f == 0.0f)) return F;
    const float a = f > F ? rise : fall;
    return a >= 1.0f ? f : __builtin_fmaf(a, f - F, F);
}
// the block's levels per frame from the carried floor: one rounded multiply each (squelch_level takes them from there, as it takes given levels)
M17_HD float squelch_floor_level(float F, float ratio) { return F * ratio; }
// ---- a-1i: the carrier scan (m17hip_wide_scan): which bins of a source's row hold a carrier, and the frequency word of one.  band[k] is squelch_band(row,
// N, k, B) of every bin, `to` the block's open threshold squelch_level(open[s], J).  Bin k is a PEAK iff band[k] >= to — a true comparison: a NaN band is no
// peak — and no bin within circular distance X beats it; bin j beats k iff band[j] > band[k], or band[j] == band[k] && j < k (a NaN neighbour beats nothing).
// A local maximum, not a greedy pick: it does not depend on the order of evaluation, a monotone skirt is never a peak (its inner neighbour beats it), and two
// peaks are more than X bins apart.  3 <= X <= N / 4.
M17_HD bool scan_beats(float bj, uint32_t j, float bk, uint32_t k) { return bj > bk || (bj == bk && j < k); }
M17_HD bool scan_peak(const float* band, uint32_t N, uint32_t k, uint32_t X, float to)
{
    const float b = band[k];
    if (!(b >= to)) return false;
    for (uint32_t d = 1; d <= X; ++d) {
        const uint32_t lo = (k + N - d) & (N - 1), hi = (k + d) & (N - 1);
        if (scan_beats(band[lo], lo, b, k) || scan_beats(band[hi], hi, b, k)) return false;
    }
    return true;
}
// the circular distance of two bins of N
M17_HD uint32_t scan_distance(uint32_t a, uint32_t b, uint32_t N)
{
    const uint32_t d = (a - b) & (N - 1);
    return d < N - d ? d : N - d;
}
// The frequency word of the carrier whose peak is bin k: the bin's word plus the centroid of what the band's bins hold over the row's median `med`.
// w_d = max(row[(k + d) & (N - 1)] - med, +0) for d = -B .. B ascending (a NaN difference is +0); two chains from +0 in that order, sum w_d and sum d w_d;
// delta their quotient, or 0 where the sum of weights is not positive or the quotient is not finite (an inf bin).  delta is NOT clamped: on the edge of a
// plateau it exceeds half a bin, and that is the carrier's offset.  The word wraps.
M17_HD int32_t scan_fcw(const float* row, uint32_t N, uint32_t logn, uint32_t k, uint32_t B, float med)
{
    float sw = 0.0f, sd = 0.0f;
    for (uint32_t i = 0; i <= 2 * B; ++i) {
        const float v = row[(k + N - B + i) & (N - 1)] - med;
        const float wd = v > 0.0f ? v : 0.0f;
        sw = sw + wd;
        sd = sd + (float)((int32_t)i - (int32_t)B) * wd;
    }
    float delta = sw > 0.0f ? sd / sw : 0.0f;
    if (!(delta - delta == 0.0f)) delta = 0.0f;
    const int64_t off = (int64_t)__builtin_rintf(delta * (float)(1u << (32 - logn)));   // (|delta| <= B < N / 2: within int64 by far)
    return (int32_t)((k << (32 - logn)) + (uint32_t)off);
}
// the word a slot is assigned for peak k.  THE OPEN GUARANTEE: where the centroid's word lands in a bin whose band is below `to`, the bin-centre word of k
// serves, whose band is not: the squelch opens every slot in the block that assigns it.
M17_HD int32_t scan_assign(const float* row, const float* band, uint32_t N, uint32_t logn, uint32_t k, uint32_t B, float med, float to)
{
    const int32_t f = scan_fcw(row, N, logn, k, B, med);
    return band[squelch_bin(f, logn)] < to ? (int32_t)(k << (32 - logn)) : f;
}
// a block assigns nothing where it has no frame or the source's open level or median is not finite
M17_HD bool scan_idle(uint32_t J, float open_level, float med) { return J == 0 || !(open_level - open_level == 0.0f) || !(med - med == 0.0f); }
// the flags of a channel in the scan's fetch
constexpr uint32_t SCAN_SLOT = 1u, SCAN_ASSIGNED = 2u, SCAN_HELD = 4u;
constexpr uint32_t SCAN_MAX_SLOTS = 256;   // per source
// One source's block, stated as plainly as possible (the host form; wide_scan_kernel gives the same words).  slot[0 .. n) are the source's pool channels
// in ascending order, fcw[] and hold[] indexed by CHANNEL: fcw the words in front of the block, rewritten for the assigned slots; flags[] by channel gets
// SCAN_SLOT | SCAN_ASSIGNED | SCAN_HELD.  A slot is HELD iff squelch_step of its unchanged word has the open bit — what the squelch kernel will compute —
// and covers the peaks within X of its bin; the uncovered peaks, band descending then bin ascending, go to the slots that are not held in ascending
// order.  Returns the peaks left over.  `scratch` holds N floats (the bands).
M17_HD uint32_t scan_source(const float* row, uint32_t N, uint32_t logn, uint32_t J, uint32_t B, uint32_t X, float open_level, float close_level, float med,
                            uint32_t hang, const uint32_t* slot, uint32_t n, const uint32_t* hold, int32_t* fcw, uint32_t* flags, float* scratch)
{
    for (uint32_t i = 0; i < n; ++i) flags[slot[i]] = SCAN_SLOT;
    if (scan_idle(J, open_level, med)) return 0;
    const float to = squelch_level(open_level, J), tc = squelch_level(close_level, J);
    for (uint32_t k = 0; k < N; ++k) scratch[k] = squelch_band(row, N, k, B);
    for (uint32_t i = 0; i < n; ++i)
        if (squelch_step(hold[slot[i]], scratch[squelch_bin(fcw[slot[i]], logn)], to, tc, hang, J) & SQUELCH_OPEN) flags[slot[i]] |= SCAN_HELD;
    uint32_t missed = 0;
    for (uint32_t k = 0; k < N; ++k) {
        if (!scan_peak(scratch, N, k, X, to)) continue;
        bool covered = false;
        for (uint32_t i = 0; i < n && !covered; ++i)
            covered = (flags[slot[i]] & SCAN_HELD) && !(flags[slot[i]] & SCAN_ASSIGNED) && scan_distance(squelch_bin(fcw[slot[i]], logn), k, N) <= X;
        if (covered) continue;
        uint32_t rank = 0;   // the uncovered peaks that beat this one
        for (uint32_t j = 0; j < N; ++j) {
            if (j == k || !scan_beats(scratch[j], j, scratch[k], k) || !scan_peak(scratch, N, j, X, to)) continue;
            bool cov = false;
            for (uint32_t i = 0; i < n && !cov; ++i)
                cov = (flags[slot[i]] & SCAN_HELD) && !(flags[slot[i]] & SCAN_ASSIGNED) && scan_distance(squelch_bin(fcw[slot[i]], logn), j, N) <= X;
            rank += cov ? 0u : 1u;
        }
        uint32_t i = 0;
        for (uint32_t r = 0; i < n; ++i) {   // the rank-th slot that is not held
            if (flags[slot[i]] & SCAN_HELD) continue;
            if (r++ == rank) break;
        }
        if (i == n) { ++missed; continue; }
        fcw[slot[i]] = scan_assign(row, scratch, N, logn, k, B, med, to);
        flags[slot[i]] |= SCAN_ASSIGNED;
    }
    return missed;
}
// ---- a-1g: the time-resolved squelch (m17hip_wide_squelch_slots): the same four functions per SLOT of a block — a group of CHAN_SURVEY_GROUP frames of the
// block's spectrum, whose row is the spectrum's first-level sum — and the tuners skip per TILE of outputs.  A block of J frames has squelch_slots(J) slots;
// slot g holds squelch_slot_frames(J, g) frames and is stepped with squelch_step(h, band, level x frames, ..., hang, frames): hang counts slots.
M17_HD uint32_t squelch_slots(uint32_t J) { return J / CHAN_SURVEY_GROUP + (J % CHAN_SURVEY_GROUP ? 1u : 0u); }
M17_HD uint32_t squelch_slot_frames(uint32_t J, uint32_t g)   // (g < squelch_slots(J))
{
    return J - CHAN_SURVEY_GROUP * g < CHAN_SURVEY_GROUP ? J - CHAN_SURVEY_GROUP * g : CHAN_SURVEY_GROUP;
}
// the slot of block sample x (G >= 1 slots): the samples in front of the first frame belong to slot 0, those behind the last slot's span to slot G - 1
M17_HD uint32_t squelch_slot_of(uint32_t x, uint32_t first, uint32_t hop, uint32_t G)
{
    if (x < first) return 0u;
    const uint64_t g = (uint64_t)(x - first) / ((uint64_t)CHAN_SURVEY_GROUP * hop);
    return g < G - 1u ? (uint32_t)g : G - 1u;
}
// the block samples [a, e) under tile t of TO outputs of a block of T outputs made from W samples: floors of 64-bit products
M17_HD void squelch_tile_span(uint32_t t, uint32_t TO, uint32_t T, uint32_t W, uint32_t& a, uint32_t& e)
{
    const uint64_t n0 = (uint64_t)t * TO, n1 = n0 + TO < T ? n0 + TO : T;
    a = (uint32_t)(n0 * W / T);
    e = (uint32_t)(n1 * W / T);
}
// Whether the tile over block samples [a, e) is tuned: some slot from the one of a to the one of e - 1 plus `lead` (within the block) is open.  bits holds
// the slots' open flags, bit g & 31 of word g >> 5.  A block without a slot (G == 0) is all open.
M17_HD bool squelch_tile_open(const uint32_t* bits, uint32_t G, uint32_t first, uint32_t hop, uint32_t lead, uint32_t a, uint32_t e)
{
    if (G == 0u) return true;
    const uint32_t g0 = squelch_slot_of(a, first, hop, G);
    uint32_t g1 = squelch_slot_of(e > a ? e - 1u : a, first, hop, G);
    g1 = G - 1u - g1 < lead ? G - 1u : g1 + lead;
    for (uint32_t g = g0; g <= g1; ++g)
        if ((bits[g >> 5] >> (g & 31u)) & 1u) return true;
    return false;
}

// ---- t1: the wideband signal generator (m17hip_synth_wide, ABI 617): FM-modulate int16 basebands and put them at offsets into wide IQ streams -------
// No reference file: the reference's users attach an FM exciter behind its modulator.  Written here, once, so that the kernels and the host form give the
// same words.  Everything up to the oscillator's argument is INTEGER RING arithmetic (uint64 / uint32, wrapping), so any summation order, scan or tiling
// gives the same phase; nothing per wideband sample is carried.
// The generator's and the modulator's hash and noise (the modulator's kernels, csrc/m17_mod_kernels.hpp, use these): splitmix64, and zero-mean
// unit-variance noise for (stream, n) — the sum of 8 uniform u16 from two splitmix64 words, exact in double.
M17_HD uint64_t mod_splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
M17_HD double mod_unit_noise(uint64_t stream, uint64_t n)
{
    const uint64_t h = mod_splitmix64(stream ^ (n * 0xD1342543DE82EF95ull));
    const uint64_t g = mod_splitmix64(h);
    int64_t sum = 0;
    for (int k = 0; k < 4; ++k) { sum += (int64_t)((h >> (16 * k)) & 0xFFFF); sum += (int64_t)((g >> (16 * k)) & 0xFFFF); }
    const double inv_sigma = 1.0 / 53510.38419625641;
    return (double)(2 * sum - 8 * 65535) * 0.5 * inv_sigma;
}
// the noise stream of source s under the configuration's seed
M17_HD uint64_t wtx_noise_stream(uint64_t seed, uint32_t s) { return mod_splitmix64(seed ^ mod_splitmix64((uint64_t)s * 0x9E3779B97F4A7C15ull + 0x57494445ull)); }
// Block sample m of a source at 48000 P / Q: baseband sample k = (m Q) div P and the place r = (m Q) mod P inside it, from a 64-bit product.
M17_HD void wtx_index(uint32_t m, uint32_t P, uint32_t Q, uint32_t& k, uint32_t& r)
{
    const uint64_t t = (uint64_t)m * Q;
    k = (uint32_t)(t / P);
    r = (uint32_t)(t % P);
}
// A2[k + 1] - A2[k] = b[k - 1] + b[k]: twice the integral of the linearly interpolated baseband over baseband sample k (int16 values as int32)
M17_HD uint64_t wtx_step(int32_t bp, int32_t b) { return (uint64_t)(int64_t)(bp + b); }
// E(m) - A2[k] P^2 = 2 b[k-1] r P + (b[k] - b[k-1]) r^2, as r (2 b[k-1] P + (b[k] - b[k-1]) r): with P <= 2000 the inner sum is below 2^28 in magnitude
// (int32), its product with r < P a 32 x 32 -> 64 bit one
M17_HD uint64_t wtx_within(int32_t bp, int32_t b, uint32_t r, uint32_t P)
{
    const int32_t t = 2 * bp * (int32_t)P + (b - bp) * (int32_t)r;
    return (uint64_t)((int64_t)t * (int64_t)(int32_t)r);
}
// The oscillator's argument: the top 32 bits of theta = K E = base + K within, base = K P^2 A2[k], plus the carrier's fcw (uint32)M + phase0 — the
// count enters as in ddc_mix, so a receiver fed from count 0 sees a constant carrier phase.
M17_HD uint64_t wtx_theta(uint64_t base, uint64_t K, uint64_t within) { return base + K * within; }
M17_HD uint32_t wtx_phase(uint64_t theta, uint32_t fcw, uint32_t M, uint32_t phase0) { return (uint32_t)(theta >> 32) + fcw * M + phase0; }
// One channel's term onto the source's sum: nco, two plain multiplies, two plain adds.
M17_HD void wtx_add(float amplitude, uint32_t p, float& re, float& im)
{
    float c, s;
    nco(p, c, s);
    const float tr = amplitude * c, ti = amplitude * s;
    re = re + tr;
    im = im + ti;
}
// sigma > 0: noise from all 64 bits of the feed's sample index M, words 2 M and 2 M + 1 of the source's stream
M17_HD void wtx_noise(uint64_t ns, uint64_t M, float sigma, float& re, float& im)
{
    re = re + (float)(mod_unit_noise(ns, 2 * M) * (double)sigma);
    im = im + (float)(mod_unit_noise(ns, 2 * M + 1) * (double)sigma);
}
// The output formats: M17HIP_IQ_I16 rintf clamped to [-32768, 32767]; M17HIP_IQ_U8 rintf(fmaf(v, 1/128, 127.5)) clamped to [0, 255] (a NaN — only
// infinities of both signs can make one — takes the upper limit on both sides of the boundary).
M17_HD int16_t wtx_i16(float v)
{
    float r = __builtin_rintf(v);
    r = r < 32767.0f ? r : 32767.0f;
    r = r > -32768.0f ? r : -32768.0f;
    return (int16_t)(int32_t)r;
}
M17_HD uint8_t wtx_u8(float v)
{
    float r = __builtin_rintf(__builtin_fmaf(v, 0.0078125f, 127.5f));
    r = r < 255.0f ? r : 255.0f;
    r = r > 0.0f ? r : 0.0f;
    return (uint8_t)(int32_t)r;
}

// ---- a2: RRC matched filter taps (M17Demodulator.h:79-118): alpha = 0.5, 10 samples per symbol, 149 symmetric taps and
// a trailing 0.0; the double literals narrowed to float.  FIR order: FirFilter.h:36-40 (newest sample first, i = 0..149).
constexpr int RRC_TAPS = 150;
constexpr double RRC_HALF[75] = {
#include "rrc_half_taps.inc"
};
M17_HD constexpr float rrc_tap(int i) { return i >= 149 ? 0.0f : (float)(i <= 74 ? RRC_HALF[i] : RRC_HALF[148 - i]); }
// y = sum_{i=0}^{n-1} taps[i] * x[newest - i], accumulated in that order, multiply and add rounded separately.
template <typename GetSample>
M17_HD float fir_dot(const float* taps, int n, GetSample newest_minus)
{
    float acc = 0.0f;
    for (int i = 0; i < n; ++i) {
        const float p = newest_minus(i) * taps[i];
        acc = acc + p;
    }
    return acc;
}

// ---- a3: the correlator's limit filter: BaseIirFilter<float,3> (IirFilter.h:26-42) with Correlator.h:38-39 ----------
// h0 = in - a1*h1 - a2*h2 (two separate subtractions), out = 0 + b0*h0 + b1*h1 + b2*h2 (accumulated from 0 in that order).
struct LimitIir {
    static constexpr float b0 = 4.24433681e-05f, b1 = 8.48867363e-05f, b2 = 4.24433681e-05f;
    static constexpr float a1 = -1.98148851f, a2 = 0.98165828f;
};
M17_HD float iir_advance(float in_abs, float h1, float h2)
{
    float h0 = in_abs;
    h0 = h0 - LimitIir::a1 * h1;
    h0 = h0 - LimitIir::a2 * h2;
    return h0;
}
M17_HD float iir_output(float h0, float h1, float h2)
{
    float r = 0.0f;
    r = r + LimitIir::b0 * h0;
    r = r + LimitIir::b1 * h1;
    r = r + LimitIir::b2 * h2;
    return r;
}

// ---- a4: Correlator::correlate (Correlator.h:51-64) against the M17 sync words (M17Demodulator.h:154-157) -------------
// The words as sign masks (bit i set = symbol i is -3): (float)(-3) * x == -(3.0f * x) exactly and r + (-p) is what r - p
// computes, so a correlation is eight multiplies by 3.0f and eight adds, oldest symbol first.
constexpr uint32_t SYNC_NEG[4] = {0xAAu, 0xB0u, 0xF2u, 0x40u};   // preamble, LSF(/stream), packet(/BERT), EOT
constexpr int8_t SYNC_SYMBOLS[4][8] = {{+3, -3, +3, -3, +3, -3, +3, -3}, {+3, +3, +3, +3, -3, -3, +3, -3},
                                       {+3, -3, +3, +3, -3, -3, -3, -3}, {+3, +3, +3, +3, +3, +3, -3, +3}};
M17_HD float correlate_mask(uint32_t neg, const float (&r)[8])
{
    float v = 0.f;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 8; ++i) {
        const float p = 3.0f * r[i];
        const float q = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, p) ^ (((neg >> i) & 1u) << 31));
        v = v + q;
    }
    return v;
}
// general form: int8 coefficient * float sample, accumulated from 0 (what the reference's loop does for any sync_t)
M17_HD float correlate_symbols(const int8_t* sync, const float (&r)[8])
{
    float v = 0.f;
    for (int i = 0; i < 8; ++i) v = v + (float)sync[i] * r[i];
    return v;
}

// ---- a6: Correlator::outer_symbol_levels (Correlator.h:81-114) -------------------------------------------------------
// get(i) = buffer_[i], i = sample_index, sample_index + 10, ... < 80.  `avg = max + min / 2.` (sic, in double).
template <typename Get>
M17_HD void outer_symbol_levels(Get get, uint32_t sample_index, float& mn, float& mx)
{
    float min_sum = 0.f, max_sum = 0.f;
    uint32_t min_count = 0, max_count = 0;
    float lo = get(sample_index), hi = lo;
    for (uint32_t i = sample_index; i < 80u; i += 10u) {
        const float v = get(i);
        lo = (v < lo) ? v : lo;   // std::min(lo, v)
        hi = (hi < v) ? v : hi;   // std::max(hi, v)
    }
    const float avg = (float)((double)hi + (double)lo / 2.);
    for (uint32_t i = sample_index; i < 80u; i += 10u) {
        const float v = get(i);
        const bool high = v > avg, low = v < avg;
        max_sum = max_sum + v * (high ? 1.f : 0.f);
        min_sum = min_sum + v * (low ? 1.f : 0.f);
        max_count += high; min_count += low;
    }
    mn = min_count > 0 ? min_sum / (float)min_count : lo;
    mx = max_count > 0 ? max_sum / (float)max_count : hi;
}

// ---- a7: one bin of NSlidingDFT::operator() (SlidingDFT.h:118-132): X = (X + delta) * c, libstdc++ complex multiply ------
// (a + bi)(c + di) = (ac - bd) + (ad + bc)i in fp32, no FMA; delta is real.
M17_HD void sdft_step(float& re, float& im, float delta, float cr, float ci)
{
    const float a = re + delta, b = im;
    const float ac = a * cr, bd = b * ci, ad = a * ci, bc = b * cr;
    re = ac - bd;
    im = ad + bc;
}
M17_HD float complex_norm(float re, float im) { return re * re + im * im; }   // std::norm
// ---- a8: DataCarrierDetect::update (DataCarrierDetect.h:63-69), level EMA in double ---------------------------------------
M17_HD float dcd_level(float level, float l1, float l2) { return (float)((double)level * 0.8 + 0.2 * (double)(l1 / l2)); }

// ---- a9/a10: the 2-state Kalman filter of KalmanFilter.h:18-108 (F = [[1,dt],[0,1]], H = [1 0], R = 0.5, Q :26) ---------
// blaze (the reference's linear-algebra dependency) is absent from the reference tree; `S` and `K` are lazy blaze
// expressions there (`auto`), so the association / rounding of `x += K*y` and `P = P - K*H*P` follows blaze's restructuring
// operators.  The order is a switch, the same in the oracle and in the C ABI (m17hip_set_kalman_order):
//   bit 0: x += double(fl32(P(:,0)*y)) * invS      [(A*s)*v -> (A*v)*s]   else  x += (double(P(:,0))*invS) * double(y)
//   bit 1: P -= double(fl32(P(i,0)*P(0,j))) * invS [(A*s)*B -> (A*B)*s]   else  P -= ((double(P(i,0))*invS) * double(P(0,j)))
//   bit 2: F*(P*F^T) instead of (F*P)*F^T
constexpr uint32_t KALMAN_ORDER_DEFAULT = 3;
struct Kalman2 {
    float x0, x1, p00, p01, p10, p11;
};
M17_HD void kalman2_reset(Kalman2& k, float z)
{
    k.x0 = z; k.x1 = 0.f;
    k.p00 = 4.f; k.p01 = 0.f; k.p10 = 0.f; k.p11 = (float)0.00000025;
}
// wrap != 0: KalmanFilter<float,SPS> (index filter, modulo SPS, :41-65); 0: SymbolKalmanFilter (:91-107).
// The order is a template parameter so that each variant is straight-line code (the kernels dispatch once per update).
//
// The update is written as its two independent halves.  The COVARIANCE half (P = F P F^T + Q; S = H P H^T + R; P = P - K H P) never
// reads x or z: it leaves the covariance after the predict step and 1 / S — all the state half needs — in a Kalman2Gain.  The STATE
// half (x = F x; y = z - H x; x += K y) reads that gain and nothing of P.  kalman2_update_as = the one after the other, operation for
// operation what the single function of rounds 1-3 did.
struct Kalman2Gain {
    float p00, p01, p10, p11;   // P after the predict step
    double invS;
};
template <uint32_t order>
M17_HD void kalman2_cov_step(Kalman2& k, uint32_t dt_u, Kalman2Gain& g)
{
    const float F00 = 1.f, F01 = (float)dt_u, F10 = 0.f, F11 = 1.f;
    const float Q00 = (float)6.25e-13, Q01 = (float)1.25e-12, Q10 = (float)1.25e-12, Q11 = (float)2.50e-12;
    float B00, B01, B10, B11;
    if (!(order & 4u)) {
        const float A00 = F00 * k.p00 + F01 * k.p10, A01 = F00 * k.p01 + F01 * k.p11;
        const float A10 = F10 * k.p00 + F11 * k.p10, A11 = F10 * k.p01 + F11 * k.p11;
        B00 = A00 * F00 + A01 * F01; B01 = A00 * F10 + A01 * F11;
        B10 = A10 * F00 + A11 * F01; B11 = A10 * F10 + A11 * F11;
    } else {
        const float A00 = k.p00 * F00 + k.p01 * F01, A01 = k.p00 * F10 + k.p01 * F11;
        const float A10 = k.p10 * F00 + k.p11 * F01, A11 = k.p10 * F10 + k.p11 * F11;
        B00 = F00 * A00 + F01 * A10; B01 = F00 * A01 + F01 * A11;
        B10 = F10 * A00 + F11 * A10; B11 = F10 * A01 + F11 * A11;
    }
    k.p00 = B00 + Q00; k.p01 = B01 + Q01; k.p10 = B10 + Q10; k.p11 = B11 + Q11;
    const float hp0 = 1.f * k.p00 + 0.f * k.p10;
    const float hp1 = 1.f * k.p01 + 0.f * k.p11;
    const float S = (hp0 * 1.f + hp1 * 0.f) + 0.5f;
    const float ph0 = k.p00 * 1.f + k.p01 * 0.f;
    const float ph1 = k.p10 * 1.f + k.p11 * 0.f;
    const double invS = 1.0 / (double)S;
    g.p00 = k.p00; g.p01 = k.p01; g.p10 = k.p10; g.p11 = k.p11; g.invS = invS;
    float n00, n01, n10, n11;
    if (order & 2u) {
        const float G00 = ph0 * 1.f, G01 = ph0 * 0.f, G10 = ph1 * 1.f, G11 = ph1 * 0.f;
        const float T00 = G00 * k.p00 + G01 * k.p10, T01 = G00 * k.p01 + G01 * k.p11;
        const float T10 = G10 * k.p00 + G11 * k.p10, T11 = G10 * k.p01 + G11 * k.p11;
        n00 = (float)((double)k.p00 - (double)T00 * invS);
        n01 = (float)((double)k.p01 - (double)T01 * invS);
        n10 = (float)((double)k.p10 - (double)T10 * invS);
        n11 = (float)((double)k.p11 - (double)T11 * invS);
    } else {
        const double K0 = (double)ph0 * invS, K1 = (double)ph1 * invS;
        const double KH00 = K0 * 1.0, KH01 = K0 * 0.0, KH10 = K1 * 1.0, KH11 = K1 * 0.0;
        n00 = (float)((double)k.p00 - (KH00 * (double)k.p00 + KH01 * (double)k.p10));
        n01 = (float)((double)k.p01 - (KH00 * (double)k.p01 + KH01 * (double)k.p11));
        n10 = (float)((double)k.p10 - (KH10 * (double)k.p00 + KH11 * (double)k.p10));
        n11 = (float)((double)k.p11 - (KH10 * (double)k.p01 + KH11 * (double)k.p11));
    }
    k.p00 = n00; k.p01 = n01; k.p10 = n10; k.p11 = n11;
}
template <uint32_t order>
M17_HD void kalman2_state_step(float& x0, float& x1, float z, uint32_t dt_u, int wrap, const Kalman2Gain& g)
{
    const float F00 = 1.f, F01 = (float)dt_u, F10 = 0.f, F11 = 1.f;
    const float nx0 = F00 * x0 + F01 * x1;
    const float nx1 = F10 * x0 + F11 * x1;
    x0 = nx0; x1 = nx1;
    const float fw = (float)wrap;
    if (wrap) {
        if ((double)(z - x0) < ((double)wrap / -2.0)) z += fw;
        else if ((double)(z - x0) > ((double)wrap / 2.0)) z -= fw;
    }
    const float y = z - (1.f * x0 + 0.f * x1);
    if (order & 1u) {
        const float hy0 = 1.f * y, hy1 = 0.f * y;
        const float t0 = g.p00 * hy0 + g.p01 * hy1;
        const float t1 = g.p10 * hy0 + g.p11 * hy1;
        x0 = (float)((double)x0 + (double)t0 * g.invS);
        x1 = (float)((double)x1 + (double)t1 * g.invS);
    } else {
        const float ph0 = g.p00 * 1.f + g.p01 * 0.f;
        const float ph1 = g.p10 * 1.f + g.p11 * 0.f;
        const double K0 = (double)ph0 * g.invS, K1 = (double)ph1 * g.invS;
        x0 = (float)((double)x0 + K0 * (double)y);
        x1 = (float)((double)x1 + K1 * (double)y);
    }
    if (wrap) {
        while (x0 >= fw) x0 -= fw;
        while (x0 < 0.f) x0 += fw;
    }
}
template <uint32_t order>
M17_HD void kalman2_update_as(Kalman2& k, float z, uint32_t dt_u, int wrap)
{
    Kalman2Gain g;
    kalman2_cov_step<order>(k, dt_u, g);
    kalman2_state_step<order>(k.x0, k.x1, z, dt_u, wrap, g);
}
M17_HD void kalman2_update(Kalman2& k, float z, uint32_t dt_u, int wrap, uint32_t order)
{
    switch (order & 7u) {
    case 0: kalman2_update_as<0>(k, z, dt_u, wrap); break;
    case 1: kalman2_update_as<1>(k, z, dt_u, wrap); break;
    case 2: kalman2_update_as<2>(k, z, dt_u, wrap); break;
    case 3: kalman2_update_as<3>(k, z, dt_u, wrap); break;
    case 4: kalman2_update_as<4>(k, z, dt_u, wrap); break;
    case 5: kalman2_update_as<5>(k, z, dt_u, wrap); break;
    case 6: kalman2_update_as<6>(k, z, dt_u, wrap); break;
    default: kalman2_update_as<7>(k, z, dt_u, wrap); break;
    }
}

// ---- a10: the gain SCHEDULE of FreqDevEstimator's two level filters (FreqDevEstimator.h:31-48: both are updated with dt = 192 and
// reset together, KalmanFilter.h:91-107).  Their covariance is therefore a function of the number of updates since the reset alone,
// the same for both, and in fp32 it reaches a FIXED POINT after 558 / 559 updates under every evaluation order (checked where the
// table is built and in tests/cxx/mirror_check.cpp): entry n = the gain of update n + 1 after a reset, entry LEVEL_SCHED_LAST for
// every later one.  A filter is then (x0, x1) plus the shared count: an update is kalman2_state_step with a table entry — no
// covariance arithmetic, no f64 division.
constexpr uint32_t LEVEL_DT = 192;
constexpr int LEVEL_SCHED_N = 576, LEVEL_SCHED_LAST = LEVEL_SCHED_N - 1;
template <uint32_t order>
inline bool level_schedule_as(Kalman2Gain* tab)   // [LEVEL_SCHED_N]; false if the covariance has not settled (cannot happen: see above)
{
    Kalman2 k;
    kalman2_reset(k, 0.f);
    for (int n = 0; n < LEVEL_SCHED_N; ++n) kalman2_cov_step<order>(k, LEVEL_DT, tab[n]);
    Kalman2 k2 = k;
    Kalman2Gain g;
    kalman2_cov_step<order>(k2, LEVEL_DT, g);
    const Kalman2Gain& l = tab[LEVEL_SCHED_LAST];
    return k2.p00 == k.p00 && k2.p01 == k.p01 && k2.p10 == k.p10 && k2.p11 == k.p11 && g.p00 == l.p00 && g.p01 == l.p01 && g.p10 == l.p10 &&
           g.p11 == l.p11 && g.invS == l.invS;
}
inline bool level_schedule(Kalman2Gain* tab, uint32_t order)
{
    switch (order & 7u) {
    case 0: return level_schedule_as<0>(tab);
    case 1: return level_schedule_as<1>(tab);
    case 2: return level_schedule_as<2>(tab);
    case 3: return level_schedule_as<3>(tab);
    case 4: return level_schedule_as<4>(tab);
    case 5: return level_schedule_as<5>(tab);
    case 6: return level_schedule_as<6>(tab);
    default: return level_schedule_as<7>(tab);
    }
}
// one level filter, scheduled: (x0, x1) after the update that uses entry g; `order` only selects how x += K y is associated (bit 0)
M17_HD void level_update(float& x0, float& x1, float z, const Kalman2Gain& g, uint32_t order)
{
    if (order & 1u) kalman2_state_step<1>(x0, x1, z, LEVEL_DT, 0, g);
    else kalman2_state_step<0>(x0, x1, z, LEVEL_DT, 0, g);
}

// ClockRecovery (ClockRecovery.h:54-88): int8 wrap of the rounded estimate into 0..9
M17_HD int32_t wrap10(int32_t v)
{
    v = (int32_t)(int8_t)v;
    v = v < 0 ? v + 10 : v;
    v = v >= 10 ? v - 10 : v;
    return (int32_t)(int8_t)v;
}
// ClockRecovery::update() (:76-88) as a pure function of (sample_estimate_, clock_estimate_, count_):
// fmod(double(float v), 10) is exact; for |v| < 1e12 it is v - 10*trunc(v/10) with one fma (the quotient estimate
// trunc(v * 0.1) is within one of the true one and the +-10 correction below makes up for it), else the library fmod.
M17_HD int32_t clock_predict(float sample_est, float clock_est, uint32_t count)
{
    const float v = sample_est + clock_est * (float)count;
    const double dv = (double)v;
    double csw;
    if (__builtin_fabs(dv) < 1.0e12) {
        const double q = __builtin_trunc(dv * 0.1);
        csw = __builtin_fma(-q, 10.0, dv);
        if (dv >= 0.0) { if (csw < 0.0) csw += 10.0; else if (csw >= 10.0) csw -= 10.0; }
        else { if (csw > 0.0) csw -= 10.0; else if (csw <= -10.0) csw += 10.0; }
    } else {
        csw = __builtin_fmod(dv, 10.0);
    }
    if (csw < 0.) csw += 10;
    else if (csw >= 10) csw -= 10;
    return wrap10((int32_t)__builtin_round(csw));
}
// The same question as a predicate, for the callers that only need "does the update leave sample_index at S?" (K5 checks every
// anti-phase sample of a chunk at once): with v = sample_estimate_ + clock_estimate_ * count_ as the float the reference forms
// (:78), and v in [-10, 19.5), fmod / the +-10 wrap / round-half-away reduce to exact interval tests on v itself:
// clock_predict == S  <=>  v, v + 10 or v - 10 lies in [S - 0.5, S + 0.5)   (S = 0 picks up [9.5, 10) through the third one).
// Outside that range (or NaN) clock_predict_near() is false and the caller has to evaluate clock_predict().
M17_HD float clock_predict_arg(float sample_est, float clock_est, uint32_t count) { return sample_est + clock_est * (float)count; }
M17_HD bool clock_predict_near(float v) { return v >= -10.f && v < 19.5f; }
M17_HD bool clock_predict_equals(float v, int32_t S)
{
    const float lo = (float)S - 0.5f, hi = (float)S + 0.5f;   // exact: S is 0..9
    return (v >= lo && v < hi) || (v >= lo - 10.f && v < hi - 10.f) || (v >= lo + 10.f && v < hi + 10.f);
}
// ClockRecovery::update(uint8_t) (:54-67): the sample index of a fresh filter estimate
M17_HD int32_t clock_index_of(float sample_est) { return wrap10((int32_t)__builtin_round((double)sample_est)); }

// FreqDevEstimator (FreqDevEstimator.h:31-48): offset and inverse deviation from the two smoothed levels
M17_HD float freqdev_offset(float mx0, float mn0) { return (float)((double)(mx0 + mn0) / 2.); }
M17_HD float freqdev_idev(float mx0, float mn0) { return (float)(6.0 / (double)(mx0 - mn0)); }

// ---- a11: SymbolEvm::update (SymbolEvm.h:31-51): distance to the nearest of {-3,-1,1,3} -----------------------------------
M17_HD float evm_error(float sample)
{
    if (sample > 2.f) return sample - 3.f;
    if (sample > 0.f) return sample - 1.f;
    if (sample > -2.f) return sample + 1.f;
    return sample + 3.f;
}
constexpr float EVM_ALPHA = (float)(1.0 / 184);   // RunningStandardDeviation<float,184>::alpha (StandardDeviation.h:60-72)
M17_HD float evm_capture(float S, float err)
{
    S = S - S * EVM_ALPHA;
    S = S + (err * err) * EVM_ALPHA;
    return S;
}

// ---- a12: llr<float,4> (Util.h:63-104,128-145) ------------------------------------------------------------------------------
// 43 table rows whose edges are ACCUMULATED in fp32 (k = -3 + 1/7; k += 1/7), lookup = first edge >= the clamped sample.
constexpr int LLR_ROWS = 43;
M17_HD void llr_edges(float* e43)
{
    const float inc = (float)(1.0 / (double)7.0f);
    float k = (float)(-3.0 + (double)inc);
    for (int n = 0; n < LLR_ROWS; ++n) { e43[n] = k; k = k + inc; }
}
// the (int8, int8) pair of row n: i falls 7..1,-1..-7 over rows 14..27, j falls over rows 0..13 and rises over 28..41
M17_HD uint32_t llr_pair_of_row(int n)
{
    int li, lj;
    if (n <= 14) { li = 7; lj = (n <= 6) ? 7 - n : ((n <= 13) ? 6 - n : -7); }
    else if (n <= 28) { lj = -7; li = (n <= 20) ? 21 - n : ((n <= 27) ? 20 - n : -7); }
    else { li = -7; lj = (n <= 34) ? n - 35 : ((n <= 41) ? n - 34 : 7); }
    return ((uint32_t)(uint8_t)(int8_t)li) | (((uint32_t)(uint8_t)(int8_t)lj) << 8);
}
// row index = std::lower_bound over the edges: guessed arithmetically, corrected against the exact edges (the guess is
// within one row of the answer because the edges are strictly increasing and within 1e-6 of -3 + (n+1)/7)
M17_HD int llr_row(float sample, const float* edges)
{
    const float cl = __builtin_fminf(3.0f, __builtin_fmaxf(-3.0f, sample));
    int n = (int)__builtin_ceilf((cl + 3.0f) * 7.0f) - 1;
    n = n < 1 ? 1 : (n > 41 ? 41 : n);
    const float e0 = edges[n - 1], e1 = edges[n], e2 = edges[n + 1];
    if (e0 >= cl) n = n - 1;
    else if (e1 >= cl) { /* the guess is the row */ }
    else if (e2 >= cl) n = n + 1;
    else n = n + 2;
    return n;
}
M17_HD uint32_t llr_slice(float sample, const float* edges) { return llr_pair_of_row(llr_row(sample, edges)); }

// ---- a17: Viterbi<Trellis<4,2>,4> (Viterbi.h:94-240) scalar pieces -----------------------------------------------------------
template <int LIMIT = 7>
M17_HD uint32_t viterbi_cost_of(int32_t min_metric) { return (uint32_t)(int64_t)__builtin_roundf((float)min_metric / (float)LIMIT); }   // :223

}  // namespace core
}  // namespace mobilinkd
