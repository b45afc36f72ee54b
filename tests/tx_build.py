"""A transmission with caller-supplied content, built on the CPU (TEST INFRASTRUCTURE ONLY): what m17hip_synth_tx_i16 must write, from the same
three inputs (kind, the 30-byte LSF, the 32-byte rows) — frame bits from the oracle's primitives (convolutional encoder, puncture, interleaver,
decorrelator, Golay), sync words, preamble and EOT as apps/m17-mod.cpp:264-504, 509-564 frame them, pulse shaping in double with the taps in
ascending order, x 7168, truncation to int16 (m17-mod.cpp:204-224), then gain, DC offset and noise as the test generator applies them.  Everything
outside the burst (lead-in, gaps, tail, the +-1 dither) is taken from oracle_lib.generate() with the same parameters, whose surroundings depend on
the burst's length only.  Slow and obvious on purpose: one frame at a time, no tables."""
import os
import re

import numpy as np

import oracle_lib as ol

BERT, STREAM, PACKET = 0, 1, 2
SYNC = {"lsf": (0x55, 0xF7), "stream": (0xFF, 0x5D), "packet": (0x75, 0xFF), "bert": (0xDF, 0x55), "eot": (0x55, 0x5D)}
DIBIT = (+1, +3, -1, -3)                                  # m17-mod.cpp:164-174
M64 = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def channel_seed(seed, cc):
    """The seed of global channel cc of a batch (include/m17hip.h, m17hip_synth_i16)."""
    return seed ^ splitmix64((cc * 0x9E3779B97F4A7C15 + 1) & M64)


def taps_double():
    """The 150 shaping taps in double: the 75 literals the oracle is compiled from, mirrored, the last one 0."""
    text = open(os.path.join(ol.ORACLE_DIR, "rrc_half_taps.inc")).read()
    half = [float(t) for t in re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S).split(",") if t.strip()]
    assert len(half) == 75
    return np.array([0.0 if i == 149 else (half[i] if i <= 74 else half[148 - i]) for i in range(150)], dtype=np.float64)


def bits_of(data, nbits):
    return np.unpackbits(np.frombuffer(bytes(data), dtype=np.uint8))[:nbits]


def finish(f368):
    f = ol.frame_op("interleave", np.asarray(f368, dtype=np.int8))
    return ol.frame_op("randomize_bits", f)


def coded(data, nbits, which, kept):
    """nbits message bits -> rate 1/2 with 4 flush bits -> puncture matrix `which` -> `kept` bits."""
    p = ol.puncture(ol.conv_encode(bits_of(data, nbits)), kept, which)
    assert p.size == kept
    return p


def lsf_frame(lsf30):
    return finish(coded(lsf30, 240, 1, 368))


def lich_bits(lsf30, n):
    seg = bytes(lsf30)[5 * n:5 * n + 5]
    words = ((seg[0] << 4) | (seg[1] >> 4), ((seg[1] & 15) << 8) | seg[2], (seg[3] << 4) | (seg[4] >> 4), ((seg[4] & 15) << 8) | (n << 5))
    out = []
    for w in words:
        e = ol.golay_encode24(w)
        out += [(e >> (23 - i)) & 1 for i in range(24)]
    return np.array(out, dtype=np.int8)


def stream_frame(lsf30, i, row):
    return finish(np.concatenate([lich_bits(lsf30, i % 6), coded(bytes(row)[:18], 144, 2, 272)]))


def packet_frame(row):
    return finish(coded(bytes(row)[:26], 206, 3, 368))


def bert_frame(row):
    return finish(coded(bytes(row)[:25], 197, 2, 368))


def byte_symbols(bs):
    return [DIBIT[(b >> (6 - 2 * k)) & 3] for b in bs for k in range(4)]


def frame_symbols(sync, f368):
    f = np.asarray(f368, dtype=np.int64)
    return byte_symbols(SYNC[sync]) + [DIBIT[int(2 * f[i] + f[i + 1])] for i in range(0, 368, 2)]


def symbols(kind, lsf30, rows, n_preamble=0):
    """The symbol stream of one transmission (n_preamble 0: two preambles for BERT, else one, as m17-mod sends them)."""
    sym = byte_symbols([0x77] * 48) * (n_preamble if n_preamble > 0 else (2 if kind == BERT else 1))
    if kind == BERT:
        for row in rows:
            sym += frame_symbols("bert", bert_frame(row))
        return np.array(sym, dtype=np.int8)
    sym += frame_symbols("lsf", lsf_frame(lsf30))
    for i, row in enumerate(rows):
        sym += frame_symbols("stream", stream_frame(lsf30, i, row)) if kind == STREAM else frame_symbols("packet", packet_frame(row))
    sym += byte_symbols(SYNC["eot"]) + [0] * 40
    return np.array(sym, dtype=np.int8)


def shape(sym, invert):
    """y[n] = sum_i taps[i] * u[n - i], u = the symbols at multiples of 10, i ascending; x 7168; truncated to int16."""
    taps, nsym = taps_double(), sym.size
    n = np.arange(nsym * 10 + 150)
    acc = np.zeros(n.size, dtype=np.float64)
    s = sym.astype(np.float64)
    for j in range(15):
        i = n % 10 + 10 * j
        k = (n - i) // 10
        ok = (i <= n) & (k < nsym)
        acc = acc + np.where(ok, s[np.clip(k, 0, nsym - 1)] * taps[i], 0.0)
    return np.trunc(acc * 7168.0 * (-1.0 if invert else 1.0)).astype(np.int16)


def unit_noise(stream, n):
    """The generator's zero-mean unit-variance noise of samples n (an array) of noise stream `stream`: eight uniform u16 summed, exact in double."""
    def mix(x):                                           # splitmix64 on uint64 arrays (numpy wraps)
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))
    h = mix(np.uint64(stream) ^ (n.astype(np.uint64) * np.uint64(0xD1342543DE82EF95)))
    g = mix(h)
    total = np.zeros(n.size, dtype=np.int64)
    for k in range(4):
        total += ((h >> np.uint64(16 * k)) & np.uint64(0xFFFF)).astype(np.int64) + ((g >> np.uint64(16 * k)) & np.uint64(0xFFFF)).astype(np.int64)
    return (2 * total - 8 * 65535).astype(np.float64) * 0.5 * (1.0 / 53510.38419625641)


def burst(p, kind, lsf30, rows):
    """The int16 waveform of p.total samples: parameters `p` (an oracle_lib.GenParams whose seed is the channel's own), content as given."""
    assert p.total > 0
    q = ol.gen_params(seed=p.seed, kind=kind, n_frames=len(rows), lead_in=p.lead_in, phase=p.phase, tail=p.tail, total=p.total, invert=p.invert,
                      lead_sigma=p.lead_sigma, noise_sigma=p.noise_sigma, dc_offset=p.dc_offset, gain=p.gain, tail_sigma=p.tail_sigma,
                      n_preamble=p.n_preamble)
    out = ol.generate(q)[:p.total].copy()                 # the surroundings: a generator burst of the same length
    shaped = shape(symbols(kind, lsf30, rows, p.n_preamble), p.invert)
    phase = p.phase if p.phase >= 0 else splitmix64(p.seed ^ 0x1234567) % 10
    start = p.lead_in + phase
    m = min(shaped.size, max(0, p.total - start))
    n = start + np.arange(m)
    v = shaped[:m].astype(np.float64) * p.gain + p.dc_offset + unit_noise(splitmix64(p.seed ^ 0x5EED), n) * p.noise_sigma
    out[start:start + m] = np.clip(np.rint(v), -32768.0, 32767.0).astype(np.int16)
    return out


def batch(base, transmissions, samples, chan0=0):
    """[channels][samples]: transmission c = (kind, lsf_or_None, rows) under `base` with the seed of global channel chan0 + c."""
    out = np.zeros((len(transmissions), samples), dtype=np.int16)
    for c, (kind, lsf30, rows) in enumerate(transmissions):
        p = ol.GenParams.from_buffer_copy(bytes(base))
        p.seed, p.total = channel_seed(base.seed, chan0 + c), samples
        out[c] = burst(p, kind, lsf30, rows)
    return out


def from_truth(gen_kind, truth, n_frames):
    """The generator's truth (oracle_lib.generate(..., with_truth=True)) as a transmission; generator kinds 2 and 4 are both packets."""
    rows = [bytes(truth["payloads"][i]) for i in range(n_frames)]
    return (BERT, None, rows) if gen_kind == 0 else (STREAM if gen_kind == 1 else PACKET, bytes(truth["lsf"]), rows)
