"""Inputs and a plain restatement for the tests of the frame decoder's device forms (TEST INFRASTRUCTURE ONLY: tests/test_decode_forms.py,
tests/test_gpu_decode_forms.py; m17hip_decode_sequences, include/m17hip.h).

The device has Viterbi<Trellis<4,2>,4>::decode three times: lane per frame with 32-bit metrics, sixteen lanes as sixteen states, and lane per
frame with packed 16-bit metrics and a sentinel of 20000.  Whole-chain runs reach the last two only on the LLRs a synthesised signal produces.
Here the LLRs are chosen: frames on which every comparison ties, on which several end states share the minimum, on which the path metric is as
large as it gets; sequences whose deferred records lie beyond slot 512 and on both sides of it; a record store that is full.

Yardstick: oracle_lib (ol.decode_frame stepped frame by frame).  `viterbi_np` restates the trellis once more, in numpy and int64, so that the
premises the inputs are built for (ties, shared minima, the largest metric) can be read off something that is not the code under test."""
import functools

import numpy as np

import m17hip
import oracle_lib as ol
import tx_build as tb

INT_MAX_HALF = (2 ** 31 - 1) // 2
METRIC_BOUND = 244 * 28            # at most 244 steps, a step adds at most 2 x 14 to the surviving metric
SHAPES = {0: (488, 240), 1: (296, 144), 2: (420, 206), 3: (402, 197)}   # kind: LSF, stream, packet, BERT -> (soft bits, message bits)
_PARITY = np.array([bin(v).count("1") & 1 for v in range(32)])
# cost_[i][j] of Viterbi.h:116-126 for the states i < 8: +-7 by the encoder's output bit j (polynomials 031 and 027) from memory i << 1
_K = np.array([[(2 * _PARITY[p & (i << 1)] - 1) * 7 for p in (0o31, 0o27)] for i in range(8)], dtype=np.int64)


def viterbi_np(soft, out_bits):
    """Viterbi.h:162-239 on N frames at once: soft [N][IN] (0 = erased).  int64 metrics, INT_MAX // 2 for unreachable states, the strict
    m0 > m2 decision, the first minimum scanning 0 to 15, cost = round(min / 7.f).  Returns a dict of arrays over the N frames: bits [N][OUT],
    cost, max_metric (the largest finite metric over all states and steps), ties / compares (add-compare-selects between two REACHABLE
    candidates, and how many of them tied: a comparison with an unreachable candidate is decided by the sentinel, not by the LLRs — the first four
    steps have some whatever the input), n_min (states that share the final minimum)."""
    s = np.atleast_2d(np.asarray(soft, dtype=np.int64))
    N, IN = s.shape
    steps = IN // 2
    m = np.full((N, 16), INT_MAX_HALF, dtype=np.int64)
    m[:, 0] = 0
    hist = np.zeros((steps, N, 16), dtype=bool)
    max_metric, ties, compares = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros(N, np.int64)
    for h in range(steps):
        s0, s1 = s[:, 2 * h, None], s[:, 2 * h + 1, None]
        c0 = np.where(s0 != 0, np.abs(_K[:, 0] - s0), 0) + np.where(s1 != 0, np.abs(_K[:, 1] - s1), 0)
        c1 = np.where(s0 != 0, np.abs(_K[:, 0] + s0), 0) + np.where(s1 != 0, np.abs(_K[:, 1] + s1), 0)
        lo, hi = m[:, :8], m[:, 8:]
        m0, m1, m2, m3 = lo + c0, lo + c1, hi + c1, hi + c0
        d0, d1 = m0 > m2, m1 > m3
        both = ((lo < INT_MAX_HALF) & (hi < INT_MAX_HALF)).sum(axis=1)
        compares += 2 * both
        ties += (((m0 == m2) & (lo < INT_MAX_HALF) & (hi < INT_MAX_HALF)).sum(axis=1) + ((m1 == m3) & (lo < INT_MAX_HALF) & (hi < INT_MAX_HALF)).sum(axis=1))
        m = np.empty_like(m)
        m[:, 0::2], m[:, 1::2] = np.where(d0, m2, m0), np.where(d1, m3, m1)
        hist[h, :, 0::2], hist[h, :, 1::2] = d0, d1
        max_metric = np.maximum(max_metric, np.where(m < INT_MAX_HALF, m, 0).max(axis=1))
    best = m.argmin(axis=1)                      # (the first of equal minima)
    low = m.min(axis=1)
    cost = np.floor((low.astype(np.float32) / np.float32(7)).astype(np.float64) + 0.5).astype(np.int64)   # std::round: no quotient is a half (2 min = 7 k has no odd k)
    bits = np.zeros((N, out_bits), dtype=np.uint8)
    state, o, index = best.copy(), out_bits, steps
    for hi_ in range(steps - 1, -1, -1):         # chainback :226-236
        if o == 0:
            break
        v = hist[hi_, np.arange(N), state]
        if index <= out_bits:
            o -= 1
            bits[:, o] = state & 1
        index -= 1
        state = (state >> 1) + 8 * v
    return dict(bits=bits, cost=cost, max_metric=max_metric, ties=ties, compares=compares, n_min=(m == low[:, None]).sum(axis=1))


def viterbi_input(sync_type, state, llr368, dep401):
    """The depunctured soft bits the frame decoder hands its Viterbi decoder for this frame, and the kind — or None where it decodes nothing
    (a LICH, a sync word the state does not expect).  M17FrameDecoder.h:353-392 with oracle_lib's frame operations."""
    buf = ol.frame_op("deinterleave", ol.frame_op("derandomize", llr368))
    if sync_type == 0:
        return 0, ol.depuncture(buf, 488, 1)
    if sync_type == 1 and state == 1:
        return 1, ol.depuncture(buf[96:], 296, 2)
    if sync_type == 2 and state in (2, 3):
        return 2, ol.depuncture(buf, 420, 3)
    if sync_type == 3:
        pre = np.zeros(402, dtype=np.int8)
        pre[401] = dep401                        # position 401 is not written by this layout: it keeps what the frame before left there
        return 3, ol.depuncture(buf, 402, 2, prefill=pre)
    return None


class Sequence:
    """C channels x F frames, the decoder state each channel starts from, a record store of rec_cap slots; .expect() steps the oracle."""

    def __init__(self, name, llr, st, rec_cap, state=None, dep401=None):
        self.name = name
        self.llr = np.ascontiguousarray(llr, dtype=np.int8)
        self.st = np.ascontiguousarray(st, dtype=np.uint8)
        self.C, self.F = self.st.shape
        assert self.llr.shape == (self.C, self.F, 368) and np.abs(self.llr.astype(np.int16)).max() <= 7
        self.rec_cap = rec_cap
        self.state = np.zeros(self.C, np.uint8) if state is None else np.asarray(state, np.uint8)
        self.dep401 = np.zeros(self.C, np.int8) if dep401 is None else np.asarray(dep401, np.int8)
        self._exp = None

    def expect(self):
        """ol.decode_frame stepped frame by frame, computed once: per channel the records (all of them, `sample_pos` = the frame that made
        them as the hook writes it), the state before every frame and after the last, the cost after every frame."""
        if self._exp is None:
            out = []
            for c in range(self.C):
                s = (int(self.state[c]), 0, np.zeros(30, np.uint8), int(self.dep401[c]), 0)
                recs, before, trace = [], [], []
                for f in range(self.F):
                    before.append(s)
                    r = ol.decode_frame(int(self.st[c, f]), self.llr[c, f], *s)
                    s = r[1:]
                    rr = r[0].copy()
                    rr["sample_pos"] = f
                    recs.append(rr)
                    trace.append(int(r[5]))   # (-1: size_t(-1))
                out.append(dict(recs=np.concatenate(recs), before=before, final=s, trace=np.array(trace, np.int64)))
            self._exp = out
        return self._exp

    def viterbi_inputs(self):
        """(channel, frame, kind, soft) of every frame that goes through a Viterbi decoder."""
        res = []
        for c, e in enumerate(self.expect()):
            for f in range(self.F):
                b = e["before"][f]
                vi = viterbi_input(int(self.st[c, f]), b[0], self.llr[c, f], b[3])
                if vi is not None:
                    res.append((c, f, vi[0], vi[1]))
        return res


# ---- frames --------------------------------------------------------------------------------------------------------------------------------
LSF_STREAM = m17hip.make_lsf("W1AW", "N0CALL", 0x0005)
LSF_FULL = m17hip.make_lsf("", "N0CALL", 0x0004)    # bits 109..111 = 1 0 0: packet, type 2 -> FULL_PACKET (M17FrameDecoder.h:113-136)
LSF_BASIC = m17hip.make_lsf("", "N0CALL", 0x0002)   # 0 1 0: packet, type 1 -> BASIC_PACKET


def _soft(bits, mag):
    return ((np.asarray(bits, np.int16) * 2 - 1) * mag).astype(np.int8)


@functools.lru_cache(maxsize=None)
def valid_frames():
    """(sync type, on-air bits) of valid frames of every kind: the oracle's own bursts (BERT, stream, BASIC packet) and a FULL_PACKET
    transmission built with tx_build — its LSF, three packet frames and one with the last-frame bit set."""
    out = []
    for kind in (0, 1, 2):
        fb, st = ol.make_frames(kind, 700 + kind, 7)
        out += [(int(t), b.copy()) for t, b in zip(st, fb)]
    rng = np.random.default_rng(612)
    out.append((0, tb.lsf_frame(LSF_FULL)))
    for i in range(4):
        row = bytearray(rng.integers(0, 256, 26).astype(np.uint8).tobytes())
        row[25] = (0x80 | (9 << 2)) if i == 3 else (i << 2)
        out.append((2, tb.packet_frame(bytes(row))))
    out.append((0, tb.lsf_frame(LSF_STREAM)))
    return out


def noisy(bits, rng, flip, erase=0.1, mag=None):
    m = rng.integers(1, 8, 368) if mag is None else mag
    fr = _soft(bits, m).astype(np.int16)
    fr = np.where(rng.random(368) < flip, -fr, fr)
    fr[rng.random(368) < erase] = 0
    return fr.astype(np.int8)


@functools.lru_cache(maxsize=None)
def class_frames():
    """[(class name, llr368)]: the frame classes, before a sync type is put on them."""
    rng = np.random.default_rng(6120)
    out = [("zero", np.zeros(368, np.int8)), ("plus7", np.full(368, 7, np.int8)), ("minus7", np.full(368, -7, np.int8)),
           ("alternating", (7 * (1 - 2 * (np.arange(368) & 1))).astype(np.int8))]
    out += [("random", rng.integers(-7, 8, 368).astype(np.int8)) for _ in range(6)]
    for k in (1, 2, 8, 32):
        for _ in range(2):
            f = np.zeros(368, np.int8)
            f[rng.choice(368, k, replace=False)] = rng.choice([-1, 1], k)
            out.append((f"sparse{k}", f))
    vf = valid_frames()
    i = 0
    for mag in range(1, 8):
        for flip in (0.0, 0.03, 0.3):
            for _ in range(2):
                out.append((f"valid_m{mag}_f{flip}", noisy(vf[i % len(vf)][1], rng, flip, mag=mag)))
                i += 5    # (coprime with the list's length: every frame of it comes up)
    out += [("negated", (-_soft(b, 7)).astype(np.int8)) for _, b in vf[::4]]
    return out


@functools.lru_cache(maxsize=None)
def seq_classes():
    """Every class frame under the four sync types, from the state in which that sync type is decoded (and a stream sync word in state LSF:
    the LICH path); the BERT frames of the oracle's burst under every dep401.  One channel each, the frame twice: in form 2 a stream or BERT
    channel's first frame goes to the packed decoder, its second — the one the state still names — to the wave decoder of the settling
    kernel."""
    llr, st, state, dep = [], [], [], []
    for _, f in class_frames():
        for s, s0 in ((0, 0), (1, 1), (1, 0), (2, 3), (2, 2), (3, 0)):
            llr.append(f); st.append(s); state.append(s0); dep.append(0)
    rng = np.random.default_rng(6121)
    berts = [b for t, b in valid_frames() if t == 3][:3]
    for d in (-7, -1, 0, 1, 7):
        for b in berts:
            for flip in (0.0, 0.03):
                llr.append(noisy(b, rng, flip)); st.append(3); state.append(4); dep.append(d)
        llr.append(np.zeros(368, np.int8)); st.append(3); state.append(0); dep.append(d)
    llr = np.stack(llr)
    return Sequence("classes", np.stack([llr, llr], axis=1), np.stack([st, st], axis=1), 4, state=state, dep401=dep)


@functools.lru_cache(maxsize=None)
def seq_walks():
    """Random walks, C = 3 (odd: the second wave of the deferred decode's last workgroup has no channel), F = 24: transmissions of random kind
    (stream, BASIC packet, FULL packet: an LSF and one to four payload frames; BERT: one to four frames) back to back under noise, every frame
    with probability 0.15 under a sync type drawn on its own, as tests/test_gpu_parity.py::test_decode_frames_random_walk_batch does."""
    vf = valid_frames()
    lsf = {"stream": vf[7][1], "basic": vf[15][1], "full": vf[23][1]}
    pay = {"stream": [b for t, b in vf[8:15]], "basic": [b for t, b in vf[16:23]], "full": [b for t, b in vf[24:28]], "bert": [b for t, b in vf[:7]]}
    assert [vf[i][0] for i in (7, 15, 23)] == [0, 0, 0] and all(t == 2 for t, _ in vf[24:28])
    sync_of = {"stream": 1, "basic": 2, "full": 2, "bert": 3}
    seqs = []
    for w in range(4):
        rng = np.random.default_rng(6170 + w)   # (the seeds: the first base tried at which the four walks visit all twenty pairs of decoder state and sync type — tests/test_decode_forms.py asserts it)
        llr, st = np.zeros((3, 24, 368), np.int8), np.zeros((3, 24), np.uint8)
        for c in range(3):
            frames = []
            while len(frames) < 24:
                kind = ("stream", "basic", "full", "bert")[rng.integers(4)]
                if kind != "bert":
                    frames.append((0, lsf[kind], rng.choice([0.0, 0.0, 0.03])))
                for _ in range(rng.integers(1, 5)):
                    frames.append((sync_of[kind], pay[kind][rng.integers(len(pay[kind]))], rng.choice([0.0, 0.03, 0.3])))
            for f, (s, b, flip) in enumerate(frames[:24]):
                llr[c, f] = noisy(b, rng, flip, erase=rng.choice([0.0, 0.1]))
                st[c, f] = rng.integers(0, 4) if rng.random() < 0.15 else s
        seqs.append(Sequence(f"walk{w}", llr, st, 48))
    return seqs


@functools.lru_cache(maxsize=None)
def seq_long():
    """C = 3, F = 530, around slot 512 of a record store (the deferred decode lists deferred slots 512 at a time).
    Channel 0: 520 stream-sync frames in state LSF whose LICH fragments are numbers 0 to 4 only — the LSF never completes: 512 or more LICH
    records, none deferred —, then the LSF frame, then nine stream frames: every deferred slot is 512 or beyond.
    Channel 1: state STREAM from the start, 530 stream frames: deferred slots on both sides of 512.
    Channel 2: 530 BERT frames under dep401 = -7: the same with the longest trellis (201 decision words a frame)."""
    rng = np.random.default_rng(6140)
    llr, st = np.zeros((3, 530, 368), np.int8), np.ones((3, 530), np.uint8)
    row = lambda: bytes(rng.integers(0, 256, 18).astype(np.uint8).tobytes())
    for f in range(520):
        llr[0, f] = noisy(tb.stream_frame(LSF_STREAM, f % 5, row()), rng, 0.01, erase=0.0)
    llr[0, 520], st[0, 520] = noisy(tb.lsf_frame(LSF_STREAM), rng, 0.0, erase=0.0), 0
    for f in range(521, 530):
        llr[0, f] = noisy(tb.stream_frame(LSF_STREAM, f % 6, row()), rng, 0.03)
    for f in range(530):
        llr[1, f] = noisy(tb.stream_frame(LSF_STREAM, f % 6, row()), rng, (0.0, 0.03, 0.3)[f % 3])
    berts, _ = ol.make_frames(0, 733, 530)
    for f in range(530):
        llr[2, f] = noisy(berts[f], rng, (0.0, 0.03, 0.3)[f % 3])
    st[2, :] = 3
    return Sequence("long", llr, st, 600, state=[0, 1, 0], dep401=[0, 0, -7])


@functools.lru_cache(maxsize=None)
def seq_full():
    """C = 3, F = 24, a record store of 7 slots: stream frames (channel 0, from state STREAM), BERT frames (channel 1) and a walk (channel 2)
    that arrive at a full store — defer_frame returns 0 and the frame is decoded in place."""
    rng = np.random.default_rng(6150)
    vf = valid_frames()
    llr, st = np.zeros((3, 24, 368), np.int8), np.zeros((3, 24), np.uint8)
    streams, berts = [b for t, b in vf if t == 1], [b for t, b in vf if t == 3]
    for f in range(24):
        llr[0, f], st[0, f] = noisy(streams[f % len(streams)], rng, (0.0, 0.03, 0.3)[f % 3]), 1
        llr[1, f], st[1, f] = noisy(berts[f % len(berts)], rng, (0.0, 0.03, 0.3)[f % 3]), 3
        t, b = vf[rng.integers(len(vf))]
        llr[2, f], st[2, f] = noisy(b, rng, 0.03), t
    return Sequence("full_store", llr, st, 7, state=[1, 0, 0], dep401=[0, 7, 0])


def all_sequences():
    return [seq_classes()] + seq_walks() + [seq_long(), seq_full()]


@functools.lru_cache(maxsize=None)
def restated():
    """viterbi_np over every frame of every sequence that goes through a Viterbi decoder, by kind: {kind: (keys [(sequence, channel, frame)],
    soft [N][IN], result dict)}."""
    by_kind = {k: ([], []) for k in range(4)}
    for q in all_sequences():
        for c, f, kind, soft in q.viterbi_inputs():
            by_kind[kind][0].append((q.name, c, f))
            by_kind[kind][1].append(soft)
    return {k: (keys, np.stack(soft), viterbi_np(np.stack(soft), SHAPES[k][1])) for k, (keys, soft) in by_kind.items()}
