"""One run or segment boundary at EVERY phase of the frame cycle (TEST INFRASTRUCTURE ONLY, numpy only): the inputs of tests/test_gpu_boundary_phases.py
and the oracle's side of them, made once per process.

The construction.  Channels are independent, so a batch can put one boundary at every phase at once: channel c of a batch carries the SAME transmission
(one kind; one generator seed and frame count, or one for the even and one for the odd channels: KINDS below) delayed by c samples, lead_in = 3072 + c, c = 0 .. 1919, over T = 24 frames of 1920 samples.  A boundary at sample e
of the stream then falls, over the batch, 1920 different distances behind the transmission's start.  The transmission is followed by loud noise (sigma
2500): the carrier detect stays on, the demodulator goes on framing noise, loses it by missing syncs, is forced to unlock and re-enters late, over and over,
so most channels are still inside a frame when the stream ends.

Why frame completions are the thing to count.  tests/test_boundary_phases.py asserts on the oracle alone that the sample_pos of the payload-frame records,
taken modulo 1920 (and modulo 640: the GPU tests cut there too), covers every residue over a batch.  A run that ends every 1920 samples then ends, on some
channel, on every sample of the locked frame cycle.  Everything else that happens in a locked cycle sits at a fixed offset from the frame's completion:
the sync phase begins with the sample behind it (77 counting samples, then the window in which the trigger rises, peaks and falls), SYNC_WAIT ends when
sync_count reaches 86, need_clock_update is set there and honoured at the next sample whose correlator index is 0, the |d| = 5 clock update comes five
samples off the symbol instant of the first payload symbol, and the framer fills two LLRs every ten samples from there to the next completion.  So once the
completions cover all residues, each of these events falls on every phase of the boundary as well, without being looked for one by one.

The float form of a batch is f32_lib.on_grid of the same int16 samples; on those floats a float stream gives what the int16 path gives (tests/test_gpu_f32_input.py),
so one oracle result serves both sample types."""
import numpy as np

import f32_lib as fl
import off_clock as oc
import oracle_lib as ol
import spliced as sp

FRAME = 1920
C, T = 1920, 24 * FRAME
MIXED_C = 384
FT_LSF, FT_LICH, FT_STREAM, FT_BASIC_PACKET, FT_FULL_PACKET, FT_BERT = range(6)
ST_UNLOCKED = 0                                         # m17_diag.demod_state

# batch -> (generator kind, frames of the even and of the odd channels, frame_type of its payload-frame records, generator seed of the even and of the
# odd channels).  The stream batch is 4 frames from one seed.  A BERT burst of 5 frames from one seed leaves 25 residues uncovered (1895 of 1920): whether the burst is acquired
# depends on where its preamble meets the carrier detect's 384-sample cadence, and 169 channels acquire nothing.  Measured (residues covered, channels
# with a record): 8 frames 1917 / 1781, 12 frames 1910 / 1834, 16 frames 1849 / 1852; with a second seed on the odd channels 5 frames 1919 / 1853,
# 8 frames 1919 / 1863, 12 frames 1920 / 1891, 16 frames 1913 / 1895.  But a burst of 12 frames ends so late that the eleven missed sync words behind it
# do not fit into the stream (51 channels show a forced unlock); at most 8 frames do.  8 frames with seed 7200 on the odd channels: 1920 residues, 1771
# channels with a forced unlock.
# A packet of 3 frames on every channel covers 1920 residues, but only 779 channels show a forced unlock (1 / 2 / 4 / 5 / 6 frames: 947 / 851 / 690 / 560 /
# 502; thirty more seeds at 1 or 3 frames: 687 .. 947 wherever the residues stay at 1920): behind its last frame the frame decoder is back in its LSF state
# and most channels lose the noise by the carrier detect's level, not by force.  So the odd channels send a packet transmission whose payload never
# comes — preamble, LSF, EOT (0 frames): the LSF leaves the decoder in its packet state, the demodulator frames noise in PACKET_SYNC and is forced out.
# 3 frames on the even and 0 on the odd channels, one seed: 1920 residues (640 of 640), 1728 LSF residues, 1328 channels with a forced unlock.
KINDS = {"stream": (1, (4, 4), FT_STREAM, (7001, 7001)), "bert": (0, (8, 8), FT_BERT, (7000, 7200)), "packet": (4, (3, 0), FT_BASIC_PACKET, (7004, 7004))}
BATCHES = ("stream", "bert", "packet")
# the packet-hole variant: a packet transmission of HOLE_FRAMES payload frames whose frames 3 .. 18 are overwritten (spliced.hole, timing kept): sixteen
# sync words go missing in PACKET_SYNC, more than MAX_MISSING_SYNC = 10, so the demodulator can give up (do_packet_sync's last branch) before the
# transmission comes back.  Plain noise as the fill does NOT get there (0 of 384 channels): a noise frame decodes with the end-of-packet bit set half of
# the time, the frame decoder returns to its LSF state and the demodulator leaves PACKET_SYNC for STREAM_SYNC after two frames on average; the
# transmission under added noise hardly does either (the band of noise levels in which a frame costs 60 or more and still decodes is narrow: 1-2 of 32
# channels at any sigma from 3000 to 7000).  The fill is therefore the transmission itself with every HOLE_EVERY-th symbol (ten samples) taken from ANOTHER
# packet transmission on the same clock, and noise ALONE over every sync word (40 samples before it to 40 behind): no sync word is found, the frames
# still decode as packet frames that are not the last, and each carries about ten confidently wrong symbols, which cost 60 or more together.  Measured
# with a coverage build of the oracle at every 16th, 18th and 20th symbol: 5, 3 and 0 of 32 channels give up; at every 14th 8 of 32; at every 12th the
# frames stop decoding.  384 channels, delayed by 5 c samples: every fifth phase.
HOLE_C, HOLE_STEP, HOLE_FRAMES, HOLE_FIRST, HOLE_N, HOLE_SIGMA, HOLE_EVERY = 384, 5, 19, 3, 16, 2500.0, 14
DCD_LTRIG = 0.1                                         # DataCarrierDetect's lower trigger level: above it a carrier detect that is on stays on

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _gen(seed, kind, n_frames, lead_in, total=T, truth=False):
    p = ol.gen_params(seed=seed, kind=kind, n_frames=n_frames, lead_in=lead_in, noise_sigma=300.0, tail_sigma=2500.0, lead_sigma=40000.0, total=total)
    return ol.generate(p, with_truth=truth)


def _frozen(x):
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x


def batch(name):
    """x [C][T] int16 (read-only) of batch `name`: "stream", "bert", "packet", "mixed" (the first MIXED_C stream channels, every second one from an inverted
    transmitter) or "hole" (HOLE_C channels)."""
    def make():
        if name == "mixed":
            x = batch("stream")[:MIXED_C]
            return _frozen(np.where(polarity()[:, None] == 1, oc.negated(x), x))
        if name == "hole":
            return _frozen(np.stack(oc.par(_hole_channel, range(HOLE_C))))
        kind, nf, _, seeds = KINDS[name]
        return _frozen(np.stack(oc.par(lambda c: _gen(seeds[c & 1], kind, nf[c & 1], 3072 + c)[:T], range(C))))
    return _cached(("x", name), make)


def polarity():
    """The polarity table of the mixed batch: every second channel inverted."""
    return (np.arange(MIXED_C) & 1).astype(np.uint8)


def _hole_channel(c):
    x, tr = _gen(7004, 4, HOLE_FRAMES, 3072 + HOLE_STEP * c, truth=True)
    x = x[:T]
    other = _gen(9999, 4, HOLE_FRAMES, 3072 + HOLE_STEP * c)[:T]
    nz = sp.noise(7004 ^ 0x5EED5, T, HOLE_SIGMA)
    fill = x.copy()
    for i in range(HOLE_FIRST, HOLE_FIRST + HOLE_N + 1):
        fs = tr["burst_start"] + (2 + i) * FRAME
        for j in range(8 + i % HOLE_EVERY, 192, HOLE_EVERY):      # symbol j of frame i, the other transmission's
            fill[fs + 10 * j - 5:fs + 10 * j + 5] = other[fs + 10 * j - 5:fs + 10 * j + 5]
        fill[fs - 40:fs + 120] = nz[fs - 40:fs + 120]             # the sync words themselves go
    return sp.hole(x, tr["burst_start"] + (2 + HOLE_FIRST) * FRAME, HOLE_N, "noise", fill)


def hole_span(c):
    """(first, one past the last) sample of channel c's hole: the generator puts the preamble at lead_in."""
    a = 3072 + HOLE_STEP * c + (2 + HOLE_FIRST) * FRAME
    return a, a + HOLE_N * FRAME


def f32(x):
    """The float form of int16 samples (f32_lib.on_grid), made in row blocks so that the float64 intermediate stays small."""
    x = np.asarray(x)
    out = np.empty(x.shape, dtype=np.float32)
    for a in range(0, x.shape[0], 64):
        out[a:a + 64] = fl.on_grid(x[a:a + 64])
    return out


class Oracle:
    """The oracle over one batch: rows[c] (records, `channel` filled in), logs[c] (every diagnostic callback), diags [C] (the final m17_diag), and the same
    flattened in (channel, order of appearance) for the partition: recs / rec_pos, log / log_pos / log_chan."""

    def __init__(self, name):
        x = batch(name)
        self.name, self.C = name, x.shape[0]
        self.rows, self.diags, self.logs = oc.oracle_of("boundary phases " + name, x, polarity() if name == "mixed" else None, logs=True)
        self.recs = np.concatenate(self.rows)
        self.rec_pos = self.recs["sample_pos"].astype(np.int64)
        self.log = np.concatenate(self.logs)
        self.log_pos = np.concatenate([oc.log_pos(l) for l in self.logs]).astype(np.int64)
        self.log_chan = np.repeat(np.arange(self.C), [l.size for l in self.logs])

    # ---- the partition: what belongs to piece k of a stream cut at ends e_0 < e_1 < ... is what the oracle reports for a sample in [e_{k-1}, e_k) ------
    def pieces(self, ends):
        """(records per piece, log entries per piece, log entries per piece and channel [pieces][C]): each piece's records in (channel, seq) order and its
        log entries in (channel, stream) order, as the library returns them for a run over that piece."""
        ends = np.asarray(ends, dtype=np.int64)
        assert (np.diff(ends) > 0).all() and ends[-1] >= T
        out = []
        for flat, pos in ((self.recs, self.rec_pos), (self.log, self.log_pos)):
            k = np.searchsorted(ends, pos, side="right")
            order = np.argsort(k, kind="stable")
            cut = np.searchsorted(k[order], np.arange(ends.size + 1))
            out.append([flat[order[cut[i]:cut[i + 1]]] for i in range(ends.size)])
        k = np.searchsorted(ends, self.log_pos, side="right")
        counts = np.zeros((ends.size, self.C), dtype=np.uint32)
        np.add.at(counts, (k, self.log_chan), 1)
        return out[0], out[1], counts

    # ---- event positions, read off the oracle alone ---------------------------------------------------------------------------------------------------
    def completions(self, frame_type):
        """(channel, sample_pos) of every record of that frame type."""
        m = self.recs["frame_type"] == frame_type
        return self.recs["channel"][m].astype(np.int64), self.rec_pos[m]

    def forced_unlocks(self):
        """(channel, sample) of the callbacks at which `locked` has fallen from 1 to 0 since the channel's previous callback while the carrier was still
        there.  The callback's own `dcd` cannot say so: dcd.unlock() clears the detector's trigger, update_dcd() runs BEFORE the callback fires, so the
        first callback behind a forced unlock reports dcd = 0 exactly as a carrier that went away does.  What tells them apart is dcd_level, the level of
        the update before: above the lower trigger (0.1) the detector would have stayed on, so the demodulator was unlocked by force; a carrier that went
        away left a level at or below it."""
        return forced_unlocks_of(self.log, self.log_pos, self.log_chan)

    def carrier_off_segments(self, seg, first=2):
        """(channel, segment index k >= first) of every segment [k seg, (k + 1) seg) of a run cut every `seg` samples over which the carrier detect is off
        throughout: it lies between two consecutive callbacks of the channel that both report dcd = 0 (or a chain of such pairs), and the carrier detect
        changes at callbacks only.  These are the segments whose front end the gate-aware schedule may skip."""
        same = self.log_chan[1:] == self.log_chan[:-1]
        off = same & (self.log["dcd"][:-1] == 0) & (self.log["dcd"][1:] == 0)
        out, last = [], None
        for a, b, c in zip(self.log_pos[:-1][off].tolist(), self.log_pos[1:][off].tolist(), self.log_chan[1:][off].tolist()):
            if last is not None and last[2] == c and last[1] == a:
                last[1] = b
            else:
                last = [a, b, c]
                out.append(last)
        found = []
        for a, b, c in out:            # samples a + 1 .. b are off
            found += [(c, k) for k in range(max(first, -(-(a + 1) // seg)), (b + 1) // seg)]
        return found

    def dcd_changes(self):
        """(channel, sample) of the callbacks at which `dcd` differs from the channel's previous callback."""
        same = self.log_chan[1:] == self.log_chan[:-1]
        m = same & (self.log["dcd"][1:] != self.log["dcd"][:-1])
        return self.log_chan[1:][m], self.log_pos[1:][m]


def oracle(name):
    return _cached(("oracle", name), lambda: Oracle(name))


def delay(name):
    """Samples by which channel c's transmission is delayed against channel 0's."""
    return np.arange(HOLE_C) * HOLE_STEP if name == "hole" else np.arange(MIXED_C if name == "mixed" else C)


def run_ends(L, total=T):
    """The ends of consecutive runs (or segments) of L samples over the stream."""
    return np.arange(L, total + L, L).clip(max=total) if total % L else np.arange(L, total + 1, L)


def forced_unlocks_of(log, pos, chan):
    same = chan[1:] == chan[:-1]
    m = same & (log["locked"][:-1] != 0) & (log["locked"][1:] == 0) & (log["dcd_level"][1:] > DCD_LTRIG)
    return chan[1:][m], pos[1:][m]


def gave_up_packet_sync(rows, log, span):
    """The sample of the callback that shows do_packet_sync giving up inside `span` of one channel, or None.  The frame decoder emits a record for every
    frame it decodes in a packet state and leaves that state exactly when the record's end-of-packet bit (payload[25] & 0x80) is set, so behind a packet
    record with that bit clear the demodulator is in PACKET_SYNC.  From there it goes to SYNC_WAIT or FRAME — locked for the rest of a frame, which only
    a carrier that goes away (dcd_level at or below 0.1) can cut short — or, at most 87 samples behind the record, to UNLOCKED through the give-up branch.
    So: a forced unlock (forced_unlocks_of) whose callback comes no more than 87 + 960 samples behind such a record, the channel's latest."""
    pos = oc.log_pos(log).astype(np.int64)
    _, at = forced_unlocks_of(log, pos, np.zeros(log.size, dtype=np.int64))
    for p in at.tolist():
        if span[0] <= p < span[1]:
            before = rows[rows["sample_pos"] < p]
            if (before.size and before["frame_type"][-1] in (FT_BASIC_PACKET, FT_FULL_PACKET) and not before["payload"][-1][25] & 0x80
                    and p - int(before["sample_pos"][-1]) <= 87 + 960):
                return p
    return None


def states_between(log, a, b):
    """demod_state of the callbacks of one channel with a <= sample < b, runs of equal values collapsed."""
    pos = oc.log_pos(log).astype(np.int64)
    st = log["demod_state"][(pos >= a) & (pos < b)].tolist()
    return [v for i, v in enumerate(st) if i == 0 or v != st[i - 1]]
