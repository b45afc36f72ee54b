"""Transmissions joined late, cut short, with holes and spliced back to back (TEST INFRASTRUCTURE ONLY, numpy only).  Every other input of the suite is a
whole, well-formed transmission: preamble, LSF, frames in order with LICH segments 0, 1, 2, ..., EOT.  The functions here cut and join the int16
waveforms that oracle_lib.generate() makes; nothing is generated or modulated anew.  The oracle and the library under test get the SAME array, so
only determinism matters: no random numbers beyond the generator's own seeds.

Geometry: `burst_start` (the generator's truth) is the first preamble sample; a preamble, an LSF and a payload frame are FRAME = 1920 samples
each, so payload frame i of a stream or packet transmission with one preamble starts at burst_start + (2 + i) * 1920 and carries LICH segment
i % 6.  (The pulse shaping spreads every symbol over 150 samples, so a cut at a frame edge leaves half a pulse of the neighbour: the receiver sees
what a receiver sees when a carrier comes or goes.)"""
import numpy as np

import off_clock as oc
import oracle_lib as ol

FRAME = 1920
GAPS = (0, 7, 400, 1920, 5000)
ST_UNLOCKED = 0          # m17_diag.demod_state of an unlocked demodulator
FT_LSF, FT_LICH, FT_STREAM, FT_BASIC_PACKET, FT_FULL_PACKET, FT_BERT = range(6)


# ---- the five operations -------------------------------------------------------------------------------------------------------------------
def noise(seed, n, sigma):
    """n samples of the generator's own tail noise: a noise-only (kind 3) waveform of that sigma (sigma 0: its +-1 dither)."""
    return ol.generate(ol.gen_params(seed=seed, kind=3, lead_in=0, noise_sigma=sigma, tail_sigma=sigma, total=n))[:n]


def late_entry(x, burst_start, n_lead_frames, k, off):
    """Drops the samples from burst_start up to (n_lead_frames + k) * FRAME + off behind it: the preamble(s), the LSF (n_lead_frames of them
    together) and k payload frames (and `off` samples of the next) go, the lead-in in front stays.  Shorter by what was dropped."""
    assert 0 <= burst_start and n_lead_frames >= 0 and k >= 0 and off >= 0
    cut = burst_start + (n_lead_frames + k) * FRAME + off
    assert cut <= x.size
    return np.concatenate([x[:burst_start], x[cut:]])


def drop_tail(x, burst_start, frames_kept, fill):
    """The transmission ends `frames_kept` frames behind burst_start (preambles and LSF count): from there on the samples are `fill`'s (a
    noise(...) array as long as x), so there is no EOT: the carrier simply disappears."""
    assert fill.shape == x.shape
    end = burst_start + frames_kept * FRAME
    assert 0 <= end <= x.size
    out = x.copy()
    out[end:] = fill[end:]
    return out


def hole(x, start, n_frames, mode, fill=None, extra=0):
    """A hole of n_frames * FRAME + extra samples at `start`.  mode "noise": overwritten with fill's samples (timing kept, syncs go missing);
    mode "remove": deleted (timing jumps by whole frames, or by frames plus `extra` samples); the result is shorter by the hole."""
    n = n_frames * FRAME + extra
    assert 0 <= start and start + n <= x.size and n >= 0
    if mode == "noise":
        assert fill is not None and fill.shape == x.shape
        out = x.copy()
        out[start:start + n] = fill[start:start + n]
        return out
    assert mode == "remove"
    return np.concatenate([x[:start], x[start + n:]])


def blank_lsf(x, burst_start, fill, n_preamble=1):
    """Only the LSF frame (the one behind the preamble(s)) is overwritten with fill's samples; the preamble stays."""
    return hole(x, burst_start + n_preamble * FRAME, 1, "noise", fill)


def splice(a, b, gap, fill):
    """Transmission b `gap` samples (fill's first) behind the end of a."""
    assert 0 <= gap <= fill.size
    return np.concatenate([a, fill[:gap], b])


# ---- the batches of tests/test_gpu_spliced.py, named here so that tests/test_spliced.py asserts its conditions on exactly these -------------------
C, T = 64, 96000
SIGMAS = (0.0, 300.0, 700.0)
_CACHE = {}


def _gen(seed, kind, n_frames, lead_in, sigma, total=0, n_preamble=0):
    p = ol.gen_params(seed=seed, kind=kind, n_frames=n_frames, lead_in=lead_in, noise_sigma=sigma, tail_sigma=max(sigma, 100.0),
                      lead_sigma=40000.0, total=total, n_preamble=n_preamble)
    return ol.generate(p, with_truth=True)


def _cached(name, make):
    if name not in _CACHE:
        b = make()
        for v in b.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[name] = b
    return _CACHE[name]


def _fill(seed, sigma, n=T + 8 * FRAME):
    return noise(seed ^ 0x5EED5, n, max(sigma, 100.0))


def _seeds(bumped):
    """Generator seeds 9300 + 7 c; the channels named in `bumped` take that many times 1000 more (searched once on the CPU, see each list)."""
    return tuple(9300 + 7 * c + 1000 * bumped.get(c, 0) for c in range(C))


OFFS = (0, 960, 7, 1913, 333, 1201)          # late entry: at a frame edge, mid-frame, and values not divisible by 10


# -- late entry: 48 streams joined k frames (and `off` samples) behind their LSF, 16 packet transmissions with the same head cut ---------------
def late_kind(c):
    return 1 if c % 4 != 3 else (2, 4)[(c // 4) % 2]


def late_channel(c, seed):
    kind, off, sigma = late_kind(c), OFFS[(c // 2) % 6], SIGMAS[c % 3]
    k = (3 * (c // 4) + c % 4) % 12 if kind == 1 else c % 5          # the 48 streams walk through k = 0 .. 11 four times
    lead = 2048 + 331 * (c % 7)
    x, tr = _gen(seed, kind, 60 if kind == 1 else 30, lead, sigma, total=T + (2 + k) * FRAME + off + 64)
    return dict(x=late_entry(x, tr["burst_start"], 2, k, off)[:T], bs=tr["burst_start"], k=k, off=off, lead=0, kind=kind, lsf=tr["lsf"], sigma=sigma)


# -- blank_lsf: 64 streams whose LSF frame is overwritten, the preamble intact.  The fill is the waveform itself one frame late, i.e. the
#    preamble's own samples once more (its pattern has a period of 20 samples, so the seam is smooth): the demodulator stays in LSF_SYNC counting
#    preamble hits and meets the first STREAM sync word there — the STREAM branch of do_lsf_sync.  (Generator tail noise as the fill does NOT get
#    there: the carrier's drop behind the preamble is taken for a BERT sync word or loses the lock, 0 of 64 channels x 40 seeds; NOTES.)
def blank_channel(c, seed):
    sigma = SIGMAS[c % 3]
    lead = 2048 + 331 * (c % 7) + 97 * (c % 5)
    x, tr = _gen(seed, 1, 60, lead, sigma, total=T)
    late = np.concatenate([x[:FRAME], x[:-FRAME]])
    return dict(x=blank_lsf(x, tr["burst_start"], late), bs=tr["burst_start"], k=0, off=0, lead=2, kind=1, lsf=tr["lsf"], sigma=sigma)


def took_stream_branch_of_lsf_sync(m, rows, log):
    """The first record is a LICH record with segment counter 0, selected by a STREAM sync word, fired where payload frame 0 ends (138 samples of
    filter delay behind it), and from the preamble on the diagnostic log goes LSF_SYNC (1) -> FRAME (6) without an unlocked entry between: the
    only way from LSF_SYNC to a frame decoded under a STREAM sync word is that branch."""
    if not rows.size:
        return False
    r = rows[0]
    if r["frame_type"] != FT_LICH or r["sync_type"] != 1 or lich_counter(r) != 0 or abs(int(r["sample_pos"]) - (m["bs"] + 3 * FRAME + 138)) > 3:
        return False
    pos = oc.log_pos(log)
    st = log["demod_state"][(pos > m["bs"] + 400) & (pos < int(r["sample_pos"]))].tolist()
    st = [v for i, v in enumerate(st) if i == 0 or v != st[i - 1]]
    return st in ([1, 6], [0, 1, 6])


# -- drop_tail: the carrier disappears; c % 4 = 0 a stream, 1 its twin that ends with EOT at the same place, 2 a packet, 3 a BERT burst ----------
def tail_channel(c, seed):
    sigma = SIGMAS[(c // 4) % 3]
    kept = 10 + (c // 4) % 9                                   # frames behind burst_start, preamble(s) and LSF included
    lead = 2048 + 331 * (c % 7)
    role = c % 4
    if role == 1:                                              # the same stream (seed of channel c - 1) sent to its end: kept - 2 payload frames, EOT
        x, tr = _gen(seed, 1, kept - 2, lead, sigma, total=T)
        return dict(x=x[:T].copy(), bs=tr["burst_start"], kept=kept, kind=1, eot=True, sigma=sigma)
    kind = (1, None, 4, 0)[role]
    x, tr = _gen(seed, kind, 40 if kind != 4 else 30, lead, sigma, total=T)
    return dict(x=drop_tail(x, tr["burst_start"], kept, _fill(seed, sigma)[:T]), bs=tr["burst_start"], kept=kept, kind=kind, eot=False, sigma=sigma)


def tail_seed_of(c, seeds):
    return seeds[c - 1] if c % 4 == 1 else seeds[c]


# -- hole: frames missing in the middle; even channels keep the timing (noise), odd ones lose it (remove) ---------------------------------------
HOLE_FRAMES = (1, 2, 3, 5, 9, 11, 12)                         # fewer and more than MAX_MISSING_SYNC = 10 missed sync words
HOLE_EXTRA = (0, 3, 7, 960, 1917, 0)


def hole_channel(c, seed):
    kind = (1, 1, 0, 2)[(c // 2) % 4]
    mode = "noise" if c % 2 == 0 else "remove"
    nf, extra, sigma = HOLE_FRAMES[(c // 2) % 7], HOLE_EXTRA[(c // 4) % 6], SIGMAS[c % 3]
    lead = 2048 + 331 * (c % 7)
    n = nf * FRAME + extra
    x, tr = _gen(seed, kind, 60 if kind != 2 else 30, lead, sigma, total=T + n)
    start = tr["burst_start"] + (10 + c % 5) * FRAME + (960 if c % 8 >= 4 else 0)
    y = hole(x, start, nf, mode, _fill(seed, sigma, T + n) if mode == "noise" else None, extra)
    return dict(x=y[:T].copy(), bs=tr["burst_start"], start=start, n=n, nf=nf, extra=extra, mode=mode, kind=kind, sigma=sigma)


# -- splice: transmission b `gap` samples behind a; kinds stream -> packet -> BERT -> stream (and stream -> stream); a ends with its EOT or, on
#    c % 8 >= 4 and for BERT (which has none), with a dropped tail; b has no lead-in, so its preamble comes straight behind
SPLICE_KINDS = ((1, 4), (4, 0), (0, 1), (1, 1))


def splice_channel(c, seed):
    ka, kb = SPLICE_KINDS[c % 4]
    gap, sigma = GAPS[c % 5], SIGMAS[(c // 5) % 3]
    na, nb = 6 + c % 7, 12 + c % 5
    a, ta = _gen(seed, ka, na, 2048 + 331 * (c % 7), sigma)
    dropped = ka == 0 or c % 8 >= 4
    if dropped:                                                # the carrier goes at a frame edge, one frame before the end
        a = a[:ta["burst_start"] + (2 + na - (1 if ka else 0)) * FRAME]
    else:                                                      # a ends with its EOT sync word (80 samples) and half a pulse behind it
        a = a[:ta["burst_start"] + (2 + na) * FRAME + 80 + 75]
    b, tb = _gen(seed + 500000, kb, nb, 0, sigma)
    f = _fill(seed, sigma)
    x = splice(a, b, gap, f)
    x = np.concatenate([x, f[x.size:T]])[:T]
    return dict(x=x, bs=ta["burst_start"], a_end=a.size, b_start=a.size + gap + tb["burst_start"], nb=nb, gap=gap, ka=ka, kb=kb, dropped=dropped, sigma=sigma)


def splice_reach(m, rows):
    """(records of a, records in b's span, samples from a's last record to the first record behind b's start)."""
    ra = rows[rows["sample_pos"] <= m["a_end"] + 300]
    rb = rows[(rows["sample_pos"] > m["b_start"] + FRAME) & (rows["sample_pos"] <= m["b_start"] + (2 + m["nb"]) * FRAME + 300)]
    fb = rows[rows["sample_pos"] > m["b_start"]]
    dist = int(fb["sample_pos"][0]) - int(ra["sample_pos"][-1]) if fb.size and ra.size else None
    return ra, rb, dist


def splice_ok(m, rows):
    ra, rb, dist = splice_reach(m, rows)
    return ra.size >= 3 and rb.size >= 3 and (m["gap"] != 0 or dist < 3 * FRAME)


def hole_reach(m, rows, log):
    """What a hole channel shows on the oracle: (records behind the hole, sample_index moved across it, sync lost and regained behind its start)."""
    pos = oc.log_pos(log)
    end = m["start"] + (m["n"] if m["mode"] == "noise" else 0)
    behind = bool((rows["sample_pos"] > end + FRAME).any())
    before, after = log[(pos < m["start"]) & (log["locked"] != 0)], log[(pos > end + 2 * FRAME) & (log["locked"] != 0)]
    moved = bool(before.size and after.size and before["sample_index"][-1] != after["sample_index"][0])
    lk = log["locked"][pos > m["start"]] != 0
    lost = bool((~lk).any() and lk[int(np.argmin(lk)):].any())
    return behind, moved, lost


def hole_ok(m, rows, log):
    behind, moved, lost = hole_reach(m, rows, log)
    if m["mode"] == "remove" and m["n"] % FRAME:
        return behind and (moved or lost)
    return behind


def build(name, channel, seeds, seed_of=None):
    def make():
        chans = oc.par(lambda c: channel(c, seeds[c] if seed_of is None else seed_of(c, seeds)), range(C))
        b = dict(x=np.stack([ch["x"] for ch in chans]), meta=chans)
        assert b["x"].shape == (C, T) and b["x"].dtype == np.int16
        return b
    return _cached(name, make)


# Generator seeds, searched once on the CPU: a channel is bumped (+ 1000 per step) when with the first seed the ORACLE does not show what the batch
# is for, so that tests/test_spliced.py can assert its conditions on EVERY channel.  late: 25, 60 (+ 1000), 38 (+ 2000): the transmission is lost at
# the cut, no LSF assembled from LICH (45 of the 48 streams held at first).  blank: 7, 11, 16, 24, 39, 43, 60 (+ 1000), 55 (+ 2000): the preamble was
# not acquired or a sync word was found late, so the first record is not payload frame 0's (56 of 64 held at first).  tail: 11 (+ 1000), 16
# (+ 2000): the transmission was not locked when its carrier went.  hole: 7, 30 (+ 1000), 23, 55 (+ 2000): no record behind the hole (a packet
# whose noise frame decoded with the end-of-packet bit set, or a transmission not acquired; 60 of 64 held at first).
SEEDS = dict(late=_seeds({25: 1, 38: 2, 60: 1}),
             blank=_seeds({7: 1, 11: 1, 16: 1, 24: 1, 39: 1, 43: 1, 55: 2, 60: 1}),
             tail=_seeds({11: 1, 16: 2}),
             hole=_seeds({7: 1, 23: 2, 30: 1, 55: 2}),
             # splice: 18 channels replaced (46 of 64 held at first): the reference mostly LOSES a transmission that keys up the instant another
             # lets go (it looks for no preamble while it counts missing syncs), so b's span holds fewer than three records with the first seed
             splice=_seeds({0: 2, 1: 1, 7: 1, 8: 4, 9: 5, 11: 1, 13: 1, 16: 2, 17: 1, 25: 11, 33: 25, 35: 1, 37: 1, 41: 36, 48: 3, 57: 7, 60: 1,
                            61: 1}))
CHANNEL = dict(late=(late_channel, None), blank=(blank_channel, None), tail=(tail_channel, tail_seed_of), hole=(hole_channel, None),
               splice=(splice_channel, None))
BATCHES = ("late", "blank", "tail", "hole", "splice")

# what the oracle reports on the head-cut packet transmissions of the late batch, per channel: records by frame type (LSF, LICH, STREAM,
# BASIC_PACKET, FULL_PACKET, BERT).  The packet sync word negated is the BERT one and the frame decoder is in its LSF state, so a packet joined
# late is reported as LICH and BERT records (11 = one run of MAX_MISSING_SYNC + 1 frames), never as packet frames.  Written down so that a
# change of the oracle shows.
PACKET_HIST = {3: (0, 2, 0, 0, 0, 11), 7: (0, 3, 0, 0, 0, 0), 11: (0, 2, 0, 0, 0, 22), 15: (0, 1, 0, 0, 0, 11), 19: (0, 2, 0, 0, 0, 11),
               23: (0, 1, 0, 0, 0, 11), 27: (0, 2, 0, 0, 0, 0), 31: (0, 1, 0, 0, 0, 11), 35: (0, 2, 0, 0, 0, 0), 39: (0, 4, 0, 0, 0, 0),
               43: (0, 2, 0, 0, 0, 11), 47: (0, 1, 0, 0, 0, 22), 51: (0, 4, 0, 0, 0, 11), 55: (0, 4, 0, 0, 0, 11), 59: (0, 0, 0, 0, 0, 21),
               63: (0, 0, 0, 0, 0, 22)}


def batch(name):
    fn, seed_of = CHANNEL[name]
    return build(name, fn, SEEDS[name], seed_of)


def rows_of(name):
    """The oracle over a batch: (x, rows, diags, logs), cached."""
    x = batch(name)["x"]
    return (x,) + oc.oracle_of("spliced " + name, x, None, logs=True)


# ---- reading the oracle's records ------------------------------------------------------------------------------------------------------------
def assembled_lsf(rows):
    """Indices of the LSF records that directly follow a LICH record, i.e. were assembled from LICH segments."""
    ft = rows["frame_type"]
    return [i for i in range(1, rows.size) if ft[i] == FT_LSF and ft[i - 1] == FT_LICH]


def late_pattern(rows):
    """(index of the first LICH record of the collection, index of the assembled LSF) when the records hold >= 1 LICH record, then an LSF record
    directly behind a LICH record, then >= 3 stream records; else None."""
    a = assembled_lsf(rows)
    if not a:
        return None
    ft = rows["frame_type"]
    i = a[0]
    j = i - 1
    while j > 0 and ft[j - 1] == FT_LICH:
        j -= 1
    return (j, i) if int((ft[i + 1:] == FT_STREAM).sum()) >= 3 else None


def lich_counter(rec):
    return int(rec["payload"][5]) >> 5


# ---- how tests/test_gpu_spliced.py feeds the batches (here, so that tests/test_spliced.py checks the same lists on the CPU) ---------------------
RUN_KINDS = ("runs_of_9600", "ragged_runs")
RAGGED = (4801, 7, 1913, 9599, 149, 7681, 3841, 1, 5003)     # no multiples of 8, 192 or 1920; all shorter than the 9600 samples a collection spans


def run_lengths(kind):
    if kind == "runs_of_9600":
        return [9600] * (T // 9600)
    lengths, pos = [], 0
    while pos < T:
        n = min(RAGGED[len(lengths) % len(RAGGED)], T - pos)
        lengths.append(n)
        pos += n
    return lengths


def straddling(name, lengths):
    """Channels whose first LICH record of the collection and whose assembled LSF lie in different runs (from the oracle's positions)."""
    _, rows, _, _ = rows_of(name)
    edges = np.cumsum(lengths)
    out = []
    for c in range(C):
        p = late_pattern(rows[c])
        if p is not None:
            a, b = (int(np.searchsorted(edges, int(rows[c]["sample_pos"][i]), side="right")) for i in p)
            if a != b:
                out.append(c)
    return out


def prefix_diags(name, kind):
    """m17_diag of an oracle demodulator fed the stream up to the end of each run, cached per (batch, run lengths)."""
    def make():
        x = batch(name)["x"]
        ends = np.cumsum(run_lengths(kind))
        return dict(diags=[ol.demod_batch(np.ascontiguousarray(x[:, :e]), cap=2 * (T // FRAME + 2) + 4, threads=oc.THREADS)[2] for e in ends])
    return _cached(("prefix", name, kind), make)["diags"]


def late_mixed_polarity():
    """The late batch with every second channel from an inverted transmitter, and the polarity table that says so."""
    def make():
        pol = (np.arange(C) & 1).astype(np.uint8)
        return dict(y=np.where(pol[:, None] == 1, oc.negated(batch("late")["x"]), batch("late")["x"]), pol=pol)
    b = _cached("late mixed polarity", make)
    return b["y"], b["pol"]


def reset_plan(name="late", L=4800):
    """The reset inside the LICH collection: every third stream channel gets a fresh demodulator at the end of the run (of L samples) that holds
    its third LICH record of the collection.  Returns {channel: sample of the restart}, from the oracle's positions."""
    _, rows, _, _ = rows_of(name)
    plan = {}
    streams = [c for c in range(C) if late_pattern(rows[c]) is not None]
    for c in streams[::3]:
        j, i = late_pattern(rows[c])
        at = (int(rows[c]["sample_pos"][j + 2]) // L + 1) * L
        if at < int(rows[c]["sample_pos"][i]) and at + 12 * FRAME < T:      # in the middle of the collection, room for a whole new one behind
            plan[c] = at
    return plan


def reset_expectation(name="late", L=4800):
    """Per channel of reset_plan(): the records, m17_diag and diagnostic log of a fresh oracle demodulator started at the restart, cached."""
    def make():
        x, plan = batch(name)["x"], reset_plan(name, L)
        out = {}
        for c, at in plan.items():
            r, d = ol.demod(x[c, at:])
            r["channel"] = c
            out[c] = (at, r, d)
        return dict(fresh=out)
    return _cached(("reset", name, L), make)["fresh"]


# ---- the long case: 8 channels x 480 000 samples (ten default segments of 48 000) --------------------------------------------------------------------
LONG_C, LONG_T, SEGMENT = 8, 480000, 48000
# lead-ins searched on the CPU (34 000 + 523 n; channel 3 with the next seed) so that the collection lies astride sample 48 000
LONG_LEADS = (37138, 38184, 35046, 34000, 34523, 34000, 34000, 35046)
LONG_HOLES = ((2, 1), (5, 3), (8, 12))          # (the segment boundary the hole lies astride, frames of noise)


def long_case():
    """A stream of more than 240 frames joined late, with three holes of noise and no EOT (it runs past the end).  The lead-in puts the LICH collection
    astride the first segment boundary (tests/test_spliced.py asserts that on the oracle's positions); each hole starts half a frame before its boundary."""
    def make():
        chans = []
        for c in range(LONG_C):
            seed, k, off, sigma = 9900 + 7 * c + (1000 if c == 3 else 0), c % 6, OFFS[c % 6], SIGMAS[c % 3]
            lead = LONG_LEADS[c]
            x, tr = _gen(seed, 1, 260, lead, sigma, total=LONG_T + (2 + k) * FRAME + off + 64)
            y = late_entry(x, tr["burst_start"], 2, k, off)[:LONG_T]
            f = noise(seed ^ 0x5EED5, LONG_T, max(sigma, 100.0))
            for seg, nf in LONG_HOLES:
                y = hole(y, seg * SEGMENT - FRAME // 2, nf, "noise", f)
            chans.append(dict(x=y, bs=tr["burst_start"], k=k, off=off, lead=0, kind=1, lsf=tr["lsf"]))
        return dict(x=np.stack([ch["x"] for ch in chans]), meta=chans)
    return _cached("long", make)


def long_rows():
    x = long_case()["x"]
    return (x,) + oc.oracle_of("spliced long", x, None, logs=True)


# ---- the scalar C++ demodulator's callback sequence as the oracle gives it (the lines tests/cxx/mirror_check prints in its cpu_demod mode) ------------
def expected_callback_lines(x):
    recs, _ = ol.demod(x)
    log = ol.demod_diag_log(x)
    events = [(int(r["sample_pos"]), 0, r) for r in recs] + [(int(d["pad"][0]) | (int(d["pad"][1]) << 32), 1, d) for d in log]
    events.sort(key=lambda e: (e[0], e[1]))
    exp = []
    for _, k, e in events:
        if k == 0:
            exp.append(f"F {int(e['frame_type'])} {int(e['cost'])} {bytes(e['payload'][:int(e['len'])]).hex()}")
        else:
            w = [int(np.array(e[f], dtype=np.float32).view(np.uint32)) for f in ("evm", "deviation", "offset", "clock")]
            exp.append(f"D {int(e['dcd'])} {w[0]:08x} {w[1]:08x} {w[2]:08x} {int(e['locked'])} {w[3]:08x} {int(e['sample_index'])} "
                       f"{int(e['sync_index'])} {int(e['clock_index'])} {int(e['viterbi_cost'])}")
    exp.append(f"END {log.size}")
    return exp, len(recs), log.size
