"""The oracle with CHOSEN matched-filter taps (tests/cxx/crafted_oracle.cpp) and the inputs the tap tests share: what m17hip_set_fir_taps
(include/m17hip.h, a test hook) makes the device compute.  With the identity taps on a float32 stream the matched filter's output is the input,
so a row written here IS what the correlator, the sync search, the level estimator and the slicer see.

TEST INFRASTRUCTURE ONLY, like oracle_lib / f32_lib: built on first use with g++ -O2 -ffp-contract=off and loaded through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "crafted_oracle.cpp")
LIB = os.path.join(ROOT, "tests", "cxx", "libcraftedoracle.so")
_lib = None

# bits of Run.state (crafted_oracle.cpp, cro_out.state): what sample n met
ST_MASK, ST_DCD, ST_SECOND_HALF, ST_WINDOW, ST_THROUGH = 7, 8, 16, 32, 64
UNLOCKED, LSF_SYNC, STREAM_SYNC, PACKET_SYNC, BERT_SYNC, SYNC_WAIT, FRAME = range(7)


class _Out(C.Structure):
    _fields_ = [("recs", C.c_void_p), ("cap", C.c_size_t), ("count", C.c_void_p), ("diag", C.c_void_p), ("log", C.c_void_p), ("log_cap", C.c_size_t),
                ("log_count", C.c_void_p), ("sym_pos", C.c_void_p), ("sym", C.c_void_p), ("sym_cap", C.c_size_t), ("sym_count", C.c_void_p),
                ("lev_pos", C.c_void_p), ("lev", C.c_void_p), ("lev_cap", C.c_size_t), ("lev_count", C.c_void_p), ("state", C.c_void_p),
                ("cidx", C.c_void_p), ("limit", C.c_void_p), ("trig", C.c_void_p), ("y", C.c_void_p)]


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(ol.ORACLE_DIR, f) for f in os.listdir(ol.ORACLE_DIR) if f.endswith((".hpp", ".inc"))]
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", SRC, "-o", tmp], check=True)
            os.replace(tmp, LIB)
        _lib = C.CDLL(LIB)
    return _lib


# ---- taps ----------------------------------------------------------------------------------------------------------------------------------
def pad150(taps149):
    t = np.zeros(150, dtype=np.float32)
    t[:149] = np.asarray(taps149, dtype=np.float32)
    return t


def delta(k):
    t = np.zeros(149, dtype=np.float32)
    t[k] = 1.0
    return t


IDENTITY = delta(0)


def ramp():
    """149 distinct small integers, none the mirror image of another: tap i = i + 1."""
    return np.arange(1, 150, dtype=np.float32)


def random_taps(seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, 149).astype(np.float32)


def tilted_rrc():
    """h'[i] = fl32(h[i] (1 + 0.02 (i - 74) / 74)): the matched filter all but unchanged, and no two mirrored taps equal."""
    h = ol.taps()[:149].astype(np.float64)
    return (h * (1.0 + 0.02 * (np.arange(149) - 74) / 74.0)).astype(np.float32)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------------
def scale(s):
    s = np.ascontiguousarray(s, dtype=np.int16)
    out = np.zeros(s.shape, dtype=np.float32)
    lib().cro_scale(ol._p(s), C.c_size_t(s.size), ol._p(out))
    return out


def fir(x, taps149, invert=None):
    """Fir150 with these taps over every row of float32 x[C][T] (state starts at zero); invert: None or one flag per channel (the sample negated)."""
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    t = pad150(taps149)
    inv = None if invert is None else np.ascontiguousarray(np.broadcast_to(np.asarray(invert, dtype=np.uint8), (x.shape[0],)))
    y = np.zeros_like(x)
    lib().cro_fir(ol._p(x), C.c_size_t(x.shape[0]), C.c_size_t(x.shape[1]), ol._p(t), None if inv is None else ol._p(inv), ol._p(y))
    return y


class Run:
    """What demod_batch hands back: recs[C][cap], counts[C], diags[C], log[C][lcap], log_counts[C] and, with taps=True, the taps into the machine."""

    def frames(self):
        return np.concatenate([self.recs[c, : self.counts[c]] for c in range(self.recs.shape[0])])

    def logs(self, c):
        return self.log[c, : self.log_counts[c]]

    def symbols(self, c):
        n = self.sym_counts[c]
        return self.sym_pos[c, :n], self.sym[c, :n, 0], self.sym[c, :n, 1]

    def levels(self, c):
        n = self.lev_counts[c]
        return self.lev_pos[c, :n], self.lev[c, :n]


def demod_batch(x, taps149=None, invert=None, threads=16, taps=False):
    """x[C][T] float32 or int16 through the oracle's demodulator whose Fir150 holds taps149 (None: the RRC taps)."""
    x = np.ascontiguousarray(x)
    assert x.ndim == 2 and x.dtype in (np.float32, np.int16)
    Cn, T = x.shape
    r = Run()
    cap, lcap = 2 * (T // 1920 + 2) + 4, T // 384 + 2
    r.recs, r.counts, r.diags = np.zeros((Cn, cap), dtype=ol.FRAME_REC), np.zeros(Cn, dtype=np.uint32), np.zeros(Cn, dtype=ol.DIAG)
    r.log, r.log_counts = np.zeros((Cn, lcap), dtype=ol.DIAG), np.zeros(Cn, dtype=np.uint32)
    o = _Out()
    o.recs, o.cap, o.count, o.diag, o.log, o.log_cap, o.log_count = ol._p(r.recs), cap, ol._p(r.counts), ol._p(r.diags), ol._p(r.log), lcap, ol._p(r.log_counts)
    step = np.zeros(16, dtype=np.uint64)
    step[:5] = (cap, 1, 1, lcap, 1)
    if taps:
        scap = vcap = T // 10 + 2
        r.sym_pos, r.sym, r.sym_counts = np.zeros((Cn, scap), np.uint32), np.zeros((Cn, scap, 2), np.float32), np.zeros(Cn, np.uint32)
        r.lev_pos, r.lev, r.lev_counts = np.zeros((Cn, vcap), np.uint32), np.zeros((Cn, vcap, 4), np.float32), np.zeros(Cn, np.uint32)
        r.state, r.cidx = np.zeros((Cn, T), np.uint8), np.zeros((Cn, T), np.uint8)
        r.limit, r.trig, r.y = np.zeros((Cn, T), np.float32), np.zeros((Cn, T, 4), np.float32), np.zeros((Cn, T), np.float32)
        o.sym_pos, o.sym, o.sym_cap, o.sym_count = ol._p(r.sym_pos), ol._p(r.sym), scap, ol._p(r.sym_counts)
        o.lev_pos, o.lev, o.lev_cap, o.lev_count = ol._p(r.lev_pos), ol._p(r.lev), vcap, ol._p(r.lev_counts)
        o.state, o.cidx, o.limit, o.trig, o.y = ol._p(r.state), ol._p(r.cidx), ol._p(r.limit), ol._p(r.trig), ol._p(r.y)
        step[5:] = (scap, 2 * scap, 1, vcap, 4 * vcap, 1, T, T, T, 4 * T, T)
    t = None if taps149 is None else pad150(taps149)
    inv = None if invert is None else np.ascontiguousarray(np.broadcast_to(np.asarray(invert, dtype=np.uint8), (Cn,)))
    lib().cro_demod_batch(ol._p(x), C.c_int(int(x.dtype == np.int16)), C.c_size_t(Cn), C.c_size_t(T), None if t is None else ol._p(t),
                          None if inv is None else ol._p(inv), C.c_int(threads), C.byref(o), ol._p(step))
    assert (r.counts <= cap).all() and (r.log_counts <= lcap).all()
    if taps:
        assert (r.sym_counts <= scap).all() and (r.lev_counts <= vcap).all()
    return r


# ---- trigger runs ----------------------------------------------------------------------------------------------------------------------------
def trigger_runs(trig):
    """[(first, last)] of the maximal stretches of consecutive samples with trig != 0 (one sync word's triggered() per sample)."""
    nz = np.flatnonzero(trig != 0)
    if nz.size == 0:
        return []
    cut = np.flatnonzero(np.diff(nz) > 1)
    first = np.concatenate([[nz[0]], nz[cut + 1]])
    last = np.concatenate([nz[cut], [nz[-1]]])
    return list(zip(first.tolist(), last.tolist()))


# ---- a stream fed in runs: the oracle's records and callbacks, run by run ------------------------------------------------------------------
def pieces(r, ends):
    """Per run k = samples [ends[k-1], ends[k]): (records of every channel in channel order, callbacks per channel as a list, counts[C])."""
    Cn = r.recs.shape[0]
    out, lo = [], 0
    for hi in ends:
        recs, logs = [], []
        for c in range(Cn):
            a = r.recs[c, : r.counts[c]]
            recs.append(a[(a["sample_pos"] >= lo) & (a["sample_pos"] < hi)])
            l = r.logs(c)
            pos = l["pad"][:, 0].astype(np.uint64) | (l["pad"][:, 1].astype(np.uint64) << np.uint64(32))
            logs.append(l[(pos >= lo) & (pos < hi)])
        out.append((np.concatenate(recs), logs, np.array([l.size for l in logs], dtype=np.uint32)))
        lo = hi
    return out


INT_FIELDS = ("dcd", "locked", "sample_index", "sync_index", "clock_index", "viterbi_cost", "n_diag", "demod_state", "n_frames")
FLOAT_FIELDS = ("evm", "deviation", "offset", "clock", "dcd_level")


def diag_mismatch(got, exp, fields=INT_FIELDS + ("pad",)):
    """None when two m17_diag arrays agree (integers equal, floats equal as words or both NaN), else (field, indices)."""
    if got.tobytes() == exp.tobytes():
        return None
    if got.size != exp.size:
        return "size", [got.size, exp.size]
    for f in fields:
        bad = got[f] != exp[f]
        if bad.any():
            return f, np.flatnonzero(bad.reshape(got.size, -1).any(axis=1))[:16].tolist()
    for f in FLOAT_FIELDS:
        same = (got[f].view(np.uint32) == exp[f].view(np.uint32)) | (np.isnan(got[f]) & np.isnan(exp[f]))
        if not same.all():
            return f, np.flatnonzero(~same)[:16].tolist()
    return None


def check_run(ctx, recs, logs, counts, room, what):
    """The context's latest run against one piece: records as bytes, every callback of the diagnostic log (tune(9, room) before the run)."""
    got = ctx.frames()
    if got.tobytes() != recs.tobytes():
        chans = np.union1d(got["channel"], recs["channel"])
        bad = [int(c) for c in chans if got[got["channel"] == c].tobytes() != recs[recs["channel"] == c].tobytes()]
        c = bad[0]
        raise AssertionError(f"{what}: records differ ({got.size} fetched / {recs.size} expected) on {len(bad)} channels {bad[:16]}; channel {c}: "
                             f"{got[got['channel'] == c][['seq', 'sample_pos', 'frame_type', 'cost']].tolist()} / "
                             f"{recs[recs['channel'] == c][['seq', 'sample_pos', 'frame_type', 'cost']].tolist()}")
    glog = ctx.diag_log(len(logs), capacity=room)
    n = np.array([l.size for l in glog], dtype=np.uint32)
    if not np.array_equal(n, counts):
        bad = np.flatnonzero(n != counts)
        raise AssertionError(f"{what}: callbacks per channel differ on {bad.size} channels {bad[:16].tolist()}: {n[bad[:16]].tolist()} / {counts[bad[:16]].tolist()}")
    m = diag_mismatch(np.concatenate(glog), np.concatenate(logs))
    if m is not None:
        chan = np.repeat(np.arange(len(glog)), n)
        raise AssertionError(f"{what}: diagnostic log differs in {m[0]}, channels {np.unique(chan[m[1]]).tolist() if m[0] != 'size' else m[1]}")


def check_stream(ctx, x, r, L, what):
    """x[C][T] through a reset context in consecutive runs of L samples (L >= T: one run), every run against the oracle result r for its samples, then
    the final m17_diag.  The diagnostic log's room is set here and put back to 0."""
    Cn, T = x.shape
    ends = list(range(L, T, L)) + [T] if L < T else [T]
    room = min(L, T) // 384 + 3
    ctx.tune(9, room)
    try:
        ctx.reset()
        lo = 0
        for k, (recs, logs, counts) in enumerate(pieces(r, ends)):
            ctx.upload(x[:, lo:ends[k]])
            ctx.run()
            check_run(ctx, recs, logs, counts, room, f"{what}, run {k} of {len(ends)}")
            lo = ends[k]
        m = diag_mismatch(ctx.diag(Cn), r.diags, INT_FIELDS)
        assert m is None, f"{what}: final m17_diag differs in {m[0]}, channels {m[1]}"
    finally:
        ctx.tune(9, 0)


# ---- the whole chain with a tilted RRC: two bursts with a carrier-off stretch between them -----------------------------------------------------------
TILT_C, TILT_T = 32, 72000
_cache = {}


def _once(key, make):
    if key not in _cache:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def tilted_input():
    """Burst, noise that loses the sync, second burst (tests/test_gpu_parity.py::test_full_chain_two_bursts_across_segments)."""
    def make():
        a = ol.generate_batch(ol.gen_params(seed=61, kind=-1, n_frames=6, lead_in=3072, noise_sigma=500.0, tail_sigma=2500.0, lead_sigma=40000.0,
                                            total=36000), TILT_C, 36000, threads=8)
        b = ol.generate_batch(ol.gen_params(seed=62, kind=-1, n_frames=8, lead_in=2000, noise_sigma=500.0, tail_sigma=500.0, lead_sigma=2500.0,
                                            total=36000), TILT_C, 36000, threads=8)
        return np.concatenate([a, b], axis=1)
    return _once("tilt_x", make)


def tilted_oracle():
    """The oracle with the tilted taps on tilted_input() (the int16 rows; tests/test_crafted.py asserts that f32_lib.on_grid of them gives the same)."""
    return _once("tilt_r", lambda: demod_batch(tilted_input(), tilted_rrc(), taps=True))


def gate_reopens(r, c):
    """Samples at which channel c's gate opens again after having closed (dcd_ 0 -> 1 behind a 1 -> 0)."""
    d = (r.state[c] & ST_DCD) != 0
    on = np.flatnonzero(d[1:] & ~d[:-1]) + 1
    off = np.flatnonzero(~d[1:] & d[:-1]) + 1
    return on[on > off[0]] if off.size else on[:0]


# ---- crafted matched-filter output: identity taps on a float32 stream ------------------------------------------------------------------------------
# Rows of at most 48 000 samples, at most 64 to a batch.  A row starts as the matched filter's own output on a generated transmission ("natural") and a
# batch then overwrites the stretch it is about, so acquisition, carrier detect and the limit filter are a real signal's.
CR_T = 48000
LEAD_GAIN = np.float32(4.0)
# (seed, generator kind, preambles, frames, lead-in): found by a search over seeds 1 .. 420 x five (kind, preambles) pairs for transmissions whose crafted
# row decodes, with the identity taps, to the frames the RRC chain decodes from the transmission itself (test_crafted.py asserts it): 24 packets with FCS,
# 24 BERT, 16 streams.  About one candidate in eight does: the carrier detect, fed the filtered row, opens elsewhere and the preamble search starts on
# another sample.
NATURAL = [(7, 4, 1, 8, 3401), (10, 4, 1, 7, 3542), (12, 4, 1, 5, 3636), (24, 4, 1, 5, 4200), (46, 4, 1, 7, 4059), (50, 4, 1, 7, 3072), (56, 4, 1, 5, 3354),
           (58, 4, 1, 7, 3448), (60, 4, 1, 5, 3542), (71, 4, 1, 8, 4059), (72, 4, 1, 5, 4106), (73, 4, 1, 6, 4153), (74, 4, 1, 7, 4200), (80, 4, 1, 5, 3307),
           (82, 4, 1, 7, 3401), (90, 4, 1, 7, 3777), (94, 4, 1, 7, 3965), (97, 4, 1, 6, 4106), (101, 4, 1, 6, 3119), (103, 4, 1, 8, 3213), (105, 4, 1, 6, 3307),
           (109, 4, 1, 6, 3495), (112, 4, 1, 5, 3636), (114, 4, 1, 7, 3730), (25, 0, 3, 6, 3072), (35, 0, 3, 8, 3542), (52, 0, 3, 5, 3166), (79, 0, 3, 8, 3260),
           (81, 0, 3, 6, 3354), (92, 0, 3, 5, 3871), (118, 0, 3, 7, 3918), (144, 0, 3, 5, 3965), (148, 0, 3, 5, 4153), (150, 0, 3, 7, 3072), (178, 0, 3, 7, 3213),
           (188, 0, 3, 5, 3683), (231, 0, 3, 8, 3354), (234, 0, 3, 7, 3495), (238, 0, 3, 7, 3683), (243, 0, 3, 8, 3918), (257, 0, 3, 6, 3401), (267, 0, 3, 8, 3871),
           (308, 0, 3, 5, 3448), (317, 0, 3, 6, 3871), (368, 0, 3, 5, 3918), (369, 0, 3, 6, 3965), (397, 0, 3, 6, 4106), (407, 0, 3, 8, 3401), (2, 1, 2, 7, 3166),
           (7, 1, 1, 8, 3401), (31, 1, 2, 8, 3354), (56, 1, 1, 5, 3354), (60, 1, 1, 5, 3542), (60, 1, 2, 5, 3542), (70, 1, 2, 7, 4012), (71, 1, 1, 8, 4059),
           (71, 1, 2, 8, 4059), (72, 1, 2, 5, 4106), (74, 1, 1, 7, 4200), (75, 1, 2, 8, 3072), (104, 1, 2, 5, 3260), (113, 1, 2, 6, 3683), (114, 1, 1, 7, 3730),
           (123, 1, 2, 8, 4153)]


def natural_params(q):
    seed, kind, npre, nfr, lead_in = q
    return ol.gen_params(seed=seed, kind=kind, n_frames=nfr, lead_in=lead_in, lead_sigma=40000.0, noise_sigma=300.0, n_preamble=npre, total=CR_T)


def natural_tx():
    """int16 transmissions [64][CR_T] and where each burst starts."""
    def make():
        s, b = [], []
        for q in NATURAL:
            x, tr = ol.generate(natural_params(q), with_truth=True)
            s.append(x[:CR_T])
            b.append(tr["burst_start"])
        return np.stack(s), np.array(b)
    return _once("natural_tx", make)


def natural():
    """float32 [64][CR_T]: from the burst's first sample on the matched filter's output on the transmission; in front of it the transmission's own white
    lead-in noise, unfiltered, times LEAD_GAIN.  (White noise keeps the carrier detect off — filtered noise has nothing at 3600 Hz and opens it — and the
    gain leaves the limit filter, which the first 1920 samples prime, near a signal's level; with the lead-in filtered, or at its own level, the sync
    search triggers on the first few symbols of the preamble and next to nothing acquires.)"""
    def make():
        s, b = natural_tx()
        x = scale(s) * LEAD_GAIN
        for c in range(s.shape[0]):
            x[c, b[c]:] = ol.fir_i16(s[c])[b[c]:]
        return x
    return _once("natural", make)


def oracle_of(name):
    """The oracle with the identity taps on batch `name` (a function of this module), taps into the machine included; made once per process."""
    return _once("oracle_" + name, lambda: demod_batch(globals()[name](), IDENTITY, taps=True))


def symbol_grid(r, c):
    """g: channel c's symbol instants are the samples n with n % 10 == g (the generator's clock is the receiver's), read off the oracle's per-symbol
    tap on the natural row."""
    pos = r.symbols(c)[0]
    g = np.bincount(pos % 10, minlength=10).argmax()
    return int(g)


def hold(row, a, b, g, off):
    """Sample and hold over [a, b): every sample of a ten-sample cell takes the row's value at the cell's symbol instant (n % 10 == g); the instant is
    the cell's sample number `off`.  Whole cells only."""
    out = row.copy()
    first = a - ((a - (g - off)) % 10)            # start of the cell that contains a
    for s in range(first, b, 10):
        if s >= 0 and s + 10 <= row.size:
            out[s:s + 10] = row[s + off]
    return out


def held_role(c):
    return 0 if c % 2 == 0 else c % 4


def held_off(c):
    """Which sample of its ten-sample cell the symbol instant is.  For the sync-word channels 4 .. 9: the nine-sample window of a *_SYNC state opens two
    samples before the expected instant, so the cell's falling edge lies inside it only when the cell ends early enough."""
    return 4 + (c // 2) % 6 if held_role(c) == 0 else (c // 4) % 10


def held_plan(c, r):
    """What channel c of the held batch holds: a list of [a, b) over the natural row, from the natural oracle's records (a frame's record fires on its
    last symbol: its sync word lies 1910 .. 1840 samples before, the next one 10 .. 80 behind)."""
    recs = r.recs[c, : r.counts[c]]
    ends = np.unique(recs["sample_pos"].astype(np.int64))
    first = int(ends[0]) - 1910
    role = held_role(c)
    if role == 0:      # every sync word with two symbols on either side
        return [(int(e) - 1930, int(e) - 1820) for e in ends] + [(int(ends[-1]) - 10, int(ends[-1]) + 100)]
    if role == 1:      # the preamble (what lies in front of the first sync word), whole
        return [(first - 1900 * NATURAL[c][2], first - 20)]
    return [(first - 600, first + 100)]   # the end of the preamble and the first sync word: acquisition itself


def held():
    def make():
        x, r = natural().copy(), oracle_of("natural")
        for c in range(x.shape[0]):
            g, off = symbol_grid(r, c), held_off(c)
            for a, b in held_plan(c, r):
                x[c] = hold(x[c], max(a, 0), min(b, CR_T), g, off)
            if held_role(c) != 0:    # the correlator's ring as the gate finds it (the last 80 of the first 1920 samples) zero: the first correlations
                x[c, 1840:1920] = 0.0    # are then the held cells' alone, bit-equal over a cell, and cross the trigger level on a cell's edge
        return x
    return _once("held", make)



def searched(r, c, w):
    """Per sample: does the machine run SyncWord w's search (operator(): the ten-entry buffer, find_peak at the falling edge) on it?  Preamble: the first
    half of do_unlocked; LSF / stream and packet / BERT: its second half and the nine-sample window of STREAM_SYNC resp. PACKET_SYNC and BERT_SYNC.  (EOT
    is only ever asked for triggered().)  From the state each sample met."""
    s = r.state[c]
    st, on = s & ST_MASK, (s & ST_DCD) != 0
    second, window = (s & ST_SECOND_HALF) != 0, (s & ST_WINDOW) != 0
    if w == 0:
        return on & (st == UNLOCKED) & ~second
    if w == 1:
        return on & (((st == UNLOCKED) & second) | ((st == STREAM_SYNC) & window))
    if w == 2:
        return on & (((st == UNLOCKED) & second) | (((st == PACKET_SYNC) | (st == BERT_SYNC)) & window))
    return np.zeros(s.size, dtype=bool)


def searched_runs(r, c, w):
    """The stretches the search of sync word w saw as ONE trigger run on channel c: [(first, last, where)] with `where` = "first" / "second" (half of
    do_unlocked) or "window", by the state that met the sample behind the run (the falling edge, where find_peak runs) — runs whose falling edge the
    search did not see are left out."""
    t, m = r.trig[c, :, w], searched(r, c, w)
    out = []
    for a, b in trigger_runs(np.where(m, t, 0)):
        if b + 1 >= t.size or not m[b + 1] or t[b + 1] != 0:
            continue
        s = r.state[c, b + 1]
        out.append((a, b, "window" if (s & ST_MASK) != UNLOCKED else ("second" if s & ST_SECOND_HALF else "first")))
    return out


# ---- levels: what Correlator::outer_symbol_levels is handed while LSF_SYNC calls it symbol after symbol ----------------------------------------------
LEVEL_KINDS = ("positive", "negative", "average", "zero")


def levels_kind(c):
    return LEVEL_KINDS[c % 4]


def levels_cells(c):
    """The eight cell values channel c writes (times its power of two): all equal and positive (nothing is above hi + lo/2 = 1.5 hi: max_count == 0), all
    equal and negative (everything is above 1.5 lo: min_count == 0), 4 / -2 / 3 (hi + lo/2 == 3: that symbol is neither high nor low), all zero."""
    a = np.float32(2.0 ** ((c // 4) % 5 - 2))
    base = {"positive": [3] * 8, "negative": [-3] * 8, "average": [4, -2, 3, 4, -2, 3, 4, -2], "zero": [0] * 8}[levels_kind(c)]
    return np.array(base, dtype=np.float32) * a


def levels_at(c, r):
    """Where: 300 + 37 (c // 4) samples into channel c's first stay in LSF_SYNC on the natural row (the preamble: no sync word triggers there on eight
    such cells, so update_values runs on every symbol)."""
    st = r.state[c] & ST_MASK
    n0 = int(np.flatnonzero(st == LSF_SYNC)[0])
    return n0 + 300 + 37 * (c // 4)


def levels():
    """The BERT and stream rows of the natural batch (three or two preambles: a long LSF_SYNC) with twelve ten-sample cells overwritten: the eight values
    of levels_cells, the last repeated four times, so the ring's eight symbols at ANY sample index are those values for a few symbols."""
    def make():
        x, r = natural().copy(), oracle_of("natural")
        for c in range(x.shape[0]):
            v = levels_cells(c)
            v = np.concatenate([v, np.roll(v, -8 % 3)[:4] if levels_kind(c) == "average" else v[:4]])
            n = levels_at(c, r)
            x[c, n:n + 10 * v.size] = np.repeat(v, 10)
        return x
    return _once("levels", make)


# ---- small but non-zero: the row decays into the subnormal range and never reaches zero -----------------------------------------------------------
SMALL_FLOORS = (1e-42, 3e-41, 1e-39, 1e-44)


def small():
    """The natural rows times 10^(-k / 300) from sample 16 000 + 37 c on, no magnitude below the channel's floor (1e-42, 3e-41, 1e-39 or 1e-44: all
    subnormal, none zero).  The sliding DFT's state keeps the rounding residue of the loud samples before, so the carrier detect's two sums stay far
    above underflow and the gate stays open while the limit filter's input, history and output go through the subnormal range."""
    def make():
        y = natural().astype(np.float64)
        for c in range(y.shape[0]):
            n0 = 16000 + 37 * c
            y[c, n0:] *= 10.0 ** (-np.arange(CR_T - n0) / 300.0)
            f = SMALL_FLOORS[c % 4]
            low = np.abs(y[c]) < f
            y[c] = np.where(low, np.where(y[c] < 0, -f, f), y[c])
        y = y.astype(np.float32)
        assert (y != 0).all()
        return y
    return _once("small", make)


# ---- exact symbols: the normalised symbols of one frame per channel hit 2, 0, -2, the 43 LLR edges and their neighbours -------------------------------
def llr_edges():
    e, l0, l1 = np.zeros(43, np.float32), np.zeros(43, np.int8), np.zeros(43, np.int8)
    ol.oracle().m17o_llr_table(ol._p(e), ol._p(l0), ol._p(l1))
    return e


def exact_targets():
    """2, 0, -2 (SymbolEvm's thresholds) and the 43 edges of the LLR table, each with the float next to it on either side: 138 values, 3 short of it
    where two lists meet."""
    base = np.concatenate([np.array([2, 0, -2], dtype=np.float32), llr_edges()])
    t = np.concatenate([base, np.nextafter(base, np.float32(np.inf)), np.nextafter(base, np.float32(-np.inf))])
    return np.unique(t.view(np.uint32)).view(np.float32)      # (as words: +0 and the subnormals next to it stay apart)


def exact_params(c):
    """(generator parameters, a) of channel c: BERT on the even channels, a stream on the odd ones, two or three preambles, a = 1/2, 1, 2 or 4."""
    p = ol.gen_params(seed=900 + c, kind=(0, 1)[c % 2], n_frames=6, lead_in=3072 + 13 * c, lead_sigma=40000.0, noise_sigma=0.0,
                      n_preamble=2 + (c // 2) % 2, total=CR_T)
    return p, np.float32(2.0 ** (c % 4 - 1))


def exact_base():
    """Rows written from the symbols themselves: every symbol s of a transmission (tx_build.symbols: preamble, sync words, frames, EOT) as ten samples
    of s a, a a power of two; in front of it the generator's white lead-in x 4 a with samples 1840 .. 1919 zero (the ring as the gate finds it), behind
    it the generator's tail.  Every symbol the level estimator ever looks at is +-3 a, so once a sync word is found through do_unlocked (dev.reset())
    with the ring full of cells, mn == -3 a and mx == 3 a exactly, the Kalman innovations are zero from then on, offset == 0 and idev == 1 / a."""
    def make():
        import tx_build as tb
        x = np.zeros((64, CR_T), dtype=np.float32)
        for c in range(64):
            p, a = exact_params(c)
            s, tr = ol.generate(p, with_truth=True)
            tx = tb.from_truth(p.kind, tr, p.n_frames)
            cells = np.repeat(tb.symbols(tx[0], tx[1], tx[2], p.n_preamble).astype(np.float32) * a, 10)
            x[c] = scale(s[:CR_T]) * np.float32(4.0) * a
            b = tr["burst_start"]
            n = min(cells.size, CR_T - b)
            x[c, b:b + n] = cells[:n]
            x[c, 1840:1920] = 0.0
        return x
    return _once("exact_base", make)


def exact_frames(r, c):
    """The frames (184 symbol positions each, by the oracle's per-symbol tap) of channel c that are sliced under idev == 1 / a and offset == 0 exactly,
    from the level tap: the last update_values before the frame's first symbol, and none inside it."""
    a = exact_params(c)[1]
    pos = r.symbols(c)[0].astype(np.int64)
    lp, lv = r.levels(c)
    out = []
    for k in range(pos.size // 184):
        p = pos[184 * k:184 * k + 184]
        i = np.searchsorted(lp, p[0]) - 1
        if i >= 0 and lv[i, 2] == np.float32(1) / a and lv[i, 3] == 0 and np.searchsorted(lp, p[-1], side="right") - 1 == i:
            out.append(p)
    return out


def exact():
    """exact_base() with ONE frame per channel rewritten: the second frame that is sliced under exact levels (exact_frames on the base rows' oracle:
    the machine is causal, so what a frame's symbols are changes nothing before it).  The sample that do_frame slices as symbol j becomes t a with t = target
    (184 c + j) mod n, so the normalised symbol (t a - 0) (1 / a) is t to the bit; what was sent there no longer matters."""
    def make():
        x, r, tg = exact_base().copy(), oracle_of("exact_base"), exact_targets()
        for c in range(64):
            fr = exact_frames(r, c)
            if len(fr) < 2:
                continue
            a = exact_params(c)[1]
            for j, n in enumerate(fr[1].tolist()):
                t = tg[(184 * c + j) % tg.size]
                f = np.float32(t * a)
                if np.float32(f * (np.float32(1) / a)).view(np.uint32) != t.view(np.uint32):
                    continue                      # (a = 1/2 and the smallest subnormal)
                x[c, n] = f
        return x
    return _once("exact", make)


def clock_census(x, taps149=None, threads=16):
    """Per channel (roundings ClockRecovery made, those whose argument is x.5 exactly, the smallest | fraction - 0.5 |) — cro_clock_census."""
    x = np.ascontiguousarray(x)
    assert x.ndim == 2 and x.dtype in (np.float32, np.int16)
    out = np.zeros((x.shape[0], 3), dtype=np.float64)
    t = None if taps149 is None else pad150(taps149)
    lib().cro_clock_census(ol._p(x), C.c_int(int(x.dtype == np.int16)), C.c_size_t(x.shape[0]), C.c_size_t(x.shape[1]), None if t is None else ol._p(t),
                           C.c_int(threads), ol._p(out))
    return out


# ---- clock rounding: ClockRecovery's std::round handed x.5 exactly -----------------------------------------------------------------------------------
# Found by clock_census over 3 x 2048 generated channels (kinds 0, 1, 4; 24.2 million roundings): none among the 2048 BERT channels, 11 stream and 9
# packet channels with one exact x.5 each.  (generator kind, channel of the 2048-channel batch of seed 7000 + kind)
ROUNDING = [(1, c) for c in (219, 496, 690, 956, 1341, 1517, 1655, 1659, 1694, 1876, 1975)] + \
           [(4, c) for c in (1045, 1102, 1293, 1411, 1808, 1848, 1961, 1989, 1991)]


def rounding():
    """int16 [20][CR_T], ordinary generated transmissions for the RRC taps: the channels of ROUNDING, each regenerated alone."""
    def make():
        rows = []
        for kind, c in ROUNDING:
            p = ol.gen_params(seed=7000 + kind, kind=kind, n_frames=12, lead_in=3072, noise_sigma=300.0, tail_sigma=2500.0, lead_sigma=40000.0, total=CR_T)
            rows.append(ol.generate_batch(p, 1, CR_T, threads=1, chan0=c)[0])
        return np.stack(rows)
    return _once("rounding", make)


def rounding_oracle():
    return _once("oracle_rounding", lambda: demod_batch(rounding(), None, taps=True))


# ---- long ties: a constant behind a quiet stretch, in the second half of do_unlocked ------------------------------------------------------------------
LONG_C = 32


def long_plan(c):
    """(sign and size of the constant, its length in samples, the quiet stretch's length)."""
    return np.float32((1, -1)[c % 2] * 5.25 * 2.0 ** ((c // 2) % 3 - 1)), 400 + 10 * (c % 16), 500 + 25 * (c % 7)


def long_ties():
    """A constant correlates with every sync word at 2 x 3 x its size at every sample alike (the LSF word sums to +2, the packet word to -2, the preamble to
    0): far below 31 x the limit of a stationary row, but the limit filter is slow, so behind a quiet stretch the constant stays above the trigger level
    for many samples — ONE trigger run, tied once the ring's eight symbols are all the constant, longer than the ten-entry buffer several times over.
    To meet it in do_unlocked's second half the rows have no preamble: natural row 24 + c % 24 (BERT) from its first frame's end on, moved up to the
    burst's start, so the gate opens on payload and the preamble search runs out after 1920 samples; from sample 6400 on the quiet stretch (the constant 1e-20: non-zero, and nothing correlates),
    the constant, and the row again.  Where the run on the tiny constant ends the search has found a "sync word" on eight equal symbols: dev.reset() and
    update_values with mn == mx, idev infinite (tests/test_crafted.py asserts it: change long_plan with that test in view)."""
    def make():
        nat, r = natural(), oracle_of("natural")
        b = natural_tx()[1]
        x = np.zeros((LONG_C, CR_T), dtype=np.float32)
        for c in range(LONG_C):
            n = 24 + c % 24
            first = int(r.recs[n, 0]["sample_pos"])
            x[c] = nat[n]
            body = nat[n, first:]
            x[c, b[n]:b[n] + body.size] = body
            x[c, b[n] + body.size:] = nat[n, CR_T - (CR_T - b[n] - body.size):] if b[n] + body.size < CR_T else 0
            v, length, quiet = long_plan(c)
            x[c, 6400:6400 + quiet] = np.float32(1e-20)
            x[c, 6400 + quiet:6400 + quiet + length] = v
        return x
    return _once("long_ties", make)
