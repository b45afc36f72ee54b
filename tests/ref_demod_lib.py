"""The REFERENCE's own demodulator beside the oracle (TEST INFRASTRUCTURE ONLY, numpy and ctypes only): the helper of tests/test_ref_demod.py,
tests/test_gpu_ref_demod.py and tests/golden/make_golden.py.

oracle/Makefile compiles, where the reference is present, mobilinkd::M17Demodulator<float> as it lies over this project's blaze stand-in
(oracle/blaze_min) into oracle/_ref/m17ref_demod_o<k>, one program per evaluation order k = 0 .. 7 of the Kalman products, and the reference's
ClockRecovery / FreqDevEstimator into oracle/_ref/libm17ref_kalman_o<k>.so.  ref_demod() runs such a program on one channel (one process per channel:
the reference keeps `initializing` and its EOT flag in function statics) and returns every frame callback and every diagnostic callback; oracle_demod()
returns the same from the oracle switched to the same order.  What the reference's callbacks do not carry (sync_type; dcd_level, demod_state, n_frames)
is 0 on the reference's side and masked on the oracle's.

The input set: channel(family, idx) names one int16 row and its polarity; FAMILIES lists the channels each family contributes (docstring of each entry).
Where oracle/_ref is absent the same comparison runs against tests/golden/ref_demod_vectors.npz (FIXTURE_CHANNELS, recorded by make_golden.py)."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

import boundary_phases as bp
import crafted_lib as cl
import off_clock as oc
import oracle_lib as ol
import spliced as sp

REF_DIR = os.path.join(ol.ORACLE_DIR, "_ref")
GOLDEN = os.path.join(ol.ROOT, "tests", "golden", "ref_demod_vectors.npz")
ORDERS = tuple(range(8))
MASKED_DIAG = ("dcd_level", "demod_state", "n_frames")      # no arguments of the reference's diagnostic callback
FIX_T = 96000                                                 # every fixture row is this long (shorter rows: quiet noise behind them, pad_row)


def have_ref():
    return all(os.path.exists(os.path.join(REF_DIR, f"m17ref_demod_o{k}")) and os.path.exists(os.path.join(REF_DIR, f"libm17ref_kalman_o{k}.so"))
               for k in ORDERS)


# ---- the demodulators ------------------------------------------------------------------------------------------------------------------------
def parse(blob):
    nf, nd = (int(v) for v in np.frombuffer(blob[:16], dtype="<u8"))
    assert len(blob) == 16 + 64 * (nf + nd)
    return (np.frombuffer(blob[16:16 + 64 * nf], dtype=ol.FRAME_REC).copy(), np.frombuffer(blob[16 + 64 * nf:], dtype=ol.DIAG).copy())


def ref_demod(x, invert, order, tmp=None):
    """(frame records, diagnostic log) of the reference's demodulator built for `order` over one int16 row."""
    x = np.ascontiguousarray(x, dtype=np.int16)
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        a, b = os.path.join(d, "in.i16"), os.path.join(d, "out.bin")
        x.tofile(a)
        subprocess.run([os.path.join(REF_DIR, f"m17ref_demod_o{order}"), a, str(int(invert)), b], check=True)
        with open(b, "rb") as f:
            return parse(f.read())


def ref_demod_many(rows, inverts, order):
    return oc.par(lambda i: ref_demod(rows[i], inverts[i], order), range(len(rows)))


class oracle_order:
    """with oracle_order(k): the oracle's Kalman products in order k; 3, the default, behind it."""

    def __init__(self, order):
        self.order = order

    def __enter__(self):
        ol.oracle().m17o_set_kalman_order(C.c_int(self.order))

    def __exit__(self, *a):
        ol.oracle().m17o_set_kalman_order(C.c_int(3))


def mask_recs(recs):
    r = recs.copy()
    r["channel"] = 0
    r["sync_type"] = 0
    return r


def mask_log(log):
    g = log.copy()
    for f in MASKED_DIAG:
        g[f] = 0
    return g


def masked(pair):
    """(records, log) cut down to what the reference's callbacks carry."""
    return mask_recs(pair[0]), mask_log(pair[1])


def oracle_demod(x, invert):
    """(frame records, diagnostic log) of the oracle under the order in force, as the oracle gives them (masked() before comparing with the reference)."""
    x = np.ascontiguousarray(x, dtype=np.int16)
    recs, _ = ol.demod(x, invert=int(invert), cap=2 * (x.size // 1920 + 2) + 4)
    return recs, ol.demod_diag_log(x, invert=int(invert), cap=x.size // 384 + 2)


def oracle_demod_many(rows, inverts, order):
    with oracle_order(order):
        return oc.par(lambda i: oracle_demod(rows[i], inverts[i]), range(len(rows)))


def first_difference(got, exp):
    """A short description of where two (records, log) pairs differ, or None."""
    for what, a, b in (("records", got[0], exp[0]), ("diagnostics", got[1], exp[1])):
        if a.tobytes() == b.tobytes():
            continue
        if a.size != b.size:
            return f"{what}: {a.size} against {b.size}"
        i = next(i for i in range(a.size) if a[i].tobytes() != b[i].tobytes())
        f = [n for n in a.dtype.names if a[i][n].tobytes() != b[i][n].tobytes()]
        return f"{what}[{i}] fields {f}: {[a[i][n].tolist() for n in f]} against {[b[i][n].tolist() for n in f]}"
    return None


# ---- the input set -----------------------------------------------------------------------------------------------------------------------------
SILENT_LEAD = 4000
BP_STRIDE = dict(stream=7, bert=7, packet=7, mixed=3, hole=1)          # odd strides: the batches treat even and odd channels differently


def silent_row():
    """DataCarrierDetect's 0 / 0: silence first, then a transmission (tests/test_oracle_vs_ref.py's carrier-detect case)."""
    p = ol.gen_params(seed=5, kind=1, n_frames=6, lead_in=3072, noise_sigma=300.0, tail_sigma=300.0, lead_sigma=40000.0, total=30000)
    return np.concatenate([np.zeros(SILENT_LEAD, np.int16), ol.generate(p)[:30000]])


def _bp_row(name, c):
    if name == "hole":
        return bp._hole_channel(c)
    if name == "mixed":
        x = _bp_row("stream", c)
        return oc.negated(x) if bp.polarity()[c] else x
    kind, nf, _, seeds = bp.KINDS[name]
    return bp._gen(seeds[c & 1], kind, nf[c & 1], 3072 + c)[:bp.T]


def _sp_row(name, c):
    fn, seed_of = sp.CHANNEL[name]
    seeds = sp.SEEDS[name]
    return fn(c, seeds[c] if seed_of is None else seed_of(c, seeds))["x"]


def channel(family, idx):
    """(int16 row, polarity) of channel `idx` of `family`, made alone (no whole batch is built for one row, except off_clock's, which are cached)."""
    if family == "random":
        return ol.random_scenario(idx), idx & 1
    if family.startswith("bp_"):
        name = family[3:]
        return _bp_row(name, idx), int(bp.polarity()[idx]) if name == "mixed" else 0
    if family.startswith("sp_"):
        return _sp_row(family[3:], idx), 0
    if family == "oc_main":
        y, pol = oc.main_mixed_polarity()
        return y[idx], int(pol[idx])
    if family == "oc_bursty":
        return oc.bursty()[0][idx], 0
    if family == "cr_rounding":
        kind, c = cl.ROUNDING[idx]
        p = ol.gen_params(seed=7000 + kind, kind=kind, n_frames=12, lead_in=3072, noise_sigma=300.0, tail_sigma=2500.0, lead_sigma=40000.0, total=cl.CR_T)
        return ol.generate_batch(p, 1, cl.CR_T, threads=1, chan0=c)[0], 0
    if family == "silent":
        return silent_row(), 0
    raise KeyError(family)


# family -> the channels it contributes.  random: the hybrid test's 240 scenarios.  bp_*: every BP_STRIDE-th channel of tests/boundary_phases.py's
# batches (tests/test_ref_demod.py repeats on the subset what tests/test_boundary_phases.py asserts on the whole).  sp_*, oc_*, cr_rounding: whole
# batches, so what tests/test_spliced.py, tests/test_off_clock.py and tests/test_crafted.py assert of them holds as it stands.
FAMILIES = dict(
    random=tuple(range(240)),
    **{"bp_" + n: tuple(range(0, bp.MIXED_C if n == "mixed" else bp.HOLE_C if n == "hole" else bp.C, s)) for n, s in BP_STRIDE.items()},
    **{"sp_" + n: tuple(range(sp.C)) for n in sp.BATCHES},
    oc_main=tuple(range(oc.MAIN_C)),
    oc_bursty=tuple(range(32)),
    cr_rounding=tuple(range(len(cl.ROUNDING))),
    silent=(0,),
)
OTHER_ORDER_SEEDS = tuple(range(24))            # the six orders that are neither 0 nor 3: random scenarios 0 .. 23


def family_rows(family):
    ch = oc.par(lambda i: channel(family, i), FAMILIES[family])
    return [c[0] for c in ch], [c[1] for c in ch]


# ---- the frozen copy ---------------------------------------------------------------------------------------------------------------------------
# At most 64 channels, some of every family.  bp_hole 60 .. : channels that give up in do_packet_sync (asserted by test_ref_demod).
FIXTURE_CHANNELS = (
    [("random", s) for s in (0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233)] +
    [("bp_stream", 0), ("bp_stream", 1001), ("bp_bert", 8), ("bp_bert", 1537), ("bp_packet", 16), ("bp_packet", 777), ("bp_mixed", 5), ("bp_mixed", 202)] +
    [("bp_hole", c) for c in (0, 14, 19, 23, 27, 31)] +
    [("sp_late", 3), ("sp_late", 25), ("sp_blank", 7), ("sp_blank", 40), ("sp_tail", 11), ("sp_tail", 30)] +
    [("sp_hole", c) for c in (0, 9, 18, 27, 36, 45, 54, 63)] + [("sp_splice", 0), ("sp_splice", 25), ("sp_splice", 41)] +
    [("oc_main", c) for c in (5, 6, 9, 10, 11, 12, 13, 27)] + [("oc_bursty", 2), ("oc_bursty", 19)] +
    [("cr_rounding", c) for c in (0, 5, 11, 19)] + [("silent", 0)]
)
assert len(FIXTURE_CHANNELS) <= 64 and len(set(FIXTURE_CHANNELS)) == len(FIXTURE_CHANNELS)
FIXTURE_ORDERS = (0, 3)


def pad_row(x, idx):
    """A row of FIX_T samples: x, and behind a shorter x quiet noise (sigma 100: the carrier detect sees no silence)."""
    x = np.asarray(x, dtype=np.int16)
    if x.size >= FIX_T:
        return np.ascontiguousarray(x[:FIX_T])
    return np.concatenate([x, sp.noise(424242 + idx, FIX_T - x.size, 100.0)])


_FIX = {}


def fixture_rows():
    """(x [n][FIX_T] int16, polarity [n] uint8) of FIXTURE_CHANNELS, regenerated from their arguments; cached, read-only."""
    if "rows" not in _FIX:
        ch = oc.par(lambda i: channel(*FIXTURE_CHANNELS[i]), range(len(FIXTURE_CHANNELS)))
        x = np.stack([pad_row(c[0], i) for i, c in enumerate(ch)])
        x.setflags(write=False)
        _FIX["rows"] = (x, np.array([c[1] for c in ch], dtype=np.uint8))
    return _FIX["rows"]


def sha256_rows(x):
    return np.array([hashlib.sha256(np.ascontiguousarray(r).tobytes()).hexdigest() for r in x])


def load_fixture():
    """The recorded file as a dict, after checking that the regenerated rows are the recorded ones (a different hash FAILS)."""
    if "npz" not in _FIX:
        z = dict(np.load(GOLDEN, allow_pickle=False))
        x, pol = fixture_rows()
        assert [tuple(v) for v in zip(z["family"].tolist(), z["index"].tolist())] == [(f, int(i)) for f, i in FIXTURE_CHANNELS], "fixture channel list"
        assert z["polarity"].tolist() == pol.tolist()
        got = sha256_rows(x)
        bad = [FIXTURE_CHANNELS[i] for i in range(len(got)) if got[i] != z["sha256"][i]]
        assert not bad, f"regenerated fixture rows differ from the recorded ones: {bad}"
        _FIX["npz"] = z
    return _FIX["npz"]


def fixture_channel(z, order, i):
    """(records, log) the reference's demodulator delivered on fixture row i under `order`."""
    rc, ro = z[f"rec_count_o{order}"], z[f"recs_o{order}"].view(ol.FRAME_REC).reshape(-1)
    lc, lo = z[f"log_count_o{order}"], z[f"log_o{order}"].view(ol.DIAG).reshape(-1)
    a, b = int(rc[:i].sum()), int(lc[:i].sum())
    return ro[a:a + int(rc[i])], lo[b:b + int(lc[i])]


# ---- clock recovery and deviation estimator ----------------------------------------------------------------------------------------------------
_KAL = {}


def kalman_lib(order):
    if order not in _KAL:
        lib = C.CDLL(os.path.join(REF_DIR, f"libm17ref_kalman_o{order}.so"))
        assert lib.ref_kalman_order() == order
        _KAL[order] = lib
    return _KAL[order]


OP_RESET, OP_UPDATE, OP_FREE = 0, 1, 2
CLOCK_COLS = ("sample_index", "clock_estimate", "sample_estimate", "x0", "x1", "P00", "P01", "P10", "P11")
# An exact x.5 for the free-running update: behind reset(3), update(6) after 1920 samples and update(9) after 1920 more, sample_estimate is one float
# under all eight orders and clock_estimate one of three neighbouring floats; sample_estimate + clock_estimate * float(count) is x.5 exactly at the first
# count for two of them and at the second for two (found by scanning counts in numpy; the test recomputes the argument from each order's trace).
HALF_COUNTS = (74650, 54957)


def clock_sequences():
    """Rows of (op, index, count) steps: `count` samples, then the operation (oracle/ref_shim.cpp ref_clock_trace, m17o_clock).  Each row starts with a reset."""
    rng = np.random.default_rng(77)
    rows = []
    # the wrap cases of KalmanFilter::update, all in one row (found by a search over random index sequences; the test reads them off the trace):
    # z - x0 a little below -5 and a little above +5, x0 carried to 10 or above and below 0
    rows.append([(OP_RESET, 7, 0)] + [(OP_UPDATE, i, 1920) for i in (8, 2, 8, 8, 3, 0, 7, 8, 4, 1)])
    rows.append([(OP_RESET, 0, 0), (OP_UPDATE, 7, 1920), (OP_UPDATE, 6, 1920), (OP_UPDATE, 9, 1920), (OP_UPDATE, 4, 1920), (OP_UPDATE, 9, 1920)])
    # dt = 0, 1, 1920, 19 200, and free-running updates between them (count runs on through them)
    rows.append([(OP_RESET, 5, 0), (OP_UPDATE, 5, 0), (OP_UPDATE, 6, 1), (OP_UPDATE, 6, 1920), (OP_FREE, 0, 960), (OP_UPDATE, 7, 960), (OP_UPDATE, 4, 19200),
                 (OP_FREE, 0, 19200), (OP_FREE, 0, 19200), (OP_UPDATE, 2, 1), (OP_UPDATE, 2, 0), (OP_RESET, 1, 77), (OP_FREE, 0, 5), (OP_UPDATE, 0, 1920)])
    # a transmitter that is slow: the index falls by one every other frame, the clock estimate goes negative, and a long free run makes
    # sample_estimate + clock_estimate * count negative (fmod's argument below 0)
    slow = [(OP_RESET, 8, 0)]
    idx = 8
    for i in range(40):
        idx = (idx - (i & 1)) % 10
        slow.append((OP_UPDATE, idx, 1920))
    slow += [(OP_FREE, 0, 192000), (OP_FREE, 0, 1920000), (OP_UPDATE, idx, 1920)]
    rows.append(slow)
    # the exact half
    for n in HALF_COUNTS:
        rows.append([(OP_RESET, 3, 0), (OP_UPDATE, 6, 1920), (OP_UPDATE, 9, 1920), (OP_FREE, 0, n), (OP_UPDATE, 2, 1920)])
    # noisy indices around a drifting one, irregular intervals
    for r in range(4):
        seq, true = [(OP_RESET, int(rng.integers(0, 10)), 0)], float(rng.uniform(0, 10))
        for i in range(120):
            dt = int(rng.choice([1920, 1920, 1920, 960, 3840, 19200, 1, 0]))
            true = (true + dt * (r - 1.5) * 2e-4) % 10
            if rng.random() < 0.2:
                seq.append((OP_FREE, 0, dt))
            else:
                seq.append((OP_UPDATE, int(np.floor(true + rng.normal(0, 0.8))) % 10, dt))
        rows.append(seq)
    # three rows of one shape for the device's kalman_kernel (m17hip_kalman_trace takes one z0 and one length for all rows; three is odd, so the last
    # wave is ragged): reset(4), then 100 update(index) steps and nothing else
    for r in range(3):
        seq, true = [(OP_RESET, 4, 0)], 4.0
        for i in range(100):
            dt = int(rng.choice([1920, 1920, 960, 3840, 19200, 1, 0, 77]))
            true = (true + dt * (r - 1) * 3e-4) % 10
            seq.append((OP_UPDATE, int(np.floor(true + rng.normal(0, 1.0))) % 10, dt))
        rows.append(seq)
    return [np.array(s, dtype=np.int64) for s in rows]


DEVICE_CLOCK_ROWS = (-3, -2, -1)          # of clock_sequences()
DEVICE_DEV_ROWS = (3, 4, 5)               # of dev_sequences()


def _clock_args(seq):
    return (np.ascontiguousarray(seq[:, 0], dtype=np.uint8), np.ascontiguousarray(seq[:, 1], dtype=np.uint8),
            np.ascontiguousarray(seq[:, 2], dtype=np.uint32))


def ref_clock_trace(order, seq):
    """[steps][9] float32 (CLOCK_COLS) of the reference's ClockRecovery<float,10> built for `order`."""
    op, index, count = _clock_args(seq)
    out = np.zeros((op.size, 9), dtype=np.float32)
    kalman_lib(order).ref_clock_trace(ol._p(op), ol._p(index), ol._p(count), C.c_size_t(op.size), ol._p(out))
    return out


def kalman_calls(seq):
    """The KalmanFilter updates a clock sequence makes, per stretch between resets: (z0, step numbers, z, dt) — count runs on through free updates."""
    out, cur, acc = [], None, 0
    for i, (op, index, count) in enumerate(seq.tolist()):
        acc += count
        if op == OP_RESET:
            cur = [float(index), [], [], []]
            out.append(cur)
            acc = 0
        elif op == OP_UPDATE:
            cur[1].append(i); cur[2].append(float(index)); cur[3].append(acc)
            acc = 0
    return [(z0, np.array(st, dtype=np.int64), np.array(z, dtype=np.float32), np.array(dt, dtype=np.uint32)) for z0, st, z, dt in out if st]


def oracle_kalman_trace(z, dt, wrap, z0):
    out = np.zeros((z.size, 6), dtype=np.float32)
    ol.oracle().m17o_kalman_trace(ol._p(np.ascontiguousarray(z)), ol._p(np.ascontiguousarray(dt)), C.c_size_t(z.size), C.c_int(wrap), C.c_float(z0), ol._p(out))
    return out


def oracle_clock_trace(seq):
    """What the oracle's ClockRecovery gives for the same steps: (sample_index [steps] uint8, clock_estimate [steps] float32) from m17o_clock, and the filter's
    state (x0, x1, P) at the update steps from m17o_kalman_trace over kalman_calls(): [(step numbers, [n][6])]."""
    op, index, count = _clock_args(seq)
    si, ce = np.zeros(op.size, dtype=np.uint8), np.zeros(op.size, dtype=np.float32)
    ol.oracle().m17o_clock(ol._p(op), ol._p(index), ol._p(count), C.c_size_t(op.size), ol._p(si), ol._p(ce))
    return si, ce, [(st, oracle_kalman_trace(z, dt, 10, z0)) for z0, st, z, dt in kalman_calls(seq)]


def free_run_arguments(seq, trace):
    """The argument std::fmod gets at each free-running update, recomputed in float32 from the trace: sample_estimate + clock_estimate * float(count),
    count running since the last reset or update(index).  [(step, argument)]"""
    out, acc = [], 0
    se = ce = np.float32(0)
    for i, (op, index, count) in enumerate(seq.tolist()):
        acc += count
        if op == OP_FREE:
            out.append((i, float(np.float32(se + np.float32(ce * np.float32(acc))))))
        else:
            acc = 0
            se, ce = (se, np.float32(0)) if op == OP_RESET else (np.float32(trace[i, 2]), np.float32(trace[i, 1]))
    return out


def dev_sequences():
    """Rows of (mn, mx, reset_before) for FreqDevEstimator::update."""
    rng = np.random.default_rng(78)
    rows = []
    n = 2000                                                     # a slowly drifting pair
    t = np.arange(n)
    mn = (-0.62 + 2e-5 * t + rng.normal(0, 0.01, n)).astype(np.float32)
    mx = (0.58 + 3e-5 * t + rng.normal(0, 0.01, n)).astype(np.float32)
    rows.append((mn, mx, np.zeros(n, dtype=np.uint8)))
    n = 60                                                       # mn == mx at the reset and in the middle of a run: idev infinite
    mn = (-0.6 + rng.normal(0, 0.02, n)).astype(np.float32)
    mx = (0.6 + rng.normal(0, 0.02, n)).astype(np.float32)
    rs = np.zeros(n, dtype=np.uint8)
    mn[0] = mx[0] = np.float32(0.25)
    rs[20] = 1
    mn[20] = mx[20] = np.float32(-0.125)
    rs[40] = 1
    rows.append((mn, mx, rs))
    n = 60                                                       # a NaN level, and an infinite one: reset_ brings the estimator back at the next update
    mn = (-0.5 + rng.normal(0, 0.02, n)).astype(np.float32)
    mx = (0.7 + rng.normal(0, 0.02, n)).astype(np.float32)
    mn[10] = np.nan
    mx[30] = np.inf
    mx[45] = np.nan
    mn[45] = np.nan
    rows.append((mn, mx, np.zeros(n, dtype=np.uint8)))
    # three rows of one shape for the device's kalman_kernel: one first pair (the estimator resets its filters to it), 300 updates, no reset, finite
    n = 300
    for r in range(3):
        mn = (-0.6 + 1e-4 * r * np.arange(n) + rng.normal(0, 0.02 * (r + 1), n)).astype(np.float32)
        mx = (0.6 - 1e-4 * r * np.arange(n) + rng.normal(0, 0.02 * (r + 1), n)).astype(np.float32)
        mn[0], mx[0] = np.float32(-0.59375), np.float32(0.609375)
        rows.append((mn, mx, np.zeros(n, dtype=np.uint8)))
    return rows


DEV_COLS = ("idev", "offset", "deviation")


def ref_dev_trace(order, row):
    mn, mx, rs = (np.ascontiguousarray(a) for a in row)
    out = np.zeros((mn.size, 3), dtype=np.float32)
    kalman_lib(order).ref_dev_trace(ol._p(mn), ol._p(mx), C.c_size_t(mn.size), ol._p(rs), ol._p(out))
    return out


def oracle_dev_trace(row):
    mn, mx, rs = (np.ascontiguousarray(a) for a in row)
    idev, offset = np.zeros(mn.size, dtype=np.float32), np.zeros(mn.size, dtype=np.float32)
    ol.oracle().m17o_freqdev(ol._p(mn), ol._p(mx), C.c_size_t(mn.size), ol._p(rs), ol._p(idev), ol._p(offset))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([idev, offset, (np.float32(2400.0) / idev).astype(np.float32)], axis=1)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))
