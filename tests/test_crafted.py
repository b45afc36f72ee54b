"""CPU-only: the premises of the tap tests (tests/test_gpu_fir_taps.py, tests/test_gpu_crafted.py), asserted on the oracle alone, each with its measured
figure in the message.  The oracle here is tests/cxx/crafted_oracle.cpp: the oracle's demodulator whose Fir150 holds caller-chosen taps — what
m17hip_set_fir_taps (include/m17hip.h, a test hook) makes the device compute — with taps into the machine (every symbol, every update of the level
estimator, per sample the state it met, the limit filter and the sync words' triggered() values)."""
import ctypes as C

import numpy as np

import crafted_lib as cl
import f32_lib as fl
import m17hip
import oracle_lib as ol


# ---- the oracle with taps, and the hook without a device -----------------------------------------------------------------------------------------
def test_the_tap_oracle_with_the_rrc_taps_is_the_oracle():
    x = cl.tilted_input()[:8, :36000]
    r = cl.demod_batch(x, None)
    r2 = cl.demod_batch(x, ol.taps()[:149], taps=True)
    recs, counts, diags = ol.demod_batch(x, cap=r.recs.shape[1], threads=8)
    assert r.recs.tobytes() == recs.tobytes() and r.diags.tobytes() == diags.tobytes() and r.counts.sum() > 8
    assert r2.recs.tobytes() == recs.tobytes() and r2.diags.tobytes() == diags.tobytes()
    for c in range(8):
        assert r.logs(c).tobytes() == ol.demod_diag_log(x[c]).tobytes()
        sym = ol.demod_symbols(x[c])
        assert np.array_equal(r2.symbols(c)[1].view(np.uint32), sym.view(np.uint32)) and sym.size > 100
    xf = fl.on_grid(x)
    rf = cl.demod_batch(xf, None)
    e = fl.demod_batch(xf, threads=8, logs=True)
    assert rf.recs.tobytes() == e[0].tobytes() and rf.diags.tobytes() == e[2].tobytes() and np.array_equal(rf.log_counts, e[4])


def test_fir_with_taps_is_fir150():
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (3, 700)).astype(np.float32)
    assert np.array_equal(cl.fir(x, ol.taps()[:149])[1].view(np.uint32), ol.fir_f32(x[1]).view(np.uint32))
    xi = rng.integers(-15, 16, (2, 700)).astype(np.float32)
    full = np.convolve(xi[0].astype(np.int64), np.arange(1, 150, dtype=np.int64))[:700]
    assert np.array_equal(cl.fir(xi, cl.ramp())[0], full.astype(np.float32))                 # taps[i] multiplies the sample i steps back
    assert np.array_equal(cl.fir(xi, cl.delta(148))[1][148:], xi[1][:700 - 148])
    assert np.array_equal(cl.fir(xi, cl.ramp(), invert=[0, 1])[1], -cl.fir(xi, cl.ramp())[1])
    s = rng.integers(-32767, 32768, 500, dtype=np.int16)
    assert np.array_equal(cl.scale(s).view(np.uint32), ol.scale(s).view(np.uint32))
    assert np.array_equal(cl.fir(cl.scale(s)[None], ol.taps()[:149])[0].view(np.uint32), ol.fir_i16(s).view(np.uint32))


def test_set_fir_taps_refuses_what_it_can_without_a_device():
    lib = m17hip.load_library()
    assert lib.m17hip_version() >= 614 and "m17hip_set_fir_taps" in m17hip.EXPORTS
    t = cl.ramp()
    assert lib.m17hip_set_fir_taps(C.c_void_p(), t.ctypes.data_as(C.c_void_p)) == -1
    assert lib.m17hip_set_fir_taps(C.c_void_p(), None) == -1


def test_tap_sets_are_not_symmetric():
    for name, t in (("ramp", cl.ramp()), ("random", cl.random_taps(6140)), ("tilted", cl.tilted_rrc())):
        eq = int((t == t[::-1]).sum())
        assert eq == 1, (name, eq)                                       # the middle tap alone is its own mirror image
        assert np.unique(t).size == 149, name
    h = ol.taps()
    assert np.array_equal(h[:149], h[:149][::-1]) and h[149] == 0        # ... and the RRC taps are: the blind spot
    assert np.abs(cl.tilted_rrc() / h[:149] - 1).max() <= 0.0201


# ---- whole chain with a tilted RRC ---------------------------------------------------------------------------------------------------------------
def test_tilted_chain_premises():
    x, r = cl.tilted_input(), cl.tilted_oracle()
    Cn = x.shape[0]
    first = np.array([(r.recs[c, :r.counts[c]]["sample_pos"] < 36000).sum() for c in range(Cn)])
    second = np.array([(r.recs[c, :r.counts[c]]["sample_pos"] >= 36000).sum() for c in range(Cn)])
    assert (first > 0).sum() >= 28 and (second > 0).sum() >= 28, ((first > 0).sum(), (second > 0).sum())       # measured: 30 and 31 of 32
    assert first.sum() > 4 * Cn and second.sum() > 4 * Cn, (first.sum(), second.sum())                             # measured: 376 and 270
    reopen = sum(cl.gate_reopens(r, c).size > 0 for c in range(Cn))
    assert reopen >= Cn // 2, reopen                                                                                # measured: 32 of 32
    # ... behind a carrier-off UPDATE POINT: the gate closes on a 960-sample point of the locked chain and opens on a 384-sample point
    # the float form of the rows is the same stream
    rf = cl.demod_batch(fl.on_grid(x), cl.tilted_rrc())
    assert rf.recs.tobytes() == r.recs.tobytes() and rf.diags.tobytes() == r.diags.tobytes() and rf.log.tobytes() == r.log.tobytes()
    # and the tilt is seen: not the RRC's records
    recs, counts, _ = ol.demod_batch(x, cap=r.recs.shape[1], threads=8)
    assert recs.tobytes() != r.recs.tobytes()


# ---- crafted rows: natural -------------------------------------------------------------------------------------------------------------------------
def _same_frames(a, b):
    return a.size == b.size and np.array_equal(a["frame_type"], b["frame_type"]) and np.array_equal(a["payload"], b["payload"])


def test_natural_rows_decode_to_the_transmissions_frames():
    s, _ = cl.natural_tx()
    ra = cl.demod_batch(s, None)
    rb = cl.oracle_of("natural")
    same = [c for c in range(64) if _same_frames(ra.recs[c, :ra.counts[c]], rb.recs[c, :rb.counts[c]]) and rb.counts[c] >= 5]
    assert len(same) == 64, (len(same), [c for c in range(64) if c not in same])
    kinds = np.array([q[1] for q in cl.NATURAL])
    assert (kinds == 4).sum() == 24 and (kinds == 0).sum() == 24 and (kinds == 1).sum() == 16
    assert rb.counts.sum() >= 400, rb.counts.sum()
    top = np.array([rb.logs(c)["dcd_level"].max() for c in range(64)])
    assert top.min() > 4.0, (top.min(), np.median(top))                # the carrier detect, fed the filtered row, opens on every channel (trigger: 4)
    print("natural: median over channels of the highest dcd_level", np.median(top))
    assert np.array_equal(rb.y[0][rb.state[0] & cl.ST_THROUGH != 0], cl.natural()[0][rb.state[0] & cl.ST_THROUGH != 0])   # identity: y[n] == x[n]


# ---- crafted rows: held ----------------------------------------------------------------------------------------------------------------------------
def _held_census():
    """Per sync word: the tied runs the search saw (two samples or more, every |v| the same word): (channel, first, last, where, sign, crosses 9 -> 0)."""
    r = cl.oracle_of("held")
    out = {0: [], 1: [], 2: []}
    longest = 0
    for w in out:
        for c in range(64):
            for a, b, where in cl.searched_runs(r, c, w):
                v = r.trig[c, a:b + 1, w]
                longest = max(longest, b - a + 1)
                if b > a and np.unique(np.abs(v).view(np.uint32)).size == 1:
                    out[w].append((c, a, b, where, bool(v[0] > 0), bool((np.diff(r.cidx[c, a:b + 1].astype(int)) < 0).any())))
    return out, longest


def test_held_rows_tie_the_sync_search():
    """Sample and hold over the sync words (even channels) and over the preamble or its end (odd channels): every correlation of a ten-sample cell is the
    same word, so find_peak's strict > on fabs, scanned in buffer order 0 .. 9, decides by ORDER alone.  What the issue asks beside that and this batch
    does not reach — the longest run the search sees here is eleven samples and not tied (a held cell is ten, the window nine), none ends in do_unlocked's
    second half, and the two-signed words tie on their negative side only — is asserted on the long-ties batch:
    test_long_rows_tie_runs_far_longer_than_the_buffer_in_the_second_half."""
    census, longest = _held_census()
    r = cl.oracle_of("held")
    pre, lsf, pkt = census[0], census[1], census[2]
    print("held: tied runs seen by the search: preamble", len(pre), "LSF / stream", len(lsf), "packet / BERT", len(pkt), "longest searched run", longest)
    assert len(pre) >= 5 and all(q[3] == "first" for q in pre), len(pre)                     # measured: 10, all in do_unlocked's first half
    assert len(lsf) >= 5 and len(pkt) >= 10, (len(lsf), len(pkt))                            # measured: 15 and 33, all in a *_SYNC window
    crossing = [q for q in lsf + pkt if q[5]]
    assert len(crossing) >= 10, len(crossing)                                                # measured: 22: the winner is buffer entry 0, not the first in time
    window = {q[0] for q in lsf + pkt if q[3] == "window"}
    assert len(window) >= 64 // 4, len(window)                                               # measured: 16 of 64
    full = [q for q in pre if q[2] - q[1] + 1 == 10]
    assert len(full) >= 1, len(full)                                                         # a whole cell of ten tied samples: every buffer entry the same
    assert r.counts.sum() >= 400 and (r.counts > 0).sum() >= 48, (r.counts.sum(), (r.counts > 0).sum())   # measured: 560 records on 55 channels
    # the ties change what is decoded: not the natural batch's records
    assert r.recs.tobytes() != cl.oracle_of("natural").recs.tobytes()


# ---- crafted rows: levels --------------------------------------------------------------------------------------------------------------------------
def test_level_rows_reach_the_estimators_fallbacks():
    """Eight equal positive symbols (max_count == 0: mx falls back to hi), eight equal negative ones (min_count == 0), eight zeros, and 4 / -2 / 3 times a
    power of two (hi + lo/2. == 3: that symbol is neither high nor low, so mn == -2 and mx == 4 exactly — with >= it would be counted high and mx 3.75):
    seen by update_values in LSF_SYNC, from the oracle's tap on it.  (idev stays finite here: in LSF_SYNC it comes from the two Kalman states.  The
    issue's "mn == mx, idev infinite" needs the update behind a dev.reset(): test_long_rows_reach_an_infinite_idev_while_locked.)"""
    r, rn = cl.oracle_of("levels"), cl.oracle_of("natural")
    hit = {k: 0 for k in cl.LEVEL_KINDS}
    for c in range(64):
        pos, lv = r.levels(c)
        n, v = cl.levels_at(c, rn), cl.levels_cells(c)
        m = lv[(pos >= n) & (pos < n + 130)]
        if cl.levels_kind(c) == "average":
            a = v[0] / np.float32(4)
            hit["average"] += bool(((m[:, 0] == -2 * a) & (m[:, 1] == 4 * a)).any())
        else:
            hit[cl.levels_kind(c)] += bool(((m[:, 0] == v[0]) & (m[:, 1] == v[0])).any())
    print("levels: channels on which update_values saw the crafted level set:", hit)
    assert all(n >= 12 for n in hit.values()), hit                        # measured: positive 13, negative 16, average 14, zero 16 of 16 each
    assert r.counts.sum() >= 400, r.counts.sum()                           # measured: 624 (the transmissions still decode behind the stretch)


# ---- crafted rows: exact symbols ---------------------------------------------------------------------------------------------------------------------
def test_exact_rows_put_every_threshold_and_edge_under_the_slicer():
    """Rows written from the symbols as ten-sample cells of s a, a a power of two: behind an acquisition through do_unlocked the outer levels are +-3 a
    exactly, offset == 0 and idev == 1 / a (from the oracle's tap on update_values), and one frame per channel is rewritten so that its normalised
    symbols are 2, 0, -2 (SymbolEvm's thresholds), the 43 LLR edges and the float next to each on either side — read back from the per-symbol tap."""
    rb, r, tg = cl.oracle_of("exact_base"), cl.oracle_of("exact"), cl.exact_targets()
    assert tg.size == 134                                                  # 46 x 3, less the four words that two of the lists share
    used = [c for c in range(64) if len(cl.exact_frames(rb, c)) >= 2]
    assert len(used) >= 32, len(used)                                      # measured: 45 of 64 channels have two frames under exact levels
    w = np.concatenate([r.symbols(c)[1].view(np.uint32) for c in range(64)])
    seen = np.array([(w == t.view(np.uint32)).sum() for t in tg])
    print("exact: channels rewritten", len(used), "; each of the", tg.size, "targets occurs at least", seen.min(), "times")
    assert seen.min() >= 1, tg[seen == 0].tolist()                         # measured: at least 54 times each
    wb = np.concatenate([rb.symbols(c)[1].view(np.uint32) for c in range(64)])
    hit_before = sum(bool((wb == t.view(np.uint32)).any()) for t in tg)
    assert hit_before <= 8, hit_before                                     # measured: 3 (0, -1 and 3 - 2^-22 occur in the unrewritten rows)
    assert r.counts.sum() >= 300, r.counts.sum()                           # measured: 582 records (703 before the rewriting)


# ---- crafted rows: small but non-zero ---------------------------------------------------------------------------------------------------------------
def test_small_rows_take_the_limit_filter_through_the_subnormal_range_with_the_gate_open():
    x, r = cl.small(), cl.oracle_of("small")
    assert (x != 0).all() and ((np.abs(x) < 1.1754944e-38).sum(axis=1) > 10000).all()
    sub = np.array([((np.abs(r.limit[c]) < 1.1754944e-38) & (r.limit[c] != 0) & ((r.state[c] & cl.ST_DCD) != 0)).sum() for c in range(64)])
    print("small: samples with a subnormal, non-zero limit while dcd is 1, per channel: min", sub.min(), "median", np.median(sub))
    assert (sub >= 5000).all(), sub.min()                                  # measured: 20 000 and more on the channels looked at; 5000 = some 2.6 frames
    late = np.array([np.isfinite(r.logs(c)["dcd_level"][-20:]).all() for c in range(64)])
    assert late.all(), np.flatnonzero(~late).tolist()                      # the carrier detect stays defined: no 0 / 0
    assert r.counts.sum() >= 400, r.counts.sum()


# ---- clock rounding ----------------------------------------------------------------------------------------------------------------------------------
def test_rounding_rows_hand_std_round_an_exact_half():
    """Every channel of the batch makes ClockRecovery round an x.5 exactly once (std::round: away from zero; rintf would go to even).  And none of the
    crafted batches does: the census of the search is in NOTES.md."""
    o = cl.clock_census(cl.rounding(), None)
    assert (o[:, 1] >= 1).all() and o[:, 0].min() > 1000, (o[:, 1].tolist(), o[:, 0].min())
    assert cl.rounding_oracle().counts.sum() >= 100, cl.rounding_oracle().counts.sum()
    for name in ("natural", "held"):
        assert cl.clock_census(getattr(cl, name)(), cl.IDENTITY)[:, 1].sum() == 0, name


# ---- crafted rows: long ties ---------------------------------------------------------------------------------------------------------------------------
def test_long_rows_tie_runs_far_longer_than_the_buffer_in_the_second_half():
    """What the held batch does not reach: trigger runs of bit-equal |v| longer than ten and than twenty samples — every buffer entry overwritten many
    times with the same word, so the winner is entry 0 whatever came first — ending in do_unlocked's SECOND half, on the LSF / stream word and on the
    packet / BERT word, with both signs."""
    r = cl.oracle_of("long_ties")
    census = {1: [], 2: []}
    for w in census:
        for c in range(cl.LONG_C):
            for a, b, where in cl.searched_runs(r, c, w):
                v = r.trig[c, a:b + 1, w]
                if np.unique(np.abs(v).view(np.uint32)).size == 1:
                    census[w].append((c, b - a + 1, where, bool(v[0] > 0)))
    for w, runs in census.items():
        long_ = [q for q in runs if q[1] > 20 and q[2] == "second"]
        print("long ties: word", w, "wholly tied runs over 20 samples ending in the second half:", len(long_), "longest", max(q[1] for q in long_))
        assert len(long_) >= 4, (w, len(long_))                              # measured: 8 and 8, 71 .. 340 samples
    signs = {q[3] for w in census for q in census[w] if q[1] > 20}
    assert signs == {True, False}, signs                                     # the LSF word ties on its positive side, the packet word on its negative
    assert any(10 < q[1] for w in census for q in census[w])
    assert r.counts.sum() >= 100, r.counts.sum()                             # measured: 210 records on 18 of 32 channels


def test_long_rows_reach_an_infinite_idev_while_locked():
    """The long tied run on the tiny constant ends in do_unlocked's second half: dev.reset(), then update_values on a ring whose eight symbols are all
    1e-20 — mn == mx, idev = 6 / 0 = +inf — and the channel goes to FRAME like that: callbacks with locked != 0, deviation == 0 and evm NaN follow."""
    r = cl.oracle_of("long_ties")
    chans, callbacks = [], 0
    for c in range(cl.LONG_C):
        lp, lv = r.levels(c)
        m = (lv[:, 0] == lv[:, 1]) & np.isinf(lv[:, 2])
        if not m.any():
            continue
        lg = r.logs(c)
        later = lg[(lg["pad"][:, 0] > lp[m][0]) & (lg["locked"] != 0) & (lg["deviation"] == 0)]
        assert later.size >= 10 and np.isnan(later["evm"]).all(), (c, later.size)      # measured: 20 .. 24 per channel, evm NaN in every one
        chans.append(c)
        callbacks += later.size
    print("long ties: mn == mx with idev infinite on channels", chans, "; locked callbacks with deviation 0 behind it:", callbacks)
    assert len(chans) >= 4, chans                                                      # measured: 8 of 32 (5, 6, 12, 13, 19, 20, 25, 27), 176 callbacks
