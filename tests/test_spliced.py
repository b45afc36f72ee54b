"""CPU: the cutting and joining helper (tests/spliced.py) and, on the ORACLE alone, the conditions under which tests/test_gpu_spliced.py can fail:
its inputs do reach the late-entry path of the demodulator (a sync word accepted without a preamble, the frame decoder's walk through the LICH
segments to an assembled LSF and on to STREAM) and the missing-sync counting of a carrier that disappears, on EVERY channel of each batch."""
import os
import subprocess

import numpy as np
import pytest

import off_clock as oc
import oracle_lib as ol
import spliced as sp

F = sp.FRAME
MAX_MISSING_SYNC = 10          # M17Demodulator.h


# ---- the operations ---------------------------------------------------------------------------------------------------------------------------
def test_the_operations_cut_and_join_what_they_say():
    x = np.arange(1, 20001, dtype=np.int16)
    fill = -np.arange(1, 20001, dtype=np.int16)
    y = sp.late_entry(x, 100, 2, 3, 7)
    assert y.size == x.size - 5 * F - 7 and np.array_equal(y[:100], x[:100]) and y[100] == x[100 + 5 * F + 7]
    y = sp.drop_tail(x, 100, 4, fill)
    assert np.array_equal(y[:100 + 4 * F], x[:100 + 4 * F]) and np.array_equal(y[100 + 4 * F:], fill[100 + 4 * F:])
    y = sp.hole(x, 500, 2, "noise", fill, extra=3)
    assert np.array_equal(y[:500], x[:500]) and np.array_equal(y[500:500 + 2 * F + 3], fill[500:500 + 2 * F + 3]) and np.array_equal(y[503 + 2 * F:], x[503 + 2 * F:])
    y = sp.hole(x, 500, 2, "remove", extra=3)
    assert y.size == x.size - 2 * F - 3 and y[499] == x[499] and y[500] == x[500 + 2 * F + 3]
    y = sp.blank_lsf(x, 100, fill)
    assert np.array_equal(y[:100 + F], x[:100 + F]) and np.array_equal(y[100 + F:100 + 2 * F], fill[100 + F:100 + 2 * F]) and np.array_equal(y[100 + 2 * F:], x[100 + 2 * F:])
    for gap in sp.GAPS:
        y = sp.splice(x[:300], x[1000:1200], gap, fill)
        assert y.size == 500 + gap and np.array_equal(y[300:300 + gap], fill[:gap]) and y[300 + gap] == x[1000]
    for op in (lambda: sp.late_entry(x, 19000, 2, 0, 0), lambda: sp.hole(x, 19000, 1, "remove"), lambda: sp.drop_tail(x, 100, 4, fill[:10])):
        with pytest.raises(AssertionError):
            op()
    n = sp.noise(5, 4000, 300.0)
    assert n.dtype == np.int16 and 250 < n.astype(np.float64).std() < 350 and np.array_equal(n, sp.noise(5, 4000, 300.0))
    assert set(np.unique(sp.noise(5, 500, 0.0)).tolist()) == {-1, 1}          # no run of exact zeros


def test_the_batches_are_deterministic_and_read_only():
    for name in sp.BATCHES:
        b = sp.batch(name)
        assert b["x"].shape == (sp.C, sp.T) and not b["x"].flags.writeable
        fn, seed_of = sp.CHANNEL[name]
        for c in (0, 17, 63):
            seed = sp.SEEDS[name][c] if seed_of is None else seed_of(c, sp.SEEDS[name])
            assert np.array_equal(fn(c, seed)["x"], b["x"][c]), (name, c)


# ---- the late-entry pattern: LICH ..., the LSF assembled from them, then the stream -------------------------------------------------------------
def _frame_of(pos, m):
    """The payload frame (counted from the transmission's first) that a record fired at sample `pos` belongs to: with `lead` frames (preamble, LSF)
    still in front and k payload frames and `off` samples cut, frame i ends at bs + (lead + i - k + 1) * 1920 - off, and its record fires the
    delay of the two pulse-shaping filters (138 samples measured, 100 .. 300 allowed) behind that."""
    return m["k"] - m["lead"] - 1 + int((pos - m["bs"] + m["off"] - 100) // F)


def _collection(name):
    x, rows, diags, logs = sp.rows_of(name)
    meta = sp.batch(name)["meta"]
    firsts = []
    for c in range(sp.C):
        m = meta[c]
        if m["kind"] != 1:
            continue
        p = sp.late_pattern(rows[c])
        assert p is not None, (name, c, rows[c]["frame_type"].tolist())
        j, i = p
        r = rows[c]
        assert i - j >= 1 and int((r["frame_type"][i + 1:] == sp.FT_STREAM).sum()) >= 3, (name, c)
        # the six segments that complete the LSF: each carries the counter its place in the transmission gives it
        six = r[i - 6:i] if i >= 6 else r[:0]
        assert six.size == 6 and (six["frame_type"] == sp.FT_LICH).all(), (name, c)
        for rec in six:
            assert sp.lich_counter(rec) == _frame_of(int(rec["sample_pos"]), m) % 6, (name, c, int(rec["sample_pos"]), sp.lich_counter(rec))
        assert sorted(sp.lich_counter(rec) for rec in six) == [0, 1, 2, 3, 4, 5], (name, c)
        # the assembled LSF is the transmitted one, reported with the record that completed it (same sample, cost 0)
        assert bytes(r["payload"][i][:30]) == bytes(m["lsf"]) and r["sample_pos"][i] == r["sample_pos"][i - 1] and r["cost"][i] == 0, (name, c)
        assert r["seq"][i] == i and (np.diff(r["seq"].astype(np.int64)) == 1).all()
        firsts.append(sp.lich_counter(six[0]))
    return firsts


def test_late_entry_streams_walk_from_lich_to_an_assembled_lsf_to_stream_on_every_channel():
    meta = sp.batch("late")["meta"]
    assert sum(1 for m in meta if m["kind"] == 1) == 48
    assert {m["off"] for m in meta} == set(sp.OFFS) and {m["k"] for m in meta if m["kind"] == 1} == set(range(12))
    firsts = _collection("late")
    assert len(firsts) == 48 and set(firsts) == {0, 1, 2, 3, 4, 5}, sorted(set(firsts))     # the collection starts at every LICH phase
    # no channel opens with an LSF record decoded from an LSF frame: the LSF went with the cut
    x, rows, _, _ = sp.rows_of("late")
    for c in range(sp.C):
        ft = rows[c]["frame_type"]
        assert not any(ft[i] == sp.FT_LSF and (i == 0 or ft[i - 1] != sp.FT_LICH) for i in range(ft.size)), c


def test_blank_lsf_streams_take_the_stream_branch_of_lsf_sync_on_every_channel():
    """The LSF frame overwritten with the preamble's continuation: the demodulator stays in LSF_SYNC behind the preamble (sync_count counting its
    hits) and accepts the first STREAM sync word there, so the first record is payload frame 0's LICH segment 0 and the log goes LSF_SYNC -> FRAME;
    then the LICH walk as on the late-entry channels, here always from phase 0.  No record lies at the LSF's position."""
    firsts = _collection("blank")
    assert firsts == [0] * sp.C
    x, rows, _, logs = sp.rows_of("blank")
    meta = sp.batch("blank")["meta"]
    for c in range(sp.C):
        r, bs = rows[c], meta[c]["bs"]
        assert sp.took_stream_branch_of_lsf_sync(meta[c], r, logs[c]), c
        assert not (r["sample_pos"] <= bs + 2 * F + 300).any(), c                            # nothing at the blanked LSF's position or before
        assert sp.late_pattern(r) == (0, 6), c


def test_noise_over_the_lsf_does_not_reach_that_branch():
    """Why the fill is not noise: with the generator's tail noise over the LSF frame the carrier's drop behind the preamble is taken for a BERT sync
    word or loses the lock (the finding in NOTES); shown on the first eight channels' waveforms."""
    for c in range(8):
        seed = sp.SEEDS["blank"][c]
        sigma = sp.SIGMAS[c % 3]
        x, tr = sp._gen(seed, 1, 60, 2048 + 331 * (c % 7) + 97 * (c % 5), sigma, total=sp.T)
        y = sp.blank_lsf(x, tr["burst_start"], sp.noise(seed ^ 0x5EED5, sp.T, max(sigma, 100.0)))
        assert not sp.took_stream_branch_of_lsf_sync(dict(bs=tr["burst_start"]), ol.demod(y)[0], oc.demod_log(y)), c


# ---- holes ----------------------------------------------------------------------------------------------------------------------------------------
def test_holes_are_crossed_or_end_the_lock_on_every_channel():
    x, rows, diags, logs = sp.rows_of("hole")
    meta = sp.batch("hole")["meta"]
    assert {m["nf"] for m in meta} == set(sp.HOLE_FRAMES) and {m["kind"] for m in meta} == {0, 1, 2}
    moved = lost = relocked_after_long = 0
    for c in range(sp.C):
        m, r = meta[c], rows[c]
        behind, mv, ls = sp.hole_reach(m, r, logs[c])
        assert behind, c                                                                    # the records continue behind the hole ...
        assert np.array_equal(r["seq"], np.arange(r.size)), c                               # ... numbered on as if there had been none
        if m["mode"] == "remove" and m["n"] % F:
            assert mv or ls, c                                                              # timing jumped by no whole number of frames
            moved += mv; lost += ls
        relocked_after_long += int(m["mode"] == "noise" and m["nf"] > MAX_MISSING_SYNC and ls)
    assert moved >= 4 and lost >= 4, (moved, lost)
    assert relocked_after_long >= 4, relocked_after_long        # more than MAX_MISSING_SYNC frames of noise: the lock is lost and found again


# ---- one transmission straight behind another -----------------------------------------------------------------------------------------------------
def test_spliced_transmissions_are_both_reported_on_every_channel():
    x, rows, _, _ = sp.rows_of("splice")
    meta = sp.batch("splice")["meta"]
    assert {m["gap"] for m in meta} == set(sp.GAPS) and {(m["ka"], m["kb"]) for m in meta} == set(sp.SPLICE_KINDS)
    assert {m["dropped"] for m in meta} == {True, False}
    other = 0
    for c in range(sp.C):
        m = meta[c]
        ra, rb, dist = sp.splice_reach(m, rows[c])
        assert ra.size >= 3 and rb.size >= 3, (c, ra.size, rb.size)                         # records of both transmissions (by position)
        if m["gap"] == 0:
            assert dist < 3 * F, (c, dist)
        # a sync word of another kind met while locked: records in b's span still selected by a's kind of sync word
        other += int(m["ka"] != m["kb"] and (rb["sync_type"] == {1: 1, 4: 2, 0: 3}[m["ka"]]).any())
    assert other >= 1, other


def test_the_long_case_lies_astride_the_segment_boundaries():
    """8 x 480 000: on the oracle's positions the first LICH record of the collection lies a frame or more before sample 48 000 and the assembled LSF
    a frame or more behind it; every hole starts half a frame before its boundary; there is no EOT (stream records up to the end)."""
    x, rows, diags, logs = sp.long_rows()
    assert x.shape == (sp.LONG_C, sp.LONG_T)
    for c in range(sp.LONG_C):
        r = rows[c]
        j, i = sp.late_pattern(r)
        assert int(r["sample_pos"][j]) < sp.SEGMENT - F and int(r["sample_pos"][i]) > sp.SEGMENT + F, c
        assert r[-1]["frame_type"] == sp.FT_STREAM and int(r[-1]["sample_pos"]) > sp.LONG_T - 2 * F, c
        assert int((r["frame_type"] == sp.FT_STREAM).sum()) >= 150, c
        for seg, nf in sp.LONG_HOLES:
            assert (r["sample_pos"] > seg * sp.SEGMENT + nf * F + 8 * F).any(), (c, seg)     # the stream is found again behind every hole


def test_the_preconditions_of_the_gpu_module_hold():
    """CPU checks of tests/test_gpu_spliced.py's inputs: the LICH collection lies astride a run boundary on every stream channel, and the inverted
    twins of the late batch report the same kinds of records under a table that says so."""
    for name, streams in (("late", 48), ("blank", 64)):
        for kind in sp.RUN_KINDS:
            assert len(sp.straddling(name, sp.run_lengths(kind))) == streams, (name, kind)
    y, pol = sp.late_mixed_polarity()
    rows, _, _ = oc.oracle_of("spliced late, mixed polarity", y, pol, logs=True)
    plain = sp.rows_of("late")[1]
    for c in range(sp.C):
        assert rows[c]["frame_type"].tolist() == plain[c]["frame_type"].tolist(), c


def test_head_cut_packets_are_reported_as_the_oracle_reported_them():
    x, rows, _, _ = sp.rows_of("late")
    meta = sp.batch("late")["meta"]
    chans = [c for c in range(sp.C) if meta[c]["kind"] != 1]
    assert chans == sorted(sp.PACKET_HIST) and {meta[c]["kind"] for c in chans} == {2, 4}
    for c in chans:
        assert tuple(int(v) for v in np.bincount(rows[c]["frame_type"], minlength=6)) == sp.PACKET_HIST[c], c
    assert sum(h[sp.FT_BERT] for h in sp.PACKET_HIST.values()) > 100 and not any(h[sp.FT_BASIC_PACKET] or h[sp.FT_FULL_PACKET] for h in sp.PACKET_HIST.values())


# ---- a carrier that disappears -------------------------------------------------------------------------------------------------------------------
def test_drop_tail_counts_missing_syncs_and_unlocks_on_every_channel():
    x, rows, diags, logs = sp.rows_of("tail")
    meta = sp.batch("tail")["meta"]
    rises = 0
    for c in range(sp.C):
        m = meta[c]
        if m["eot"]:
            continue
        end = m["bs"] + m["kept"] * F
        lg, pos = logs[c], oc.log_pos(logs[c])
        assert lg["demod_state"][pos <= end][-1] != sp.ST_UNLOCKED, c                       # locked when the carrier goes
        after = pos > end
        assert ((lg["demod_state"][after] == sp.ST_UNLOCKED) & (lg["locked"][after] == 0)).any(), c
        # missing_sync_count (high half of m17_diag.pad[1]) at the end of runs that stop 1, 2, ... frames behind the cut: it rises
        ends = [ol.demod(x[c, :end + 960 + n * F])[1] for n in range(1, 12)]
        msc = [int(d["pad"][1]) >> 16 for d in ends if d["demod_state"] != sp.ST_UNLOCKED]      # (unlocked, the same word counts samples)
        run = 1
        while run < len(msc) and msc[run] == msc[run - 1] + 1:
            run += 1
        assert run >= 3, (c, msc)
        locked_ends = [end + 960 + n * F for n, d in zip(range(1, 12), ends) if d["demod_state"] != sp.ST_UNLOCKED]
        first_unlocked = int(pos[after & (lg["demod_state"] == sp.ST_UNLOCKED)][0])
        assert first_unlocked > locked_ends[run - 1], (c, first_unlocked, locked_ends[run - 1])    # first the count rises, then the lock goes
        rises += max(msc[:run]) >= MAX_MISSING_SYNC
    assert rises >= 8, rises                                                                # the limit itself is reached on some


def test_a_stream_cut_without_eot_ends_differently_from_its_twin_with_eot():
    x, rows, diags, logs = sp.rows_of("tail")
    meta = sp.batch("tail")["meta"]
    later = 0
    for c in range(0, sp.C, 4):
        cut, whole = meta[c], meta[c + 1]
        assert cut["kind"] == 1 and whole["eot"] and not cut["eot"] and cut["kept"] == whole["kept"]
        assert (int(diags[c]["n_diag"]), rows[c].size) != (int(diags[c + 1]["n_diag"]), rows[c + 1].size), c
        s_cut = rows[c][rows[c]["frame_type"] == sp.FT_STREAM]
        s_whole = rows[c + 1][rows[c + 1]["frame_type"] == sp.FT_STREAM]
        later += int(s_cut.size and (not s_whole.size or s_cut["sample_pos"][-1] - cut["bs"] > s_whole["sample_pos"][-1] - whole["bs"]))
    # (12 of 16, not all: on noisy channels the twin's EOT is missed now and then and it runs on as long as the cut one)
    assert later >= 12, later          # without EOT the demodulator goes on reporting stream frames from noise until the count runs out


# ---- the oracle pinned to the reference on these waveforms ---------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(os.path.join(ol.ORACLE_DIR, "_ref", "libm17ref.so")), reason="oracle/_ref not built (reference not present)")
def test_the_orchestrator_over_the_references_own_operators_equals_the_oracle_on_cut_waveforms():
    """Records, the last diagnostic callback and every diagnostic callback, byte for byte, on 8 channels of each batch."""
    n = 0
    for name in sp.BATCHES:
        x = sp.batch(name)["x"]
        for c in range(0, 64, 8):
            ro, do = ol.demod(x[c])
            rh, dh = ol.hybrid_demod(x[c])
            assert ro.tobytes() == rh.tobytes() and do.tobytes() == dh.tobytes(), (name, c)
            assert ol.demod_diag_log(x[c]).tobytes() == ol.hybrid_diag_log(x[c]).tobytes(), (name, c)
            n += 1
    assert n >= 24


MIRROR = os.environ.get("M17_MIRROR_CHECK") or os.path.join(ol.ROOT, "tests", "cxx", "mirror_check")   # built by build() (tests/test_cxx_mirror.py)


@pytest.mark.parametrize("name,c", [("late", 0), ("late", 3), ("blank", 1), ("tail", 0), ("tail", 2), ("hole", 9), ("hole", 10), ("splice", 2), ("splice", 5)])
def test_the_scalar_cpu_demodulator_equals_the_oracle_on_cut_waveforms(tmp_path, name, c):
    """tests/test_cxx_mirror.py's comparison (every frame and diagnostic callback in order, bit for bit) on one or two waveforms per batch."""
    x = np.ascontiguousarray(sp.batch(name)["x"][c])
    x.tofile(tmp_path / "x.i16")
    r = subprocess.run([MIRROR, "cpu_demod", str(tmp_path / "x.i16")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    exp, n_recs, n_diag = sp.expected_callback_lines(x)
    assert n_recs >= 10 and n_diag > 90
    assert lines == exp


def test_a_reset_inside_the_collection_starts_it_over():
    """tests/test_gpu_spliced.py restarts every third late-entry stream between the run with its third LICH record and the next: on the oracle the
    restart falls before the LSF is assembled, and the fresh demodulator collects six more LICH records in front of its LSF, numbered from 0."""
    _, rows, _, _ = sp.rows_of("late")
    fresh = sp.reset_expectation()
    assert len(fresh) == 16, len(fresh)                      # every third of the 48 streams
    broken = 0
    for c, (at, r, d) in fresh.items():
        j, i = sp.late_pattern(rows[c])
        assert int(rows[c]["sample_pos"][j + 2]) < at < int(rows[c]["sample_pos"][i]), c
        p = sp.late_pattern(r)
        assert np.array_equal(r["seq"], np.arange(r.size)), c
        if c in (0, 8, 44):             # measured: restarted there, the reference does not find these three streams again (no LSF assembled)
            assert p is None, c
            continue
        assert p is not None and p[1] - p[0] >= 6, c
        assert bytes(r["payload"][p[1]][:30]) == bytes(sp.batch("late")["meta"][c]["lsf"]), c
        broken += 1
    assert broken == 13
