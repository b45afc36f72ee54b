"""CPU: the conditions under which tests/test_gpu_boundary_phases.py can fail, asserted on the ORACLE alone over exactly its inputs (tests/boundary_phases.py,
whose docstring has the construction and the argument why frame completions are what has to be counted).  Each is a condition, not a measurement: a change
of the generator or of the batches that empties the GPU tests fails here, without a GPU.  The figures in the messages are the measured ones."""
import numpy as np
import pytest

import boundary_phases as bp

# forced unlocks: channels that show one (of 1920), and distinct positions of those callbacks minus the channel's delay.  Measured: stream 1863 / 1253,
# BERT 1771 / 464, packet 1328 / 1995 (boundary_phases.KINDS says what the packet batch needed for it).
FORCED_MIN = 1000


@pytest.mark.parametrize("name", bp.BATCHES)
def test_payload_frames_complete_on_every_phase(name):
    """The payload-frame records of a batch cover all 1920 residues of sample_pos % 1920 — and of % 640, which follows but is what the runs of 640 cut at."""
    o = bp.oracle(name)
    _, pos = o.completions(bp.KINDS[name][2])
    for mod in (1920, 640):
        got = np.unique(pos % mod).size
        assert got == mod, f"{name}: payload-frame completions cover {got} of {mod} residues"
    assert max(r.size for r in o.rows) < 2 * (bp.T // 1920 + 2) + 4          # (the room the oracle's helper gives a channel: nothing was cut off)


@pytest.mark.parametrize("name", ["stream", "packet"])
def test_lsf_records_cover_most_phases(name):
    """Acquisition is quantised by the carrier detect's 384-sample cadence, so the LSF records cannot cover every residue from one seed.  Measured: 1727
    (stream) and 1728 (packet)."""
    _, pos = bp.oracle(name).completions(bp.FT_LSF)
    got = np.unique(pos % 1920).size
    assert got >= 1700, f"{name}: LSF records cover {got} residues"


@pytest.mark.parametrize("name", bp.BATCHES)
def test_forced_unlocks_at_many_phases(name):
    """Channels whose log shows `locked` falling with the carrier still there (boundary_phases.Oracle.forced_unlocks says how that is read off a log whose
    `dcd` is already 0 at that callback), and the spread of those callbacks against the channels' delays."""
    o = bp.oracle(name)
    ch, pos = o.forced_unlocks()
    chans, distinct = np.unique(ch).size, np.unique(pos - bp.delay(name)[ch]).size
    assert chans >= FORCED_MIN and distinct >= 3, f"{name}: {chans} channels show a forced unlock, {distinct} distinct positions minus delay"
    # and never with dcd = 1 in that very callback: the reading above is the only one there is
    same = o.log_chan[1:] == o.log_chan[:-1]
    assert not (same & (o.log["locked"][:-1] != 0) & (o.log["locked"][1:] == 0) & (o.log["dcd"][1:] != 0)).any()


@pytest.mark.parametrize("name", bp.BATCHES + ("mixed", "hole"))
def test_the_carrier_detect_changes_and_most_channels_end_inside_a_frame(name):
    o = bp.oracle(name)
    ch, _ = o.dcd_changes()
    assert np.unique(ch).size == o.C, f"{name}: dcd changes on {np.unique(ch).size} of {o.C} channels"
    in_frame = int((o.diags["demod_state"] != bp.ST_UNLOCKED).sum())
    # measured: stream 1920, BERT 1090 (its eleven missed sync words end shortly before the stream does), packet 1822, mixed 384, hole 383
    assert in_frame > o.C // 2, f"{name}: {in_frame} of {o.C} channels end locked"
    # a run of 1920 samples fires at most five callbacks (the diagnostic-log room of 8 the GPU tests ask for is enough)
    counts = np.zeros((bp.T // 640, o.C), dtype=np.int64)
    np.add.at(counts, (o.log_pos // 640, o.log_chan), 1)
    assert counts.reshape(-1, 3, o.C).sum(axis=1).max() <= 5 and counts.max() <= 2


def test_the_gate_aware_front_end_has_segments_to_skip():
    """What tests/test_gpu_boundary_phases.py's gate-aware cell rests on: cut every 640 samples, every channel of the packet batch has segments k >= 2 over
    which the carrier detect is off throughout (measured: 1920 channels, 4877 segments, all of them in front of the transmission — behind a forced unlock
    the detector is off for one interval of 384 samples and comes straight back on the noise).  Cut every 1920 samples there is none: that cell runs
    the gate-aware schedule (the front end follows K5 of segment k - 2) with nothing to skip, which is said here so that nobody takes it for more."""
    o = bp.oracle("packet")
    off = o.carrier_off_segments(640)
    assert len({c for c, _ in off}) == bp.C and len(off) >= 4000, (len({c for c, _ in off}), len(off))
    assert not o.carrier_off_segments(1920)


def test_mixed_polarity_batch_is_the_stream_batch_under_its_table():
    """Every second channel negated, and the oracle under the table reports on them what it reports on the plain ones."""
    x, y, pol = bp.batch("stream")[:bp.MIXED_C], bp.batch("mixed"), bp.polarity()
    assert pol.tolist() == [0, 1] * (bp.MIXED_C // 2)
    assert (y[pol == 0] == x[pol == 0]).all() and (y[pol == 1] == bp.oc.negated(x[pol == 1])).all()
    # (-32768 has no opposite and the loud lead-in saturates, so a negated channel is not bit for bit its plain twin: the oracle runs on y itself)
    o = bp.oracle("mixed")
    ch, pos = o.completions(bp.FT_STREAM)
    assert np.unique(pos % 1920).size == bp.MIXED_C and np.unique(ch[(ch & 1) == 1]).size == bp.MIXED_C // 2


def test_packet_hole_reaches_the_give_up_branch_of_packet_sync():
    """do_packet_sync's last branch (eleven missed sync words, each frame costing 60 or more: UNLOCKED and dcd.unlock()) is the one line of the oracle's
    orchestrator that no other CPU input of the suite executes.  Measured on the hole batch: 132 of 384 channels leave PACKET_SYNC for UNLOCKED there
    (boundary_phases.gave_up_packet_sync says how that is read off records and log); a coverage build of the oracle counts the branch 263 times over
    the two passes (records, log) the helper makes per channel."""
    o = bp.oracle("hole")
    at = {c: bp.gave_up_packet_sync(o.rows[c], o.logs[c], (bp.hole_span(c)[0], bp.T)) for c in range(o.C)}
    gave = [c for c in at if at[c] is not None]
    assert len(gave) >= 100, f"{len(gave)} of {o.C} channels give up in PACKET_SYNC"
    last10 = last11 = 0
    for c in gave:
        r = o.rows[c]
        r = r[(r["sample_pos"] >= bp.hole_span(c)[0]) & (r["sample_pos"] < at[c])]
        # at least eleven consecutive packet frames behind the hole's start; the first missed sync word counts whatever its frame cost, every further
        # one only at a cost of 60 or more (a cheaper frame leaves the count as it is), and the frame in front of the give-up cost 60 or more
        assert r.size >= 11 and (r["frame_type"][-11:] == bp.FT_BASIC_PACKET).all() and int((r["cost"] >= 60).sum()) >= 10 and r["cost"][-1] >= 60, c
        last10 += bool((r["cost"][-10:] >= 60).all())
        last11 += bool((r["cost"][-11:] >= 60).all())
        st = bp.states_between(o.logs[c], at[c] - 960, at[c] + 1)
        assert st[-1] == bp.ST_UNLOCKED and st[0] != bp.ST_UNLOCKED, (c, st)
    # the plain case — the frames that count come in a row, none cheaper than 60 between them — is the common one: the ten that follow the first missed
    # sync word on 125 of the 132 channels, and all eleven (the first damaged frame is seldom that costly) on 3
    assert last10 >= 100 and last11 >= 1, (last10, last11)
    # the give-ups are spread over the delays: a run boundary meets them at many phases
    assert np.unique([(at[c] - bp.delay("hole")[c]) % 1920 for c in gave]).size >= 50
