"""GPU tests of who makes the LAST pass of a run's deferred EVM fold (m17hip_tune key 17, csrc/m17hip.hip: EvmFold).  The pass is owed once the run is
queued and taken by whoever comes first: the next run's first limit-filter replay (launch_gate_seg), the run's own deferred decode (flush_payload),
somebody who asks for m17_diag (flush_fold), or the end of the next run.  A pass that is skipped, made twice or made over the wrong rows leaves another
RunningStandardDeviation in the channel, so m17_diag.evm at the end of the run after it has other bits than the oracle's.

8 channels, runs of 9600 samples.  A call sequence of r runs reads m17_diag once, after its last run (a read in between would take the owed pass itself);
it is made for every r, so the m17_diag of every run is compared, evm as its uint32 word, and the records of the runs fetched byte for byte."""
import numpy as np
import pytest

import m17hip
import oracle_lib as ol

pytestmark = pytest.mark.gpu

Cn, T, N = 8, 9600, 6
FIELDS = ("dcd", "locked", "sample_index", "viterbi_cost", "n_diag", "demod_state", "n_frames", "deviation", "offset", "clock")


def _stream():
    p = ol.gen_params(seed=7117, kind=-1, n_frames=N * T // 1920 - 3, lead_in=1000, noise_sigma=700.0, tail_sigma=700.0, lead_sigma=40000.0, total=N * T)
    return ol.generate_batch(p, Cn, N * T, threads=4)


def _expect(x):
    """Per run r: the oracle's records of that run (ordered by channel, seq) and its m17_diag at the end of the run, from the stream up to there."""
    out = []
    for r in range(N):
        recs, counts, diags = ol.demod_batch(x[:, :(r + 1) * T], cap=2 * ((r + 1) * T // 1920 + 2) + 4, threads=4)
        rows = [recs[c, :counts[c]] for c in range(Cn)]
        out.append((np.concatenate([rc[rc["sample_pos"] >= r * T] for rc in rows]), diags))
    return out


def _vacuity(exp):
    """Every channel fires a diagnostic callback in every run and ends every run with another evm word than the run before: a pass that is skipped or
    made twice cannot go unseen."""
    for r in range(N):
        n, w = exp[r][1]["n_diag"], exp[r][1]["evm"].view(np.uint32)
        assert (n > (exp[r - 1][1]["n_diag"] if r else 0)).all(), (r, n)
        assert r == 0 or (w != exp[r - 1][1]["evm"].view(np.uint32)).all(), (r, w)


@pytest.fixture(scope="module")
def feed():
    import torch
    x = _stream()
    exp = _expect(x)
    _vacuity(exp)                                   # (before any context is opened)
    chunks = [np.ascontiguousarray(x[:, r * T:(r + 1) * T]) for r in range(N)]
    return chunks, [torch.from_numpy(ch).pin_memory() for ch in chunks], exp


def _context(keys):
    c = m17hip.Context(Cn, T)
    for k, v in keys.items():
        c.tune(k, v)
    return c


def _check_diag(c, exp, r):
    d = c.diag(Cn)
    assert np.array_equal(d["evm"].view(np.uint32), exp[r][1]["evm"].view(np.uint32)), (r, d["evm"], exp[r][1]["evm"])
    for f in FIELDS:
        assert np.array_equal(d[f], exp[r][1][f], equal_nan=True), (r, f)


def _check_recs(c, exp, r):
    got = c.frames()
    got = got[np.lexsort((got["seq"], got["channel"]))]
    assert got.tobytes() == exp[r][0].tobytes(), r


def _back_to_back(c, feed, r, staged_first):
    """r runs in place with no fetch between them (staged_first: the first one from pinned memory, so that the context streams: its payload work then
    waits on the copy stream until somebody asks for it), then m17_diag and the records of the last two runs."""
    chunks, pins, exp = feed
    c.reset()
    for k in range(r):
        if k == 0 and staged_first:
            c.upload_async(pins[0].data_ptr(), Cn, T)
            c.run(channels=Cn, samples=T)
        else:
            c.upload(chunks[k])
            c.run()
    _check_diag(c, exp, r - 1)
    _check_recs(c, exp, r - 1)
    if r > 1:
        c.frames_select(1)
        _check_recs(c, exp, r - 2)
        c.frames_select(0)
    c.upload_wait()


@pytest.mark.parametrize("seg", [4800, 0], ids=["a_two_segments", "b_one_segment"])
def test_the_pass_rides_the_next_runs_replay(feed, seg):
    """(a) key 3 = 4800, two segments: the context streams (its first run was staged), so nothing is queued behind a run; the owed pass of run k is taken
    in launch_gate_seg by the replay that runs ahead for segment 1 of run k + 1, beside K5 of its segment 0: last = 2, m17_diag not settled by it.
    (b) key 3 = 0, one segment: taken in launch_gate_seg by the only replay of run k + 1, in front of its K5: last = 1.
    The last run's pass in both: flush_fold, from m17hip_diag_fetch."""
    c = _context({3: seg})
    for r in range(1, N + 1):
        _back_to_back(c, feed, r, True)
    c.close()


def test_c_diag_after_every_run_takes_every_pass(feed):
    """(c) a context that streams, every run staged by the run call and followed by m17hip_diag_fetch: every pass is made by flush_fold, last = 1."""
    chunks, pins, exp = feed
    c = _context({})
    c.reset()
    for r in range(N):
        c.upload_async(pins[r].data_ptr(), Cn, T)
        c.run(channels=Cn, samples=T)
        _check_diag(c, exp, r)
        _check_recs(c, exp, r)
    c.upload_wait()
    c.close()


@pytest.mark.parametrize("keys", [{}, {15: 0}, {15: 0, 3: 4800}], ids=["d_beside_the_decode", "d_no_deferred_decode", "d_no_deferred_decode_two_segments"])
def test_d_a_context_that_never_staged_input(feed, keys):
    """(d) the payload stream is the main stream and a run's payload work is queued behind it at once (flush_after_run): the owed pass rides the run's own
    deferred decode in flush_payload (fold_beside_decode), last = 1, and nothing is owed when the next run begins.  With key 15 = 0 there is no deferred
    decode to ride: the pass stays owed and goes as in (b) — or, with two segments, as in (a) — and the last one with flush_fold."""
    c = _context(keys)
    for r in range(1, N + 1):
        _back_to_back(c, feed, r, False)
    c.close()


@pytest.mark.parametrize("seg", [4800, 0], ids=["two_segments", "one_segment"])
@pytest.mark.parametrize("order", ["fetch_then_run", "run_then_fetch"])
def test_e_staged_live_feed(feed, order, seg):
    """(e) stage(k + 1), m17hip_demod_front(k + 1), then run k's records and run(k + 1) in either order.  m17hip_demod_front queues the replay of segment 0
    early (key 25); with one segment that replay takes run k's owed pass (launch_gate_seg, k == 0, last = 1) from inside m17hip_demod_front; with two
    segments it is not the one, and the run call's replay ahead for segment 1 takes it (last = 2).  The last run's pass: flush_fold."""
    chunks, pins, exp = feed
    c = _context({3: seg})
    for r in range(1, N + 1):
        c.reset()
        c.upload_async(pins[0].data_ptr(), Cn, T)
        c.run(channels=Cn, samples=T)
        for k in range(r):
            if k + 1 < r:
                c.upload_async(pins[k + 1].data_ptr(), Cn, T)
                c.front(channels=Cn, samples=T)
                if order == "run_then_fetch":
                    c.run(channels=Cn, samples=T)
                    c.frames_select(1)
            _check_recs(c, exp, k)
            c.frames_select(0)
            if k + 1 < r and order != "run_then_fetch":
                c.run(channels=Cn, samples=T)
        _check_diag(c, exp, r - 1)
        c.upload_wait()
    c.close()


def test_f_keys_17_and_18_between_runs(feed):
    """(f) in place with key 15 = 0, so that a pass stays owed until the next run (a run that begins while one is owed writes the other buffer).
    run 0 writes ev_ops2[0]; run 1 ev_ops2[1]; key 17 = 0 (flush_fold, both buffers released); run 2 folds inside K5 and writes neither; key 17 = 1;
    run 3 writes ev_ops2[1] (nothing owed: the parity stays); run 4 ev_ops2[0]; key 18 = 2048 floats per row (flush_fold, both released);
    run 5 writes ev_ops2[0] at the new pitch (ev_row_floats(9600) = 1060 fit).  A fresh context per length r, m17_diag after the last step."""
    chunks, pins, exp = feed
    before = {2: (17, 0), 3: (17, 1), 5: (18, 2048)}
    for r in range(1, N + 1):
        c = _context({15: 0})
        for k in range(r):
            if k in before:
                c.tune(*before[k])
            c.upload(chunks[k])
            c.run()
        if r in before:          # (the key set behind the last run as well: its flush_fold is the taker)
            c.tune(*before[r])
        _check_diag(c, exp, r - 1)
        _check_recs(c, exp, r - 1)
        c.close()
