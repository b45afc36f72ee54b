"""GPU tests of the frame decoder's three device forms on chosen LLRs (m17hip_decode_sequences, include/m17hip.h: form 0 the lane-per-frame
decoder with 32-bit metrics, form 1 the wave decoder K5 runs, form 2 K5's deferral, then settle_tail_kernel and decode_deferred_kernel with its
packed 16-bit metrics, as m17hip_demod_run queues them) against ol.decode_frame stepped frame by frame.  No tolerance anywhere: integer work.
The inputs and what they are built to reach: tests/decode_forms_lib.py; that they reach it: tests/test_decode_forms.py (CPU).

Which tests fail when a decoder is changed wrongly (scratch builds, measured; NOTES.md has the table): the packed decoder's decision also set
on a tie — every sequence under form 2; its end-state scan taking the last minimum — classes, walk1, walk3, long under form 2; the wave
decoder's decision read off the other candidate, or set on a tie — every sequence under forms 1 and 2; position 401 not carried into a deferred
record — every sequence under form 2; the deferred decode's slot list forgetting where its chunk starts — long under form 2, and nothing else
in the suite."""
import numpy as np
import pytest

import decode_forms_lib as dl
import m17hip

pytestmark = pytest.mark.gpu

NAMES = ["classes", "walk0", "walk1", "walk2", "walk3", "long", "full_store"]


@pytest.fixture(scope="module")
def ctx():
    c = m17hip.Context(4, 4800)   # (the hook works in the operator scratch: the context's own size does not matter)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sequences():
    return {q.name: q for q in dl.all_sequences()}


def _check(q, out):
    recs, nrec, ovf, state, lich, lsf, dep401, cost, trace = out
    assert recs.shape == (q.C, q.rec_cap) and trace.shape == (q.C, q.F)
    over = False
    for c, e in enumerate(q.expect()):
        n = len(e["recs"])
        assert int(nrec[c]) == n, (c, int(nrec[c]), n)
        k = min(n, q.rec_cap)
        over |= n > q.rec_cap
        got = recs[c, :k].copy()
        exp = e["recs"][:k].copy()
        # the hook's own bookkeeping: the sequence, the callback's index, the frame that made the record
        assert (got["channel"] == c).all() and np.array_equal(got["seq"], np.arange(k)) and np.array_equal(got["sample_pos"], exp["sample_pos"]), c
        for a in (got, exp):
            a["channel"] = 0; a["seq"] = 0; a["sample_pos"] = 0
        if got.tobytes() != exp.tobytes():
            bad = [i for i in range(k) if got[i].tobytes() != exp[i].tobytes()]
            raise AssertionError((q.name, c, len(bad), bad[:8], got[bad[0]], exp[bad[0]]))
        assert not recs[c, k:].tobytes().strip(b"\0"), (c, "slots beyond the channel's records were written")
        assert (int(state[c]), int(lich[c]), lsf[c].tolist(), int(dep401[c]), int(cost[c])) == (e["final"][0], e["final"][1], e["final"][2].tolist(),
                                                                                                 e["final"][3], e["final"][4]), c
        if not np.array_equal(trace[c], e["trace"]):
            bad = np.nonzero(trace[c] != e["trace"])[0]
            raise AssertionError((q.name, c, "cost_trace", len(bad), bad[:8].tolist(), trace[c][bad[:8]].tolist(), e["trace"][bad[:8]].tolist()))
        # no deferred-cost tag is left anywhere: bit 31 is set in -1 alone
        assert ((trace[c] >= 0) | (trace[c] == -1)).all() and ((got["cost"] >= 0) | (got["cost"] == -1)).all() and int(cost[c]) >= -1, c
    assert ovf == int(over)


def _run(ctx, q, form, frames=None):
    F = q.F if frames is None else frames
    return ctx.decode_sequences(form, q.llr[:, :F], q.st[:, :F], q.rec_cap, state=q.state, dep401=q.dep401)


@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_forms_equal_the_oracle(ctx, sequences, name, form):
    q = sequences[name]
    _check(q, _run(ctx, q, form))


def test_full_store_is_reached_with_frames_left_to_defer(ctx, sequences):
    """The premise of full_store[2] on the device's own outputs: the store overflows (flag, counts beyond rec_cap) and the three forms agree on
    every output, so the frames that found it full were decoded in place with their exact costs."""
    q = sequences["full_store"]
    outs = [_run(ctx, q, form) for form in (0, 1, 2)]
    assert all(o[2] == 1 for o in outs) and (outs[0][1] > q.rec_cap).all()
    for o in outs[1:]:
        assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(outs[0], o))


def test_form_0_on_one_frame_equals_decode_frames(ctx, sequences):
    q = sequences["classes"]
    recs, nrec, ovf, state, lich, lsf, dep401, cost, trace = _run(ctx, q, 0, frames=1)
    r1, n1, s1, li1, lsf1, d1, c1 = ctx.decode_frames(q.llr[:, 0], q.st[:, 0], state=q.state, dep401=q.dep401)
    assert ovf == 0 and np.array_equal(nrec, n1) and np.array_equal(state, s1) and np.array_equal(lich, li1) and np.array_equal(lsf, lsf1)
    assert np.array_equal(dep401, d1) and np.array_equal(cost, c1) and np.array_equal(trace[:, 0], c1)
    a, b = recs[:, :2].copy(), r1.copy()
    for x in (a, b):
        x["channel"] = 0; x["seq"] = 0; x["sample_pos"] = 0
    assert a.tobytes() == b.tobytes() and not recs[:, 2:].tobytes().strip(b"\0")


def test_refusals_on_a_live_context(ctx):
    """The argument errors of tests/test_decode_forms.py hold with a context as well, before any launch: nothing is written."""
    llr = np.zeros((1, 2, 368), np.int8)
    for form, bad in ((3, llr), (0, np.where(np.arange(368) == 367, 8, llr)), (2, np.where(np.arange(368) == 0, -8, llr))):
        with pytest.raises(m17hip.M17HipError):
            ctx.decode_sequences(form, bad, np.zeros((1, 2), np.uint8), 4)
    with pytest.raises(m17hip.M17HipError):
        ctx.decode_sequences(2, llr, np.zeros((1, 2), np.uint8), 4, dep401=[8])
    with pytest.raises(m17hip.M17HipError):
        ctx.decode_sequences(1, llr, np.zeros((1, 2), np.uint8), 0)
