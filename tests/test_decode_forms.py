"""CPU-only: the premises of tests/test_gpu_decode_forms.py, on the reference alone.  The inputs of tests/decode_forms_lib.py are built to reach
what whole-chain runs reach by chance or never — ties in every comparison, end states that share the minimum, every pair of decoder state and
sync type, deferred records beyond slot 512 and on both sides of it, a full record store.  Here the oracle (and a numpy restatement of the
trellis, first shown to equal the oracle's) says that they do; the GPU module then compares the device's three forms of the decoder with the
oracle on them.  And what m17hip_decode_sequences can refuse without a device."""
import ctypes as C

import numpy as np
import pytest

import decode_forms_lib as dl
import m17hip
import oracle_lib as ol


def test_numpy_restatement_equals_the_oracle_on_every_frame():
    n = 0
    for kind, (keys, soft, r) in dl.restated().items():
        assert len(keys) >= 100, kind   # every layout is there in numbers
        for i, key in enumerate(keys):
            cost, bits = ol.viterbi(soft[i], dl.SHAPES[kind][1])
            assert cost == int(r["cost"][i]) and np.array_equal(bits, r["bits"][i]), (kind, key)
        n += len(keys)
    print(f"{n} frames through a Viterbi decoder, four layouts")


def _class_results(name):
    """The restatement's results of the class frames called `name`, by layout."""
    q = dl.seq_classes()
    names = [nm for nm, _ in dl.class_frames() for _ in range(6)]
    out = {k: [] for k in range(4)}
    for kind, (keys, _, r) in dl.restated().items():
        for i, (seq, c, f) in enumerate(keys):
            if seq == q.name and c < len(names) and names[c] == name:
                out[kind].append({k: int(v[i]) for k, v in r.items() if k != "bits"})
    return out


def test_all_zero_frames_tie_in_every_comparison():
    """Every bit erased: all branch costs are 0, so wherever two reachable paths meet they tie — the decision must be 0 (`m0 > m2` is strict)
    sixteen times a step.  dep401 = 0 here; under another value the BERT layout's last step is not erased (the dep401 channels)."""
    res = _class_results("zero")
    for kind in range(4):
        assert res[kind], kind
        for r in res[kind]:
            # (two reachable paths first meet in step 4: the sixteen states are reached after four steps from state 0)
            assert r["compares"] == 16 * (dl.SHAPES[kind][0] // 2 - 4) and r["ties"] == r["compares"], (kind, r)
            assert r["n_min"] == 16 and r["cost"] == 0


def test_every_layout_has_frames_whose_final_minimum_is_shared():
    for kind, (keys, _, r) in dl.restated().items():
        shared = int((r["n_min"] >= 2).sum())
        assert shared >= 1, kind
        # ... and not only the all-zero frame: minima shared by 2 .. 15 states, where taking the last one instead of the first changes the result
        assert int(((r["n_min"] >= 2) & (r["n_min"] < 16)).sum()) >= 1, kind
        print(f"layout {kind}: {shared} of {len(keys)} frames end in a shared minimum")


def test_walks_visit_every_pair_of_decoder_state_and_sync_type():
    seen = set()
    for q in dl.seq_walks():
        assert (q.C, q.F) == (3, 24)
        for c, e in enumerate(q.expect()):
            seen |= {(e["before"][f][0], int(q.st[c, f])) for f in range(q.F)}
    assert seen == {(s, t) for s in range(5) for t in range(4)}


def test_packet_channel_reaches_full_packet_and_its_last_frame():
    """The FULL_PACKET LSF built with tx_build sends the decoder to state 3; a packet frame with the last-frame bit takes it back to LSF."""
    hit_full = hit_last = False
    for q in dl.seq_walks() + [dl.seq_classes()]:
        for c, e in enumerate(q.expect()):
            states = [b[0] for b in e["before"]] + [e["final"][0]]
            r = e["recs"]
            hit_full |= bool((r["frame_type"] == 4).any())
            for k in np.nonzero(r["frame_type"] == 4)[0]:
                if r["payload"][k][25] & 0x80:
                    hit_last |= states[int(r["sample_pos"][k]) + 1] == 0
    assert hit_full and hit_last


def test_largest_path_metric_is_within_the_bound_of_design_6():
    """a step adds at most 2 x 14 to a surviving metric, 244 steps at the most: 6832 < 2^15 - 20000 is what the packed decoder's
    16-bit metrics and its sentinel rest on.  The largest value over this set is printed (NOTES.md has it next to the bound)."""
    worst = {kind: int(r["max_metric"].max()) for kind, (_, _, r) in dl.restated().items()}
    print("largest finite path metric by layout:", worst)
    assert max(worst.values()) <= dl.METRIC_BOUND == 6832
    # the all +7 / all -7 / alternating frames are there to drive it up: far from any codeword they still cost at most 14 a step
    assert max(worst.values()) >= 1000


def test_slot_layout_of_the_long_channels():
    q = dl.seq_long()
    e = q.expect()
    deferred = [np.nonzero(np.isin(x["recs"]["frame_type"], (2, 5)))[0] for x in e]   # stream and BERT payload records: the ones form 2 defers
    assert all(len(x["recs"]) <= q.rec_cap for x in e)
    # channel 0: 512 or more LICH records first, the LSF never completes; then the LSF frame; every deferred record at slot 512 or beyond
    r0 = e[0]["recs"]
    assert (r0["frame_type"][:512] == 1).all() and all(b[0] == 0 for b in e[0]["before"][:521]) and e[0]["before"][521][0] == 1
    assert len(deferred[0]) >= 4 and deferred[0].min() >= 512
    # channels 1 and 2: deferred records in both chunks of the slot list, stream and BERT
    for c, ft in ((1, 2), (2, 5)):
        assert (e[c]["recs"]["frame_type"] == ft).all()
        assert (deferred[c] < 512).sum() >= 64 and (deferred[c] >= 512).sum() >= 4, c
    assert q.C % 2 == 1


def test_full_store_channels_overflow_on_payload_frames():
    q = dl.seq_full()
    for c, e in enumerate(q.expect()):
        r = e["recs"]
        assert len(r) > q.rec_cap, c
        assert np.isin(r["frame_type"][q.rec_cap:], (2, 5)).any(), c   # a frame that would be deferred arrives at a full store


def test_decode_sequences_refuses_what_it_can_without_a_device():
    lib = m17hip.load_library()
    assert lib.m17hip_version() >= 612 and "m17hip_decode_sequences" in m17hip.EXPORTS

    def call(ctx=C.c_void_p(), form=0, Cn=1, F=1, cap=2, llr=0, dep=0, state=0, st=0, cost=0, null=None):
        a = dict(llr=np.full((max(Cn, 1), max(F, 1), 368), llr, np.int8), st=np.full((max(Cn, 1), max(F, 1)), st, np.uint8), state=np.full(max(Cn, 1), state, np.uint8),
                 lich=np.zeros(max(Cn, 1), np.uint8), lsf=np.zeros((max(Cn, 1), 30), np.uint8), dep=np.full(max(Cn, 1), dep, np.int8),
                 cost=np.full(max(Cn, 1), cost, np.int64), recs=np.zeros((max(Cn, 1), max(cap, 1)), m17hip.FRAME_REC), nrec=np.zeros(max(Cn, 1), np.uint32),
                 ovf=np.zeros(1, np.uint32), trace=np.full((max(Cn, 1), max(F, 1)), 77, np.int32))
        p = {k: (None if k == null else ol._p(v)) for k, v in a.items()}
        code = lib.m17hip_decode_sequences(ctx, C.c_int(form), p["llr"], p["st"], C.c_uint32(Cn), C.c_uint32(F), C.c_uint32(cap), p["state"], p["lich"], p["lsf"],
                                           p["dep"], p["cost"], p["recs"], p["nrec"], p["ovf"], p["trace"])
        assert (a["trace"] == 77).all() and not a["recs"].tobytes().strip(b"\0") and a["nrec"][0] == 0   # a refusal writes nothing
        return code

    assert call() == -1   # a null context, everything else in order
    for kw in (dict(form=3), dict(form=-1), dict(Cn=0), dict(F=0), dict(cap=0), dict(llr=8), dict(llr=-8), dict(llr=-128), dict(dep=8), dict(dep=-8),
               dict(state=5), dict(st=4), dict(cost=-2), dict(cost=1 << 31), dict(null="llr"), dict(null="trace"), dict(null="ovf")):
        assert call(**kw) == -1, kw
    # the binding looks at the arrays before it calls the library
    ctx = m17hip.Context.__new__(m17hip.Context)
    ctx.lib, ctx.h = lib, C.c_void_p()
    for bad in (np.zeros((2, 3, 367), np.int8), np.zeros((6, 368), np.int8)):
        with pytest.raises(TypeError):
            ctx.decode_sequences(0, bad, np.zeros((2, 3), np.uint8), 4)
    with pytest.raises(TypeError):
        ctx.decode_sequences(0, np.zeros((2, 3, 368), np.int8), np.zeros((3, 2), np.uint8), 4)
    with pytest.raises(m17hip.M17HipError):
        ctx.decode_sequences(0, np.full((1, 1, 368), 8, np.int8), np.zeros((1, 1), np.uint8), 4)
