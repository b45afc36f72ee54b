"""BASELINE configs[4] on the device: the impairment grid in one synthesis (m17hip_synth_sweep_i16), the per-channel sweep words
(m17hip_sweep_stats) and the sweep tool (tools/impairment_sweep.py), against single-point synthesis, the per-channel fetches and the oracle."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import m17hip
import oracle_lib as ol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import impairment_sweep  # noqa: E402

EINVAL, ESTATE, EOVERFLOW = -1, -4, -5
NCPU = min(16, os.cpu_count() or 1)
POINTS5 = np.array([(0.0, 100.0, 0.0, 1.0), (400.0, 400.0, 1000.0, 0.7), (800.0, 900.0, -2500.0, 1.2), (1500.0, 1500.0, 2500.0, 1.0),
                    (4000.0, 4000.0, -1000.0, 0.9)], dtype=m17hip.IMPAIRMENT_DTYPE)


def _points(n):
    return {1: POINTS5[1:2], 5: POINTS5, 30: impairment_sweep.grid()}[n]


def _kw(T, kind=0, seed=4242):
    return dict(seed=seed, kind=kind, n_frames=T // 1920 + 2, lead_in=3072, lead_sigma=40000.0, total=T)


def _base(T, kind=0):
    return ol.gen_params(noise_sigma=123.0, tail_sigma=456.0, dc_offset=-7.0, gain=1.5, **_kw(T, kind))   # (replaced by every point)


def _at(T, pt, kind=0):
    """The single-point parameters of `pt`: what m17hip_synth_sweep_i16 must equal."""
    return ol.gen_params(noise_sigma=float(pt["noise_sigma"]), tail_sigma=float(pt["tail_sigma"]), dc_offset=float(pt["dc_offset"]),
                         gain=float(pt["gain"]), **_kw(T, kind))


def _hip():
    return C.CDLL("libamdhip64.so")


@pytest.mark.parametrize("n_points,chan0,Cn,T,kind,stage", [
    (1, 0, 7, 24000, 0, False),
    (5, 1000, 23, 24000 + 77, -1, False),
    (30, 0, 61, 48000 + 13, 0, False),
    (30, 1000, 37, 9600 + 5, -1, True),
    (5, 0, 12, 30000 + 100, 0, True),
])
def test_grid_synthesis_equals_single_point_synthesis(n_points, chan0, Cn, T, kind, stage):
    pts = _points(n_points)
    ctx = m17hip.Context(Cn, T)
    if stage:   # key 16: the grid goes to the staging slab; the run that follows takes it, and the slab it ran on is read back
        ctx.tune(16, 1)
    ctx.synth_sweep(_base(T, kind), pts, Cn, T, chan0=chan0)
    if stage:
        ctx.reset(); ctx.run()
    x = ctx.download()
    ctx.close()
    one = m17hip.Context(Cn, T)
    for p in range(n_points):
        one.synth(_at(T, pts[p], kind), Cn, T, chan0=chan0)
        y = one.download()
        rows = [c for c in range(Cn) if (chan0 + c) % n_points == p]
        assert rows
        assert np.array_equal(x[rows], y[rows]), (p, rows)
    one.close()
    for c in sorted({0, Cn // 2, Cn - 1}):   # ... and the test generator
        g = chan0 + c
        ref = ol.generate_batch(_at(T, pts[g % n_points], kind), 1, T, threads=1, chan0=g)
        assert np.array_equal(x[c], ref[0]), c


def _words_vs_fetches(ctx, Cn, P, base):
    w = ctx.sweep_stats(P, Cn)
    st, d = ctx.bert_stats(Cn), ctx.diag(Cn)
    for f in ("bits", "errors", "synced", "frames"):
        assert np.array_equal(w[f], st[f]), f
    assert w["evm"].tobytes() == d["evm"].tobytes()
    assert np.array_equal(w["channel"], base + np.arange(Cn, dtype=np.uint32))
    assert np.array_equal(w["point"], (base + np.arange(Cn)) % P)
    assert np.all(w["flags"] == 1)
    return w


def test_sweep_stats_equal_bert_stats_and_diag():
    Cn, T, P, base = 96, 48000, 30, 1000
    ctx = m17hip.Context(Cn, T)
    ctx.tune(6, 1)
    ctx.set_channel_base(base)
    ctx.synth_sweep(_base(T), impairment_sweep.grid(), Cn, T, chan0=base)
    ctx.reset(); ctx.run()
    w = _words_vs_fetches(ctx, Cn, P, base)
    assert (w["bits"] > 0).mean() >= 0.9 and (w["frames"] > 0).mean() >= 0.9   # (the loudest points lose a channel now and then)
    ctx.run()   # a continued stream: the PRBS9 counts go on, the words follow
    _words_vs_fetches(ctx, Cn, P, base)
    ctx.close()


def test_sweep_stats_wait_for_the_staged_run_in_flight():
    """A fresh context: an in-place first run, then staged input, front, run and sweep_stats at once (no synchronisation in between): the words
    are those the same call returns after hipDeviceSynchronize, and those of the same two runs made one at a time."""
    Cn, T, P = 2048, 96000, 30
    pts = impairment_sweep.grid()
    hip = _hip()

    def two_runs(wait):
        ctx = m17hip.Context(Cn, T)
        ctx.tune(6, 1)
        ctx.synth_sweep(_base(T), pts, Cn, T, chan0=0)
        ctx.reset(); ctx.run()
        if wait:
            assert hip.hipDeviceSynchronize() == 0
        ctx.tune(16, 1)
        ctx.synth_sweep(_base(T), pts, Cn, T, chan0=Cn)
        ctx.tune(16, 0)
        if wait:
            assert hip.hipDeviceSynchronize() == 0
        ctx.front(); ctx.run()
        if wait:
            assert hip.hipDeviceSynchronize() == 0
        w = ctx.sweep_stats(P, Cn)
        assert hip.hipDeviceSynchronize() == 0
        again = ctx.sweep_stats(P, Cn)
        ctx.close()
        return w, again

    fast, fast_again = two_runs(False)
    slow, _ = two_runs(True)
    assert fast.tobytes() == fast_again.tobytes()
    assert fast.tobytes() == slow.tobytes()
    assert fast["frames"].sum() > 0


def test_one_grid_run_equals_point_by_point_runs_and_the_oracle():
    Cn, T, P = 90, 48000, 30
    pts = impairment_sweep.grid()
    ctx = m17hip.Context(Cn, T)
    ctx.tune(6, 1)
    ctx.synth_sweep(_base(T), pts, Cn, T)
    x = ctx.download()
    ctx.reset(); ctx.run()
    w = ctx.sweep_stats(P, Cn)
    got = ctx.frames()
    ctx.close()
    one = m17hip.Context(Cn, T)
    one.tune(6, 1)
    for p in range(P):
        one.synth(_at(T, pts[p]), Cn, T)
        one.reset(); one.run()
        st, d = one.bert_stats(Cn), one.diag(Cn)
        for c in range(p, Cn, P):
            assert (int(w["bits"][c]), int(w["errors"][c]), int(w["synced"][c]), int(w["frames"][c])) == \
                (int(st["bits"][c]), int(st["errors"][c]), int(st["synced"][c]), int(st["frames"][c])), (p, c)
            assert w["evm"][c].tobytes() == d["evm"][c].tobytes(), (p, c)
    one.close()
    rows = [0, 7, 29, 44, 61, 89]
    recs, counts, diags = ol.demod_batch(x[rows], cap=2 * (T // 1920 + 2) + 4, threads=NCPU)
    for i, c in enumerate(rows):
        e = recs[i, : counts[i]].copy()
        e["channel"] = c
        assert got[got["channel"] == c].tobytes() == e.tobytes(), c
        bert = e[e["frame_type"] == 5]
        bits, errs, sync = ol.bert_count(bert["payload"][:, :25]) if bert.size else (0, 0, False)
        assert (int(w["bits"][c]), int(w["errors"][c]), bool(w["synced"][c]), int(w["frames"][c])) == (bits, errs, bool(sync), bert.size), c
        assert w["evm"][c].tobytes() == diags["evm"][i].tobytes(), c


def test_sweep_error_paths():
    Cn, T = 8, 48000
    ctx = m17hip.Context(Cn, T)
    lib, h = ctx.lib, ctx.h
    base = _base(T)
    good = POINTS5.copy()

    def synth(pts, n=None):
        ptr = None if pts is None else pts.ctypes.data_as(C.c_void_p)
        return lib.m17hip_synth_sweep_i16(h, C.byref(base), ptr, C.c_uint32(len(pts) if n is None else n), C.c_uint32(Cn), C.c_uint32(T), C.c_uint32(0))

    assert synth(None, 5) == EINVAL
    assert synth(good, 0) == EINVAL
    big = np.resize(good, m17hip.MAX_SWEEP_POINTS + 1)
    assert synth(big) == EINVAL
    assert synth(np.resize(good, m17hip.MAX_SWEEP_POINTS)) == 0
    for field, value in (("noise_sigma", np.nan), ("tail_sigma", np.nan), ("noise_sigma", -1.0), ("tail_sigma", -0.5), ("gain", np.inf),
                         ("gain", np.nan), ("dc_offset", -np.inf)):
        bad = good.copy()
        bad[field][3] = value
        assert synth(bad) == EINVAL, (field, value)
    bad_base = _base(T)
    bad_base.kind = 9
    assert lib.m17hip_synth_sweep_i16(h, C.byref(bad_base), good.ctypes.data_as(C.c_void_p), C.c_uint32(5), C.c_uint32(Cn), C.c_uint32(T), C.c_uint32(0)) == EINVAL
    assert synth(good) == 0
    ctx.synth_sweep(base, good, Cn, T)   # (the binding: the context's channels / samples for run())

    w = np.zeros(Cn, dtype=m17hip.CHAN_STAT_DTYPE)

    def stats(P=5):
        return lib.m17hip_sweep_stats(h, C.c_uint32(P), w.ctypes.data_as(C.c_void_p), C.c_uint32(Cn))

    assert stats(0) == EINVAL
    ctx.tune(6, 1)
    assert stats() == ESTATE              # no run yet
    ctx.reset(); ctx.run()
    assert stats() == 0 and np.all(w["flags"] == 1)
    good_w = w.copy()
    ctx.reset()
    assert stats() == ESTATE              # no run since the reset
    ctx.run()
    ctx.tune(6, 0)
    assert stats() == ESTATE              # BERT statistics off
    ctx.tune(6, 1)
    ctx.tune(18, 64)                      # 64 deferred EVM operations per channel: a 48 000-sample run writes thousands
    ctx.reset(); ctx.run()
    w[:] = 0
    assert stats() == EOVERFLOW
    assert np.all(w["flags"] == 0)
    for f in ("channel", "point", "bits", "errors", "synced", "frames"):
        assert np.array_equal(w[f], good_w[f]), f
    assert ctx.sweep_stats(5, Cn)["flags"].sum() == 0   # (the binding hands such words over)
    ctx.tune(18, 0)
    ctx.reset(); ctx.run()
    assert stats() == 0 and w.tobytes() == good_w.tobytes()
    ctx.close()


def test_sweep_tool_one_gpu_checks_against_the_oracle():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "impairment_sweep.py"), "--gpus", "1", "--channels", "2048", "--samples", "48000",
                        "--slab", "1000", "--check", "1"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(res["points"]) == 30 and sum(p["channels"] for p in res["points"]) == 2048
    assert res["parity_vs_oracle"] == {"checked": 30, "mismatches": 0}
    assert res["world"] == 1 and res["channels"] == 2048 and res["samples"] == 48000
    assert all(p["frames"] > 0 for p in res["points"])
    assert res["msamples_per_s"] > 0 and res["msamples_per_s_runs"] >= res["msamples_per_s"]
