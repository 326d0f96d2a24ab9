"""ssym_spotter_* under SSYM_STEP_PACED on the GPU against the numpy restatement (tests/paced_watch_ref.py), bit for bit,
through test_gpu_watch's machinery: the profile, the best after every push and the events with the push that emits each,
however a lane is cut into pushes -- among the cuts the one-row, two-row, 63-row and 64-row chunks of the kernel's hand-off
argument; the best against ssym_dtw_spot_step on the prefix; every event's cost against ssym_dtw_align_step on its cut;
planted copies through watch() on a real stream; NaN and infinite frames; every DIMR; SSYM_STEP_SYMMETRIC against
ssym_spotter_create; and every refusal of ssym_spotter_create_step.  Outputs are sentinel-filled before every call."""
import ctypes

import numpy as np
import pytest

import paced_ref
import paced_watch_ref
import watch_ref
from soundsym_amd import Engine, Sound, Spotter, push_sounds, watch
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments
from test_gpu_watch import NO, _W, _bits, _check_split, _frames

pytestmark = pytest.mark.gpu

STEPS = {"symmetric": nat.STEP_SYMMETRIC, "paced": nat.STEP_PACED}


class _PW(_W):
    """_W with a spotter made by ssym_spotter_create_step itself, whatever the step (Engine.spotter takes the plain call for
    "symmetric")."""

    def __init__(self, tgt, dim, n_lanes=1, max_cost=None, dtype="f64", squared=False, step="paced"):
        self.tgt, self.dim, self.n_lanes, self.squared = tgt, dim, n_lanes, squared
        self.e = Engine(metric="dtw", dtype=dtype, squared=squared)
        tf, to = pack_segments(tgt, dim, np.float32 if dtype == "f32" else np.float64)
        self.q = self.e.queries(tf, to, dim)
        self.limit = max_cost
        mc = None if max_cost is None else np.ascontiguousarray(np.broadcast_to(np.asarray(max_cost, dtype=np.float64), (len(tgt),)))
        out = ctypes.c_void_p()
        rc = nat.lib().ssym_spotter_create_step(self.e.ctx, self.q.ptr, n_lanes, None if mc is None else mc.ctypes.data,
                                                STEPS[step], ctypes.byref(out))
        assert rc == nat.SSYM_OK, nat.lib().ssym_last_error(self.e.ctx)
        self.sp = Spotter(self.e, out.value, self.q, n_lanes, step)


def _profiles(lanes, tgt, squared, prof=None):
    prof = {} if prof is None else prof
    for l, lane in enumerate(lanes):
        for t, b in enumerate(tgt):
            if (l, t) not in prof:
                prof[(l, t)] = paced_watch_ref.whole_profile(lane, b, squared)
    return prof


def _limits(prof, n_tgt, lane=0):
    """One threshold per target, the 0.4 quantile of the finite part of its own profile (+inf where there is none)."""
    out = []
    for t in range(n_tgt):
        d = prof[(lane, t)][0]
        d = d[np.isfinite(d)]
        out.append(float(np.quantile(d, 0.4)) if d.size else np.inf)
    return out


# ---- 1. split invariance at every chunk shape of the hand-off argument, with ties ------------------------------------------

TGT_FRAMES = [1, 2, 3, 63, 64, 65, 129, 0]
LANE = 200
SPLITS = {"whole": [0, LANE], "ones": list(range(LANE + 1)),
          "1_2_63_64_65": [0, 1, 3, 3, 66, 130, 195, 195, LANE],           # pushes of 1, 2, 0, 63, 64, 65, 0, 5 rows
          "66_1_2_64": [0, 66, 66, 67, 69, 133, LANE],                     # 66 (a full chunk and a two-row one), 0, 1, 2, 64, 67
          "64_1_2_130": [0, 64, 65, 67, 197, LANE]}                        # a one-row and a two-row push right after a full chunk
KINDS = {"int": (2, True), "real": (13, False)}                             # dim, squared
_DATA = {}


def _data(kind):
    """The lane, the targets and the profile cache of a kind: made once, shared, never written to again."""
    if kind not in _DATA:
        dim, squared = KINDS[kind]
        rng = np.random.default_rng(0x9ACE + dim)
        lane, tgt = _frames(rng, LANE, dim, kind), [_frames(rng, f, dim, kind) for f in TGT_FRAMES]
        _DATA[kind] = (lane, tgt, _profiles([lane], tgt, squared))
    return _DATA[kind]


@pytest.mark.parametrize("limited", [True, False])
@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_split_gives_the_whole(kind, split, limited):
    lane, tgt, prof = _data(kind)
    dim, squared = KINDS[kind]
    w = _PW(tgt, dim, max_cost=_limits(prof, len(tgt)) if limited else None, squared=squared)
    reps = _check_split(w, [lane], [SPLITS[split]], dict(prof))
    w.close()
    assert sum(r.stats["events"] for r in reps.values()) >= 3
    for t, f in enumerate(TGT_FRAMES):                                         # rows no path can end at, and the profile's length
        assert prof[(0, t)][0].shape == ((LANE,) if f else (0,))
    if kind == "int":
        # ties are real: the least value of an end column is held by several rows, and the rule replaces pending events
        assert any(np.count_nonzero(prof[(0, t)][0] == prof[(0, t)][0].min()) > 1 for t in range(len(tgt) - 1))
        assert sum(r.stats["replaced"] for r in reps.values()) > 0


def test_two_lanes_advance_at_different_rates():
    lane, tgt, prof = _data("int")
    rng = np.random.default_rng(0x2A9E5)
    lanes = [lane, _frames(rng, 150, 2, "int")]
    cuts = [[0, 1, 3, 66, 66, 130, 131, 200], [0, 0, 64, 65, 67, 67, 150, 150]]
    both = _profiles(lanes, tgt, True, {k: v for k, v in prof.items()})
    w = _PW(tgt, 2, n_lanes=2, max_cost=_limits(both, len(tgt)), squared=True)
    reps = _check_split(w, lanes, cuts, both)
    w.close()
    assert all(sum(r.stats["events"] for (l, _), r in reps.items() if l == k) >= 3 for k in range(2))


# ---- 2, 3, 4. the best is ssym_dtw_spot_step's on the prefix; spans keep the bounds; costs are ssym_dtw_align_step's ------------

def test_best_is_the_paced_spot_of_the_prefix_and_event_costs_are_the_paced_alignments():
    rng = np.random.default_rng(0x3A9ED)
    dim = 13
    tgt = [_frames(rng, f, dim, "real") for f in (7, 24, 0, 70, 1)]
    lanes = [_frames(rng, f, dim, "real") for f in (150, 90, 130)]
    lanes[0][40:47] = tgt[0]                                                   # as it is
    lanes[2][60:107:2] = tgt[1]                                                # every second frame of the stretch
    lanes[1][10:45] = tgt[3][::2]                                              # each frame of the stretch doubled in the target
    tgt[3][1::2] = tgt[3][::2]
    cuts = [[0, 64, 64, 129, 150], [0, 0, 1, 3, 90], [0, 130, 130, 130, 130]]
    nT = len(tgt)
    prof = _profiles(lanes, tgt, False)
    w = _PW(tgt, dim, n_lanes=3, max_cost=[float(np.quantile(prof[(0, t)][0][np.isfinite(prof[(0, t)][0])], 0.3))
                                           if tgt[t].shape[0] else np.inf for t in range(nT)])
    si, ti = np.repeat(np.arange(3, dtype=np.uint32), nT), np.tile(np.arange(nT, dtype=np.uint32), 3)
    seen = []

    def after(p):
        seen.extend((l, t) + e for (l, t), evs in w.events().items() for e in evs)
        sf, so = pack_segments([lanes[l][:cuts[l][p + 1]] for l in range(3)], dim)
        d = w.e.dictionary(sf, so, dim)
        c1, s1, e1 = w.e.dtw_spot(d, w.q, si, ti, step="paced")
        cost, start, end = w.sp.best()
        assert np.array_equal(_bits(cost.reshape(-1)), _bits(c1)), p
        assert np.array_equal(start.reshape(-1), s1) and np.array_equal(end.reshape(-1), e1), p
        d.close()

    _check_split(w, lanes, cuts, prof, flush_end=False, after_push=after)
    for l in range(3):
        w.sp.flush(l)
        seen.extend((ll, t) + e for (ll, t), evs in w.events().items() for e in evs)
    assert (0, 0, 0.0, 40, 46) in seen and (2, 1, 0.0, 60, 106) in seen and (1, 3, 0.0, 10, 44) in seen
    assert not any(t == 2 for _, t, *_ in seen) and len(seen) >= 10
    assert np.isinf(w.sp.best()[0][:, 2]).all() and (w.sp.best()[2][:, 2] == NO).all()
    # every emitted cost is the paced alignment's on its cut, every span keeps the slope bounds, spans are disjoint
    cf, co = pack_segments([lanes[l][s:e + 1] for l, t, c, s, e in seen], dim)
    d = w.e.dictionary(cf, co, dim)
    cost, length, _, _ = w.e.dtw_align(d, w.q, np.arange(len(seen), dtype=np.uint32), np.array([t for _, t, *_ in seen], dtype=np.uint32),
                                       step="paced")
    for row, (l, t, c, s, e) in enumerate(seen):
        lo, hi = paced_ref.span_bounds(tgt[t].shape[0])
        assert _bits(c) == _bits(cost[row]) and length[row] == tgt[t].shape[0], (row, l, t)
        assert lo <= e - s + 1 <= hi
    for l in range(3):
        for t in range(nT):
            spans = [(s, e) for ll, tt, c, s, e in seen if (ll, tt) == (l, t)]
            assert spans == sorted(spans) and all(a[1] < b[0] for a, b in zip(spans, spans[1:]))
    d.close()
    w.close()


# ---- planted copies through watch() on a real stream ------------------------------------------------------------------------

def test_watch_reports_planted_copies_at_cost_zero_with_one_per_frame_threshold():
    rng = np.random.default_rng(0x0A7CED)
    e = Engine(metric="dtw", dtype="f64")
    rate = 16000.0
    n = 1024 + 256 * 399
    recs = [rng.standard_normal(n), rng.standard_normal(n - 3000)]
    frames = e.mfcc(recs[0], rate).reshape(400, -1)                            # a pushed sound is bit for bit the sound analysed whole
    nc = frames.shape[1]
    feats = [frames[50:67:2], frames[120:131], np.repeat(frames[300:305], 2, axis=0), np.zeros((0, nc))]
    spans = [(50, 66), (120, 130), (300, 304)]
    targets = [Sound(np.zeros(0), rate, f.reshape(-1), "t%d" % k, ncoeffs=nc) for k, f in enumerate(feats)]
    sounds = [Sound.from_samples(r[:1500], rate, engine=e) for r in recs]
    push_sounds(sounds, [r[1500:1501] for r in recs], e)
    wt = watch(sounds, targets, engine=e, step="paced", max_cost_per_frame=1e-9)
    assert wt.spotter.step == "paced"
    got, polls = wt.poll(), 1
    cuts = [1501, 1502, 9000, 9001, 30000, 30000, 33333, 70000, 100000, n]
    for lo, hi in zip(cuts, cuts[1:]):
        push_sounds(sounds, [r[lo:hi] for r in recs], e)
        got += wt.poll()
        polls += 1
    assert len(got) == 3 and sounds[0].num_frames() == 400                     # emitted by polls, before any flush
    got += wt.flush()
    assert [(s, t, sp.start_frame, sp.end_frame) for s, t, sp in got] == [(0, t, lo, hi) for t, (lo, hi) in enumerate(spans)]
    for s, t, sp in got:
        assert sp.cost == 0.0 and sp.cost_per_frame == 0.0 and sp.source_index == 0
    best = wt.best()
    assert [(b.start_frame, b.end_frame, b.cost, b.cost_per_frame) for b in best[0][:3]] == [(lo, hi, 0.0, 0.0) for lo, hi in spans]
    assert not best[0][3] and not best[1][3] and all(b and b.cost_per_frame > 1e-9 for b in best[1][:3])
    wt.close()
    e.close()


# ---- 5. features that are not finite ---------------------------------------------------------------------------------------

def test_a_nan_frame_costs_a_bounded_stretch_paced_and_the_rest_of_the_lane_symmetric():
    lane, target = paced_watch_ref.nan_case()
    fb, cuts = target.shape[0], [0, 90, 101, 102, 125, 400]
    prof = _profiles([lane], [target], False)
    w = _PW([target], 13, max_cost=1e-9 * fb)
    seen = []
    _check_split(w, [lane], [cuts], prof, after_push=lambda p: seen.extend(e for evs in w.events().values() for e in evs))
    assert seen == [(0.0, 120, 130)]                                           # emitted by a push, with no reset in between
    c, s, e_ = w.sp.best()
    assert (c[0, 0], int(s[0, 0]), int(e_[0, 0])) == (0.0, 120, 130)
    w.close()
    sym = _PW([target], 13, max_cost=1e-9 * fb, step="symmetric")
    total = 0
    for lo, hi in zip(cuts, cuts[1:]):
        rc, n, pd, ps, _ = sym.push([lane[lo:hi]])
        assert rc == nat.SSYM_OK
        total += n
        if lo >= 101:
            assert not np.isfinite(pd[0][0]).any()                             # nothing finite after the NaN frame
    assert total + sym.sp.flush(0) == 0
    sym.close()


def test_a_nan_target_frame_and_an_infinite_source_frame():
    rng = np.random.default_rng(0x1F1A)
    dim = 5
    lane = _frames(rng, 150, dim, "real")
    tgt = [_frames(rng, f, dim, "real") for f in (9, 9, 1)]
    lane[110:119] = tgt[1]
    tgt[0][4, 2] = np.nan                                                      # on every path of target 0
    lane[70, 1] = np.inf
    prof = _profiles([lane], tgt, False)
    assert not np.isfinite(prof[(0, 0)][0]).any()
    d1 = prof[(0, 1)][0]
    lo = paced_ref.span_bounds(9)[0]
    bad = np.flatnonzero(~np.isfinite(d1[lo - 1:])) + lo - 1
    assert bad.size and bad.min() >= 70 and bad.max() <= 70 + 2 * 9 - 2        # no later end has frame 70 in its span
    assert np.flatnonzero(~np.isfinite(prof[(0, 2)][0])).tolist() == [70]
    w = _PW(tgt, dim)
    reps = _check_split(w, [lane], [[0, 1, 2, 66, 71, 72, 73, 150]], prof)
    c, s, e_ = w.sp.best()
    assert np.isinf(c[0, 0]) and s[0, 0] == NO and e_[0, 0] == NO and reps[(0, 0)].stats["events"] == 0
    assert (c[0, 1], int(s[0, 1]), int(e_[0, 1])) == (0.0, 110, 118)
    w.close()


# ---- 6. every DIMR and its padding edges -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 14, 15, 16, 17, 40, 41, 64])
def test_every_dimr(dim):
    rng = np.random.default_rng(0xD1A9 + dim)
    lane, tgt = _frames(rng, 130, dim, "real"), [_frames(rng, 5, dim, "real"), _frames(rng, 70, dim, "real")]
    w = _PW(tgt, dim)
    reps = _check_split(w, [lane], [[0, 1, 64, 65, 130]], _profiles([lane], tgt, False))
    w.close()
    assert sum(r.stats["events"] for r in reps.values()) >= 2


# ---- 7. SSYM_STEP_SYMMETRIC is ssym_spotter_create ------------------------------------------------------------------------

def test_the_symmetric_step_is_the_plain_spotter():
    rng = np.random.default_rng(0x5E9)
    tgt = [_frames(rng, f, 3, "int") for f in (1, 4, 65, 0)]
    lane = _frames(rng, 150, 3, "int")
    cuts = [0, 1, 3, 66, 66, 130, 150]
    a, b = _W(tgt, 3, max_cost=9.0, squared=True), _PW(tgt, 3, max_cost=9.0, squared=True, step="symmetric")
    _check_split(b, [lane], [cuts], flush_end=False)                           # against watch_ref: the symmetric restatement
    events = 0
    for lo, hi in zip(cuts, cuts[1:]):
        ra = a.push([lane[lo:hi]])
        assert ra[0] == nat.SSYM_OK
        events += ra[1]
    b.sp.reset(0)
    for lo, hi in zip(cuts, cuts[1:]):
        rb = b.push([lane[lo:hi]])
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a.sp.best(), b.sp.best()))
    assert a.events() == b.events() and a.sp.flush(0) == b.sp.flush(0) and a.events() == b.events() and events >= 3
    a.close()
    b.close()


# ---- 8. errors ------------------------------------------------------------------------------------------------------------

def test_every_refusal_of_create_step_names_it_and_leaves_null():
    L, fn = nat.lib(), b"ssym_spotter_create_step"
    e = Engine(metric="dtw", dtype="f64")
    q = e.queries(np.zeros(10), np.array([0, 1, 2], dtype=np.uint64), 5)
    long_q = e.queries(np.zeros(2049), np.array([0, 2049], dtype=np.uint64), 1)
    edge_q = e.queries(np.zeros(2048), np.array([0, 2048], dtype=np.uint64), 1)
    nan = np.array([1.0, np.nan])
    INV, UNS = nat.SSYM_E_INVALID, nat.SSYM_E_UNSUPPORTED

    def refused(ctx, qp, lanes, max_cost, step, want, text=b""):
        out = ctypes.c_void_p(7)
        rc = L.ssym_spotter_create_step(ctx, qp, lanes, None if max_cost is None else max_cost.ctypes.data, step, ctypes.byref(out))
        err = L.ssym_last_error(ctx)
        assert rc == want and out.value is None and err.startswith(fn + b": ") and text in err, (rc, err)

    for step in (2, 7, 0xFFFFFFFF):
        refused(e.ctx, q.ptr, 1, None, step, INV, b"step must be SSYM_STEP_SYMMETRIC or SSYM_STEP_PACED")
    refused(e.ctx, long_q.ptr, 1, None, nat.STEP_PACED, UNS, b"more than 2048 frames")
    refused(e.ctx, q.ptr, 1, nan, nat.STEP_PACED, INV, b"max_cost[1] is NaN")
    refused(e.ctx, None, 1, None, nat.STEP_PACED, INV)
    refused(e.ctx, q.ptr, 0, None, nat.STEP_PACED, INV)
    assert L.ssym_spotter_create_step(e.ctx, q.ptr, 1, None, nat.STEP_PACED, None) == INV
    assert L.ssym_last_error(e.ctx) == fn + b": out is NULL"
    for kw in (dict(band=4), dict(metric="refcos")):
        e2 = Engine(dtype="f64", **kw)
        q2 = e2.queries(np.zeros(10), np.array([0, 2], dtype=np.uint64), 5)
        for step in STEPS.values():
            refused(e2.ctx, q2.ptr, 1, None, step, UNS)
        e2.close()
    # what paced refuses the symmetric step takes, and the limit itself is taken by both
    for qq, step in ((long_q, nat.STEP_SYMMETRIC), (edge_q, nat.STEP_SYMMETRIC), (edge_q, nat.STEP_PACED)):
        out = ctypes.c_void_p()
        assert L.ssym_spotter_create_step(e.ctx, qq.ptr, 1, None, step, ctypes.byref(out)) == nat.SSYM_OK and out.value
        assert L.ssym_spotter_destroy(e.ctx, out.value) == nat.SSYM_OK
    with pytest.raises(nat.SsymError) as err:
        e.spotter(long_q, 1, step="paced")
    assert err.value.code == UNS
    # a spotter is untouched by the refusals around it: it goes on to the restatement's result
    rng = np.random.default_rng(0xE779)
    tgt, lane = [_frames(rng, f, 5, "int") for f in (4, 6)], _frames(rng, 80, 5, "int")
    w = _PW(tgt, 5, squared=True)
    rc, *_ = w.push([lane[:30]])
    assert rc == nat.SSYM_OK
    refused(w.e.ctx, w.q.ptr, 1, None, 9, INV)
    refused(w.e.ctx, w.q.ptr, 1, nan, nat.STEP_PACED, INV)
    x, off = lane[30:40].reshape(-1).copy(), np.array([10, 0], dtype=np.uint64)
    out = w.call(lambda n, pd, ps, f: L.ssym_spotter_push(w.e.ctx, w.sp.ptr, x.ctypes.data, off.ctypes.data, f, n, pd, ps), [10])
    assert out[0] == INV and out[1] == 0xDEADBEEF and (out[4][0] == -12345.5).all() and w.sp.counts()[0] == 30
    rc, nev, pd, ps, _ = w.push([lane[30:]])
    for t in range(2):
        d, s = paced_watch_ref.whole_profile(lane, tgt[t], True)
        assert rc == nat.SSYM_OK and np.array_equal(_bits(pd[0][t]), _bits(d[30:])) and np.array_equal(ps[0][t], s[30:])
    w.close()
    e.close()
