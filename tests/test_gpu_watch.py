"""ssym_spotter_* on the GPU against the numpy restatement (tests/watch_ref.py), bit for bit: the profile, the best after
every push and the events with the push that emits each, however a lane is cut into pushes; against ssym_dtw_spot on the
prefix and ssym_pair_matrix(exact = 1) on the cuts; follow on a real stream, flush, reset, the slice path, watch(), and every
error the header lists.  Outputs are sentinel-filled before every call."""
import ctypes

import numpy as np
import pytest

import spot_ref
import watch_ref
from dtw_path_ref import same_floats
from soundsym_amd import Engine, Sound, push_sounds, watch
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

SENT32, SENTF = 0xDEADBEEF, -12345.5
NO = nat.NO_MATCH


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _frames(rng, f, dim, kind):
    if kind == "int":
        return rng.integers(0, 3, size=(f, dim)).astype(np.float64)        # {0, 1, 2}: exact sums, real ties
    if kind == "zero":
        return np.zeros((f, dim))                                          # digital silence: every cost ties
    return rng.standard_normal((f, dim)).astype(np.float32).astype(np.float64)   # (f32 values: both dtypes hold them)


class _W:
    """An engine, a resident query set and a spotter over `n_lanes` lanes; push() goes through ctypes into sentinel-filled
    outputs and returns what the call wrote."""

    def __init__(self, tgt, dim, n_lanes=1, max_cost=None, dtype="f64", squared=False):
        self.tgt, self.dim, self.n_lanes, self.squared = tgt, dim, n_lanes, squared
        self.e = Engine(metric="dtw", dtype=dtype, squared=squared)
        tf, to = pack_segments(tgt, dim, np.float32 if dtype == "f32" else np.float64)
        self.q = self.e.queries(tf, to, dim)
        self.limit = max_cost
        self.sp = self.e.spotter(self.q, n_lanes, max_cost)

    def close(self):
        self.sp.close()
        self.e.close()

    def limit_of(self, t):
        return None if self.limit is None else float(np.broadcast_to(self.limit, (len(self.tgt),))[t])

    def call(self, fn, rows, device=False):
        """fn(n_events*, profile cost*, profile start*, flags) with sentinel-filled profile outputs one entry longer than
        needed: (rc, n_events, cost [lane][target][row], start ...)."""
        total = int(np.sum(rows)) * len(self.tgt)
        pd, ps = np.full(total + 1, SENTF), np.full(total + 1, SENT32, dtype=np.uint32)
        n = ctypes.c_uint64(SENT32)
        if device:
            import torch
            dd, ds = torch.from_numpy(pd).cuda(), torch.from_numpy(ps.view(np.int32)).cuda()
            rc = fn(ctypes.byref(n), dd.data_ptr(), ds.data_ptr(), nat.OUT_DEVICE)
            torch.cuda.synchronize()
            pd, ps = dd.cpu().numpy(), ds.cpu().numpy().view(np.uint32)
        else:
            rc = fn(ctypes.byref(n), pd.ctypes.data, ps.ctypes.data, 0)
        if rc == nat.SSYM_OK:
            assert pd[total] == SENTF and ps[total] == SENT32
        cuts = np.cumsum([0] + [int(r) * len(self.tgt) for r in rows])
        shape = lambda x: [x[cuts[l]:cuts[l + 1]].reshape(len(self.tgt), int(rows[l])) for l in range(self.n_lanes)]
        return rc, n.value, shape(pd), shape(ps), (pd, ps)

    def push(self, chunks, device=False):
        x = np.concatenate([np.asarray(c, dtype=np.float64).reshape(-1) for c in chunks] + [np.zeros(1)])
        off = np.cumsum([0] + [len(c) for c in chunks]).astype(np.uint64)
        fn = lambda n, pd, ps, flags: nat.lib().ssym_spotter_push(self.e.ctx, self.sp.ptr, x.ctypes.data, off.ctypes.data,
                                                                  flags, n, pd, ps)
        out = self.call(fn, [len(c) for c in chunks], device)
        self.sp.n_events = out[1] if out[0] == nat.SSYM_OK else 0
        return out

    def events(self):
        """{(lane, target): [(cost, start, end), ...]} of the last call, and the order check."""
        lane, tgt, cost, start, end = self.sp.events()
        keys = list(zip(lane.tolist(), tgt.tolist(), end.tolist()))
        assert keys == sorted(keys)                                        # ordered by (lane, target, end)
        out = {}
        for k in range(lane.size):
            out.setdefault((int(lane[k]), int(tgt[k])), []).append((float(cost[k]), int(start[k]), int(end[k])))
        return out


def _same_events(got, want):
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        assert _bits(g[0]) == _bits(w[0]) and g[1:] == w[1:], (g, w)


def _check_split(w, lanes, cut_lists, profiles=None, flush_end=True, after_push=None):
    """Feed lane l its frames cut at cut_lists[l] (all lists equally long: push p takes rows cuts[p] ... cuts[p+1] - 1 of
    every lane) and compare every push with the restatement: the profile by NaN mask and then bit for bit (a NaN's sign
    and payload are the processor's own), everything else bit for bit.  after_push(p), when given, runs after push p has
    been compared.  Returns the restatement's Reporters."""
    nT, nL = len(w.tgt), len(lanes)
    prof = profiles if profiles is not None else {}
    want = {}
    for l in range(nL):
        for t in range(nT):
            if (l, t) not in prof:
                prof[(l, t)] = watch_ref.whole_profile(lanes[l], w.tgt[t], w.squared)
            want[(l, t)] = watch_ref.drive(*prof[(l, t)], cut_lists[l], w.limit_of(t),
                                           flush_after=(len(cut_lists[l]) - 2,) if flush_end else ())
    for p in range(len(cut_lists[0]) - 1):
        chunks = [lanes[l][cut_lists[l][p]:cut_lists[l][p + 1]] for l in range(nL)]
        rc, n, pd, ps, _ = w.push(chunks)
        assert rc == nat.SSYM_OK, nat.lib().ssym_last_error(w.e.ctx)
        ev = w.events()
        assert n == sum(len(v) for v in ev.values()) == sum(len(want[k][0][p]) for k in want)
        cost, start, end = w.sp.best()
        for (l, t), (per_push, bests, _, _) in want.items():
            lo, hi = cut_lists[l][p], cut_lists[l][p + 1]
            d, s = prof[(l, t)]
            if d.size:
                assert np.array_equal(np.isnan(pd[l][t]), np.isnan(d[lo:hi])), (l, t, p)
                assert same_floats(pd[l][t], d[lo:hi]), (l, t, p)
                assert np.array_equal(ps[l][t], s[lo:hi].astype(np.uint32)), (l, t, p)
            else:                                               # a target without frames: "no path" in every new row
                assert (pd[l][t] == np.inf).all() and (ps[l][t] == NO).all(), (l, t, p)
            _same_events(ev.get((l, t), []), per_push[p])
            assert _bits(cost[l, t]) == _bits(bests[p][0]) and (int(start[l, t]), int(end[l, t])) == bests[p][1:], (l, t, p)
        if after_push is not None:
            after_push(p)
    assert np.array_equal(w.sp.counts(), [c[-1] for c in cut_lists])
    if flush_end:
        for l in range(nL):
            n = w.sp.flush(l)
            ev = w.events()
            assert n == sum(len(v) for v in ev.values())
            for t in range(nT):
                _same_events(ev.get((l, t), []), want[(l, t)][2][len(cut_lists[l]) - 2])
    return {k: v[3] for k, v in want.items()}


TGT_FRAMES = [1, 2, 63, 64, 65, 129]      # one column, the 64-step refill, ring 64 vs 128
LANE = 200
_RANDOM = [0, 0, 17, 17, 17, 80, 81, 144, 144, 145, 199, LANE, LANE]          # empty pushes, first, middle and last
SPLITS = {"whole": [0, LANE], "ones": list(range(LANE + 1)), "63": list(range(0, LANE, 63)) + [LANE],
          "64": list(range(0, LANE, 64)) + [LANE], "65": list(range(0, LANE, 65)) + [LANE], "random": _RANDOM}
_DATA = {}


def _data(kind):
    if kind not in _DATA:
        rng = np.random.default_rng(0xA7C4 + len(kind))
        _DATA[kind] = (_frames(rng, LANE, 3, kind), [_frames(rng, f, 3, kind) for f in TGT_FRAMES], {})
    return _DATA[kind]


# ---- 1. split invariance at every chunk and refill edge, with ties ------------------------------------------------------

@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("kind,squared,dtype", [("int", True, "f64"), ("real", False, "f32"), ("zero", False, "f64")])
def test_every_split_gives_the_whole(kind, squared, dtype, split):
    lane, tgt, prof = _data(kind)
    d0 = watch_ref.whole_profile(lane, tgt[2], squared)[0]
    limit = None if kind == "zero" else [None, float(np.quantile(d0, 0.4))][squared]
    w = _W(tgt, 3, max_cost=limit, dtype=dtype, squared=squared)
    reps = _check_split(w, [lane], [SPLITS[split]], prof)
    w.close()
    assert sum(r.stats["events"] for r in reps.values()) >= 3
    if kind != "real":
        # ties are real: the least value of an end column is held by several rows, and backtraces pass tied cells
        assert any(np.count_nonzero(prof[(0, t)][0] == prof[(0, t)][0].min()) > 1 for t in range(len(tgt)))
        D = spot_ref.matrices(lane, tgt[3], squared)[0]
        dg, up, lf = D[:-1, :-1], D[:-1, 1:], D[1:, :-1]
        least = np.minimum(np.minimum(dg, up), lf)
        assert np.count_nonzero((dg == least).astype(int) + (up == least) + (lf == least) > 1) > 100      # min3 and the predecessor rule


# ---- 2. every DIMR and its padding edges ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [13, 14, 16, 40, 41, 64])
def test_every_dimr(dim):
    rng = np.random.default_rng(0xD1A + dim)
    lane, tgt = _frames(rng, 70, dim, "real"), [_frames(rng, 9, dim, "real"), _frames(rng, 2, dim, "int")]
    w = _W(tgt, dim)
    _check_split(w, [lane], [[0, 1, 64, 70]])
    w.close()


# ---- 3. lanes at different progress; the best is ssym_dtw_spot's on the prefix; costs are the exact kernel's ---------------

def test_three_lanes_at_different_progress_against_spot_and_pair_matrix():
    rng = np.random.default_rng(0x3A9E)
    dim = 13
    tgt = [_frames(rng, f, dim, "real") for f in (7, 24, 0, 70)]
    lanes = [_frames(rng, f, dim, "real") for f in (150, 90, 130)]
    lanes[0][40:47] = tgt[0]
    lanes[2][100:124] = tgt[1]
    cuts = [[0, 64, 64, 129, 150], [0, 0, 1, 1, 90], [0, 130, 130, 130, 130]]
    w = _W(tgt, dim, n_lanes=3)
    nT = len(tgt)
    want = {(l, t): watch_ref.watch(lanes[l], tgt[t], cuts[l], flush_after=(3,)) for l in range(3) for t in range(nT)}
    seen = []
    for p in range(4):
        rc, n, pd, ps, _ = w.push([lanes[l][cuts[l][p]:cuts[l][p + 1]] for l in range(3)])
        assert rc == nat.SSYM_OK
        ev = w.events()
        assert n == sum(len(v) for v in ev.values()) == sum(len(v[0][p]) for v in want.values())
        for k, v in want.items():
            _same_events(ev.get(k, []), v[0][p])
        seen += [(l, t) + e for (l, t), evs in ev.items() for e in evs]
        # consequence 2: ssym_dtw_spot on the frames consumed so far
        pre = [lanes[l][:cuts[l][p + 1]] for l in range(3)]
        sf, so = pack_segments(pre, dim)
        d = w.e.dictionary(sf, so, dim)
        si, ti = np.repeat(np.arange(3, dtype=np.uint32), nT), np.tile(np.arange(nT, dtype=np.uint32), 3)
        c1, s1, e1 = w.e.dtw_spot(d, w.q, si, ti)
        cost, start, end = w.sp.best()
        assert np.array_equal(_bits(cost.reshape(-1)), _bits(c1))
        assert np.array_equal(start.reshape(-1), s1) and np.array_equal(end.reshape(-1), e1)
        d.close()
    tm = w.e.timings()
    assert tm["n_pairs"] == 3 * nT
    for l in range(3):                                                     # the lanes end: what is pending comes out
        w.sp.flush(l)
        ev = w.events()
        assert set(k[0] for k in ev) <= {l}
        for t in range(nT):
            _same_events(ev.get((l, t), []), want[(l, t)][2][3])
        seen += [(l, t) + e for (l, t), evs in ev.items() for e in evs]
    assert len(seen) >= 3 and (2, 1, 0.0, 100, 123) in seen and (0, 0, 0.0, 40, 46) in seen
    assert not any(t == 2 for _, t, *_ in seen)                            # a target without frames never reports
    assert np.isinf(w.sp.best()[0][:, 2]).all() and (w.sp.best()[2][:, 2] == NO).all()
    # consequence 4: every emitted cost is ssym_pair_matrix(exact = 1) on its cut; consequence 3: disjoint, ascending
    cf, co = pack_segments([lanes[l][s:e + 1] for l, t, c, s, e in seen], dim)
    d = w.e.dictionary(cf, co, dim)
    plain = w.e.pair_matrix(d, w.q, exact=True)
    for row, (l, t, c, s, e) in enumerate(seen):
        assert _bits(c) == _bits(plain[row, t])
    for l in range(3):
        for t in range(nT):
            spans = sorted((s, e) for ll, tt, c, s, e in seen if (ll, tt) == (l, t))
            assert all(a[1] < b[0] for a, b in zip(spans, spans[1:]))
    w.close()


# ---- 4. more pairs than workgroups: grid stride and state indexing --------------------------------------------------------

def test_2200_pairs_walk_the_grid_stride():
    rng = np.random.default_rng(0x2200)
    tgt = [_frames(rng, 3, 2, "int") for _ in range(1100)]
    lanes = [_frames(rng, 70, 2, "int"), _frames(rng, 66, 2, "int")]
    assert 2 * 1100 > 8 * 256
    w = _W(tgt, 2, n_lanes=2, max_cost=1.0, squared=True)
    reps = _check_split(w, lanes, [[0, 65, 70], [0, 1, 66]])
    assert sum(r.stats["events"] for r in reps.values()) > 2200
    w.close()


# ---- 5. follow on a real stream, with a push that makes the lane buffer move ----------------------------------------------

def test_follow_reads_the_stream_in_place_and_equals_push():
    rng = np.random.default_rng(0xF011)
    e = Engine(metric="dtw", dtype="f64")
    st = e.stream(2, 16000.0, ncoeffs=12, capacity=4096)
    tgt_wave = rng.standard_normal(1024 + 256 * 5)
    tgt = e.mfcc(tgt_wave, 16000.0, 12)
    tf, to = pack_segments([tgt, tgt[:3]], 12)
    q = e.queries(tf, to, 12)
    a, b = e.spotter(q, 2), e.spotter(q, 2)
    waves = [np.concatenate([rng.standard_normal(3072), tgt_wave, rng.standard_normal(40000)]), rng.standard_normal(30000)]
    blocks = [(0, 2000), (2000, 2100), (2100, 4000), (4000, 44000)]       # the last one outgrows the capacity: the buffer moves
    before = st.frames_device(0).ptr
    for lo, hi in blocks:
        chunk = [x[lo:hi] for x in waves]
        held = st.counts()[1].astype(int)
        st.push(np.concatenate(chunk), np.cumsum([0] + [c.size for c in chunk]))
        na, pda, psa = a.follow(st, want_profile=True)
        ev_a = a.events()
        new = [st.read(l, int(held[l])) for l in range(2)]
        nb, pdb, psb = b.push(np.concatenate(new), np.cumsum([0] + [x.shape[0] for x in new]), want_profile=True)
        ev_b = b.events()
        assert na == nb and all(np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                                               y.view(np.uint64) if y.dtype == np.float64 else y) for x, y in zip(ev_a, ev_b))
        for l in range(2):
            assert np.array_equal(_bits(pda[l]), _bits(pdb[l])) and np.array_equal(psa[l], psb[l])
    assert st.frames_device(0).ptr != before and np.array_equal(a.counts(), st.counts()[1])
    # the whole against the restatement, and the target found where it was put
    for l in range(2):
        whole = st.read(l)
        d, s = watch_ref.whole_profile(whole, tgt)
        c, s0, e0 = a.best()
        end = int(np.argmin(d))
        assert _bits(c[l, 0]) == _bits(d[end]) and (int(s0[l, 0]), int(e0[l, 0])) == (int(s[end]), end)
    # a stream reset without a spotter reset is refused and names the remedy; after the reset the lane starts over
    st.reset(1)
    with pytest.raises(nat.SsymError) as err:
        a.follow(st)
    assert err.value.code == nat.SSYM_E_INVALID and b"ssym_spotter_reset" in nat.lib().ssym_last_error(e.ctx)
    assert np.array_equal(a.counts(), b.counts())                          # the refused call changed nothing
    a.reset(1)
    st.push(np.concatenate([np.zeros(0), waves[1][:5000]]), [0, 0, 5000])
    a.follow(st)
    fresh = e.spotter(q, 1)
    fresh.push(st.read(1))
    assert np.array_equal(_bits(a.best()[0][1]), _bits(fresh.best()[0][0])) and a.counts()[1] == st.counts()[1][1]
    for x in (a, b, fresh):
        x.close()
    e.close()


# ---- 6. the slice path ----------------------------------------------------------------------------------------------------

def test_a_small_scratch_limit_runs_slices_with_the_same_results(monkeypatch):
    rng = np.random.default_rng(0x511C)
    tgt = [_frames(rng, f, 3, "int") for f in (4, 9, 65)]
    lanes = [_frames(rng, 150, 3, "int"), _frames(rng, 40, 3, "int")]
    monkeypatch.setenv("SSYM_SPOTTER_SCRATCH_BYTES", str(12 * 3 * 2 * 23))      # 23 rows of a lane per slice
    w = _W(tgt, 3, n_lanes=2, max_cost=[9.0, 18.0, 120.0], squared=True)
    reps = _check_split(w, lanes, [[0, 150], [0, 40]])
    assert w.e.timings()["main_launches"] == 0                                # (the last call was a flush)
    assert sum(r.stats["events"] for r in reps.values()) >= 6
    w.sp.reset(0)
    w.sp.reset(1)
    rc, n, _, _, _ = w.push(lanes)
    assert rc == nat.SSYM_OK and w.e.timings()["main_launches"] == 7          # ceil(150 / 23)
    w.events()                                                                # ordered by (lane, target, end) across slices
    w.close()


# ---- 7. watch() end to end ------------------------------------------------------------------------------------------------

def test_watch_polls_sounds_that_are_fed_block_by_block():
    rng = np.random.default_rng(0x0A7C)
    e = Engine(metric="dtw", dtype="f64")
    rate = 16000.0
    word = rng.standard_normal(1024 + 256 * 7)
    tgt = Sound.from_samples(word, rate, engine=e)
    recs = [np.concatenate([rng.standard_normal(5120), word, rng.standard_normal(9000)]), rng.standard_normal(12000)]
    sounds = [Sound.from_samples(r[:1500], rate, engine=e) for r in recs]
    with pytest.raises(ValueError):
        watch(sounds, [tgt], engine=e)                                         # not resident yet
    push_sounds(sounds, [r[1500:2000] for r in recs], e)
    wt = watch(sounds, [tgt], max_cost=1e-6, engine=e)
    got = wt.poll()
    for lo in range(2000, 16000, 4000):
        push_sounds(sounds, [r[lo:lo + 4000] for r in recs], e)
        got += wt.poll()
    got += wt.flush()
    assert len(got) == 1
    sound, target, sp = got[0]
    assert (sound, target, sp.source_index) == (0, 0, 0) and sp.cost <= 1e-6
    lo, hi = sp.sample_span(sounds[0].samples().size)
    assert abs(lo - 5120) <= 256 and sp.num_frames() >= tgt.num_frames() - 1
    best = wt.best()
    assert best[0][0].end_frame == sp.end_frame and best[1][0].cost > 1e-6
    wt.close()
    e.close()


# ---- 8. errors, device outputs --------------------------------------------------------------------------------------------

def test_every_listed_error_leaves_outputs_and_state_untouched():
    rng = np.random.default_rng(0xE77)
    dim = 5
    tgt = [_frames(rng, f, dim, "int") for f in (4, 6)]
    lane = _frames(rng, 80, dim, "int")
    w = _W(tgt, dim, squared=True)
    L, ctx, sp = nat.lib(), w.e.ctx, w.sp.ptr
    rc, *_ = w.push([lane[:30]])
    assert rc == nat.SSYM_OK
    inv = nat.SSYM_E_INVALID
    x, off = lane[30:40].reshape(-1).copy(), np.array([0, 10], dtype=np.uint64)
    n = ctypes.c_uint64(SENT32)

    def untouched(fn, want):
        out = w.call(fn, [10])
        assert out[0] == want and out[1] == SENT32 and (out[4][0] == SENTF).all() and (out[4][1] == SENT32).all()
        assert L.ssym_last_error(ctx) and w.sp.counts()[0] == 30

    untouched(lambda n, pd, ps, f: L.ssym_spotter_push(ctx, None, x.ctypes.data, off.ctypes.data, f, n, pd, ps), inv)
    untouched(lambda n, pd, ps, f: L.ssym_spotter_push(ctx, sp, x.ctypes.data, None, f, n, pd, ps), inv)
    untouched(lambda n, pd, ps, f: L.ssym_spotter_push(ctx, sp, None, off.ctypes.data, f, n, pd, ps), inv)
    down = np.array([10, 0], dtype=np.uint64)
    untouched(lambda n, pd, ps, f: L.ssym_spotter_push(ctx, sp, x.ctypes.data, down.ctypes.data, f, n, pd, ps), inv)
    untouched(lambda n, pd, ps, f: L.ssym_spotter_follow(ctx, sp, None, f, n, pd, ps), inv)
    huge = np.array([0, 2 ** 31], dtype=np.uint64)
    untouched(lambda n, pd, ps, f: L.ssym_spotter_push(ctx, sp, x.ctypes.data, huge.ctypes.data, f, n, pd, ps), nat.SSYM_E_UNSUPPORTED)
    assert b"2147483647" in L.ssym_last_error(ctx)
    assert L.ssym_spotter_push(ctx, sp, x.ctypes.data, off.ctypes.data, 0, None, None, None) == inv
    assert L.ssym_spotter_flush(ctx, sp, 1, ctypes.byref(n)) == inv and L.ssym_spotter_flush(ctx, sp, 0, None) == inv
    assert L.ssym_spotter_reset(ctx, sp, 1) == inv and n.value == SENT32
    other = Engine(metric="dtw", dtype="f64")
    assert L.ssym_spotter_push(other.ctx, sp, x.ctypes.data, off.ctypes.data, 0, ctypes.byref(n), None, None) == inv
    st = w.e.stream(2, 16000.0, ncoeffs=dim)
    st7 = w.e.stream(1, 16000.0, ncoeffs=7)
    for s in (st, st7):
        untouched(lambda n, pd, ps, f, s=s: L.ssym_spotter_follow(ctx, sp, s.ptr, f, n, pd, ps), inv)
    # create: lanes, NaN, NULLs, limits, contexts
    out = ctypes.c_void_p(7)
    nan = np.array([1.0, np.nan])
    assert L.ssym_spotter_create(ctx, w.q.ptr, 0, None, ctypes.byref(out)) == inv and out.value is None
    assert L.ssym_spotter_create(ctx, w.q.ptr, 1, nan.ctypes.data, ctypes.byref(out)) == inv
    assert L.ssym_spotter_create(ctx, None, 1, None, ctypes.byref(out)) == inv
    assert L.ssym_spotter_create(ctx, w.q.ptr, 1, None, None) == inv
    long_q = w.e.queries(np.zeros(4097), np.array([0, 4097], dtype=np.uint64), 1)
    wide_q = w.e.queries(np.zeros(65), np.array([0, 1], dtype=np.uint64), 65)
    for q in (long_q, wide_q):
        assert L.ssym_spotter_create(ctx, q.ptr, 1, None, ctypes.byref(out)) == nat.SSYM_E_UNSUPPORTED
    for kw in (dict(band=4), dict(metric="refcos")):
        e2 = Engine(dtype="f64", **kw)
        q2 = e2.queries(np.zeros(10), np.array([0, 2], dtype=np.uint64), 5)
        assert L.ssym_spotter_create(e2.ctx, q2.ptr, 1, None, ctypes.byref(out)) == nat.SSYM_E_UNSUPPORTED
        e2.close()
    # an empty query set is allowed: pushes only count
    none_q = w.e.queries(np.zeros(0), np.zeros(1, dtype=np.uint64), dim)
    empty = w.e.spotter(none_q, 2)
    assert empty.push(np.zeros((5, dim)), [0, 2, 5]) == 0 and empty.counts().tolist() == [2, 3] and empty.flush(1) == 0
    empty.close()
    # after all the refused calls: the rest of the lane gives the reference's result
    fresh = _W(tgt, dim, squared=True)
    _check_split(fresh, [lane], [[0, 30, 80]])
    rc, nev, pd, ps, _ = w.push([lane[30:]])
    d, s = watch_ref.whole_profile(lane, tgt[1], True)
    assert rc == nat.SSYM_OK and np.array_equal(_bits(pd[0][1]), _bits(d[30:])) and np.array_equal(ps[0][1], s[30:])
    assert np.array_equal(_bits(w.sp.best()[0]), _bits(fresh.sp.best()[0]))
    other.close()
    fresh.close()
    w.close()


def test_device_outputs():
    import torch
    rng = np.random.default_rng(0xDE7)
    tgt = [_frames(rng, f, 4, "int") for f in (3, 5)]
    lanes = [_frames(rng, 70, 4, "int"), _frames(rng, 10, 4, "int")]
    host, dev = _W(tgt, 4, 2, max_cost=9.0, squared=True), _W(tgt, 4, 2, max_cost=9.0, squared=True)
    a, b = host.push(lanes), dev.push(lanes, device=True)
    assert a[0] == b[0] == nat.SSYM_OK and a[1] == b[1] >= 1
    assert np.array_equal(_bits(a[4][0]), _bits(b[4][0])) and np.array_equal(a[4][1], b[4][1])
    n = a[1]
    words = [torch.full((n,), 7, dtype=torch.int32, device="cuda") for _ in range(4)]
    cost = torch.full((n,), SENTF, dtype=torch.float64, device="cuda")
    rc = nat.lib().ssym_spotter_events(dev.e.ctx, dev.sp.ptr, words[0].data_ptr(), words[1].data_ptr(), cost.data_ptr(),
                                       words[2].data_ptr(), words[3].data_ptr(), nat.OUT_DEVICE)
    assert rc == nat.SSYM_OK
    lane, t, c, s, e = host.sp.events()
    for got, want in zip(words, (lane, t, s, e)):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(_bits(cost.cpu().numpy()), _bits(c))
    bc = torch.full((4,), SENTF, dtype=torch.float64, device="cuda")
    be = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    assert nat.lib().ssym_spotter_best(dev.e.ctx, dev.sp.ptr, bc.data_ptr(), None, be.data_ptr(), nat.OUT_DEVICE) == nat.SSYM_OK
    assert np.array_equal(_bits(bc.cpu().numpy()), _bits(host.sp.best()[0].reshape(-1)))
    assert np.array_equal(be.cpu().numpy().view(np.uint32), host.sp.best()[2].reshape(-1))
    host.close()
    dev.close()
