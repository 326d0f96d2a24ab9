"""The mosaicker (ssym_mosaicker_*, DESIGN.md section 2 "Live mosaic") end to end on the GPU: every call's frames and state
against tests/live_mosaic_ref.py bit for bit, and the frames from reset to flush against Engine.dtw_mosaic on the same f64
context.  The restatement is held to tests/mosaic_ref.py on the CPU (tests/test_live_mosaic_ref.py)."""
import numpy as np
import pytest

import live_mosaic_ref as ref
import mosaic_ref
import mosaicker_gpu as mg
from paced_match_gpu import bits
from soundsym_amd import SsymError
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

INF = float("inf")


def _cuts(T, step):
    return list(range(0, T, step)) + [T]


def _feed(live, x, cuts, lane=0, empty_between=False):
    for a, b in zip(cuts[:-1], cuts[1:]):
        chunks = [x[:0]] * live.n_lanes
        chunks[lane] = x[a:b]
        live.push(chunks)
        if empty_between:
            assert live.push([x[:0]] * live.n_lanes) == {}


@pytest.fixture(scope="module")
def planted():
    recs, x, _ = mosaic_ref.planted_case(0.05)
    extra = mosaic_ref.planted_case(0.3, seed=0x51CE)[1]
    return recs, np.concatenate([x, extra, x[::-1]], axis=0)[:96]          # 93 frames


@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("penalty,gap", [(1.0, None), (4.0, 2.5), (0.0, None)])
def test_pushes_of_1_of_7_and_of_everything(planted, penalty, gap, squared):
    recs, x = planted
    T = x.shape[0]
    with mg.Dict(recs, 13, squared=squared) as D:
        runs = []
        for step, between in ((1, False), (7, True), (T, False)):
            live = mg.Live(D, 1, penalty, gap)
            _feed(live, x, _cuts(T, step), empty_between=between)      # after every push: the restatement's c(n), frame for frame
            if step == 1 and penalty:
                assert 0 < len(live.emitted[0]) <= T and live.lag() < 16
            live.flush()
            mg.same_as_offline(D, live.emitted[0], x, penalty, gap)
            runs.append(live.emitted[0])
            live.close()
        assert runs[0] == runs[1] == runs[2]


def test_slices_of_5_change_nothing(planted):
    recs, x = planted
    with mg.Dict(recs, 13) as D, mg.hooks(SSYM_MOSAICKER_SLICE=5):
        live = mg.Live(D, 1, 1.0)
        _feed(live, x, [0, 3, 40, 41, x.shape[0]])
        live.flush()
        mg.same_as_offline(D, live.emitted[0], x, 1.0)
        live.close()


@pytest.fixture(scope="module")
def laggard():
    """a target that resembles nothing, at a penalty that keeps pieces long: the restatement's lag passes 16 and then 32"""
    rng = np.random.default_rng(0x7A61)
    segs = [mosaic_ref._real(rng, (n, 3)) for n in (30, 25)]
    x = mosaic_ref._real(rng, (96, 3))
    lag = [n - 1 - c for n, c in enumerate(ref.commits(segs, x, 20.0), start=1)]
    assert max(lag[:40]) > 16 and max(lag) > 32 and lag[-1] < max(lag)
    return segs, x


def test_ring_of_16_wraps_and_grows_twice(laggard):
    segs, x = laggard
    with mg.Dict(segs, 3) as D, mg.hooks(SSYM_MOSAICKER_RING=16):
        live = mg.Live(D, 1, 20.0)
        assert live.mk.counts()[1] == 16
        caps = []
        for a, b in zip(_cuts(96, 4)[:-1], _cuts(96, 4)[1:]):
            live.push([x[a:b]])
            caps.append(live.mk.counts()[1])
            assert caps[-1] >= live.lag() + 1 or live.lag() == b
        assert caps[-1] >= 64 and set(caps) >= {16, 32, 64} and caps == sorted(caps)
        assert 0 < len(live.emitted[0]) < 96                                 # columns were committed through the wrapped ring
        live.flush()
        mg.same_as_offline(D, live.emitted[0], x, 20.0)
        live.close()


def test_scratch_cap_refuses_and_a_flush_then_works(laggard):
    segs, x = laggard
    G, dim = 55, 3
    col = G + 4 + 8 * dim
    budget = G * (1 + 8 * dim) + 16 + (56 * G + 24 + 128) + 20 * col           # room for a ring of 16 columns, not of 32
    with mg.Dict(segs, 3) as D, mg.hooks(SSYM_MOSAICKER_SCRATCH_BYTES=budget):
        mk = D.e.mosaicker(D.d, 1, 20.0)
        assert mk.counts()[1] == 16
        with pytest.raises(SsymError) as err:
            mk.push(x)
        assert err.value.code == nat.SSYM_E_UNSUPPORTED and "flush" in str(err.value)
        n = int(mk.counts()[0][0])
        assert 16 <= n < 96 and mk.counts()[1] == 16
        # the lane is as it was after the last slice: what those slices committed is in the log
        lane = ref.Lane(segs, 3, 20.0)
        want = lane.push(x[:n])
        mg.same_frames(mg.by_lane(mk).get(0, []), want)
        total, covered, committed = mk.best()
        assert (float(total[0]), int(covered[0]), int(committed[0])) == lane.best()
        assert mk.flush() == n - len(want)
        mg.same_as_offline(D, want + mg.by_lane(mk)[0], x[:n], 20.0)
        mk.close()
    with mg.Dict(segs, 3) as D, mg.hooks(SSYM_MOSAICKER_SCRATCH_BYTES=budget - 8 * col):
        with pytest.raises(SsymError) as err:
            D.e.mosaicker(D.d, 1, 20.0)
        assert err.value.code == nat.SSYM_E_UNSUPPORTED


def test_three_lanes_unequal_pushes_reset_and_flush():
    rng = np.random.default_rng(0x3A9E6)
    segs = [mosaic_ref._real(rng, (n, 5)) for n in (17, 0, 40, 9)]
    x = [mosaic_ref._real(rng, (n, 5)) for n in (70, 33, 51)]
    for t in x:                                                               # spans of the recordings, so that pieces form
        t[5:25] = segs[2][10:30]
    with mg.Dict(segs, 5) as D:
        live = mg.Live(D, 3, 1.0, 3.0)
        at = [0, 0, 0]
        while at[0] < 70 or at[2] < 51:                                        # lane 1 stays idle
            take = [int(rng.integers(0, 12)) * int(rng.integers(0, 2)), 0, int(rng.integers(0, 9))]
            live.push([t[a:a + k] for t, a, k in zip(x, at, take)])
            at = [min(a + k, t.shape[0]) for t, a, k in zip(x, at, take)]
        assert live.mk.counts()[0].tolist() == [70, 0, 51]
        before = [list(e) for e in live.emitted]
        state = [a.copy() for a in live.mk.best()]
        live.reset(2)                                                          # the others are untouched
        now = live.mk.best()
        assert all(a[:2].tobytes() == b[:2].tobytes() for a, b in zip(state, now)) and now[2][2] == 0
        live.push([x[0][:0], x[1], x[2][:20]])
        live.flush(0)
        mg.same_as_offline(D, live.emitted[0], x[0], 1.0, 3.0)
        assert live.emitted[0][:len(before[0])] == before[0]
        with pytest.raises(SsymError) as err:                                  # a flushed lane has ended
            live.mk.push(np.concatenate([x[0][:1], x[1][:0], x[2][:0]]), [0, 1, 1, 1])
        assert err.value.code == nat.SSYM_E_INVALID and "reset" in str(err.value)
        live.flush(1)
        live.flush(2)
        mg.same_as_offline(D, live.emitted[1], x[1], 1.0, 3.0)
        mg.same_as_offline(D, live.emitted[2], x[2][:20], 1.0, 3.0)
        live.reset(0)
        live.push([x[2], x[1][:0], x[2][:0]])
        live.flush(0)
        mg.same_as_offline(D, live.emitted[0], x[2], 1.0, 3.0)
        live.close()


def test_follow_is_push_of_the_streams_frames():
    rng = np.random.default_rng(0xF0111)
    waves = [rng.standard_normal(9000) * 0.3, np.sin(0.03 * np.arange(7000)) + 0.1 * rng.standard_normal(7000)]
    with mg.Dict([np.zeros((1, 12))], 12) as D0:                                # synthetic samples analysed on the GPU
        recs = [D0.e.mfcc(np.sin(0.05 * np.arange(6000)) + 0.05 * rng.standard_normal(6000), 44100.0, 12),
                D0.e.mfcc(waves[0][2000:6000], 44100.0, 12)]
    with mg.Dict(recs, 12) as D:
        e = D.e
        st = e.stream(2, 44100.0, 12)
        followed, pushed = e.mosaicker(D.d, 2, 1.0), mg.Live(D, 2, 1.0)
        have = [0, 0]
        for cut in ((0, 0), (3000, 500), (3000, 4000), (9000, 7000)):
            chunks = [w[h:c] for w, h, c in zip(waves, have, cut)]
            have = list(cut)
            st.push(np.concatenate(chunks), np.concatenate([[0], np.cumsum([c.size for c in chunks])]))
            consumed = followed.counts()[0]
            n = followed.follow(st)
            got = mg.by_lane(followed)
            want = pushed.push([st.read(l)[int(consumed[l]):] for l in range(2)])
            assert got == want and n == sum(len(v) for v in want.values())
            for a, b in zip(followed.best(), pushed.mk.best()):
                assert a.tobytes() == b.tobytes()
        assert followed.counts()[0].tolist() == st.counts()[1].tolist() and int(followed.counts()[0][0]) > 10
        followed.close()
        pushed.close()
        st.close()


def test_nan_target_frame_kills_the_lane_without_gaps(planted):
    recs, x = planted
    x = x[:40].copy()
    x[22, 3] = np.nan
    with mg.Dict(recs, 13) as D:
        live = mg.Live(D, 2, 1.0)
        _feed(live, x[:30], [0, 9, 18, 30])
        live.push([x[:0], x[:12]])                                            # the other lane is untouched by the dead one
        cap = live.mk.counts()[1]
        total, covered, committed = live.mk.best()
        assert total[0] == INF and covered[0] == 22 and committed[0] <= 22 and total[1] < INF
        _feed(live, x[30:], [0, 4, 10])                                        # counted, nothing else
        assert live.mk.counts()[1] == cap and live.mk.counts()[0].tolist() == [40, 12]
        assert live.mk.best()[1][0] == 22
        live.flush(0)
        assert len(live.emitted[0]) == 22
        mg.same_as_offline(D, live.emitted[0], x[:22], 1.0)
        assert mg.offline(D, x, 1.0)[1][0] == INF
        live.close()


def test_dead_lane_leaves_the_capacity_alone():
    rng = np.random.default_rng(0xDEAD)
    segs = [mosaic_ref._real(rng, (20, 2))]
    x = mosaic_ref._real(rng, (80, 2))
    x[3] = np.nan
    with mg.Dict(segs, 2) as D, mg.hooks(SSYM_MOSAICKER_RING=16):
        live = mg.Live(D, 1, 2.0)
        live.push([x[:8]])
        live.push([x[8:]])                                                     # 72 frames more than the ring has columns
        assert live.mk.counts()[1] == 16 and live.mk.counts()[0].tolist() == [80]
        live.flush()
        mg.same_as_offline(D, live.emitted[0], x[:3], 2.0)
        live.close()


def test_nan_target_frame_is_one_gap_frame_with_a_gap_cost(planted):
    recs, x = planted
    x = x[:40].copy()
    x[22, 3] = np.nan
    with mg.Dict(recs, 13) as D:
        live = mg.Live(D, 1, 1.0, 2.0)
        _feed(live, x, [0, 9, 18, 30, 40])
        live.flush()
        f = live.emitted[0][22]
        assert (f[1], f[2], f[3], f[4]) == (nat.COVER_GAP, nat.NO_MATCH, 2.0, 1) and live.mk.best()[1][0] == 40
        mg.same_as_offline(D, live.emitted[0], x, 1.0, 2.0)
        live.close()


def test_nan_dictionary_frame_is_never_chosen(planted):
    recs, x = planted
    recs = [r.copy() for r in recs]
    recs[1][9] = np.nan                                                        # inside the span the target copies
    with mg.Dict(recs, 13) as D:
        live = mg.Live(D, 1, 1.0)
        _feed(live, x, _cuts(x.shape[0], 11))
        live.flush()
        assert len(live.emitted[0]) == x.shape[0]
        assert all(not (f[1] == 1 and f[2] == 9) and np.isfinite(f[3]) for f in live.emitted[0])
        mg.same_as_offline(D, live.emitted[0], x, 1.0)
        live.close()


def test_target_of_one_frame_and_of_none(planted):
    recs, x = planted
    with mg.Dict(recs, 13) as D:
        live = mg.Live(D, 2, 1.0)
        live.push([x[:1], x[:0]])
        live.flush(0)
        assert len(live.emitted[0]) == 1 and live.emitted[0][0][4] == 1
        mg.same_as_offline(D, live.emitted[0], x[:1], 1.0)
        assert live.flush(1) == [] and live.mk.best()[0][1] == INF
        live.close()


def test_planted_pieces_come_out_a_frame_or_two_behind():
    recs, x, pieces = mosaic_ref.planted_case()
    with mg.Dict(recs, 13) as D:
        live = mg.Live(D, 1, 1.0)
        want = list(range(11)) + [10, 12, 12, 14, 14, 16, 16, 18, 18, 20, 20, 22] + list(range(23, 31))
        for n in range(1, x.shape[0] + 1):
            live.push([x[n - 1:n]])
            assert int(live.mk.best()[2][0]) == want[n - 1] + 1
        live.flush()
        got = mosaic_ref.pieces_of((np.array([3]),) + (None,) + ref.frames_to_arrays(live.emitted[0], x.shape[0])[1:], [0, x.shape[0]], 0)
        assert got == pieces
        live.close()


def test_timings_split_forward_and_commit(planted):
    recs, x = planted
    with mg.Dict(recs, 13) as D:
        mk = D.e.mosaicker(D.d, 1, 1.0)
        mk.push(x)
        t = D.e.timings()
        assert t["main_ms"] > 0 and t["reduce_ms"] > 0 and t["n_pairs"] == 123 * x.shape[0] and t["main_launches"] == 1
        mk.close()


def test_out_device_for_frames_and_best(planted):
    from paced_match_gpu import SENT32
    recs, x = planted
    with mg.Dict(recs, 13) as D:
        mk = D.e.mosaicker(D.d, 2, 1.0)
        n = mk.push(np.concatenate([x[:60], x[10:40]]), [0, 60, 90])
        assert n > 10
        host, dev = mk.frames(), mk.frames(on_device=True)
        for h, d in zip(host, dev):
            d = d.cpu().numpy()
            assert h.tobytes() == (d if h.dtype == np.float64 else d.view(np.uint32)).tobytes()
        for h, d in zip(mk.best(), mk.best(on_device=True)):
            d = d.cpu().numpy()
            assert h.tobytes() == (d if h.dtype == np.float64 else d.view(np.uint32)).tobytes()
        # every output is nullable
        lib, ctx = nat.lib(), D.e.ctx
        only = np.full(n + 1, SENT32, dtype=np.uint32)
        assert lib.ssym_mosaicker_frames(ctx, mk.ptr, None, only.ctypes.data, None, None, None, None, 0) == nat.SSYM_OK
        assert np.array_equal(only[:n], host[1]) and only[n] == SENT32
        assert lib.ssym_mosaicker_best(ctx, mk.ptr, None, None, None, 0) == nat.SSYM_OK
        assert nat.lib().ssym_mosaicker_counts(mk.ptr, None, None) == nat.SSYM_OK
        mk.close()


def test_a_dictionary_appended_to_is_refused_at_the_next_push(planted):
    recs, x = planted
    with mg.Dict(recs, 13) as D:
        mk = D.e.mosaicker(D.d, 1, 1.0)
        mk.push(x[:5])
        D.e.dictionary_append(D.d, *pack_segments(recs[:1], 13, np.float64))
        with pytest.raises(SsymError) as err:
            mk.push(x[5:9])
        assert err.value.code == nat.SSYM_E_INVALID and "appended" in str(err.value)
        assert mk.counts()[0].tolist() == [5]
        mk.close()
