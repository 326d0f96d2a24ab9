"""The coverer (ssym_coverer_*, DESIGN.md section 2 "Live cover") end to end on the GPU: every push's pieces and state against
tests/live_cover_ref.py bit for bit, and -- where noted -- against ssym_dtw_cover on the same context.  The restatement is
held to tests/cover_ref.py on the CPU (tests/test_live_cover_ref.py), so the consequences 1 - 6 shown there carry over."""
import ctypes

import numpy as np
import pytest

import cover_ref
import coverer_gpu as cg
import live_cover_cases as cases
from paced_match_gpu import SENT32, SENTF, bits
from soundsym_amd import Engine, SsymError
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

INF = float("inf")
LENS12 = [3, 1, 8, 2, 5, 4, 7, 1, 6, 8, 2, 3]             # 12 segments of 1 ... 8 frames


@pytest.fixture(scope="module")
def case400():
    return cases.random_case(0xB400, LENS12, 400)


def _feed(live, x, cuts):
    before_flush = 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        before_flush += sum(len(v) for v in live.push([x[a:b]]).values())
    return before_flush


@pytest.mark.parametrize("dtype,squared", [("f64", False), ("f64", True), ("f32", False), ("f32", True)])
@pytest.mark.parametrize("penalty", [0.0, 2.0])
def test_consequences_on_400_frames_in_pushes_of_5(case400, penalty, dtype, squared):
    segs, x = case400
    with cg.Dict(segs, 3, dtype, squared) as D:
        live = cg.Live(D, 1, penalty)
        cuts = cases.even_cuts(400, 5)
        committed = 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            committed += sum(len(v) for v in live.push([x[a:b]]).values())       # 1, 2: pieces and total are the restatement's
            if b in (5, 100, 255, 400):
                # 1 and 3 against ssym_dtw_cover of the prefix on this context: the total's bits, and what is committed is
                # how its cover starts
                pieces, total = cg.offline(D, x[:b], penalty)
                assert bits([live.cv.best()[0][0]]).tolist() == bits([total]).tolist()
                cg.same_pieces(live.emitted[0], pieces[:len(live.emitted[0])], "prefix of %d" % b)
        live.flush()                                                             # 4
        pieces, total = cg.offline(D, x, penalty)
        cg.same_pieces(live.emitted[0], pieces)
        assert len(pieces) > 40 and committed >= 0.9 * len(pieces)               # nearly all of it came before the flush
        assert live.cv.best()[1].tolist() == [400] and live.cv.best()[2].tolist() == [400]
        assert bits([cover_ref.resum(live.emitted[0], penalty)]).tolist() == bits([total]).tolist()
        # 5: a piece's cost is the paced alignment's for the cut
        some = live.emitted[0][::7]
        q = D.queries([x[a:e + 1] for _, a, e, _ in some])
        cost = D.e.dtw_align(D.d, q, np.array([p[0] for p in some], dtype=np.uint32), np.arange(len(some), dtype=np.uint32),
                             step="paced")[0]
        assert bits(cost).tolist() == bits([p[3] for p in some]).tolist()
        live.close()


def test_cuts_do_not_matter(case400):
    segs, x = case400
    rng = np.random.default_rng(0xC075)
    with cg.Dict(segs, 3) as D:
        runs = []
        for cuts in (cases.random_cuts(rng, 400, 3), cases.random_cuts(rng, 400, 40), [0, 400]):
            live = cg.Live(D, 1, 2.0)
            _feed(live, x, cuts)
            runs.append(list(live.emitted[0]))
            live.flush()
            live.close()
        assert runs[0] == runs[1] == runs[2] and len(runs[0]) > 40


def test_planted_case_in_pushes_of_16():
    segs, x, planted = cover_ref.planted_case(1e-3)
    with cg.Dict(segs, 13) as D:
        live = cg.Live(D, 1, 0.0)
        before = _feed(live, x, cases.even_cuts(x.shape[0], 16))
        live.flush()
        assert [p[:3] for p in live.emitted[0]] == planted and 0 < before < len(planted)
        cg.same_pieces(live.emitted[0], cg.offline(D, x, 0.0)[0])
        live.close()


def test_three_lanes_with_ragged_pushes():
    segs, x0 = cases.random_case(0xB401, LENS12, 150)
    x = [x0, cases.random_case(0xB402, LENS12, 90)[1], cases.random_case(0xB403, LENS12, 37)[1]]
    rng = np.random.default_rng(0x3A9E5)
    with cg.Dict(segs, 3) as D:
        live = cg.Live(D, 3, 2.0)
        at = [0, 0, 0]
        live.push([x[0][:0], x[1][:0], x[2][:0]])                                # a push without frames
        while any(a < t.shape[0] for a, t in zip(at, x)):
            take = [int(rng.integers(0, 12)) * int(rng.integers(0, 2)) for _ in x]        # often none for a lane
            live.push([t[a:a + k] for t, a, k in zip(x, at, take)])
            at = [min(a + k, t.shape[0]) for t, a, k in zip(x, at, take)]
        assert live.cv.counts()[0].tolist() == [150, 90, 37]
        for l in (2, 0, 1):
            live.flush(l)
        for l in range(3):
            cg.same_pieces(live.emitted[l], cg.offline(D, x[l], 2.0)[0], "lane %d" % l)
        live.close()


def test_follow_is_push_of_the_streams_frames():
    rng = np.random.default_rng(0xF0110)
    segs = [cases._real(rng, (n, 12)) * 4.0 for n in (1, 3, 6, 2, 9)]
    waves = [rng.standard_normal(9000) * 0.3, np.sin(0.03 * np.arange(7000)) + 0.1 * rng.standard_normal(7000)]
    with cg.Dict(segs, 12) as D:
        e = D.e
        st = e.stream(2, 44100.0, 12)
        followed, pushed = e.coverer(D.d, 2, 1.0), cg.Live(D, 2, 1.0)
        have = [0, 0]
        for cut in ((0, 0), (3000, 500), (3000, 4000), (9000, 7000)):
            chunks = [w[h:c] for w, h, c in zip(waves, have, cut)]
            have = list(cut)
            st.push(np.concatenate(chunks), np.concatenate([[0], np.cumsum([c.size for c in chunks])]))
            consumed = followed.counts()[0]
            n = followed.follow(st)
            got = cg.by_lane(followed)
            want = pushed.push([st.read(l)[int(consumed[l]):] for l in range(2)])
            assert got == want and n == sum(len(v) for v in want.values())
            for a, b in zip(followed.best(), pushed.cv.best()):
                assert a.tobytes() == b.tobytes()
        assert followed.counts()[0].tolist() == st.counts()[1].tolist() and min(followed.counts()[0]) > 20
        followed.flush(0)
        assert followed.follow(st) == 0                                          # an ended lane is skipped, the other has nothing new
        st.reset(1)
        with pytest.raises(SsymError) as err:                                    # the stream holds fewer frames than were consumed
            followed.follow(st)
        assert err.value.code == nat.SSYM_E_INVALID and "ssym_coverer_reset" in str(err.value)
        followed.reset(1)
        assert followed.follow(st) == 0 and followed.counts()[0][1] == 0
        for h in (followed, pushed, st):
            h.close()


def test_out_device_for_pieces_and_best(case400):
    segs, x = case400
    with cg.Dict(segs, 3) as D:
        cv = D.e.coverer(D.d, 2, 0.0)
        n = cv.push(np.concatenate([x[:120], x[200:260]]), [0, 120, 180])
        assert n > 10
        host, dev = cv.pieces(), cv.pieces(on_device=True)
        for h, d in zip(host, dev):
            d = d.cpu().numpy()
            assert h.tobytes() == (d if h.dtype == np.float64 else d.view(np.uint32)).tobytes()
        for h, d in zip(cv.best(), cv.best(on_device=True)):
            d = d.cpu().numpy()
            assert h.tobytes() == (d if h.dtype == np.float64 else d.view(np.uint32)).tobytes()
        # every output is nullable
        lib, ctx = nat.lib(), D.e.ctx
        only = np.full(n + 1, SENT32, dtype=np.uint32)
        assert lib.ssym_coverer_pieces(ctx, cv.ptr, None, None, only.ctypes.data, None, None, 0) == nat.SSYM_OK
        assert np.array_equal(only[:n], host[2]) and only[n] == SENT32
        assert lib.ssym_coverer_best(ctx, cv.ptr, None, None, None, 0) == nat.SSYM_OK
        cv.close()


def test_reset_reuse_and_an_ended_lane(case400):
    segs, x = case400
    with cg.Dict(segs, 3) as D:
        live = cg.Live(D, 2, 0.0)
        live.push([x[:60], x[100:130]])
        live.flush(0)
        assert live.flush(0) == []                                               # nothing is left
        before = (live.cv.counts(), [a.copy() for a in live.cv.best()])
        n = ctypes.c_uint64(77)
        off = np.array([0, 3, 3], dtype=np.uint64)
        rc = nat.lib().ssym_coverer_push(D.e.ctx, live.cv.ptr, x.ctypes.data, off.ctypes.data, 0, ctypes.byref(n))
        assert rc == nat.SSYM_E_INVALID and n.value == 77 and "ended" in cg.error(D.e)
        assert live.cv.counts()[0].tolist() == before[0][0].tolist()
        live.push([x[:0], x[130:150]])                                           # the other lane goes on; none for the ended one is fine
        live.reset(0)
        live.push([x[200:300], x[150:170]])                                      # the lane starts again at frame 0
        live.flush(0)
        cg.same_pieces(live.emitted[0], cg.offline(D, x[200:300], 0.0)[0])
        live.close()


def test_non_finite_frames(case400):
    segs, x = case400
    x = x[:120].copy()
    for bad in (float("nan"), INF):
        y = x.copy()
        y[47, 1] = bad
        with cg.Dict(segs, 3) as D:
            live = cg.Live(D, 2, 2.0)
            for a, b in zip(range(0, 120, 5), range(5, 125, 5)):
                live.push([y[a:b], x[a:b]])                                      # lane 1 is the clean recording
                if b > 47:
                    total, covered, committed = live.cv.best()
                    assert total[0] == INF and covered[0] == 47 and committed[0] <= 47 and np.isfinite(total[1])
            live.flush(0)
            live.flush(1)
            cg.same_pieces(live.emitted[0], cg.offline(D, y[:47], 2.0)[0])       # the flush gives the cover of the prefix
            cg.same_pieces(live.emitted[1], cg.offline(D, x, 2.0)[0])            # the other lane is untouched
            assert live.cv.best()[2].tolist() == [47, 120]
            live.close()
    poisoned = [a.copy() for a in segs]
    poisoned[2][3, 0] = float("nan")
    with cg.Dict(poisoned, 3) as D:
        live = cg.Live(D, 1, 0.0)
        _feed(live, x, cases.even_cuts(120, 5))
        live.flush()
        assert live.emitted[0] and all(p[0] != 2 for p in live.emitted[0])
        live.close()


# -- refusals -----------------------------------------------------------------------------------------------------------------

def _create(e, d_ptr, lanes=1, penalty=0.0):
    out = ctypes.c_void_p(0x5E7)
    rc = nat.lib().ssym_coverer_create(e.ctx, d_ptr, lanes, penalty, ctypes.byref(out))
    return rc, out.value


def test_creation_refusals(case400):
    segs, _ = case400
    lib = nat.lib()
    with cg.Dict(segs, 3) as D:
        for bad in (-1.0, float("nan"), INF):
            assert _create(D.e, D.d.ptr, 1, bad) == (nat.SSYM_E_INVALID, None)
        assert "piece_penalty must be finite and not negative" in cg.error(D.e)
        assert _create(D.e, None) == (nat.SSYM_E_INVALID, None)
        assert _create(D.e, D.d.ptr, 0) == (nat.SSYM_E_INVALID, None)
        assert lib.ssym_coverer_create(D.e.ctx, D.d.ptr, 1, 0.0, None) == nat.SSYM_E_INVALID
        assert lib.ssym_coverer_create(None, D.d.ptr, 1, 0.0, None) == nat.SSYM_E_INVALID
        assert _create(D.e, D.d.ptr, 65536) == (nat.SSYM_E_UNSUPPORTED, None)
        empty = D.e.dictionary(*pack_segments([], 3, np.float64), 3)
        assert _create(D.e, empty.ptr) == (nat.SSYM_E_EMPTY_DICT, None)
    rng = np.random.default_rng(7)
    for kw, src, dim in ((dict(metric="refcos"), segs, 3), (dict(band=4), segs, 3),
                         (dict(), [cases._real(rng, (129, 3))], 3), (dict(), [cases._real(rng, (4, 65))], 65)):
        with cg.Dict(src, dim, **kw) as D:
            assert _create(D.e, D.d.ptr) == (nat.SSYM_E_UNSUPPORTED, None), kw
            with pytest.raises(SsymError) as err:
                D.e.coverer(D.d)
            assert err.value.code == nat.SSYM_E_UNSUPPORTED
    # lanes x 2 Fmax x 2 Fmax x 12 bytes beyond the scratch: 683 lanes at Fmax = 128
    with cg.Dict([cases._real(rng, (128, 3))], 3) as D:
        assert _create(D.e, D.d.ptr, 683) == (nat.SSYM_E_UNSUPPORTED, None) and "fewer lanes" in cg.error(D.e)
        rc, ptr = _create(D.e, D.d.ptr, 2)
        assert rc == nat.SSYM_OK and lib.ssym_coverer_destroy(D.e.ctx, ptr) == nat.SSYM_OK


def test_call_refusals_leave_outputs_and_coverer_as_they_were(case400):
    segs, x = case400
    lib = nat.lib()
    with cg.Dict(segs, 3) as D, cg.Dict(segs, 3) as other:
        live = cg.Live(D, 2, 2.0)
        live.push([x[:50], x[50:80]])
        ctx, cv = D.e.ctx, live.cv.ptr
        state = lambda: (live.cv.counts(), [a.tobytes() for a in live.cv.best()], [a.tobytes() for a in live.cv.pieces()])
        before = state()
        n = ctypes.c_uint64(77)
        good = np.array([0, 2, 4], dtype=np.uint64)
        u = np.full(64, SENT32, dtype=np.uint32)
        f = np.full(64, SENTF)
        st3, st_dim = D.e.stream(3, 44100.0, 3), D.e.stream(2, 44100.0, 12)
        refused = [
            lib.ssym_coverer_push(ctx, None, x.ctypes.data, good.ctypes.data, 0, ctypes.byref(n)),
            lib.ssym_coverer_push(ctx, cv, x.ctypes.data, None, 0, ctypes.byref(n)),
            lib.ssym_coverer_push(ctx, cv, x.ctypes.data, good.ctypes.data, 0, None),
            lib.ssym_coverer_push(ctx, cv, None, good.ctypes.data, 0, ctypes.byref(n)),
            lib.ssym_coverer_push(ctx, cv, x.ctypes.data, np.array([0, 4, 2], dtype=np.uint64).ctypes.data, 0, ctypes.byref(n)),
            lib.ssym_coverer_push(other.e.ctx, cv, x.ctypes.data, good.ctypes.data, 0, ctypes.byref(n)),
            lib.ssym_coverer_push(None, cv, x.ctypes.data, good.ctypes.data, 0, ctypes.byref(n)),
            lib.ssym_coverer_follow(ctx, cv, None, 0, ctypes.byref(n)),
            lib.ssym_coverer_follow(ctx, cv, st3.ptr, 0, ctypes.byref(n)),
            lib.ssym_coverer_follow(ctx, cv, st_dim.ptr, 0, ctypes.byref(n)),
            lib.ssym_coverer_follow(other.e.ctx, cv, st3.ptr, 0, ctypes.byref(n)),
            lib.ssym_coverer_flush(ctx, cv, 2, ctypes.byref(n)),
            lib.ssym_coverer_flush(ctx, cv, 0, None),
            lib.ssym_coverer_flush(ctx, None, 0, ctypes.byref(n)),
            lib.ssym_coverer_flush(other.e.ctx, cv, 0, ctypes.byref(n)),
            lib.ssym_coverer_reset(ctx, cv, 2),
            lib.ssym_coverer_reset(ctx, None, 0),
            lib.ssym_coverer_reset(other.e.ctx, cv, 0),
            lib.ssym_coverer_pieces(ctx, None, u.ctypes.data, u.ctypes.data, u.ctypes.data, u.ctypes.data, f.ctypes.data, 0),
            lib.ssym_coverer_pieces(other.e.ctx, cv, u.ctypes.data, u.ctypes.data, u.ctypes.data, u.ctypes.data, f.ctypes.data, 0),
            lib.ssym_coverer_best(ctx, None, f.ctypes.data, u.ctypes.data, u.ctypes.data, 0),
            lib.ssym_coverer_best(other.e.ctx, cv, f.ctypes.data, u.ctypes.data, u.ctypes.data, 0),
            lib.ssym_coverer_counts(None, u.ctypes.data, None),
            lib.ssym_coverer_destroy(other.e.ctx, cv),
        ]
        assert refused == [nat.SSYM_E_INVALID] * len(refused), refused
        assert n.value == 77 and (u == SENT32).all() and (f == SENTF).all()
        assert lib.ssym_coverer_destroy(ctx, None) == nat.SSYM_OK
        assert lib.ssym_coverer_counts(cv, None, None) == nat.SSYM_OK
        assert str(state()) == str(before)
        live.push([x[50:90], x[80:85]])                                          # and it goes on as if nothing had been asked
        # a dictionary appended to since: the next push is refused
        D.e.dictionary_append(D.d, *pack_segments([x[:4]], 3, np.float64))
        rc = lib.ssym_coverer_push(ctx, cv, x.ctypes.data, good.ctypes.data, 0, ctypes.byref(n))
        assert rc == nat.SSYM_E_INVALID and n.value == 77 and "appended" in cg.error(D.e)
        for h in (st3, st_dim, live):
            h.close()


def test_python_checks_before_the_library(case400):
    segs, x = case400
    with cg.Dict(segs, 3) as D:
        cv = D.e.coverer(D.d, 2)
        for call in (lambda: cv.push(x[:4]), lambda: cv.push(x[:4], [0, 4]), lambda: cv.push(x[:4], [0, 3, 2]),
                     lambda: cv.push(x[:4], [0, 2, 5]), lambda: cv.push(np.zeros(7), [0, 1, 2]), lambda: cv.flush(2),
                     lambda: cv.reset(-1), lambda: D.e.coverer(D.d, 0), lambda: D.e.coverer(D.d, 1, -1.0)):
            with pytest.raises(ValueError):
                call()
        assert cv.counts()[0].tolist() == [0, 0] and cv.counts()[1] == 1024
        assert cv.d is D.d                                                       # the coverer keeps its dictionary alive
        cv.close()
        cv.close()


# -- cover_live end to end ----------------------------------------------------------------------------------------------------

def test_cover_live_polls_sounds_that_are_fed_block_by_block():
    from soundsym_amd import Cover, Sound, SoundDictionary, push_sounds
    rng = np.random.default_rng(0x11FE)
    e = Engine(metric="dtw", dtype="f64")
    rate = 16000.0
    words = [rng.standard_normal(1024 + 256 * k) * (0.2 + 0.1 * k) for k in (0, 2, 5, 9)]
    d = SoundDictionary(engine=e)
    d.sounds = [Sound.from_samples(w, rate, engine=e) for w in words]
    # about 260 and 190 frames against W = 20: long enough for commits before the flush
    recs = [np.concatenate([x for _ in range(6) for x in (words[2], words[0], rng.standard_normal(3000) * 0.3, words[3], words[1])]),
            rng.standard_normal(50000) * 0.25]
    sounds = [Sound.from_samples(r[:1500], rate, engine=e) for r in recs]
    with pytest.raises(ValueError, match="share one stream"):
        d.cover_live(sounds)                                                     # not resident yet
    push_sounds(sounds, [r[1500:2000] for r in recs], e)
    live = d.cover_live(sounds, 1.0)
    got = live.poll()
    for lo in range(2000, 68000, 9000):
        push_sounds(sounds, [r[lo:lo + 9000] for r in recs], e)
        new = live.poll()
        assert [(s, p.start_frame) for s, p in new] == sorted((s, p.start_frame) for s, p in new)
        got += new
    consumed, covered, committed, total = live.pending()
    assert consumed.tolist() == [s.num_frames() for s in sounds] == covered.tolist() and (committed < consumed).all()
    before = len(got)
    got += live.flush()
    want = d.cover(sounds, 1.0)                                                  # the offline cover of the finished sounds
    assert 0 < before < len(got) == sum(len(c) for c in want)
    for k, (mine, c) in enumerate(zip(live.covers(), want)):
        assert isinstance(mine, Cover) and mine.num_frames == c.num_frames and len(mine) == len(c) > 0
        assert [(p.source_index, p.start_frame, p.end_frame) for p in mine.pieces] == \
               [(p.source_index, p.start_frame, p.end_frame) for p in c.pieces]
        assert np.array([p.cost for p in mine.pieces] + [mine.total]).tobytes() == \
               np.array([p.cost for p in c.pieces] + [c.total]).tobytes()
        assert [p for s, p in got if s == k] == mine.pieces
        assert total[k] == c.total
    assert live.pending()[2].tolist() == consumed.tolist()
    live.close()
    e.close()
