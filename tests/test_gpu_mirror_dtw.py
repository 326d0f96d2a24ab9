"""include/soundsym.hpp's DTW-family methods, run by tests/cpp/test_mirror_dtw.cpp ONCE on the case set of
tests/mirror_cases.py, against the Python mirror (soundsym_amd/api.py) on the same sounds, call for call and bit for bit:
both mirrors put the same arrays into the same entry points of the same library, so every index expression of the header's
marshalling either gives the Python mirror's result or is wrong.  One call of each kind is also held to its restatement
(dtw_path_ref, paced_ref, spot_all_ref, span_ref / warp_ref, watch_ref), bit for bit as the GPU test of that call holds it, so
that a reading of an output layout both mirrors share does not pass.  Refusals are compared by code: what Python raises for
the same mistake (ValueError: SSYM_E_INVALID; SsymError: its code) is the model."""
import os
import subprocess
import time

import numpy as np
import pytest

import dtw_path_ref
import mirror_cases as mc
import paced_ref
import span_ref
import spot_all_ref
from soundsym_amd import Engine, Sound, SoundDictionary, Spot
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "cpp", "test_mirror_dtw")
NO = nat.NO_MATCH
NCOEFFS = mc.NCOEFFS
STEPS = (("sym", "symmetric"), ("paced", "paced"))


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).reshape(-1).view(np.uint64)


class _Child:
    """The one run of the program: return code, output, wall time and the parsed result file (None when it wrote none)."""

    def __init__(self, cases, folder):
        case_file, result_file = os.path.join(folder, "cases.bin"), os.path.join(folder, "results.bin")
        mc.write_arrays(case_file, cases.arrays())
        if not os.path.exists(EXE):
            subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp")])
        t0 = time.perf_counter()
        r = subprocess.run([EXE, case_file, result_file], capture_output=True, text=True, timeout=300)
        self.seconds = time.perf_counter() - t0
        self.returncode, self.output = r.returncode, r.stdout + r.stderr
        self.results = mc.read_arrays(result_file) if os.path.exists(result_file) else None
        print("test_mirror_dtw: %.2f s, exit %d, %d arrays" % (self.seconds, self.returncode, len(self.results or ())))


class _World:
    """The Python mirror on the same sounds: an f64 dtw engine without a band, the segment dictionary S and the recording
    dictionary R."""

    def __init__(self, cases):
        self.cases = cases
        self.e = Engine(metric="dtw", dtype="f64")
        snd = lambda pair: Sound(pair[0], mc.RATE, pair[1].reshape(-1))
        self.recs, self.tgts, self.segs, self.repl = ([snd(p) for p in x] for x in (cases.recs, cases.tgts, cases.segs, cases.repl))
        self.S, self.R = self.dictionary(self.segs), self.dictionary(self.recs)
        self.args = cases.args
        self.S.warp(self.tgts[:1], indices=[0])       # the device-resident maps go through torch: its start-up belongs here

    def dictionary(self, sounds, engine=None):
        d = SoundDictionary(engine=engine or self.e)
        d.sounds = list(sounds)
        return d

    def queries(self, tgts, engine=None):
        flat, off = pack_segments([t.mfccs() for t in tgts], NCOEFFS, np.float64)
        return (engine or self.e).queries(flat, off, NCOEFFS)

    def close(self):
        self.e.close()


@pytest.fixture(scope="module")
def cases():
    return mc.build()


@pytest.fixture(scope="module")
def child(cases, tmp_path_factory):
    return _Child(cases, str(tmp_path_factory.mktemp("mirror_dtw")))


@pytest.fixture
def res(child):
    """The program's results; every test fails here, from the saved record, when the one run ended abnormally."""
    assert child.returncode == 0 and child.results is not None, "exit %r\n%s" % (child.returncode, child.output)
    return child.results


@pytest.fixture(scope="module")
def world(cases, child):
    # (after the child: a run that ended in a signal leaves the GPU alone for the rest of the module)
    assert child.returncode in (0, 1), "exit %r\n%s" % (child.returncode, child.output)
    w = _World(cases)
    yield w
    w.close()


# ---- comparisons ---------------------------------------------------------------------------------------------------
def _same_f64(got, want, what):
    assert got.dtype == np.float64 and got.size == np.size(want), (what, got.size, np.size(want))
    assert np.array_equal(_bits(got), _bits(want)), (what, got, want)


def _same_ints(got, want, dtype, what):
    want = np.asarray(want).reshape(-1)
    assert got.dtype == dtype and got.size == want.size and np.array_equal(got.astype(np.uint64), want.astype(np.uint64)), (what, got, want)


def _ok(res, name):
    assert res[name + ".code"][0] == 0.0, (name, res[name + ".code"][0])


def _alignments(res, p):
    """[(cost, source index, path [L, 2], map)] as the program laid them out."""
    cost, src, poff, moff = res[p + ".cost"], res[p + ".src"], res[p + ".path_off"], res[p + ".map_off"]
    assert cost.dtype == np.float64 and src.dtype == np.uint32 and poff.dtype == np.uint64 and moff.dtype == np.uint64
    assert poff.size == cost.size + 1 == moff.size == src.size + 1 and res[p + ".path"].size == 2 * int(poff[-1])
    path, fmap = res[p + ".path"].reshape(-1, 2), res[p + ".map"]
    assert fmap.size == int(moff[-1])
    return [(cost[t], int(src[t]), path[int(poff[t]):int(poff[t + 1])], fmap[int(moff[t]):int(moff[t + 1])])
            for t in range(cost.size)]


def _same_alignments(res, p, want):
    got = _alignments(res, p)
    assert len(got) == len(want), p
    for t, ((cost, src, path, fmap), w) in enumerate(zip(got, want)):
        assert _bits(cost)[0] == _bits(w.cost)[0] and src == w.source_index, (p, t, cost, w.cost, src, w.source_index)
        assert np.array_equal(path, w.path) and np.array_equal(fmap, w.frame_map), (p, t)
        assert (fmap.size == 0) == (path.shape[0] == 0), (p, t)


def _spots(res, p):
    cost, src, start, end = (res[p + x] for x in (".cost", ".src", ".start", ".end"))
    assert cost.dtype == np.float64 and all(x.dtype == np.uint32 for x in (src, start, end))
    assert cost.size == src.size == start.size == end.size
    return [(int(src[k]), int(start[k]), int(end[k]), cost[k]) for k in range(cost.size)]


def _same_spots(res, p, want):
    got = _spots(res, p)
    assert len(got) == len(want), (p, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[:3] == (w.source_index, w.start_frame, w.end_frame) and _bits(g[3])[0] == _bits(w.cost)[0], (p, k, g, w)


def _same_spot_lists(res, p, want):
    off = res[p + ".off"]
    assert off.dtype == np.uint64 and off.size == len(want) + 1 and np.array_equal(off, np.concatenate([[0], np.cumsum([len(x) for x in want])])), (p, off)
    _same_spots(res, p, [sp for x in want for sp in x])


def _same_sound_lists(res, p, want, d):
    off, idx = res[p + ".off"], res[p + ".idx"]
    flat = [next(i for i, s in enumerate(d.sounds) if s is x) for row in want for x in row]
    _same_ints(off, np.concatenate([[0], np.cumsum([len(x) for x in want])]), np.uint64, p)
    _same_ints(idx, flat, np.uint32, p)


def _same_events(res, p, events):
    lane, tgt, cost, start, end = events
    _same_ints(res[p + ".lane"], lane, np.uint32, p)
    _same_ints(res[p + ".target"], tgt, np.uint32, p)
    _same_ints(res[p + ".src"], lane, np.uint32, p)                         # Spot.source_index is the lane
    _same_ints(res[p + ".start"], start, np.uint32, p)
    _same_ints(res[p + ".end"], end, np.uint32, p)
    _same_f64(res[p + ".cost"], cost, p)


def _same_best(res, p, best):
    """[lane * n_targets + target], the lane as source_index, three SSYM_NO_MATCH where there is none."""
    cost, start, end = best
    lanes, targets = cost.shape
    src = np.where(end == NO, NO, np.repeat(np.arange(lanes), targets).reshape(lanes, targets))
    _same_ints(res[p + ".src"], src, np.uint32, p)
    _same_ints(res[p + ".start"], np.where(end == NO, NO, start), np.uint32, p)
    _same_ints(res[p + ".end"], end, np.uint32, p)
    _same_f64(res[p + ".cost"], cost, p)


def _try(call):
    """(code, result): Python's answer to a call as the code the C++ mirror would throw."""
    try:
        return 0, call()
    except nat.SsymError as err:
        return err.code, None
    except ValueError:
        return nat.SSYM_E_INVALID, None


def _same_code(res, name, code):
    assert int(res[name + ".code"][0]) == code, (name, res[name + ".code"][0], code)


# ---- a ... d: the match family -------------------------------------------------------------------------------------
def test_a_match_indices_step(res, world):
    S, tgts, dist = world.S, world.tgts, world.args["distances"]
    for name in ("a.paced", "a.paced.costs", "a.paced.dist", "a.paced.dist.costs", "a.sym"):
        _ok(res, name)
    idx, cost = S.match_indices(tgts, step="paced")
    _same_ints(res["a.paced.idx"], idx, np.uint32, "a.paced")
    _same_ints(res["a.paced.costs.idx"], idx, np.uint32, "a.paced.costs")
    _same_f64(res["a.paced.costs.cost"], cost, "a.paced.costs")
    assert idx[5] == 0 and cost[5] == np.inf                                # the frameless target: 0 and +inf
    assert mc.SEG_FRAMES[idx[3]] in (17, 33) and np.isfinite(cost[3]) and cost[1] == np.inf and idx[1] == 0
    idx, cost = S.match_indices(tgts, dist, step="paced")
    _same_ints(res["a.paced.dist.idx"], idx, np.uint32, "a.paced.dist")
    _same_ints(res["a.paced.dist.costs.idx"], idx, np.uint32, "a.paced.dist.costs")
    _same_f64(res["a.paced.dist.costs.cost"], cost, "a.paced.dist.costs")
    # SSYM_STEP_SYMMETRIC is match_indices
    idx, _ = S.match_indices(tgts, dist)
    _same_ints(res["a.sym.idx"], idx, np.uint32, "a.sym")
    _same_ints(res["a.sym.match_indices"], idx, np.uint32, "a.sym")
    q = world.queries(tgts)
    _same_f64(res["a.sym.cost"], world.e.match(S.resident(), q, dist)[1], "a.sym")
    q.close()


def test_b_pair_matrix_step(res, world):
    q = world.queries(world.tgts[1:])
    for name, step in STEPS:
        _ok(res, "b." + name)
        want = world.e.pair_matrix(world.S.resident(), q, exact=True, step=step)
        assert want.shape == (6, 5)
        _same_f64(res["b.%s.out" % name], want, name)                       # row-major [sounds][targets]
        if step == "paced":
            fits = np.array([[paced_ref.span_bounds(t)[0] <= f <= paced_ref.span_bounds(t)[1] and f > 0 and t > 0
                              for t in mc.TGT_FRAMES[1:]] for f in mc.SEG_FRAMES])
            assert np.array_equal(np.isfinite(res["b.paced.out"]).reshape(6, 5), fits)
    q.close()


def test_c_candidates(res, world):
    S, tgts, dist = world.S, world.tgts, world.args["distances"]
    for k in (1, 3, 9):
        _ok(res, "c.k%d" % k)
        want = S.candidates(tgts, k, dist)
        _same_sound_lists(res, "c.k%d" % k, want, S)
        assert all(len(row) <= min(k, 6) for row in want)
    assert max(np.diff(res["c.k9.off"].astype(np.int64))) <= 6 and NO not in res["c.k9.idx"]      # SSYM_NO_MATCH entries dropped
    _ok(res, "c.plain")
    _same_sound_lists(res, "c.plain", S.candidates(tgts, 3), S)


def test_d_chain_indices(res, world):
    _ok(res, "d.chain")
    idx, _ = world.e.chain(world.S.resident(), world.tgts[3].mfccs(), world.args["chain.distances"])
    assert idx.size == 5
    _same_ints(res["d.chain.idx"], idx, np.uint32, "d.chain")


# ---- e, f: align and warp ------------------------------------------------------------------------------------------
def test_e_align(res, world, cases):
    for which, indices in mc.INDICES.items():
        for name, step in STEPS:
            p = "e.%s.%s" % (name, which)
            _ok(res, p)
            want = world.S.align(world.tgts, indices=indices, step=step)
            _same_alignments(res, p, want)
            got = _alignments(res, p)
            assert [g[1] for g in got] == list(indices)                     # source_index echoed
            for g in got:
                if g[2].shape[0]:
                    assert tuple(g[2][0]) == (0, 0) and (np.diff(g[2].astype(np.int64), axis=0) >= 0).all()     # forward order
            assert any(g[2].shape[0] == 0 for g in got) and any(g[2].shape[0] > 0 for g in got)
    # ... and the symmetric call against its restatement, bit for bit (tests/test_gpu_align.py)
    for which, indices in mc.INDICES.items():
        for t, (g, s) in enumerate(zip(_alignments(res, "e.sym." + which), indices)):
            cost, path, fmap = dtw_path_ref.align(cases.segs[s][1], cases.tgts[t][1])
            assert _bits(g[0])[0] == _bits(cost)[0], (which, t, g[0], cost)
            assert np.array_equal(g[2].astype(np.int64), path) and np.array_equal(g[3].astype(np.int64), fmap), (which, t)


def test_f_warp(res, world):
    total = sum(t.samples().size for t in world.tgts)
    for which, indices in mc.INDICES.items():
        outs = {}
        for search in (0, 7, 512):
            p = "f.s%d.%s" % (search, which)
            _ok(res, p)
            want = world.S.warp(world.tgts, indices=indices, search=search)
            assert want.size == total
            _same_f64(res[p + ".out"], want, p)
            outs[search] = res[p + ".out"]
        assert not np.array_equal(_bits(outs[0]), _bits(outs[7])) and not np.array_equal(_bits(outs[7]), _bits(outs[512]))
    # a pair without a finite cost takes the length fit: target 2 on the frameless segment ("a") gets its 500 samples
    at = sum(t.samples().size for t in world.tgts[:2])
    seg = world.segs[5].samples()
    assert np.array_equal(_bits(res["f.s0.a.out"][at:at + seg.size]), _bits(seg)) and not res["f.s0.a.out"][at + seg.size:at + 8 * mc.HOP].any()


# ---- g, h: spot and spot_all ---------------------------------------------------------------------------------------
def test_g_spot(res, world, cases):
    si = world.args["spot.indices"]
    for name, step in STEPS:
        _ok(res, "g." + name)
        _ok(res, "g.%s.idx" % name)
        _same_spots(res, "g." + name, world.R.spot(world.tgts, step=step))
        _same_spots(res, "g.%s.idx" % name, world.R.spot(world.tgts, indices=si, step=step))
        assert _spots(res, "g." + name)[5] == (NO, NO, NO, np.inf)          # no frames: three SSYM_NO_MATCH, the library's cost
    assert _spots(res, "g.paced.idx")[3] == (NO, NO, NO, np.inf) and _spots(res, "g.sym.idx")[3][:3] == (2, 0, 0)
    # ... and the paced search against its restatement, bit for bit (tests/test_gpu_paced.py)
    feats = [f for _, f in cases.recs]
    for t, g in enumerate(_spots(res, "g.paced")):
        best = paced_ref.spot_best(feats, cases.tgts[t][1])
        assert g[:3] == (best[0], best[2], best[3]) and _bits(g[3])[0] == _bits(best[1])[0], (t, g, best)


def _merged_ref(cases, t, k, limit=None):
    out = []
    for r, (_, f) in enumerate(cases.recs):
        count, cost, start, end = spot_all_ref.spot_all(f, cases.tgts[t][1], k, limit)
        out += [(float(cost[m]), r, int(end[m]), int(start[m])) for m in range(count)]
    return sorted(out)


def test_h_spot_all(res, world, cases):
    R, tgts, si = world.R, world.tgts, world.args["spot.indices"]
    limit = float(world.args["spot_all.max_cost"][0])
    for k in (1, 8, 64):
        _ok(res, "h.sym.k%d" % k)
        _same_spot_lists(res, "h.sym.k%d" % k, R.spot_all(tgts, max_spots=k))
    for p, kw in (("h.paced.k8", dict(step="paced")), ("h.sym.idx", dict(indices=si)), ("h.paced.idx", dict(indices=si, step="paced")),
                  ("h.sym.max_cost", dict(max_cost=limit)), ("h.sym.idx.max_cost", dict(indices=si, max_cost=limit))):
        _ok(res, p)
        _same_spot_lists(res, p, R.spot_all(tgts, max_spots=8, **kw))
    lengths = lambda p: np.diff(res[p + ".off"].astype(np.int64)).tolist()
    free, cut = lengths("h.sym.k8"), lengths("h.sym.max_cost")
    assert cut[1] == 0 and 0 < cut[2] < free[2] and cut[3] == 1 < free[3]   # a list emptied, lists cut short
    assert max(lengths("h.sym.k64")) > 64                                   # max_spots applies per recording
    # the two identical recordings tie on cost: (cost, source index, end frame)
    off = int(res["h.sym.k8.off"][2])
    head = [(s[3], s[0], s[2]) for s in _spots(res, "h.sym.k8")[off:off + 4]]
    assert head == [(0.0, 3, 12), (0.0, 3, 32), (0.0, 4, 12), (0.0, 4, 32)]
    # ... and the whole merged lists against the restatement, bit for bit (tests/test_gpu_spot_all.py)
    for p, lim in (("h.sym.k8", None), ("h.sym.max_cost", limit)):
        offs, flat = res[p + ".off"], _spots(res, p)
        for t in range(6):
            want = _merged_ref(cases, t, 8, lim)
            got = flat[int(offs[t]):int(offs[t + 1])]
            assert len(got) == len(want), (p, t)
            for g, w in zip(got, want):
                assert (g[0], g[2], g[1]) == (w[1], w[2], w[3]) and _bits(g[3])[0] == _bits(w[0])[0], (p, t, g, w)


# ---- i: the span calls ---------------------------------------------------------------------------------------------
def _heads(lists):
    return [x[0] if x else Spot.none() for x in lists]


def _hand():
    return [Spot.none() if r == NO else Spot(r, a, b, 0.0) for r, a, b in mc.HAND]


def test_i_align_spans_and_warp_spans(res, world, cases):
    R, tgts = world.R, world.tgts
    off = np.concatenate([[0], np.cumsum([t.samples().size for t in tgts])])
    for name, step in STEPS:
        sets = (("spot", R.spot(tgts, step=step)), ("spot.idx", R.spot(tgts, indices=world.args["spot.indices"], step=step)),
                ("heads", _heads(R.spot_all(tgts, max_spots=8, step=step))), ("hand", _hand()))
        for which, spots in sets:
            p = "i.%s.%s" % (name, which)
            _ok(res, p)
            _same_alignments(res, p + ".align", R.align(tgts, spans=spots, step=step))
            for search in (0, 64):
                want = R.warp(tgts, spans=spots, search=search, step=step)
                assert want.size == off[-1]
                _same_f64(res["%s.warp.s%d" % (p, search)], want, (p, search))
            # an empty Spot: an empty Alignment, zeros in the output
            for t, sp in enumerate(spots):
                if not sp:
                    g = _alignments(res, p + ".align")[t]
                    assert g[1] == NO and g[0] == np.inf and g[2].shape[0] == 0 and g[3].size == 0
                    assert not res[p + ".warp.s0"][off[t]:off[t + 1]].any() and not res[p + ".warp.s64"][off[t]:off[t + 1]].any()
            assert sum(not sp for sp in spots) >= 1
    hand = _alignments(res, "i.sym.hand.align")
    assert hand[3][1] == NO and off[4] - off[3] == 33 * mc.HOP              # the empty Spot by hand has samples to zero
    assert [int(g[2][-1][0]) for g in hand[:3]] == [0, 19, 9]               # the spans that end on a last frame: last - first
    # ... and warp_spans against its restatement, bit for bit (tests/test_gpu_span_warp.py): span_ref's alignment of every
    # span, then span_ref's window warp over Spot.sample_span's samples
    maps, m_off, frames, pair_len, idx, first, length = [], [0], [], [], [], [], []
    for t, (r, a, b) in enumerate(mc.HAND):
        _, path, fmap = span_ref.NO_PATH if r == NO else span_ref.align_one(cases.recs[r][1], cases.tgts[t][1], a, b)
        maps += [int(v) for v in fmap]
        m_off.append(len(maps))
        frames.append(len(fmap))
        pair_len.append(len(path))
        w = (0, 0) if r == NO else span_ref.sample_window(a, b, cases.recs[r][0].size)
        idx.append(0 if r == NO else r)
        first.append(w[0])
        length.append(w[1])
    want = span_ref.warp_spans([s for s, _ in cases.recs], idx, first, length, off, np.array(maps, dtype=np.int64), m_off, frames, pair_len)
    _same_f64(res["i.sym.hand.warp.s0"], want, "span_ref")
    assert length[1] == 20 * mc.HOP and length[4] == cases.recs[1][0].size - 5 * mc.HOP < 65 * mc.HOP      # whole frames; the clamp


# ---- j: the Spotter ------------------------------------------------------------------------------------------------
def _feed(world, recs, row, done, only=None):
    """(features, frame offsets) of one push: lane l gets row[l] frames of its recording from done[l] on."""
    blocks, off = [], [0]
    for l, r in enumerate(recs):
        n = row[l] if only is None or l == only else 0
        blocks.append(world.cases.recs[r][1][done[l]:done[l] + n])
        if only is None or l == only:
            done[l] += n
        off.append(off[-1] + n)
    return np.concatenate(blocks).reshape(-1), np.array(off, dtype=np.uint64)


def _events_of(res, p):
    return [(int(l), int(t)) + s for l, t, s in zip(res[p + ".lane"], res[p + ".target"], _spots(res, p))]


@pytest.mark.parametrize("limited", [False, True], ids=["free", "max_cost"])
@pytest.mark.parametrize("name,step", STEPS)
@pytest.mark.parametrize("lanes", [1, 3])
def test_j_spotter(res, world, cases, lanes, name, step, limited):
    p = "j.l%d.%s.%s" % (lanes, name, "max_cost" if limited else "free")
    _ok(res, p)
    recs, pushes = mc.spotter_lanes(lanes)
    again = mc.AGAIN[lanes]
    limits = world.args["spotter.max_cost"] if limited else None
    q = world.queries(world.tgts)
    sp = world.e.spotter(q, lanes, limits, step=step)
    try:
        done = [0] * lanes
        for k, row in enumerate(pushes):
            sp.push(*_feed(world, recs, row, done))
            _same_events(res, "%s.push%d" % (p, k), sp.events())             # in arrival order
            _same_best(res, "%s.push%d.best" % (p, k), sp.best())
            _same_ints(res["%s.push%d.counts" % (p, k)], sp.counts(), np.uint64, (p, k))
        for l in range(lanes):
            sp.flush(l)
            _same_events(res, "%s.flush%d" % (p, l), sp.events())
        sp.reset(again)
        _same_ints(res[p + ".reset.counts"], sp.counts(), np.uint64, p)
        _same_best(res, p + ".reset.best", sp.best())
        assert res[p + ".reset.counts"][again] == 0 and (res[p + ".reset.best.end"].reshape(lanes, -1)[again] == NO).all()
        done = [0] * lanes
        for k, row in enumerate(pushes):
            sp.push(*_feed(world, recs, row, done, only=again))
            _same_events(res, "%s.again%d" % (p, k), sp.events())
        sp.flush(again)
        _same_events(res, p + ".again.flush", sp.events())
        _same_best(res, p + ".again.best", sp.best())
        _same_ints(res[p + ".again.counts"], sp.counts(), np.uint64, p)
    finally:
        sp.close()
        q.close()
    # the second pass of the lane that was reset gives the first pass's events again
    for k in range(len(pushes)):
        assert _events_of(res, "%s.again%d" % (p, k)) == [e for e in _events_of(res, "%s.push%d" % (p, k)) if e[0] == again], (p, k)
    assert _events_of(res, p + ".again.flush") == _events_of(res, "%s.flush%d" % (p, again))
    assert np.array_equal(_bits(res[p + ".again.best.cost"]), _bits(res["%s.push%d.best.cost" % (p, len(pushes) - 1)]))
    # ... and events and bests against the restatement, bit for bit (tests/test_gpu_watch.py, tests/test_gpu_paced_watch.py)
    per_push, bests, flushed = mc.expected_events(cases, lanes, step, limits)
    same = lambda got, want: len(got) == len(want) and all(
        g[:3] == (w[0], w[1], w[0]) and g[3:5] == (w[3], w[4]) and _bits(g[5])[0] == _bits(w[2])[0] for g, w in zip(got, want))
    for k in range(len(pushes)):
        assert same(_events_of(res, "%s.push%d" % (p, k)), per_push[k]), (p, k)
        got = _spots(res, "%s.push%d.best" % (p, k))
        for l in range(lanes):
            for t in range(6):
                cost, start, end = bests[k][l][t]
                g = got[l * 6 + t]
                assert g[:3] == ((l, start, end) if end != NO else (NO, NO, NO)) and _bits(g[3])[0] == _bits(cost)[0], (p, k, l, t)
    for l in range(lanes):
        assert same(_events_of(res, "%s.flush%d" % (p, l)), flushed[l]), (p, l)


def test_j_follow(res, world):
    _ok(res, "j.follow")
    st = world.e.stream(2, mc.RATE)
    q = world.queries(world.tgts)
    sp = world.e.spotter(q, 2)
    try:
        done, seen = [0, 0], 0
        for k, row in enumerate(mc.FOLLOW):
            blocks = [world.recs[l].samples()[done[l]:done[l] + row[l]] for l in range(2)]
            done = [done[l] + row[l] for l in range(2)]
            st.push(np.concatenate(blocks), np.concatenate([[0], np.cumsum(row)]))
            sp.follow(st)
            _same_events(res, "j.follow.push%d" % k, sp.events())
            _same_best(res, "j.follow.push%d.best" % k, sp.best())
            _same_ints(res["j.follow.push%d.counts" % k], sp.counts(), np.uint64, k)
            seen += res["j.follow.push%d.lane" % k].size
        assert np.array_equal(sp.counts(), st.counts()[1]) and sp.counts()[0] == 300 and sp.counts()[1] >= 66
        for l in range(2):
            sp.flush(l)
            _same_events(res, "j.follow.flush%d" % l, sp.events())
            seen += res["j.follow.flush%d.lane" % l].size
        assert seen > 0
    finally:
        sp.close()
        q.close()
        st.close()


# ---- k: a replaced entry -------------------------------------------------------------------------------------------
def test_k_a_replaced_entry_is_followed(res, world):
    for name in ("k.spot", "k.spot.paced", "k.align", "k.warp_spans"):
        _ok(res, name)
    R, S = world.dictionary(world.recs), world.dictionary(world.segs)
    R.spot(world.tgts)                                                       # resident before the replacement, as in the program
    S.align(world.tgts, indices=mc.INDICES["a"])
    R.sounds[0] = world.repl[0]
    S.sounds[2] = world.repl[1]
    _same_spots(res, "k.spot", R.spot(world.tgts))
    _same_spots(res, "k.spot.paced", R.spot(world.tgts, step="paced"))
    _same_alignments(res, "k.align", S.align(world.tgts, indices=mc.INDICES["a"]))
    _same_f64(res["k.warp_spans.out"], R.warp(world.tgts, spans=R.spot(world.tgts)), "k.warp_spans")
    # the new content: target 3 sits elsewhere in the new recording 0, and is the new segment 2 itself
    assert _spots(res, "k.spot")[3][:3] == (0, mc.MOVED33, mc.MOVED33 + 32) and _spots(res, "g.sym")[3][:3] == (0, mc.PLANT33, mc.PLANT33 + 32)
    new, old = _alignments(res, "k.align")[3], _alignments(res, "e.sym.a")[3]
    assert new[0] == 0.0 and np.array_equal(new[2][:, 0], new[2][:, 1]) and old[0] > 1.0
    assert not np.array_equal(_bits(res["k.warp_spans.out"]), _bits(res["i.sym.spot.warp.s0"]))


# ---- l, m: refusals and the empty target list -------------------------------------------------------------------------
def _every_method(res, p, world, d, tgts, with_spotter, code=None):
    """The calls of the program's every_method() on the Python mirror: the same code, and where that is 0 the same results.
    code: the one code every call must give (an empty dictionary), whatever Python does."""
    n = len(tgts)
    idx, spots, e = [0] * n, [Spot(0, 0, 0, 0.0)] * n, d.engine

    def pair_matrix():
        q = world.queries(tgts, e)
        try:
            return e.pair_matrix(d.resident(), q, exact=True, step="paced")
        finally:
            q.close()

    def spotter(step):
        q = world.queries(tgts, e)
        try:
            sp = e.spotter(q, 2, None, step=step)
            try:
                return sp.counts(), sp.best()
            finally:
                sp.close()
        finally:
            q.close()

    def check(name, call, same):
        want, out = (code, None) if code is not None else _try(call)
        _same_code(res, name, want)
        if want == 0:
            same(out)

    check(p + ".match_indices_step", lambda: d.match_indices(tgts, step="paced"),
          lambda out: (_same_ints(res[p + ".match_indices_step.idx"], out[0], np.uint32, p), _same_f64(res[p + ".match_indices_step.cost"], out[1], p)))
    check(p + ".pair_matrix_step", pair_matrix, lambda out: _same_f64(res[p + ".pair_matrix_step.out"], out, p))
    check(p + ".candidates", lambda: d.candidates(tgts, 2), lambda out: _same_sound_lists(res, p + ".candidates", out, d))
    for name, step in STEPS:
        s = "." + name
        check(p + ".align" + s, lambda: d.align(tgts, indices=idx, step=step), lambda out: _same_alignments(res, p + ".align" + s, out))
        check(p + ".spot" + s, lambda: d.spot(tgts, step=step), lambda out: _same_spots(res, p + ".spot" + s, out))
        check(p + ".spot.idx" + s, lambda: d.spot(tgts, indices=idx, step=step), lambda out: _same_spots(res, p + ".spot.idx" + s, out))
        check(p + ".spot_all" + s, lambda: d.spot_all(tgts, step=step), lambda out: _same_spot_lists(res, p + ".spot_all" + s, out))
        check(p + ".spot_all.idx" + s, lambda: d.spot_all(tgts, indices=idx, step=step),
              lambda out: _same_spot_lists(res, p + ".spot_all.idx" + s, out))
        check(p + ".align_spans" + s, lambda: d.align(tgts, spans=spots, step=step),
              lambda out: _same_alignments(res, p + ".align_spans" + s, out))
        check(p + ".warp_spans" + s, lambda: d.warp(tgts, spans=spots, step=step), lambda out: _same_f64(res[p + ".warp_spans" + s], out, p))
        if with_spotter:
            check(p + ".spotter" + s, lambda: spotter(step),
                  lambda out: (_same_ints(res[p + ".spotter" + s + ".counts"], out[0], np.uint64, p), _same_best(res, p + ".spotter" + s + ".best", out[1])))
    check(p + ".warp", lambda: d.warp(tgts, indices=idx), lambda out: _same_f64(res[p + ".warp.out"], out, p))
    check(p + ".wsola", lambda: d.warp(tgts, indices=idx, search=7), lambda out: _same_f64(res[p + ".wsola.out"], out, p))
    check(p + ".wsola_spans", lambda: d.warp(tgts, spans=spots, search=7), lambda out: _same_f64(res[p + ".wsola_spans.out"], out, p))


def test_l_refusals_by_their_arguments(res, world):
    S, R, tgts, e = world.S, world.R, world.tgts, world.e
    si, ia = world.args["spot.indices"], mc.INDICES["a"]
    five, outside = [0] * 5, [0, 1, 99, 2, 4, 3]
    good = [Spot(0, 0, 5, 0.0)] * 6
    beyond, outside_spots = list(good), list(good)
    beyond[2], outside_spots[2] = Spot(1, 60, 70, 0.0), Spot(99, 0, 5, 0.0)

    def spotter(lanes, max_cost, then):
        q = world.queries(tgts)
        try:
            sp = e.spotter(q, lanes, max_cost)
            try:
                then(sp)
            finally:
                sp.close()
        finally:
            q.close()

    calls = {
        "l.align.length": lambda: S.align(tgts, indices=five),
        "l.align.length.paced": lambda: S.align(tgts, indices=five, step="paced"),
        "l.align.length.none": lambda: S.align([], indices=five),
        "l.warp.length": lambda: S.warp(tgts, indices=five),
        "l.spot.length": lambda: R.spot(tgts, indices=five),
        "l.spot.length.paced": lambda: R.spot(tgts, indices=five, step="paced"),
        "l.spot_all.length": lambda: R.spot_all(tgts, indices=five),
        "l.align_spans.length": lambda: R.align(tgts, spans=good[:5]),
        "l.warp_spans.length": lambda: R.warp(tgts, spans=good[:5]),
        "l.spotter.max_cost.length": lambda: spotter(1, [1.0] * 5, lambda sp: None),
        "l.spotter.frame_offsets.length": lambda: spotter(3, None, lambda sp: sp.push(np.zeros(NCOEFFS), [0, 1, 1])),
        "l.align.outside": lambda: S.align(tgts, indices=outside),
        "l.warp.outside": lambda: S.warp(tgts, indices=outside),
        "l.spot.outside": lambda: R.spot(tgts, indices=outside),
        "l.spot_all.outside": lambda: R.spot_all(tgts, indices=outside),
        "l.align_spans.outside": lambda: R.align(tgts, spans=outside_spots),
        "l.warp_spans.outside": lambda: R.warp(tgts, spans=outside_spots),
        "l.align_spans.beyond": lambda: R.align(tgts, spans=beyond),
        "l.warp_spans.beyond": lambda: R.warp(tgts, spans=beyond),
        "l.warp.search513": lambda: S.warp(tgts, indices=ia, search=513),
        "l.warp_spans.search513": lambda: R.warp(tgts, spans=good, search=513),
        "l.spot_all.max_spots0": lambda: R.spot_all(tgts, max_spots=0),
        "l.spot_all.max_spots65": lambda: R.spot_all(tgts, max_spots=65),
        "l.spot_all.idx.max_spots0": lambda: R.spot_all(tgts, indices=si, max_spots=0),
        "l.spot_all.idx.max_spots65": lambda: R.spot_all(tgts, indices=si, max_spots=65),
        "l.flush.lane": lambda: spotter(2, None, lambda sp: sp.flush(2)),
        "l.reset.lane": lambda: spotter(2, None, lambda sp: sp.reset(2)),
    }
    for name, call in calls.items():
        code, _ = _try(call)
        assert code == nat.SSYM_E_INVALID, name                               # every one of them is a mistake in Python
        _same_code(res, name, code)
    assert sum(k.startswith("l.") and k.endswith(".code") and "refcos" not in k and "empty" not in k for k in res) == len(calls)


def test_l_a_refcos_context_and_an_empty_dictionary(res, world):
    r = Engine(metric="refcos", dtype="f64")
    try:
        _every_method(res, "l.refcos", world, world.dictionary(world.recs, r), world.tgts, True)
    finally:
        r.close()
    # every DTW-family method refuses a refcos context; candidates is no such method
    for key, value in res.items():
        if key.startswith("l.refcos.") and key.endswith(".code"):
            assert (int(value[0]) == 0) == (key == "l.refcos.candidates.code"), key
    _every_method(res, "l.empty", world, world.dictionary([]), world.tgts, False, code=nat.SSYM_E_EMPTY_DICT)
    _same_code(res, "l.empty.chain", nat.SSYM_E_EMPTY_DICT)
    _same_code(res, "l.empty.empty", nat.SSYM_E_EMPTY_DICT)
    assert _try(lambda: world.dictionary([]).align([], indices=[]))[0] == nat.SSYM_E_EMPTY_DICT
    assert _try(lambda: world.dictionary([]).spot(world.tgts))[0] == nat.SSYM_E_EMPTY_DICT


def test_m_an_empty_target_list(res, world):
    _every_method(res, "m", world, world.R, [], True)
    for key, value in res.items():
        if key.startswith("m.") and key.endswith(".code"):
            assert int(value[0]) == 0, key                                    # Python returns empty results; so does the mirror
    assert all(res[k].size == 0 for k in ("m.align.sym.cost", "m.warp.out", "m.spot.paced.cost", "m.warp_spans.sym", "m.wsola_spans.out"))
    assert res["m.spot_all.sym.off"].tolist() == [0] and res["m.spotter.sym.counts"].tolist() == [0, 0]


def test_the_run_wrote_every_call(child, res):
    assert "every call returned or threw a soundsym::Error" in child.output
    codes = [k for k in res if k.endswith(".code")]
    assert len(codes) == 148 and not any(res[k][0] in (9998.0, 9999.0) for k in codes)
