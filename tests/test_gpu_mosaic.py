"""ssym_dtw_mosaic on the GPU held to tests/mosaic_ref.py bit for bit (DESIGN.md section 2 "Mosaic", section 5.25) on the
cases of the contract: the segment boundary, the planted spans with and without noise, the intruder left as gap frames, NaN
and infinite frames on either side, rounds of fewer workgroups than targets under a lowered scratch cap, every refusal
with the outputs unwritten, the total against ssym_spot_queries_step and the pieces against ssym_dtw_align_spans on the GPU,
and results that do not depend on what the context ran before."""
import numpy as np
import pytest

import mosaic_ref as ref
from mosaic_gpu import GAP, INF, NAN, NONE, Sets, bits, call, check, error, pieces_of, real, same
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu


def test_boundary_is_two_pieces():
    segs, x, pieces = ref.boundary_case()
    with Sets(segs, [x], 13) as sets:
        for penalty in (0.3, 20.0):
            got = check(sets, penalty)
            assert pieces_of(got, sets.tgt, 0) == pieces and bits(got[1][0]) == bits(penalty + penalty)


@pytest.mark.parametrize("noise", [0.0, 1e-3])
def test_planted_spans_come_back(noise):
    recs, x, pieces = ref.planted_case(noise)
    with Sets(recs, [x], 13) as sets:
        got = check(sets, 1.0)
        assert pieces_of(got, sets.tgt, 0) == pieces
        if not noise:
            assert got[1][0] == 3.0
        check(sets, 0.0, device=True)                        # frame-wise at penalty 0: the restatement's fragments


def test_intruder_frames_are_gap_frames():
    recs, x, pieces, (first, last) = ref.intruder_case()
    with Sets(recs, [x], 13, dtype="f32") as sets:
        got = check(sets, 1.0, 1.5)
        assert got[1][0] == 8.0
        assert pieces_of(got, sets.tgt, 0) == ([pieces[0]] + [(GAP, NONE, NONE, j, j) for j in range(first, last + 1)] +
                                                [pieces[1]])
        assert (got[5][first:last + 1] == 1.5).all()


def test_non_finite_frames():
    recs, x, _ = ref.planted_case()
    bad = [a.copy() for a in recs]
    bad[1][9] = NAN
    bad[2][0, 3] = INF
    bad[0][39] = NAN                                         # the dictionary's frame 39, next to segment 1's first
    y = x.copy()
    y[12, 5] = NAN
    with Sets(bad, [x, x[:1]], 13) as sets:
        got = check(sets, 1.0)
        assert got[0][0] > 0
        on = {(int(s), int(f)) for s, f in zip(got[3], got[4])}
        assert not on & {(1, 9), (2, 0), (0, 39)}
        check(sets, 1.0, 1.5, device=True)
    with Sets(recs, [x, y], 13) as sets:
        got = check(sets, 1.0)
        assert got[0][0] == 3 and got[0][1] == 0 and got[1][1] == INF
        got = check(sets, 1.0, 1.5, device=True)
        found = pieces_of(got, sets.tgt, 1)
        assert [p for p in found if p[0] == GAP] == [(GAP, NONE, NONE, 12, 12)] and found[0][0] != GAP and found[-1][0] != GAP


def test_rounds_under_a_lowered_scratch_cap(monkeypatch):
    """Five targets, room for two workgroups: three rounds on the same slabs, short targets of the same call included."""
    rng = np.random.default_rng(21)
    src = [real(rng, 70, 5), real(rng, 61, 5)]
    tgt = [real(rng, f, 5) for f in (33, 2, 0, 40, 17)]
    G, T = 131, 40
    slab, shared = G * T + 32 * G + 8 + 4 * T, 144 + 8 * 5 * G       # per workgroup; pos and the transposed frames, per call
    with Sets(src, tgt, 5) as sets:
        want = check(sets, 0.3, 0.7)
        assert sets.e.timings()["main_launches"] == 1
        monkeypatch.setenv("SSYM_MOSAIC_SCRATCH_BYTES", str(2 * slab + shared + slab // 2))
        same(check(sets, 0.3, 0.7), want)
        assert sets.e.timings()["main_launches"] == 3
        same(check(sets, 0.3, 0.7, device=True), want)
        monkeypatch.setenv("SSYM_MOSAIC_SCRATCH_BYTES", str(slab + shared - 1))      # one byte short of the longest target
        rc, _, untouched = call(sets, 0.3, 0.7)
        assert rc == nat.SSYM_E_UNSUPPORTED and untouched and "ssym_dtw_mosaic" in error(sets)
        monkeypatch.delenv("SSYM_MOSAIC_SCRATCH_BYTES")
        same(check(sets, 0.3, 0.7), want)


def test_refusals_leave_the_outputs_unwritten():
    rng = np.random.default_rng(22)
    src, tgt = [real(rng, 9, 3)], [real(rng, 4, 3)]
    with Sets(src, tgt, 3) as sets:
        for penalty, gap in ((NAN, INF), (-1.0, INF), (INF, INF), (0.0, NAN), (0.0, -0.5), (0.0, -INF)):
            for device in (False, True):
                rc, _, untouched = call(sets, penalty, gap, device=device)
                assert rc == nat.SSYM_E_INVALID and untouched and "ssym_dtw_mosaic" in error(sets)
        check(sets, 0.0, INF)
    for kw in (dict(metric="refcos"), dict(band=3)):
        with Sets(src, tgt, 3, **kw) as sets:
            rc, _, untouched = call(sets, 0.3)
            assert rc == nat.SSYM_E_UNSUPPORTED and untouched and "ssym_dtw_mosaic" in error(sets)
    wide = [real(rng, 5, 65)]
    with Sets(wide, wide, 65) as sets:
        rc, _, untouched = call(sets, 0.3)
        assert rc == nat.SSYM_E_UNSUPPORTED and untouched
    with Sets([], tgt, 3) as sets:
        rc, _, untouched = call(sets, 0.3)
        assert rc == nat.SSYM_E_EMPTY_DICT and untouched
    with Sets(src, [], 3) as sets:                           # no targets: success with nothing written
        rc, _, untouched = call(sets, 0.3)
        assert rc == nat.SSYM_OK and untouched


def test_against_spotting_on_the_gpu():
    """(4): at penalty 0 without gaps total <= ssym_spot_queries_step(PACED)'s cost; on small-integer features, squared,
    with a penalty of 1024 the mosaic is that call's spot and total == penalty + cost."""
    rng = np.random.default_rng(23)
    lens = (5, 9, 12, 7, 3)
    src = [real(rng, 30, 3), real(rng, 41, 3), real(rng, 25, 3)]
    tgt = [real(rng, f, 3) for f in lens]
    with Sets(src, tgt, 3) as sets:
        got = check(sets, 0.0)
        _, cost, _, _ = sets.e.spot_queries(sets.d, sets.q, step="paced")
        assert (got[1] <= cost).all()
    src = [rng.integers(0, 4, (f, 3)).astype(np.float64) for f in (30, 41, 25)]
    tgt = [rng.integers(0, 4, (f, 3)).astype(np.float64) for f in lens]
    with Sets(src, tgt, 3, squared=True) as sets:
        got = check(sets, 1024.0)
        idx, cost, start, end = sets.e.spot_queries(sets.d, sets.q, step="paced")
        for t, f in enumerate(lens):
            assert pieces_of(got, sets.tgt, t) == [(int(idx[t]), int(start[t]), int(end[t]), 0, f - 1)]
            assert got[1][t] == 1024.0 + cost[t]


def piece_costs(pieces, cost):
    out = []
    for _, _, _, a, b in pieces:
        acc = float(cost[a])
        for j in range(a + 1, b + 1):
            acc = float(cost[j]) + acc
        out.append(acc)
    return out


@pytest.mark.parametrize("exact", [False, True])
def test_against_span_alignment_on_the_gpu(exact):
    """(5): a piece's cost is at least ssym_dtw_align_spans(SSYM_STEP_PACED)'s for (segment, [first, last], the cut), and
    equal to it on exactly representable inputs."""
    rng = np.random.default_rng(24)
    if exact:
        src = [rng.integers(0, 4, (f, 2)).astype(np.float64) for f in (14, 9, 20)]
        x = rng.integers(0, 4, (31, 2)).astype(np.float64)
    else:
        src, x = [real(rng, f, 2) for f in (14, 9, 20)], real(rng, 31, 2)
    with Sets(src, [x], 2, squared=exact) as sets:
        got = check(sets, 0.5)
        pieces = pieces_of(got, sets.tgt, 0)
        assert len(pieces) >= 2
        cuts = sets.e.queries(*pack_segments([x[a:b + 1] for _, _, _, a, b in pieces], 2, np.float64), 2)
        spans = (np.array([p[1] for p in pieces], dtype=np.uint32), np.array([p[2] for p in pieces], dtype=np.uint32))
        alone, _, _, _ = sets.e.dtw_align(sets.d, cuts, [p[0] for p in pieces], step="paced", spans=spans)
        mine = np.array(piece_costs(pieces, got[5]))
        assert (mine >= alone).all()
        if exact:
            assert (bits(mine) == bits(alone)).all()


def test_results_do_not_depend_on_what_the_context_ran_before():
    recs, x, _ = ref.planted_case(1e-3)
    rng = np.random.default_rng(25)
    other = [real(rng, 300, 13)]
    with Sets(recs, [x, x[:7]], 13) as sets:
        want = check(sets, 1.0, 1.5)
        sets.e.match(sets.d, sets.q)
        sets.e.dtw_cover(sets.d, sets.e.queries(*pack_segments([x[:9]], 13, np.float64), 13), 1.0)
        big = sets.e.dictionary(*pack_segments(other, 13, np.float64), 13)
        qs = sets.e.queries(*pack_segments([x, x], 13, np.float64), 13)
        sets.e.dtw_mosaic(big, qs, 0.1)                       # larger slabs, other contents
        sets.e.spot_queries(sets.d, sets.q, step="paced")
        same(check(sets, 1.0, 1.5), want)
        same(check(sets, 1.0, 1.5, device=True), want)
