"""ssym_dtw_cover_gaps on the GPU held to tests/cover_gaps_ref.py bit for bit (DESIGN.md section 2 "Cover with gaps", section
5.23): counts, totals, all four piece arrays and the padding of the unused slots; targets of 0, 1, 3, 40 and 600 frames (past
the chain's 512-entry ring) in one call; gap_cost = +inf against ssym_dtw_cover on the same context; the planted intruder, a
NaN frame, a target too short for every segment and the tie; SSYM_OUT_DEVICE; every refusal; and ssym_dtw_cover unchanged
by the calls around it."""
import numpy as np
import pytest

import cover_gaps_ref as ref
import cover_ref
from cover_gpu import INF, SENT32, SENTF, Sets, bits, error, pieces_of, real, same
from cover_gpu import call as call_plain
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu

GAP = ref.GAP
SIZES = (0, 1, 3, 40, 600)
PENALTIES = (0.0, 2.0)
GAP_COSTS = (0.0, 0.5, 3.0, INF)


def call(sets, penalty=0.0, gap_cost=INF, device=False):
    """ssym_dtw_cover_gaps into sentinel-filled outputs with one entry more than each needs:
    (rc, (count, total, src, start, end, cost), untouched)."""
    m, frames = len(sets.tgt), int(sum(np.asarray(x).shape[0] for x in sets.tgt))
    sizes = (m, m, frames, frames, frames, frames)
    outs = [np.full(n + 1, SENTF) if k in (1, 5) else np.full(n + 1, SENT32, dtype=np.uint32) for k, n in enumerate(sizes)]
    head = (sets.e.ctx, sets.d.ptr, sets.q.ptr, float(penalty), float(gap_cost))
    if device:
        import torch
        dev = [torch.from_numpy(o if o.dtype == np.float64 else o.view(np.int32)).cuda() for o in outs]
        torch.cuda.synchronize()
        rc = nat.lib().ssym_dtw_cover_gaps(*head, nat.OUT_DEVICE, *(d.data_ptr() for d in dev))
        torch.cuda.synchronize()
        outs = [d.cpu().numpy() if o.dtype == np.float64 else d.cpu().numpy().view(np.uint32) for d, o in zip(dev, outs)]
    else:
        rc = nat.lib().ssym_dtw_cover_gaps(*head, 0, *(o.ctypes.data for o in outs))
    sent = lambda o: SENTF if o.dtype == np.float64 else SENT32
    untouched = all(o[n] == sent(o) for o, n in zip(outs, sizes))
    if rc != nat.SSYM_OK:
        untouched = untouched and all((o == sent(o)).all() for o in outs)
    return rc, tuple(o[:n] for o, n in zip(outs, sizes)), bool(untouched)


def check(sets, penalty, gap_cost, want, **kw):
    rc, got, untouched = call(sets, penalty, gap_cost, **kw)
    assert rc == nat.SSYM_OK, error(sets)
    assert untouched
    same(got, want)
    return got


@pytest.fixture(scope="module")
def ragged():
    """The ragged dictionary (1 ... 40 frames and one segment of 128) and the targets of SIZES frames, with the
    restatement's tables, computed once.  The two longer targets alternate noisy copies of dictionary segments (a few
    tenths per frame away from them) with frames of their own (about 5 per frame away from everything), so that a gap_cost
    between the two leaves some frames uncovered and covers the others."""
    class R:
        pass
    r = R()
    rng = np.random.default_rng(0x6A9C)
    r.src = [real(rng, n, 13) for n in (1, 5, 40, 12, 33, 7, 128, 21, 2, 17)]

    def mixed(frames):
        parts, k = [], 0
        while sum(p.shape[0] for p in parts) < frames:
            a = r.src[(2, 6, 4, 7, 3, 9)[k % 6]]
            parts += [(a + 0.05 * rng.standard_normal(a.shape)).astype(np.float32).astype(np.float64), real(rng, 3 + 4 * (k % 3), 13)]
            k += 1
        return np.concatenate(parts)[:frames]

    r.tgt = [mixed(n) if n >= 40 else real(rng, n, 13) for n in SIZES]
    r.tabs = cover_ref.all_tables(r.src, r.tgt)
    return r


@pytest.fixture(scope="module")
def ragged_sets(ragged):
    with Sets(ragged.src, ragged.tgt, 13) as sets:
        yield sets


@pytest.mark.parametrize("gap_cost", GAP_COSTS)
@pytest.mark.parametrize("penalty", PENALTIES)
def test_ragged_targets_in_one_call(ragged, ragged_sets, penalty, gap_cost):
    sets = ragged_sets
    rc, before, _ = call_plain(sets, penalty)
    assert rc == nat.SSYM_OK, error(sets)
    want = ref.arrays(ragged.src, ragged.tgt, penalty, gap_cost, tabs=ragged.tabs)
    got = check(sets, penalty, gap_cost, want)
    check(sets, penalty, gap_cost, want, device=True)
    off = np.concatenate([[0], np.cumsum(SIZES)])
    assert got[0][0] == 0 and got[1][0] == INF                                # no frames: no cover, gaps or not
    if gap_cost < INF:
        assert (got[0][1:] > 0).all() and np.isfinite(got[1][1:]).all()       # consequence 5
        for t in range(1, len(SIZES)):
            pieces = pieces_of(got, ragged.tgt, t)
            assert ref.tiles(pieces, SIZES[t])
            assert bits(ref.resum(pieces, penalty)) == bits(got[1][t])
            assert all(bits(c) == bits(gap_cost) for s, _, _, c in pieces if s == GAP)
        # the unused slots keep SSYM_NO_MATCH: a gap is not an empty slot
        tail = slice(off[4] + int(got[0][4]), off[5])
        assert (got[2][tail] == cover_ref.NONE).all() and (got[5][tail] == INF).all()
    else:
        same(got, before)                                                      # consequence 6, all six outputs
        same(got, cover_ref.arrays(ragged.src, ragged.tgt, penalty, tabs=ragged.tabs))
    if gap_cost == 0.0:
        assert (got[2][:off[5]][got[2][:off[5]] != cover_ref.NONE] == GAP).all() and (got[1][1:] == 0.0).all()
    # ssym_dtw_cover on the same context still returns what it returned before the calls
    rc, after, untouched = call_plain(sets, penalty)
    assert rc == nat.SSYM_OK and untouched
    same(after, before)


def test_the_gaps_of_the_ragged_set_mix_with_pieces(ragged, ragged_sets):
    """The parameters above reach all three kinds of cover on the long target: gaps only, pieces only, both."""
    kinds = set()
    for gap_cost in GAP_COSTS:
        got = check(ragged_sets, 0.0, gap_cost, ref.arrays(ragged.src, ragged.tgt, 0.0, gap_cost, tabs=ragged.tabs))
        src = [p[0] for p in pieces_of(got, ragged.tgt, 4)]
        kinds.add((GAP in src, any(s != GAP for s in src)))
    assert kinds == {(True, False), (False, True), (True, True)}


def test_planted_intruder():
    segs, x, planted, (first, last) = ref.intruder_case()
    with Sets(segs, [x], 13) as sets:
        got = check(sets, 0.0, 1.0, ref.arrays(segs, [x], 0.0, 1.0))
        pieces = pieces_of(got, [x], 0)
        check(sets, 0.0, 1.0, ref.arrays(segs, [x], 0.0, 1.0), device=True)
    assert bits(got[1][0]) == bits(7.0)
    assert [p[:3] for p in pieces if p[0] != GAP] == planted and all(p[3] == 0.0 for p in pieces if p[0] != GAP)
    assert [p for p in pieces if p[0] == GAP] == [(GAP, f, f, 1.0) for f in range(first, last + 1)]


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_one_frame_that_is_not_finite(value):
    segs, x, planted, at = ref.nan_case()
    x[at] = value
    with Sets(segs, [x, x[:at + 1], x[at:]], 13) as sets:
        rc, plain, _ = call_plain(sets)
        assert rc == nat.SSYM_OK and plain[0].tolist() == [0, 0, 0]           # without gaps: no cover at all
        got = check(sets, 0.0, 1.0, ref.arrays(segs, [x, x[:at + 1], x[at:]], 0.0, 1.0))
    pieces = pieces_of(got, [x], 0)
    assert [p for p in pieces if p[0] == GAP] == [(GAP, at, at, 1.0)] and bits(got[1][0]) == bits(1.0)
    assert [p[:3] for p in pieces if p[0] != GAP] == planted                  # the frames on both sides are covered
    tgts = [x, x[:at + 1], x[at:]]                                            # the bad frame last in a target, and first
    assert pieces_of(got, tgts, 1)[-1] == (GAP, at, at, 1.0) and pieces_of(got, tgts, 2)[0] == (GAP, 0, 0, 1.0)
    assert bits(got[1][1:]).tolist() == bits([1.0, 1.0]).tolist()


def test_a_target_too_short_for_every_segment():
    segs, x = ref.short_case()
    with Sets(segs, [x], 13) as sets:
        rc, plain, _ = call_plain(sets, 2.0)
        assert rc == nat.SSYM_OK and plain[0][0] == 0 and plain[1][0] == INF
        for gap_cost in (0.5, 3.0):
            got = check(sets, 2.0, gap_cost, ref.arrays(segs, [x], 2.0, gap_cost))
            assert pieces_of(got, [x], 0) == [(GAP, f, f, gap_cost) for f in range(3)] and got[1][0] == 3 * gap_cost


def test_a_piece_wins_a_tie_against_a_gap():
    segs, x, gap_cost, want = ref.tie_case()
    with Sets(segs, [x], 1) as sets:
        got = check(sets, 0.0, gap_cost, ref.arrays(segs, [x], 0.0, gap_cost))
        assert pieces_of(got, [x], 0) == want and got[1][0] == 4.0
        under = float(np.nextafter(gap_cost, 0.0))
        got = check(sets, 0.0, under, ref.arrays(segs, [x], 0.0, under))
        assert got[2].tolist() == [GAP] * 4


def test_refusals(ragged):
    with Sets(ragged.src, ragged.tgt[:4], 13) as sets:
        for bad in (float("nan"), -1.0, -INF, -1e-300):
            rc, _, untouched = call(sets, 0.0, bad)
            assert rc == nat.SSYM_E_INVALID and untouched and "gap_cost" in error(sets)
            rc, _, untouched = call(sets, 0.0, bad, device=True)
            assert rc == nat.SSYM_E_INVALID and untouched
        for bad in (float("nan"), -1.0, INF):
            rc, _, untouched = call(sets, bad, 1.0)
            assert rc == nat.SSYM_E_INVALID and untouched and "piece_penalty" in error(sets)
        want = ref.arrays(ragged.src, ragged.tgt[:4], 0.0, 0.5, tabs=ragged.tabs[:4])
        check(sets, 0.0, 0.5, want)                                            # the context goes on after the refusals
    for kw in (dict(metric="refcos"), dict(band=8)):
        with Sets(ragged.src, ragged.tgt[:4], 13, **kw) as sets:
            rc, _, untouched = call(sets, 0.0, 1.0)
            assert rc == nat.SSYM_E_UNSUPPORTED and untouched and "ssym_dtw_cover_gaps" in error(sets)
