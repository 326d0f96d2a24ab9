"""Paced matching on the GPU (ssym_match_queries_step and ssym_pair_matrix_step with SSYM_STEP_PACED) against the numpy
restatement (tests/paced_match_ref.py), bit for bit: the matrix and the match on ragged sets in both dtypes, squared and
not, against ssym_dtw_align_step's costs over the full pair list, with distances, an index base and device outputs; the
case that motivates the call and the planted cuts that cost exactly 0.0; both ties of the cell on integer features; every
match aligned at its cost; features that are not finite; the symmetric step as the existing calls; the same bits whatever
the context ran before; every refusal."""
import numpy as np
import pytest

import nonfinite_cases
import paced_match_ref as ref
import paced_path_ref
from dtw_path_ref import local_costs
from paced_ref import _down
from paced_match_gpu import (INF, NAN, PACED, SENT32, SENTF, SYMMETRIC, Sets, align_costs, bits, check_match, check_matrix,
                             error, match, matrix, real, same_as_align, same_bits)
from soundsym_amd import HOP, Sound, SoundDictionary, SoundSequence, SsymError
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

DIM = 13


# -- ragged sets: 37 sources x 9 targets of 1 ... 40 frames ---------------------------------------------------------------
class _Ragged:
    def __init__(self):
        rng = np.random.default_rng(0x9ACED)
        fa = [1, 40, 2, 39] + [int(f) for f in rng.integers(1, 41, size=33)]
        fb = [1, 40, 2, 21, 20] + [int(f) for f in rng.integers(3, 41, size=4)]
        self.src = [real(rng, f, DIM) for f in fa]
        self.tgt = [real(rng, f, DIM) for f in fb]
        self.want = {sq: ref.matrix(self.src, self.tgt, sq) for sq in (False, True)}
        self.distance = np.array([0.0, 90.0, 3.5, 70.0, 55.5, 120.0, 1e6, 40.0, 61.25])


@pytest.fixture(scope="module")
def ragged():
    return _Ragged()


@pytest.mark.parametrize("dtype,squared", [("f64", False), ("f64", True), ("f32", False), ("f32", True)])
def test_matrix_and_match_on_ragged_sets(ragged, dtype, squared):
    want = ragged.want[squared]
    assert want.shape == (37, 9) and np.isinf(want).any() and np.isfinite(want).sum() > 100
    with Sets(ragged.src, ragged.tgt, DIM, dtype, squared) as sets:
        mat = check_matrix(sets, want)
        same_as_align(mat, align_costs(sets)[0])
        check_match(sets, want)
        dist = ragged.distance * (40.0 if squared else 1.0)
        check_match(sets, want, dist)
        check_match(sets, want, dist, base=1000)
        check_match(sets, want, None, base=1000, device=True)
        check_match(sets, want, dist, base=7, device=True)
        check_match(sets, want, dist, want_cost=False)
        check_match(sets, want, dist, device=True, want_cost=False)
        # the flags that mean nothing under the paced pattern change nothing
        check_match(sets, want, dist, flags=nat.DTW_FORCE_EXACT | nat.DTW_PRUNE)
        tm = sets.e.timings()
        assert tm["n_pairs"] == 37 * 9 and tm["main_ms"] > 0 and tm["reduce_ms"] > 0 and tm["used_filter"] == 0


def test_every_finite_match_is_aligned_at_its_cost(ragged):
    """Contract point 2: ssym_dtw_align_step on (returned index, target) gives out_len = Fb and the returned cost."""
    with Sets(ragged.src, ragged.tgt, DIM) as sets:
        for dist in (None, ragged.distance):
            rc, idx, cost, _ = match(sets, dist)
            assert rc == nat.SSYM_OK and np.isfinite(cost).sum() >= 8
            acost, alen, _, amap = sets.e.dtw_align(sets.d, sets.q, idx, step="paced")
            for t in range(len(ragged.tgt)):
                if np.isfinite(cost[t]):
                    assert int(alen[t]) == ragged.tgt[t].shape[0] and bits(acost[t]) == bits(cost[t]), t
                    assert paced_path_ref.admissible(amap[t], ragged.src[int(idx[t])].shape[0])


# -- the motivating case, and the 0.0 cases --------------------------------------------------------------------------------
def _sound(feats, k):
    rng = np.random.default_rng(0x50 + k)
    return Sound(rng.standard_normal(feats.shape[0] * HOP), 8000.0, feats.reshape(-1), "s%d" % k, ncoeffs=feats.shape[1])


def test_the_motivating_case():
    src, tgt = ref.abc_case()
    with Sets(src, tgt, DIM) as sets:
        idx, cost = sets.e.match(sets.d, sets.q)
        assert idx.tolist() == [0] and cost[0] == 0.0                     # the symmetric search: A
        idx, cost = sets.e.match(sets.d, sets.q, step="paced")
        want = ref.matrix(src, tgt)
        assert idx.tolist() == [1] and bits(cost[0]) == bits(want[1, 0])   # the paced search: B
        d = SoundDictionary(engine=sets.e)
        d.sounds = [_sound(s, k) for k, s in enumerate(src)]
        targets = [_sound(tgt[0], 9)]
        old = d.align(targets, step="paced")
        new = d.align(targets, step="paced", match_step="paced")
        assert len(old) == len(new) == 1
        assert old[0].source_index == 0 and len(old[0]) == 0 and old[0].cost == INF      # A cannot be aligned
        assert new[0].source_index == 1 and len(new[0]) == 10 and bits(new[0].cost) == bits(want[1, 0])
        assert [len(a) for a in SoundSequence.new(targets).align_to_dictionary(d, step="paced", match_step="paced")] == [10]
        i2, c2 = d.match_indices(targets, step="paced", per_frame=True)
        assert i2.tolist() == [1] and c2[0] == want[1, 0] / 10.0
        i3, _ = d.match_indices(targets, [want[2, 0] / 10.0], step="paced", per_frame=True)
        assert i3.tolist() == [2]
        assert SoundSequence.new(targets).clone_from_dictionary(d, step="paced").sounds()[0] is d.sounds[1]
        assert SoundSequence.new(targets).morph_to([want[2, 0] / 10.0], d, step="paced", per_frame=True).sounds()[0] is d.sounds[2]
        warped = d.warp(targets, step="paced", match_step="paced")
        assert warped.shape == (10 * HOP,)


def test_planted_cuts_cost_exactly_zero():
    """A target that is a cut of an entry with every second frame dropped, or every frame doubled, matches it at 0.0."""
    rng = np.random.default_rng(0x2E0)
    entry, short = real(rng, 39, DIM), real(rng, 17, DIM)
    src = [real(rng, 30, DIM), entry, real(rng, 20, DIM), short, real(rng, 35, DIM)]
    tgt = [entry[::2], np.repeat(short, 2, axis=0), np.repeat(entry[4:24], 2, axis=0), entry[3:36:2]]
    src.append(entry[4:24])                     # the cut the doubled target was made from
    src.append(entry[3:36])
    for squared in (False, True):
        with Sets(src, tgt, DIM, squared=squared) as sets:
            rc, idx, cost, _ = match(sets)
            assert rc == nat.SSYM_OK and idx.tolist() == [1, 3, 5, 6]
            assert (bits(cost) == bits(np.zeros(4))).all()
            check_match(sets, ref.matrix(src, tgt, squared))


# -- both ties of the cell ----------------------------------------------------------------------------------------------------
def _finite_ties(a, b):
    """(cells with E(i-2,j-1) == E(i-1,j-1), cells with H == N), finite values only, of paced_path_ref.forward's recurrence."""
    c = local_costs(a, b, True)
    n = np.full(c.shape[0], INF)
    n[0] = c[0, 0]
    e, pred, state = n.copy(), 0, 0
    for j in range(1, c.shape[1]):
        p, p2 = _down(e, 1, INF), _down(e, 2, INF)
        pred += int(((p2 == p) & np.isfinite(p)).sum())
        h, n = c[:, j] + n, c[:, j] + np.minimum(p, p2)
        state += int(((h == n) & np.isfinite(n)).sum())
        e = np.minimum(h, n)
    return pred, state


def test_both_ties_of_the_cell_on_integer_features():
    """Features in {0, 1, 2}, one value per frame, sources of 3 ... 5 frames, targets of 3 and 4: every sum is exact, so the
    second diagonal equals the first and H equals N in many cells, and strict < has to keep row i - 1 and state N."""
    rng = np.random.default_rng(0x71E5)
    ints = lambda f: rng.integers(0, 3, size=(f, 1)).astype(np.float64)
    src = [ints(3 + k % 3) for k in range(12)]
    tgt = [ints(3 + k % 2) for k in range(6)]
    ties = np.array([_finite_ties(a, b) for a in src for b in tgt if paced_path_ref.feasible(a.shape[0], b.shape[0])])
    assert (ties.sum(axis=0) > 20).all()
    for squared in (False, True):
        want = ref.matrix(src, tgt, squared)
        assert np.isfinite(want).sum() > 40
        with Sets(src, tgt, 1, squared=squared) as sets:
            same_as_align(check_matrix(sets, want), align_costs(sets)[0])
            check_match(sets, want)


# -- features that are not finite ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,value,squared", nonfinite_cases.VALUES, ids=["%s-%s" % (n, "squared" if sq else "rooted")
                                                                           for n, _, sq in nonfinite_cases.VALUES])
def test_features_that_are_not_finite(name, value, squared):
    """The value in a source's first, middle or last frame (sources that share a pack with clean ones, and one of 70 frames
    at rows 0, 64 and 69) and in a target's first, middle or last frame, in the frame's last element (next to the padding)."""
    rng = np.random.default_rng(0xBAD)
    u = real(rng, 20, DIM)
    clean = [u + real(rng, 20, DIM, 0.01), real(rng, 12, DIM), real(rng, 27, DIM)]
    long_ = real(rng, 70, DIM)
    src, poisoned = [], []
    for place in (0, 9, 19):
        s = u + real(rng, 20, DIM, 0.001)                  # closer to u than any clean source: it would win
        s[place, DIM - 1] = value
        src += [clean[len(src) // 2 % 3], s]
        poisoned.append(len(src) - 1)
    for place in (0, 64, 69):
        s = long_.copy()
        s[place, DIM - 1] = value
        src.append(s)
        poisoned.append(len(src) - 1)
    src += clean + [long_]
    tgt = [u, real(rng, 40, DIM)]
    for place in (0, 9, 19):
        t = u.copy()
        t[place, DIM - 1] = value
        tgt.append(t)
    want = ref.matrix(src, tgt, squared)
    with Sets(src, tgt, DIM, squared=squared) as sets:
        mat = check_matrix(sets, want)
        acost, alen = align_costs(sets)
        same_as_align(mat, acost)
        assert ((alen > 0) == np.isfinite(mat)).all()
        idx, cost = check_match(sets, want)
        keep = [k for k in range(len(src)) if k not in poisoned]
        # a pair with a cost that is not finite never wins; the clean neighbours in the same packs are what they are alone
        assert np.isfinite(cost[:2]).all() and not np.isfinite(want[poisoned[0], 0]) and not np.isfinite(want[poisoned[2], 0])
        for t in range(len(tgt)):
            assert np.isfinite(want[idx[t], t]) or (idx[t] == 0 and cost[t] == INF), t
            if t >= 2:                                 # a value that is not finite in a target frame is on every path
                assert not np.isfinite(want[keep, t]).any()      # (a source with the same value in the same place may cancel it)
    alone = [src[k] for k in keep]
    with Sets(alone, tgt, DIM, squared=squared) as sets:
        rc, mat2, _ = matrix(sets)
        assert rc == nat.SSYM_OK and same_bits(mat2, mat[keep])


# -- the symmetric step ---------------------------------------------------------------------------------------------------
def test_the_symmetric_step_is_the_existing_calls(ragged):
    for dtype in ("f64", "f32"):
        with Sets(ragged.src, ragged.tgt, DIM, dtype) as sets:
            n, m = len(ragged.src), len(ragged.tgt)
            for dist, base, flags in ((None, 0, 0), (ragged.distance, 5, 0), (None, 0, nat.DTW_FORCE_EXACT)):
                rc, idx, cost, untouched = match(sets, dist, base, step=SYMMETRIC, flags=flags)
                route = sets.e.timings()["used_filter"]
                assert rc == nat.SSYM_OK and untouched, error(sets)
                widx, wcost = sets.e.match(sets.d, sets.q, dist, index_base=base, force_exact=bool(flags))
                assert route == sets.e.timings()["used_filter"]
                assert np.array_equal(idx, widx) and (bits(cost) == bits(wcost)).all()
            rc, mat, untouched = matrix(sets, SYMMETRIC)
            assert rc == nat.SSYM_OK and untouched
            assert (bits(mat) == bits(sets.e.pair_matrix(sets.d, sets.q, exact=True))).all()
            assert (bits(sets.e.pair_matrix(sets.d, sets.q, step="paced")) == bits(matrix(sets)[1])).all()


# -- history ----------------------------------------------------------------------------------------------------------------
def test_the_same_bits_whatever_the_context_ran_before(ragged):
    dist = ragged.distance
    with Sets(ragged.src, ragged.tgt, DIM) as sets:
        fresh = match(sets, dist, 3)[1:3] + (matrix(sets)[1],)
    with Sets(ragged.src, ragged.tgt, DIM) as sets:
        rng = np.random.default_rng(0x415)
        # other sets on the SAME engine first, all NaN
        other_src = [np.full((f, DIM), NAN) for f in (64, 50, 7)]
        other_tgt = [np.full((f, DIM), NAN) for f in rng.integers(5, 60, size=20)]
        d2 = sets.e.dictionary(*pack_segments(other_src, DIM, np.float64), DIM)
        q2 = sets.e.queries(*pack_segments(other_tgt, DIM, np.float64), DIM)
        sets.e.match(d2, q2, np.full(20, NAN))
        sets.e.match(d2, q2, np.full(20, NAN), step="paced")
        sets.e.pair_matrix(d2, q2, step="paced")
        sets.e.match(sets.d, sets.q)                                        # a symmetric match
        sets.e.dtw_spot(sets.d, sets.q, np.arange(9, dtype=np.uint32))      # a spot
        sets.e.dtw_align(sets.d, sets.q, np.arange(9, dtype=np.uint32), step="paced")      # an align
        q2.close()
        d2.close()
        again = match(sets, dist, 3)[1:3] + (matrix(sets)[1],)
    for a, b in zip(fresh, again):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert same_bits(fresh[2], ragged.want[False])


# -- refusals ---------------------------------------------------------------------------------------------------------------
CALLS = {"ssym_match_queries_step": lambda sets, **kw: match(sets, **kw)[0::3],
         "ssym_pair_matrix_step": lambda sets, **kw: matrix(sets, **kw)[0::2]}


@pytest.mark.parametrize("fn", sorted(CALLS))
def test_every_refusal_names_its_entry_point(fn):
    call = CALLS[fn]
    small = [np.zeros((4, 2)), np.zeros((3, 2))]
    with Sets(small, small, 2) as sets:
        assert call(sets, step=7) == (nat.SSYM_E_INVALID, True)
        assert error(sets) == fn + ": step must be SSYM_STEP_SYMMETRIC or SSYM_STEP_PACED"
        assert call(sets) == (nat.SSYM_OK, True)
    with Sets(small, small, 2, band=3) as sets:
        assert call(sets) == (nat.SSYM_E_UNSUPPORTED, True)
        assert error(sets).startswith(fn + ": the paced step pattern bounds the slope itself")
        assert call(sets, step=SYMMETRIC)[0] == nat.SSYM_OK           # the band is the symmetric search's
    with Sets(small, small, 2, metric="refcos") as sets:
        assert call(sets) == (nat.SSYM_E_UNSUPPORTED, True)
        assert error(sets) == fn + ": the context's metric is refcos, which has no step pattern"
        with pytest.raises(SsymError) as err:
            sets.e.match(sets.d, sets.q, step="paced") if fn.startswith("ssym_match") else sets.e.pair_matrix(sets.d, sets.q, step="paced")
        assert err.value.code == nat.SSYM_E_UNSUPPORTED
    with Sets([], small, 2) as sets:
        assert call(sets) == (nat.SSYM_E_EMPTY_DICT, True)
        assert error(sets) == fn + ": empty dictionary"
    limit = fn + ": a source has more than 4096 frames, a target more than 2048, or frames have more than 64 values"
    with Sets(small, small + [np.zeros((2049, 2))], 2) as sets:
        assert call(sets) == (nat.SSYM_E_UNSUPPORTED, True)
        assert error(sets).startswith(limit)
    with Sets(small + [np.zeros((4097, 2))], small, 2) as sets:
        assert call(sets) == (nat.SSYM_E_UNSUPPORTED, True)
        assert error(sets).startswith(limit)
    wide = [np.zeros((3, 65))]
    with Sets(wide, wide, 65) as sets:
        assert call(sets) == (nat.SSYM_E_UNSUPPORTED, True)
        assert error(sets).startswith(limit)
    with Sets(small, small, 2) as sets:
        L = nat.lib()
        assert L.ssym_pair_matrix_step(sets.e.ctx, sets.d.ptr, sets.q.ptr, PACED, None) == nat.SSYM_E_INVALID
        assert error(sets) == "ssym_pair_matrix_step: out_matrix is NULL"
        assert L.ssym_match_queries_step(sets.e.ctx, sets.d.ptr, sets.q.ptr, None, 0, PACED, None, None, 0) == nat.SSYM_E_INVALID
        assert error(sets) == "ssym_match_queries_step: out_idx is NULL"
        assert L.ssym_match_queries_step(sets.e.ctx, None, sets.q.ptr, None, 0, PACED, None, None, 0) == nat.SSYM_E_INVALID
        assert error(sets) == "ssym_match_queries_step: dictionary or queries handle is NULL"
    with Sets(small, [], 2) as sets:                                    # no targets: nothing to do, nothing written
        assert call(sets) == (nat.SSYM_OK, True)
