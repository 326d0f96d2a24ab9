"""ssym_dtw_cover on the GPU held to tests/cover_ref.py bit for bit (DESIGN.md section 2 "Cover", section 5.23): counts,
totals, all four piece arrays and the padding of the unused slots, on both engine dtypes and with the squared option; every
piece's cost against the library's own paced matrix and paced alignment of the cut; ragged targets in one call; features
that are not finite; penalties; reconstruct_covered against the hand-made warp route; every refusal."""
import numpy as np
import pytest

import cover_ref as ref
from cover_gpu import INF, SENT32, SENTF, Sets, bits, call, check, error, pieces_of, real, same  # noqa: F401
from soundsym_amd import HOP, Cover, Engine, Sound, SoundDictionary, SoundSequence, SsymError
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def planted():
    """The planted case and its noisy twin with their restatements, computed once."""
    class P:
        pass
    p = P()
    p.segs, p.target, p.pieces = ref.planted_case()
    _, p.noisy, _ = ref.planted_case(noise=1e-3)
    p.want = {(sq, k): ref.arrays(p.segs, [x], 0.0, sq) for sq in (False, True) for k, x in (("exact", p.target), ("noisy", p.noisy))}
    return p


@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_planted_case_and_its_noisy_twin(planted, dtype, squared):
    for kind, x in (("exact", planted.target), ("noisy", planted.noisy)):
        with Sets(planted.segs, [x], 13, dtype, squared) as sets:
            got = check(sets, want=planted.want[squared, kind])
            assert [(s, a, e) for s, a, e, _ in pieces_of(got, [x], 0)] == planted.pieces
            if kind == "exact":
                assert bits(got[1][0]) == bits(0.0) and (bits(got[5][:got[0][0]]) == bits(0.0)).all()
            check(sets, want=planted.want[squared, kind], device=True)


@pytest.fixture(scope="module")
def ragged():
    """A ragged dictionary and several ragged targets, an empty one among them, with the restatement's tables."""
    class R:
        pass
    r = R()
    rng = np.random.default_rng(0xC07E)
    r.src = [real(rng, n, 13) for n in (5, 40, 12, 0, 33, 7, 21, 1, 17, 2, 29, 9)]
    r.tgt = [real(rng, n, 13) for n in (70, 0, 1, 33, 130, 9)]
    r.tabs = {sq: ref.all_tables(r.src, r.tgt, sq) for sq in (False, True)}
    return r


@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ragged_targets_in_one_call_and_one_call_each(ragged, dtype, squared):
    want = ref.arrays(ragged.src, ragged.tgt, 0.0, squared, tabs=ragged.tabs[squared])
    with Sets(ragged.src, ragged.tgt, 13, dtype, squared) as sets:
        got = check(sets, want=want)
        assert got[0][1] == 0 and got[1][1] == INF and got[0][4] > 3
        check(sets, want=want, device=True)
    if dtype == "f64":
        off = np.concatenate([[0], np.cumsum([x.shape[0] for x in ragged.tgt])])
        for t, x in enumerate(ragged.tgt):
            with Sets(ragged.src, [x], 13, dtype, squared) as one:
                rc, alone, untouched = call(one)
                assert rc == nat.SSYM_OK and untouched
                same(alone, [w[t:t + 1] if k < 2 else w[off[t]:off[t + 1]] for k, w in enumerate(want)])


@pytest.mark.parametrize("squared", [False, True])
def test_every_piece_costs_what_the_paced_matrix_and_alignment_give_the_cut(ragged, squared):
    """Consequence 2 through the library itself: the cut goes straight into pair_matrix(step="paced") and align(step="paced")."""
    want = ref.arrays(ragged.src, ragged.tgt, 0.0, squared, tabs=ragged.tabs[squared])
    with Sets(ragged.src, ragged.tgt, 13, "f64", squared) as sets:
        got = check(sets, want=want)
    pieces = [(t, p) for t in range(len(ragged.tgt)) for p in pieces_of(got, ragged.tgt, t)]
    assert len(pieces) > 10
    cuts = [ragged.tgt[t][a:e + 1] for t, (_, a, e, _) in pieces]
    with Sets(ragged.src, cuts, 13, "f64", squared) as sets:
        mat = sets.e.pair_matrix(sets.d, sets.q, step="paced")
        cost, length, _, _ = sets.e.dtw_align(sets.d, sets.q, np.array([p[0] for _, p in pieces], dtype=np.uint32), step="paced")
    for k, (t, (s, a, e, c)) in enumerate(pieces):
        assert bits(mat[s, k]) == bits(c) and bits(cost[k]) == bits(c) and length[k] == e - a + 1
        # ... and no source does better on that cut, the lower index on a tie
        col = mat[:, k]
        assert s == int(np.flatnonzero(col == np.nanmin(col))[0])
    # consequence 3: the total is the chain's own sum
    for t in range(len(ragged.tgt)):
        if got[0][t]:
            assert bits(ref.resum(pieces_of(got, ragged.tgt, t))) == bits(got[1][t])


@pytest.mark.parametrize("name,value", [("nan", np.nan), ("inf", np.inf), ("ninf", -np.inf)])
def test_features_that_are_not_finite(planted, name, value):
    rng = np.random.default_rng(6)
    x = real(rng, 40, 13)
    bad_target = x.copy()
    bad_target[17, 3] = value
    with Sets(planted.segs, [x, bad_target, x[:20]], 13) as sets:
        got = check(sets)
        assert got[0][1] == 0 and got[1][1] == INF and got[0][0] > 0 and got[0][2] > 0
    # a dictionary segment with such a frame is never chosen: the cover of the dictionary with that segment empty
    for n, row in ((0, 0), (3, 12), (9, 28), (6, 0)):
        broken = [s.copy() for s in planted.segs]
        broken[n][row, 5] = value
        emptied = [s if k != n else s[:0] for k, s in enumerate(planted.segs)]
        with Sets(broken, [x, planted.target], 13) as sets:
            got = check(sets)
            if name == "nan":                   # (a path may step over an infinite frame, never past a NaN: P keeps it)
                same(got, ref.arrays(emptied, [x, planted.target]))
                assert n not in got[2][:got[0][0]].tolist()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_penalties(planted, dtype):
    x = real(np.random.default_rng(40), 40, 13)
    tabs = ref.all_tables(planted.segs, [x, planted.noisy])
    counts = []
    with Sets(planted.segs, [x, planted.noisy], 13, dtype) as sets:
        for penalty in (0.0, 2.0, 20.0):
            got = check(sets, penalty, want=ref.arrays(planted.segs, [x, planted.noisy], penalty, tabs=tabs))
            assert bits(ref.resum(pieces_of(got, [x, planted.noisy], 0), penalty)) == bits(got[1][0])
            counts.append(int(got[0][0]))
    assert counts[0] > counts[1] > counts[2] >= 1


# -- reconstruct_covered -----------------------------------------------------------------------------------------------------

def _sound(rng, feats, extra=0):
    return Sound(rng.standard_normal(feats.shape[0] * HOP + extra), 16000.0, feats.reshape(-1), None, ncoeffs=feats.shape[1])


@pytest.mark.parametrize("search", [0, 64])
def test_reconstruct_covered_is_the_hand_made_warp_route(planted, search):
    rng = np.random.default_rng(0x5EED)
    d = SoundDictionary(engine=Engine(metric="dtw", dtype="f64"))
    d.sounds = [_sound(rng, s) for s in planted.segs]
    try:
        for feats, extra in ((planted.target, 100), (real(rng, 50, 13), 0)):
            target = _sound(rng, feats, extra)
            cover, samples, pcm = d.reconstruct_covered(target, search=search, want_pcm32=True)
            assert isinstance(cover, Cover) and cover and samples.size == target.samples().size == pcm.size
            want = ref.cover(planted.segs, feats)
            assert [(p.source_index, p.start_frame, p.end_frame) for p in cover.pieces] == [w[:3] for w in want[0]]
            assert bits(cover.total) == bits(want[1]) and (bits([p.cost for p in cover.pieces]) == bits([w[3] for w in want[0]])).all()
            assert d.cover([target])[0].indices().tolist() == cover.indices().tolist()
            # by hand: cut at the pieces, warp every cut from its sound under the paced pattern
            lens = cover.segment_lengths(target.samples().size)
            cuts, at = [], 0
            for p, n in zip(cover.pieces, lens):
                cuts.append(Sound(target.samples()[at:at + n], 16000.0, feats[p.start_frame:p.end_frame + 1].reshape(-1), None, 13))
                at += n
            by_hand = d.warp(cuts, indices=cover.indices(), step="paced", search=search)
            assert np.array_equal(samples, by_hand)
            seq = SoundSequence.from_cover(target, cover)
            assert np.array_equal(samples, d.warp(seq.sounds(), indices=cover.indices(), step="paced", search=search))
            if feats is planted.target:
                # the planted exact-copy target: what warp gives the true cut
                assert [(p.source_index, p.start_frame, p.end_frame) for p in cover.pieces] == planted.pieces
                true_cuts, at = [], 0
                for k, (s, a, e) in enumerate(planted.pieces):
                    n = (e - a + 1) * HOP if k + 1 < len(planted.pieces) else target.samples().size - a * HOP
                    true_cuts.append(Sound(target.samples()[at:at + n], 16000.0, feats[a:e + 1].reshape(-1), None, 13))
                    at += n
                true = d.warp(true_cuts, indices=[s for s, _, _ in planted.pieces], step="paced", search=search)
                assert np.array_equal(samples, true)
        # a target without a cover takes what reconstruct_from_dictionary gives it whole
        broken = planted.noisy[:30].copy()
        broken[4, 4] = np.nan
        target = _sound(rng, broken, 17)
        cover, samples = d.reconstruct_covered(target, search=search)
        assert not cover and cover.total == INF and samples.size == target.samples().size
        assert np.array_equal(samples, SoundSequence([target]).reconstruct_from_dictionary(d))
        assert d.cover([]) == []
    finally:
        d.engine.close()


# -- refusals ---------------------------------------------------------------------------------------------------------------

def test_every_refusal_by_code_and_message():
    fn = "ssym_dtw_cover"
    refused = lambda sets, **kw: call(sets, **kw)[0::2]
    small = [np.zeros((4, 2)), np.zeros((3, 2))]
    with Sets(small, small, 2) as sets:
        for bad in (-1.0, float("nan"), INF, -INF):
            assert refused(sets, penalty=bad) == (nat.SSYM_E_INVALID, True)
            assert error(sets) == fn + ": piece_penalty must be finite and not negative"
        assert refused(sets) == (nat.SSYM_OK, True)
        L = nat.lib()
        u, f = np.zeros(8, dtype=np.uint32), np.zeros(8)
        outs = [u.ctypes.data, f.ctypes.data, u.ctypes.data, u.ctypes.data, u.ctypes.data, f.ctypes.data]
        for k in range(6):
            args = list(outs)
            args[k] = None
            assert L.ssym_dtw_cover(sets.e.ctx, sets.d.ptr, sets.q.ptr, 0.0, 0, *args) == nat.SSYM_E_INVALID
            assert error(sets) == fn + ": out_count, out_total, out_src, out_start, out_end and out_cost must not be NULL"
        assert L.ssym_dtw_cover(sets.e.ctx, None, sets.q.ptr, 0.0, 0, *outs) == nat.SSYM_E_INVALID
        assert error(sets) == fn + ": dictionary or queries handle is NULL"
        assert not u.any() and not f.any()
    with Sets(small, small, 2, band=3) as sets:
        assert refused(sets) == (nat.SSYM_E_UNSUPPORTED, True)
        assert error(sets).startswith(fn + ": the paced step pattern bounds the slope itself")
    with Sets(small, small, 2, metric="refcos") as sets:
        assert refused(sets) == (nat.SSYM_E_UNSUPPORTED, True)
        assert error(sets) == fn + ": the context's metric is refcos, which has no alignment to cover with"
        with pytest.raises(SsymError) as err:
            sets.e.dtw_cover(sets.d, sets.q)
        assert err.value.code == nat.SSYM_E_UNSUPPORTED
    with Sets([], small, 2) as sets:
        assert refused(sets) == (nat.SSYM_E_EMPTY_DICT, True)
        assert error(sets) == fn + ": empty dictionary"
    limit = fn + ": a dictionary segment has more than 128 frames, or frames have more than 64 values"
    with Sets(small + [np.zeros((129, 2))], small, 2) as sets:
        assert refused(sets) == (nat.SSYM_E_UNSUPPORTED, True)
        assert error(sets) == limit
    wide = [np.zeros((3, 65))]
    with Sets(wide, wide, 65) as sets:
        assert refused(sets) == (nat.SSYM_E_UNSUPPORTED, True)
        assert error(sets) == limit
    # the tables of one source block and the back-pointers: frames x 2 Fmax x 12 + frames x 16 bytes <= 512 MiB
    frames = (512 << 20) // (2 * 128 * 12 + 16) + 1
    with Sets([np.zeros((128, 1))], [np.zeros((frames, 1))], 1) as sets:
        assert refused(sets) == (nat.SSYM_E_UNSUPPORTED, True)
        assert error(sets).startswith(fn + ": the tables need frames x 2 Fmax x 12 + frames x 16 bytes, more than 512 MiB")
    with Sets(small, [], 2) as sets:                                    # no targets: nothing to do, nothing written
        assert refused(sets) == (nat.SSYM_OK, True)
        assert refused(sets, penalty=-1.0) == (nat.SSYM_E_INVALID, True)
    with Sets(small, [np.zeros((0, 2))], 2) as sets:                    # a target without frames: no cover, no slots
        rc, got, untouched = call(sets)
        assert rc == nat.SSYM_OK and untouched and got[0].tolist() == [0] and got[1].tolist() == [INF]
