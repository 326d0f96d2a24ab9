"""tests/mirror_cases.py on the CPU: the container's round trip, and that the case set holds every edge it is there for --
each of them read off the restatements (paced_path_ref, spot_ref, paced_ref, spot_all_ref, dtw_path_ref, watch_ref), so that
no edge of tests/test_gpu_mirror_dtw.py is there in name only."""
import numpy as np
import pytest

import dtw_path_ref
import mirror_cases as mc
import paced_path_ref
import paced_ref
import spot_all_ref
import spot_ref

NO = mc.NO_MATCH
HOP = mc.HOP


@pytest.fixture(scope="module")
def cases():
    return mc.build()


def _written(tmp_path, raw):
    path = str(tmp_path / "raw.bin")
    with open(path, "wb") as f:
        f.write(raw)
    return path


def test_the_container_round_trip(tmp_path):
    arrays = {
        "f": np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, 1.0 / 3.0]),
        "u32": np.array([0, 1, 0xFFFFFFFF], dtype=np.uint32),
        "u64": np.array([0, 1 << 40, (1 << 64) - 1], dtype=np.uint64),
        "empty.f": np.zeros(0), "empty.u32": np.zeros(0, dtype=np.uint32), "empty.u64": np.zeros(0, dtype=np.uint64),
        "n" * mc.MAX_NAME: np.arange(3, dtype=np.uint32),
        "big-endian": np.arange(4, dtype=">u4"),
        "matrix": np.arange(6.0).reshape(2, 3),
    }
    path = str(tmp_path / "a.bin")
    mc.write_arrays(path, arrays)
    back = mc.read_arrays(path)
    assert list(back) == list(arrays)
    for name, a in arrays.items():
        b = back[name]
        assert b.ndim == 1 and b.size == a.size and b.dtype == a.dtype.newbyteorder("="), name
        if a.dtype.kind == "f":
            assert np.array_equal(b.view(np.uint64), a.reshape(-1).view(np.uint64)), name      # bits, NaN and -0.0 included
        else:
            assert np.array_equal(b, a.reshape(-1)), name
    raw = open(path, "rb").read()
    assert raw[:8] == b"SSYMARR1" and raw[8:12] == (len(arrays)).to_bytes(4, "little")
    assert raw[12] == 1 and raw[13:14] == b"f" and raw[14] == 0 and raw[15:23] == (7).to_bytes(8, "little")
    for bad in ({"": np.zeros(1)}, {"n" * 256: np.zeros(1)}, {"i": np.zeros(1, dtype=np.int32)}, {"h": np.zeros(1, np.float32)}):
        with pytest.raises(ValueError):
            mc.write_arrays(str(tmp_path / "bad.bin"), bad)
    first = raw[12:12 + 1 + 1 + 9 + 7 * 8]                                                      # the entry "f"
    twice = raw[:8] + (2).to_bytes(4, "little") + first + first
    assert list(mc.read_arrays(_written(tmp_path, raw[:8] + (1).to_bytes(4, "little") + first))) == ["f"]
    for cut in (raw[:-1], raw + b"\0", b"SSYMARR2" + raw[8:], twice):
        open(str(tmp_path / "cut.bin"), "wb").write(cut)
        with pytest.raises(ValueError):
            mc.read_arrays(str(tmp_path / "cut.bin"))


def test_the_cases_are_a_function_of_the_seed(cases):
    a, b, c = cases.arrays(), mc.build().arrays(), mc.build(mc.SEED + 1).arrays()
    assert list(a) == list(b) == list(c)
    assert all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)
    assert not np.array_equal(a["rec0.mfccs"], c["rec0.mfccs"])
    assert all(v.dtype in (np.float64, np.uint32, np.uint64) for v in a.values()) and max(map(len, a)) <= mc.MAX_NAME


def test_shapes_and_sample_counts(cases):
    frames = lambda sounds: tuple(f.shape[0] for _, f in sounds)
    samples = lambda sounds: tuple(s.size for s, _ in sounds)
    assert frames(cases.recs) == (300, 70, 1, 40, 40) and frames(cases.tgts) == (1, 2, 8, 33, 65, 0)
    assert frames(cases.segs) == (4, 17, 33, 66, 130, 0)
    assert all(f.shape[1] == mc.NCOEFFS for _, f in cases.recs + cases.tgts + cases.segs + cases.repl)
    # recordings: what analysis would leave, one that ends inside its last frame, and exact ones
    assert samples(cases.recs) == (300 * HOP + 768, 70 * HOP - 100, HOP, 40 * HOP, 40 * HOP)
    assert np.array_equal(cases.recs[3][1], cases.recs[4][1]) and np.array_equal(cases.recs[3][0], cases.recs[4][0])
    # targets: whole frames, a single sample, none
    assert samples(cases.tgts) == (HOP, 1, 8 * HOP, 33 * HOP, 65 * HOP, 0)
    assert samples(cases.segs)[5] > 0                          # the frameless segment's length fit copies something
    assert frames(cases.repl) == (300, 33) and samples(cases.repl) == (samples(cases.recs)[0], samples(cases.segs)[2])
    # the spans by hand end on the last frame of a recording of each kind; the short one takes the clamp, the long one not
    kinds = {}
    for r, a, b in mc.HAND:
        if r != NO and b == mc.REC_FRAMES[r] - 1:
            size = mc.REC_SAMPLES[r]
            kinds[np.sign(size - mc.REC_FRAMES[r] * HOP)] = ((b + 1) * HOP > size)
    assert kinds == {1: False, 0: False, -1: True}
    assert sum(r == NO for r, _, _ in mc.HAND) == 1 and len(mc.HAND) == len(cases.tgts)
    # the push schedules feed every recording whole, in blocks around the 64-row chunk, with empty pushes
    for lanes in (1, 3):
        recs, pushes = mc.spotter_lanes(lanes)
        assert [sum(row[l] for row in pushes) for l in range(lanes)] == [mc.REC_FRAMES[r] for r in recs]
        assert {0, 1, 63, 64, 65} <= {row[0] for row in pushes}
    assert any(row[1] == 0 and row[0] > 0 for row in mc.PUSH3)
    assert [sum(row[l] for row in mc.FOLLOW) for l in range(2)] == list(mc.REC_SAMPLES[:2])


def test_the_paced_shape_rule_splits_the_segments(cases):
    ok = [paced_path_ref.feasible(f, 33) for f in mc.SEG_FRAMES]
    assert ok == [False, True, True, False, False, False]
    assert not any(paced_path_ref.feasible(f, 0) for f in mc.SEG_FRAMES)        # the frameless target fits nothing
    # the matrix of pair_matrix_step (6 segments x targets 1 ... 5): 2 frames take 1 ... 3, 8 take 4 ... 15, 33 take 17 ... 65,
    # 65 take 33 ... 129 -- finite and infinite entries in no pattern a transposed or shifted read would keep
    fits = np.array([[paced_path_ref.feasible(f, t) for t in mc.TGT_FRAMES[1:]] for f in mc.SEG_FRAMES])
    assert fits.shape == (6, 5) and not fits[5].any() and not fits[:, 4].any()
    assert [int(x) for x in fits.sum(axis=0)] == [0, 1, 2, 2, 0] and [int(x) for x in fits.sum(axis=1)] == [1, 1, 2, 1, 0, 0]


def test_align_and_warp_get_pairs_with_and_without_a_finite_cost(cases):
    for which, idx in mc.INDICES.items():
        sym = [dtw_path_ref.align(cases.segs[s][1], cases.tgts[t][1])[0] for t, s in enumerate(idx)]
        paced = [paced_path_ref.align(cases.segs[s][1], cases.tgts[t][1])[0] for t, s in enumerate(idx)]
        assert np.isfinite(sym).tolist() == [mc.SEG_FRAMES[s] > 0 and mc.TGT_FRAMES[t] > 0 for t, s in enumerate(idx)]
        assert np.isfinite(paced).tolist() == [paced_path_ref.feasible(mc.SEG_FRAMES[s], mc.TGT_FRAMES[t]) for t, s in enumerate(idx)]
        assert np.isinf(sym).any() and np.isfinite(sym).sum() >= 4
    finite = lambda which: [paced_path_ref.feasible(mc.SEG_FRAMES[s], mc.TGT_FRAMES[t]) for t, s in enumerate(mc.INDICES[which])]
    assert finite("a") == [False, False, False, True, False, False]               # 33 on 33; 130 is too long for 65
    assert finite("b") == [False, False, True, True, True, False]                 # 4 for 8 and 17 for 33: the shortest
    # a symmetric path has Fa + Fb - 1 cells at most and Fb map entries: the two offset arrays differ from the first pair on
    _, path, fmap = dtw_path_ref.align(cases.segs[0][1], cases.tgts[0][1])
    assert path.shape[0] == 4 and fmap.size == 1 and (path[:, 0] != path[:, 1]).any()


def test_spots_are_found_where_they_were_planted(cases):
    feats = [f for _, f in cases.recs]
    for ref in (spot_ref, paced_ref):
        b3, b4 = ref.spot_best(feats, cases.tgts[3][1]), ref.spot_best(feats, cases.tgts[4][1])
        assert (b3[0], b3[2], b3[3]) == (0, mc.PLANT33, mc.PLANT33 + 32) and (b4[0], b4[2], b4[3]) == (0, mc.PLANT65, mc.PLANT65 + 64)
        b2 = ref.spot_best(feats, cases.tgts[2][1])
        assert b2 == (3, 0.0, mc.PLANT8[0], mc.PLANT8[0] + 7)                       # the lower of the two equal recordings
        assert ref.spot_best(feats, cases.tgts[5][1]) == (NO, np.inf, NO, NO)      # no frames: no spot
        far = ref.spot_best(feats, cases.tgts[1][1])
        assert far[0] != NO and far[1] > 100.0                                      # far from everything, and still a spot
        moved = ref.spot_best([cases.repl[0][1]] + feats[1:], cases.tgts[3][1])
        assert (moved[0], moved[2], moved[3]) == (0, mc.MOVED33, mc.MOVED33 + 32)   # case k
    # with indices: 33 frames inside the one-frame recording have a symmetric spot and no paced one
    r, t = mc.SPOT_INDICES[3], 3
    assert spot_ref.spot(feats[r], cases.tgts[t][1])[1:] == (0, 0) and paced_ref.spot(feats[r], cases.tgts[t][1]) == (np.inf, NO, NO)
    for t, r in enumerate(mc.SPOT_INDICES[:5]):
        assert spot_ref.spot(feats[r], cases.tgts[t][1])[2] != NO
    # case k's other half: segment 2 replaced by target 3 itself aligns on the diagonal at cost zero
    cost, path, _ = dtw_path_ref.align(cases.repl[1][1], cases.tgts[3][1])
    assert cost == 0.0 and np.array_equal(path[:, 0], path[:, 1])
    assert dtw_path_ref.align(cases.segs[2][1], cases.tgts[3][1])[0] > 1.0


def _merged(cases, t, k, limit=None, ref=spot_all_ref):
    out = []
    for r, (_, f) in enumerate(cases.recs):
        count, cost, start, end = ref.spot_all(f, cases.tgts[t][1], k, limit)
        out += [(float(cost[m]), r, int(end[m]), int(start[m])) for m in range(count)]
    return sorted(out)


def test_spot_all_has_its_tie_and_its_threshold_bites(cases):
    for ref in (spot_all_ref, paced_ref):
        got = _merged(cases, 2, 8, None, ref)
        ends = [p + 7 for p in mc.PLANT8]
        assert [g[:3] for g in got[:4]] == [(0.0, 3, ends[0]), (0.0, 3, ends[1]), (0.0, 4, ends[0]), (0.0, 4, ends[1])]
        # ... an order that (cost, end frame) alone does not give
        assert sorted(got[:4], key=lambda g: (g[0], g[2])) != got[:4]
    # max_spots 1, 8 and 64 give lists of different lengths; 64 is reached by the one-frame target in the long recording
    assert spot_all_ref.spot_all(cases.recs[0][1], cases.tgts[0][1], 64)[0] == 64
    assert [len(_merged(cases, 3, k)) for k in (1, 8, 64)] == sorted({len(_merged(cases, 3, k)) for k in (1, 8, 64)})
    limit = float(cases.args["spot_all.max_cost"][0])
    free = [len(_merged(cases, t, 8)) for t in range(6)]
    cut = [len(_merged(cases, t, 8, limit)) for t in range(6)]
    assert free[5] == 0 and all(f > 0 for f in free[:5])
    assert cut[1] == 0 and cut[3] == 1 and cut[4] == 1 and 0 < cut[2] < free[2] and cut[0] > 1      # emptied, cut short, kept


@pytest.mark.parametrize("step", ["symmetric", "paced"])
@pytest.mark.parametrize("lanes", [1, 3])
def test_the_spotter_cases_emit_events_in_pushes_and_flushes(cases, lanes, step):
    free = mc.expected_events(cases, lanes, step)
    cut = mc.expected_events(cases, lanes, step, cases.args["spotter.max_cost"])
    n = lambda ev: sum(len(x) for x in ev[0]) + sum(len(x) for x in ev[2])
    assert n(cut) < n(free) and sum(len(x) for x in cut[0]) > 0
    assert sum(len(x) for x in free[0]) > 0 and sum(len(x) for x in free[2]) > 0          # in pushes and at the flush
    assert any(len({e[:2] for e in x}) > 1 for x in free[0])                              # several (lane, target) in one push
    assert any(e[0] != e[1] for x in free[0] for e in x)                                  # a lane is not its target
    # the planted copies are reported where they lie, and the best differs from lane to lane
    got = {(e[0], e[1], e[3], e[4]) for x in cut[0] + cut[2] for e in x}
    assert (0, 3, mc.PLANT33, mc.PLANT33 + 32) in got and (0, 4, mc.PLANT65, mc.PLANT65 + 64) in got
    last = free[1][-1]
    assert last[0][5] == (np.inf, NO, NO) and all(last[0][t][2] != NO for t in range(5))
    if lanes == 3:
        assert last[2][2] == (0.0, mc.PLANT8[0], mc.PLANT8[0] + 7) and last[0][2] != last[2][2]
