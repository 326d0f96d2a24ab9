"""No call's result depends on what its context ran before ("What a context carries between calls").

Every probe of tests/history_cases.py -- one call family at the smallest shape at which its routes still differ -- runs on
a fresh context and on contexts made dirty through the public API: by its hostile twin (the same size classes, so every
block the probe allocates comes out of the cache and was last written with NaN, +inf, 1e300 or a flood of ties under
other lengths), by the same calls three times as large, by the other route of the same family, by refused calls and a
begun step that is never finished, on handles that are not new, and in a gauntlet of all families on one context, in
both orders.  The dirty answer must be the fresh answer bit for bit (np.array_equal with equal_nan), and where
Engine.timings() names the route, the route must be the same.

That demand is what fresh against fresh shows: test_two_fresh_contexts_agree_bit_for_bit runs every probe on two new
contexts.  The fresh answer itself is held once to the reference of its family's own test (the CPU oracle and the numpy
restatements under tests/), so that the comparison is not one of two wrong answers."""
import numpy as np
import pytest

import dtw_path_ref
import history_cases as hc
import paced_path_ref
import paced_ref
import paced_watch_ref
import partition_ref
import pitch_ref
import spot_all_ref
import spot_ref
import tail_ref
import topk_ref
import warp_ref
import watch_ref
import wsola_ref
from soundsym_amd import Engine
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu

PROBES = sorted(hc.PROBES)
EXACT_RTOL = 1e-12                       # dtw costs against the oracle (tests/test_gpu_distance_routes.py)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def assert_same_outputs(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        if not same(g, w):
            g, w = np.asarray(g), np.asarray(w)
            where = np.argwhere(~((g == w) | ((g != g) & (w != w)))) if g.shape == w.shape else None
            first = tuple(where[0]) if where is not None and len(where) else None
            raise AssertionError("%s: output %d differs from the fresh context's%s" % (
                what, k, "" if first is None else " first at %s: %r against %r (%d entries differ)" % (
                    first, g[first], w[first], len(where))))


class Fresh:
    """Every probe's answer on a context that has done nothing else, computed once."""

    def __init__(self):
        self.known = {}

    def __call__(self, name):
        if name not in self.known:
            e = hc.new_engine(hc.PROBES[name].ctx)
            try:
                self.known[name] = hc.PROBES[name].run(e)
            finally:
                e.close()
        return self.known[name]


@pytest.fixture(scope="module")
def fresh():
    return Fresh()


def run_dirty(probe, prelude, fresh, what):
    want, want_route = fresh(probe.name)
    e = hc.new_engine(probe.ctx)
    try:
        prelude(e)
        got, route = probe.run(e)
    finally:
        e.close()
    assert route == want_route, (what, route, want_route)
    assert_same_outputs(got, want, what)


# -- fresh against fresh, and fresh against the references ------------------------------------------------------------
@pytest.mark.parametrize("name", PROBES)
def test_two_fresh_contexts_agree_bit_for_bit(fresh, name):
    probe = hc.PROBES[name]
    want, want_route = fresh(name)
    e = hc.new_engine(probe.ctx)
    try:
        got, route = probe.run(e)
    finally:
        e.close()
    assert route == want_route
    assert_same_outputs(got, want, name + " on a second fresh context")


def _matrix(oracle, probe, D, src=None):
    sf, so = hc.pack_segments(src if src is not None else D["src"], D.dim)
    tf, to = D.flat("tgt")
    if probe.ctx["metric"] == "refcos":
        return oracle.refcos_matrix(sf, so, tf, to, D.dim)
    return oracle.dtw_match_all(sf, so, tf, to, D.dim, band=probe.ctx.get("band", -1), nthreads=oracle.max_threads(),
                                want_matrix=True)[2]


def _rows(probe, mat, k, idx, val, dist=None, base=0):
    """The library's rows against tests/topk_ref.py on the oracle's matrix: refcos bit for bit, dtw indices equal and
    costs within 1e-12 relative."""
    refcos = probe.ctx["metric"] == "refcos"
    want_idx, want_val = topk_ref.rows(mat, k, dist, index_base=base, **(topk_ref.REFCOS if refcos else topk_ref.DTW))
    idx, val = np.asarray(idx).reshape(mat.shape[1], k), np.asarray(val).reshape(mat.shape[1], k)
    if k == 1:
        assert np.array_equal(idx.astype(np.int64), want_idx)
        if refcos:
            assert np.array_equal(val, want_val)
        else:
            with np.errstate(invalid="ignore"):
                assert ((val == want_val) | (np.abs(val - want_val) <= EXACT_RTOL * np.abs(want_val))).all()
    else:
        topk_ref.check_rows(idx, val, want_idx, want_val, rtol=0.0 if refcos else EXACT_RTOL)


def _distances(probe, m):
    dtw = probe.ctx["metric"] == "dtw"
    return hc._edge_distances(m, 0.0, 60.0 if dtw else 1.2, 1e6 if dtw else 1e301)


def check_search(oracle, probe, D, out):
    _rows(probe, _matrix(oracle, probe, D), 1, out[0], out[1])


def check_distances(oracle, probe, D, out):
    mat = _matrix(oracle, probe, D)
    _rows(probe, mat, 1, out[0], out[1], _distances(probe, mat.shape[1]), 3)


def check_topk(k):
    return lambda oracle, probe, D, out: _rows(probe, _matrix(oracle, probe, D), k, out[0], out[1])


def check_match_one(oracle, probe, D, out):
    mat = _matrix(oracle, probe, D)
    dists = (0.0, 7.5) if probe.ctx["metric"] == "dtw" else (1.0, 0.4)
    for t, dist in enumerate(dists):
        _rows(probe, mat[:, t:t + 1], 1, out[2 * t], out[2 * t + 1], np.array([dist]))


def check_batches(counts, with_distance):
    def check(oracle, probe, D, out):
        mat = _matrix(oracle, probe, D)
        for k, c in enumerate(counts):
            dist = hc._edge_distances(c, 0.0, 60.0 if probe.ctx["metric"] == "dtw" else 1.2, 1e6) if with_distance else None
            _rows(probe, mat[:, :c], 1, out[2 * k], out[2 * k + 1], dist)
    return check


def check_pruned_step(oracle, probe, D, out):
    mat = _matrix(oracle, probe, D)
    _rows(probe, mat, 1, out[0], out[1], None, 2)
    _rows(probe, mat, 1, out[4], out[5])
    assert np.isfinite(out[3]).all() and (out[3] >= np.min(mat, axis=0) * (1 - EXACT_RTOL)).all()      # candidates: costs of real pairs


def check_begin_finish(oracle, probe, D, out):
    mat = _matrix(oracle, probe, D)
    _rows(probe, mat, 1, out[0], out[1], hc._edge_distances(mat.shape[1], 0.0, 60.0, 1e6), 1)


def check_chain(oracle, probe, D, out):
    metric = probe.ctx["metric"]
    sf, so = D.flat("src")
    want_idx, want_val = oracle.chain(sf, so, D.dim, D["start"][0].reshape(-1), hc.CHAIN_DISTANCES[metric], metric=metric)
    assert np.array_equal(out[0].astype(np.int64), want_idx)
    if metric == "refcos":
        assert np.array_equal(out[1], want_val)                  # the key |sim - distance|, bit for bit
    else:
        assert np.all(np.abs(out[1] - want_val) <= EXACT_RTOL * np.abs(want_val))


def check_pair_matrix(oracle, probe, D, out):
    mat = _matrix(oracle, probe, D)
    got = out[-1]
    if probe.ctx["metric"] == "refcos":
        assert np.array_equal(got, mat, equal_nan=True)
    else:
        fin = np.isfinite(mat)
        assert np.array_equal(np.isfinite(got), fin) and np.all(np.abs(got[fin] - mat[fin]) <= EXACT_RTOL * mat[fin])


def check_unholdable(oracle, probe, D, out):
    src = [s.copy() for s in D["src"]]
    src[5] *= 1e40
    src[9][0, 3] = np.nan
    _rows(probe, _matrix(oracle, probe, D, src), 1, out[0], out[1])


def check_align(step):
    def check(oracle, probe, D, out):
        cost, length, paths, maps = out
        at = mat = 0
        band = probe.ctx.get("band", -1)
        for p, (a, b) in enumerate(zip(D["src"], D["tgt"])):
            if step == "paced":
                want_cost, want_path, want_map = paced_path_ref.align(a, b)
            else:
                want_cost, want_path, want_map = dtw_path_ref.align(a, b, band=band)
            assert dtw_path_ref.same_floats(cost[p:p + 1], np.array([want_cost])), (p, cost[p], want_cost)
            assert length[p] == len(want_path)
            assert np.array_equal(paths[at:at + length[p]].astype(np.int64), want_path)
            at += int(length[p])
            assert np.array_equal(maps[mat:mat + len(want_map)].astype(np.int64), want_map)
            mat += len(want_map)
        assert at == len(paths) and mat == len(maps)
    return check


def check_spot(step):
    one = spot_ref.spot if step == "symmetric" else paced_ref.spot
    best = spot_ref.spot_best if step == "symmetric" else paced_ref.spot_best
    every = spot_all_ref.spot_all if step == "symmetric" else paced_ref.spot_all

    def check(oracle, probe, D, out):
        cost, start, end, qi, qc, qs, qe, count, ac, as_, ae = out
        src, tgt = hc._all_pairs(D)
        for p, (s, t) in enumerate(zip(src, tgt)):
            want = one(D["src"][s], D["tgt"][t])
            assert dtw_path_ref.same_floats(cost[p:p + 1], np.array([want[0]])) and (start[p], end[p]) == want[1:], (p, want)
        for t, b in enumerate(D["tgt"]):
            wi, wc, ws, we = best(D["src"], b)
            assert qi[t] == (wi + 4 if wi != spot_ref.NO_MATCH else wi) and (qs[t], qe[t]) == (ws, we)
            assert dtw_path_ref.same_floats(qc[t:t + 1], np.array([wc]))
        limit = hc.spot_limit(cost)
        some = 0
        for p, (s, t) in enumerate(zip(src, tgt)):
            wn, wc, ws, we = every(D["src"][s], D["tgt"][t], hc.SPOT_K, limit)
            assert count[p] == wn and dtw_path_ref.same_floats(ac[p], wc) and np.array_equal(as_[p], ws) and np.array_equal(ae[p], we)
            some += wn
        assert 0 < some < hc.SPOT_K * len(src)                 # the threshold admits some
    return check


def check_spotter(step):
    profile = watch_ref.whole_profile if step == "symmetric" else paced_watch_ref.whole_profile
    one = spot_ref.spot if step == "symmetric" else paced_ref.spot

    def check(oracle, probe, D, out):
        lanes, tgt = D["src"], D["tgt"]
        n_l, n_t = len(lanes), len(tgt)
        per_push = 1 + 2 * n_l + 5 + 3
        cuts = [hc.spotter_cuts(x.shape[0]) for x in lanes]
        for p in range(len(hc.SPOTTER_CUTS) - 1):
            block = out[p * per_push:(p + 1) * per_push]
            pd, ps = block[1:1 + n_l], block[1 + n_l:1 + 2 * n_l]
            for t in range(n_t):                                # lane 0 is never reset: its profile is the whole's
                d, s = profile(lanes[0], tgt[t])
                if d.size:
                    lo, hi = cuts[0][p], cuts[0][p + 1]
                    assert dtw_path_ref.same_floats(pd[0][t], d[lo:hi]) and np.array_equal(ps[0][t], s[lo:hi].astype(np.uint32))
                else:                                           # a target without frames: "no path" in every row
                    assert all((pd[l][t] == np.inf).all() and (ps[l][t] == nat.NO_MATCH).all() for l in range(n_l))
        cost, start, end = out[-3:]
        consumed = [lanes[0], lanes[1][cuts[1][hc.SPOTTER_RESET_AFTER + 1]:]]
        for l in range(n_l):
            for t in range(n_t):
                want = one(consumed[l], tgt[t])
                assert dtw_path_ref.same_floats(cost[l, t:t + 1], np.array([want[0]])) and (start[l, t], end[l, t]) == want[1:]
        counts = out[3 * per_push]
        assert counts.tolist() == [x.shape[0] for x in consumed]
    return check


def _mfcc_close(oracle, got, x, nc):
    from test_gpu_mfcc_shapes import assert_close, log_energies
    assert_close(got, oracle.mfcc(x, hc.RATE, nc), log_energies(x, hc.RATE, nc, 100.0, 8000.0), nc)


def check_mfcc(oracle, probe, D, out):
    for i, x in enumerate(D["snd"]):
        nc = (12, 40)[i % 2]
        _mfcc_close(oracle, out[2 * i], x, nc)
        assert np.allclose(out[2 * i + 1], np.mean(out[2 * i], axis=0), rtol=1e-12, atol=1e-12)


def check_mfcc_batch(oracle, probe, D, out):
    feats, fo, mean = out
    for i, x in enumerate(D["snd"]):
        frames = Engine.mfcc_num_frames(x.size)
        assert fo[i + 1] - fo[i] == frames
        if frames:
            _mfcc_close(oracle, feats[int(fo[i]):int(fo[i + 1])], x, 12)
        else:
            assert np.isnan(mean[i]).all()


def check_sequence(oracle, probe, D, out):
    from test_gpu_sequence import _check_distances, _mean_fold, _same_bits
    dist, mean, sim = out
    means = [_mean_fold(b, D.dim) for b in D["blk"]]
    assert all(_same_bits(mean[i], means[i]) for i in range(len(means)))
    _check_distances(dist, sim, means, oracle)


def check_descriptors(oracle, probe, D, out):
    mp, pc, mv, pv, freq, st, u, woff = out
    x, off = D.samples("snd")
    mp_r, pc_r, pv_r, tracks = pitch_ref.descriptors(x, off)
    assert np.array_equal(mp, mp_r) and np.array_equal(mv, mp_r)
    assert np.allclose(pc, pc_r, rtol=1e-11, atol=0) and np.allclose(pv, pv_r, rtol=1e-11, atol=0)
    assert list(np.diff(woff)) == [len(t["freq"]) for t in tracks]
    cat = {k: np.concatenate([t[k] for t in tracks]) for k in tracks[0]}
    assert np.allclose(u, cat["unvoiced"], rtol=1e-11, atol=0)
    clear = cat["gap"] > 1e-9
    assert np.allclose(freq[clear], cat["freq"][clear], rtol=1e-11, atol=0)
    assert np.allclose(st[clear], cat["strength"][clear], rtol=1e-11, atol=0)


def check_stream(oracle, probe, D, out):
    n_pushes, lanes = len(hc.STREAM_CUTS), D["snd"]
    at = 2 * n_pushes
    ns, nf = out[at], out[at + 1]
    assert ns.tolist() == [x.size for x in lanes]
    new = np.sum([out[2 * p] for p in range(n_pushes)], axis=0)
    assert np.array_equal(new, nf)
    for l, x in enumerate(lanes):
        _mfcc_close(oracle, out[at + 2 + l], x, 12)
    pushed = np.concatenate([out[2 * p + 1] for p in range(n_pushes)])
    assert pushed.shape[0] == int(nf.sum())
    mp, mean = out[at + 2 + len(lanes)], out[at + 3 + len(lanes)]
    assert np.array_equal(mp, pitch_ref.descriptors(*D.samples("snd"))[0])
    assert np.allclose(mean, [np.mean(out[at + 2 + l], axis=0) for l in range(len(lanes))], rtol=1e-12, atol=1e-12)
    ns2, nf2, again, mp2, mean2 = out[-9:-4]                     # lane 0 after its reset and 1100 samples more
    assert ns2.tolist() == [1100] + ns.tolist()[1:] and nf2[0] == again.shape[0] == Engine.mfcc_num_frames(1100)
    _mfcc_close(oracle, again, lanes[0][:1100], 12)
    assert mp2[0] == pitch_ref.max_power(lanes[0][:1100]) and np.array_equal(mp2[1:], mp[1:])
    assert np.allclose(mean2[0], np.mean(again, axis=0), rtol=1e-12, atol=1e-12) and np.array_equal(mean2[1:], mean[1:])
    _mfcc_close(oracle, out[-3], lanes[1], 12)                   # the seeded lane, analysed by its first push


def check_reconstruct(oracle, probe, D, out):
    rec, pcm, w, wpcm, s, spcm, pos = out
    x, off = D.samples("snd")
    idx, ooff, maps, moff, frames, pair_len = hc.recon_maps(D)
    bits = lambda v: np.asarray(v, dtype=np.float64).view(np.uint64)
    assert np.array_equal(bits(rec), bits(tail_ref.reconstruct(x, off, idx, ooff)))
    assert np.array_equal(pcm, tail_ref.pcm32_array(rec))
    assert np.array_equal(bits(w), bits(warp_ref.warp(D["snd"], idx, ooff, maps, moff, frames, pair_len)))
    assert np.array_equal(wpcm, warp_ref.pcm32(w))
    want, want_pos = wsola_ref.wsola(D["snd"], idx, ooff, maps, moff, frames, pair_len, hc.WSOLA_SEARCH)
    assert np.array_equal(pos, want_pos)
    assert np.array_equal(bits(s), bits(want)) and np.array_equal(spcm, warp_ref.pcm32(s))
    assert not np.array_equal(bits(s), bits(w))                  # (the search does move frames here)


def check_partition(oracle, probe, D, out):
    std, weights, means, covs, ll, iters, letters, post, seg, vseg, votes = out
    close = lambda got, want, tol: np.all(np.abs(got - want) <= tol * (1.0 + np.abs(want)))
    train, other = D["trn"][0], np.concatenate(D["oth"])
    assert close(std, partition_ref.standardize(train), 1e-12)
    want = partition_ref.gmm_train(partition_ref.standardize(train), hc.gmm_rows(train.shape[0]), max_iters=5)
    assert iters[0] == want["iters"]
    for got, key in ((weights, "weights"), (means, "means"), (covs, "covs")):
        assert np.allclose(got, want[key], rtol=1e-9, atol=1e-12), key
    assert np.allclose(ll[0], want["log_lik"], rtol=1e-9)
    want_post, _ = partition_ref.posteriors(partition_ref.standardize(other), weights, means, covs)
    assert np.allclose(post, want_post, rtol=0, atol=1e-9)
    assert np.array_equal(letters, partition_ref.letters(post))
    assert seg.tolist() == vseg.tolist() and int(seg.sum()) == other.shape[0]


def check_merge(oracle, probe, D, out):
    costs, idx, dist = hc.merge_inputs(D.variant)
    for k, d in enumerate((None, None, dist)):
        wi, wc = tail_ref.merge(costs, idx, d)
        assert np.array_equal(out[2 * k], wi) and np.array_equal(out[2 * k + 1], wc)


CHECKS = {
    "dtw_search": check_search, "dtw_search_f32": check_search, "dtw_long_rows": check_search, "dtw_band8": check_search,
    "dtw_wide64": check_search, "dtw_distances": check_distances, "dtw_topk3": check_topk(3), "dtw_topk64": check_topk(64),
    "dtw_match_one": check_match_one, "dtw_few_batch": check_batches((4, 5), False), "dtw_match_batch": check_batches((65,), True),
    "dtw_pruned_step": check_pruned_step, "dtw_begin_finish": check_begin_finish, "dtw_chain": check_chain,
    "dtw_pair_matrix": check_pair_matrix,
    "align": check_align("symmetric"), "align_lds": check_align("symmetric"), "align_slab": check_align("symmetric"),
    "align_paced": check_align("paced"), "align_band6": check_align("symmetric"),
    "spot_sym": check_spot("symmetric"), "spot_paced": check_spot("paced"),
    "spotter_sym": check_spotter("symmetric"), "spotter_paced": check_spotter("paced"),
    "refcos_70x45": check_search, "refcos_q8": check_search, "refcos_f64": check_search, "refcos_tile": check_search,
    "refcos_unholdable": check_unholdable, "refcos_distances": check_distances, "refcos_topk8": check_topk(8),
    "refcos_match_one": check_match_one, "refcos_few_batch": check_batches((64, 65), False), "refcos_chain": check_chain,
    "refcos_chain_append": check_chain, "refcos_pair_matrix": check_pair_matrix,
    "mfcc": check_mfcc, "mfcc_batch": check_mfcc_batch, "sequence": check_sequence, "descriptors": check_descriptors,
    "stream": check_stream, "reconstruct": check_reconstruct, "partition": check_partition, "merge": check_merge,
}

# the route each probe is named for, on the fresh context (the dirty runs are held to the same)
ROUTES = {
    "dtw_search": dict(used_filter=1), "dtw_search_f32": dict(used_filter=1), "dtw_long_rows": dict(used_filter=1),
    "dtw_band8": dict(used_filter=1), "dtw_wide64": dict(used_filter=1), "dtw_distances": dict(used_filter=1),
    "dtw_topk3": dict(used_filter=1), "dtw_begin_finish": dict(used_filter=1),
    "dtw_pruned_step": dict(begin_pruned=1, call_pruned=1),
    "dtw_few_batch": {"packed/4": 0, "packed/5": 1, "used_filter/4": 0, "used_filter/5": 1},
    "refcos_70x45": dict(refcos_filter=0), "refcos_q8": dict(refcos_filter=2), "refcos_f64": dict(refcos_filter=1),
    "refcos_tile": dict(refcos_filter=0), "refcos_unholdable": dict(refcos_filter=1), "refcos_distances": dict(refcos_filter=2),
    "refcos_topk8": dict(refcos_filter=2), "refcos_few_batch": {"packed/64": 0, "packed/65": 1},
}


def test_every_probe_has_a_reference_check():
    assert set(CHECKS) == set(hc.PROBES)


@pytest.mark.parametrize("name", PROBES)
def test_the_fresh_answer_is_the_references(oracle, fresh, name):
    probe = hc.PROBES[name]
    out, route = fresh(name)
    print(name, "route:", route)
    for key, want in ROUTES.get(name, {}).items():
        assert route[key] == want, (key, route)
    CHECKS[name](oracle, probe, probe.data(), out)


# -- probe x prelude --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prelude", sorted(hc.PRELUDES))
@pytest.mark.parametrize("name", PROBES)
def test_the_dirty_answer_is_the_fresh_answer(fresh, name, prelude):
    probe = hc.PROBES[name]
    run_dirty(probe, lambda e: hc.PRELUDES[prelude](e, probe), fresh, "%s after %s" % (name, prelude))


def test_the_refused_calls_are_refused():
    for ctx in (hc.DTW64, hc.REFCOS):
        e = hc.new_engine(ctx)
        got = hc.refused_calls(e)
        e.close()
        assert len(got) == 5 and all(err is not None for err in got.values()), got
        assert "non-decreasing" in str(got["decreasing offsets"])


def test_finish_after_an_unfinished_begin_and_another_search_is_refused(fresh):
    """The header: any other matching call on the context ends a begun pair, and ssym_match_finish then fails."""
    import torch
    probe = hc.PROBES["dtw_search"]
    e = hc.new_engine(probe.ctx)
    hc.unfinished_begin(e)
    got, _ = probe.run(e)
    assert_same_outputs(got, fresh("dtw_search")[0], "dtw_search after an unfinished begin")
    b = torch.zeros(40, dtype=torch.float64, device="cuda")
    oi, oc = torch.zeros(40, dtype=torch.int32, device="cuda"), torch.zeros(40, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(nat.SsymError, match="without ssym_match_begin"):
        e.match_finish(b, oi, oc)
    e.close()


@pytest.mark.parametrize("first,second", hc.OTHER_ROUTES + [(b, a) for a, b in hc.OTHER_ROUTES])
def test_the_other_route_first(fresh, first, second):
    a, b = hc.PROBES[first], hc.PROBES[second]
    assert hc.ctx_key(a.ctx) == hc.ctx_key(b.ctx)
    run_dirty(b, lambda e: hc.dirty_run(e, a, hc.PLAIN), fresh, "%s after %s" % (second, first))


@pytest.mark.parametrize("name", [n for n in PROBES if hc.PROBES[n].takes_dict])
def test_used_handles(fresh, name):
    probe = hc.PROBES[name]
    want, want_route = fresh(name)
    e = hc.new_engine(probe.ctx)
    try:
        with hc.Handles() as h:
            d = hc.used_dictionary(e, probe, h)
            got, route = probe.run(e, dictionary=d)
    finally:
        e.close()
    assert route == want_route, (route, want_route)
    assert_same_outputs(got, want, name + " on a used dictionary")


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("key", sorted(hc.by_ctx()), ids=lambda k: "-".join(str(v) for _, v in k))
def test_gauntlet(fresh, key, reverse):
    """One context per metric and dtype runs every probe's hostile twin followed by that probe, all families in one order;
    a second context runs them in the reverse order.  The twins' values take turns."""
    ctx, probes = hc.by_ctx()[key]
    order = list(reversed(probes)) if reverse else probes
    e = hc.new_engine(ctx)
    try:
        for k, probe in enumerate(order):
            hc.dirty_run(e, probe, hc.twin(hc.FILLS[k % len(hc.FILLS)]))
            got, route = probe.run(e)
            want, want_route = fresh(probe.name)
            assert route == want_route, (probe.name, route, want_route)
            assert_same_outputs(got, want, "%s, step %d of the gauntlet" % (probe.name, k))
    finally:
        e.close()
