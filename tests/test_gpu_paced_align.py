"""Paced alignment on the GPU (ssym_dtw_align_step with SSYM_STEP_PACED) against the numpy restatement
(tests/paced_path_ref.py): cost bits, len, path and map exactly equal.  Shapes inside and outside the pattern's bounds,
chunk and hand-off edges (skips that cross rows 62 -> 64 and 63 -> 65, repeats on rows 63 and 64), every DIMR and its
padding, the direction matrix on either side of the LDS boundary and at the limits, every way of listing pairs, a spotted
span cut and re-aligned, the symmetric step as the old call, features that are not finite, the warp along device maps,
and every refusal.  Outputs are sentinel-filled where the call is made through ctypes."""
import os
import re

import numpy as np
import pytest

import paced_path_ref as ref
import paced_ref
from dtw_path_ref import local_costs, same_floats
from soundsym_amd import HOP, Engine, Sound, SoundDictionary, SoundSequence
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT32, SENTF = 0xDEADBEEF, -12345.5
NO = nat.NO_MATCH
PACED, SYMMETRIC = nat.STEP_PACED, nat.STEP_SYMMETRIC


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


class _Sets:
    """An engine with a resident dictionary and query set made from lists of [frames, dim] arrays; the restatement's
    answer for a pair is computed once."""

    def __init__(self, src, tgt, dim, dtype="f64", squared=False, band=-1, metric="dtw"):
        self.src, self.tgt, self.dim, self.squared = src, tgt, dim, squared
        npd = np.float32 if dtype == "f32" else np.float64
        self.e = Engine(metric=metric, dtype=dtype, band=band, squared=squared)
        sf, so = pack_segments(src, dim, npd)
        tf, to = pack_segments(tgt, dim, npd)
        self.d, self.q = self.e.dictionary(sf, so, dim), self.e.queries(tf, to, dim)
        self._ref = {}

    def close(self):
        self.e.close()

    def ref(self, s, t):
        """(cost, path [L, 2], map [L]) of the restatement."""
        if (s, t) not in self._ref:
            self._ref[(s, t)] = ref.align(self.src[s], self.tgt[t], self.squared)
        return self._ref[(s, t)]


def _align(sets, src_idx, tgt_idx=None, base=0, step=PACED, device=False, want_map=True, offsets=None, plain=False):
    """ssym_dtw_align_step (plain: ssym_dtw_align) through ctypes into sentinel-filled outputs, with one entry more than
    the pairs need: (rc, cost, len, path [cells, 2], map, p_off, m_off)."""
    src = np.ascontiguousarray(src_idx, dtype=np.uint32)
    tgt = None if tgt_idx is None else np.ascontiguousarray(tgt_idx, dtype=np.uint32)
    n = src.size
    p_off, m_off = sets.e.dtw_align_sizes(sets.d, sets.q, src, tgt, base) if offsets is None else offsets
    cost = np.full(n + 1, SENTF)
    length = np.full(n + 1, SENT32, dtype=np.uint32)
    path = np.full((int(p_off[-1]) + 1, 2), SENT32, dtype=np.uint32)
    fmap = np.full(int(m_off[-1]) + 1, SENT32, dtype=np.uint32)
    L = nat.lib()
    head = [sets.e.ctx, sets.d.ptr, sets.q.ptr, src.ctypes.data, None if tgt is None else tgt.ctypes.data, n, base]
    call = L.ssym_dtw_align if plain else L.ssym_dtw_align_step
    if not plain:
        head.append(step)
    if device:
        import torch
        dcost = torch.from_numpy(cost).cuda()
        dlen = torch.from_numpy(length.view(np.int32)).cuda()
        dpath = torch.from_numpy(path.view(np.int32).reshape(-1)).cuda()
        dmap = torch.from_numpy(fmap.view(np.int32)).cuda()
        rc = call(*head, dcost.data_ptr(), dlen.data_ptr(), p_off.ctypes.data, dpath.data_ptr(), m_off.ctypes.data,
                  dmap.data_ptr() if want_map else None, nat.OUT_DEVICE)
        torch.cuda.synchronize()
        cost = dcost.cpu().numpy()
        length = dlen.cpu().numpy().view(np.uint32)
        path = dpath.cpu().numpy().view(np.uint32).reshape(-1, 2)
        fmap = dmap.cpu().numpy().view(np.uint32)
    else:
        rc = call(*head, cost.ctypes.data, length.ctypes.data, p_off.ctypes.data, path.ctypes.data, m_off.ctypes.data,
                  fmap.ctypes.data if want_map else None, 0)
    return rc, cost, length, path, fmap, p_off, m_off


def _untouched(out):
    return all(((x == SENTF) if x.dtype == np.float64 else (x == SENT32)).all() for x in out[1:5])


def _check(sets, src_idx, tgt_idx, out, base=0, with_map=True):
    """Every pair of a call equal to the restatement, element for element; every slot a pair did not write, and the entry
    beyond the pairs, untouched; the contract's consequences (1) on every path.  Returns the number of pairs with a path."""
    rc, cost, length, path, fmap, p_off, m_off = out
    assert rc == nat.SSYM_OK, nat.lib().ssym_last_error(sets.e.ctx)
    n = len(src_idx)
    assert cost[n] == SENTF and length[n] == SENT32 and (path[int(p_off[n]):] == SENT32).all() and (fmap[int(m_off[n]):] == SENT32).all()
    found = 0
    for p in range(n):
        t = p if tgt_idx is None else int(tgt_idx[p])
        p0, p1, m0, m1 = int(p_off[p]), int(p_off[p + 1]), int(m_off[p]), int(m_off[p + 1])
        want_cost, want_path, want_map = (float("inf"),) + ref.EMPTY if int(src_idx[p]) == NO else sets.ref(int(src_idx[p]) - base, t)
        L = want_path.shape[0]
        assert same_floats(cost[p], want_cost) and (np.isnan(want_cost) or _bits(cost[p]) == _bits(want_cost)), (p, cost[p], want_cost)
        assert int(length[p]) == L, (p, int(length[p]), L)
        assert np.array_equal(path[p0:p0 + L].astype(np.int64), want_path), p
        assert (path[p0 + L:p1] == SENT32).all(), p                       # nothing beyond the path is written
        if L and with_map:
            fa, fb = sets.src[int(src_idx[p]) - base].shape[0], sets.tgt[t].shape[0]
            assert L == fb == m1 - m0 and np.isfinite(cost[p])
            assert np.array_equal(fmap[m0:m1].astype(np.int64), want_map), p
            assert ref.admissible(fmap[m0:m1], fa), p
            found += 1
        else:
            assert (fmap[m0:m1] == SENT32).all(), p
            found += int(L > 0)
    return found


def _check_grouped(sets, src_idx, tgt_idx, out):
    """_check for long lists drawn from a few shapes (index_base 0, with maps): all pairs of one (source, target) at once."""
    rc, cost, length, path, fmap, p_off, m_off = out
    assert rc == nat.SSYM_OK, nat.lib().ssym_last_error(sets.e.ctx)
    src_idx, tgt_idx = np.asarray(src_idx), np.asarray(tgt_idx)
    n = src_idx.size
    assert cost[n] == SENTF and length[n] == SENT32 and (path[int(p_off[n]):] == SENT32).all() and (fmap[int(m_off[n]):] == SENT32).all()
    keys = np.where(src_idx == NO, -1, src_idx.astype(np.int64) * 1000 + tgt_idx)
    p_off, m_off = p_off.astype(np.int64), m_off.astype(np.int64)
    found = 0
    for key in np.unique(keys):
        pairs = np.flatnonzero(keys == key)
        want_cost, want_path, want_map = (float("inf"),) + ref.EMPTY if key < 0 else sets.ref(int(key) // 1000, int(key) % 1000)
        L = want_path.shape[0]
        assert same_floats(cost[pairs], np.full(pairs.size, want_cost)), (key, want_cost)
        assert (length[pairs] == L).all(), (key, L)
        room, frames = p_off[pairs + 1] - p_off[pairs], m_off[pairs + 1] - m_off[pairs]
        if key >= 0:
            assert (room == room[0]).all() and (frames == frames[0]).all()
            got = path[p_off[pairs][:, None] + np.arange(room[0])]
            assert (got[:, :L] == want_path[None]).all() and (got[:, L:] == SENT32).all(), key
            got = fmap[m_off[pairs][:, None] + np.arange(frames[0])]
            assert (got == want_map[None]).all() if L else (got == SENT32).all(), key
        else:
            assert (room == 0).all() and (frames == 0).all()
        found += pairs.size if L else 0
    return found


def _ints(rng, f, dim):
    return rng.integers(0, 3, size=(f, dim)).astype(np.float64)            # {0, 1, 2}: exact sums, real ties


def _reals(rng, f, dim):
    return rng.standard_normal((f, dim)).astype(np.float32).astype(np.float64)      # (what an f32 engine holds too)


def _distinct(rng, f, dim):
    """Frames no two of which are equal, far apart: a copy of a frame is the only place it costs 0."""
    x = rng.integers(100, 200, size=(f, dim)).astype(np.float64)
    x[:, 0] = 1000.0 + 7.0 * np.arange(f)
    return x


def _inside(rng, fb):
    """A source length drawn inside the bounds of a target of fb frames: every drawn pair is feasible."""
    lo, hi = paced_ref.span_bounds(fb)
    return int(rng.integers(lo, hi + 1))


def _feasible_sets(rng, mk, n, fb_lo, fb_hi, dim, **kw):
    """n pairs (source p, target p), target lengths drawn in fb_lo ... fb_hi, source lengths inside their bounds."""
    fbs = [int(rng.integers(fb_lo, fb_hi + 1)) for _ in range(n)]
    return _Sets([mk(rng, _inside(rng, fb), dim) for fb in fbs], [mk(rng, fb, dim) for fb in fbs], dim, **kw)


# ---- 1. exactness: ties, real values, both cost modes, both engine dtypes ---------------------------------------------------

@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("dim", [1, 13])
@pytest.mark.parametrize("kind,squared", [("int", True), ("int", False), ("real", True), ("real", False)])
def test_random_feasible_pairs_equal_the_restatement(kind, squared, dim, dtype):
    rng = np.random.default_rng(0xA71 + 2 * dim + squared)
    s = _feasible_sets(rng, _ints if kind == "int" else _reals, 40, 1, 90, dim, dtype=dtype, squared=squared)
    idx = np.arange(40, dtype=np.uint32)
    out = _align(s, idx)
    assert _check(s, idx, None, out) == 40
    # consequence (2): the cost is the path's own sum, in path order
    for p in range(0, 40, 7):
        c = local_costs(s.src[p], s.tgt[p], squared)
        m = out[4][int(out[6][p]):int(out[6][p + 1])].astype(np.int64)
        assert _bits(ref.resum(c, m)) == _bits(out[1][p])
    s.close()


# ---- 2. the shape rule -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,squared", [("int", True), ("real", False)])
def test_a_five_frame_target_against_every_source_length(kind, squared):
    rng = np.random.default_rng(0xA72 + squared)
    mk = _ints if kind == "int" else _reals
    s = _Sets([mk(rng, f, 13) for f in range(1, 12)], [mk(rng, 5, 13)], 13, squared=squared)
    si, ti = np.arange(11, dtype=np.uint32), np.zeros(11, dtype=np.uint32)
    out = _align(s, si, ti)
    assert _check(s, si, ti, out) == 7                                   # 5 frames take sources of 3 ... 9
    assert [int(x) for x in out[2][:11]] == [0, 0, 5, 5, 5, 5, 5, 5, 5, 0, 0]
    assert np.isposinf(out[1][[0, 1, 9, 10]]).all()
    s.close()


def test_every_target_length_against_a_65_frame_source():
    rng = np.random.default_rng(0xA73)
    src = _reals(rng, 65, 3)
    s = _Sets([src], [_reals(rng, f, 3) for f in range(1, 71)], 3)
    si, ti = np.zeros(70, dtype=np.uint32), np.arange(70, dtype=np.uint32)
    out = _align(s, si, ti)
    # 65 source frames fit targets of 33 ... 129 frames
    assert _check(s, si, ti, out) == 70 - 32
    assert (out[2][:32] == 0).all() and np.isposinf(out[1][:32]).all() and (out[2][32:70] == np.arange(33, 71)).all()
    s.close()


# ---- 3. chunk and hand-off edges ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,squared", [("int", True), ("real", False)])
def test_source_lengths_around_the_chunk_edges(kind, squared):
    rng = np.random.default_rng(0xA74 + squared)
    mk = _ints if kind == "int" else _reals
    frames = [63, 64, 65, 66, 127, 128, 129, 130]
    src = [mk(rng, f, 13) for f in frames]
    # per source: the shortest and the longest target it fits (every step a skip, every frame repeated), and two in between
    tgt, si, ti = [], [], []
    for k, fa in enumerate(frames):
        for fb in (fa // 2 + 1, fa, int(rng.integers(fa // 2 + 1, 2 * fa + 1)), 2 * fa):
            assert ref.feasible(fa, fb)
            si.append(k)
            ti.append(len(tgt))
            tgt.append(mk(rng, fb, 13))
    s = _Sets(src, tgt, 13, squared=squared)
    assert _check(s, si, ti, _align(s, si, ti)) == len(si)
    s.close()


@pytest.mark.parametrize("odd", [False, True])
def test_a_decimated_target_whose_skips_cross_the_chunk_edges(odd):
    """Every second source frame: all steps are +2 and the cost is 0.  Even rows (map[j] = 2 j) step 62 -> 64 and 126 ->
    128, through the second hand-off row; with the pinned row 0 followed by the odd rows (map[j] = 2 j - 1) they step
    63 -> 65 and 127 -> 129, through the first hand-off row into lane 1's second diagonal."""
    rng = np.random.default_rng(0xA75 + odd)
    src = _distinct(rng, 135, 13)
    rows = np.concatenate([[0], np.arange(1, 135, 2)]) if odd else np.arange(0, 135, 2)
    src = src[:int(rows[-1]) + 1]
    s = _Sets([src], [src[rows]], 13, squared=True)
    out = _align(s, [0], [0])
    assert _check(s, [0], [0], out) == 1
    assert out[1][0] == 0.0 and np.array_equal(out[4][:rows.size], rows)
    if not odd:
        assert np.array_equal(out[4][:rows.size], 2 * np.arange(rows.size)) and src.shape[0] == 2 * rows.size - 1
    for a, b in (((63, 65), (127, 129)) if odd else ((62, 64), (126, 128))):
        j = int(np.flatnonzero(rows == a)[0])
        assert rows[j + 1] == b
    s.close()


def test_a_doubled_target_repeats_on_rows_63_and_64():
    rng = np.random.default_rng(0xA76)
    src = _distinct(rng, 70, 13)
    tgt = np.repeat(src, 2, axis=0)
    s = _Sets([src], [tgt], 13, squared=True)
    out = _align(s, [0], [0])
    assert _check(s, [0], [0], out) == 1
    assert out[1][0] == 0.0 and src.shape[0] == tgt.shape[0] // 2
    assert np.array_equal(out[4][:140], np.arange(140) // 2)             # rows 63 and 64 each taken twice
    s.close()


# ---- 4. dim -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 13, 14, 15, 16, 17, 40, 41, 64])
def test_padding_edges_of_every_dimr(dim):
    rng = np.random.default_rng(0xA77 + dim)
    for mk, squared in ((_ints, True), (_reals, False)):
        s = _Sets([mk(rng, 130, dim), mk(rng, 70, dim), mk(rng, 9, dim)], [mk(rng, 9, dim), mk(rng, 70, dim), mk(rng, 129, dim)],
                  dim, squared=squared)
        si, ti = [0, 0, 1, 1, 2, 1], [1, 2, 1, 2, 0, 0]                   # the last one: 70 frames do not fit 9
        assert _check(s, si, ti, _align(s, si, ti)) == 5
        s.close()


# ---- 5. the direction matrix: LDS, the global slab, the limits ---------------------------------------------------------------

def _dir_lds_bytes():
    text = open(os.path.join(ROOT, "soundsym_amd", "csrc", "dtw_align.hip")).read()
    return int(re.search(r"\bkAlignDirLdsBytes\s*=\s*([0-9]+)\s*;", text).group(1))


@pytest.mark.parametrize("fa,fb", [(256, 256), (257, 256), (1024, 2048), (4095, 2048)])
def test_direction_matrix_in_lds_in_the_slab_and_at_the_limits(fa, fb):
    lds = _dir_lds_bytes()
    assert (fa * ((fb + 15) // 16) * 4 <= lds) == ((fa, fb) == (256, 256))
    rng = np.random.default_rng(0xA78 + fa)
    s = _Sets([_reals(rng, fa, 2)], [_reals(rng, fb, 2)], 2)
    out = _align(s, [0], [0])
    assert _check(s, [0], [0], out) == 1
    dev = _align(s, [0], [0], device=True)
    for x, y in zip(out[1:5], dev[1:5]):
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)
    s.close()


def _scratch_bytes():
    text = open(os.path.join(ROOT, "soundsym_amd", "csrc", "dtw_align.hip")).read()
    m = re.search(r"\bkAlignScratchBytes\s*=\s*\(size_t\)\s*([0-9]+)\s*<<\s*([0-9]+)\s*;", text)
    return int(m.group(1)) << int(m.group(2))


def _followed(kinds, g, first, then):
    """How often a pair of a kind in `first` is followed, in the same workgroup of a grid of g, by one of a kind in `then`."""
    return int(np.count_nonzero(np.isin(kinds[:-g], first) & np.isin(kinds[g:], then)))


def test_slab_and_lds_pairs_in_one_call_and_a_slab_reused():
    """One workgroup's slab holds a pair after another: the second walk must read its own codes, not the lines the first
    left in the cache.  Pairs small enough for LDS sit between them.  A call runs min(pairs, 8 per CU, scratch / largest
    slab) workgroups, so the list is more than twice as long as the largest of those grids."""
    rng = np.random.default_rng(0xA79)
    shapes = [(300, 300), (20, 20), (280, 400), (257, 256), (10, 12), (400, 300)]
    dir_bytes = np.array([fa * ((fb + 15) // 16) * 4 for fa, fb in shapes])
    in_slab = np.flatnonzero(dir_bytes > _dir_lds_bytes())
    assert in_slab.tolist() == [0, 2, 3, 5]
    s = _Sets([_ints(rng, fa, 2) for fa, _ in shapes], [_ints(rng, fb, 2) for _, fb in shapes], 2, squared=True)
    n = 5000
    si = rng.integers(0, len(shapes), size=n).astype(np.uint32)
    for cus in (64, 256, 304):
        g = min(8 * cus, _scratch_bytes() // int(dir_bytes.max()))
        assert n > 2 * g and g == 8 * cus                                # (the slabs of this list do not cap the grid)
        assert _followed(si, g, in_slab, in_slab) >= 500                 # a slab used again, by a pair of another or the same shape
        assert _followed(si, g, in_slab, [1, 4]) >= 200 and _followed(si, g, [1, 4], in_slab) >= 200
    assert _check_grouped(s, si, si, _align(s, si, si)) == n
    s.close()


def test_more_pairs_than_workgroups_with_every_kind_of_pair_in_one_list():
    """Workgroup b of a grid of g walks pairs b, b + g, ...: every kind of pair is followed by every other in the same
    wave -- one-chunk and multi-chunk pairs (both hand-off rows rewritten), pairs dropped before the recurrence (a shape
    without a path, an empty source, an empty target, SSYM_NO_MATCH) and a pair whose cost is NaN (dropped after it,
    before the walk's barriers)."""
    rng = np.random.default_rng(0xA7F1)
    dim = 3
    poisoned = _ints(rng, 130, dim)
    poisoned[70, 1] = np.nan
    #            one chunk  two chunks  four chunks  no path    no source  NaN        no target
    shapes = [(20, 24), (130, 100), (200, 150), (130, 9), (0, 24), (130, 100), (24, 0)]
    src = [_ints(rng, fa, dim) for fa, _ in shapes]
    src[5] = poisoned
    s = _Sets(src, [_ints(rng, fb, dim) for _, fb in shapes], dim, squared=True)
    assert np.isnan(s.ref(5, 5)[0]) and [s.ref(k, k)[1].shape[0] for k in range(7)] == [24, 100, 150, 0, 0, 0, 0]
    n = 5000
    assert n > 2 * 8 * 256                            # 8 workgroups per CU, 256 CUs: every workgroup walks several pairs
    kinds = rng.integers(0, 8, size=n)                # 7: SSYM_NO_MATCH
    si = np.where(kinds == 7, NO, kinds).astype(np.uint32)
    ti = np.where(kinds == 7, rng.integers(0, 7, size=n), kinds).astype(np.uint32)
    for cus in (64, 256, 304):
        g = 8 * cus
        if n <= g:
            continue
        for first in ([3, 4, 6, 7], [5], [1, 2], [0]):
            for then in ([0], [1, 2], [5], [3, 4, 6, 7]):
                assert _followed(kinds, g, first, then) >= 20, (cus, first, then)
    out = _align(s, si, ti)
    assert _check_grouped(s, si, ti, out) == int(np.count_nonzero(kinds <= 2))
    assert np.isnan(out[1][:n][kinds == 5]).all() and np.isposinf(out[1][:n][np.isin(kinds, [3, 4, 6, 7])]).all()
    dev = _align(s, si, ti, device=True)
    for x, y in zip(out[1:5], dev[1:5]):
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)
    s.close()


# ---- 6. pair lists ------------------------------------------------------------------------------------------------------------

def test_pairings_index_base_no_match_empty_and_infeasible_pairs_device_outputs():
    rng = np.random.default_rng(0xA7A)
    dim = 13
    mk = lambda f: rng.integers(-3, 4, size=(f, dim)).astype(np.float64)
    src = [mk(f) for f in (30, 0, 90, 1, 150, 64, 0, 77, 5)]
    tgt = [mk(f) for f in (20, 0, 60, 1, 80, 64, 7)]
    s = _Sets(src, tgt, dim, squared=True)
    first = np.array([0, 2, 2, 3, 4, 5, 8], dtype=np.uint32)              # tgt_idx = NULL: pair p uses target p
    a = _align(s, first)
    b = _align(s, first, np.arange(7, dtype=np.uint32))
    assert _check(s, first, None, a) == 6                                 # (target 1 is empty)
    for x, y in zip(a[1:5], b[1:5]):
        assert np.array_equal(x, y)
    _check(s, first[:3], None, _align(s, first[:3]))                      # fewer pairs than targets
    # repeats, any pairing, SSYM_NO_MATCH, index_base = 1: feasible, infeasible, empty and missing in one list
    si = np.array([6, 6, 1, NO, 5, 6, NO, 3, 2, 8, 5, 9, 4], dtype=np.uint32)
    ti = np.array([5, 5, 0, 2, 4, 5, 0, 2, 4, 1, 6, 6, 3], dtype=np.uint32)
    out = _align(s, si, ti, base=1)
    found = _check(s, si, ti, out, base=1)
    assert found == 8
    for p in (3, 6, 8, 9, 10):                                            # no match, no match, empty source, empty target, 150 into 7
        assert np.isposinf(out[1][p]) and out[2][p] == 0
    dev = _align(s, si, ti, base=1, device=True)
    assert dev[0] == nat.SSYM_OK
    for x, y in zip(out[1:5], dev[1:5]):
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)
    nomap = _align(s, si, ti, base=1, want_map=False)
    assert _check(s, si, ti, nomap, base=1, with_map=False) == found and (nomap[4] == SENT32).all()
    # offsets of the caller's own: exactly Fb cells per pair is enough, one fewer is refused
    fb = np.array([0 if x == NO or src[x - 1].shape[0] == 0 else tgt[t].shape[0] for x, t in zip(si, ti)], dtype=np.uint64)
    tight = np.concatenate([[0], np.cumsum(fb)]).astype(np.uint64)
    got = _align(s, si, ti, base=1, offsets=(tight, tight.copy()))
    assert _check(s, si, ti, got, base=1) == found
    short = tight.copy()
    short[1:] -= 1
    bad = _align(s, si, ti, base=1, offsets=(short, tight.copy()))
    assert bad[0] == nat.SSYM_E_INVALID and _untouched(bad) and b"offsets of pair 0" in nat.lib().ssym_last_error(s.e.ctx)
    # the Python layer: host and device
    cost, length, paths, maps = s.e.dtw_align(s.d, s.q, si, ti, index_base=1, step="paced")
    assert np.array_equal(_bits(cost), _bits(out[1][:-1])) and np.array_equal(length, out[2][:-1])
    for p in range(si.size):
        p0, m0 = int(out[5][p]), int(out[6][p])
        assert np.array_equal(paths[p], out[3][p0:p0 + int(length[p])]) and np.array_equal(maps[p], out[4][m0:m0 + int(length[p])])
    dcost, dlen, dpath, dmap, p_off, m_off = s.e.dtw_align_device(s.d, s.q, si, ti, index_base=1, step="paced")
    assert dcost.is_cuda and np.array_equal(_bits(dcost.cpu().numpy()), _bits(cost))
    assert np.array_equal(dlen.cpu().numpy().view(np.uint32), length)
    hm = dmap.cpu().numpy().view(np.uint32)
    for p in range(si.size):
        assert np.array_equal(hm[int(m_off[p]):int(m_off[p]) + int(length[p])], maps[p])
    s.close()


def test_4096_short_pairs_in_one_call_equal_one_call_each_in_any_order():
    rng = np.random.default_rng(0xA7B)
    n = 4096
    # (16 ... 24 frames on both sides lie inside one another's bounds)
    s = _Sets([_reals(rng, int(f), 5) for f in rng.integers(16, 25, size=n)], [_reals(rng, int(f), 5) for f in rng.integers(16, 25, size=n)], 5)
    idx = np.arange(n, dtype=np.uint32)
    cost, length, paths, maps = s.e.dtw_align(s.d, s.q, idx, idx, step="paced")
    assert (length > 0).all()
    for p in range(0, n, 9):
        want = s.ref(p, p)
        assert _bits(cost[p]) == _bits(want[0]) and np.array_equal(maps[p], want[2]) and np.array_equal(paths[p], want[1])
    order = rng.permutation(n).astype(np.uint32)
    c2, l2, p2, m2 = s.e.dtw_align(s.d, s.q, order, order, step="paced")
    assert np.array_equal(_bits(c2), _bits(cost[order])) and np.array_equal(l2, length[order])
    assert all(np.array_equal(m2[k], maps[int(order[k])]) for k in range(n))
    L = nat.lib()
    one_c, one_l = np.zeros(1), np.zeros(1, dtype=np.uint32)
    one_p, one_m = np.zeros((64, 2), dtype=np.uint32), np.zeros(64, dtype=np.uint32)
    off = np.zeros(2, dtype=np.uint64)
    for p in range(n):
        off[1] = s.tgt[p].shape[0]
        rc = L.ssym_dtw_align_step(s.e.ctx, s.d.ptr, s.q.ptr, idx[p:].ctypes.data, idx[p:].ctypes.data, 1, 0, PACED,
                                   one_c.ctypes.data, one_l.ctypes.data, off.ctypes.data, one_p.ctypes.data, off.ctypes.data,
                                   one_m.ctypes.data, 0)
        assert rc == nat.SSYM_OK and _bits(one_c[0]) == _bits(cost[p]) and one_l[0] == length[p]
        assert np.array_equal(one_m[:int(one_l[0])], maps[p]) and np.array_equal(one_p[:int(one_l[0])], paths[p])
    s.close()


# ---- 7. spot -> cut -> align --------------------------------------------------------------------------------------------------

def _recording(rng, frames, nc, plants):
    f = 6.0 + rng.standard_normal((frames, nc))                           # noise away from the targets' frames
    for at, what in plants:
        f[at:at + what.shape[0]] = what
    return Sound(rng.standard_normal(frames * HOP), 8000.0, f.reshape(-1), "rec", ncoeffs=nc)


def test_a_paced_spot_cut_and_aligned_has_the_spots_cost_bits():
    rng = np.random.default_rng(0xA7C)
    nc = 5
    tgt_f = rng.standard_normal((12, nc))
    long_f = rng.standard_normal((30, nc))
    noisy = lambda x: x + 0.05 * rng.standard_normal(x.shape)
    e = Engine(metric="dtw", dtype="f64")
    d = SoundDictionary(engine=e)
    # three plants of the short target at three paces (as it is, every second frame, every frame doubled), one of the long one
    d.sounds = [_recording(rng, 260, nc, ((10, noisy(tgt_f)), (70, noisy(tgt_f[::2])), (120, noisy(np.repeat(tgt_f, 2, axis=0))),
                                          (180, noisy(long_f))))]
    targets = [Sound(rng.standard_normal(12 * HOP), 8000.0, tgt_f.reshape(-1), "t", ncoeffs=nc),
               Sound(rng.standard_normal(30 * HOP), 8000.0, long_f.reshape(-1), "l", ncoeffs=nc)]
    spots = d.spot(targets, step="paced")
    assert [(sp.start_frame, sp.end_frame) for sp in spots][1] == (180, 209) and all(sp.cost > 0 for sp in spots)
    cut = d.cut(spots)
    al = cut.align(targets, indices=[0, 1], step="paced")
    feats = d.sounds[0].mfcc_arrays()
    for t, (sp, a) in enumerate(zip(spots, al)):
        assert _bits(a.cost) == _bits(sp.cost), t                         # consequence (4)
        want = ref.align(feats[sp.start_frame:sp.end_frame + 1], targets[t].mfcc_arrays())
        assert _bits(a.cost) == _bits(want[0]) and np.array_equal(a.frame_map, want[2]) and np.array_equal(a.path, want[1])
        assert len(a) == targets[t].num_frames() and ref.admissible(a.frame_map, sp.num_frames())
    # the default is the symmetric alignment of the same cut, as before: another recurrence, another cost
    sym = cut.align(targets, indices=[0, 1])
    assert [len(x) >= targets[t].num_frames() for t, x in enumerate(sym)] == [True, True]
    assert any(_bits(x.cost) != _bits(y.cost) for x, y in zip(sym, al))
    # every occurrence, K = 3
    occ = d.spot_all([targets[0]], max_spots=3, step="paced")[0]
    assert len(occ) == 3
    for sp, (first, last) in zip(sorted(occ, key=lambda x: x.start_frame), ((10, 21), (70, 75), (120, 143))):
        assert first <= sp.start_frame <= sp.end_frame <= last              # one span inside every plant: three paces
    cut3 = d.cut(occ)
    al3 = cut3.align([targets[0]] * 3, indices=[0, 1, 2], step="paced")
    for sp, a in zip(occ, al3):
        assert _bits(a.cost) == _bits(sp.cost) and len(a) == 12 and ref.admissible(a.frame_map, sp.num_frames())
    seq = SoundSequence.new([targets[0]] * 3)
    assert [x.cost for x in seq.align_to_dictionary(cut3, step="paced")] == \
        [x.cost for x in cut3.align([targets[0]] * 3, step="paced")]
    e.close()


# ---- 8. the symmetric step is the old call ------------------------------------------------------------------------------------

@pytest.mark.parametrize("band", [-1, 6])
def test_symmetric_step_is_ssym_dtw_align_bit_for_bit(band):
    rng = np.random.default_rng(0xA7D + band)
    dim = 13
    src = [_reals(rng, f, dim) for f in (130, 0, 64, 7, 300)]
    tgt = [_reals(rng, f, dim) for f in (128, 70, 0, 9, 301)]
    s = _Sets(src, tgt, dim, band=band)
    si = np.array([0, 2, NO, 3, 1, 0, 4, 2], dtype=np.uint32)
    ti = np.array([0, 1, 0, 3, 0, 2, 4, 0], dtype=np.uint32)
    for device in (False, True):
        old = _align(s, si, ti, plain=True, device=device)
        new = _align(s, si, ti, step=SYMMETRIC, device=device)
        assert old[0] == new[0] == nat.SSYM_OK
        for x, y in zip(old[1:5], new[1:5]):
            assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)
        assert (old[2][:-1] > 0).sum() >= 4
    s.close()


# ---- 9. features that are not finite ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", [float("nan"), float("inf"), 1e200])
@pytest.mark.parametrize("squared", [True, False])
def test_a_non_finite_value_in_a_source_or_a_target_frame(value, squared):
    rng = np.random.default_rng(0xA7E)
    dim = 13
    base_src, base_tgt = _reals(rng, 130, dim), _reals(rng, 100, dim)
    src, tgt = [base_src], [base_tgt]
    for row in (0, 10, 63, 64, 65, 129):
        a = base_src.copy()
        a[row, dim - 1] = value
        src.append(a)
    for col in (0, 50, 99):
        b = base_tgt.copy()
        b[col, 2] = value
        tgt.append(b)
    s = _Sets(src, tgt, dim, squared=squared)
    si = np.repeat(np.arange(len(src), dtype=np.uint32), len(tgt))
    ti = np.tile(np.arange(len(tgt), dtype=np.uint32), len(src))
    out = _align(s, si, ti)
    found = _check(s, si, ti, out)                                        # the restatement's cost (NaN where it has NaN), len, slots
    for p in range(si.size):
        k, t = int(si[p]), int(ti[p])
        pinned = k in (1, 6) or t >= 1                                    # the first or last source frame, or any target frame: on every path
        if pinned or (value != value and k >= 1):                         # ... and a NaN source frame floods the rows behind it
            assert not np.isfinite(out[1][p]) and out[2][p] == 0, (p, out[1][p])
    # a source frame whose local costs are +inf (not NaN) can be stepped over, as in paced spotting: the restatement decides,
    # and the path then avoids the row
    if value == value:
        assert found == 1 + 4
        for k, row in ((2, 10), (3, 63), (4, 64), (5, 65)):
            p = k * len(tgt)
            m = out[4][int(out[6][p]):int(out[6][p + 1])]
            assert row not in m and np.isfinite(out[1][p])
    else:
        assert found == 1
    s.close()


# ---- 10. the warp along device maps -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("search", [0, 64])
def test_warp_along_paced_device_maps_equals_the_warp_of_the_restatements_maps(search):
    rng = np.random.default_rng(0xA7F)
    nc = 5
    fbs = [12, 30, 7, 64, 9]
    fas = [20, 17, 13, 100, 40]                                           # the last one: 40 frames do not fit 9 -> the length fit
    assert [ref.feasible(a, b) for a, b in zip(fas, fbs)] == [True] * 4 + [False]
    mk = lambda f: Sound(rng.uniform(-1, 1, size=f * HOP + int(rng.integers(0, HOP))), 8000.0,
                         rng.standard_normal((f, nc)).reshape(-1), ncoeffs=nc)
    e = Engine(metric="dtw", dtype="f64")
    d = SoundDictionary(engine=e)
    d.sounds = [mk(f) for f in fas]
    targets = [mk(f) for f in fbs]
    idx = np.arange(5)
    maps, lengths = [], []
    for k in range(5):
        _, _, m = ref.align(d.sounds[k].mfcc_arrays(), targets[k].mfcc_arrays())
        lengths.append(m.size)
        maps.append(m if m.size else np.zeros(fbs[k], dtype=np.int64))
    assert lengths == fbs[:4] + [0]
    m_off = np.concatenate([[0], np.cumsum(fbs)]).astype(np.uint64)
    out_off = np.concatenate([[0], np.cumsum([t.samples().size for t in targets])]).astype(np.uint64)
    flat = np.concatenate(maps).astype(np.uint32)
    if search:
        want = e.reconstruct_wsola(d.resident_samples(), idx, out_off, flat, m_off, np.array(fbs), np.array(lengths, np.uint32), search)
        got = d.warp(targets, indices=idx, search=search, step="paced")
    else:
        want = e.reconstruct_warped(d.resident_samples(), idx, out_off, flat, m_off, np.array(fbs), np.array(lengths, np.uint32))
        got = d.warp(targets, indices=idx, step="paced")
    assert np.array_equal(_bits(got), _bits(want))
    # the pair that fits no paced path is the length fit of the plain reconstruction
    plain = e.reconstruct(d.resident_samples(), idx, out_off)
    assert np.array_equal(_bits(got[int(out_off[4]):]), _bits(plain[int(out_off[4]):]))
    assert not np.array_equal(_bits(got[:int(out_off[4])]), _bits(plain[:int(out_off[4])]))
    if not search:
        sym = d.warp(targets, indices=idx)
        assert not np.array_equal(_bits(sym), _bits(got))                 # the symmetric alignment warps the last pair too
    e.close()


# ---- 11. limits and refusals ----------------------------------------------------------------------------------------------------

def test_limits_and_an_unknown_step():
    rng = np.random.default_rng(0xA80)
    mk = lambda f: rng.integers(-2, 3, size=(f, 2)).astype(np.float64)
    s = _Sets([mk(1100), mk(4097), mk(4096)], [mk(2048), mk(2049), mk(3)], 2, squared=True)
    zero = np.zeros(1, dtype=np.uint32)
    assert _check(s, [0, 2], [0, 2], _align(s, [0, 2], [0, 2])) == 1      # at the limits: 2048 target frames; 4096 source frames listed
    assert _check(s, [2], [2], _align(s, [2], [2])) == 0                   # a call none of whose pairs has a path sizes nothing
    out = _align(s, zero, [1])
    assert out[0] == nat.SSYM_E_UNSUPPORTED and b"2048" in nat.lib().ssym_last_error(s.e.ctx) and _untouched(out)
    out = _align(s, [1], [0])
    assert out[0] == nat.SSYM_E_UNSUPPORTED and b"4096" in nat.lib().ssym_last_error(s.e.ctx) and _untouched(out)
    for step in (2, 7, 0xffffffff):
        out = _align(s, zero, zero, step=step)
        assert out[0] == nat.SSYM_E_INVALID and b"step" in nat.lib().ssym_last_error(s.e.ctx) and _untouched(out)
    assert _align(s, zero, [1], step=SYMMETRIC)[0] == nat.SSYM_OK        # 2049 frames: the symmetric limit holds
    with pytest.raises(nat.SsymError):
        s.e.dtw_align(s.d, s.q, [0], [1], step="paced")
    with pytest.raises(ValueError):
        s.e.dtw_align(s.d, s.q, [0], [0], step="itakura")
    s.close()
    wide = _Sets([np.zeros((3, 65))], [np.zeros((3, 65))], 65)
    out = _align(wide, zero)
    assert out[0] == nat.SSYM_E_UNSUPPORTED and _untouched(out)
    wide.close()


@pytest.mark.parametrize("kw", [dict(band=0), dict(band=32), dict(metric="refcos")])
def test_banded_and_refcos_contexts_are_refused(kw):
    rng = np.random.default_rng(1)
    s = _Sets([rng.standard_normal((8, 12))], [rng.standard_normal((6, 12))], 12, **kw)
    out = _align(s, np.zeros(1, dtype=np.uint32))
    assert out[0] == nat.SSYM_E_UNSUPPORTED and _untouched(out)
    assert (b"refcos" if "metric" in kw else b"band") in nat.lib().ssym_last_error(s.e.ctx)
    out = _align(s, np.zeros(1, dtype=np.uint32), step=9)
    assert out[0] == nat.SSYM_E_INVALID and _untouched(out)               # the step is looked at first
    s.close()
