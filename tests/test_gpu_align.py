"""ssym_dtw_align on the GPU against the numpy restatement (tests/dtw_path_ref.py), the exact kernels and the oracle:
exact equality where the arithmetic is exact (integer features, squared cost, real ties), optimality and bit-equal costs
on real-valued features, every shape edge of the kernel (64-row chunks, the 128-frame ring, the LDS / global-scratch
boundary of the direction matrix, the 4096-frame limit, bands), every way of listing pairs, the recordings end to end,
and every error the header lists."""
import ctypes
import os
import re

import numpy as np
import pytest

import dtw_path_ref as ref
from soundsym_amd import DeviceFrames, Engine, Sound, SoundDictionary, SoundSequence
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT32, SENTF = 0xDEADBEEF, -12345.5


def _const(name):
    text = open(os.path.join(ROOT, "soundsym_amd", "csrc", "dtw_align.hip")).read()
    m = re.search(r"\b%s\s*=\s*([0-9]+)\s*;" % name, text)
    assert m, name
    return int(m.group(1))


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


class _Sets:
    """An engine with a resident dictionary and query set made from lists of [frames, dim] arrays."""

    def __init__(self, src, tgt, dim, dtype="f64", band=-1, squared=False, metric="dtw"):
        self.src, self.tgt, self.dim, self.band, self.squared = src, tgt, dim, band, squared
        npd = np.float32 if dtype == "f32" else np.float64
        self.e = Engine(metric=metric, dtype=dtype, band=band, squared=squared)
        sf, so = pack_segments(src, dim, npd)
        tf, to = pack_segments(tgt, dim, npd)
        self.d, self.q = self.e.dictionary(sf, so, dim), self.e.queries(tf, to, dim)

    def close(self):
        self.e.close()

    def ref(self, s, t, want_ties=False):
        return ref.align(np.asarray(self.src[s], dtype=np.float64), np.asarray(self.tgt[t], dtype=np.float64), self.band,
                         self.squared, want_ties)


def _raw(sets, src_idx, tgt_idx=None, base=0, want_map=True, device=False, offsets=None):
    """ssym_dtw_align through ctypes into sentinel-filled outputs: (rc, cost, len, path [cells, 2], map, p_off, m_off)."""
    src = np.ascontiguousarray(src_idx, dtype=np.uint32)
    tgt = None if tgt_idx is None else np.ascontiguousarray(tgt_idx, dtype=np.uint32)
    n = src.size
    if offsets is None:
        p_off, m_off = sets.e.dtw_align_sizes(sets.d, sets.q, src, tgt, base)
    else:
        p_off, m_off = offsets
    cost = np.full(n, SENTF)
    length = np.full(n, SENT32, dtype=np.uint32)
    path = np.full((int(p_off[-1]), 2), SENT32, dtype=np.uint32)
    fmap = np.full(int(m_off[-1]), SENT32, dtype=np.uint32)
    L = nat.lib()
    tp = None if tgt is None else tgt.ctypes.data
    if device:
        import torch
        dcost = torch.from_numpy(cost).cuda()
        dlen = torch.from_numpy(length.view(np.int32)).cuda()
        dpath = torch.from_numpy(path.view(np.int32).reshape(-1)).cuda()
        dmap = torch.from_numpy(fmap.view(np.int32)).cuda()
        rc = L.ssym_dtw_align(sets.e.ctx, sets.d.ptr, sets.q.ptr, src.ctypes.data, tp, n, base, dcost.data_ptr(),
                              dlen.data_ptr(), p_off.ctypes.data, dpath.data_ptr(), m_off.ctypes.data,
                              dmap.data_ptr() if want_map else None, nat.OUT_DEVICE)
        torch.cuda.synchronize()
        cost = dcost.cpu().numpy()
        length = dlen.cpu().numpy().view(np.uint32)
        path = dpath.cpu().numpy().view(np.uint32).reshape(-1, 2)
        fmap = dmap.cpu().numpy().view(np.uint32)
    else:
        rc = L.ssym_dtw_align(sets.e.ctx, sets.d.ptr, sets.q.ptr, src.ctypes.data, tp, n, base, cost.ctypes.data,
                              length.ctypes.data, p_off.ctypes.data, path.ctypes.data, m_off.ctypes.data,
                              fmap.ctypes.data if want_map else None, 0)
    return rc, cost, length, path, fmap, p_off, m_off


def _check_against_ref(sets, src_idx, tgt_idx, out, exact_cost=True, base=0):
    """Every pair of a call equal to the restatement, element for element; slots beyond what a pair wrote untouched.
    Returns the number of pairs whose reference backtrace met a tie."""
    rc, cost, length, path, fmap, p_off, m_off = out
    assert rc == nat.SSYM_OK, nat.lib().ssym_last_error(sets.e.ctx)
    tied = 0
    for p in range(len(src_idx)):
        t = p if tgt_idx is None else int(tgt_idx[p])
        p0, p1, m0, m1 = int(p_off[p]), int(p_off[p + 1]), int(m_off[p]), int(m_off[p + 1])
        if int(src_idx[p]) == nat.NO_MATCH:
            want_cost, want_path, want_map, ties = float("inf"), np.zeros((0, 2), np.int64), np.zeros(0, np.int64), 0
        else:
            want_cost, want_path, want_map, ties = sets.ref(int(src_idx[p]) - base, t, want_ties=True)
        tied += int(ties > 0)
        L = want_path.shape[0]
        assert int(length[p]) == L, (p, int(length[p]), L)
        if exact_cost:
            assert _bits(cost[p]) == _bits(want_cost), (p, cost[p], want_cost)
        else:
            assert (np.isinf(want_cost) and np.isinf(cost[p])) or abs(cost[p] - want_cost) <= 1e-12 * abs(want_cost)
        assert np.array_equal(path[p0:p0 + L].astype(np.int64), want_path), p
        assert (path[p0 + L:p1] == SENT32).all(), p                       # nothing beyond the path is written
        if L:
            assert np.array_equal(fmap[m0:m1].astype(np.int64), want_map), p
        else:
            assert (fmap[m0:m1] == SENT32).all(), p
    return tied


def _int_segments(rng, n, lo, hi, dim, amp):
    return [rng.integers(-amp, amp + 1, size=(int(rng.integers(lo, hi + 1)), dim)).astype(np.float64) for _ in range(n)]


# ---- 1. exactness where the arithmetic is exact ---------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("dim", [1, 2])
def test_integer_features_equal_the_restatement_with_real_ties(dim, dtype):
    rng = np.random.default_rng(0x71E5 + dim)
    src = _int_segments(rng, 40, 2, 40, dim, 1)
    tgt = _int_segments(rng, 40, 2, 40, dim, 1)
    # digital silence on both sides, and silence inside a sound
    src += [np.zeros((17, dim)), np.zeros((70, dim)), np.concatenate([src[0], np.zeros((30, dim)), src[1]])]
    tgt += [np.zeros((33, dim)), np.zeros((9, dim)), np.concatenate([tgt[0], np.zeros((25, dim)), tgt[1]])]
    s = _Sets(src, tgt, dim, dtype=dtype, squared=True)
    idx = np.arange(len(src), dtype=np.uint32)
    tied = _check_against_ref(s, idx, None, _raw(s, idx))
    # every silence block against every other
    pairs = [(a, b) for a in (40, 41, 42) for b in (40, 41, 42)]
    si, ti = np.array([a for a, _ in pairs], np.uint32), np.array([b for _, b in pairs], np.uint32)
    _check_against_ref(s, si, ti, _raw(s, si, ti))
    s.close()
    print("pairs whose reference backtrace met a tie: %d of %d" % (tied, len(src)))
    assert tied >= 36, tied                          # the tie rule is exercised, not just stated


# ---- 2. real-valued features, both cost modes --------------------------------------------------------------------------

def _check_real_valued(s, src_idx, tgt_idx, oracle, matrix):
    rc, cost, length, path, fmap, p_off, m_off = _raw(s, src_idx, tgt_idx)
    assert rc == nat.SSYM_OK
    differ = []
    for p in range(len(src_idx)):
        a, b = np.asarray(s.src[src_idx[p]], np.float64), np.asarray(s.tgt[tgt_idx[p]], np.float64)
        want = oracle.dtw(a.reshape(-1), b.reshape(-1), s.dim, band=s.band, squared=s.squared)
        assert _bits(cost[p]) == _bits(matrix[src_idx[p], tgt_idx[p]]), p      # the bits of ssym_pair_matrix(exact = 1)
        if not np.isfinite(want):
            assert np.isinf(cost[p]) and length[p] == 0
            continue
        assert abs(cost[p] - want) <= 1e-12 * abs(want)
        L = int(length[p])
        got = path[int(p_off[p]):int(p_off[p]) + L].astype(np.int64)
        ref.check_path(got, a.shape[0], b.shape[0], s.band)
        m = fmap[int(m_off[p]):int(m_off[p + 1])].astype(np.int64)
        assert np.array_equal(m, ref.frame_map(got, b.shape[0]))
        assert abs(ref.resum(a, b, got, s.squared) - want) <= 1e-12 * abs(want)        # optimal, whatever the tie rule
        rcost, rpath, _ = s.ref(int(src_idx[p]), int(tgt_idx[p]))
        if _bits(rcost) != _bits(cost[p]):
            differ.append(p)
        assert np.array_equal(got, rpath), (p, "cost bits differ" if differ and differ[-1] == p else "same cost bits")
    print("pairs whose cost differs in bits from the restatement's: %d of %d %s" % (len(differ), len(src_idx), differ))


@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("shape", [(100, 128, 100, 128, 13, -1), (5, 40, 5, 40, 12, -1), (200, 256, 200, 256, 40, 32)])
def test_real_valued_features_optimal_path_and_bit_equal_cost(shape, squared, oracle):
    fa_lo, fa_hi, fb_lo, fb_hi, dim, band = shape
    rng = np.random.default_rng(0x2EA1 + dim)
    src = [rng.standard_normal((int(rng.integers(fa_lo, fa_hi + 1)), dim)).astype(np.float32) for _ in range(10)]
    tgt = [rng.standard_normal((int(rng.integers(fb_lo, fb_hi + 1)), dim)).astype(np.float32) for _ in range(8)]
    s = _Sets(src, tgt, dim, dtype="f32", band=band, squared=squared)
    matrix = s.e.pair_matrix(s.d, s.q, exact=True)
    si = np.repeat(np.arange(10, dtype=np.uint32), 8)
    ti = np.tile(np.arange(8, dtype=np.uint32), 10)
    _check_real_valued(s, si, ti, oracle, matrix)
    s.close()


# ---- 3. shapes ---------------------------------------------------------------------------------------------------------

EDGE_SHAPES = [  # (source frames lo..hi, target frames lo..hi, dim, band): test_gpu_exact.py's edges and dims
    (1, 70, 1, 70, 13, -1), (100, 200, 250, 300, 13, -1), (60, 130, 120, 135, 12, -1), (250, 256, 380, 390, 13, -1),
    (64, 64, 128, 128, 14, -1), (65, 65, 129, 129, 48, -1), (63, 66, 127, 130, 1, -1), (120, 140, 60, 70, 40, -1),
    (190, 200, 190, 200, 64, -1),
]


@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_shape_edges_unbanded(shape):
    fa_lo, fa_hi, fb_lo, fb_hi, dim, band = shape
    rng = np.random.default_rng(0x5A9E + dim + fa_lo)
    src, tgt = _int_segments(rng, 6, fa_lo, fa_hi, dim, 3), _int_segments(rng, 5, fb_lo, fb_hi, dim, 3)
    s = _Sets(src, tgt, dim, band=band, squared=True)
    si, ti = np.repeat(np.arange(6, dtype=np.uint32), 5), np.tile(np.arange(5, dtype=np.uint32), 6)
    _check_against_ref(s, si, ti, _raw(s, si, ti))
    s.close()


@pytest.mark.parametrize("dim", [13, 40])
@pytest.mark.parametrize("band", [0, 3, 32])
def test_banded_pairs_reachable_and_not(band, dim):
    rng = np.random.default_rng(0xBA2D + band + dim)
    src, tgt = [], []
    for k in range(24):
        fa = int(rng.integers(1, 300))
        fb = max(1, fa + int(rng.integers(-band, band + 1)))          # reachable: |Fa - Fb| <= r
        if k % 6 == 5:
            fb = fa + band + 1 + int(rng.integers(0, 40))             # kept on purpose: the band cuts the end cell
        src.append(rng.integers(-3, 4, size=(fa, dim)).astype(np.float64))
        tgt.append(rng.integers(-3, 4, size=(fb, dim)).astype(np.float64))
    s = _Sets(src, tgt, dim, band=band, squared=True)
    idx = np.arange(24, dtype=np.uint32)
    out = _raw(s, idx)
    _check_against_ref(s, idx, None, out)
    length, cost = out[2], out[1]
    assert (length[5::6] == 0).all() and np.isinf(cost[5::6]).all() and (length[np.arange(24) % 6 != 5] > 0).all()
    if band == 0:
        for p in np.flatnonzero(length):
            L = int(length[p])
            cells = out[3][int(out[5][p]):int(out[5][p]) + L]
            assert np.array_equal(cells[:, 0], np.arange(L)) and np.array_equal(cells[:, 1], np.arange(L))
    s.close()


def test_one_frame_empty_and_lopsided_segments():
    rng = np.random.default_rng(0x10B5)
    dim = 12
    mk = lambda f: rng.integers(-3, 4, size=(f, dim)).astype(np.float64)
    src = [mk(1), mk(0), mk(1), mk(700), mk(3), mk(64), mk(129)]
    tgt = [mk(1), mk(5), mk(0), mk(2), mk(900), mk(1), mk(65)]
    s = _Sets(src, tgt, dim, squared=True)
    si, ti = np.repeat(np.arange(7, dtype=np.uint32), 7), np.tile(np.arange(7, dtype=np.uint32), 7)
    out = _raw(s, si, ti)
    _check_against_ref(s, si, ti, out)
    assert (out[2][(si == 1) | (ti == 2)] == 0).all() and np.isinf(out[1][(si == 1) | (ti == 2)]).all()
    s.close()


def test_direction_matrix_on_either_side_of_the_lds_boundary_and_at_the_frame_limit():
    lds, limit = _const("kAlignDirLdsBytes"), _const("kAlignMaxFrames")
    assert lds % 64 == 0 and limit == 4096
    rng = np.random.default_rng(0x1D5)
    dim = 2
    mk = lambda f: rng.integers(-2, 3, size=(f, dim)).astype(np.float64)
    fb = 250                                       # ceil(250 / 16) = 16 dwords per row
    under = lds // (16 * 4)                        # Fa * 16 * 4 == lds: the last pair that stays in LDS
    src = [mk(under), mk(under + 1), mk(limit), mk(40), mk(limit)]
    tgt = [mk(fb), mk(fb), mk(40), mk(limit), mk(limit)]
    s = _Sets(src, tgt, dim, squared=True)
    for group in ([0, 1], [2], [3], [4], [0, 1, 2, 3]):       # alone and mixed: LDS and scratch pairs in one call
        idx = np.array(group, dtype=np.uint32)
        _check_against_ref(s, idx, idx, _raw(s, idx, idx))
    s.close()
    # beyond the limit: refused before any device work
    s = _Sets([mk(limit + 1), mk(3)], [mk(3), mk(limit + 1)], dim, squared=True)
    for group in ([0], [1]):
        idx = np.array(group, dtype=np.uint32)
        out = _raw(s, idx, idx)
        assert out[0] == nat.SSYM_E_UNSUPPORTED and b"4096" in nat.lib().ssym_last_error(s.e.ctx)
        assert (out[1] == SENTF).all() and (out[2] == SENT32).all() and (out[3] == SENT32).all()
    s.close()


def test_long_banded_pair_through_global_scratch():
    rng = np.random.default_rng(0x6B)
    mk = lambda f: rng.integers(-3, 4, size=(f, 13)).astype(np.float64)
    s = _Sets([mk(1500), mk(1490)], [mk(1520), mk(1400)], 13, band=32, squared=True)
    idx = np.array([0, 1], dtype=np.uint32)
    out = _raw(s, idx)
    _check_against_ref(s, idx, None, out)
    assert out[2][0] > 0 and out[2][1] == 0
    s.close()


# ---- 4. pairing and batch ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_pairings_index_base_no_match_and_device_outputs(dtype):
    rng = np.random.default_rng(0x9A12)
    dim = 13
    src, tgt = _int_segments(rng, 9, 1, 90, dim, 3), _int_segments(rng, 7, 1, 90, dim, 3)
    s = _Sets(src, tgt, dim, dtype=dtype, squared=True)
    first = np.array([3, 0, 8, 8, 1, 2, 5], dtype=np.uint32)
    a = _raw(s, first)                                               # tgt_idx = NULL: pair p uses target p
    b = _raw(s, first, np.arange(7, dtype=np.uint32))
    _check_against_ref(s, first, None, a)
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)
    short = _raw(s, first[:3])                                       # fewer pairs than targets
    _check_against_ref(s, first[:3], None, short)
    # repeats, any pairing, SSYM_NO_MATCH, index_base = 1
    si = np.array([4, 4, 9, nat.NO_MATCH, 1, 4, nat.NO_MATCH, 9], dtype=np.uint32)
    ti = np.array([6, 6, 0, 2, 5, 6, 0, 0], dtype=np.uint32)
    out = _raw(s, si, ti, base=1)
    _check_against_ref(s, si, ti, out, base=1)
    assert np.isinf(out[1][[3, 6]]).all() and (out[2][[3, 6]] == 0).all()
    # device outputs, with and without the map
    dev = _raw(s, si, ti, base=1, device=True)
    for x, y in zip(out[1:5], dev[1:5]):
        assert np.array_equal(x, y)
    nomap = _raw(s, si, ti, base=1, want_map=False)
    devnomap = _raw(s, si, ti, base=1, want_map=False, device=True)
    for o in (nomap, devnomap):
        assert o[0] == nat.SSYM_OK and np.array_equal(o[3], out[3]) and np.array_equal(o[2], out[2])
        assert (o[4] == SENT32).all()
    # offsets with more room than asked for, not starting at 0
    p_off, m_off = out[5] * np.uint64(2) + np.uint64(5), out[6] + np.arange(9, dtype=np.uint64) * np.uint64(3) + np.uint64(2)
    wide = _raw(s, si, ti, base=1, offsets=(p_off, m_off))
    assert wide[0] == nat.SSYM_OK and (wide[3][:5] == SENT32).all() and (wide[4][:2] == SENT32).all()
    for p in range(8):
        L = int(out[2][p])
        assert np.array_equal(wide[3][int(p_off[p]):int(p_off[p]) + L], out[3][int(out[5][p]):int(out[5][p]) + L])
        assert (wide[3][int(p_off[p]) + L:int(p_off[p + 1])] == SENT32).all()
    # the Python layer
    cost, length, paths, maps = s.e.dtw_align(s.d, s.q, si, ti, index_base=1)
    assert np.array_equal(cost, out[1]) and np.array_equal(length, out[2])
    for p in range(8):
        assert np.array_equal(paths[p], out[3][int(out[5][p]):int(out[5][p]) + int(out[2][p])])
        assert maps[p].size == (tgt[ti[p]].shape[0] if out[2][p] else 0)
    assert s.e.dtw_align(s.d, s.q, si, ti, index_base=1, want_map=False)[3] is None
    s.close()


def test_4096_pairs_in_one_call_equal_one_call_each_and_any_order():
    rng = np.random.default_rng(0x4096)
    dim = 13
    src = [rng.standard_normal((int(rng.integers(5, 41)), dim)).astype(np.float32) for _ in range(96)]
    tgt = [rng.standard_normal((int(rng.integers(5, 41)), dim)).astype(np.float32) for _ in range(64)]
    s = _Sets(src, tgt, dim, dtype="f32")
    si = rng.integers(0, 96, size=4096).astype(np.uint32)
    ti = rng.integers(0, 64, size=4096).astype(np.uint32)
    cost, length, paths, maps = s.e.dtw_align(s.d, s.q, si, ti)
    again = s.e.dtw_align(s.d, s.q, si, ti)
    assert np.array_equal(_bits(cost), _bits(again[0])) and np.array_equal(length, again[1])
    assert all(np.array_equal(x, y) for x, y in zip(paths, again[2])) and all(np.array_equal(x, y) for x, y in zip(maps, again[3]))
    order = rng.permutation(4096)
    shuf = s.e.dtw_align(s.d, s.q, si[order], ti[order])
    assert np.array_equal(_bits(shuf[0]), _bits(cost[order])) and np.array_equal(shuf[1], length[order])
    assert all(np.array_equal(shuf[2][k], paths[order[k]]) and np.array_equal(shuf[3][k], maps[order[k]]) for k in range(4096))
    for p in range(4096):
        c1, l1, p1, m1 = s.e.dtw_align(s.d, s.q, si[p:p + 1], ti[p:p + 1])
        assert _bits(c1[0]) == _bits(cost[p]) and l1[0] == length[p]
        assert np.array_equal(p1[0], paths[p]) and np.array_equal(m1[0], maps[p])
    for p in range(0, 4096, 97):                                     # and they are the restatement's
        _, rpath, rmap = s.ref(int(si[p]), int(ti[p]))
        assert np.array_equal(paths[p].astype(np.int64), rpath) and np.array_equal(maps[p].astype(np.int64), rmap)
    s.close()


def test_sets_made_from_device_frames():
    import torch
    rng = np.random.default_rng(0xDF)
    dim = 12
    src, tgt = _int_segments(rng, 5, 3, 80, dim, 3), _int_segments(rng, 5, 3, 80, dim, 3)
    host = _Sets(src, tgt, dim, squared=True)
    want = host.e.dtw_align(host.d, host.q, np.arange(5))
    sf, so = pack_segments(src, dim, np.float64)
    tf, to = pack_segments(tgt, dim, np.float64)
    ds, dt = torch.from_numpy(sf).cuda(), torch.from_numpy(tf).cuda()
    d = host.e.dictionary(DeviceFrames(ds.data_ptr(), sf.size // dim, dim, ds), so, dim)
    q = host.e.queries(DeviceFrames(dt.data_ptr(), tf.size // dim, dim, dt), to, dim)
    got = host.e.dtw_align(d, q, np.arange(5))
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])
    assert all(np.array_equal(x, y) for x, y in zip(got[2], want[2])) and all(np.array_equal(x, y) for x, y in zip(got[3], want[3]))
    host.close()


# ---- 5. end to end on the recordings -----------------------------------------------------------------------------------

def test_align_on_the_reference_recordings(oracle):
    from soundsym_amd import io as sio
    from soundsym_amd.api import HOP, NCOEFFS, frame_features
    gold = os.path.join(ROOT, "tests", "golden")
    e = Engine(metric="dtw", dtype="f64")
    s_smp, srate = sio.read_wav(os.path.join(gold, "audio", "sample.wav"))
    t_smp, rate = sio.read_wav(os.path.join(gold, "audio", "Section_7_1.wav"))
    seg = 16 * HOP
    lens = [seg] * (s_smp.size // seg) + ([s_smp.size % seg] if s_smp.size % seg else [])
    source = Sound(s_smp, srate, frame_features(s_smp, srate, engine=e))
    dictionary = SoundDictionary.from_segments(source, lens, engine=e)
    dictionary.sounds = [x for x in dictionary.sounds if x.num_frames() > 0]
    targets = []
    for a, b, label in sio.audacity_labels_to_timestamps(os.path.join(gold, "vowel.txt")):
        piece = t_smp[int(round(a * rate)):int(round(b * rate)) + 1]
        if piece.size >= HOP:
            targets.append(Sound(piece, rate, frame_features(piece, rate, engine=e), label))
    assert len(dictionary.sounds) == 284 and len(targets) == 55
    idx, cost = dictionary.match_indices(targets)
    al = dictionary.align(targets)
    assert len(al) == 55 and len(SoundSequence.new(targets).align_to_dictionary(dictionary)) == 55
    for t, x in enumerate(al):
        assert x.source_index == int(idx[t]) and _bits(x.cost) == _bits(cost[t])
        a = dictionary.sounds[x.source_index].mfccs().reshape(-1, NCOEFFS)
        b = targets[t].mfccs().reshape(-1, NCOEFFS)
        want = oracle.dtw(a.reshape(-1), b.reshape(-1), NCOEFFS)
        path = x.path.astype(np.int64)
        ref.check_path(path, a.shape[0], b.shape[0])
        assert np.array_equal(x.frame_map.astype(np.int64), ref.frame_map(path, b.shape[0]))
        assert abs(x.cost - want) <= 1e-12 * abs(want) and abs(ref.resum(a, b, path) - want) <= 1e-12 * abs(want)
        assert 0.0 <= x.diagonal_share() <= 1.0
    chosen = dictionary.align(targets[:5], indices=[0, 7, 7, 283, 1])
    assert [c.source_index for c in chosen] == [0, 7, 7, 283, 1] and all(len(c) > 0 for c in chosen)
    e.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------

def _untouched(out):
    return (out[1] == SENTF).all() and (out[2] == SENT32).all() and (out[3] == SENT32).all() and (out[4] == SENT32).all()


def test_every_listed_error_leaves_the_outputs_untouched():
    rng = np.random.default_rng(0xE77)
    dim = 12
    src, tgt = _int_segments(rng, 4, 2, 20, dim, 2), _int_segments(rng, 3, 2, 20, dim, 2)
    s = _Sets(src, tgt, dim, squared=True)
    L, ctx = nat.lib(), s.e.ctx
    idx = np.array([0, 1, 2], dtype=np.uint32)
    good = _raw(s, idx)
    assert good[0] == nat.SSYM_OK
    p_off, m_off = good[5], good[6]

    def call(d=s.d.ptr, q=s.q.ptr, src_idx=idx, tgt_idx=None, n=3, base=0, poff=p_off, moff=m_off, null=()):
        cost, length = np.full(3, SENTF), np.full(3, SENT32, dtype=np.uint32)
        path, fmap = np.full((int(p_off[-1]) + 8, 2), SENT32, dtype=np.uint32), np.full(int(m_off[-1]) + 8, SENT32, dtype=np.uint32)
        ptr = lambda name, arr: None if name in null or arr is None else arr.ctypes.data
        rc = L.ssym_dtw_align(ctx, d, q, ptr("src", src_idx), ptr("tgt", tgt_idx), n, base, ptr("cost", cost),
                              ptr("len", length), ptr("poff", poff), ptr("path", path), ptr("moff", moff),
                              ptr("map", fmap), 0)
        assert _untouched((rc, cost, length, path, fmap)), rc
        return rc

    inv = nat.SSYM_E_INVALID
    assert call(d=None) == inv and call(q=None) == inv
    for name in ("src", "cost", "len", "poff", "path", "moff"):
        assert call(null=(name,)) == inv, name
        assert L.ssym_last_error(ctx)
    assert call(src_idx=np.array([0, 4, 1], dtype=np.uint32)) == inv                      # beyond the dictionary
    assert call(src_idx=np.array([1, 2, 0], dtype=np.uint32), base=1) == inv              # below index_base
    assert call(tgt_idx=np.array([0, 3, 1], dtype=np.uint32)) == inv                      # beyond the targets
    assert call(src_idx=np.array([0, 1, 2, 3], dtype=np.uint32), n=4, poff=np.zeros(5, np.uint64), moff=np.zeros(5, np.uint64)) == inv   # NULL tgt_idx, 4 pairs, 3 targets
    bad = p_off.copy(); bad[2] -= np.uint64(1); bad[3] -= np.uint64(1)
    assert call(poff=bad) == inv                                                          # too small for pair 1
    bad = p_off.copy(); bad[1], bad[2] = p_off[2], p_off[1]
    assert call(poff=bad) == inv                                                          # decreasing
    bad = m_off.copy(); bad[3] -= np.uint64(1)
    assert call(moff=bad) == inv
    # a set of another dimension
    other = s.e.queries(np.zeros(3 * 13), np.array([0, 1, 2, 3], dtype=np.uint64), 13)
    assert call(q=other.ptr) == inv
    # an empty dictionary
    empty = s.e.dictionary(np.zeros(0), np.zeros(1, dtype=np.uint64), dim)
    assert call(d=empty.ptr) == nat.SSYM_E_EMPTY_DICT
    assert L.ssym_dtw_align_sizes(empty.ptr, s.q.ptr, idx.ctypes.data, None, 3, 0, p_off.copy().ctypes.data,
                                  m_off.copy().ctypes.data) == nat.SSYM_E_EMPTY_DICT
    # n_pairs = 0 succeeds and does nothing, even with nothing to write to
    assert call(n=0) == nat.SSYM_OK
    assert L.ssym_dtw_align(ctx, s.d.ptr, s.q.ptr, None, None, 0, 0, None, None, None, None, None, None, 0) == nat.SSYM_OK
    # _sizes holds the same index checks
    assert L.ssym_dtw_align_sizes(s.d.ptr, s.q.ptr, np.array([9], np.uint32).ctypes.data, None, 1, 0,
                                  p_off.copy().ctypes.data, m_off.copy().ctypes.data) == inv
    # dim beyond the kernel's registers
    s.close()
    wide = _Sets([np.zeros((3, 65))], [np.zeros((3, 65))], 65)
    out = _raw(wide, np.array([0], dtype=np.uint32))
    assert out[0] == nat.SSYM_E_UNSUPPORTED and _untouched(out)
    wide.close()


def test_a_refcos_context_is_refused():
    rng = np.random.default_rng(1)
    s = _Sets([rng.standard_normal((5, 12))], [rng.standard_normal((6, 12))], 12, metric="refcos")
    out = _raw(s, np.array([0], dtype=np.uint32))
    assert out[0] == nat.SSYM_E_UNSUPPORTED and _untouched(out)
    assert b"refcos" in nat.lib().ssym_last_error(s.e.ctx)
    with pytest.raises(nat.SsymError):
        s.e.dtw_align(s.d, s.q, [0])
    s.close()
