"""Paced matching at every shape where its kernel takes another path, bit for bit against tests/paced_match_ref.py: packs
that end exactly at lane 63 and one-frame sources next to 63-frame ones, 64-row chunks and their hand-off rows, the target
ring's refills at 64 and 128 columns, the limits and the first shapes beyond them, every DIMR and its padding, packed
against unpacked and every source-block size (the result must not depend on how sources fall into packs and blocks),
and the fold's corners."""
import numpy as np
import pytest

import paced_match_ref as ref
from paced_match_gpu import (INF, NAN, SENTF, Sets, align_costs, bits, check_match, check_matrix, error, match, matrix, real,
                             same_as_align, same_bits)
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu

# the order packs a 1-frame source next to a 63-frame one (1 + 63 = 64: the pack ends exactly at lane 63), 31 + 33 and
# 32 + 32 as well; 15 + 16 + 17 + 2 leaves room, 64 fills a wave alone, 65 ... 129 run in chunks
SRC_FRAMES = [1, 63, 31, 33, 32, 32, 15, 16, 17, 2, 64, 65, 127, 128, 129, 63, 1, 64]
TGT_FRAMES = [1, 2, 3, 33, 64, 65, 130]


class _Edges:
    def __init__(self):
        rng = np.random.default_rng(0xED6E5)
        self.src = [real(rng, f, 13) for f in SRC_FRAMES]
        self.tgt = [real(rng, f, 13) for f in TGT_FRAMES]
        self.want = ref.matrix(self.src, self.tgt)
        self.distance = np.array([1.0, 2.0, 9.0, 150.0, 330.0, 300.0, 700.0])


@pytest.fixture(scope="module")
def edges():
    return _Edges()


def test_pack_and_chunk_edges(edges):
    assert sorted(set(SRC_FRAMES)) == [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129]
    assert np.isfinite(edges.want).any(axis=0).all() and np.isfinite(edges.want[11:15]).any()
    for dtype in ("f64", "f32"):
        with Sets(edges.src, edges.tgt, 13, dtype) as sets:
            mat = check_matrix(sets, edges.want)
            same_as_align(mat, align_costs(sets)[0])
            check_match(sets, edges.want)
            check_match(sets, edges.want, edges.distance, base=11)


def test_one_pair_at_the_limits():
    rng = np.random.default_rng(0x4095)
    src, tgt = [real(rng, 4095, 3)], [real(rng, 2048, 3)]
    want = ref.matrix(src, tgt)
    assert np.isfinite(want[0, 0])
    with Sets(src, tgt, 3) as sets:
        check_matrix(sets, want)
        idx, cost = check_match(sets, want, base=2)
        acost, alen, _, _ = sets.e.dtw_align(sets.d, sets.q, [0], step="paced")
        assert alen[0] == 2048 and bits(acost[0]) == bits(cost[0])


@pytest.mark.parametrize("frames,side", [(2049, "tgt"), (4097, "src")])
def test_the_first_shapes_beyond_the_limits_are_refused(frames, side):
    small = [np.zeros((3, 2)), np.zeros((5, 2))]
    big = [np.zeros((frames, 2))]
    with Sets(small + (big if side == "src" else []), small + (big if side == "tgt" else []), 2) as sets:
        assert match(sets)[0::3] == (nat.SSYM_E_UNSUPPORTED, True)
        assert error(sets).startswith("ssym_match_queries_step: ")
        assert match(sets, device=True)[0::3] == (nat.SSYM_E_UNSUPPORTED, True)
        assert matrix(sets)[0::2] == (nat.SSYM_E_UNSUPPORTED, True)
        assert error(sets).startswith("ssym_pair_matrix_step: ")
        assert sets.e.timings()["n_pairs"] == 0                      # no call got as far as its timings


@pytest.mark.parametrize("dim", [1, 14, 15, 16, 17, 40, 41, 64])
def test_every_dimr(dim):
    rng = np.random.default_rng(0xD1 + dim)
    src = [real(rng, f, dim) for f in (9, 30, 25, 1, 70, 40, 12, 33, 64)]
    tgt = [real(rng, f, dim) for f in (20, 40, 1, 66)]
    want = ref.matrix(src, tgt)
    for squared in (False, True):
        w = want if not squared else ref.matrix(src, tgt, True)
        with Sets(src, tgt, dim, squared=squared) as sets:
            mat = check_matrix(sets, w)
            same_as_align(mat, align_costs(sets)[0])
            check_match(sets, w)


def _dups():
    """Identical sources on both sides of a pack edge and of a block edge: target D (24 frames); [X20, D, D, D, Y10, D] packs
    as X + D | D + D | Y + D (20 + 24 + 24 > 64) and, three sources to a block, splits between the second and third D."""
    rng = np.random.default_rng(0xD0B)
    d, x, y = real(rng, 24, 13), real(rng, 20, 13), real(rng, 10, 13)
    return [x, d, d.copy(), d.copy(), y, d.copy()], [d, real(rng, 15, 13)]


def test_packed_is_unpacked_and_no_block_size_matters(edges, monkeypatch):
    dsrc, dtgt = _dups()
    dwant = ref.matrix(dsrc, dtgt)
    with Sets(edges.src, edges.tgt, 13) as sets, Sets(dsrc, dtgt, 13) as dups, Sets(dsrc[2:], dtgt, 13) as dups2:
        base = match(sets, edges.distance, 4)
        base_mat = matrix(sets)[1]
        for knobs in ({"SSYM_PACED_MATCH_PACK": "0"}, {"SSYM_PACED_MATCH_BLOCK": "1"}, {"SSYM_PACED_MATCH_BLOCK": "3"},
                      {"SSYM_PACED_MATCH_BLOCK": "64"}, {"SSYM_PACED_MATCH_PACK": "0", "SSYM_PACED_MATCH_BLOCK": "5"}, {}):
            with monkeypatch.context() as mp:
                for k, v in knobs.items():
                    mp.setenv(k, v)
                mat = check_matrix(sets, edges.want)
                assert (bits(mat) == bits(base_mat)).all(), knobs
                got = match(sets, edges.distance, 4)
                assert got[0] == nat.SSYM_OK and np.array_equal(got[1], base[1]) and (bits(got[2]) == bits(base[2])).all(), knobs
                check_match(sets, edges.want)
                # the lowest index among identical sources, wherever packs and blocks end
                idx, cost = check_match(dups, dwant)
                assert idx[0] == 1 and bits(cost[0]) == bits(0.0), knobs
                idx, cost = check_match(dups2, dwant[2:])
                assert idx[0] == 0 and bits(cost[0]) == bits(0.0), knobs
                idx, _ = check_match(dups2, dwant[2:], base=9, device=True)
                assert idx[0] == 9, knobs


def test_the_folds_corners():
    rng = np.random.default_rng(0xF01D)
    src = [real(rng, 12, 13), np.zeros((0, 13)), real(rng, 10, 13), real(rng, 14, 13)]
    # 40 frames: no source fits (12 < 20); 0 frames: empty; 3 frames: none fits (10 > 5); 11 and 12: every source with frames fits
    tgt = [real(rng, 40, 13), np.zeros((0, 13)), real(rng, 3, 13), real(rng, 11, 13), real(rng, 12, 13)]
    want = ref.matrix(src, tgt)
    assert np.isinf(want[:, :3]).all() and np.isinf(want[1]).all() and np.isfinite(want[[0, 2, 3], 3:]).all()
    with Sets(src, tgt, 13) as sets:
        check_matrix(sets, want)
        idx, cost = check_match(sets, want, base=6)
        assert idx[:3].tolist() == [6, 6, 6] and np.isposinf(cost[:3]).all() and (idx[3:] != 7).all()
        idx, cost = check_match(sets, want, [0.0, 0.0, 0.0, NAN, INF], base=6, device=True)
        assert idx.tolist() == [6] * 5 and np.isposinf(cost).all()
        idx, cost = check_match(sets, want, [NAN, INF, -INF, -INF, 1e300])
        assert idx[3] == 0 and cost[3] == INF and np.isfinite(cost[4])
    # one source; and a thousand sources against one target
    with Sets(src[2:3], tgt, 13) as sets:
        check_match(sets, want[2:3], base=1)
    many = [real(rng, int(f), 5) for f in rng.integers(1, 30, size=1000)]
    many[700] = many[300].copy()
    one = [many[300][::2]]
    want = ref.matrix(many, one)
    with Sets(many, one, 5) as sets:
        check_matrix(sets, want)
        idx, cost = check_match(sets, want)
        assert idx[0] == 300 and bits(cost[0]) == bits(0.0)
        check_match(sets, want, [np.nanmax(np.where(np.isfinite(want), want, NAN))])
