"""ssym_dtw_cover at the smallest shapes at which its kernels can still go wrong: targets at the
edges of the starts a workgroup takes, whatever that number is forced to; sources of 1, 2, 3, 63, 64, 65 and
kCoverMaxSourceFrames frames with an empty one in one dictionary; a target shorter than every source's shortest window;
every width of frame the layouts distinguish; and source blocks, strips and starts of every size giving the same bits."""
import numpy as np
import pytest

import cover_ref as ref
from cover_gpu import INF, Sets, call, check, real, same
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

MAX_FRAMES = 128            # kCoverMaxSourceFrames (tests/test_cover_api.py reads it from the source)
# 1, 2, 63, 64, 65, 130 and the edges of 24 and 128 starts per workgroup
TARGET_FRAMES = (1, 2, 23, 24, 25, 63, 64, 65, 127, 128, 129, 130)


@pytest.fixture(scope="module")
def edges():
    """Sources of every edge length in one dictionary, targets of every edge length, and the restatement's tables."""
    class E:
        pass
    e = E()
    rng = np.random.default_rng(0xED6E)
    e.src = [real(rng, n, 13) for n in (1, 64, 3, 0, 63, 2, MAX_FRAMES, 65)]
    e.tgt = [real(rng, n, 13) for n in TARGET_FRAMES]
    e.tabs = ref.all_tables(e.src, e.tgt)
    e.want = {p: ref.arrays(e.src, e.tgt, p, tabs=e.tabs) for p in (0.0, 3.0)}
    return e


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_edge_lengths_of_sources_and_targets(edges, dtype):
    with Sets(edges.src, edges.tgt, 13, dtype) as sets:
        got = check(sets, want=edges.want[0.0])
        assert (got[0] > 0).all()                               # the 1-frame source covers everything, at a price
        got = check(sets, 3.0, want=edges.want[3.0])
        assert (got[0] <= edges.want[0.0][0]).all() and got[0][-1] < edges.want[0.0][0][-1]
        check(sets, 3.0, want=edges.want[3.0], device=True)


KNOBS = ({"SSYM_COVER_STARTS": "24"}, {"SSYM_COVER_STARTS": "128"}, {"SSYM_COVER_STARTS": "1"}, {"SSYM_COVER_STARTS": "64"},
         {"SSYM_COVER_BLOCK": "1"}, {"SSYM_COVER_BLOCK": "3"}, {"SSYM_COVER_BLOCK": "64"}, {"SSYM_COVER_STRIP": "1"},
         {"SSYM_COVER_STRIP": "7"}, {"SSYM_COVER_STARTS": "24", "SSYM_COVER_BLOCK": "2", "SSYM_COVER_STRIP": "5"}, {})


def test_no_launch_shape_matters(edges, monkeypatch):
    """Starts per workgroup, sources per block and columns per strip, forced through the hooks: the same bits."""
    with Sets(edges.src, edges.tgt, 13) as sets:
        base = check(sets, want=edges.want[0.0])
        for knobs in KNOBS:
            with monkeypatch.context() as mp:
                for k, v in knobs.items():
                    mp.setenv(k, v)
                same(check(sets, want=edges.want[0.0]), base)
        with monkeypatch.context() as mp:                       # a production process is not steered by a stray variable
            mp.setenv("SSYM_TEST_HOOKS", "0")
            mp.setenv("SSYM_COVER_STARTS", "3")
            same(check(sets, want=edges.want[0.0]), base)


def test_short_sources_take_the_wide_layout_and_blocks_fold_in_index_order(monkeypatch):
    """A dictionary of short sources only (64 starts, one strip) with every segment twice: the lower index wins across
    source blocks of every size."""
    rng = np.random.default_rng(0xB10C)
    half = [real(rng, n, 5) for n in (5, 9, 1, 12, 7, 3, 16, 2, 11)]
    src = half + [s.copy() for s in half]
    tgt = [real(rng, n, 5) for n in (65, 130)] + [np.concatenate([half[3], half[0], np.repeat(half[4], 2, axis=0)])]
    want = ref.arrays(src, tgt)
    assert want[2][want[2] != ref.NONE].max() < len(half) and want[1][2] == 0.0
    with Sets(src, tgt, 5) as sets:
        for block in (None, "1", "2", "5", "9", "10", "18"):
            with monkeypatch.context() as mp:
                if block:
                    mp.setenv("SSYM_COVER_BLOCK", block)
                check(sets, want=want)


def test_a_target_shorter_than_every_sources_shortest_window():
    rng = np.random.default_rng(0x5407)
    src = [real(rng, n, 13) for n in (5, 9, MAX_FRAMES, 64, 7)]             # windows of at least 3 frames
    tgt = [real(rng, n, 13) for n in (2, 1, 3, 0, 4, 6)]
    with Sets(src, tgt, 13) as sets:
        got = check(sets)
        assert got[0].tolist()[:2] == [0, 0] and got[1][0] == INF and got[0][2] == 1 and got[0][3] == 0
        assert got[0][4] == 1                                               # 4 = 3 + 1 has no second piece
        assert got[0][5] >= 1


@pytest.mark.parametrize("dim", [1, 12, 13, 14, 15, 16, 17, 40, 41, 64])
def test_every_width_of_frame(dim):
    rng = np.random.default_rng(0xD1 + dim)
    src = [real(rng, n, dim) for n in (4, 9, 1, 17, 6)]
    tgt = [real(rng, n, dim) for n in (66, 5)]
    for squared in (False, True):
        with Sets(src, tgt, dim, "f64", squared) as sets:
            got = check(sets)
            assert (got[0] > 0).all()


def test_the_context_keeps_no_state_between_calls(edges):
    """A long call, a short one and the long one again on one context (the scratch is reused and shrinks in use)."""
    with Sets(edges.src, edges.tgt, 13) as sets:
        first = check(sets, want=edges.want[0.0])
        small = sets.e.queries(*pack_segments(edges.tgt[:3], 13, np.float64), 13)
        count = sets.e.dtw_cover(sets.d, small, 1.0)[0]
        assert count.tolist() == ref.arrays(edges.src, edges.tgt[:3], 1.0)[0].tolist()
        rc, again, untouched = call(sets)
        assert rc == nat.SSYM_OK and untouched
        same(again, first)
