"""ssym_dtw_cover with more targets than its grids have workgroups, on targets longer than its ring, and where the chain's
lanes tie: 65 599 targets in one call, so that cover_forward_kernel's grid z (65535) and
cover_chain_kernel's 8 workgroups per CU both take a second target -- the two targets run through every ordered pair of 8
kinds for either stride (tests/count_cases.py, checked in tests/test_count_cases.py) --; targets of 511, 512, 513 and 1300
frames held to tests/cover_ref.py directly; and dictionaries with W > 64 whose tilings tie across the wave's lanes.  Bit
for bit against tests/cover_ref.py, which runs over the distinct targets once."""
import numpy as np
import pytest

import count_cases as cc
import cover_ref as ref
import coverer_gpu as cg
from cover_gpu import Sets, check, pieces_of, same

pytestmark = pytest.mark.gpu


def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def big():
    c = cc.cover_case(num_cus())
    c.want = cc.gather_cover(c.want_u, c.frames, c.ids)
    return c


@pytest.fixture(scope="module")
def sets(big):
    with Sets(big.src, big.tgt, big.dim) as s:
        yield s


def test_65599_targets_are_covered(big, sets):
    g = cc.chain_stride(num_cus())
    assert len(big.tgt) == cc.FORWARD_STRIDE + 64 > g + 64
    count = check(sets, cc.COVER_PENALTY, want=big.want)[0]
    for stride in (g, cc.FORWARD_STRIDE):
        assert ((count[:64] == 0) & (count[stride:stride + 64] > 0)).any()       # a cover after none, in one workgroup
    check(sets, cc.COVER_PENALTY, want=big.want, device=True)


@pytest.mark.parametrize("knobs", [{"SSYM_COVER_BLOCK": "2"}, {"SSYM_COVER_STARTS": "24"}])
def test_no_launch_shape_matters_beyond_the_grid(big, sets, knobs, monkeypatch):
    """Several source blocks (a fold over every entry of the tables) and 24 starts per workgroup: the same bits."""
    with monkeypatch.context() as mp:
        for k, v in knobs.items():
            mp.setenv(k, v)
        check(sets, cc.COVER_PENALTY, want=big.want)


@pytest.fixture(scope="module")
def long():
    segs, tgt = cc.long_case()
    tabs = ref.all_tables(segs, tgt)
    return segs, tgt, {p: ref.arrays(segs, tgt, p, tabs=tabs) for p in (0.0, 2.0)}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_targets_around_and_beyond_the_ring(long, dtype):
    segs, tgt, want = long
    with Sets(segs, tgt, 3, dtype) as s:
        for penalty in (0.0, 2.0):
            got = check(s, penalty, want=want[penalty])
            assert (got[0] > 30).all() and all(pieces_of(got, tgt, t)[-1][2] == x.shape[0] - 1 for t, x in enumerate(tgt))
        same(check(s, 2.0, want=want[2.0], device=True), want[2.0])


@pytest.mark.parametrize("fmax", [40, 128])
def test_ties_across_the_waves_lanes(fmax):
    """Totals that count the pieces: at the end of a long run many last pieces tie, in different lanes of the chain's wave,
    and the shortest one sits in a higher lane than another (tests/test_count_cases.py holds that).  The cover's chain
    and, through a one-lane coverer fed 7 frames at a time, the coverer's."""
    segs, x, penalty = cc.tie_case(fmax)
    want = ref.arrays(segs, [x], penalty)
    with Sets(segs, [x], 2) as s:
        got = check(s, penalty, want=want)
        pieces = pieces_of(got, [x], 0)
    assert len(pieces) == want[0][0] > 3
    with cg.Dict(segs, 2) as D:
        live = cg.Live(D, 1, penalty)
        for a in range(0, x.shape[0], 7):
            live.push([x[a:a + 7]])
        live.flush()
        cg.same_pieces(live.emitted[0], pieces)
        assert np.array(live.cv.best()[0][0]).view(np.uint64) == np.array(want[1][0]).view(np.uint64)
        live.close()
