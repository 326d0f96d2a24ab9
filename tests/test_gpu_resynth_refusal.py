"""What ssym_resynth_* refuses, and in which order, on the GPU: every refusal leaves the resynthesiser as it was (nothing
consumed, the next good call gives the restatement's samples)."""
import ctypes

import numpy as np
import pytest

import live_resynth_ref as ref
from resynth_gpu import G, Live, columns, same, tile
from soundsym_amd import Engine, SsymError
from soundsym_amd import _native as nat
from warp_ref import HOP

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = nat.SSYM_E_INVALID, nat.SSYM_E_UNSUPPORTED


@pytest.fixture(scope="module")
def rig():
    class R:
        pass
    r = R()
    rng = np.random.default_rng(0x4EF)
    r.sounds = [rng.normal(size=n) * 0.3 for n in (5000, 2600)]
    r.e = Engine(metric="dtw", dtype="f64", device=0)
    r.store = r.e.samples(np.concatenate(r.sounds), np.array([0, 5000, 7600], dtype=np.uint64))
    yield r
    r.store.close()
    r.e.close()


def _refused(call, code=INVALID, match=None):
    with pytest.raises(SsymError) as err:
        call()
    assert err.value.code == code, err.value
    if match:
        assert match in str(err.value), err.value


def test_create_refusals_come_in_their_order(rig):
    L, ctx, out = nat.lib(), rig.e.ctx, ctypes.c_void_p(7)
    err = lambda: L.ssym_last_error(ctx).decode()
    assert L.ssym_resynth_create(ctx, rig.store.ptr, 1, 0, None) == INVALID and "out is NULL" in err()
    assert L.ssym_resynth_create(ctx, None, 0, 513, ctypes.byref(out)) == INVALID and "NULL or n_lanes is 0" in err() and not out.value
    assert L.ssym_resynth_create(ctx, rig.store.ptr, 0, 513, ctypes.byref(out)) == INVALID and "n_lanes is 0" in err()
    assert L.ssym_resynth_create(ctx, rig.store.ptr, 65536, 513, ctypes.byref(out)) == INVALID and "512 samples" in err()
    assert L.ssym_resynth_create(ctx, rig.store.ptr, 65536, 512, ctypes.byref(out)) == UNSUPPORTED and "65535 lanes" in err()
    assert not out.value
    for bad in (513, -1, True, 1.0):
        with pytest.raises(ValueError):
            rig.e.resynth(rig.store, 1, bad)
    with pytest.raises(ValueError):
        rig.e.resynth(rig.store, 0)
    refcos = Engine(metric="refcos", dtype="f64", device=0)          # either kind of context
    try:
        smp = refcos.samples(rig.sounds[0], np.array([0, 5000], dtype=np.uint64))
        rs = refcos.resynth(smp, 65535, 512)
        assert rs.push([65534], [0], [0], [1], [1]) == 0 and rs.flush(65534, 300) == 300
        off, out_smp = rs.samples()
        assert off[65534] == 0 and off[65535] == 300
        same(out_smp, ref.offline(rig.sounds[:1], [(0, 1, 1)], 300, 512))
        rs.close()
        smp.close()
    finally:
        refcos.close()


def test_push_refusals_come_in_their_order_and_consume_nothing(rig):
    live = Live(rig.e, rig.store, rig.sounds, 3, 8)
    rs = live.rs
    push = lambda rows, at=None, lanes=None: rs.push(*columns(rows, at or {l: live.refs[l].n for l in rows}))
    try:
        live.push({0: tile(0, [4, 5]), 2: [G]})
        before = [a.copy() for a in rs.counts()]
        # one entry, several faults: the earlier check is the one reported
        _refused(lambda: rs.push([3], [9], [7], [0], [0]), match="outside the resynthesiser's lanes")
        _refused(lambda: rs.push([1, 0], [0, 2], [0, 0], [0, 0], [1, 1]), match="ordered by (lane, column)")
        _refused(lambda: rs.push([0], [3], [7], [0], [0]), match="does not continue")
        _refused(lambda: rs.push([1], [0], [7], [0], [0]), match="starts no tile")
        _refused(lambda: rs.push([0], [2], [2], [9], [0]), match="neither a sound of the store")
        _refused(lambda: rs.push([0], [2], [2], [9], [1]), match="neither a sound of the store")
        for frame, src in ((8, 0), (4, 0), (6, 1), (6, nat.COVER_GAP)):          # a step of 3, a step back, another sound, a gap
            _refused(lambda: push({0: [(src, frame, 0)]}), match="within a tile")
        _refused(lambda: push({0: [(0, 5, 0), (0, 5, 0)]}), match="never by 0 twice")        # 5, 5, 5 (entry 1 is the fault)
        _refused(lambda: push({2: [(nat.COVER_GAP, nat.NO_MATCH, 0)]}), match="a gap frame starts a tile")
        # an earlier entry's fault before a later entry's, whatever their kinds
        _refused(lambda: push({0: [(0, 9, 0)], 1: [(0, 0, 0)]}), match="within a tile")
        _refused(lambda: push({0: [(0, 6, 0)], 1: [(0, 0, 0)]}), match="starts no tile")
        L, n = nat.lib(), ctypes.c_uint64(5)
        one = np.zeros(1, dtype=np.uint32)
        p = one.ctypes.data
        assert L.ssym_resynth_push(rig.e.ctx, rs.ptr, p, p, p, p, None, 1, ctypes.byref(n)) == INVALID and n.value == 5
        assert L.ssym_resynth_push(rig.e.ctx, rs.ptr, p, p, p, p, p, 1, None) == INVALID
        assert L.ssym_resynth_push(rig.e.ctx, None, p, p, p, p, p, 1, ctypes.byref(n)) == INVALID
        assert L.ssym_resynth_push(rig.e.ctx, rs.ptr, None, None, None, None, None, 0, ctypes.byref(n)) == nat.SSYM_OK and n.value == 0
        assert [a.tolist() for a in rs.counts()] == [a.tolist() for a in before]
        live.push({0: [(0, 5, 0), (0, 7, 0)], 1: tile(1, [2])})          # nothing was consumed: the restatement's samples
        live.flush(0, 4 * HOP + 10)
        _refused(lambda: push({0: tile(0, [1])}), match="has ended")
        _refused(lambda: rs.push([0], [9], [0], [1], [1]), match="does not continue")       # the column before the ended lane
        live.reset(0)
        live.push({0: tile(0, [1])})
    finally:
        live.close()


def test_flush_reset_and_samples_refusals(rig):
    live = Live(rig.e, rig.store, rig.sounds, 2, 0)
    rs, L, ctx = live.rs, nat.lib(), rig.e.ctx
    other = Engine(metric="dtw", dtype="f64", device=0)
    n = ctypes.c_uint64(5)
    try:
        live.push({1: tile(0, [0, 1, 2])})
        with pytest.raises(ValueError):
            rs.flush(2, 0)
        with pytest.raises(ValueError):
            rs.flush(0, -1)
        with pytest.raises(ValueError):
            rs.reset(2)
        assert L.ssym_resynth_flush(ctx, rs.ptr, 2, 0, ctypes.byref(n)) == INVALID and n.value == 5
        assert L.ssym_resynth_flush(ctx, rs.ptr, 1, 9999, None) == INVALID
        assert L.ssym_resynth_flush(ctx, None, 1, 9999, ctypes.byref(n)) == INVALID
        assert L.ssym_resynth_flush(other.ctx, rs.ptr, 1, 9999, ctypes.byref(n)) == INVALID
        assert b"another context" in L.ssym_last_error(other.ctx)
        assert L.ssym_resynth_reset(ctx, rs.ptr, 2) == INVALID
        _refused(lambda: rs.flush(1, 3 * HOP - 1), match="less than the lane's frames")
        assert rs.counts()[1].tolist() == [0, HOP]              # (hop 0 left with frame 2; nothing since)
        off = np.zeros(3, dtype=np.uint64)
        assert L.ssym_resynth_samples(ctx, rs.ptr, off.ctypes.data, None, None, 2) == INVALID
        assert L.ssym_resynth_samples(ctx, None, off.ctypes.data, None, None, 0) == INVALID
        assert L.ssym_resynth_samples(ctx, rs.ptr, off.ctypes.data, None, None, 0) == nat.SSYM_OK and off.tolist() == [0, 0, HOP]
        live.flush(1, 3 * HOP)
        _refused(lambda: rs.flush(1, 3 * HOP), match="has ended")
        live.flush(0, 0)                                        # a lane without frames or samples
        assert rs.n_samples == 0
        assert L.ssym_resynth_counts(None, None, None) == INVALID
        assert L.ssym_resynth_destroy(ctx, None) == nat.SSYM_OK and L.ssym_resynth_destroy(other.ctx, rs.ptr) == INVALID
    finally:
        other.close()
        live.close()
