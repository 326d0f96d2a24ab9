"""Every refusal of ssym_follower_* in its order: the code, the message, nothing consumed (counts unchanged, the next good call
has the bits of a run without the refusal) and the outputs all sentinel; where two faults meet, the earlier is reported.

push: the handle | unknown flag bits | NULL offsets or count | the offsets' start | lane by lane: a decrease, the lane has
ended, the 2^40 limit | the ring cap | NULL arrays.  create: ctx | out | max_gain | lanes.  flush: the handle | a lane outside
the lanes or a NULL count | a lane that has ended.  samples: the handle | unknown flag bits."""
import ctypes

import numpy as np
import pytest

import follow_ref as fr
import follower_gpu as wg
import live_follow_ref as lf
from follow_ref import HOP
from soundsym_amd import Engine
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = nat.SSYM_E_INVALID, nat.SSYM_E_UNSUPPORTED
BIG = 1 << 40


@pytest.fixture(scope="module")
def engines():
    e, other = Engine(metric="dtw", dtype="f64"), Engine(metric="refcos", dtype="f64")
    yield e, other
    e.close()
    other.close()


@pytest.fixture(scope="module")
def pair():
    y, _, x, _ = fr.ragged_case([9 * HOP + 40], 0xF0130)
    return y, x


def _started(e, pair, n_lanes=3):
    """a follower in mid-flight: every lane fed 1000 samples of both, lane 2 flushed"""
    y, x = pair
    live = wg.Live(e, n_lanes)
    live.push([y[:1000]] * n_lanes, [x[:1000]] * n_lanes, "start")
    live.flush(n_lanes - 1, "start flush")
    return live


def _refused(live, call, code, *words):
    before = live.fl.counts()
    res = call()
    assert res.rc == code, (res.rc, res.message)
    for w in words:
        assert w in res.message, (w, res.message)
    assert res.untouched and live.fl.counts() == before == live.ref.counts()
    return res


def test_create_refuses_in_order_before_any_device_work(engines):
    e, _ = engines
    lib = nat.lib()
    out = ctypes.c_void_p(0x1234)
    assert lib.ssym_follower_create(None, 0, 0.5, ctypes.byref(out)) == INVALID and out.value == 0x1234        # ctx first, nothing written
    assert lib.ssym_follower_create(e.ctx, 0, 0.5, None) == INVALID and "out is NULL" in wg._message(e)
    for gain in (0.5, float("nan"), float("inf"), -8.0):
        f = wg.Follower(e, 0, gain)                                           # max_gain before the lanes
        assert f.rc == INVALID and f.ptr is None and "max_gain" in f.message
        f = wg.Follower(e, lf.MAX_LANES + 1, gain)
        assert f.rc == INVALID and "max_gain" in f.message
    f = wg.Follower(e, 0)
    assert f.rc == INVALID and f.ptr is None and "n_lanes" in f.message
    f = wg.Follower(e, lf.MAX_LANES + 1)
    assert f.rc == UNSUPPORTED and f.ptr is None and "16384" in f.message
    f = wg.Follower(e, 1, 1.0)                                                # the least max_gain there is
    assert f.rc == nat.SSYM_OK
    f.close()


def test_push_refuses_in_its_order_and_consumes_nothing(engines, pair):
    e, other = engines
    y, x = pair
    live = _started(e, pair)
    a = [y[1000:1300]] * 2 + [None]
    b = [x[1000:1300]] * 2 + [None]
    # the handle before everything: NULL, or another context's, with every later fault beside it
    r = _refused(live, lambda: live.fl.push(a, b, ptr=None, flags=1 << 20, null=("off", "count")), INVALID, "ssym_follower_push", "follower handle is NULL")
    r = _refused(live, lambda: live.fl.push(a, b, ctx=other.ctx, flags=1 << 20), INVALID)
    assert "belongs to another context" in (nat.lib().ssym_last_error(other.ctx) or b"").decode()
    # flags before the NULL offsets; SSYM_OUT_DEVICE is no flag of a push
    _refused(live, lambda: live.fl.push(a, b, flags=1 << 20, null=("off",)), INVALID, "unknown flag bits")
    _refused(live, lambda: live.fl.push(a, b, flags=nat.OUT_DEVICE), INVALID, "unknown flag bits")
    # NULL offsets or count before the offsets' start
    for null in (("off",), ("r_off",), ("count",)):
        _refused(live, lambda: live.fl.push(a, b, null=null, off=[1, 300, 600, 600] if "off" not in null else None), INVALID, "must not be NULL")
    # the start before the lanes
    _refused(live, lambda: live.fl.push(a, b, off=[1, 0, 600, 600]), INVALID, "start at 0")
    _refused(live, lambda: live.fl.push(a, b, r_off=[7, 300, 600, 600], off=[0, 300, 200, 600]), INVALID, "start at 0")
    # lane by lane, the earliest lane's fault first: lane 0's limit before lane 1's decrease before lane 2's end
    _refused(live, lambda: live.fl.push(a, b, off=[0, BIG, 200, 900], null=("samples",)), UNSUPPORTED, "lane 0", "2^40")
    _refused(live, lambda: live.fl.push(a, b, off=[0, 300, 200, 900]), INVALID, "decrease", "lane 1")
    _refused(live, lambda: live.fl.push(a, b, r_off=[0, 300, 200, 900]), INVALID, "decrease", "lane 1")
    # ... and within a lane: the decrease, the end, the limit
    _refused(live, lambda: live.fl.push(a, b, off=[0, 300, 600, 500]), INVALID, "decrease", "lane 2")
    _refused(live, lambda: live.fl.push(a, b, off=[0, 300, 600, 600 + BIG]), INVALID, "lane 2", "has ended", "ssym_follower_reset")
    _refused(live, lambda: live.fl.push(a, b, r_off=[0, 300, 600, 601]), INVALID, "lane 2", "has ended")
    _refused(live, lambda: live.fl.push(a, b, off=[0, 300, 300 + BIG - 1000, 300 + BIG - 1000], null=("samples",)), UNSUPPORTED, "lane 1", "2^40")
    _refused(live, lambda: live.fl.push(a, b, r_off=[0, BIG - 1000, BIG - 1000, BIG - 1000], null=("ref",)), UNSUPPORTED, "lane 0", "2^40")
    ok = live.fl.push([None] * 3, [None] * 3, off=[0, 0, 0, 0], r_off=[0, 0, 0, 0])          # (a push of nothing is no fault)
    assert ok.rc == nat.SSYM_OK and ok.n == 0
    # the ring cap before the NULL arrays: three lanes share 2^25 samples per signal, 2^23 each (a power of two)
    room = (1 << 23) - 1000
    _refused(live, lambda: live.fl.push(a, b, off=[0, room + 1, room + 1, room + 1], null=("samples",)), UNSUPPORTED, "rings", "512 MiB")
    _refused(live, lambda: live.fl.push(a, b, r_off=[0, 0, room + 1, room + 1], null=("ref",)), UNSUPPORTED, "rings")
    # NULL arrays last
    _refused(live, lambda: live.fl.push(a, b, null=("samples",)), INVALID, "samples and ref must not be NULL")
    _refused(live, lambda: live.fl.push(a, b, null=("ref",)), INVALID, "samples and ref must not be NULL")
    _refused(live, lambda: live.fl.push(a, [None] * 3, null=("samples", "ref")), INVALID, "must not be NULL")
    ok = live.fl.push([None] * 3, b, null=("samples",))                      # ... but an array that holds nothing may be NULL
    assert ok.rc == nat.SSYM_OK
    live.ref.push([None] * 3, b)
    # the next good call has the bits of a run without the refusals, and so has the whole
    live.push(a, [None] * 3, "after the refusals")
    live.push([y[1300:], y[1300:2000], None], [x[1300:], x[1300:], None], "the rest")
    live.flush(0, "flush")
    live.flush(1, "flush")
    for l, (ly, lx) in enumerate([(y, x), (y[:2000], x)]):
        out, gain = live.total(l)
        want_out, want_g = fr.follow_one(ly, lx)
        assert wg.same_bits(out, want_out) and wg.same_bits(gain, want_g)
    live.close()


def test_flush_reset_and_samples_refuse(engines, pair):
    e, other = engines
    live = _started(e, pair)
    _refused(live, lambda: live.fl.flush(0, ptr=None, null=("count",)), INVALID, "ssym_follower_flush", "follower handle is NULL")
    _refused(live, lambda: live.fl.flush(3), INVALID, "lane outside the follower's lanes")
    _refused(live, lambda: live.fl.flush(0xFFFFFFFF), INVALID, "lane outside")
    _refused(live, lambda: live.fl.flush(0, null=("count",)), INVALID, "out_n_samples is NULL")
    _refused(live, lambda: live.fl.flush(2), INVALID, "lane 2", "has ended", "ssym_follower_reset")
    assert live.fl.reset(3).rc == INVALID and "lane outside the follower's lanes" in wg._message(e)
    assert nat.lib().ssym_follower_reset(e.ctx, None, 0) == INVALID and "handle is NULL" in wg._message(e)
    assert live.fl.counts() == live.ref.counts()
    # samples: the logs of the last call (the flush of lane 2) stay readable after every refusal above
    want = [(np.zeros(0), np.zeros(0))] * 2 + [(live.outs[2][-1], live.gains[2][-1])]
    wg.assert_logs(live.fl.read(), want, "after the refusals")
    for out_dev in (False, True):
        logs = live.fl.read(out_dev=out_dev, flags=2, room=(1000, 10))
        assert logs.rc == INVALID and "unknown flag bits" in logs.message and logs.untouched
        logs = live.fl.read(out_dev=out_dev, ptr=None, room=(1000, 10))
        assert logs.rc == INVALID and "handle is NULL" in logs.message and logs.untouched
    assert nat.lib().ssym_follower_destroy(other.ctx, live.fl.ptr) == INVALID              # another context's: not destroyed
    wg.assert_logs(live.fl.read(out_dev=True), want, "still there")
    live.close()
