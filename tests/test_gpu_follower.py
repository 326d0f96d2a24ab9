"""ssym_follower_* through ctypes against tests/live_follow_ref.py, bit for bit: one lane of 20 hops + 100 samples under every
way of cutting it -- all at once, 1 / 255 / 256 / 257 / 513 samples at a time, x far ahead, x far behind, alternating -- every
call's samples, pcm and gains into sentinel-filled outputs, the concatenation against ssym_follow_envelope run on the GPU in
the same test; host and device inputs and outputs in every combination of the three flags; Engine.follower over the same
calls."""
import numpy as np
import pytest

import follow_gpu as fg
import follow_ref as fr
import follower_gpu as wg
from follow_ref import HOP
from soundsym_amd import Engine
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu

N = 20 * HOP + 100


@pytest.fixture(scope="module")
def eng():
    e = Engine(metric="dtw", dtype="f64")
    yield e
    e.close()


@pytest.fixture(scope="module")
def pair():
    """(y, x) of N samples each, a stretch far too quiet so that its gains meet max_gain; computed once, left unchanged."""
    y, _, x, _ = fr.ragged_case([N], 0xF0111E)
    y[700:1900] *= 1e-3
    return y, x


def _steps(m):
    return [(m, m)] * (N // m + 1)


CUTS = {
    "all_at_once": [],
    "by_1": _steps(1),
    "by_255": _steps(255),
    "by_256": _steps(256),
    "by_257": _steps(257),
    "by_513": _steps(513),
    "x_far_ahead": [(0, N)] + [(300, 0)] * 18,
    "x_far_behind": [(N, 0)] + [(0, 300)] * 18,
    "alternating": [(700, 0), (0, 700)] * 8,
}


def _offline(eng, y, x, max_gain=8.0):
    res = fg.call(eng, y, [0, y.size], x, [0, x.size], max_gain)
    assert res.rc == nat.SSYM_OK, res.message
    return res


@pytest.mark.parametrize("name", list(CUTS))
def test_every_cut_gives_the_restatements_calls_and_the_offline_whole(eng, pair, name):
    y, x = pair
    live = wg.Live(eng, 1)
    if name == "by_1":
        # the first three hops and the last one a sample at a time (every call held), the stretch between in one push
        wg.feed(live, [pair], [(1, 1)] * (3 * HOP + 2) + [(N - 4 * HOP - 2, N - 4 * HOP - 2)] + [(1, 1)] * (HOP - 1), name)
    else:
        wg.feed(live, [pair], CUTS[name], name)
    live.flush(0, name + " flush")
    out, gain = live.total(0)
    off = _offline(eng, y, x)
    assert fg.same_bits(out, off.out) and fg.same_bits(gain, off.gain) and np.array_equal(fr.pcm32(out), off.pcm)
    assert np.any(gain == 8.0) and np.any((gain > 0.0) & (gain < 8.0))
    live.close()


@pytest.mark.parametrize("out_dev", [False, True], ids=["host_out", "device_out"])
@pytest.mark.parametrize("x_dev", [False, True], ids=["host_ref", "device_ref"])
@pytest.mark.parametrize("y_dev", [False, True], ids=["host_samples", "device_samples"])
def test_every_placement_gives_the_same_bits(eng, pair, y_dev, x_dev, out_dev):
    y, x = pair
    live = wg.Live(eng, 2)
    lanes = [pair, (x[:3000] / 3.0, x[:2500])]
    wg.feed(live, lanes, [(513, 257), (0, 600), (1400, 1000)], "placement", y_dev=y_dev, x_dev=x_dev, out_dev=out_dev)
    for lane, (ly, lx) in enumerate(lanes):
        live.flush(lane, "placement flush", out_dev=out_dev)
        out, gain = live.total(lane)
        off = _offline(eng, ly, lx)
        assert fg.same_bits(out, off.out) and fg.same_bits(gain, off.gain)
    live.close()


def test_each_output_alone_and_all_null(eng, pair):
    live = wg.Live(eng, 1)
    wg.feed(live, [pair], [(2000, 2000)], "outputs")
    want = live.ref.push([pair[0][2000:4000]], [pair[1][2000:4000]])
    assert live.fl.push([pair[0][2000:4000]], [pair[1][2000:4000]]).rc == nat.SSYM_OK
    for out_dev in (False, True):
        for keys in (("out",), ("pcm",), ("gain",), ("off",), ("g_off",), ("out", "g_off"), ("pcm", "gain", "off")):
            logs = live.fl.read(out_dev=out_dev, want=keys)
            assert [k for k in ("out", "pcm", "gain") if getattr(logs, k) is not None] == [k for k in keys if k in ("out", "pcm", "gain")]
            wg.assert_logs(logs, want, keys)
        logs = live.fl.read(out_dev=out_dev, want=())
        assert logs.rc == nat.SSYM_OK
    live.close()


def test_engine_follower_over_the_same_calls(eng, pair):
    y, x = pair
    f = eng.follower(1, 8.0)
    ref = wg.lf.LiveFollower(1, 8.0)
    outs, gains = [], []
    import torch
    for i, (a, b) in enumerate([(0, 1000), (1000, 1001), (1001, 4000), (4000, N)]):
        ys, xs = y[a:b], x[a:b]
        (want_out, want_g), = ref.push([ys], [xs])
        on_device = i % 2 == 1
        n = f.push(torch.from_numpy(ys.copy()).cuda() if on_device else ys, None, xs, [0, xs.size])
        assert n == f.n_samples == want_out.size
        off, out, pcm, g_off, g = f.samples(want_pcm32=True, want_gains=True, on_device=on_device)
        if on_device:
            out, pcm, g = out.cpu().numpy(), pcm.cpu().numpy(), g.cpu().numpy()
        assert list(off) == [0, want_out.size] and list(g_off) == [0, want_g.size]
        assert fg.same_bits(out, want_out) and np.array_equal(pcm, fr.pcm32(want_out)) and fg.same_bits(g, want_g)
        assert len(f.samples()) == 2 and len(f.samples(want_gains=True)) == 4
        outs.append(out)
        gains.append(g)
    ny, nx, rel = f.counts()
    assert (int(ny[0]), int(nx[0]), int(rel[0])) == (N, N, 18 * HOP)
    assert f.flush(0) == N - 18 * HOP
    off, out, g_off, g = f.samples(want_gains=True)
    whole = eng.follow_envelope(y, [0, N], x, [0, N], 8.0, want_gains=True)
    assert fg.same_bits(np.concatenate(outs + [out]), whole[0]) and fg.same_bits(np.concatenate(gains + [g]), whole[-1])
    with pytest.raises(nat.SsymError) as err:
        f.push(y[:10], None, x[:10], None)
    assert err.value.code == nat.SSYM_E_INVALID and "has ended" in str(err.value)
    f.reset(0)
    assert f.push(y[:10], None, None, None) == 0
    f.close()
    f.close()
