"""include/soundsym.hpp's class Follower, run by tests/cpp/test_mirror_follower.cpp ONCE on signals this file writes, against
the Python layer (Engine.follower) on the same calls, bit for bit -- every push's and flush's offsets, samples, pcm and gains,
and the counts -- and once against the restatement (tests/live_follow_ref.py), so that a reading of the outputs both mirrors
share does not pass.  Refusals are compared by code: what Python raises for the same mistake (ValueError: SSYM_E_INVALID; a
library refusal: its code) is the model."""
import os
import subprocess

import numpy as np
import pytest

import follow_ref as fr
import live_follow_ref as lf
import mirror_cases as mc
from soundsym_amd import Engine
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "cpp", "test_mirror_follower")
LENGTHS, REF_LENGTHS = (4097, 300, 7937), (4000, 900, 8100)
Y_CUTS, X_CUTS = (0, 300, 2900, 8200), (0, 700, 2500, 8200)
RESET_LANE, RESET_AFTER = 1, 0
MAX_GAIN = 4.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want, what):
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), what


@pytest.fixture(scope="module")
def signals():
    y, off, x, r_off = fr.ragged_case(LENGTHS, seed=0xF0140, ref_lengths=REF_LENGTHS)
    y[100:1500] *= 1e-3                             # a stretch far too quiet: the gains meet max_gain
    return y, off, x, r_off


@pytest.fixture(scope="module")
def res(signals, tmp_path_factory):
    """The one run of the program and its parsed result file."""
    y, off, x, r_off = signals
    folder = str(tmp_path_factory.mktemp("mirror_follower"))
    case_file, result_file = os.path.join(folder, "cases.bin"), os.path.join(folder, "results.bin")
    mc.write_arrays(case_file, {"follower.samples": y, "follower.off": off, "follower.ref": x, "follower.r_off": r_off,
                                "follower.y_cuts": np.array(Y_CUTS, dtype=np.uint64), "follower.x_cuts": np.array(X_CUTS, dtype=np.uint64),
                                "follower.reset": np.array([RESET_LANE, RESET_AFTER], dtype=np.uint32),
                                "follower.max_gain": np.array([MAX_GAIN])})
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "-f", "follower.mk"])
    r = subprocess.run([EXE, case_file, result_file], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and os.path.exists(result_file), "exit %r\n%s" % (r.returncode, r.stdout + r.stderr)
    return mc.read_arrays(result_file)


def _lanes(signals):
    y, off, x, r_off = signals
    return [(y[int(a):int(b)], x[int(c):int(d)]) for a, b, c, d in zip(off[:-1], off[1:], r_off[:-1], r_off[1:])]


def _pushes(signals):
    return [[(ly[Y_CUTS[p]:Y_CUTS[p + 1]], lx[X_CUTS[p]:X_CUTS[p + 1]]) for ly, lx in _lanes(signals)] for p in range(len(Y_CUTS) - 1)]


def _offsets(parts):
    return np.concatenate([[0], np.cumsum([a.size for a in parts])]).astype(np.uint64)


def _block(res, name, off, out, pcm, g_off, gains):
    assert res[name + ".code"][0] == 0.0, name
    assert res[name + ".off"].tolist() == [float(v) for v in off] and res[name + ".g_off"].tolist() == [float(v) for v in g_off], name
    _same(res[name + ".out"], out, name + " samples")
    assert np.array_equal(res[name + ".pcm"], np.asarray(pcm, dtype=np.float64)), name + " pcm"
    _same(res[name + ".gains"], gains, name + " gains")


@pytest.mark.parametrize("tag,metric", [("a", "dtw"), ("r", "refcos")])
def test_every_call_bit_for_bit(res, signals, tag, metric):
    e = Engine(metric=metric, dtype="f64")
    try:
        f = e.follower(len(LENGTHS), MAX_GAIN)
        ref = lf.LiveFollower(len(LENGTHS), MAX_GAIN)
        assert res[tag + ".create.code"][0] == 0.0
        released = 0
        for p, new in enumerate(_pushes(signals)):
            ys, xs = [a for a, _ in new], [b for _, b in new]
            released += f.push(np.concatenate(ys), _offsets(ys), np.concatenate(xs), _offsets(xs))
            got = f.samples(want_pcm32=True, want_gains=True)
            _block(res, "%s.push%d" % (tag, p), *got)
            want = ref.push(ys, xs)                                   # ... and the restatement
            _same(res["%s.push%d.out" % (tag, p)], np.concatenate([o for o, _ in want]), "live_follow_ref samples")
            _same(res["%s.push%d.gains" % (tag, p)], np.concatenate([g for _, g in want]), "live_follow_ref gains")
            if p == RESET_AFTER:
                f.reset(RESET_LANE)
                ref.reset(RESET_LANE)
                assert res[tag + ".reset.code"][0] == 0.0
        assert released > 20 * fr.HOP
        assert res[tag + ".counts.code"][0] == 0.0
        for key, want in zip(("ny", "nx", "released"), f.counts()):
            assert res["%s.counts.%s" % (tag, key)].tolist() == want.astype(np.float64).tolist() and key
        assert [int(v) for v in res[tag + ".counts.ny"]] == ref.counts()[0]
        for l in range(len(LENGTHS)):
            f.flush(l)
            _block(res, "%s.flush%d" % (tag, l), *f.samples(want_pcm32=True, want_gains=True))
            o, g = ref.flush(l)
            _same(res["%s.flush%d.out" % (tag, l)], o, "live_follow_ref flush")
            _same(res["%s.flush%d.gains" % (tag, l)], g, "live_follow_ref flush gains")
        f.close()
    finally:
        e.close()


def test_one_lane_with_the_bare_signals(res, signals):
    y, x = _lanes(signals)[0]
    assert res["b.code"][0] == 0.0
    out, g = fr.follow_one(y, x, 8.0)                                  # the default max_gain is 8
    h = min(y.size, x.size) // fr.HOP
    assert res["b.push.off"].tolist() == [0.0, (h - 2) * fr.HOP] and res["b.push.g_off"].tolist() == [0.0, h - 1.0]
    _same(np.concatenate([res["b.push.out"], res["b.flush.out"]]), out, "whole")
    _same(np.concatenate([res["b.push.gains"], res["b.flush.gains"]]), g, "whole gains")
    assert np.array_equal(np.concatenate([res["b.push.pcm"], res["b.flush.pcm"]]), fr.pcm32(out).astype(np.float64))


def test_refusals_by_code_against_python(res):
    e = Engine(metric="dtw", dtype="f64")
    try:
        f = e.follower(2)
        one = np.array([1.0])
        two = np.array([1.0, 2.0])
        python = {
            "l.gain.low": lambda: e.follower(1, 0.5),
            "l.gain.nan": lambda: e.follower(1, float("nan")),
            "l.lanes.none": lambda: e.follower(0),
            "l.offsets.count": lambda: f.push(one, [0, 1], None, [0, 0, 0]),
            "l.offsets.start": lambda: f.push(two, [1, 1, 2], None, [0, 0, 0]),
            "l.offsets.decrease": lambda: f.push(two, [0, 2, 1], None, [0, 0, 0]),
            "l.samples.short": lambda: f.push(one, [0, 1, 2], None, [0, 0, 0]),
            "l.lane.outside": lambda: f.flush(2),
            "l.reset.outside": lambda: f.reset(2),
        }
        for name, call in python.items():
            with pytest.raises(ValueError):
                call()
            assert res[name + ".code"][0] == float(nat.SSYM_E_INVALID), (name, res[name + ".code"][0])
        with pytest.raises(ValueError):
            e.follower(16385)                                          # Python stops it; the mirror leaves it to the library
        assert res["l.lanes.many.code"][0] == float(nat.SSYM_E_UNSUPPORTED)
        assert res["l.flush.ok.code"][0] == 0.0 and f.flush(1) == 0
        for name, call in (("l.lane.ended", lambda: f.flush(1)), ("l.push.ended", lambda: f.push(one, [0, 0, 1], None, [0, 0, 0]))):
            with pytest.raises(nat.SsymError) as err:
                call()
            assert res[name + ".code"][0] == float(err.value.code) == float(nat.SSYM_E_INVALID), name
        assert sorted(k[:-5] for k in res if k.startswith("l.")) == sorted(list(python) + ["l.lanes.many", "l.flush.ok", "l.lane.ended", "l.push.ended"])
        f.close()
    finally:
        e.close()
