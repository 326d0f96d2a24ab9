"""include/soundsym.hpp's Coverer, run by tests/cpp/test_mirror_coverer.cpp ONCE on sounds of tests/mirror_cases.py, against
the Python Coverer (Engine.coverer) on the same sounds, call for call and bit for bit, and once against the restatement
(tests/live_cover_ref.py), so that a reading of the outputs both mirrors share does not pass.  Refusals are compared by
code: what Python raises for the same mistake (ValueError: SSYM_E_INVALID; SsymError: its code) is the model."""
import os
import subprocess

import numpy as np
import pytest

import live_cover_ref
import mirror_cases as mc
from soundsym_amd import Engine, SsymError
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "cpp", "test_mirror_coverer")
PENALTIES = (0.0, 2.5, 40.0)
SEGMENTS = 4                       # segments of 4, 17, 33 and 66 frames; the fifth has 130, more than a coverer takes
LANES, BLOCK = 2, 48               # the recordings of 300 and 70 frames, in pushes of 48 frames
NAMES = ("lane", "src", "start", "end", "cost")


@pytest.fixture(scope="module")
def cases():
    c = mc.build()
    c.args = {"penalties": np.array(PENALTIES), "cover.segments": np.array([SEGMENTS], dtype=np.uint64),
              "coverer.block": np.array([BLOCK], dtype=np.uint64), "coverer.lanes": np.array([LANES], dtype=np.uint64)}
    return c


@pytest.fixture(scope="module")
def res(cases, tmp_path_factory):
    """The one run of the program and its parsed result file."""
    folder = str(tmp_path_factory.mktemp("mirror_coverer"))
    case_file, result_file = os.path.join(folder, "cases.bin"), os.path.join(folder, "results.bin")
    mc.write_arrays(case_file, cases.arrays())
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "-f", "coverer.mk"])
    r = subprocess.run([EXE, case_file, result_file], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and os.path.exists(result_file), "exit %r\n%s" % (r.returncode, r.stdout + r.stderr)
    return mc.read_arrays(result_file)


def _chunks(cases, p):
    return [f[p * BLOCK:(p + 1) * BLOCK] for _, f in cases.recs[:LANES]]


def _push(cv, chunks):
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in chunks])])
    cv.push(np.concatenate(chunks), off)
    return cv.pieces()


def _same(res, p, want):
    assert res[p + ".code"][0] == 0.0, (p, res[p + ".code"][0])
    for name, w in zip(NAMES, want):
        got = res["%s.%s" % (p, name)]
        assert got.dtype == w.dtype and got.tobytes() == w.tobytes(), (p, name)


def _same_best(res, p, cv):
    assert res[p + ".code"][0] == 0.0
    for name, w in zip(("total", "covered", "committed"), cv.best()):
        assert res["%s.%s" % (p, name)].tobytes() == w.tobytes(), (p, name)


def test_coverer_call_for_call(res, cases):
    e = Engine(metric="dtw", dtype="f64")
    d = e.dictionary(*pack_segments([f for _, f in cases.segs[:SEGMENTS]], 12, np.float64), 12)
    cv = e.coverer(d, LANES, PENALTIES[1])
    refs = [live_cover_ref.Lane([f for _, f in cases.segs[:SEGMENTS]], PENALTIES[1]) for _ in range(LANES)]
    pushes = int(res["a.pushes"][0])
    assert pushes == -(-300 // BLOCK)
    committed = 0
    for p in range(pushes):
        got = _push(cv, _chunks(cases, p))
        _same(res, "a.push%d" % p, got)
        _same_best(res, "a.push%d.best" % p, cv)
        # ... and once against the restatement
        want = [(l,) + piece for l, (r, c) in enumerate(zip(refs, _chunks(cases, p))) for piece in r.push(c)]
        assert list(zip(*(a.tolist() for a in got[:4]))) == [w[:4] for w in want]
        assert got[4].tobytes() == np.array([w[4] for w in want], dtype=np.float64).tobytes()
        committed += len(want)
    assert committed >= 0 and sum(len(r.emitted) for r in refs) == committed
    assert res["a.counts"].tolist() == cv.counts()[0].tolist() == [300, 70] and res["a.capacity"][0] == cv.counts()[1] == 1024
    for l in reversed(range(LANES)):
        cv.flush(l)
        _same(res, "a.flush%d" % l, cv.pieces())
    _same_best(res, "a.best", cv)
    assert res["a.best.committed"].tolist() == [300, 70]
    again = [cases.recs[1][1], cases.recs[1][1][:0]]
    with pytest.raises(SsymError) as err:
        _push(cv, again)
    assert res["b.ended.code"][0] == float(err.value.code) == float(nat.SSYM_E_INVALID)
    cv.reset(0)
    assert res["b.reset.code"][0] == 0.0
    _same(res, "b.again", _push(cv, again))
    cv.flush(0)
    _same(res, "b.flush", cv.pieces())
    assert res["b.counts"].tolist() == cv.counts()[0].tolist() == [70, 70]
    assert res["b.flush.lane"].size + res["b.again.lane"].size == res["a.flush1.lane"].size + sum(
        int((res["a.push%d.lane" % p] == 1).sum()) for p in range(pushes))       # lane 0 now holds what lane 1 held
    for h in (cv, d):
        h.close()
    e.close()


def _code(call):
    try:
        call()
    except ValueError:
        return float(nat.SSYM_E_INVALID)
    except SsymError as err:
        return float(err.code)
    return 0.0


def test_refusals_by_code(res, cases):
    e, r = Engine(metric="dtw", dtype="f64"), Engine(metric="refcos", dtype="f64")
    try:
        pack = lambda segs: pack_segments([f for _, f in segs], 12, np.float64)
        d, long_d, empty = e.dictionary(*pack(cases.segs[:SEGMENTS]), 12), e.dictionary(*pack(cases.segs), 12), e.dictionary(*pack([]), 12)
        rd = r.dictionary(*pack(cases.segs[:SEGMENTS]), 12)
        cv = e.coverer(d, LANES)
        x = cases.recs[1][1]
        for name, call in (("l.lane", lambda: cv.flush(LANES)), ("l.reset", lambda: cv.reset(LANES)),
                           ("l.offsets", lambda: cv.push(x, [0])), ("l.negative", lambda: e.coverer(d, 1, -1.0)),
                           ("l.nan", lambda: e.coverer(d, 1, float("nan"))), ("l.lanes", lambda: e.coverer(d, 0)),
                           ("l.long", lambda: e.coverer(long_d)), ("l.empty", lambda: e.coverer(empty)),
                           ("l.refcos", lambda: r.coverer(rd))):
            want = _code(call)
            assert want != 0.0 and res[name + ".code"][0] == want, (name, res[name + ".code"][0], want)
        assert res["l.long.code"][0] == float(nat.SSYM_E_UNSUPPORTED) == res["l.refcos.code"][0]
        assert res["l.empty.code"][0] == float(nat.SSYM_E_EMPTY_DICT) and res["l.negative.code"][0] == float(nat.SSYM_E_INVALID)
        cv.close()
    finally:
        e.close()
        r.close()
