"""include/soundsym.hpp's Mosaicker, run by tests/cpp/test_mirror_mosaicker.cpp ONCE on sounds of tests/mirror_cases.py, against
the Python Mosaicker (Engine.mosaicker) on the same sounds, call for call and bit for bit, and once against the restatement
(tests/live_mosaic_ref.py), so that a reading of the outputs both mirrors share does not pass.  Refusals are compared by
code: what Python raises for the same mistake (ValueError: SSYM_E_INVALID; SsymError: its code) is the model."""
import os
import subprocess

import numpy as np
import pytest

import live_mosaic_ref
import mirror_cases as mc
from soundsym_amd import Engine, SsymError
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "cpp", "test_mirror_mosaicker")
PENALTIES = (0.0, 2.5, 40.0)
GAP = 30.0
LANES, BLOCK = 2, 48               # the recordings of 300 and 70 frames, in pushes of 48 frames
NAMES = ("lane", "column", "src", "frame", "cost", "start")


@pytest.fixture(scope="module")
def cases():
    c = mc.build()
    c.args = {"penalties": np.array(PENALTIES), "mosaicker.gap": np.array([GAP]),
              "mosaicker.block": np.array([BLOCK], dtype=np.uint64), "mosaicker.lanes": np.array([LANES], dtype=np.uint64)}
    return c


@pytest.fixture(scope="module")
def res(cases, tmp_path_factory):
    """The one run of the program and its parsed result file."""
    folder = str(tmp_path_factory.mktemp("mirror_mosaicker"))
    case_file, result_file = os.path.join(folder, "cases.bin"), os.path.join(folder, "results.bin")
    mc.write_arrays(case_file, cases.arrays())
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "-f", "mosaicker.mk"])
    r = subprocess.run([EXE, case_file, result_file], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and os.path.exists(result_file), "exit %r\n%s" % (r.returncode, r.stdout + r.stderr)
    return mc.read_arrays(result_file)


def _chunks(cases, p):
    return [f[p * BLOCK:(p + 1) * BLOCK] for _, f in cases.recs[:LANES]]


def _push(mk, chunks):
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in chunks])])
    mk.push(np.concatenate(chunks), off)
    return mk.frames()


def _same(res, p, want):
    assert res[p + ".code"][0] == 0.0, (p, res[p + ".code"][0])
    for name, w in zip(NAMES, want):
        got = res["%s.%s" % (p, name)]
        assert got.dtype == w.dtype and got.tobytes() == w.tobytes(), (p, name)


def _same_best(res, p, mk):
    assert res[p + ".code"][0] == 0.0
    for name, w in zip(("total", "covered", "committed"), mk.best()):
        assert res["%s.%s" % (p, name)].tobytes() == w.tobytes(), (p, name)


def test_mosaicker_call_for_call(res, cases):
    e = Engine(metric="dtw", dtype="f64")
    segs = [f for _, f in cases.segs]
    d = e.dictionary(*pack_segments(segs, 12, np.float64), 12)
    mk = e.mosaicker(d, LANES, PENALTIES[1], GAP)
    refs = [live_mosaic_ref.Lane(segs, 12, PENALTIES[1], GAP) for _ in range(LANES)]
    pushes = int(res["a.pushes"][0])
    assert pushes == -(-300 // BLOCK)
    committed = 0
    for p in range(pushes):
        got = _push(mk, _chunks(cases, p))
        _same(res, "a.push%d" % p, got)
        _same_best(res, "a.push%d.best" % p, mk)
        # ... and once against the restatement
        want = [(l,) + f for l, (r, c) in enumerate(zip(refs, _chunks(cases, p))) for f in r.push(c)]
        assert list(zip(*(got[k].tolist() for k in (0, 1, 2, 3, 5)))) == [(w[0], w[1], w[2], w[3], int(w[5])) for w in want]
        assert got[4].tobytes() == np.array([w[4] for w in want], dtype=np.float64).tobytes()
        committed += len(want)
    assert committed > 0
    assert res["a.counts"].tolist() == mk.counts()[0].tolist() == [300, 70] and res["a.capacity"][0] == mk.counts()[1]
    for l in reversed(range(LANES)):
        mk.flush(l)
        _same(res, "a.flush%d" % l, mk.frames())
    _same_best(res, "a.best", mk)
    assert res["a.best.committed"].tolist() == [300, 70]
    again = [cases.recs[1][1], cases.recs[1][1][:0]]
    with pytest.raises(SsymError) as err:
        _push(mk, again)
    assert res["b.ended.code"][0] == float(err.value.code) == float(nat.SSYM_E_INVALID)
    mk.reset(0)
    assert res["b.reset.code"][0] == 0.0
    _same(res, "b.again", _push(mk, again))
    mk.flush(0)
    _same(res, "b.flush", mk.frames())
    assert res["b.counts"].tolist() == mk.counts()[0].tolist() == [70, 70]
    assert res["b.flush.lane"].size + res["b.again.lane"].size == 70
    plain = e.mosaicker(d, 1, PENALTIES[1])
    plain.push(cases.recs[1][1])
    _same(res, "c.plain", plain.frames())
    plain.flush(0)
    want = plain.frames()
    for name, w in zip(NAMES, want):
        assert res["c.flush." + name].tobytes() == w.tobytes(), name
    for h in (plain, mk, d):
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
        d, empty = e.dictionary(*pack(cases.segs), 12), e.dictionary(*pack([]), 12)
        rd = r.dictionary(*pack(cases.segs), 12)
        mk = e.mosaicker(d, LANES)
        x = cases.recs[1][1]
        for name, call in (("l.lane", lambda: mk.flush(LANES)), ("l.reset", lambda: mk.reset(LANES)),
                           ("l.offsets", lambda: mk.push(x, [0])), ("l.negative", lambda: e.mosaicker(d, 1, -1.0)),
                           ("l.nan", lambda: e.mosaicker(d, 1, float("nan"))), ("l.gap", lambda: e.mosaicker(d, 1, 1.0, -2.0)),
                           ("l.lanes", lambda: e.mosaicker(d, 0)), ("l.empty", lambda: e.mosaicker(empty)),
                           ("l.refcos", lambda: r.mosaicker(rd))):
            want = _code(call)
            assert want != 0.0 and res[name + ".code"][0] == want, (name, res[name + ".code"][0], want)
        assert res["l.refcos.code"][0] == float(nat.SSYM_E_UNSUPPORTED)
        assert res["l.empty.code"][0] == float(nat.SSYM_E_EMPTY_DICT) and res["l.negative.code"][0] == float(nat.SSYM_E_INVALID)
        mk.close()
    finally:
        e.close()
        r.close()
