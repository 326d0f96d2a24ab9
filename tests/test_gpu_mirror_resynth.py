"""include/soundsym.hpp's Resynth, run by tests/cpp/test_mirror_resynth.cpp ONCE on sounds of tests/mirror_cases.py behind a
Mosaicker, against the Python Resynth (Engine.resynth) on the same sounds, call for call and bit for bit, and once against the
restatement (tests/live_resynth_ref.py), so that a reading of the outputs both mirrors share does not pass.  Refusals are
compared by code: what Python raises for the same mistake (ValueError: SSYM_E_INVALID; SsymError: its code) is the model."""
import os
import subprocess

import numpy as np
import pytest

import live_resynth_ref
import mirror_cases as mc
from soundsym_amd import Engine, SsymError
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "cpp", "test_mirror_resynth")
PENALTIES = (0.0, 2.5, 40.0)
GAP = 30.0
SEARCH = 24
LANES, BLOCK = 2, 48               # the recordings of 300 and 70 frames, in pushes of 48 frames
ROWS = ([0, 0, 0], [0, 1, 2], [1, 1, nat.COVER_GAP], [3, 4, nat.NO_MATCH], [1, 0, 1])


@pytest.fixture(scope="module")
def cases():
    c = mc.build()
    c.args = {"penalties": np.array(PENALTIES), "mosaicker.gap": np.array([GAP]),
              "mosaicker.block": np.array([BLOCK], dtype=np.uint64), "mosaicker.lanes": np.array([LANES], dtype=np.uint64),
              "resynth.search": np.array([SEARCH], dtype=np.uint64)}
    return c


@pytest.fixture(scope="module")
def res(cases, tmp_path_factory):
    """The one run of the program and its parsed result file."""
    folder = str(tmp_path_factory.mktemp("mirror_resynth"))
    case_file, result_file = os.path.join(folder, "cases.bin"), os.path.join(folder, "results.bin")
    mc.write_arrays(case_file, cases.arrays())
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "-f", "resynth.mk"])
    r = subprocess.run([EXE, case_file, result_file], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and os.path.exists(result_file), "exit %r\n%s" % (r.returncode, r.stdout + r.stderr)
    return mc.read_arrays(result_file)


def _store(e, cases):
    smp = [s for s, _ in cases.segs]
    return e.samples(np.concatenate(smp), np.concatenate([[0], np.cumsum([s.size for s in smp])]).astype(np.uint64))


def _same(res, p, rs):
    """The program's samples of call p against the Python resynthesiser's last call."""
    assert res[p + ".code"][0] == 0.0, (p, res[p + ".code"][0])
    off, smp, pcm = rs.samples(want_pcm32=True)
    assert res[p + ".offsets"].tolist() == off.tolist(), p
    assert res[p + ".samples"].tobytes() == smp.tobytes(), p
    assert res[p + ".pcm"].tobytes() == pcm.tobytes(), p
    return off, smp


def test_resynth_call_for_call(res, cases):
    e = Engine(metric="dtw", dtype="f64")
    segs = [f for _, f in cases.segs]
    d = e.dictionary(*pack_segments(segs, 12, np.float64), 12)
    store = _store(e, cases)
    mk = e.mosaicker(d, LANES, PENALTIES[1], GAP)
    R, P = e.resynth(store, LANES, SEARCH), e.resynth(store, LANES, 0)
    sounds = [s for s, _ in cases.segs]
    refs = [live_resynth_ref.LiveResynth(sounds, SEARCH) for _ in range(LANES)]
    pushes = int(res["a.pushes"][0])
    assert pushes == -(-300 // BLOCK)

    def both(name, frames):
        R.take(mk)
        off, smp = _same(res, name + ".take", R)
        P.push(*(frames[k] for k in (0, 1, 2, 3, 5)))
        _same(res, name + ".rows", P)
        for l, r in enumerate(refs):                            # ... and once against the restatement
            k = np.flatnonzero(frames[0] == l)
            want = r.push(list(zip(frames[2][k].tolist(), frames[3][k].tolist(), frames[5][k].tolist()))) if k.size else np.zeros(0)
            assert smp[int(off[l]):int(off[l + 1])].tobytes() == want.tobytes(), (name, l)
        return smp.size

    early = 0
    for p in range(pushes):
        chunks = [f[p * BLOCK:(p + 1) * BLOCK] for _, f in cases.recs[:LANES]]
        mk.push(np.concatenate(chunks), np.concatenate([[0], np.cumsum([c.shape[0] for c in chunks])]))
        early += both("a.push%d" % p, mk.frames())
    assert early > 0 and res["a.counts"].tolist() == R.counts()[0].tolist()
    assert res["a.released"].tolist() == R.counts()[1].tolist()
    for l in reversed(range(LANES)):
        total = cases.recs[l][1].shape[0] * 256 + 100
        mk.flush(l)
        both("a.flush%d" % l, mk.frames())
        R.flush(l, total)
        off, smp = _same(res, "a.flush%d.end" % l, R)
        assert smp.tobytes() == refs[l].flush(total).tobytes()
        P.flush(l, total)
        _same(res, "a.flush%d.rows.end" % l, P)
    assert res["a.released.end"].tolist() == R.counts()[1].tolist() == [300 * 256 + 100, 70 * 256 + 100]
    with pytest.raises(SsymError) as err:
        P.push(*ROWS)
    assert res["b.ended.code"][0] == float(err.value.code) == float(nat.SSYM_E_INVALID)
    P.reset(0)
    assert res["b.reset.code"][0] == 0.0
    P.push(*ROWS)
    _same(res, "b.again", P)
    P.flush(0, 3 * 256 + 77)
    _same(res, "b.flush", P)
    assert res["b.counts"].tolist() == P.counts()[0].tolist() == [3, 70]
    for h in (P, R, mk, store, d):
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
        d = e.dictionary(*pack_segments([f for _, f in cases.segs], 12, np.float64), 12)
        store = _store(e, cases)
        mk, P, R = e.mosaicker(d, LANES, PENALTIES[1], GAP), e.resynth(store, LANES), e.resynth(store, LANES, SEARCH)
        mk.push(cases.recs[1][1], [0, 70, 70])
        R.take(mk)

        def short():
            P.push(*ROWS)
            P.flush(0, 3 * 256 - 1)

        def empty():
            e.resynth(e.samples(np.zeros(0), np.zeros(1, dtype=np.uint64)))

        n = len(cases.segs)
        for name, call in (("l.twice", lambda: R.take(mk)), ("l.lane", lambda: P.flush(LANES, 0)), ("l.reset", lambda: P.reset(LANES)),
                           ("l.short", short), ("l.column", lambda: P.push([0], [7], [1], [3], [1])),
                           ("l.step", lambda: P.push([0], [3], [nat.COVER_GAP], [nat.NO_MATCH], [0])),
                           ("l.src", lambda: P.push([0], [3], [n], [0], [1])), ("l.search", lambda: e.resynth(store, 1, 513)),
                           ("l.lanes", lambda: e.resynth(store, 0)), ("l.empty", empty)):
            want = _code(call)
            assert want != 0.0 and res[name + ".code"][0] == want, (name, res[name + ".code"][0], want)
        assert res["l.twice.code"][0] == res["l.short.code"][0] == float(nat.SSYM_E_INVALID)
        rs = r.resynth(_store(r, cases), 1, 16)                 # either kind of context
        rs.push(*ROWS)
        _same(res, "l.refcos", rs)
        rs.close()
        for h in (R, P, mk):
            h.close()
    finally:
        e.close()
        r.close()
