"""include/soundsym.hpp's SoundDictionary::cover, run by tests/cpp/test_mirror_cover.cpp ONCE on sounds of
tests/mirror_cases.py, against the Python mirror (SoundDictionary.cover) on the same sounds, call for call and bit for bit,
and once against the restatement (tests/cover_ref.py), so that a reading of the output layout both mirrors share does not
pass.  Refusals are compared by code: what Python raises for the same mistake (ValueError: SSYM_E_INVALID; SsymError: its
code) is the model."""
import os
import subprocess

import numpy as np
import pytest

import cover_ref
import mirror_cases as mc
from soundsym_amd import EmptyDictionaryError, Engine, Sound, SoundDictionary, SsymError
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "cpp", "test_mirror_cover")
PENALTIES = (0.0, 2.5, 40.0)
SEGMENTS = 4                       # segments of 4, 17, 33 and 66 frames; the fifth has 130, more than a cover takes


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).reshape(-1).view(np.uint64)


@pytest.fixture(scope="module")
def cases():
    c = mc.build()
    c.args = {"penalties": np.array(PENALTIES), "cover.segments": np.array([SEGMENTS], dtype=np.uint64)}
    return c


@pytest.fixture(scope="module")
def res(cases, tmp_path_factory):
    """The one run of the program and its parsed result file."""
    folder = str(tmp_path_factory.mktemp("mirror_cover"))
    case_file, result_file = os.path.join(folder, "cases.bin"), os.path.join(folder, "results.bin")
    mc.write_arrays(case_file, cases.arrays())
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "-f", "cover.mk"])
    r = subprocess.run([EXE, case_file, result_file], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and os.path.exists(result_file), "exit %r\n%s" % (r.returncode, r.stdout + r.stderr)
    return mc.read_arrays(result_file)


@pytest.fixture(scope="module")
def world(cases, res):
    class W:
        pass
    w = W()
    w.e = Engine(metric="dtw", dtype="f64")
    snd = lambda pair: Sound(pair[0], mc.RATE, pair[1].reshape(-1))
    w.recs, w.tgts, w.segs = ([snd(p) for p in x] for x in (cases.recs, cases.tgts, cases.segs))

    def dictionary(sounds, engine=None):
        d = SoundDictionary(engine=engine or w.e)
        d.sounds = list(sounds)
        return d
    w.dictionary = dictionary
    w.S = dictionary(w.segs[:SEGMENTS])
    yield w
    w.e.close()


def _same_covers(res, p, want):
    assert res[p + ".code"][0] == 0.0, (p, res[p + ".code"][0])
    off, total = res[p + ".off"], res[p + ".total"]
    assert off.dtype == np.uint64 and off.size == len(want) + 1 and total.size == len(want)
    for name in ("src", "start", "end"):
        assert res["%s.%s" % (p, name)].dtype == np.uint32 and res["%s.%s" % (p, name)].size == int(off[-1])
    for t, w in enumerate(want):
        a, b = int(off[t]), int(off[t + 1])
        assert b - a == len(w) and _bits(total[t])[0] == _bits(w.total)[0], (p, t, total[t], w.total)
        got = list(zip(res[p + ".src"][a:b].tolist(), res[p + ".start"][a:b].tolist(), res[p + ".end"][a:b].tolist()))
        assert got == [(x.source_index, x.start_frame, x.end_frame) for x in w.pieces], (p, t)
        assert np.array_equal(_bits(res[p + ".cost"][a:b]), _bits([x.cost for x in w.pieces])), (p, t)


def test_cover_call_for_call(res, world):
    for k, penalty in enumerate(PENALTIES):
        _same_covers(res, "a.p%d" % k, world.S.cover(world.tgts, penalty))
    _same_covers(res, "a.default", world.S.cover(world.tgts))
    for t, tgt in enumerate(world.tgts):
        _same_covers(res, "b.t%d" % t, world.S.cover([tgt], PENALTIES[1]))
    T = world.dictionary(world.tgts)
    _same_covers(res, "c.self", T.cover(world.tgts))
    _same_covers(res, "c.segs", T.cover(world.S.sounds, PENALTIES[1]))
    _same_covers(res, "m", world.S.cover([]))
    # the penalties do something: fewer pieces for the 65-frame target, and every target covers itself at no cost
    counts = [int(np.diff(res["a.p%d.off" % k])[4]) for k in range(3)]
    assert counts[0] > counts[2] >= 1
    assert (res["c.self.total"][[0, 1, 2, 3, 4]] == 0.0).all() and res["c.self.total"][5] == np.inf


def test_cover_against_the_restatement(res, cases):
    """The layout both mirrors read, held to tests/cover_ref.py once."""
    segs = [f for _, f in cases.segs[:SEGMENTS]]
    for k, penalty in ((1, PENALTIES[1]),):
        p = "a.p%d" % k
        off = res[p + ".off"]
        for t, (_, x) in enumerate(cases.tgts):
            pieces, total = cover_ref.cover(segs, x, penalty)
            a, b = int(off[t]), int(off[t + 1])
            assert b - a == len(pieces) and _bits(res[p + ".total"][t])[0] == _bits(total)[0]
            got = list(zip(res[p + ".src"][a:b].tolist(), res[p + ".start"][a:b].tolist(), res[p + ".end"][a:b].tolist()))
            assert got == [w[:3] for w in pieces]
            assert np.array_equal(_bits(res[p + ".cost"][a:b]), _bits([w[3] for w in pieces]))
    assert int(off[-1]) > 6


def _code(call):
    try:
        call()
    except ValueError:
        return float(nat.SSYM_E_INVALID)
    except EmptyDictionaryError as e:
        return float(e.code)
    except SsymError as e:
        return float(e.code)
    return 0.0


def test_refusals_by_code(res, world):
    long_segs, long_recs = world.dictionary(world.segs), world.dictionary(world.recs)
    empty = world.dictionary([])
    r = Engine(metric="refcos", dtype="f64")
    try:
        refcos = world.dictionary(world.S.sounds, r)
        for name, call in (("l.long.segs", lambda: long_segs.cover(world.tgts)), ("l.long.recs", lambda: long_recs.cover(world.tgts)),
                           ("l.negative", lambda: world.S.cover(world.tgts, -1.0)),
                           ("l.nan", lambda: world.S.cover(world.tgts, float("nan"))),
                           ("l.inf", lambda: world.S.cover(world.tgts, float("inf"))),
                           ("l.empty", lambda: empty.cover(world.tgts)), ("l.empty.empty", lambda: empty.cover([])),
                           ("l.refcos", lambda: refcos.cover(world.tgts))):
            want = _code(call)
            assert want != 0.0 and res[name + ".code"][0] == want, (name, res[name + ".code"][0], want)
    finally:
        r.close()
    assert res["l.long.segs.code"][0] == float(nat.SSYM_E_UNSUPPORTED) == res["l.refcos.code"][0]
    assert res["l.empty.code"][0] == float(nat.SSYM_E_EMPTY_DICT) and res["l.negative.code"][0] == float(nat.SSYM_E_INVALID)
