"""include/soundsym.hpp's SoundDictionary::cover overload with gap_cost, run by tests/cpp/test_mirror_cover_gaps.cpp ONCE on
the planted-intruder case (tests/cover_gaps_ref.py, 12 values per frame as the mirror's sounds have), against the Python
mirror (SoundDictionary.cover(gap_cost=)) on the same sounds, call for call and bit for bit, and once against the
restatement, so that a reading of the output layout both mirrors share does not pass.  Refusals are compared by code: what
Python raises for the same mistake (ValueError: SSYM_E_INVALID; SsymError: its code) is the model."""
import os
import subprocess

import numpy as np
import pytest

import cover_gaps_ref as ref
import mirror_cases as mc
from soundsym_amd import HOP, EmptyDictionaryError, Engine, Sound, SoundDictionary, SsymError
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "cpp", "test_mirror_cover_gaps")
PENALTIES = (0.0, 2.5)
GAPS = (1.0, 0.0, 400.0, float("inf"))
GAP = ref.GAP


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).reshape(-1).view(np.uint64)


@pytest.fixture(scope="module")
def case():
    """The intruder case and two more targets: the intruder's frames alone, and no frames."""
    class C:
        pass
    c = C()
    c.segs, c.x, c.planted, (c.first, c.last) = ref.intruder_case(dim=12)
    rng = np.random.default_rng(0x6A95)
    sound = lambda feats: (rng.standard_normal(feats.shape[0] * HOP) * 0.1, feats)
    c.seg_sounds = [sound(s) for s in c.segs]
    c.tgt_sounds = [sound(x) for x in (c.x, c.x[c.first:c.last + 1], c.x[:0])]
    return c


@pytest.fixture(scope="module")
def res(case, tmp_path_factory):
    """The one run of the program and its parsed result file."""
    folder = str(tmp_path_factory.mktemp("mirror_cover_gaps"))
    case_file, result_file = os.path.join(folder, "cases.bin"), os.path.join(folder, "results.bin")
    arrays = {"penalties": np.array(PENALTIES), "gaps": np.array(GAPS)}
    for kind, sounds in (("seg", case.seg_sounds), ("tgt", case.tgt_sounds)):
        for i, (smp, feats) in enumerate(sounds):
            arrays["%s%d.samples" % (kind, i)] = smp
            arrays["%s%d.mfccs" % (kind, i)] = feats.reshape(-1)
    mc.write_arrays(case_file, arrays)
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "-f", "cover_gaps.mk"])
    r = subprocess.run([EXE, case_file, result_file], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and os.path.exists(result_file), "exit %r\n%s" % (r.returncode, r.stdout + r.stderr)
    return mc.read_arrays(result_file)


@pytest.fixture(scope="module")
def world(case):
    class W:
        pass
    w = W()
    w.e = Engine(metric="dtw", dtype="f64")
    snd = lambda pair: Sound(pair[0], mc.RATE, pair[1].reshape(-1))
    w.tgts, w.segs = ([snd(p) for p in x] for x in (case.tgt_sounds, case.seg_sounds))

    def dictionary(sounds, engine=None):
        d = SoundDictionary(engine=engine or w.e)
        d.sounds = list(sounds)
        return d
    w.dictionary = dictionary
    w.S = dictionary(w.segs)
    yield w
    w.e.close()


def _tiles(cover):
    """(src or SSYM_COVER_GAP, start, end, cost) of a Python Cover's tiles: what the C++ Cover's pieces hold."""
    return [(GAP if p.is_gap else p.source_index, p.start_frame, p.end_frame, p.cost) for p in cover.pieces]


def _same_covers(res, p, want):
    assert res[p + ".code"][0] == 0.0, (p, res[p + ".code"][0])
    off, total = res[p + ".off"], res[p + ".total"]
    assert off.dtype == np.uint64 and off.size == len(want) + 1 and total.size == len(want)
    for t, w in enumerate(want):
        a, b = int(off[t]), int(off[t + 1])
        tiles = _tiles(w)
        assert b - a == len(tiles) and _bits(total[t])[0] == _bits(w.total)[0], (p, t, total[t], w.total)
        got = list(zip(res[p + ".src"][a:b].tolist(), res[p + ".start"][a:b].tolist(), res[p + ".end"][a:b].tolist()))
        assert got == [x[:3] for x in tiles], (p, t)
        assert np.array_equal(_bits(res[p + ".cost"][a:b]), _bits([x[3] for x in tiles])), (p, t)


def test_cover_with_gaps_call_for_call(res, world, case):
    for k, penalty in enumerate(PENALTIES):
        for g, gap in enumerate(GAPS):
            _same_covers(res, "a.p%d.g%d" % (k, g), world.S.cover(world.tgts, penalty, gap))
    _same_covers(res, "a.plain", world.S.cover(world.tgts, PENALTIES[0]))
    for t, tgt in enumerate(world.tgts):
        _same_covers(res, "b.t%d" % t, world.S.cover([tgt], PENALTIES[0], GAPS[0]))
    _same_covers(res, "m", world.S.cover([], 0.0, 1.0))
    # the planted intruder at gap_cost 1: the planted pieces and ONE gap entry for the run of 7 frames
    p = "a.p0.g0"
    n = int(res[p + ".off"][1])
    got = list(zip(res[p + ".src"][:n].tolist(), res[p + ".start"][:n].tolist(), res[p + ".end"][:n].tolist(), res[p + ".cost"][:n].tolist()))
    assert got == [(s, a, e, 0.0) for s, a, e in case.planted[:3]] + [(GAP, case.first, case.last, 7.0)] + \
                  [(s, a, e, 0.0) for s, a, e in case.planted[3:]]
    assert res[p + ".total"].tolist() == [7.0, 7.0, np.inf]
    # +inf is the call without a gap_cost
    for name in ("off", "src", "start", "end", "cost", "total"):
        assert res["a.p0.g3." + name].tobytes() == res["a.plain." + name].tobytes()
    assert GAP not in res["a.plain.src"].tolist() and GAP in res["a.p0.g1.src"].tolist()


def test_cover_with_gaps_against_the_restatement(res, case):
    """The layout both mirrors read, held to tests/cover_gaps_ref.py once."""
    for (k, g) in ((1, 0), (0, 2)):
        p = "a.p%d.g%d" % (k, g)
        off = res[p + ".off"]
        for t, (_, x) in enumerate(case.tgt_sounds):
            pieces, total = ref.cover(case.segs, x, PENALTIES[k], GAPS[g])
            tiles = ref.merged(pieces)
            a, b = int(off[t]), int(off[t + 1])
            assert b - a == len(tiles) and _bits(res[p + ".total"][t])[0] == _bits(total)[0]
            got = list(zip(res[p + ".src"][a:b].tolist(), res[p + ".start"][a:b].tolist(), res[p + ".end"][a:b].tolist()))
            assert got == [w[:3] for w in tiles]
            assert np.array_equal(_bits(res[p + ".cost"][a:b]), _bits([w[3] for w in tiles]))


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
    empty = world.dictionary([])
    r = Engine(metric="refcos", dtype="f64")
    try:
        refcos = world.dictionary(world.S.sounds, r)
        for name, call in (("l.negative", lambda: world.S.cover(world.tgts, 0.0, -1.0)),
                           ("l.nan", lambda: world.S.cover(world.tgts, 0.0, float("nan"))),
                           ("l.ninf", lambda: world.S.cover(world.tgts, 0.0, -float("inf"))),
                           ("l.penalty", lambda: world.S.cover(world.tgts, -1.0, 1.0)),
                           ("l.empty", lambda: empty.cover(world.tgts, 0.0, 1.0)),
                           ("l.refcos", lambda: refcos.cover(world.tgts, 0.0, 1.0))):
            want = _code(call)
            assert want != 0.0 and res[name + ".code"][0] == want, (name, res[name + ".code"][0], want)
    finally:
        r.close()
    assert res["l.negative.code"][0] == float(nat.SSYM_E_INVALID) == res["l.nan.code"][0]
    assert res["l.refcos.code"][0] == float(nat.SSYM_E_UNSUPPORTED) and res["l.empty.code"][0] == float(nat.SSYM_E_EMPTY_DICT)
