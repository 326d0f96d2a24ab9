"""include/soundsym.hpp's SoundDictionary::mosaic, run by tests/cpp/test_mirror_mosaic.cpp ONCE on the planted intruder case
(tests/mosaic_ref.py, 12 values per frame as the mirror's sounds have), against the Python mirror (SoundDictionary.mosaic)
on the same sounds, call for call and bit for bit, and once against the restatement, so that a reading of the output layout
both mirrors share does not pass.  Refusals are compared by code: what Python raises for the same mistake (ValueError:
SSYM_E_INVALID; SsymError: its code) is the model."""
import os
import subprocess

import numpy as np
import pytest

import mirror_cases as mc
import mosaic_ref as ref
from soundsym_amd import HOP, EmptyDictionaryError, Engine, Sound, SoundDictionary, SsymError
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "cpp", "test_mirror_mosaic")
PENALTIES = (1.0, 0.0)
GAPS = (1.5, 0.0, 400.0, float("inf"))
GAP, NONE = ref.GAP, ref.NONE


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
    folder = str(tmp_path_factory.mktemp("mirror_mosaic"))
    case_file, result_file = os.path.join(folder, "cases.bin"), os.path.join(folder, "results.bin")
    arrays = {"penalties": np.array(PENALTIES), "gaps": np.array(GAPS)}
    for kind, sounds in (("seg", case.seg_sounds), ("tgt", case.tgt_sounds)):
        for i, (smp, feats) in enumerate(sounds):
            arrays["%s%d.samples" % (kind, i)] = smp
            arrays["%s%d.mfccs" % (kind, i)] = feats.reshape(-1)
    mc.write_arrays(case_file, arrays)
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "-f", "mosaic.mk"])
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


def _tiles(mosaic):
    """(src or SSYM_COVER_GAP, first, last, start, end, cost, frame_map) of a Python Mosaic's tiles: what the C++ pieces hold."""
    return [(GAP, NONE, NONE, p.start_frame, p.end_frame, p.cost, []) if p.is_gap else
            (p.source_index, p.source_first, p.source_last, p.start_frame, p.end_frame, p.cost, p.frame_map.tolist())
            for p in mosaic.pieces]


def _got_tiles(res, p, t):
    off, m_off = res[p + ".off"], res[p + ".map_off"]
    out = []
    for k in range(int(off[t]), int(off[t + 1])):
        out.append(tuple(int(res[p + "." + n][k]) for n in ("src", "first", "last", "start", "end")) +
                   (float(res[p + ".cost"][k]), res[p + ".map"][int(m_off[k]):int(m_off[k + 1])].tolist()))
    return out


def _same_mosaics(res, p, want):
    assert res[p + ".code"][0] == 0.0, (p, res[p + ".code"][0])
    off, total, fc_off = res[p + ".off"], res[p + ".total"], res[p + ".fc_off"]
    assert off.dtype == np.uint64 and off.size == len(want) + 1 and total.size == len(want)
    for t, w in enumerate(want):
        assert _bits(total[t])[0] == _bits(w.total)[0], (p, t, total[t], w.total)
        got, tiles = _got_tiles(res, p, t), _tiles(w)
        assert [g[:5] + g[6:] for g in got] == [x[:5] + x[6:] for x in tiles], (p, t)
        assert np.array_equal(_bits([g[5] for g in got]), _bits([x[5] for x in tiles])), (p, t)
        fc = res[p + ".fc"][int(fc_off[t]):int(fc_off[t + 1])]
        assert np.array_equal(_bits(fc), _bits(w.frame_costs if w else [])), (p, t)


def test_mosaic_call_for_call(res, world, case):
    for k, penalty in enumerate(PENALTIES):
        for g, gap in enumerate(GAPS):
            _same_mosaics(res, "a.p%d.g%d" % (k, g), world.S.mosaic(world.tgts, penalty, gap))
    _same_mosaics(res, "a.plain", world.S.mosaic(world.tgts, PENALTIES[0]))
    for t, tgt in enumerate(world.tgts):
        _same_mosaics(res, "b.t%d" % t, world.S.mosaic([tgt], PENALTIES[0], GAPS[0]))
    _same_mosaics(res, "m", world.S.mosaic([], 0.0, 1.0))
    # the planted intruder at penalty 1, gap_cost 1.5: the two planted pieces around ONE gap entry for the run of 4 frames
    got = _got_tiles(res, "a.p0.g0", 0)
    assert [g[:6] for g in got] == [case.planted[0] + (0.0,), (GAP, NONE, NONE, case.first, case.last, 6.0), case.planted[1] + (0.0,)]
    assert res["a.p0.g0.total"].tolist() == [8.0, 6.0, np.inf]
    # +inf is the call without a gap_cost
    for name in ("off", "src", "first", "last", "start", "end", "cost", "map", "total", "fc"):
        assert res["a.p0.g3." + name].tobytes() == res["a.plain." + name].tobytes()
    assert GAP not in res["a.plain.src"].tolist() and GAP in res["a.p0.g1.src"].tolist()


def test_mosaic_against_the_restatement(res, case):
    """The layout both mirrors read, held to tests/mosaic_ref.py once."""
    for (k, g) in ((0, 0), (1, 2)):
        p = "a.p%d.g%d" % (k, g)
        want = ref.arrays(case.segs, [x for _, x in case.tgt_sounds], PENALTIES[k], GAPS[g])
        off = np.concatenate([[0], np.cumsum([x.shape[0] for _, x in case.tgt_sounds])])
        for t in range(len(case.tgt_sounds)):
            assert _bits(res[p + ".total"][t])[0] == _bits(want[1][t])[0]
            merged = []
            for s, first, last, a, b in ref.pieces_of(want, off, t):
                if s == GAP and merged and merged[-1][0] == GAP:
                    merged[-1] = (GAP, NONE, NONE, merged[-1][3], b)
                else:
                    merged.append((s, first, last, a, b))
            assert [g_[:5] for g_ in _got_tiles(res, p, t)] == merged
            fc = res[p + ".fc"][int(res[p + ".fc_off"][t]):int(res[p + ".fc_off"][t + 1])]
            assert np.array_equal(_bits(fc), _bits(want[5][off[t]:off[t + 1]] if want[0][t] else []))


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
        for name, call in (("l.negative", lambda: world.S.mosaic(world.tgts, 0.0, -1.0)),
                           ("l.nan", lambda: world.S.mosaic(world.tgts, 0.0, float("nan"))),
                           ("l.ninf", lambda: world.S.mosaic(world.tgts, 0.0, -float("inf"))),
                           ("l.penalty", lambda: world.S.mosaic(world.tgts, -1.0, 1.0)),
                           ("l.empty", lambda: empty.mosaic(world.tgts, 0.0, 1.0)),
                           ("l.refcos", lambda: refcos.mosaic(world.tgts, 0.0, 1.0))):
            want = _code(call)
            assert want != 0.0 and res[name + ".code"][0] == want, (name, res[name + ".code"][0], want)
    finally:
        r.close()
    assert res["l.negative.code"][0] == float(nat.SSYM_E_INVALID) == res["l.nan.code"][0]
    assert res["l.refcos.code"][0] == float(nat.SSYM_E_UNSUPPORTED) and res["l.empty.code"][0] == float(nat.SSYM_E_EMPTY_DICT)
