"""ssym_samples_create / ssym_reconstruct at every shape they accept, against tests/tail_ref.py; the oracle is
consulted once per case as a second opinion.

reconstruct_kernel handles 4096 samples per workgroup, 16 per thread in four groups of four, on a grid of
(ceil(longest target / 4096), n_targets): the lengths here cross every 256-stride and every chunk boundary, put whole
workgroups beyond a short target, and take the y extent past 65 535.  Everything is exact: samples as uint64 bit
patterns (so -0.0, NaN payloads and the +0.0 of the padding are pinned), pcm as int32."""
import ctypes
import os

import numpy as np
import pytest

import tail_ref
from soundsym_amd import Engine, Sound, SoundDictionary, SoundSequence, SsymError, synth
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu

LENS = [0, 1, 3, 255, 256, 257, 1023, 1024, 4095, 4096, 4097, 8191, 8192, 8193, 3 * 4096 + 1, 40000]
SENTF, SENT32 = -7.25, -1515870811            # 0xA5A5A5A5 as i32
M31 = 2147483647


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _store(rng, lens):
    """Sounds of the given lengths with a few special bit patterns among ordinary samples."""
    sounds = [rng.uniform(-1.1, 1.1, size=n) for n in lens]
    for s in sounds:
        if s.size >= 3:
            s[0], s[s.size // 2], s[-1] = -0.0, np.nan, -s[-1]
    smp = np.concatenate(sounds) if sounds else np.zeros(0)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return smp, off


def _offsets(tlen):
    return np.concatenate([[0], np.cumsum(tlen)]).astype(np.uint64)


def _check(e, oracle, smp, off, idx, ooff, h=None):
    """One call with both outputs against tail_ref (and the oracle); returns (samples, pcm)."""
    own = h is None
    if own:
        h = e.samples(smp, off)
    want = tail_ref.reconstruct(smp, off, idx, ooff)
    assert np.array_equal(_bits(want), _bits(oracle.reconstruct(smp, off, idx, ooff)))
    got, pcm = e.reconstruct(h, idx, ooff, want_pcm32=True)
    assert np.array_equal(_bits(got), _bits(want))
    probe = np.unique(np.concatenate([np.arange(0, want.size, 97), np.flatnonzero(np.isnan(want))[:50]])).astype(np.int64)
    assert pcm.dtype == np.int32 and np.array_equal(pcm[probe], tail_ref.pcm32_array(want[probe]))
    from soundsym_amd import io as sio
    assert np.array_equal(pcm, sio.pcm32(want))        # every sample, by the package's host conversion
    if own:
        h.close()
    return got, pcm


# ---- lengths ------------------------------------------------------------------------------------------------------------

def test_every_target_length_against_every_source_length(oracle):
    """16 target lengths x 17 source lengths (the same 16 and one longer than all): shorter, equal and longer sources
    at every target length."""
    rng = np.random.default_rng(0x5EC0)
    slens = LENS + [50000]
    smp, off = _store(rng, slens)
    idx = np.array([s for _ in LENS for s in range(len(slens))], dtype=np.uint32)
    tlen = np.array([t for t in LENS for _ in slens], dtype=np.uint64)
    for t in LENS:
        rel = {np.sign(s - t) for s in slens}
        assert rel == ({0, 1} if t == 0 else {-1, 0, 1})
    e = Engine(metric="refcos", dtype="f64")
    _check(e, oracle, smp, off, idx, _offsets(tlen))
    assert e.timings()["main_launches"] == 1
    e.close()


def test_one_long_target_among_many_short_ones(oracle):
    rng = np.random.default_rng(0x5EC1)
    smp, off = _store(rng, [40000, 5, 0, 300, 70000])
    tlen = rng.integers(0, 8, size=401).astype(np.uint64)
    tlen[200] = 40000                                   # ten workgroups per row, nine of them beyond every other target
    idx = rng.integers(0, 5, size=401).astype(np.uint32)
    idx[200] = 4
    e = Engine(metric="refcos", dtype="f64")
    _check(e, oracle, smp, off, idx, _offsets(tlen))
    idx[200] = 1                                        # ... and the long target filled from a 5-sample sound
    _check(e, oracle, smp, off, idx, _offsets(tlen))
    e.close()


# ---- counts -------------------------------------------------------------------------------------------------------------

def _max_grid_y():
    hip = ctypes.CDLL(nat.hip_runtime_path())
    v = ctypes.c_int(0)
    rc = hip.hipDeviceGetAttribute(ctypes.byref(v), 30, 0)        # hipDeviceAttributeMaxGridDimY
    return v.value if rc == 0 else None


@pytest.mark.parametrize("n_targets", [1, 2, 1000, 70000])
def test_target_counts(oracle, n_targets):
    rng = np.random.default_rng(0x5EC2 + n_targets)
    slens = rng.integers(0, 12, size=50)
    smp, off = _store(rng, slens)
    tlen = rng.integers(0, 8, size=n_targets).astype(np.uint64)
    idx = rng.integers(0, 50, size=n_targets).astype(np.uint32)
    print("maxGridSize[1] =", _max_grid_y(), " n_targets =", n_targets)
    e = Engine(metric="refcos", dtype="f64")
    _check(e, oracle, smp, off, idx, _offsets(tlen))
    e.close()


# ---- indices ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pick", ["same", "permutation", "last", "empty_sound"])
def test_indices(oracle, pick):
    rng = np.random.default_rng(0x5EC3)
    slens = [700, 0, 4097, 256, 1, 5000, 33, 9000]
    smp, off = _store(rng, slens)
    n = len(slens)
    idx = {"same": np.full(40, 2), "permutation": rng.permutation(n), "last": np.full(5, n - 1),
           "empty_sound": np.full(6, 1)}[pick].astype(np.uint32)
    tlen = rng.choice([0, 1, 255, 700, 4096, 4097, 9001], size=idx.size).astype(np.uint64)
    tlen[0] = 4097
    e = Engine(metric="refcos", dtype="f64")
    got, pcm = _check(e, oracle, smp, off, idx, _offsets(tlen))
    if pick == "empty_sound":
        assert not _bits(got).any() and not pcm.any()            # all padding: +0.0
    e.close()


# ---- outputs ------------------------------------------------------------------------------------------------------------

def _raw(e, h, idx, ooff, n, out, pcm):
    p = lambda a: None if a is None else a.ctypes.data
    return nat.lib().ssym_reconstruct(e.ctx, h, p(idx), p(ooff), n, p(out), p(pcm))


def test_which_outputs_are_written(oracle):
    rng = np.random.default_rng(0x5EC4)
    smp, off = _store(rng, [5000, 17, 0, 4096])
    idx = np.array([0, 3, 1, 2, 0], dtype=np.uint32)
    ooff = _offsets([4097, 5000, 300, 9, 0])
    total = int(ooff[-1])
    want = tail_ref.reconstruct(smp, off, idx, ooff)
    want_pcm = tail_ref.pcm32_array(want)
    assert np.array_equal(_bits(want), _bits(oracle.reconstruct(smp, off, idx, ooff)))
    assert np.array_equal(want_pcm, oracle.pcm32(want))
    e = Engine(metric="refcos", dtype="f64")
    h = e.samples(smp, off)
    for use_out, use_pcm in [(True, False), (False, True), (True, True), (False, False)]:
        out, pcm = np.full(total + 4, SENTF), np.full(total + 4, SENT32, dtype=np.int32)
        rc = _raw(e, h.ptr, idx, ooff, 5, out if use_out else None, pcm if use_pcm else None)
        assert rc == nat.SSYM_OK
        assert np.array_equal(_bits(out[:total]), _bits(want)) if use_out else (out == SENTF).all()
        assert np.array_equal(pcm[:total], want_pcm) if use_pcm else (pcm == SENT32).all()
        assert (out[total:] == SENTF).all() and (pcm[total:] == SENT32).all()
    # nothing to write: targets of no samples, and no targets
    out, pcm = np.full(4, SENTF), np.full(4, SENT32, dtype=np.int32)
    assert _raw(e, h.ptr, idx, np.zeros(6, dtype=np.uint64), 5, out, pcm) == nat.SSYM_OK
    assert _raw(e, h.ptr, idx, np.zeros(1, dtype=np.uint64), 0, out, pcm) == nat.SSYM_OK
    assert (out == SENTF).all() and (pcm == SENT32).all()
    h.close()
    e.close()


# ---- scratch ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("interleave", [False, True])
def test_scratch_regrowth(oracle, interleave):
    """Small call, large call, small call on one engine (with a match and a chain in between the second time): each
    equals the same call on a fresh engine."""
    rng = np.random.default_rng(0x5EC5)
    smp, off = _store(rng, [3000, 120000, 64, 0])
    calls = [(np.array([2, 0], dtype=np.uint32), _offsets([100, 50])),
             (rng.integers(0, 4, size=3000).astype(np.uint32), _offsets(rng.integers(0, 900, size=3000))),
             (np.array([1], dtype=np.uint32), _offsets([7]))]
    e = Engine(metric="refcos", dtype="f64")
    h = e.samples(smp, off)
    feats = rng.normal(size=(300, 4, 12))
    foff = np.arange(301, dtype=np.uint64) * 4
    d, q = e.dictionary(feats.reshape(-1), foff, 12), e.queries(feats[:90].reshape(-1), foff[:91], 12)
    for idx, ooff in calls:
        got, pcm = _check(e, oracle, smp, off, idx, ooff, h)
        fresh = Engine(metric="refcos", dtype="f64")
        fgot, fpcm = fresh.reconstruct(fresh.samples(smp, off), idx, ooff, want_pcm32=True)
        fresh.close()
        assert np.array_equal(_bits(got), _bits(fgot)) and np.array_equal(pcm, fpcm)
        if interleave:
            mi, _ = e.match(d, q)
            assert np.array_equal(mi, np.arange(90))
            e.chain(d, feats[0], [1.0, 0.5, 0.2])
    e.close()


# ---- between ssym_match_begin and ssym_match_finish ---------------------------------------------------------------------

@pytest.mark.parametrize("with_distance", [False, True])
def test_between_begin_and_finish(oracle, with_distance):
    """A reconstruct, a samples_create and a merge_shards between the two halves of a sharded step on the same context:
    finish returns what the uninterrupted sequence returns, bit for bit, or refuses -- never another answer.  With
    per-target distances the merge is given distances of its own, which land where begin left its."""
    torch = pytest.importorskip("torch")
    g = synth.make_grid(256, 96, 32, 13, 0x5EED0A00)
    m = 96
    e = Engine(metric="dtw", dtype="f32")
    so, to = np.arange(257, dtype=np.uint64) * 32, np.arange(m + 1, dtype=np.uint64) * 32
    d, q = e.dictionary(g.sources.reshape(-1), so, 13), e.queries(g.targets.reshape(-1), to, 13)
    rng = np.random.default_rng(0x5EC6)
    dist = rng.uniform(0.5, 2.0, size=m) * np.median(e.pair_matrix(d, q), axis=0) if with_distance else None
    want_idx, want_cost = e.match(d, q, distance=dist, index_base=3)
    bounds = torch.empty(m, dtype=torch.float64, device="cuda")
    oi = torch.empty(m, dtype=torch.int32, device="cuda")
    oc = torch.empty(m, dtype=torch.float64, device="cuda")
    e.match_begin(d, q, bounds, distance=dist, index_base=3)
    assert e.timings()["used_filter"] == 1
    # the three calls
    smp, off = _store(rng, [300000, 17])
    h = e.samples(smp, off)
    idx, ooff = rng.integers(0, 2, size=2000).astype(np.uint32), _offsets(rng.integers(0, 600, size=2000))
    _check(e, oracle, smp, off, idx, ooff, h)
    costs = torch.from_numpy(rng.integers(0, 9, size=(3, 500)).astype(np.float64)).cuda()
    sidx = torch.from_numpy(rng.integers(0, 1000, size=(3, 500)).astype(np.int32)).cuda()
    mdist = rng.uniform(0, 9, size=500) if with_distance else None
    mi, mc = torch.empty(500, dtype=torch.int32, device="cuda"), torch.empty(500, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    e.merge_shards(costs, sidx, mi, mc, mdist)
    wi, wc = tail_ref.merge(costs.cpu().numpy(), sidx.cpu().numpy(), mdist)
    assert np.array_equal(mi.cpu().numpy(), wi) and np.array_equal(mc.cpu().numpy(), wc)
    try:
        e.match_finish(bounds, oi, oc)
    except SsymError as err:
        assert with_distance and "without ssym_match_begin" in str(err)      # the documented refusal
    else:
        assert np.array_equal(oi.cpu().numpy().astype(np.int64), want_idx.astype(np.int64))
        assert np.array_equal(_bits(oc.cpu().numpy()), _bits(want_cost))
    # and the context is as good as new
    again_idx, again_cost = e.match(d, q, distance=dist, index_base=3)
    assert np.array_equal(again_idx, want_idx) and np.array_equal(_bits(again_cost), _bits(want_cost))
    e.close()


# ---- conversion ---------------------------------------------------------------------------------------------------------

def test_conversion_edges_and_seeded_values(oracle):
    na = np.nextafter
    edges = [0.0, -0.0, 1.0, -1.0, na(1.0, 0.0), na(-1.0, 0.0), na(1.0, np.inf), na(-1.0, -np.inf), 0.5, -0.5,
             1.0 / M31, -1.0 / M31, 0.9 / M31, -0.9 / M31, 1.9 / M31, -1.9 / M31, np.inf, -np.inf, np.nan,
             5e-324, -5e-324, 1e300, -1e300]
    by_hand = [0, 0, M31, -M31, M31 - 1, -(M31 - 1), M31, -M31, 1073741823, -1073741823,
               1, -1, 0, 0, 1, -1, M31, -M31 - 1, 0, 0, 0, M31, -M31 - 1]     # worked out in tests/test_tail_ref.py
    rng = np.random.default_rng(0x5EC7)
    vals = np.concatenate([np.array(edges, dtype=np.float64), rng.uniform(-1.2, 1.2, size=10000)])
    want = tail_ref.pcm32_array(vals)
    assert want[:len(edges)].tolist() == by_hand
    assert np.array_equal(want, oracle.pcm32(vals))
    e = Engine(metric="refcos", dtype="f64")
    h = e.samples(vals, [0, vals.size])
    out, pcm = e.reconstruct(h, [0], [0, vals.size + 3], want_pcm32=True)
    assert np.array_equal(_bits(out[:vals.size]), _bits(vals)) and not _bits(out[vals.size:]).any()
    assert np.array_equal(pcm[:vals.size], want) and pcm[vals.size:].tolist() == [0, 0, 0]
    e.close()


# ---- errors -------------------------------------------------------------------------------------------------------------

def test_samples_create_errors():
    e = Engine(metric="refcos", dtype="f64")
    L = nat.lib()
    smp = np.arange(10, dtype=np.float64)

    def create(samples, offsets, n):
        out = ctypes.c_void_p(0x1234)
        p = lambda a: None if a is None else a.ctypes.data
        rc = L.ssym_samples_create(e.ctx, p(samples), p(offsets), n, ctypes.byref(out))
        return rc, out.value

    u64 = lambda *v: np.array(v, dtype=np.uint64)
    for samples, offsets, n in [(smp, None, 2), (smp, u64(1, 4, 10), 2), (smp, u64(0, 6, 4), 2), (None, u64(0, 4, 10), 2)]:
        rc, ptr = create(samples, offsets, n)
        assert rc == nat.SSYM_E_INVALID and not ptr and L.ssym_last_error(e.ctx)
    rc, ptr = create(None, u64(0, 0, 0), 2)              # NULL samples are fine when there are none
    assert rc == nat.SSYM_OK and ptr
    out, pcm = np.full(3, SENTF), np.full(3, SENT32, dtype=np.int32)
    assert _raw(e, ptr, np.array([1], dtype=np.uint32), u64(0, 3), 1, out, pcm) == nat.SSYM_OK
    assert not _bits(out).any() and not pcm.any()
    L.ssym_samples_destroy(e.ctx, ptr)
    rc, ptr = create(smp, u64(0), 0)                     # a store of no sounds exists, and cannot be gathered from
    assert rc == nat.SSYM_OK and ptr
    out, pcm = np.full(3, SENTF), np.full(3, SENT32, dtype=np.int32)
    assert _raw(e, ptr, np.array([0], dtype=np.uint32), u64(0, 3), 1, out, pcm) == nat.SSYM_E_EMPTY_DICT
    assert (out == SENTF).all() and (pcm == SENT32).all()
    L.ssym_samples_destroy(e.ctx, ptr)
    e.close()


def test_reconstruct_errors_leave_the_outputs_untouched(oracle):
    rng = np.random.default_rng(0x5EC8)
    smp, off = _store(rng, [100, 50, 7])
    e = Engine(metric="refcos", dtype="f64")
    h = e.samples(smp, off)
    good_idx, good_off = np.array([0, 2, 1], dtype=np.uint32), _offsets([60, 60, 60])
    u64 = lambda *v: np.array(v, dtype=np.uint64)
    cases = {
        "store": dict(h=None), "idx": dict(idx=None), "offsets": dict(ooff=None),
        "offsets[0] != 0": dict(ooff=u64(1, 60, 120, 180)), "decreasing offsets": dict(ooff=u64(0, 120, 60, 180)),
        "index == n": dict(idx=np.array([0, 3, 1], dtype=np.uint32)),
        "SSYM_NO_MATCH": dict(idx=np.array([0, 1, nat.NO_MATCH], dtype=np.uint32)),
    }
    for name, kw in cases.items():
        out, pcm = np.full(200, SENTF), np.full(200, SENT32, dtype=np.int32)
        args = dict(h=h.ptr, idx=good_idx, ooff=good_off)
        args.update(kw)
        rc = _raw(e, args["h"], args["idx"], args["ooff"], 3, out, pcm)
        assert rc == nat.SSYM_E_INVALID, name
        assert (out == SENTF).all() and (pcm == SENT32).all(), name
        assert nat.lib().ssym_last_error(e.ctx), name
    _check(e, oracle, smp, off, good_idx, good_off, h)              # the context still works
    assert e.timings()["main_launches"] == 1
    e.close()


# ---- the Python layer ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ["refcos", "dtw"])
def test_reconstruct_from_dictionary_on_the_reference_recordings(metric):
    from soundsym_amd import io as sio
    from soundsym_amd.api import HOP, frame_features
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    e = Engine(metric=metric, dtype="f64")
    s_smp, srate = sio.read_wav(os.path.join(gold, "audio", "sample.wav"))
    t_smp, rate = sio.read_wav(os.path.join(gold, "audio", "Section_7_1.wav"))
    seg = 16 * HOP
    lens = [seg] * (s_smp.size // seg) + ([s_smp.size % seg] if s_smp.size % seg else [])
    source = Sound(s_smp, srate, frame_features(s_smp, srate, engine=e))
    dictionary = SoundDictionary.from_segments(source, lens, engine=e)
    dictionary.sounds = [x for x in dictionary.sounds if x.num_frames() > 0]
    targets = []
    for a, b, label in sio.audacity_labels_to_timestamps(os.path.join(gold, "vowel.txt")):
        piece = t_smp[int(round(a * rate)):int(round(b * rate)) + 1]
        if piece.size >= HOP:
            targets.append(Sound(piece, rate, frame_features(piece, rate, engine=e), label))
    assert len(dictionary.sounds) == 284 and len(targets) == 55
    seq = SoundSequence.new(targets)
    got, pcm = seq.reconstruct_from_dictionary(dictionary, want_pcm32=True)
    host = seq.clone_from_dictionary(dictionary).to_sound().samples()          # the host path of the mirror
    assert got.size == sum(t.samples().size for t in targets)
    assert np.array_equal(_bits(got), _bits(host))
    assert np.array_equal(pcm, sio.pcm32(host))
    assert np.array_equal(pcm[::13], tail_ref.pcm32_array(host[::13]))
    e.close()
