"""ssym_reconstruct_wsola on the GPU against the restatement (tests/wsola_ref.py): positions and samples bit for bit,
since the definition fixes every rounding and the order of every sum -- host and device maps, host and device outputs,
every search width, ragged and long pairs, the length-fit fallback, empty targets, sources shorter than a window, more
targets than the search kernel has workgroups; no search = the plain warp; the chain match -> align -> wsola on the
recordings; beside a begin .. finish pair; every error the header lists; and a sinusoid that stays one."""
import os

import numpy as np
import pytest

import warp_ref
import wsola_ref as ref
from soundsym_amd import Engine, Sound, SoundDictionary, SoundSequence, SsymError, synth
from soundsym_amd import _native as nat
from soundsym_amd.api import HOP, NCOEFFS, frame_features
from soundsym_amd.engine import pack_segments
from test_wsola_ref import SINE_MAPS, sine_case, trimmed

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTF, SENT32, SENTP = -12345.5, -559038737, np.uint64(0xDEADBEEFCAFEF00D)
SEARCH_GRID = 2048                        # kWsolaMaxGrid: the search kernel's workgroups; targets beyond it: grid-stride


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.uint64)


def _raw(e, smp, idx, off, maps, m_off, frames, plen=None, search=0, map_device=False, out_device=False, want_out=True,
         want_pcm=True, want_pos=True, flags=None, null=(), s_ptr=True):
    """ssym_reconstruct_wsola through ctypes into sentinel-filled outputs: (rc, out, pcm, pos)."""
    import torch
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    m_off = np.ascontiguousarray(m_off, dtype=np.uint64)
    frames = np.ascontiguousarray(frames, dtype=np.uint32)
    maps = None if maps is None else np.ascontiguousarray(maps, dtype=np.uint32)
    plen = None if plen is None else np.ascontiguousarray(plen, dtype=np.uint32)
    total = int(off[-1]) if off.size else 0
    slots = int(m_off[-1]) if m_off.size else 0
    out = np.full(total + 4, SENTF)
    pcm = np.full(total + 4, SENT32, dtype=np.int32)
    pos = np.full(slots + 4, SENTP, dtype=np.uint64)
    keep = []
    fl = 0

    def dev(a):
        t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
        keep.append(t)
        return t.data_ptr() if t.numel() else None

    if map_device:
        fl |= nat.WARP_MAP_DEVICE
        map_p = None if maps is None else dev(maps)
        len_p = None if plen is None else dev(plen)
    else:
        map_p = None if maps is None or not maps.size else maps.ctypes.data
        len_p = None if plen is None else plen.ctypes.data
    if out_device:
        fl |= nat.OUT_DEVICE
        dout, dpcm = torch.from_numpy(out).cuda(), torch.from_numpy(pcm).cuda()
        dpos = torch.from_numpy(pos.view(np.int64)).cuda()
        out_p, pcm_p, pos_p = dout.data_ptr(), dpcm.data_ptr(), dpos.data_ptr()
        torch.cuda.synchronize()
    else:
        out_p, pcm_p, pos_p = out.ctypes.data, pcm.ctypes.data, pos.ctypes.data
    ptr = lambda name, p: None if name in null else p
    rc = nat.lib().ssym_reconstruct_wsola(
        e.ctx, smp.ptr if s_ptr else None, ptr("idx", idx.ctypes.data), ptr("off", off.ctypes.data), idx.size,
        ptr("map", map_p), ptr("moff", m_off.ctypes.data), ptr("frames", frames.ctypes.data), len_p, search,
        fl if flags is None else flags, pos_p if want_pos else None, out_p if want_out else None,
        pcm_p if want_pcm else None)
    if out_device:
        torch.cuda.synchronize()
        out, pcm, pos = dout.cpu().numpy(), dpcm.cpu().numpy(), dpos.cpu().numpy().view(np.uint64)
    assert (out[total:] == SENTF).all() and (pcm[total:] == SENT32).all() and (pos[slots:] == SENTP).all()
    return rc, out[:total], pcm[:total], pos[:slots]


def _untouched(res):
    return (res[1] == SENTF).all() and (res[2] == SENT32).all() and (res[3] == SENTP).all()


def _want_pos(pos_ref):
    """The restatement's positions as the sentinel-filled output must read: unset slots keep the sentinel."""
    return np.where(pos_ref == ref.UNSET, SENTP, pos_ref)


def _store(e, sounds):
    flat = np.concatenate(sounds) if sounds else np.zeros(0)
    return e.samples(flat, _offsets([s.size for s in sounds]))


def _case(rng, n_targets, lo=5, hi=40, n_sounds=24):
    """Ragged targets of lo ... hi frames on sources of every kind: long, shorter than a window (300 and 700 samples),
    empty; smooth periodic sources (where the search has something to find) and noise; monotone maps with repeats and
    skips, arbitrary maps, maps far beyond any source; targets without frames, without a path, of no samples."""
    s_len = rng.integers(2000, 14000, size=n_sounds)
    s_len[0], s_len[1], s_len[2], s_len[3] = (hi + 8) * HOP, 300, 0, 700
    sounds = []
    for i, v in enumerate(s_len):
        k = np.arange(int(v))
        if i % 2:
            sounds.append(rng.uniform(-1.0, 1.0, size=int(v)))
        else:
            f1, f2 = rng.uniform(60, 600, size=2)
            sounds.append(0.6 * np.sin(2 * np.pi * f1 * k / 44100.0 + rng.uniform(0, 6)) + 0.3 * np.sin(2 * np.pi * f2 * k / 44100.0)
                          + 0.02 * rng.standard_normal(int(v)))
    idx = rng.integers(0, n_sounds, size=n_targets).astype(np.uint32)
    frames = rng.integers(lo, hi + 1, size=n_targets).astype(np.uint32)
    lens = frames.astype(np.int64) * HOP + rng.integers(-255, 1024, size=n_targets)
    plen = rng.integers(1, 80, size=n_targets).astype(np.uint32)
    which = rng.random(n_targets)
    frames[which < 0.08] = 0                                   # no map frames: the length fit
    plen[(which > 0.08) & (which < 0.16)] = 0                  # no path: the length fit
    lens[(which > 0.16) & (which < 0.20)] = 0                  # an empty target
    if n_targets >= 6:
        idx[:6] = [0, 1, 2, 3, 0, 0]
        frames[:6], plen[:6] = np.maximum(frames[:6], lo), 1
        lens[:6] = frames[:6].astype(np.int64) * HOP + 700
        lens[5] = 0
    else:
        idx[0], plen[0], frames[0] = 0, 1, hi
        lens[0] = hi * HOP + 700
    room = frames.astype(np.int64) + rng.integers(0, 3, size=n_targets)
    m_off = _offsets(room) + np.uint64(3)                      # offsets need not start at 0
    maps = np.full(int(m_off[-1]), 0xABCDEF01, dtype=np.uint32)
    for t in range(n_targets):
        f, sf = int(frames[t]), int(s_len[idx[t]]) // HOP
        if not f:
            continue
        kind = t % 4
        if kind == 0:
            m = np.sort(rng.integers(0, max(sf, 1), size=f))
        elif kind == 1:
            m = np.minimum(np.arange(f) * max(sf, 1) // f, max(sf - 1, 0))          # a steady stretch, as DTW gives
        elif kind == 2:
            m = rng.integers(0, sf + 4, size=f)
        else:
            m = rng.integers(0, max(sf, 1), size=f)
            far = rng.integers(0, f, size=max(1, f // 5))
            m[far] = rng.choice([0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 0x01000000, sf, sf + 1, sf + 2], size=far.size)
        maps[int(m_off[t]):int(m_off[t]) + f] = m.astype(np.uint32)
    return sounds, idx, _offsets(lens), maps, m_off, frames, plen


def _check(e, smp, case, search, kws=(dict(),)):
    sounds, idx, off, maps, m_off, frames, plen = case
    want, want_pos = ref.wsola(sounds, idx, off, maps, m_off, frames, plen, search)
    first = None
    for kw in kws:
        rc, out, pcm, pos = _raw(e, smp, idx, off, maps, m_off, frames, plen, search, **kw)
        assert rc == nat.SSYM_OK, (kw, nat.lib().ssym_last_error(e.ctx))
        bad_pos = np.flatnonzero(pos != _want_pos(want_pos))
        bad = np.flatnonzero(_bits(out) != _bits(want))
        print("S %d %s: %d targets, %d positions (%d differ), %d samples (%d differ)" % (
            search, kw, idx.size, int(np.count_nonzero(want_pos != ref.UNSET)), bad_pos.size, want.size, bad.size))
        assert bad_pos.size == 0, (kw, bad_pos[:5], pos[bad_pos[:5]], want_pos[bad_pos[:5]])
        assert bad.size == 0, (kw, bad[:5], out[bad[:5]], want[bad[:5]])
        assert np.array_equal(pcm, ref.pcm32(out)), kw
        first = first or (out, pcm, pos)
    return first


ALL_PATHS = (dict(), dict(map_device=True), dict(out_device=True), dict(map_device=True, out_device=True))


# ---- 1. bit-equal to the restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("search", [0, 1, 64, 256, 512])
def test_equal_to_the_restatement_at_every_search_width(search):
    rng = np.random.default_rng(0x0A50 + search)
    n = 1 if search == 1 else 9
    case = _case(rng, n)
    e = Engine(metric="dtw", dtype="f64")
    smp = _store(e, case[0])
    out, pcm, pos = _check(e, smp, case, search, ALL_PATHS)
    sounds, idx, off, maps, m_off, frames, plen = case
    tm = e.timings()
    assert tm["reduce_ms"] > 0 and tm["total_ms"] >= tm["reduce_ms"] and tm["main_launches"] == 1 and tm["main_ms"] > 0
    # the targets without a map or without a path: ssym_reconstruct's bits, and no position written
    fit, fit_pcm = e.reconstruct(smp, idx, off, want_pcm32=True)
    for t in np.flatnonzero((frames == 0) | (plen == 0)):
        a, b = int(off[t]), int(off[t + 1])
        assert np.array_equal(_bits(out[a:b]), _bits(fit[a:b])) and np.array_equal(pcm[a:b], fit_pcm[a:b])
        assert (pos[int(m_off[t]):int(m_off[t + 1])] == SENTP).all()
    # one output at a time; no positions wanted; without pair_len every target with frames follows its map
    only = _raw(e, smp, idx, off, maps, m_off, frames, plen, search, want_pcm=False, want_pos=False)
    assert only[0] == nat.SSYM_OK and np.array_equal(_bits(only[1]), _bits(out)) and (only[2] == SENT32).all() and (only[3] == SENTP).all()
    only = _raw(e, smp, idx, off, maps, m_off, frames, plen, search, want_out=False)
    assert only[0] == nat.SSYM_OK and np.array_equal(only[2], pcm) and (only[1] == SENTF).all() and np.array_equal(only[3], pos)
    rc, out3, _, pos3 = _raw(e, smp, idx, off, maps, m_off, frames, None, search)
    want3, want_pos3 = ref.wsola(sounds, idx, off, maps, m_off, frames, None, search)
    assert rc == nat.SSYM_OK and np.array_equal(_bits(out3), _bits(want3)) and np.array_equal(pos3, _want_pos(want_pos3))
    # the Python layer, host and device maps
    import torch
    got, gpcm, gpos = e.reconstruct_wsola(smp, idx, off, maps, m_off, frames, plen, search, want_pcm32=True, want_pos=True)
    assert np.array_equal(_bits(got), _bits(out)) and np.array_equal(gpcm, pcm)
    assert np.array_equal(gpos, np.where(pos == SENTP, ref.UNSET, pos))
    dmaps, dlen = torch.from_numpy(maps.view(np.int32)).cuda(), torch.from_numpy(plen.view(np.int32)).cuda()
    assert np.array_equal(_bits(e.reconstruct_wsola(smp, idx, off, dmaps, m_off, frames, dlen, search)), _bits(out))
    e.close()


@pytest.mark.parametrize("n_targets", [40, SEARCH_GRID + 453])
def test_many_ragged_targets_and_more_than_the_search_grid(n_targets):
    # (a narrow search keeps the restatement affordable at thousands of targets; the kernel's path is the same)
    rng = np.random.default_rng(0x6A1D + n_targets)
    case = _case(rng, n_targets)
    e = Engine(metric="dtw", dtype="f64")
    smp = _store(e, case[0])
    _check(e, smp, case, 3 if n_targets > SEARCH_GRID else 48, (dict(), dict(map_device=True, out_device=True)))
    e.close()


def test_pairs_of_128_frames():
    rng = np.random.default_rng(0x128F)
    case = _case(rng, 6, lo=128, hi=128)
    e = Engine(metric="dtw", dtype="f64")
    smp = _store(e, case[0])
    _check(e, smp, case, 64, (dict(), dict(map_device=True, out_device=True)))
    e.close()


# ---- 2. no search: the plain warp ---------------------------------------------------------------------------------------

def test_no_search_is_reconstruct_warped_bit_for_bit():
    rng = np.random.default_rng(0x5EA0)
    sounds, idx, off, maps, m_off, frames, plen = _case(rng, 300)
    e = Engine(metric="dtw", dtype="f64")
    smp = _store(e, sounds)
    plain, plain_pcm = e.reconstruct_warped(smp, idx, off, maps, m_off, frames, plen, want_pcm32=True)
    for kw in (dict(), dict(map_device=True, out_device=True)):
        rc, out, pcm, pos = _raw(e, smp, idx, off, maps, m_off, frames, plen, 0, **kw)
        assert rc == nat.SSYM_OK and np.array_equal(_bits(out), _bits(plain)) and np.array_equal(pcm, plain_pcm)
        for t in range(idx.size):
            a, f = int(m_off[t]), int(frames[t]) if plen[t] else 0
            assert np.array_equal(pos[a:a + f], maps[a:a + f].astype(np.uint64) * np.uint64(HOP))
            assert (pos[a + f:int(m_off[t + 1])] == SENTP).all()
    # a diagonal map on noise: the search finds lag 0 everywhere, so today's output
    x = rng.standard_normal(30 * HOP + 99)
    smp2 = _store(e, [x])
    ident = np.arange(30, dtype=np.uint32)
    got, gpos = e.reconstruct_wsola(smp2, [0], [0, x.size], ident, [0, 30], [30], None, 256, want_pos=True)
    assert np.array_equal(gpos, ident.astype(np.uint64) * np.uint64(HOP))
    assert np.array_equal(_bits(got), _bits(e.reconstruct_warped(smp2, [0], [0, x.size], ident, [0, 30], [30])))
    e.close()


# ---- 3. the chain: match -> align (device outputs) -> wsola (device maps) ----------------------------------------------

def test_chain_on_the_reference_recordings():
    import torch
    from soundsym_amd import io as sio
    gold = os.path.join(ROOT, "tests", "golden")
    e = Engine(metric="dtw", dtype="f64")
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
    n, search = len(targets), 200
    L = nat.lib()
    d, smp = dictionary.resident(), dictionary.resident_samples()
    flat, f_off = pack_segments([t.mfccs() for t in targets], NCOEFFS, e.np_dtype)
    q = e.queries(flat, f_off, NCOEFFS)
    off = _offsets([t.samples().size for t in targets])
    idx, cost = np.zeros(n, dtype=np.uint32), np.zeros(n)
    nat.check(L.ssym_match_queries(e.ctx, d.ptr, q.ptr, None, 0, idx.ctypes.data, cost.ctypes.data, 0), e.ctx)
    p_off, m_off = e.dtw_align_sizes(d, q, idx)
    dcost = torch.empty(n, dtype=torch.float64, device="cuda")
    dlen = torch.empty(n, dtype=torch.int32, device="cuda")
    dpath = torch.empty(max(2 * int(p_off[-1]), 1), dtype=torch.int32, device="cuda")
    dmap = torch.full((max(int(m_off[-1]), 1),), 0x7ABCDEF0, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nat.check(L.ssym_dtw_align(e.ctx, d.ptr, q.ptr, idx.ctypes.data, None, n, 0, dcost.data_ptr(), dlen.data_ptr(),
                               p_off.ctypes.data, dpath.data_ptr(), m_off.ctypes.data, dmap.data_ptr(), nat.OUT_DEVICE), e.ctx)
    frames = np.diff(m_off.astype(np.int64)).astype(np.uint32)
    total = int(off[-1])
    out, pcm = np.full(total, SENTF), np.full(total, SENT32, dtype=np.int32)
    pos = np.full(int(m_off[-1]), SENTP, dtype=np.uint64)
    nat.check(L.ssym_reconstruct_wsola(e.ctx, smp.ptr, idx.ctypes.data, off.ctypes.data, n, dmap.data_ptr(), m_off.ctypes.data,
                                       frames.ctypes.data, dlen.data_ptr(), search, nat.WARP_MAP_DEVICE, pos.ctypes.data,
                                       out.ctypes.data, pcm.ctypes.data), e.ctx)
    q.close()
    maps, lengths = dmap.cpu().numpy().view(np.uint32), dlen.cpu().numpy().view(np.uint32)
    assert (lengths > 0).all()
    want, want_pos = ref.wsola([s.samples() for s in dictionary.sounds], idx, off, maps, m_off, frames, lengths, search)
    assert np.array_equal(pos, _want_pos(want_pos))
    assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(pcm, ref.pcm32(out))
    moved = np.count_nonzero(pos != maps[:pos.size].astype(np.uint64) * np.uint64(HOP))
    print("recordings: %d of %d frames moved by the search" % (moved, pos.size))
    assert moved > 0 and np.isfinite(out).all()
    assert np.abs(out).max() <= np.abs(s_smp).max() * (1 + 1e-12)          # every sample a weighted mean of source samples
    # the Python layer: three library calls of its own, the same arrays; search = 0 is the plain warp's output
    got, gpcm, gpos, g_off = dictionary.warp(targets, want_pcm32=True, search=search, want_pos=True)
    assert np.array_equal(_bits(got), _bits(out)) and np.array_equal(gpcm, pcm) and np.array_equal(gpos, pos)
    assert np.array_equal(g_off, m_off)
    seq = SoundSequence.new(targets).reconstruct_warped_from_dictionary(dictionary, search=search)
    assert np.array_equal(_bits(seq), _bits(out))
    plain = SoundSequence.new(targets).reconstruct_warped_from_dictionary(dictionary)
    assert np.array_equal(_bits(plain), _bits(dictionary.warp(targets, search=0))) and not np.array_equal(_bits(plain), _bits(out))
    e.close()


# ---- 4. beside the other calls of a context ----------------------------------------------------------------------------

def test_between_begin_and_finish_and_two_runs_alike():
    torch = pytest.importorskip("torch")
    g = synth.make_grid(256, 96, 32, 13, 0x5EED0A00)
    m = 96
    e = Engine(metric="dtw", dtype="f32")
    so, to = np.arange(257, dtype=np.uint64) * 32, np.arange(m + 1, dtype=np.uint64) * 32
    d, q = e.dictionary(g.sources.reshape(-1), so, 13), e.queries(g.targets.reshape(-1), to, 13)
    want_idx, want_cost = e.match(d, q, index_base=3)
    bounds = torch.empty(m, dtype=torch.float64, device="cuda")
    oi = torch.empty(m, dtype=torch.int32, device="cuda")
    oc = torch.empty(m, dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(0xBE62)
    sounds, idx, off, maps, m_off, frames, plen = _case(rng, 60)
    smp = _store(e, sounds)
    first = _raw(e, smp, idx, off, maps, m_off, frames, plen, 100)
    e.match_begin(d, q, bounds, index_base=3)
    between = _raw(e, smp, idx, off, maps, m_off, frames, plen, 100)
    e.match_finish(bounds, oi, oc)
    assert np.array_equal(oi.cpu().numpy().astype(np.int64), want_idx.astype(np.int64))
    assert np.array_equal(_bits(oc.cpu().numpy()), _bits(want_cost))
    after = _raw(e, smp, idx, off, maps, m_off, frames, plen, 100)
    want, want_pos = ref.wsola(sounds, idx, off, maps, m_off, frames, plen, 100)
    for res in (first, between, after):
        assert res[0] == nat.SSYM_OK and np.array_equal(_bits(res[1]), _bits(want)) and np.array_equal(res[2], first[2])
        assert np.array_equal(res[3], _want_pos(want_pos))
    e.close()


# ---- 5. errors ---------------------------------------------------------------------------------------------------------

def test_every_listed_error_leaves_the_outputs_untouched():
    rng = np.random.default_rng(0xE45)
    sounds = [rng.uniform(-1, 1, size=v) for v in (3000, 0, 900)]
    e = Engine(metric="dtw", dtype="f64")
    smp = _store(e, sounds)
    good = dict(idx=[0, 2, 1], off=[0, 2000, 2600, 3000], maps=np.arange(20, dtype=np.uint32) % 5, m_off=[0, 8, 12, 20],
                frames=[8, 3, 0], plen=[9, 0, 4], search=32)
    rc, out, pcm, pos = _raw(e, smp, **good)
    want, want_pos = ref.wsola(sounds, good["idx"], good["off"], good["maps"], good["m_off"], good["frames"], good["plen"], 32)
    assert rc == nat.SSYM_OK and np.array_equal(_bits(out), _bits(want)) and np.array_equal(pos, _want_pos(want_pos))

    def bad(code=nat.SSYM_E_INVALID, store=smp, **change):
        args = dict(good)
        args.update(change)
        for kw in (dict(), dict(map_device=True, out_device=True)):
            res = _raw(e, store, **args, **kw)
            assert res[0] == code and _untouched(res), (change, kw, res[0])
            assert nat.lib().ssym_last_error(e.ctx), change

    bad(s_ptr=False)
    for name in ("idx", "off", "moff", "frames"):
        bad(null=(name,))
    bad(null=("map",))                                                  # frames asked for, no map
    bad(search=513)
    bad(search=0xFFFFFFFF)
    bad(off=[1, 2000, 2600, 3000])
    bad(off=[0, 2600, 2000, 3000])
    bad(m_off=[0, 12, 8, 20])
    bad(m_off=[0, 7, 12, 20])                                           # room for 7 frames, 8 asked
    bad(idx=[0, 3, 1])
    bad(idx=[0, nat.NO_MATCH, 1])
    for flags in (2, 4, 8, 64, 0x80000000, nat.WARP_MAP_DEVICE | 16):
        bad(flags=flags)
    empty = e.samples(np.zeros(0), np.zeros(1, dtype=np.uint64))
    bad(code=nat.SSYM_E_EMPTY_DICT, store=empty)
    # nothing to do: success, nothing written -- no targets, no samples, no sample outputs (positions alone are no work)
    res = _raw(e, smp, [], [0], None, [0], [], search=32)
    assert res[0] == nat.SSYM_OK
    res = _raw(e, smp, [0, 2], [0, 0, 0], good["maps"], [0, 8, 12], [8, 3], search=32)
    assert res[0] == nat.SSYM_OK and _untouched(res)
    res = _raw(e, smp, **good, want_out=False, want_pcm=False)
    assert res[0] == nat.SSYM_OK and _untouched(res)
    # a NULL map is fine when no target has frames: the length fit throughout
    res = _raw(e, smp, good["idx"], good["off"], None, [0, 0, 0, 0], [0, 0, 0], search=32)
    fit = e.reconstruct(smp, good["idx"], good["off"])
    assert res[0] == nat.SSYM_OK and np.array_equal(_bits(res[1]), _bits(fit))
    # the Python layer raises what the library returns
    with pytest.raises(SsymError):
        e.reconstruct_wsola(smp, [0, 3, 1], good["off"], good["maps"], good["m_off"], good["frames"], search=32)
    e.close()


# ---- 6. what it is for ---------------------------------------------------------------------------------------------------

def test_a_sinusoid_stays_a_sinusoid_on_the_gpu():
    """The nine cases of test_wsola_ref.test_a_sinusoid_stays_a_sinusoid in one call, S = 256: the purity is the
    restatement's by bit-equality (0.99411 ... 0.99997 against the plain warp's 0.00112 ... 0.00331), asserted here all the
    same with the same bounds."""
    cases = [(f, k) + sine_case(f, k) for f in (97.0, 220.0, 313.0) for k in sorted(SINE_MAPS)]
    sounds = [c[2] for c in cases]
    maps = np.concatenate([c[3] for c in cases]).astype(np.uint32)
    frames = [len(c[3]) for c in cases]
    off, m_off = _offsets([c[4] for c in cases]), _offsets(frames)
    idx = np.arange(len(cases), dtype=np.uint32)
    e = Engine(metric="dtw", dtype="f64")
    smp = _store(e, sounds)
    out, pos = e.reconstruct_wsola(smp, idx, off, maps, m_off, frames, None, 256, want_pos=True)
    plain = e.reconstruct_warped(smp, idx, off, maps, m_off, frames)
    want, want_pos = ref.wsola(sounds, idx, off, maps, m_off, frames, None, 256)
    assert np.array_equal(pos, want_pos) and np.array_equal(_bits(out), _bits(want))
    for t, (freq, kind, _, _, _) in enumerate(cases):
        a, b = int(off[t]), int(off[t + 1])
        p_wsola, p_plain = ref.purity(trimmed(out[a:b]), freq, 44100.0), ref.purity(trimmed(plain[a:b]), freq, 44100.0)
        print("%5.0f Hz %-12s plain %.5f wsola %.5f" % (freq, kind, p_plain, p_wsola))
        assert p_wsola >= 0.99
        assert p_plain <= 0.05
    e.close()
