"""ssym_reconstruct_warped on the GPU against the restatement (tests/warp_ref.py): bit for bit, since the definition
fixes every rounding -- across target counts, ragged lengths, sources shorter / longer / empty, any map content, the
length-fit fallback, host and device maps, host and device outputs, the 32-bit conversion; the three-call chain match ->
align -> warp with the maps left on the device, on synthetic sets and on the recordings; the Python layer; every error
the header lists."""
import os

import numpy as np
import pytest

import warp_ref as ref
from soundsym_amd import Engine, Sound, SoundDictionary, SoundSequence, SsymError, synth
from soundsym_amd import _native as nat
from soundsym_amd.api import HOP, NCOEFFS, analyze_mfccs, frame_features
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTF, SENT32 = -12345.5, -559038737


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.uint64)


def _raw(e, smp, idx, off, maps, m_off, frames, plen=None, map_device=False, out_device=False, want_out=True,
         want_pcm=True, flags=None, null=(), s_ptr=True):
    """ssym_reconstruct_warped through ctypes into sentinel-filled outputs: (rc, out, pcm)."""
    import torch
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    m_off = np.ascontiguousarray(m_off, dtype=np.uint64)
    frames = np.ascontiguousarray(frames, dtype=np.uint32)
    maps = None if maps is None else np.ascontiguousarray(maps, dtype=np.uint32)
    plen = None if plen is None else np.ascontiguousarray(plen, dtype=np.uint32)
    total = int(off[-1]) if off.size else 0
    out = np.full(total + 4, SENTF)
    pcm = np.full(total + 4, SENT32, dtype=np.int32)
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
        out_p, pcm_p = dout.data_ptr(), dpcm.data_ptr()
        torch.cuda.synchronize()
    else:
        out_p, pcm_p = out.ctypes.data, pcm.ctypes.data
    ptr = lambda name, p: None if name in null else p
    rc = nat.lib().ssym_reconstruct_warped(
        e.ctx, smp.ptr if s_ptr else None, ptr("idx", idx.ctypes.data), ptr("off", off.ctypes.data), idx.size,
        ptr("map", map_p), ptr("moff", m_off.ctypes.data), ptr("frames", frames.ctypes.data), len_p,
        fl if flags is None else flags, out_p if want_out else None, pcm_p if want_pcm else None)
    if out_device:
        torch.cuda.synchronize()
        out, pcm = dout.cpu().numpy(), dpcm.cpu().numpy()
    assert (out[total:] == SENTF).all() and (pcm[total:] == SENT32).all()          # nothing beyond the output
    return rc, out[:total], pcm[:total]


def _untouched(res):
    return (res[1] == SENTF).all() and (res[2] == SENT32).all()


def _case(rng, n_targets, n_sounds=48):
    """A sample store and a call's arguments that cover the ground the header states: ragged targets of 5 ... 40
    frames whose lengths are no multiples of 256, a few of 0 ... 40 000 samples, sources shorter and longer than their
    targets and empty ones, repeated indices, monotone and arbitrary maps with values far beyond any source, targets
    without map frames and targets without a path."""
    s_len = rng.integers(0, 12000, size=n_sounds)
    s_len[rng.integers(0, n_sounds, size=4)] = 0
    s_len[0], s_len[1] = 45000, 300
    sounds = [rng.uniform(-1.0, 1.0, size=int(v)) for v in s_len]
    idx = rng.integers(0, n_sounds, size=n_targets).astype(np.uint32)
    frames = rng.integers(5, 41, size=n_targets).astype(np.uint32)
    lens = frames.astype(np.int64) * HOP + rng.integers(-255, 1024, size=n_targets)
    big = rng.integers(0, n_targets, size=max(1, min(6, n_targets // 2)))
    lens[big] = rng.integers(0, 40001, size=big.size)
    plen = rng.integers(1, 80, size=n_targets).astype(np.uint32)
    which = rng.random(n_targets)
    frames[which < 0.08] = 0                                   # no map frames: the length fit
    plen[(which > 0.08) & (which < 0.16)] = 0                  # no path: the length fit
    if n_targets >= 7:                                         # lengths around the 4096-sample chunk, the longest target
        lens[:7] = [0, 1, 4095, 4096, 4097, 8193, 40000]
        idx[:7] = [0, 0, 0, 1, 0, 2, 0]
        frames[3:7], plen[3:7] = [16, 17, 33, 157], 1
    else:
        lens[0], idx[0], frames[0], plen[0] = 8191 + 4096, 0, 40, 1
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
            m[far] = rng.choice([0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 0x01000000, 0x00FFFFFF, sf, sf + 1], size=far.size)
        maps[int(m_off[t]):int(m_off[t]) + f] = m.astype(np.uint32)
    return sounds, idx, _offsets(lens), maps, m_off, frames, plen


def _store(e, sounds):
    flat = np.concatenate(sounds) if sounds else np.zeros(0)
    return e.samples(flat, _offsets([s.size for s in sounds]))


# ---- 1. bit-equal to the restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n_targets", [1, 7, 300, 4096])
def test_equal_to_the_restatement_on_every_path(n_targets):
    rng = np.random.default_rng(0x3A2F + n_targets)
    sounds, idx, off, maps, m_off, frames, plen = _case(rng, n_targets)
    e = Engine(metric="dtw", dtype="f64")
    smp = _store(e, sounds)
    want = ref.warp(sounds, idx, off, maps, m_off, frames, plen)
    rc, out, pcm = _raw(e, smp, idx, off, maps, m_off, frames, plen)
    assert rc == nat.SSYM_OK, nat.lib().ssym_last_error(e.ctx)
    differ = np.flatnonzero(_bits(out) != _bits(want))
    print("n_targets %d: %d samples, %d differ in bits from the restatement" % (n_targets, want.size, differ.size))
    assert differ.size == 0, (differ[:5], out[differ[:5]], want[differ[:5]])
    assert np.array_equal(pcm, ref.pcm32(out))
    tm = e.timings()
    assert tm["main_launches"] == 1 and tm["main_ms"] > 0 and tm["total_ms"] == tm["main_ms"]
    # the targets without a map or without a path: ssym_reconstruct's bits
    fit, fit_pcm = e.reconstruct(smp, idx, off, want_pcm32=True)
    for t in np.flatnonzero((frames == 0) | (plen == 0)):
        a, b = int(off[t]), int(off[t + 1])
        assert np.array_equal(_bits(out[a:b]), _bits(fit[a:b])) and np.array_equal(pcm[a:b], fit_pcm[a:b])
    # the same call again; the map and lengths in device memory; the outputs in device memory; both
    for kw in (dict(), dict(map_device=True), dict(out_device=True), dict(map_device=True, out_device=True)):
        rc2, out2, pcm2 = _raw(e, smp, idx, off, maps, m_off, frames, plen, **kw)
        assert rc2 == nat.SSYM_OK, kw
        assert np.array_equal(_bits(out2), _bits(out)) and np.array_equal(pcm2, pcm), kw
    # one output at a time; without pair_len every target with frames follows its map
    only = _raw(e, smp, idx, off, maps, m_off, frames, plen, want_pcm=False)
    assert only[0] == nat.SSYM_OK and np.array_equal(_bits(only[1]), _bits(out)) and (only[2] == SENT32).all()
    only = _raw(e, smp, idx, off, maps, m_off, frames, plen, want_out=False)
    assert only[0] == nat.SSYM_OK and np.array_equal(only[2], pcm) and (only[1] == SENTF).all()
    if n_targets <= 300:
        rc3, out3, _ = _raw(e, smp, idx, off, maps, m_off, frames, None)
        assert rc3 == nat.SSYM_OK and np.array_equal(_bits(out3), _bits(ref.warp(sounds, idx, off, maps, m_off, frames)))
        # the Python layer, host and device maps
        import torch
        got, gpcm = e.reconstruct_warped(smp, idx, off, maps, m_off, frames, plen, want_pcm32=True)
        assert np.array_equal(_bits(got), _bits(out)) and np.array_equal(gpcm, pcm)
        dmaps, dlen = torch.from_numpy(maps.view(np.int32)).cuda(), torch.from_numpy(plen.view(np.int32)).cuda()
        assert np.array_equal(_bits(e.reconstruct_warped(smp, idx, off, dmaps, m_off, frames, dlen)), _bits(out))
    e.close()


def test_long_targets_and_identity_maps():
    # one target of many chunks whose map is the identity: the sound comes back (to rounding), every chunk boundary
    # included; and the same target from a source half as long: zeros beyond where the source's frames reach
    rng = np.random.default_rng(0x1DE)
    n = 40 * 4096 + 77
    x = rng.uniform(-1, 1, size=n)
    frames = n // HOP
    ident = np.arange(frames, dtype=np.uint32)
    e = Engine(metric="dtw", dtype="f64")
    smp = _store(e, [x, x[:n // 2]])
    off, m_off = _offsets([n, n]), _offsets([frames, frames])
    rc, out, pcm = _raw(e, smp, [0, 1], off, np.concatenate([ident, ident]), m_off, [frames, frames])
    assert rc == nat.SSYM_OK
    want = ref.warp([x, x[:n // 2]], [0, 1], off, np.concatenate([ident, ident]), m_off, [frames, frames])
    assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(pcm, ref.pcm32(out))
    k = np.arange(1, frames * HOP)
    assert (np.abs(out[k] - x[k]) <= 4 * 2.0 ** -52 * np.abs(x[k])).all()
    assert (_bits(out[n + n // 2:]) == 0).all()
    e.close()


# ---- 2. the chain: match -> align (device outputs) -> warp (device maps) -----------------------------------------------

def _chain(e, d, q, smp, n, off):
    """The three library calls with the alignment left on the device; returns (out, pcm, idx, maps, lengths, m_off)
    with the maps and lengths read back afterwards for the restatement."""
    import torch
    L = nat.lib()
    idx, cost = np.zeros(n, dtype=np.uint32), np.zeros(n)
    nat.check(L.ssym_match_queries(e.ctx, d.ptr, q.ptr, None, 0, idx.ctypes.data, cost.ctypes.data, 0), e.ctx)
    p_off, m_off = e.dtw_align_sizes(d, q, idx)
    dcost = torch.empty(n, dtype=torch.float64, device="cuda")
    dlen = torch.empty(n, dtype=torch.int32, device="cuda")
    dpath = torch.empty(max(2 * int(p_off[-1]), 1), dtype=torch.int32, device="cuda")
    dmap = torch.full((max(int(m_off[-1]), 1),), 0x7ABCDEF0, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nat.check(L.ssym_dtw_align(e.ctx, d.ptr, q.ptr, idx.ctypes.data, None, n, 0, dcost.data_ptr(), dlen.data_ptr(),
                               p_off.ctypes.data, dpath.data_ptr(), m_off.ctypes.data, dmap.data_ptr(), nat.OUT_DEVICE),
              e.ctx)
    frames = np.diff(m_off.astype(np.int64)).astype(np.uint32)
    total = int(off[-1])
    out, pcm = np.full(total, SENTF), np.full(total, SENT32, dtype=np.int32)
    nat.check(L.ssym_reconstruct_warped(e.ctx, smp.ptr, idx.ctypes.data, off.ctypes.data, n, dmap.data_ptr(),
                                        m_off.ctypes.data, frames.ctypes.data, dlen.data_ptr(), nat.WARP_MAP_DEVICE,
                                        out.ctypes.data, pcm.ctypes.data), e.ctx)
    return out, pcm, idx, dmap.cpu().numpy().view(np.uint32), dlen.cpu().numpy().view(np.uint32), m_off, dcost.cpu().numpy(), cost


def _check_chain(dictionary, targets):
    e = dictionary.engine
    n = len(targets)
    flat, f_off = pack_segments([t.mfccs() for t in targets], NCOEFFS, e.np_dtype)
    q = e.queries(flat, f_off, NCOEFFS)
    off = _offsets([t.samples().size for t in targets])
    out, pcm, idx, maps, lengths, m_off, acost, mcost = _chain(e, dictionary.resident(), q, dictionary.resident_samples(), n, off)
    q.close()
    frames = np.diff(m_off.astype(np.int64))
    assert np.array_equal(frames, [t.num_frames() for t in targets])
    assert np.array_equal(_bits(acost[lengths > 0]), _bits(mcost[lengths > 0]))
    want = ref.warp([s.samples() for s in dictionary.sounds], idx, off, maps, m_off, frames, lengths)
    assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(pcm, ref.pcm32(out))
    # the maps are ssym_dtw_align's own: what the host path of the same call returns
    _, hlen, _, hmaps = e.dtw_align(dictionary.resident(), e.queries(flat, f_off, NCOEFFS), idx)
    assert np.array_equal(hlen, lengths)
    for t in range(n):
        if lengths[t]:
            assert np.array_equal(hmaps[t], maps[int(m_off[t]):int(m_off[t + 1])])
    # the Python layer: three library calls of its own, the same array
    got, gpcm = dictionary.warp(targets, want_pcm32=True)
    assert np.array_equal(_bits(got), _bits(out)) and np.array_equal(gpcm, pcm)
    seq = SoundSequence.new(targets).reconstruct_warped_from_dictionary(dictionary)
    assert np.array_equal(_bits(seq), _bits(out))
    assert np.array_equal(_bits(dictionary.warp(targets, indices=idx)), _bits(out))
    # beside the length fit: same length, same targets, and different wherever a match had to be stretched
    plain = SoundSequence.new(targets).reconstruct_from_dictionary(dictionary)
    assert plain.size == out.size
    return out, idx, lengths, plain


@pytest.mark.parametrize("shape", [(40, 30, 5, 40), (200, 150, 5, 40), (12, 9, 60, 130)])
def test_chain_on_ragged_synthetic_sets(shape):
    n_src, n_tgt, lo, hi = shape
    rng = np.random.default_rng(0xC4A1 + n_src)
    e = Engine(metric="dtw", dtype="f64")

    def make(n):
        samples = [rng.uniform(-1, 1, size=int(rng.integers(lo, hi + 1)) * HOP + int(rng.integers(0, HOP))) for _ in range(n)]
        feats = analyze_mfccs(samples, 44100.0, NCOEFFS, e, pad_tail=True)
        return [Sound(s, 44100.0, f) for s, f in zip(samples, feats)]

    dictionary = SoundDictionary(engine=e)
    dictionary.sounds = make(n_src)
    targets = make(n_tgt)
    targets[1] = Sound(rng.uniform(-1, 1, size=100), 44100.0, np.zeros(0))        # no frames: no path, the length fit
    out, idx, lengths, plain = _check_chain(dictionary, targets)
    assert lengths[1] == 0 and (lengths[np.arange(n_tgt) != 1] > 0).all()
    a, b = int(np.sum([t.samples().size for t in targets[:1]])), int(np.sum([t.samples().size for t in targets[:2]]))
    assert np.array_equal(_bits(out[a:b]), _bits(plain[a:b]))
    e.close()


def test_chain_on_the_reference_recordings():
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
    out, idx, lengths, plain = _check_chain(dictionary, targets)
    assert (lengths > 0).all() and np.isfinite(out).all()
    assert np.abs(out).max() <= np.abs(s_smp).max() * (1 + 1e-12)          # every sample a weighted mean of source samples
    # targets longer than their 16-frame match: the length fit leaves silence where the warp still plays the match
    off = _offsets([t.samples().size for t in targets])
    longer = [t for t in range(55) if targets[t].num_frames() > 18]
    assert longer
    sounding = 0
    for t in longer:
        tail = slice(int(off[t]) + 17 * HOP, int(off[t]) + (targets[t].num_frames() - 1) * HOP)
        assert (plain[tail] == 0).all()
        sounding += int(np.count_nonzero(out[tail]))
    assert sounding > 0
    e.close()


# ---- 3. beside the other calls of a context ----------------------------------------------------------------------------

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
    rng = np.random.default_rng(0xBE61)
    sounds, idx, off, maps, m_off, frames, plen = _case(rng, 500)
    smp = _store(e, sounds)
    first = _raw(e, smp, idx, off, maps, m_off, frames, plen)
    e.match_begin(d, q, bounds, index_base=3)
    between = _raw(e, smp, idx, off, maps, m_off, frames, plen)
    e.match_finish(bounds, oi, oc)
    assert np.array_equal(oi.cpu().numpy().astype(np.int64), want_idx.astype(np.int64))
    assert np.array_equal(_bits(oc.cpu().numpy()), _bits(want_cost))
    after = _raw(e, smp, idx, off, maps, m_off, frames, plen)
    want = ref.warp(sounds, idx, off, maps, m_off, frames, plen)
    for res in (first, between, after):
        assert res[0] == nat.SSYM_OK and np.array_equal(_bits(res[1]), _bits(want)) and np.array_equal(res[2], first[2])
    e.close()


# ---- 4. errors ---------------------------------------------------------------------------------------------------------

def test_every_listed_error_leaves_the_outputs_untouched():
    rng = np.random.default_rng(0xE44)
    sounds = [rng.uniform(-1, 1, size=v) for v in (3000, 0, 900)]
    e = Engine(metric="dtw", dtype="f64")
    smp = _store(e, sounds)
    good = dict(idx=[0, 2, 1], off=[0, 2000, 2600, 3000], maps=np.arange(20, dtype=np.uint32) % 5, m_off=[0, 8, 12, 20],
                frames=[8, 3, 0], plen=[9, 0, 4])
    rc, out, pcm = _raw(e, smp, **good)
    assert rc == nat.SSYM_OK and np.array_equal(_bits(out), _bits(ref.warp(sounds, good["idx"], good["off"], good["maps"],
                                                                      good["m_off"], good["frames"], good["plen"])))

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
    # nothing to do: success, nothing written -- no targets, no samples, no outputs
    res = _raw(e, smp, [], [0], None, [0], [])
    assert res[0] == nat.SSYM_OK
    res = _raw(e, smp, [0, 2], [0, 0, 0], good["maps"], [0, 8, 12], [8, 3])
    assert res[0] == nat.SSYM_OK
    res = _raw(e, smp, **good, want_out=False, want_pcm=False)
    assert res[0] == nat.SSYM_OK and _untouched(res)
    # a NULL map is fine when no target has frames: the length fit throughout
    res = _raw(e, smp, good["idx"], good["off"], None, [0, 0, 0, 0], [0, 0, 0])
    fit = e.reconstruct(smp, good["idx"], good["off"])
    assert res[0] == nat.SSYM_OK and np.array_equal(_bits(res[1]), _bits(fit))
    # the Python layer raises what the library returns
    with pytest.raises(SsymError):
        e.reconstruct_warped(smp, [0, 3, 1], good["off"], good["maps"], good["m_off"], good["frames"])
    e.close()


def test_a_refcos_engine_is_refused_in_python():
    rng = np.random.default_rng(2)
    e = Engine(metric="refcos", dtype="f64")
    sounds = [rng.uniform(-1, 1, size=2000)]
    smp = _store(e, sounds)
    with pytest.raises(SsymError) as err:
        e.reconstruct_warped(smp, [0], [0, 1500], [0, 1, 2, 3], [0, 4], [4])
    assert err.value.code == nat.SSYM_E_UNSUPPORTED
    d = SoundDictionary(engine=e)
    d.sounds = [Sound(sounds[0], 44100.0, rng.standard_normal(7 * NCOEFFS))]
    with pytest.raises(SsymError) as err:
        d.warp([d.sounds[0]])
    assert err.value.code == nat.SSYM_E_UNSUPPORTED
    with pytest.raises(SsymError):
        SoundSequence.new([d.sounds[0]]).reconstruct_warped_from_dictionary(d)
    e.close()
