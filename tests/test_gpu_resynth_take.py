"""ssym_resynth_take on the GPU: a mosaicker on tests/mosaic_ref.py's planted_case and intruder_case with synthetic samples
per recording, its frame logs taken device to device after pushes of 1 frame, of 7 frames and of all frames.  The samples
from reset to flush equal SoundDictionary.reconstruct_mosaic(mosaic=...) of the same frames, bit for bit, samples and pcm,
for search 0 and 64 and both gap_fills; a second take of one log is refused."""
import numpy as np
import pytest

import mirror_cases as mc
import mosaic_ref
from resynth_gpu import bits, same
from soundsym_amd import HOP, Engine, Sound, SoundDictionary, SsymError
from soundsym_amd import _native as nat
from soundsym_amd._native import COVER_GAP
from soundsym_amd.api import Mosaic, _mosaic_tiles

pytestmark = pytest.mark.gpu

CASES = {"planted": (mosaic_ref.planted_case, 1.0, None), "intruder": (mosaic_ref.intruder_case, 1.0, 1.5)}


@pytest.fixture(scope="module", params=sorted(CASES))
def world(request):
    class W:
        pass
    w = W()
    make, w.penalty, w.gap = CASES[request.param]
    w.recs, w.x = make()[:2]
    rng = np.random.default_rng(0x7A4E)
    w.rec_smp = [rng.standard_normal(a.shape[0] * HOP + 100) * 0.1 for a in w.recs]
    w.tgt_smp = rng.standard_normal(w.x.shape[0] * HOP + 777) * 0.1
    w.e = Engine(metric="dtw", dtype="f64")
    w.D = SoundDictionary(engine=w.e)
    dim = w.x.shape[1]
    w.D.sounds = [Sound(s, mc.RATE, a.reshape(-1), ncoeffs=dim) for s, a in zip(w.rec_smp, w.recs)]
    w.target = Sound(w.tgt_smp, mc.RATE, w.x.reshape(-1), ncoeffs=dim)
    w.want = {}
    yield w
    w.e.close()


def _run(w, block, search):
    """The target pushed `block` frames at a time into a one-lane mosaicker, every log taken: (frames as the mosaicker
    reported them, samples, pcm) from reset to flush."""
    mk = w.e.mosaicker(w.D.resident(), 1, w.penalty, w.gap)
    rs = w.e.resynth(w.D.resident_samples(), 1, search)
    rows, smp, pcm = [], [], []

    def take(n_frames):
        if n_frames:
            rows.append([a.copy() for a in mk.frames()])
        n = rs.take(mk)
        off, s, p = rs.samples(want_pcm32=True)
        assert n == s.size == p.size == int(off[1])
        smp.append(s), pcm.append(p)
        with pytest.raises(SsymError) as err:                  # the same log twice
            rs.take(mk)
        assert err.value.code == nat.SSYM_E_INVALID and "taken already" in str(err.value)
        assert rs.counts()[0][0] == sum(r[0].size for r in rows)

    try:
        for at in range(0, w.x.shape[0], block):
            take(mk.push(w.x[at:at + block]))
        take(mk.flush(0))
        rs.flush(0, w.tgt_smp.size)
        off, s, p = rs.samples(want_pcm32=True)
        smp.append(s), pcm.append(p)
    finally:
        rs.close()
        mk.close()
    cols = [np.concatenate([r[k] for r in rows]) for k in range(6)]
    return cols, np.concatenate(smp), np.concatenate(pcm)


@pytest.mark.parametrize("search", (0, 64))
@pytest.mark.parametrize("block", (1, 7, 1 << 20))
def test_taken_logs_resynthesise_to_reconstruct_mosaic(world, block, search):
    w = world
    (lane, col, src, frame, cost, start), smp, pcm = _run(w, block, search)
    assert col.tolist() == list(range(w.x.shape[0])) and smp.size == w.tgt_smp.size == pcm.size
    assert (w.gap is None) == (not (src == COVER_GAP).any())
    mosaic = Mosaic(_mosaic_tiles(np.flatnonzero(start), src, frame, cost), 0.0, col.size, cost)
    for gap_fill in ("silence", "target"):
        key = (search, gap_fill)
        if key not in w.want:
            w.want[key] = w.D.reconstruct_mosaic(w.target, gap_fill=gap_fill, search=search, want_pcm32=True, mosaic=mosaic)[1:]
        out, out_pcm = w.want[key]
        got, got_pcm = smp.copy(), pcm.copy()
        if gap_fill == "target":                              # the resynthesiser's gaps are +0.0; the host fills them
            gap = np.repeat(src == COVER_GAP, HOP)
            assert not got[:gap.size][gap].any()
            got[:gap.size][gap] = w.tgt_smp[:gap.size][gap]
            got_pcm[:gap.size][gap] = out_pcm[:gap.size][gap]
        same(got, out, "block %d, search %d, %s" % (block, search, gap_fill))
        assert np.array_equal(got_pcm, out_pcm)
    assert np.abs(smp).max() > 0


def test_take_refusals(world):
    w = world
    mk, two = w.e.mosaicker(w.D.resident(), 1, w.penalty, w.gap), w.e.mosaicker(w.D.resident(), 2, w.penalty, w.gap)
    rs = w.e.resynth(w.D.resident_samples(), 1)
    other = Engine(metric="dtw", dtype="f64")
    try:
        with pytest.raises(SsymError, match="no frame log yet"):
            rs.take(mk)
        with pytest.raises(ValueError, match="lanes"):
            rs.take(two)
        rc = nat.lib().ssym_resynth_take(w.e.ctx, rs.ptr, two.ptr, None)
        assert rc == nat.SSYM_E_INVALID
        import ctypes
        n = ctypes.c_uint64(9)
        assert nat.lib().ssym_resynth_take(w.e.ctx, rs.ptr, two.ptr, ctypes.byref(n)) == nat.SSYM_E_INVALID and n.value == 9
        assert nat.lib().ssym_resynth_take(other.ctx, rs.ptr, mk.ptr, ctypes.byref(n)) == nat.SSYM_E_INVALID
        committed = mk.push(w.x[:12])
        assert committed and rs.take(mk) >= 0
        late = w.e.resynth(w.D.resident_samples(), 1)
        for at in range(12, w.x.shape[0] + 4, 4):              # the next log that holds frames: it starts at column `committed`
            if mk.push(w.x[at:at + 4]) if at < w.x.shape[0] else mk.flush(0):
                break
        else:
            raise AssertionError("the mosaicker committed nothing more")
        try:
            with pytest.raises(SsymError, match="does not continue"):
                late.take(mk)                                  # a resynthesiser that has consumed nothing
            assert late.counts()[0][0] == 0
        finally:
            late.close()
        rs.flush(0, committed * HOP)
        with pytest.raises(SsymError, match="has ended"):
            rs.take(mk)                                        # the columns continue, but the lane was flushed
        frames, released = rs.counts()
        assert frames[0] == committed and released[0] == committed * HOP      # a refused take consumes nothing
    finally:
        other.close()
        rs.close()
        two.close()
        mk.close()
