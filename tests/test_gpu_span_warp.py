"""ssym_reconstruct_warped_spans and ssym_reconstruct_wsola_spans on the GPU against the existing calls on a store made of the
slices, bit for bit: samples, their 32-bit conversion and the searched positions -- windows at the start, in the middle and
at the end of sounds of 0 to 70 000 samples, empty windows, maps that repeat, skip and run past the window, every search
width, the length-fit fallbacks, device maps and device outputs; samples outside the windows poisoned; the errors."""
import numpy as np
import pytest

import span_ref
from soundsym_amd import Engine
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu

SOUNDS = (0, 1, 1023, 5000, 70000)
KINDS = ("diagonal", "repeats", "skips", "past")
F = 6                                         # target frames of a map
SENTF, SENT32, SENTP = -12345.5, -559038737, np.uint64(0xDEADBEEFCAFEF00D)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _windows(n):
    """(first, len) of the windows a sound of n samples takes: all of it, (1, 1024), (255, 257), (768, 1280), its last sample,
    an empty one."""
    cand = [(0, n), (1, 1024), (255, 257), (768, 1280), (n - 1, 1), (min(n, 700), 0)]
    return [(a, k) for a, k in cand if a >= 0 and a + k <= n]


def _map(kind, win_len, rng):
    wf = win_len // 256 + 1
    if kind == "diagonal":
        return np.arange(F)
    if kind == "repeats":
        return np.arange(F) // 2
    if kind == "skips":
        return (np.arange(F) * 2 + rng.integers(0, 2, size=F)) % max(wf, 1)
    m = np.arange(F) + max(wf - 3, 0)         # runs past the window's last frame
    m[-1] = 0xFFFFFFFF
    return m


class _Case:
    """Every (sound, window, map kind) as one target; fallbacks on a few of them."""

    def __init__(self):
        rng = np.random.default_rng(0x5BA9)
        self.sounds = [rng.normal(size=n) * 0.3 for n in SOUNDS]
        idx, first, length, maps, frames, out_len = [], [], [], [], [], []
        for s, n in enumerate(SOUNDS):
            for a, k in _windows(n):
                for kind in KINDS:
                    idx.append(s), first.append(a), length.append(k)
                    maps.append(_map(kind, k, rng))
                    frames.append(F)
                    out_len.append((F * 256 + 300, 1500, 100, F * 256 + 1024)[len(idx) % 4])
        self.idx = np.array(idx, dtype=np.uint32)
        self.first, self.length = np.array(first, dtype=np.uint64), np.array(length, dtype=np.uint64)
        self.frames = np.array(frames, dtype=np.uint32)
        self.frames[5::11] = 0                                                     # F = 0: the length fit
        self.pair_len = np.where(np.arange(len(idx)) % 7 == 3, 0, 11).astype(np.uint32)      # pair_len = 0: the length fit
        out_len[2] = 0                                                             # a target without output samples
        self.m_off = np.concatenate([[0], np.cumsum([F + 1] * len(idx))]).astype(np.uint64)  # (one slack slot per target)
        self.maps = np.zeros(int(self.m_off[-1]), dtype=np.uint32)
        for t, m in enumerate(maps):
            self.maps[int(self.m_off[t]):int(self.m_off[t]) + F] = m
        self.o_off = np.concatenate([[0], np.cumsum(out_len)]).astype(np.uint64)
        self.n = len(idx)
        self.slices = span_ref.slices(self.sounds, self.idx, self.first, self.length)

    def store(self, e, sounds):
        off = np.concatenate([[0], np.cumsum([x.size for x in sounds])]).astype(np.uint64)
        return e.samples(np.concatenate(sounds), off)


@pytest.fixture(scope="module")
def case():
    return _Case()


@pytest.fixture(scope="module")
def eng():
    e = Engine(metric="dtw", dtype="f64")
    yield e
    e.close()


@pytest.fixture(scope="module")
def stores(eng, case):
    """(the sounds, the slices: sound t is target t's window)."""
    return case.store(eng, case.sounds), case.store(eng, case.slices)


def _run(e, smp, c, idx, windows, search, maps=None, pair_len="own"):
    """(samples, pcm, pos or None) of the warped call (search None) or the WSOLA call, with or without windows."""
    pl = c.pair_len if isinstance(pair_len, str) else pair_len
    args = (smp, idx, c.o_off, c.maps if maps is None else maps, c.m_off, c.frames, pl)
    kw = {} if windows is None else {"windows": windows}
    if search is None:
        out, pcm = e.reconstruct_warped(*args, want_pcm32=True, **kw)
        return out, pcm, None
    return e.reconstruct_wsola(*args, search=search, want_pcm32=True, want_pos=True, **kw)


@pytest.fixture(scope="module")
def answers(eng, case, stores):
    """The existing calls on the store of slices, computed once: search -> (samples, pcm, pos)."""
    return {s: _run(eng, stores[1], case, np.arange(case.n), None, s) for s in (None, 0, 7, 512)}


def _assert_same(got, want, what):
    assert np.array_equal(_bits(got[0]), _bits(want[0])), what
    assert np.array_equal(got[1], want[1]), what
    if want[2] is not None:
        assert np.array_equal(got[2], want[2]), what


def test_the_case_holds_what_it_should(case):
    assert case.n == len(KINDS) * sum(len(_windows(n)) for n in SOUNDS) and case.n > 60
    assert {(int(a), int(k)) for a, k in zip(case.first, case.length)} >= {(0, 70000), (1, 1024), (255, 257), (768, 1280),
                                                                            (69999, 1), (4999, 1), (700, 0), (0, 0), (0, 1)}
    assert (case.frames == 0).any() and (case.pair_len == 0).any() and (np.diff(case.o_off.astype(np.int64)) == 0).any()
    past = [(int(case.maps[int(case.m_off[t]):int(case.m_off[t]) + F].max()) + 1) * 256 > int(case.length[t]) for t in range(case.n)]
    assert sum(past) > case.n // 4                                                  # maps that reach past their window


@pytest.mark.parametrize("search", [None, 0, 7, 512])
def test_windows_equal_the_existing_call_on_the_slices(eng, case, stores, answers, search):
    got = _run(eng, stores[0], case, case.idx, (case.first, case.length), search)
    _assert_same(got, answers[search], "search %r" % (search,))
    if search == 0:
        assert np.array_equal(_bits(got[0]), _bits(answers[None][0]))               # no search: the plain warp
    if search == 512:
        assert not np.array_equal(got[2], answers[7][2])                            # (the widths do differ here)


def test_the_restatement_agrees(case, answers):
    """tests/span_ref.py on the targets of the 1023-sample sound, where the CPU loops are quick."""
    keep = [t for t in range(case.n) if case.idx[t] == 2]
    sub = lambda x: np.asarray(x)[keep]
    frames, pl = sub(case.frames), sub(case.pair_len)
    m_off = np.concatenate([[0], np.cumsum([F + 1] * len(keep))]).astype(np.uint64)
    maps = np.concatenate([case.maps[int(case.m_off[t]):int(case.m_off[t + 1])] for t in keep])
    o_len = np.diff(case.o_off.astype(np.int64))[keep]
    o_off = np.concatenate([[0], np.cumsum(o_len)]).astype(np.uint64)
    want = span_ref.warp_spans(case.sounds, sub(case.idx), sub(case.first), sub(case.length), o_off, maps, m_off, frames, pl)
    got = np.concatenate([answers[None][0][int(case.o_off[t]):int(case.o_off[t + 1])] for t in keep])
    assert np.array_equal(_bits(got), _bits(want))
    want, _ = span_ref.wsola_spans(case.sounds, sub(case.idx), sub(case.first), sub(case.length), o_off, maps, m_off, frames, pl, 7)
    got = np.concatenate([answers[7][0][int(case.o_off[t]):int(case.o_off[t + 1])] for t in keep])
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("search", [None, 7, 512])
def test_samples_outside_the_windows_are_never_read(eng, case, answers, search):
    """One copy of its sound per target, NaN in every sample outside the target's window: all outputs keep their bits."""
    copies, first = [], []
    for t in range(case.n):
        a, k = int(case.first[t]), int(case.length[t])
        lo, hi = max(a - 2000, 0), min(a + k + 4000, SOUNDS[case.idx[t]])            # (a stretch around the window is enough)
        x = np.full(hi - lo, np.nan)
        x[a - lo:a - lo + k] = case.sounds[case.idx[t]][a:a + k]
        copies.append(x)
        first.append(a - lo)
    smp = case.store(eng, copies)
    try:
        got = _run(eng, smp, case, np.arange(case.n), (np.array(first, dtype=np.uint64), case.length), search)
    finally:
        smp.close()
    _assert_same(got, answers[search], "poisoned, search %r" % (search,))
    assert not np.isnan(got[0]).any()


def test_device_maps_and_device_outputs(eng, case, stores, answers):
    import torch
    dmaps = torch.from_numpy(case.maps.view(np.int32)).cuda()
    dlen = torch.from_numpy(case.pair_len.view(np.int32)).cuda()
    torch.cuda.synchronize()
    for search in (None, 7):
        got = _run(eng, stores[0], case, case.idx, (case.first, case.length), search, maps=dmaps, pair_len=dlen)
        _assert_same(got, answers[search], "device maps, search %r" % (search,))
    # SSYM_OUT_DEVICE, through ctypes: samples, pcm and positions land in the caller's device arrays
    total, slots = int(case.o_off[-1]), int(case.m_off[-1])
    out = torch.full((total,), SENTF, dtype=torch.float64, device="cuda")
    pcm = torch.full((total,), SENT32, dtype=torch.int32, device="cuda")
    pos = torch.from_numpy(np.full(slots, SENTP, dtype=np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    rc = nat.lib().ssym_reconstruct_wsola_spans(
        eng.ctx, stores[0].ptr, case.idx.ctypes.data, case.first.ctypes.data, case.length.ctypes.data, case.o_off.ctypes.data,
        case.n, dmaps.data_ptr(), case.m_off.ctypes.data, case.frames.ctypes.data, dlen.data_ptr(), 7,
        nat.OUT_DEVICE | nat.WARP_MAP_DEVICE, pos.data_ptr(), out.data_ptr(), pcm.data_ptr())
    torch.cuda.synchronize()
    assert rc == nat.SSYM_OK
    want = answers[7]
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want[0])) and np.array_equal(pcm.cpu().numpy(), want[1])
    hpos = pos.cpu().numpy().view(np.uint64)
    live = want[2] != np.iinfo(np.uint64).max
    assert np.array_equal(hpos[live], want[2][live]) and (hpos[~live] == SENTP).all()
    out.fill_(SENTF)
    torch.cuda.synchronize()
    rc = nat.lib().ssym_reconstruct_warped_spans(
        eng.ctx, stores[0].ptr, case.idx.ctypes.data, case.first.ctypes.data, case.length.ctypes.data, case.o_off.ctypes.data,
        case.n, dmaps.data_ptr(), case.m_off.ctypes.data, case.frames.ctypes.data, dlen.data_ptr(),
        nat.OUT_DEVICE | nat.WARP_MAP_DEVICE, out.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == nat.SSYM_OK and np.array_equal(_bits(out.cpu().numpy()), _bits(answers[None][0]))


def test_lags_that_would_reach_before_the_window_are_not_admissible(eng, case, stores):
    """A window that starts mid-recording, a map that goes back to its first frame: the lags -512 ... -1 of nominal position 0
    would read the recording before the window; they are cut off as they are at the start of a sound."""
    idx = np.array([3], dtype=np.uint32)
    first, length = np.array([768], dtype=np.uint64), np.array([1280], dtype=np.uint64)
    maps, m_off, frames = np.array([1, 0, 0, 2, 1], dtype=np.uint32), np.array([0, 5], dtype=np.uint64), np.array([5], dtype=np.uint32)
    o_off = np.array([0, 2000], dtype=np.uint64)
    cut = case.store(eng, [case.sounds[3][768:768 + 1280].copy()])
    try:
        want = eng.reconstruct_wsola(cut, [0], o_off, maps, m_off, frames, search=512, want_pos=True)
    finally:
        cut.close()
    got = eng.reconstruct_wsola(stores[0], idx, o_off, maps, m_off, frames, search=512, want_pos=True, windows=(first, length))
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])
    ref, ref_pos = span_ref.wsola_spans(case.sounds, idx, first, length, o_off, maps, m_off, frames, None, 512)
    assert np.array_equal(got[1], ref_pos) and np.array_equal(_bits(got[0]), _bits(ref))
    assert (got[1] < 1280).all() and got[1][1] <= 512 and got[1][2] <= 512          # relative to the window, never before it


@pytest.mark.parametrize("first,length", [(0, 5001), (5000, 1), (5001, 0), (2 ** 63, 2 ** 63), (2 ** 64 - 1, 2)])
def test_windows_beyond_their_sound_are_refused_with_the_outputs_unwritten(eng, case, stores, first, length):
    idx = np.array([3, 3], dtype=np.uint32)
    wf, wl = np.array([0, first], dtype=np.uint64), np.array([5000, length], dtype=np.uint64)
    assert span_ref.window_status(SOUNDS, idx, [0, first], [5000, length]) == span_ref.E_INVALID
    o_off, m_off = np.array([0, 300, 600], dtype=np.uint64), np.array([0, 2, 4], dtype=np.uint64)
    maps, frames = np.zeros(4, dtype=np.uint32), np.array([2, 2], dtype=np.uint32)
    out, pcm, pos = np.full(600, SENTF), np.full(600, SENT32, dtype=np.int32), np.full(4, SENTP, dtype=np.uint64)
    L = nat.lib()
    head = (eng.ctx, stores[0].ptr, idx.ctypes.data, wf.ctypes.data, wl.ctypes.data, o_off.ctypes.data, 2, maps.ctypes.data,
            m_off.ctypes.data, frames.ctypes.data, None)
    assert L.ssym_reconstruct_warped_spans(*head, 0, out.ctypes.data, pcm.ctypes.data) == nat.SSYM_E_INVALID
    assert b"window 1" in L.ssym_last_error(eng.ctx)
    assert L.ssym_reconstruct_wsola_spans(*head, 7, 0, pos.ctypes.data, out.ctypes.data, pcm.ctypes.data) == nat.SSYM_E_INVALID
    assert (out == SENTF).all() and (pcm == SENT32).all() and (pos == SENTP).all()
    # NULL window arrays, and the existing call's own refusals with their codes
    assert L.ssym_reconstruct_warped_spans(*head[:3], None, wl.ctypes.data, *head[5:], 0, out.ctypes.data, None) == nat.SSYM_E_INVALID
    ok = np.array([0, 0], dtype=np.uint64)
    assert L.ssym_reconstruct_wsola_spans(*head[:3], ok.ctypes.data, ok.ctypes.data, *head[5:], 513, 0, None, out.ctypes.data,
                                          None) == nat.SSYM_E_INVALID                       # search beyond 512
    bad = np.array([3, 9], dtype=np.uint32)
    assert L.ssym_reconstruct_warped_spans(eng.ctx, stores[0].ptr, bad.ctypes.data, ok.ctypes.data, ok.ctypes.data, *head[5:], 0,
                                           out.ctypes.data, None) == nat.SSYM_E_INVALID    # an index outside the store
    assert (out == SENTF).all()
