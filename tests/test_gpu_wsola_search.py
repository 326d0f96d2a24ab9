"""Which lag wins in wsola_search_kernel, and odd samples through both resynthesis kernels.  The planted cases of
tests/wsola_cases.py put the winner -- alone, or tied with one or two others -- on every edge of the kernel's division
of the lags among threads, rounds and waves, and on the edges of the admissible range; their answer is known by
construction and test_wsola_ref.py holds it to the restatement, so the GPU is held to both, positions exactly and
samples bit for bit.  The width sweep runs test_gpu_wsola's ragged case at the widths next to which a wave gains or
loses a round.  The odd samples (NaN, +-inf, -0.0, subnormals, squares that underflow or overflow) go through WSOLA and
the plain warp: positions exactly, the NaN mask exactly, the bits wherever the restatement's sample is a number."""
import time

import numpy as np
import pytest

import warp_ref
import wsola_cases as wc
import wsola_ref as ref
from soundsym_amd import Engine
from soundsym_amd import _native as nat
from test_gpu_wsola import ALL_PATHS, _bits, _case, _check, _raw, _store

pytestmark = pytest.mark.gpu

HOST_AND_DEVICE = (ALL_PATHS[0], ALL_PATHS[3])         # host arrays; device map and outputs: the search writes out_pos itself


def _hold(cases, S):
    """All cases as the targets of one call, through both paths: the restatement's positions and bits (_check), and
    the positions the cases were built to have."""
    call, planted = wc.pack(cases)
    e = Engine(metric="dtw", dtype="f64")
    smp = _store(e, call[0])
    t0 = time.perf_counter()
    out, pcm, pos = _check(e, smp, call, S, HOST_AND_DEVICE)
    print("S %d: %d cases, %.2f s with the restatement" % (S, len(cases), time.perf_counter() - t0))
    wrong = np.flatnonzero(pos != planted)
    assert wrong.size == 0, [(cases[int(np.searchsorted(call[4], i, side="right")) - 1].name, int(pos[i]), int(planted[i]))
                             for i in wrong[:5]]
    e.close()


@pytest.mark.parametrize("S", wc.PLANT_WIDTHS)
def test_planted_winners_and_ties(S):
    _hold(wc.plant_cases(S), S)


@pytest.mark.parametrize("S", wc.EDGE_WIDTHS)
def test_edges_of_the_admissible_range_and_flat_sources(S):
    _hold(wc.edge_cases(S) + wc.flat_cases(S), S)


@pytest.mark.parametrize("S", [2, 31, 32, 33, 63, 95, 96, 127, 128, 159, 160, 255, 383, 384, 447, 448, 511])
def test_ordinary_data_at_the_widths_where_a_wave_gains_a_round(S):
    rng = np.random.default_rng(0x51DE + S)
    case = _case(rng, 5)
    e = Engine(metric="dtw", dtype="f64")
    smp = _store(e, case[0])
    _check(e, smp, case, S, HOST_AND_DEVICE)
    e.close()


def _same_outside_nan(got, want, what):
    """The NaN mask equal, the bits equal wherever the restatement's sample is a number (the definition does not fix a
    generated NaN's sign or payload)."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    bad = np.flatnonzero(~nan & (_bits(got) != _bits(want)))
    print("%s: %d samples, %d NaN, %d differ" % (what, want.size, int(nan.sum()), bad.size))
    assert bad.size == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("S", wc.ODD_WIDTHS)
def test_odd_samples_through_wsola(S):
    sounds, idx, off, maps, m_off, frames, _ = wc.odd_call()
    want, want_pos = wc.odd_reference(S)
    assert not (want_pos == ref.UNSET).any()
    e = Engine(metric="dtw", dtype="f64")
    smp = _store(e, sounds)
    for kw in HOST_AND_DEVICE:
        rc, out, pcm, pos = _raw(e, smp, idx, off, maps, m_off, frames, None, S, **kw)
        assert rc == nat.SSYM_OK, (kw, nat.lib().ssym_last_error(e.ctx))
        wrong = np.flatnonzero(pos != want_pos)
        assert wrong.size == 0, (kw, wrong[:5], pos[wrong[:5]], want_pos[wrong[:5]])
        _same_outside_nan(out, want, "S %d %s" % (S, kw))
        assert np.array_equal(pcm, ref.pcm32(out)), kw
    e.close()


def test_odd_samples_through_the_plain_warp():
    import torch
    sounds, idx, off, maps, m_off, frames, _ = wc.odd_call()
    want = wc.odd_reference(None)
    e = Engine(metric="dtw", dtype="f64")
    smp = _store(e, sounds)
    out, pcm = e.reconstruct_warped(smp, idx, off, maps, m_off, frames, want_pcm32=True)
    _same_outside_nan(out, want, "plain warp, host map")
    assert np.array_equal(pcm, warp_ref.pcm32(out))
    dmaps = torch.from_numpy(maps.view(np.int32)).cuda()
    _same_outside_nan(e.reconstruct_warped(smp, idx, off, dmaps, m_off, frames), want, "plain warp, device map")
    e.close()
