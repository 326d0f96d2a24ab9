"""The restatement of live resynthesis (tests/live_resynth_ref.py) held to the offline per-tile render on the CPU: cut
invariance, the release rule's tightness for search = 0, and the bound on the hops held back."""
import itertools

import numpy as np
import pytest

import live_resynth_ref as ref
from live_resynth_ref import GAP, HOP, NO_MATCH

SEARCHES = (0, 8, 300)


def _sounds(seed=0x5A17):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n) for n in (5000, 2600, 1)]


def _paced(rng, first, frames):
    """A map from `first` in steps of 0, 1 or 2, never 0 twice in a row."""
    out, prev = [first], 1
    for _ in range(frames - 1):
        step = int(rng.integers(0 if prev else 1, 3))
        out.append(out[-1] + step)
        prev = step
    return out


def _sequence(rng, sounds, n_tiles, max_tile=12, gaps="some"):
    """(src, frame, start) rows: tiles of 1 ... max_tile frames, gaps first, last and in runs, first > 0, and recordings
    that end inside the reach (a tile may start within a few hops of its recording's end, or beyond it)."""
    rows = []

    def gap_run(n):
        rows.extend((GAP, NO_MATCH, 1) for _ in range(n))

    if gaps == "some":
        gap_run(int(rng.integers(1, 3)))
    for t in range(n_tiles):
        src = int(rng.integers(0, len(sounds)))
        hops = len(sounds[src]) // HOP
        first = int(rng.integers(0, hops + 3)) if rng.random() < 0.6 else max(0, hops - int(rng.integers(0, 6)))
        fmap = _paced(rng, first, int(rng.integers(1, max_tile + 1)))
        rows.extend((src, f, int(j == 0)) for j, f in enumerate(fmap))
        if gaps == "some" and rng.random() < 0.4:
            gap_run(int(rng.integers(1, 4)))
    if gaps == "some":
        gap_run(2)
    return rows


def _run(sounds, rows, cuts, total, search, cache, reach=None):
    """The pushes' outputs and the hops held after each; cuts: the sizes of the pushes."""
    live = ref.LiveResynth(sounds, search, reach, cache)
    parts, held, at = [], [], 0
    for m in cuts:
        parts.append(live.push(rows[at:at + m]))
        held.append(live.held)
        at += m
    assert at == len(rows)
    parts.append(live.flush(total))
    return parts, held


def _compositions(n):
    for mask in range(1 << (n - 1)):
        cuts, run = [], 1
        for k in range(n - 1):
            if mask >> k & 1:
                cuts.append(run)
                run = 1
            else:
                run += 1
        yield cuts + [run]


@pytest.mark.parametrize("search", SEARCHES)
def test_every_cut_of_a_short_sequence_gives_the_offline_render(search):
    sounds, rng, cache = _sounds(), np.random.default_rng(0xC07 + search), {}
    for trial in range(4):
        rows = _sequence(rng, sounds, 3, max_tile=4, gaps="some" if trial % 2 else "none")[:10]
        rows[0] = (rows[0][0], rows[0][1], 1)
        total = len(rows) * HOP + (0, 300, 768, 1023)[trial]
        want = ref.offline(sounds, rows, total, search, cache)
        # frame by frame: what each consumed frame releases
        one, _ = _run(sounds, rows, [1] * len(rows), total, search, cache)
        counts = np.cumsum([p.size for p in one[:-1]])
        for cuts in _compositions(len(rows)):
            parts, _ = _run(sounds, rows, cuts, total, search, cache)
            got = np.concatenate(parts)
            assert got.size == total and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (trial, cuts)
            ends = np.cumsum(cuts) - 1                      # the same released counts as frame by frame
            assert np.array_equal(np.cumsum([p.size for p in parts[:-1]]), counts[ends]), (trial, cuts)


@pytest.mark.parametrize("search", SEARCHES)
def test_random_cuts_of_long_sequences_give_the_offline_render(search):
    sounds, rng, cache = _sounds(), np.random.default_rng(0xA11 + search), {}
    R = ref.reach(search)
    for trial in range(3):
        rows = _sequence(rng, sounds, 5, max_tile=12)
        total = len(rows) * HOP + int(rng.integers(0, 1200))
        want = ref.offline(sounds, rows, total, search, cache)
        one, held_one = _run(sounds, rows, [1] * len(rows), total, search, cache)
        assert max(held_one) <= 2 * R                       # the hold bound
        counts = np.cumsum([p.size for p in one[:-1]])
        for _ in range(4):
            cuts = []
            while sum(cuts) < len(rows):
                cuts.append(min(int(rng.integers(1, 9)), len(rows) - sum(cuts)))
            parts, held = _run(sounds, rows, cuts, total, search, cache)
            got = np.concatenate(parts)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (trial, cuts)
            assert np.array_equal(np.cumsum([p.size for p in parts[:-1]]), counts[np.cumsum(cuts) - 1])
            assert max(held) <= 2 * R


def test_a_diagonal_map_holds_R_hops_and_no_map_more_than_2R():
    sounds = [np.random.default_rng(3).standard_normal(40 * HOP)]
    for search in (0, 8, 256, 257, 512):
        R = ref.reach(search)
        assert R == {0: 2, 8: 5, 256: 5, 257: 6, 512: 6}[search]
        live = ref.LiveResynth(sounds, 0, R, {})             # (the counts depend on R alone; the plain warp renders fast)
        for j in range(30):
            live.push([(0, j, int(j == 0))])
            assert live.held == min(j + 1, R)
        slow = ref.LiveResynth(sounds, 0, R, {})
        fmap = [j // 2 for j in range(1, 40)]                # steps 1, 0, 1, 0, ...: the slowest paced map
        for j, f in enumerate(fmap):
            slow.push([(0, f, int(j == 0))])
            assert slow.held <= 2 * R
        assert slow.held == 2 * R


def test_the_plain_warp_reach_is_tight():
    """search = 0: R - 1 = 1 releases a hop whose bits a later frame changes.  Steps 0, 1, 0 up to hop 3: its tap at frame 0
    reads source hop map[0] + 3 = map[3] + 2, which the window (map[3] + 1 + 1) * HOP of R = 1 ends before."""
    sounds = [np.random.default_rng(9).standard_normal(20 * HOP)]
    rows = [(0, f, int(j == 0)) for j, f in enumerate([5, 5, 6, 6, 7, 8, 9, 10])]
    total = len(rows) * HOP
    want = ref.offline(sounds, rows, total, 0)
    good, _ = _run(sounds, rows, [1] * len(rows), total, 0, None)
    assert np.array_equal(np.concatenate(good).view(np.uint64), want.view(np.uint64))
    early, _ = _run(sounds, rows, [1] * len(rows), total, 0, None, reach=1)
    got = np.concatenate(early)
    assert got.size == total
    differ = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64)) // HOP
    assert differ.size and set(differ.tolist()) == {3}


def test_gaps_lanes_without_frames_and_the_flush():
    sounds, cache = _sounds(), {}
    live = ref.LiveResynth(sounds)
    assert live.flush(700).tolist() == [0.0] * 700           # a lane without frames: N zeros
    live = ref.LiveResynth(sounds, 8)
    out = live.push([(GAP, NO_MATCH, 1), (GAP, NO_MATCH, 1)])
    assert out.size == 2 * HOP and not out.any() and live.held == 0      # gap frames leave at once
    out = live.push([(0, 2, 1), (0, 3, 0)])
    assert out.size == 0 and live.held == 2
    out = live.push([(GAP, NO_MATCH, 1)])                    # a start closes the tile before it
    assert out.size == 3 * HOP and live.held == 0
    tail = live.flush(5 * HOP + 300)
    assert tail.size == 300 and not tail.any()               # behind a gap: silence
    with pytest.raises(AssertionError):
        live.push([(0, 0, 1)])
    with pytest.raises(AssertionError):
        ref.LiveResynth(sounds).flush(-1)
    rows = [(1, 9, 1), (1, 10, 0), (1, 12, 0)]               # a recording of 2600 samples: 10 hops and a bit
    want = ref.offline(sounds, rows, 3 * HOP + 1023, 0, cache)
    parts, _ = _run(sounds, rows, [2, 1], 3 * HOP + 1023, 0, cache)
    assert np.array_equal(np.concatenate(parts).view(np.uint64), want.view(np.uint64))
    assert want[1:2600 - 9 * HOP].all() and not want[2600 - 9 * HOP:].any()    # the window holds 296 samples; w[0] = 0
