"""The linear oracle of live resynthesis (tests/resynth_slices.py) held to the restatement (tests/live_resynth_ref.py) on
the CPU, call for call and bit for bit, and its map generators to what they promise: the hops they hold and the tile rule
of ssym_resynth_push.  tests/test_gpu_resynth_shapes.py trusts the oracle only because this file passes."""
import numpy as np
import pytest

import live_resynth_ref as ref
import resynth_slices as rsl
from live_resynth_ref import GAP, HOP, NO_MATCH
from resynth_gpu import G, tile
from test_gpu_resynth import LANE, SOUND_SAMPLES, TAIL       # the hand-written lanes (importing them needs no GPU)

def sounds(seed=0x7E5):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=n) * 0.3 for n in SOUND_SAMPLES]


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), what


def both(snd, rows, total, search, cuts, cache, what):
    """Every call on a LiveResynth and on a SlicedLane."""
    live, sliced = ref.LiveResynth(snd, search, None, cache), rsl.SlicedLane(snd, rows, total, search, cache)
    at = 0
    for m in cuts:
        same(sliced.push(m), live.push(rows[at:at + m]), (what, "push at", at))
        assert (sliced.n, sliced.released, sliced.held) == (live.n, live.released, live.held), (what, at)
        at += m
    assert at == len(rows)
    same(sliced.flush(), live.flush(total), (what, "flush"))
    assert sliced.ended and sliced.held == 0


def admissible(rows, n_sounds):
    """ssym_resynth_push's checks of one lane's rows, restated: the first row starts a tile; src is a sound or GAP; within a
    tile one sound, steps 0, 1 or 2, never 0 twice in a row; a gap frame starts a tile."""
    src = last = step = None
    for k, (s, f, start) in enumerate(rows):
        if k == 0 and not start:
            return False
        if s != GAP and not 0 <= s < n_sounds:
            return False
        if not 0 <= f <= 0xFFFFFFFF:
            return False
        if start:
            src, last, step = s, f, None
            continue
        d = f - last
        if src == GAP or s != src or d < 0 or d > 2 or (d == 0 and step == 0):
            return False
        last, step = f, d
    return True


@pytest.mark.parametrize("kind", ("one", "all"))
@pytest.mark.parametrize("search", (0, 8, 257))
def test_sliced_lanes_are_the_restatements_on_the_hand_written_lanes(search, kind):
    snd, cache = sounds(), {}
    for l, rows in LANE.items():
        cuts = [1] * len(rows) if kind == "one" else [len(rows)]
        both(snd, rows, len(rows) * HOP + TAIL[l], search, cuts, cache, (l, search, kind))


@pytest.mark.parametrize("search", (0, 8))
def test_sliced_lanes_are_the_restatements_on_random_lanes(search):
    snd, cache = sounds(), {}
    hops = [s.size // HOP for s in snd]
    for seed in range(20):
        rng = np.random.default_rng(0x51CE + seed)
        rows = rsl.random_lane(rng, 30, len(snd), hops, gap_rate=(0.0, 0.2, 0.5)[seed % 3])
        assert len(rows) == 30 and admissible(rows, len(snd))
        total = 30 * HOP + int(rng.integers(0, 1200))
        cuts = []
        while sum(cuts) < 30:
            cuts.append(min(int(rng.integers(0, 7)), 30 - sum(cuts)))          # pushes of no frame among them
        both(snd, rows, total, search, cuts, cache, (seed, search, "random cuts"))
        both(snd, rows, total, search, [1] * 30, cache, (seed, search, "one"))


def test_released_after_is_the_restatements_count():
    snd = sounds()
    for seed in range(8):
        rows = rsl.random_lane(np.random.default_rng(0xAF7 + seed), 40, len(snd), [s.size // HOP for s in snd])
        for search in (0, 8, 256, 257, 512):
            live = ref.LiveResynth(snd, 0, ref.reach(search), {})       # the counts depend on R alone
            after = rsl.released_after(rows, search)
            assert after[0] == 0 and len(after) == len(rows) + 1
            for k, row in enumerate(rows):
                live.push([row])
                assert live.released == after[k + 1], (seed, search, k)


@pytest.mark.parametrize("search", (0, 8, 256, 257, 512))
def test_the_slow_map_holds_2R_hops_and_the_fast_map_half_of_R(search):
    R = ref.reach(search)
    for phase in (0, 1):
        rows = rsl.slow_map(40, 3, phase)
        steps = np.diff([r[1] for r in rows]).tolist()
        assert steps[:4] == ([1, 0, 1, 0] if phase == 0 else [0, 1, 0, 1]) and set(steps) == {0, 1}
        after = rsl.released_after(rows, search)
        held = [k - after[k] for k in range(len(rows) + 1)]
        assert max(held) == 2 * R and held[-1] >= 2 * R - 1
    rows = rsl.fast_map(40, 3)
    assert set(np.diff([r[1] for r in rows]).tolist()) == {2}
    after = rsl.released_after(rows, search)
    held = [k - after[k] for k in range(len(rows) + 1)]
    assert max(held) == (R + 1) // 2 == held[-1]


def test_every_generated_row_passes_the_tile_rule_of_push():
    for n in (1, 2, 3, 40):
        for phase in (0, 1):
            assert admissible(rsl.slow_map(n, 7, phase, src=1), 2) and len(rsl.slow_map(n, 7, phase)) == n
        assert admissible(rsl.fast_map(n, 0, src=1), 2) and len(rsl.fast_map(n, 0)) == n
    assert not admissible(tile(0, [4, 4, 4]), 1) and not admissible(tile(0, [4, 7]), 1) and not admissible(tile(0, [4, 3]), 1)
    assert not admissible(tile(1, [4]), 1) and not admissible([(0, 4, 0)], 1) and not admissible([G, (GAP, NO_MATCH, 0)], 1)
    past = gaps = 0
    for seed in range(40):
        rng = np.random.default_rng(0x6E4 + seed)
        hops = [40, 43, 20, 0]
        rows = rsl.random_lane(rng, 60, 4, hops, gap_rate=0.25)
        assert len(rows) == 60 and admissible(rows, 4), seed
        assert max(b - a for a, b in ref.tiles(rows)) <= 24
        past += any(s != GAP and f > hops[s] for s, f, _ in rows)
        gaps += any(s == GAP for s, _, _ in rows)
    assert past >= 20 and gaps >= 20                 # what the generator is for does occur


def test_frames_at_the_32_bit_end_render_silence():
    """A tile at frames 2^32 - 6 ... 2^32 - 1: its window is empty, its output zeros, and the counts are the rule's."""
    snd = sounds()
    top = 1 << 32
    rows = tile(0, [top - 6, top - 5, top - 3, top - 2, top - 1])
    assert admissible(rows, len(snd))
    for search in (0, 8):
        both(snd, rows, 5 * HOP + 300, search, [1] * 5, {}, ("32-bit end", search))
        lane = rsl.SlicedLane(snd, rows, 5 * HOP + 300, search)
        assert not lane.whole.any()
        assert rsl.released_after(rows, search) == ([0, 0, 0, 2, 2, 3] if search == 0 else [0, 0, 0, 0, 0, 1])
