"""ssym_resynth_* at the edges of its mapping (soundsym_amd/csrc/resynth.hip), against the linear oracle
(tests/resynth_slices.py, held to the restatement by tests/test_resynth_slices.py): every call bit for bit on samples and
pcm, with its count, the lane offsets and counts(); every lane's concatenation from reset to flush against `offline`.

The other resynthesis tests run one hand-written world of 1 or 4 lanes chosen for the definition.  The edges here belong to
the mapping, each named with the statement of resynth.hip it walks:

    lane counts      resynth_feed_kernel: `l = blockIdx.x * blockDim.x + threadIdx.x` in 64-thread blocks, `if (l >= a.nLanes)`;
                     resynth_search_kernel: `l = blockIdx.x`; resynth_synth_kernel: `l = blockIdx.y`.  1, 63, 64, 65 and 130
                     lanes; kResynthMaxLanes = 65535, the synthesis grid's y, with frames on its first and last lanes.
    growth           resynth_run: `if (hopNeed > rs->hopCap)` frees the hop list and allocates pow2_at_least(max(hopNeed, 256));
                     LaneLog::room (lane_feed.hpp) does the same for the samples.  A small call, one of more than 5000
                     entries, a small one again with the big list full, a big one again.
    stale entries    a lane's stretch of the list is `room + (kWarpTaps - 1)` entries, the feed kernel writes `cnt + 3` of them;
                     what lies behind is an earlier call's, with tile ids (column numbers) equal across lanes.  The synthesis
                     kernel's `for (u ...; h0 + u < count; ...)` keeps them out: hop u takes entries u ... u + 3, so no hop
                     below count reads entry count + 3 or beyond (the fill guard `h0 + tid < count + (kWarpTaps - 1)` only
                     keeps the loads inside the stretch).
    group edges      resynth_synth_kernel: `h0 = blockIdx.x * kResynthHops`, `if (h0 >= count) return`, the grid's x sized by
                     the largest lane: 0, 1, 15, 16, 17, 32 and 33 hops in one call; `if (k >= samples) continue` and the feed
                     kernel's `(s.tail + kWarpHop - 1) / kWarpHop` tail hops: tails of 16 and 17 hops and 16 hops +- 1 sample.
    the full ring    kResynthRing = 16 slots, `ring[st.n % kResynthRing] = ...` with 2 R unreleased frames and three of
                     history; the search kernel's `if (r + (kWarpTaps - 1) >= hops) ring[col % kResynthRing].pos = pos` and
                     the feed kernel's history `ring[col % kResynthRing]` carry the WSOLA chain through calls of 0, 1, 2 hops.
    the clip         the feed kernel's `end = min((st.last + 1) * kWarpHop, nSrc)`: an open tile whose hops leave by the reach
                     rule while the clip is active, n_src no multiple of HOP, wsola_step's `hi` and template reads under it.
    32-bit ends      `(uint64_t)ring[...].map + a.reach <= st.last`, `(uint64_t)st.first * kWarpHop`, `e.map - st.first`: a tile
                     at frames 2^32 - 6 ... 2^32 - 1.  Flushes that release nothing, pushes of no frame.

The store: sounds of 40 * HOP + 40, 43 * HOP + 201, 20 * HOP + 40 samples and of one sample."""
import numpy as np
import pytest

import resynth_slices as rsl
from live_resynth_ref import HOP, reach
from resynth_gpu import G, SlicedLive
from soundsym_amd import Engine, SsymError

pytestmark = pytest.mark.gpu

SOUND_SAMPLES = (40 * HOP + 40, 43 * HOP + 201, 20 * HOP + 40, 1)
SHORT = 2                                            # the sound of 20 hops and 40 samples
HOPS = [n // HOP for n in SOUND_SAMPLES]
CACHE = {s: {} for s in (0, 8, 256, 257, 512)}       # tiles rendered, shared by the tests of this module


class _Rig:
    def __init__(self):
        rng = np.random.default_rng(0x5EA9E5)
        self.sounds = [rng.normal(size=n) * 0.3 for n in SOUND_SAMPLES]
        self.e = Engine(metric="dtw", dtype="f64", device=0)
        off = np.concatenate([[0], np.cumsum(SOUND_SAMPLES)]).astype(np.uint64)
        self.store = self.e.samples(np.concatenate(self.sounds), off)

    def live(self, n_lanes, search, lanes):
        return SlicedLive(self.e, self.store, self.sounds, n_lanes, search, lanes, CACHE[search])

    def close(self):
        self.store.close()
        self.e.close()


@pytest.fixture(scope="module")
def rig():
    r = _Rig()
    yield r
    r.close()


def lane_of(rng, n_frames, gap_rate=0.2):
    return rsl.random_lane(rng, n_frames, len(SOUND_SAMPLES), HOPS, gap_rate)


def with_tail(rows, tail):
    return rows, len(rows) * HOP + tail


# ---- 1, 2: lanes -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("search", (0, 8))
@pytest.mark.parametrize("n_lanes", (1, 63, 64, 65, 130))
def test_lane_counts_around_the_feed_kernels_block(rig, n_lanes, search):
    """A different lane of 20 frames on every lane but those = 2 (mod 5); three pushes cut at lane-dependent columns, with
    lanes absent from the first and the second; the flushes in descending order, lanes without frames to zeros."""
    rng = np.random.default_rng(0x1A7E + n_lanes)
    lanes = {l: with_tail(lane_of(rng, 20), (l * 37) % 300) for l in range(n_lanes) if l % 5 != 2}
    live = rig.live(n_lanes, search, lanes)
    try:
        first = {l: (l * 3) % 8 for l in lanes if l % 4 != 1}                   # lanes 0, 8, ... take no frame
        second = {l: (l * 5) % 9 for l in lanes if l % 4 != 3}
        live.push(first, "first push")
        live.push(second, "second push")
        live.push({l: 20 - live.refs[l].n for l in lanes}, "third push")
        for l in range(n_lanes - 1, -1, -1):
            n = live.flush(l, None if l in lanes else 300 + l)
            if l not in lanes:
                assert n == 300 + l and not live.refs[l].whole.any()
    finally:
        live.close()


@pytest.mark.parametrize("search", (0, 8))
def test_the_lane_limit(rig, search):
    """65535 lanes, frames on the first and last lanes of the feed kernel's first, second and last blocks and in the
    middle.  (That 65536 are refused: tests/test_gpu_resynth_refusal.py.)"""
    n_lanes = 65535
    rng = np.random.default_rng(0x11317)
    lanes = {l: with_tail(lane_of(rng, 20), 100 + l % 7) for l in (0, 63, 64, 32767, 65534)}
    live = rig.live(n_lanes, search, lanes)
    try:
        live.push({l: 7 + l % 5 for l in lanes}, "first push")
        live.push({l: 20 - live.refs[l].n for l in lanes}, "second push")
        for l in (65534, 0, 40000, 64, 63, 32767):
            live.flush(l, None if l in lanes else 700)
    finally:
        live.close()


# ---- 3: growth ---------------------------------------------------------------------------------------------------------

def test_the_hop_list_and_the_sample_log_grow_and_are_reused(rig):
    n_lanes, small, other = 130, 7, 100
    rng = np.random.default_rng(0x6407)
    frames = {l: 70 + (5 if l == small else 0) + (1 if l in (small, other) else 0) for l in range(n_lanes)}
    lanes = {l: with_tail(lane_of(rng, frames[l]), (l % 3) * 100) for l in range(n_lanes)}
    live = rig.live(n_lanes, 0, lanes)

    def need():                                      # hopNeed of the last call: room + 3 per lane of the call
        return sum(room + 3 for room, _ in live.calls[-1].values())
    try:
        live.push({small: 5}, "call 1")
        assert need() <= 256                         # the list's first size
        live.push({l: 40 for l in lanes}, "call 2")
        assert need() > 5000                         # it grows: 8192 entries
        live.push({small: 1, other: 1}, "call 3")
        assert need() <= 256                         # small again, in the big list full of call 2's entries
        live.push({l: 30 for l in lanes}, "call 4")
        assert 256 < need() <= 8192
        assert all(live.refs[l].n == frames[l] for l in lanes)
        for l in range(n_lanes):
            live.flush(l)
    finally:
        live.close()


# ---- 4: stale entries --------------------------------------------------------------------------------------------------

STALE_STARTS = (0, 7, 20, 21, 37, 48)                # every lane's tiles start at these columns (48: the end)


def stale_lane(l):
    """Lane l: slow maps on even lanes, fast maps on odd ones, another sound and another first frame than its neighbours."""
    rows = []
    for t, (a, b) in enumerate(zip(STALE_STARTS[:-1], STALE_STARTS[1:])):
        src = (l + t) % len(SOUND_SAMPLES)
        rows += rsl.slow_map(b - a, l + 2 * t, (l // 2 + t) % 2, src) if l % 2 == 0 else rsl.fast_map(b - a, (l + 3 * t) % 9, src)
    return rows


def stale_schedule(kind):
    """Per call {lane: frames}, 48 frames on each of 8 lanes in the end."""
    left, calls, c = {l: 48 for l in range(8)}, [], 0
    while any(left.values()):
        if kind == "growing":                        # every lane 1, 2, 3, 4, 5, 1, ... frames
            take = {l: min(1 + c % 5, left[l]) for l in left}
        else:                                        # "rotating": another subset of the lanes in each call: the stretches shift
            take = {l: min(1 + (l + c) % 4, left[l]) for l in left if (l + c) % 3}
        take = {l: k for l, k in take.items() if k}
        for l, k in take.items():
            left[l] -= k
        calls.append(take)
        c += 1
    return calls


@pytest.mark.parametrize("kind", ("growing", "rotating"))
@pytest.mark.parametrize("search", (0, 8))
def test_stale_entries_of_the_reused_hop_list_are_no_taps(rig, search, kind):
    lanes = {l: with_tail(stale_lane(l), 100 * l) for l in range(8)}
    assert all([j for j, r in enumerate(rows) if r[2]] == list(STALE_STARTS[:-1]) for rows, _ in lanes.values())
    calls = stale_schedule(kind)
    # the inputs do what they are for: some lane leaves at least 4 entries of its stretch unwritten in at least three calls
    at, slack = {l: 0 for l in lanes}, {l: 0 for l in lanes}
    for take in calls:
        for l, k in take.items():
            after = rsl.released_after(lanes[l][0], search)
            room, count = (at[l] - after[at[l]]) + k, after[at[l] + k] - after[at[l]]
            slack[l] += room - count >= 4
            at[l] += k
    assert max(slack.values()) >= 3, slack
    live = rig.live(8, search, lanes)
    try:
        for c, take in enumerate(calls):
            live.push(take, "%s, call %d" % (kind, c))
        assert max(sum(room - hops >= 4 for room, hops in (call[l] for call in live.calls if l in call)) for l in lanes) >= 3
        for l in (3, 0, 7, 4, 1, 6, 2, 5):
            live.flush(l)
    finally:
        live.close()


# ---- 5: group edges ----------------------------------------------------------------------------------------------------

GROUP_HOPS = (0, 1, 15, 16, 17, 32, 33)
GROUP_TAILS = (16 * HOP, 17 * HOP, 16 * HOP - 1, 16 * HOP + 1, 0, 1, 255)


def group_lane(hops, search, l):
    """(rows, frames of the first call): the second call takes the rest and releases exactly `hops` hops.  The first call's
    frames open a fast tile and are all held; the second brings whole fast tiles, each closed by the next start, and a last
    start whose frame stays held.  0 hops: a frame of step 0 on an open tile, which releases nothing."""
    if hops == 0:
        return rsl.slow_map(2, 5, 1, 0), 1
    p = min(hops, (reach(search) + 1) // 2)          # a fast tile holds ceil(R / 2) frames
    sizes, left = [], hops - p
    while left:
        sizes.append(min(left, (12, 7, 9)[len(sizes) % 3]))
        left -= sizes[-1]
    rows = rsl.fast_map(p, l, l % 2)
    for t, n in enumerate(sizes):
        rows += rsl.fast_map(n, (3 * l + 5 * t) % 16, (l + t) % 3)
    return rows + rsl.fast_map(1, 9 + l, (l + 1) % 2), p


@pytest.mark.parametrize("search", (0, 8))
def test_synthesis_group_edges_in_one_call_and_tails_around_16_hops(rig, search):
    built = [group_lane(h, search, l) for l, h in enumerate(GROUP_HOPS)]
    lanes = {l: with_tail(rows, GROUP_TAILS[l]) for l, (rows, _) in enumerate(built)}
    for l, (rows, p) in enumerate(built):            # the inputs do what they are for
        after = rsl.released_after(rows, search)
        assert after[p] == 0 and after[len(rows)] - after[p] == GROUP_HOPS[l], (l, after)
        assert len(rows) - after[len(rows)] >= 1     # a held remainder: the flush has a hop and the tail
    live = rig.live(len(lanes), search, lanes)
    try:
        assert live.push({l: p for l, (_, p) in enumerate(built)}, "first call") == 0
        n = live.push({l: len(rows) - p for l, (rows, p) in enumerate(built)}, "the call of the group edges")
        assert n == sum(GROUP_HOPS) * HOP and [live.calls[-1][l][1] for l in lanes] == list(GROUP_HOPS)
        for l in lanes:
            held = live.held(l)
            assert held == (2 if GROUP_HOPS[l] == 0 else 1) and live.flush(l) == held * HOP + GROUP_TAILS[l]
    finally:
        live.close()


# ---- 6: the full ring --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("search", (0, 8, 256, 257, 512))
def test_the_ring_at_its_fullest_through_several_wraps(rig, search):
    """The slowest admissible map, 40 frames, one frame per call: 2 R frames held (4, 10, 10, 12, 12) after every frame of
    step 0 and 2 R - 1 after every frame of step 1, which releases two -- no map pushed frame by frame holds 2 R after
    every call, since a frame that releases nothing is followed by one that must.  So the condition on the inputs is: at
    least 28 consecutive calls (the ring wraps at 16) with 2 R - 1 or 2 R frames held, 2 R after at least 14 of them."""
    R = reach(search)
    released = set()
    for phase in (0, 1):
        rows = rsl.slow_map(40, 2 + phase, phase, phase)
        after = rsl.released_after(rows, search)
        held = [k - after[k] for k in range(1, 41)]
        full = [h >= 2 * R - 1 for h in held]
        assert max(held) == 2 * R and all(full[12:]) and sum(h == 2 * R for h in held[12:]) >= 14, held
        released |= {after[k + 1] - after[k] for k in range(40)}
        for step in (1, 3, 13):
            live = rig.live(1, search, {0: with_tail(rows, 300)})
            try:
                for a in range(0, 40, step):
                    live.push({0: min(step, 40 - a)}, "phase %d, frames from %d" % (phase, a))
                    assert live.held(0) <= 2 * R
                live.flush(0)
            finally:
                live.close()
    assert released == {0, 1, 2}                     # calls of 0, 1 and 2 hops all occur


# ---- 7: the clip -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", (0, 1, 2))
@pytest.mark.parametrize("search", (0, 8, 257, 512))
def test_an_open_tile_runs_out_of_its_recording(rig, search, seed):
    """One tile on the sound of 20 * HOP + 40 samples, from frame 12 to beyond frame 30 in random admissible steps, never
    closed before the flush; a tail of 300."""
    rng = np.random.default_rng(0xC11B + seed)
    fmap = 12 + np.concatenate([[0], np.cumsum(rsl.paced_steps(rng, 60))])
    fmap = fmap[:int(np.argmax(fmap > 33)) + 1].tolist()             # to the first frame beyond 33
    rows = [(SHORT, f, int(j == 0)) for j, f in enumerate(fmap)]
    assert fmap[0] == 12 and fmap[-1] > 33 and len(fmap) <= 40
    after = rsl.released_after(rows, search)
    n_src = SOUND_SAMPLES[SHORT]
    # some hop leaves by the reach rule, not at the flush, while the window's end is clipped
    assert any(after[k + 1] > after[k] and (fmap[k] + 1) * HOP > n_src for k in range(len(rows)))
    assert n_src % HOP and after[len(rows)] < len(rows)
    live = rig.live(1, search, {0: with_tail(rows, 300)})
    try:
        for k in range(len(rows)):
            live.push({0: 1}, "frame %d" % k)
        live.flush(0)
    finally:
        live.close()


# ---- 8: 32-bit ends and calls that release nothing ---------------------------------------------------------------------

@pytest.mark.parametrize("search", (0, 8))
def test_a_tile_at_the_32_bit_end_of_frame(rig, search):
    top = 1 << 32
    rows = [(0, f, int(j == 0)) for j, f in enumerate((top - 6, top - 5, top - 3, top - 2, top - 1))]
    after = rsl.released_after(rows, search)
    assert after == ([0, 0, 0, 2, 2, 3] if search == 0 else [0, 0, 0, 0, 0, 1])       # map[j] + R <= L in 64 bits
    for cuts in ([1] * 5, [5], [2, 3]):
        live = rig.live(2, search, {1: with_tail(rows, 300)})
        try:
            for m in cuts:
                live.push({1: m}, "cuts %r" % cuts)
            assert live.flush(1) == (5 - after[5]) * HOP + 300 and not live.refs[1].whole.any()
        finally:
            live.close()


@pytest.mark.parametrize("search", (0, 8))
def test_calls_that_release_nothing(rig, search):
    rng = np.random.default_rng(0xE0)
    big = lane_of(rng, 60, 0.1)
    lanes = {0: ([G, G, G], 3 * HOP), 1: with_tail(big, 0), 3: ([], 0), 4: with_tail(rsl.fast_map(3, 4, 1) + [G], 0)}
    live = rig.live(5, search, lanes)
    try:
        assert live.push({}, "no frame, before any other call") == 0
        assert live.flush(3) == 0                                # a fresh lane ends with no sample at all
        with pytest.raises(SsymError, match="has ended"):
            live.rs.push([3], [0], [0], [0], [1])
        assert live.push({0: 3, 4: 4}, "gap frames only; a tile closed by a gap frame") == 7 * HOP
        assert live.held(0) == 0 and live.held(4) == 0
        assert live.flush(0) == 0 and live.flush(4) == 0         # every frame left before, tail 0
        live.push({1: 60}, "a large call")
        assert live.push({}, "no frame, after a large call") == 0
        assert live.push({1: 0}, "no frame again") == 0
        live.flush(1)
        assert live.flush(2, 0) == 0                             # ... and a lane never touched
    finally:
        live.close()


# ---- 9: random, end to end ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("search", (0, 8))
def test_random_lanes_schedules_a_reset_and_tails(rig, search, seed):
    rng = np.random.default_rng(0x9A4D + 16 * seed + search)
    n_lanes, n_calls, mid = 5, 12, 6

    def cuts(n, calls):                              # the frames of `calls` pushes that sum to n, zeros among them
        at = np.sort(rng.integers(0, n + 1, size=calls - 1))
        return np.diff(np.concatenate([[0], at, [n]])).tolist()

    def lane():
        return with_tail(lane_of(rng, 60, float(rng.uniform(0.0, 0.4))), int(rng.integers(0, 5 * HOP + 1)))

    lanes = {l: lane() for l in range(n_lanes)}
    plan = {l: cuts(60, n_calls) for l in lanes}
    victim = int(rng.integers(0, n_lanes))
    live = rig.live(n_lanes, search, lanes)
    try:
        for c in range(n_calls):
            if c == mid:
                live.reset(victim, *lane())
                plan[victim] = [0] * mid + cuts(60, n_calls - mid)
            live.push({l: plan[l][c] for l in lanes}, "call %d" % c)
        for l in rng.permutation(n_lanes).tolist():
            live.flush(l)
    finally:
        live.close()
