"""A linear oracle for live resynthesis and the maps that drive it to its edges -- TEST INFRASTRUCTURE, no GPU.

tests/live_resynth_ref.py's LiveResynth renders the open tile again from its first frame at every release: quadratic in the
tile's length, minutes for a long tile under a wide search.  tests/test_live_resynth_ref.py holds it to the theorem that
makes a linear oracle legitimate: from reset to flush the live output is `offline`'s, bit for bit.  So what a call returns
for a lane is a slice of `offline`, and the slice's ends follow from the release rule alone, which needs no samples.
tests/test_resynth_slices.py holds this file to LiveResynth call for call before any GPU test relies on it.

    released_after   the counts-only walk of the release rule: hops that have left after each prefix of a lane's frames
    SlicedLane       one lane whose frames and length are known beforehand: `offline` once, push(k) / flush() slice it
    slow_map         steps 1, 0, 1, 0 ... (phase 0) or 0, 1, 0, 1 ... (phase 1): the slowest admissible map, 2 R hops held
    fast_map         all steps 2: the fastest, ceil(R / 2) hops held
    random_lane      tiles of 1 ... 24 frames with random admissible steps, gap runs, tiles that run past their recording

The generators return (src, frame, start) rows as ssym_resynth_push takes them; every map of a generator is one tile."""
import numpy as np

from live_resynth_ref import GAP, HOP, NO_MATCH, offline, reach


def released_after(frames, search):
    """out[k]: the hops that have left once the first k rows of `frames` are consumed, k = 0 ... len(frames).  A hop
    leaves when its tile is closed by a start, at once as a gap frame, or when map[j] + R <= L."""
    R = reach(search)
    out, rel, src, maps = [0], 0, GAP, []
    for n, (s, f, start) in enumerate(frames):
        if start or n == 0:
            rel, src = n, int(s)                     # the tile before is closed; rel is the open tile's first column
        maps.append(int(f))
        if src == GAP:
            rel = n + 1
        else:
            while rel <= n and maps[rel] + R <= maps[n]:
                rel += 1
        out.append(rel)
    return out


class SlicedLane:
    """One lane that will consume `frames` and end with total_samples samples.  n, released, held and ended read as
    LiveResynth's."""

    def __init__(self, sounds, frames, total_samples, search=0, cache=None):
        self.frames, self.total = list(frames), int(total_samples)
        assert self.total >= len(self.frames) * HOP
        self.whole = offline(sounds, self.frames, self.total, search, cache)
        self.after = released_after(self.frames, search)
        self.n, self.released, self.ended = 0, 0, False

    @property
    def held(self):
        return self.n - self.released

    def rows(self, k):
        """The next k rows, not consumed."""
        assert self.n + k <= len(self.frames)
        return self.frames[self.n:self.n + k]

    def push(self, k):
        """Consume the next k rows; the samples this releases."""
        assert not self.ended and 0 <= k and self.n + k <= len(self.frames)
        self.n += k
        a, self.released = self.released, self.after[self.n]
        return self.whole[a * HOP:self.released * HOP]

    def flush(self):
        assert not self.ended and self.n == len(self.frames)
        self.ended = True
        a, self.released = self.released, self.n
        return self.whole[a * HOP:]


def _tile(src, fmap):
    return [(int(src), int(f), int(j == 0)) for j, f in enumerate(fmap)]


def slow_map(n, first, phase=0, src=0):
    """One tile of n frames from `first`: steps 1, 0, 1, 0 ... (phase 0) or 0, 1, 0, 1 ... (phase 1)."""
    return _tile(src, [first + (j + 1 - phase) // 2 for j in range(n)])


def fast_map(n, first, src=0):
    """One tile of n frames from `first`, all steps 2."""
    return _tile(src, [first + 2 * j for j in range(n)])


def paced_steps(rng, n):
    """n steps of 0, 1 or 2, never 0 twice in a row."""
    out, prev = [], 1
    for _ in range(n):
        prev = int(rng.integers(0 if prev else 1, 3))
        out.append(prev)
    return out


def random_lane(rng, n_frames, n_sounds, frames_per_sound, gap_rate=0.2):
    """n_frames rows: sounding tiles of 1 ... 24 frames on random sounds with random admissible steps, gap runs of
    1 ... 3 frames before a tile with probability gap_rate, and three tiles in ten placed within five hops of their
    recording's end, so that they run past it.  frames_per_sound: the whole hops of each sound."""
    rows = []
    while len(rows) < n_frames:
        if rng.random() < gap_rate:
            rows.extend([(GAP, NO_MATCH, 1)] * int(rng.integers(1, 4)))
            continue
        src = int(rng.integers(0, n_sounds))
        hops = int(frames_per_sound[src])
        first = max(0, hops - int(rng.integers(0, 6))) if rng.random() < 0.3 else int(rng.integers(0, hops + 3))
        steps = paced_steps(rng, int(rng.integers(1, 25)) - 1)
        rows.extend(_tile(src, first + np.concatenate([[0], np.cumsum(steps)]).astype(np.int64)))
    return rows[:n_frames]
