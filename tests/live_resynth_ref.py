"""Plain restatement of live resynthesis (ssym_resynth_*; DESIGN.md section 2 "Live resynthesis", the comment in
include/soundsym_amd.h) -- TEST INFRASTRUCTURE, what the GPU is held to bit for bit.

Defined by reduction, and so is this file: a tile is rendered by tests/span_ref.py (which slices the window and asks
tests/warp_ref.py or tests/wsola_ref.py), and the class below only decides WHEN a hop leaves and with which window.

    frames      (src, frame, start) per column; src = GAP a gap frame; a tile starts at every start = 1
    offline     the reference output of a finished lane: every tile rendered whole, the last one to the lane's end
    LiveResynth the incremental form: push(frames) / flush(total_samples) return the samples they release
    release     hop j leaves when its tile is closed, when map[j] + R <= L (L the open tile's latest map value), or at
                once as a gap frame; the open tile is rendered with the window end (L + 1) * HOP, clipped to the recording
"""
import numpy as np

import span_ref
from warp_ref import HOP, pcm32  # noqa: F401

GAP = 0xFFFFFFFE
NO_MATCH = 0xFFFFFFFF


def reach(search):
    """R of the release rule."""
    return 2 if search == 0 else (search + 1279) // 256


def render_tile(sounds, src, fmap, last, n_out, search, cache=None):
    """n_out samples of the tile with map `fmap` of sound src, rendered with the window [min(first * HOP, n_src),
    min((last + 1) * HOP, n_src)), the map fmap - first and pos[0] = 0: the _spans call for one target."""
    key = (int(src), tuple(int(v) for v in fmap), int(last), int(n_out), int(search))
    if cache is not None and key in cache:
        return cache[key]
    n_src = len(sounds[src])
    first = int(fmap[0])
    a, b = min(first * HOP, n_src), min((int(last) + 1) * HOP, n_src)
    rel = np.asarray(fmap, dtype=np.int64) - first
    args = (sounds, [src], [a], [max(b - a, 0)], [0, n_out], rel, [0, len(rel)], [len(rel)])
    out = span_ref.wsola_spans(*args, search=search)[0] if search else span_ref.warp_spans(*args)
    if cache is not None:
        cache[key] = out
    return out


def tiles(frames):
    """[(first column, one past the last column)] of a lane's frames."""
    cuts = [j for j, f in enumerate(frames) if f[2] or j == 0] + [len(frames)]
    return list(zip(cuts[:-1], cuts[1:]))


def offline(sounds, frames, total_samples, search=0, cache=None):
    """The reference output of a lane that ended with total_samples samples."""
    out = np.zeros(total_samples, dtype=np.float64)
    spans = tiles(frames)
    for i, (a, b) in enumerate(spans):
        n = (total_samples - a * HOP) if i == len(spans) - 1 else (b - a) * HOP
        if frames[a][0] != GAP:
            fmap = [f[1] for f in frames[a:b]]
            out[a * HOP:a * HOP + n] = render_tile(sounds, frames[a][0], fmap, fmap[-1], n, search, cache)
    return out


class LiveResynth:
    """One lane.  reach_override: another R than the rule's (the tightness test plants R - 1)."""

    def __init__(self, sounds, search=0, reach_override=None, cache=None):
        self.sounds, self.search, self.cache = sounds, int(search), cache
        self.R = reach(self.search) if reach_override is None else reach_override
        self.maps, self.n, self.released, self.ended = [], 0, 0, False
        self.a, self.src, self.L = None, GAP, 0          # the open tile

    @property
    def held(self):
        return self.n - self.released

    def _release(self, upto, tail=0):
        """Hops released ... upto - 1 of the open tile (and `tail` samples behind hop upto - 1), rendered as of now."""
        count = (upto - self.released) * HOP + tail
        if count == 0:
            return np.zeros(0)
        if self.a is None or self.src == GAP:
            out = np.zeros(count)
        else:
            fmap = self.maps[self.a:upto]
            out = render_tile(self.sounds, self.src, fmap, self.L, (upto - self.a) * HOP + tail, self.search, self.cache)
            out = out[(self.released - self.a) * HOP:]
        self.released = upto
        return out

    def push(self, frames):
        """Consume (src, frame, start) rows; the samples this releases."""
        assert not self.ended
        out = [np.zeros(0)]
        for src, frame, start in frames:
            src, frame = int(src), int(frame)
            if start or self.a is None:
                out.append(self._release(self.n))                    # the tile is closed
                self.a, self.src = self.n, src
            self.maps.append(frame)
            self.n += 1
            self.L = frame
            if self.src == GAP:
                out.append(self._release(self.n))
                continue
            j = self.released
            while j < self.n and self.maps[j] + self.R <= self.L:
                j += 1
            out.append(self._release(j))
        return np.concatenate(out)

    def flush(self, total_samples):
        assert not self.ended and total_samples >= self.n * HOP
        self.ended = True
        return self._release(self.n, total_samples - self.n * HOP)
