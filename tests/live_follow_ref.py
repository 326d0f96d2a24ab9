"""Plain restatement of live envelope following (ssym_follower_*; DESIGN.md section 2 "Live envelope following", the comment
in include/soundsym_amd.h) -- test infrastructure, what the GPU and the host plan are held to.

A lane receives y (the resynthesis) and x (the reference) in any amounts; ny and nx are the counts consumed since its reset.
With h = min(ny, nx) // HOP, before a flush: max(0, h - 1) boundaries are settled and max(0, h - 2) hops released.  The flush
settles every boundary of follow_ref.boundaries(ny) and releases the rest of y.

LiveFollower does NOT run a resumable algorithm: at every call it renders follow_ref.follow_one on the whole consumed prefix
(y[:ny], x[:nx]) and returns the slice the closed-form counts name.  So a test that holds the concatenation against
follow_one of the finished signals checks the rule's safety -- that a settled gain or a released sample never changes
afterwards -- instead of assuming it.

plan() restates soundsym_amd/csrc/follower_plan.hpp: from the lanes' (ny, nx, released, ended) and a call's amounts the new
counts, the per-lane released and settled ranges, the block table, the stretch offsets of the logs and the ring capacity.
"""
import numpy as np

import follow_ref as fr
from follow_ref import HOP, MAX_GAIN  # noqa: F401

BLOCK = 32                       # boundaries per entry of the block table
RING_MIN = 2048                  # samples per lane and signal, at least
RING_BYTES = 512 << 20           # both rings of an object, at most
MAX_LANES = RING_BYTES // (16 * RING_MIN)
MAX_LEN = 1 << 40
NO_LANE = 0xFFFFFFFF
assert MAX_LANES == 16384


def settled(ny, nx) -> int:
    """Boundaries settled before the flush."""
    return max(0, min(int(ny), int(nx)) // HOP - 1)


def released_hops(ny, nx) -> int:
    """Hops released before the flush."""
    return max(0, min(int(ny), int(nx)) // HOP - 2)


class Lane:
    def __init__(self):
        self.y, self.x = np.zeros(0), np.zeros(0)
        self.released, self.settled, self.ended = 0, 0, False

    @property
    def ny(self):
        return int(self.y.size)

    @property
    def nx(self):
        return int(self.x.size)


class LiveFollower:
    """n_lanes lanes.  push and flush return, per lane, (samples, gains): what the call released and settled."""

    def __init__(self, n_lanes=1, max_gain=MAX_GAIN, hold_back=0):
        """hold_back: hops of look-ahead taken away from the rule (-1 releases one hop earlier: the planted case)."""
        self.lanes = [Lane() for _ in range(n_lanes)]
        self.max_gain, self.hold_back = float(max_gain), int(hold_back)

    def _render(self, ln, rel_to, set_to):
        out, g = fr.follow_one(ln.y, ln.x, self.max_gain)
        res = out[ln.released:rel_to].copy(), g[ln.settled:set_to].copy()
        ln.released, ln.settled = rel_to, set_to
        return res

    def push(self, ys, xs):
        """ys, xs: per lane the new samples (None or empty: nothing)."""
        res = []
        for ln, y, x in zip(self.lanes, ys, xs):
            y = np.zeros(0) if y is None else np.asarray(y, dtype=np.float64).reshape(-1)
            x = np.zeros(0) if x is None else np.asarray(x, dtype=np.float64).reshape(-1)
            if ln.ended:
                assert y.size == 0 and x.size == 0, "the lane has ended"
                res.append((np.zeros(0), np.zeros(0)))
                continue
            if y.size == 0 and x.size == 0:                        # nothing new: nothing settles (and no render: many idle lanes)
                res.append((np.zeros(0), np.zeros(0)))
                continue
            ln.y, ln.x = np.concatenate([ln.y, y]), np.concatenate([ln.x, x])
            h = min(ln.ny, ln.nx) // HOP - self.hold_back
            res.append(self._render(ln, max(ln.released, max(0, h - 2) * HOP), max(ln.settled, max(0, h - 1))))
        return res

    def flush(self, lane):
        ln = self.lanes[lane]
        assert not ln.ended
        res = self._render(ln, ln.ny, fr.boundaries(ln.ny))
        ln.ended = True
        return res

    def reset(self, lane):
        self.lanes[lane] = Lane()

    def counts(self):
        return ([ln.ny for ln in self.lanes], [ln.nx for ln in self.lanes], [ln.released for ln in self.lanes])


def run_cuts(y, x, cuts, max_gain=MAX_GAIN, hold_back=0):
    """One lane fed (y, x) by `cuts` -- a list of (my, mx) amounts; what is left of either goes in with a last push -- then
    flushed: (samples, gains), concatenated over the calls."""
    f = LiveFollower(1, max_gain, hold_back)
    ay = ax = 0
    outs, gs = [], []
    for my, mx in list(cuts) + [(len(y), len(x))]:
        (o, g), = f.push([y[ay:ay + my]], [x[ax:ax + mx]])
        ay, ax = min(ay + my, len(y)), min(ax + mx, len(x))
        outs.append(o)
        gs.append(g)
    o, g = f.flush(0)
    return np.concatenate(outs + [o]), np.concatenate(gs + [g])


def random_cuts(rng, ny, nx, top=700):
    """Amounts that eat (ny, nx) in random steps of 0 ... top samples, the two signals on their own."""
    cuts, ay, ax = [], 0, 0
    while ay < ny or ax < nx:
        my, mx = (int(rng.integers(0, top + 1)) if rng.random() < 0.8 else 0 for _ in range(2))
        my, mx = min(my, ny - ay), min(mx, nx - ax)
        cuts.append((my, mx))
        ay, ax = ay + my, ax + mx
    return cuts


# ---- the host plan (follower_plan.hpp) ------------------------------------------------------------------------------------

def held_from(released) -> int:
    return max(0, released // HOP - 2) * HOP


def pow2_at_least(x) -> int:
    p = 1
    while p < x:
        p <<= 1
    return p


def plan(lanes, my=None, mx=None, flush_lane=NO_LANE):
    """lanes: per lane (ny, nx, released, ended).  my / mx: per lane the amounts of a push (None: a flush of flush_lane).
    Returns a dict: steps (per lane: ny, nx, my, mx, yAt, xAt, setFirst, setCount, relFirst, relCount, outAt, gainAt), table
    ((lane, first, count)), samples, gains, maxAppend, maxReleased, maxBlock, ringCap, after (the lanes after the call)."""
    n = len(lanes)
    my = [0] * n if my is None else [int(v) for v in my]
    mx = [0] * n if mx is None else [int(v) for v in mx]
    steps, table, after = [], [], []
    samples = gains = max_append = max_released = max_block = held = 0
    y_at = x_at = 0
    for l, (ny, nx, released, ended) in enumerate(lanes):
        s = dict(ny=ny + my[l], nx=nx + mx[l], my=my[l], mx=mx[l], yAt=y_at, xAt=x_at, setFirst=0, setCount=0, relFirst=released,
                 relCount=0, outAt=samples, gainAt=gains)
        y_at, x_at = y_at + my[l], x_at + mx[l]
        if ended:
            s["setFirst"] = fr.boundaries(ny)
            steps.append(s)
            after.append((ny, nx, released, 1))
            continue
        s["setFirst"] = settled(ny, nx)
        set_end, rel_end = settled(s["ny"], s["nx"]), released_hops(s["ny"], s["nx"]) * HOP
        if l == flush_lane:
            set_end, rel_end = fr.boundaries(s["ny"]), s["ny"]
        s["setCount"], s["relCount"] = set_end - s["setFirst"], rel_end - released
        for b in range(0, s["setCount"], BLOCK):
            table.append((l, s["setFirst"] + b, min(BLOCK, s["setCount"] - b)))
            max_block = max(max_block, table[-1][2])
        samples, gains = samples + s["relCount"], gains + s["setCount"]
        max_append = max(max_append, my[l], mx[l])
        max_released = max(max_released, s["relCount"])
        held = max(held, max(s["ny"], s["nx"]) - held_from(released))
        steps.append(s)
        after.append((s["ny"], s["nx"], rel_end, 1 if l == flush_lane else 0))
    cap = pow2_at_least(max(held, RING_MIN))
    return dict(steps=steps, table=table, samples=samples, gains=gains, maxAppend=max_append, maxReleased=max_released,
                maxBlock=max_block, ringCap=cap, fits=cap <= RING_BYTES // 16 // n, after=after)
