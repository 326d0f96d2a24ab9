"""The inputs of tests/test_gpu_wavefront_nonfinite.py and what the restatements make of them -- TEST INFRASTRUCTURE.

One case = one poisoned value in otherwise clean, real-valued data of `dim` values per frame:

    target   70 frames: 35 distinct frames, each twice, so that the 35 distinct frames on their own align with it at cost 0
    one      a one-frame target (column 0 alone, which restarts in every row)
    source   130 frames of noise with the 35 frames planted at rows 10 ... 44 and 80 ... 114: two clean copies, one on
             each side of rows 63 ... 65, both after rows 0 and 1, both before row 129
    other    a clean second source, so that a fold over sources has something to prefer

    value    NaN, +inf, -inf (rooted cost), +-1e200 (squared: the product overflows to +inf; rooted: 1e400 overflows
             before the square root)
    place    source row 0, 1, 63, 64, 65 or 129 (first row, both sides of the 64-row chunk's hand-off, last row), or target
             column 0, 1, 63, 64 or 69 (the free-start column, both sides of the ring's refill, the last column)

The value goes into the frame's last element: the one next to the zero padding (13 -> 14, 41 -> 64 values)."""
import functools

import numpy as np

import dtw_path_ref
import spot_all_ref
import spot_ref
import watch_ref

NAN, INF = float("nan"), float("inf")
VALUES = [("nan", NAN, False), ("+inf", INF, False), ("-inf", -INF, False), ("+1e200", 1e200, True), ("+1e200", 1e200, False),
          ("-1e200", -1e200, True), ("-1e200", -1e200, False)]
PLACES = [("src", r) for r in (0, 1, 63, 64, 65, 129)] + [("tgt", j) for j in (0, 1, 63, 64, 69)]
DIMS = (13, 41)
CASES = [(dim, name, squared, side, frame) for dim in DIMS for name, _, squared in VALUES for side, frame in PLACES]
PLANTS = ((10, 44), (80, 114))
K = 4
PUSHES = [0, 1, 64, 65, 130]


def ident(case):
    dim, name, squared, side, frame = case
    return "dim%d-%s-%s-%s%d" % (dim, name, "squared" if squared else "rooted", side, frame)


def _real(rng, f, dim):
    return rng.standard_normal((f, dim)).astype(np.float32).astype(np.float64)       # (f32 values: both dtypes hold them)


@functools.lru_cache(maxsize=None)
def _clean(dim):
    rng = np.random.default_rng(0xC1EA + dim)
    u = _real(rng, 35, dim)
    source = _real(rng, 130, dim)
    for lo, hi in PLANTS:
        source[lo:hi + 1] = u
    return np.repeat(u, 2, axis=0), _real(rng, 1, dim), source, _real(rng, 90, dim)


class Case:
    """The data of one case and, computed once and never written to again, the restatements' results for it."""

    def __init__(self, case):
        self.dim, self.name, self.squared, self.side, self.frame = case
        self.value = dict((n, v) for n, v, _ in VALUES)[self.name]
        target, one, source, other = (x.copy() for x in _clean(self.dim))
        (source if self.side == "src" else target)[self.frame, self.dim - 1] = self.value
        self.sources, self.targets = [source, other], [target, one]
        self._prof = {}

    # -- restatements ----------------------------------------------------------------------------------------------------
    def profile(self, s, t):
        """(delta, s) of source s against target t (spot_all_ref.profile, which is watch_ref.whole_profile's)."""
        if (s, t) not in self._prof:
            self._prof[(s, t)] = watch_ref.whole_profile(self.sources[s], self.targets[t], self.squared)
        return self._prof[(s, t)]

    def spot(self, s, t):
        """spot_ref.spot's (cost, start, end), from the cached profile."""
        delta, st = self.profile(s, t)
        end, cost = spot_ref.first_end(delta)
        return (INF, spot_ref.NO_MATCH, spot_ref.NO_MATCH) if end == spot_ref.NO_MATCH else (cost, int(st[end]), end)

    def spot_best(self, t):
        best = (spot_ref.NO_MATCH, INF, spot_ref.NO_MATCH, spot_ref.NO_MATCH)
        for s in range(len(self.sources)):
            cost, start, end = self.spot(s, t)
            if cost < best[1]:
                best = (s, cost, start, end)
        return best

    def spot_all(self, s, t):
        """(count, cost [K], start [K], end [K])."""
        return spot_all_ref.padded(spot_all_ref.select(*self.profile(s, t), K), K)

    def watch(self, t, cuts=PUSHES):
        """watch_ref.drive of the poisoned source against target t, flushed after the last push."""
        return watch_ref.drive(*self.profile(0, t), cuts, None, flush_after=(len(cuts) - 2,))

    def cuts_around(self):
        """One frame at a time around the poisoned row (around row 64 when the target holds the value), so that what the
        row leaves behind crosses the stored state."""
        r = self.frame if self.side == "src" else 64
        return sorted(set([0, 130] + [x for x in range(r - 1, r + 4) if 0 <= x <= 130]))

    def plain_pairs(self):
        """Plain pairs cut from the same data for ssym_dtw_align: (sources, targets, [(source, target), ...]) -- 40 frames
        around the poisoned row (or around row 64), a clean plant, the clean second source; both targets."""
        r = self.frame if self.side == "src" else 64
        lo = max(0, min(r - 20, 90))
        src = [self.sources[0][lo:lo + 40], self.sources[0][PLANTS[0][0]:PLANTS[0][1] + 1], self.sources[1][:50]]
        return src, self.targets, [(s, t) for s in range(3) for t in range(2)]

    def align(self, a, b):
        return dtw_path_ref.align(a, b, -1, self.squared)


@functools.lru_cache(maxsize=None)
def get(case):
    return Case(case)


def profile_np_minimum(a, b, squared):
    """The end column as np.minimum (order-free, NaN for any NaN operand) would have it: what the restatement gave
    before it stated the oracle's comparison order."""
    c = dtw_path_ref.local_costs(a, b, squared)
    fa, fb = c.shape
    D = np.full((fa + 1, fb + 1), np.inf)
    for s in range(fa + fb - 1):
        i = np.arange(max(0, s - fb + 1), min(fa - 1, s) + 1)
        j = s - i
        cur = c[i, j] + np.minimum(np.minimum(D[i, j + 1], D[i + 1, j]), D[i, j])
        D[i + 1, j + 1] = np.where(j == 0, c[i, j], cur)
    return D[1:, -1]
