"""Cases with more tasks than a grid has workgroups -- TEST INFRASTRUCTURE shared by tests/test_count_cases.py (CPU) and the
GPU tests test_gpu_paced_match_counts.py, test_gpu_cover_counts.py and test_gpu_coverer_lanes.py.  No GPU is needed here.

dtw_match_paced_kernel, cover_forward_kernel and cover_chain_kernel reach the targets beyond their grid by a stride, so one
workgroup handles target b, then b + stride, and carries LDS and registers from the one to the next.  A case here has

    kinds     8 kinds of target per family (frames, or "no source fits", or "a NaN frame")
    drawn     the targets that share a workgroup with another one are drawn one by one: target b < 64 has kind
              (b // 8) % 8 and target stride + b has kind b % 8, so that the two targets workgroup b visits in a row run
              through all 64 ordered pairs of kinds
    bulk      everything else only occupies indices: it is taken from a pool of 64 short targets (0 ... 6 frames)
    uniq/ids  the distinct targets and, per target, which of them it is.  A target's result does not depend on its
              neighbours, so the restatements run once over `uniq` and `gather` / `gather_cover` lay the results out

Every value is an f32 value, so both engine dtypes hold it."""
import numpy as np

import cover_ref
import live_cover_cases
import paced_match_ref

INF, NAN = float("inf"), float("nan")
POOL = 64

PACED_STRIDE = 65536                 # kMatchPacedGridX
FORWARD_STRIDE = 65535               # kCoverGridZ
COVER_SCRATCH = 512 << 20            # kCoverScratchBytes
COVER_RING = 512                     # kCoverRing


def chain_stride(cus):
    """cover_chain_kernel's grid: 8 workgroups per CU."""
    return 8 * cus


def first_kind(b):
    return (b // 8) % 8


def second_kind(b):
    return b % 8


def _real(rng, frames, dim):
    return rng.standard_normal((frames, dim)).astype(np.float32).astype(np.float64)


def drawn_kinds(strides):
    """target index -> kind of every target that is drawn one by one, for workgroups that step by each of `strides`."""
    kinds = {b: first_kind(b) for b in range(64)}
    for stride in strides:
        for b in range(64):
            assert stride + b not in kinds, (stride, b)
            kinds[stride + b] = second_kind(b)
    return kinds


def visits(b, stride, m):
    """The targets workgroup b of a grid of `stride` workgroups handles, in order."""
    return list(range(b, m, stride))


class Counted:
    """m targets over a dictionary: src, uniq (the distinct targets), ids [m] (target t is uniq[ids[t]]), kinds (index ->
    kind of the drawn targets)."""

    def __init__(self, src, dim, m, kinds, draw, seed):
        rng = np.random.default_rng(seed)
        self.src, self.dim, self.m, self.kinds = src, dim, m, kinds
        self.uniq = [_real(rng, int(f), dim) for f in rng.integers(0, 7, size=POOL)]
        self.uniq[0], self.uniq[1] = np.zeros((0, dim)), _real(rng, 6, dim)          # both ends of the pool's range occur
        self.ids = rng.integers(0, POOL, size=m).astype(np.int64)
        for t in sorted(kinds):
            self.ids[t] = len(self.uniq)
            self.uniq.append(draw(rng, kinds[t]))
        self.frames = np.array([u.shape[0] for u in self.uniq], dtype=np.int64)
        self.tgt = [self.uniq[i] for i in self.ids]

    def total_frames(self):
        return int(self.frames[self.ids].sum())


# -- paced matching ------------------------------------------------------------------------------------------------------

PACED_SRC_FRAMES = (1, 2, 3, 5, 9, 30, 63, 64, 70)
PACED_KIND_FRAMES = (0, 1, 3, 33, 64, 65, 130, 300)      # 300: no source is feasible (70 < 150); 130, 300: not resident
PACED_M = PACED_STRIDE + 64


def paced_case(seed=0x65600):
    """65 600 targets against 9 sources, dim 2.  Also .want_u [9][uniq] (the restatement's matrix), .distance_u [uniq] (per
    distinct target: near one of its finite costs, so that the fold's key is not the cost itself)."""
    rng = np.random.default_rng(seed)
    src = [_real(rng, f, 2) for f in PACED_SRC_FRAMES]
    c = Counted(src, 2, PACED_M, drawn_kinds([PACED_STRIDE]), lambda r, k: _real(r, PACED_KIND_FRAMES[k], 2), seed + 1)
    c.want_u = paced_match_ref.matrix(src, c.uniq)
    c.distance_u = np.ones(len(c.uniq))
    for u in range(len(c.uniq)):
        fin = c.want_u[:, u][np.isfinite(c.want_u[:, u])]
        if fin.size:
            c.distance_u[u] = np.float32(fin[int(rng.integers(fin.size))] + rng.uniform(-0.5, 0.5))
    return c


def gather(per_uniq, ids):
    """Per-target arrays from per-distinct-target ones (the last axis is the target's)."""
    return tuple(np.ascontiguousarray(a[..., ids]) for a in per_uniq)


def clamp_case(seed=0x1030):
    """1030 sources of 1 ... 3 frames against 5 short targets: with one source per block asked for, the grid-y clamp
    (kMatchPacedGridY = 1023) makes blocks of 2.  Sources 1021 and 1025 are the same 3 frames as target 0, in blocks 510
    and 512 on either side of index 1023: both cost 0.0 and the lower index must win.  Returns (src, tgt)."""
    rng = np.random.default_rng(seed)
    src = [_real(rng, int(f), 2) for f in rng.integers(1, 4, size=1030)]
    tgt = [_real(rng, f, 2) for f in (3, 1, 2, 5, 4)]
    src[1021], src[1025] = tgt[0].copy(), tgt[0].copy()
    return src, tgt


# -- cover ---------------------------------------------------------------------------------------------------------------

COVER_SRC_FRAMES = (1, 3, 2, 0, 3)                        # Fmax 3: W = 6
COVER_KIND_FRAMES = (0, 1, 5, 64, 65, 130, 600, 20)       # 600 passes kCoverRing; kind 7: 20 frames, one of them NaN
COVER_NAN_KIND = 7
COVER_M = FORWARD_STRIDE + 64
COVER_PENALTY = 1.0


def _cover_target(rng, kind):
    x = _real(rng, COVER_KIND_FRAMES[kind], 2)
    if kind == COVER_NAN_KIND:
        x[int(rng.integers(3, 17)), int(rng.integers(2))] = NAN       # no window holds this frame: no cover
    return x


def cover_case(cus, seed=0x65599):
    """65 599 targets against a dictionary with Fmax 3, dim 2, for a device of `cus` CUs: targets b and b + 8 cus (the
    chain's stride) and targets b and b + 65535 (the forward pass's) both run through the 64 pairs of kinds.  Also
    .want_u, cover_ref.arrays over the distinct targets at COVER_PENALTY."""
    g = chain_stride(cus)
    assert 64 <= g and g + 64 <= FORWARD_STRIDE
    rng = np.random.default_rng(seed)
    src = [_real(rng, f, 2) for f in COVER_SRC_FRAMES]
    c = Counted(src, 2, COVER_M, drawn_kinds([g, FORWARD_STRIDE]), _cover_target, seed + 1)
    c.want_u = cover_ref.arrays(src, c.uniq, COVER_PENALTY)
    return c


def gather_cover(want_u, frames_u, ids):
    """cover_ref.arrays of the targets uniq[ids] from cover_ref.arrays of uniq: counts and totals per target, and every
    target's slots (pieces, then the padding) moved to where its frames lie in the longer list."""
    count, total, src, start, end, cost = want_u
    off_u = np.concatenate([[0], np.cumsum(frames_u)])
    lens = frames_u[ids]
    off = np.concatenate([[0], np.cumsum(lens)])
    slot = np.repeat(off_u[ids] - off[:-1], lens) + np.arange(off[-1])
    return count[ids], total[ids], src[slot], start[slot], end[slot], cost[slot]


def cover_scratch_bytes(frames, width):
    """What ssym_dtw_cover asks of its scratch: one block's tables and the back-pointers."""
    return frames * width * 12 + frames * 16


def long_case(seed=0x1300):
    """Targets of 511, 512, 513 and 1300 frames (around and far beyond kCoverRing) over the 12 segments of at most 8 frames
    the coverer's tests use.  Returns (segments, targets)."""
    lens = [3, 1, 8, 2, 5, 4, 7, 1, 6, 8, 2, 3]
    segs, x = live_cover_cases.random_case(seed, lens, 511 + 512 + 513 + 1300)
    cuts = np.cumsum([0, 511, 512, 513, 1300])
    return segs, [x[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def tie_case(fmax):
    """A dictionary with W = 2 fmax > 64 on which tilings tie: (segments, target, penalty).  Frames are constant 0 or 1 in
    runs, the segments are constant too, so every piece over a run of its own value costs 0.0, a piece across two runs
    costs more than the penalty, and a total counts the pieces.  A run of 2 fmax + 10 ... 30 frames takes two pieces,
    and at its end many splits tie: the shortest last piece must win, and it sits in a higher lane than the last piece of
    65 frames (lane 0) that ties with it."""
    assert fmax in (40, 128)
    rng = np.random.default_rng(0x71E + fmax)
    # (the restatement of a coverer pays for every frame of every segment at every push: fmax 128 gets the fewest it needs)
    lens = [fmax, fmax, fmax // 2, fmax // 2, 5, 3] if fmax == 40 else [fmax, 3, fmax // 2, 5]
    segs = [np.full((n, 2), float(k % 2)) for k, n in enumerate(lens)]
    runs = []
    for k in range(7 if fmax == 40 else 2):
        n = 2 * fmax + 10 + int(rng.integers(0, 21)) if k % 3 != 1 else int(rng.integers(fmax // 2, fmax)) if fmax == 40 else 12
        runs.append(np.full((n, 2), float(k % 2)))
    return segs, np.concatenate(runs, axis=0), 1.0


def tied_lengths(M, S, penalty):
    """Per end e, the lengths L (ascending) whose v = (M + penalty) + best(e - L) is the least one, by cover_ref.chain's
    own additions; [] where no length has a finite v."""
    T, W = M.shape
    best = np.full(T + 1, INF)
    best[0] = 0.0
    out = []
    for e in range(T):
        vs = []
        for L in range(1, min(e + 1, W) + 1):
            s = e - L + 1
            if S[s, L - 1] != cover_ref.NONE:
                vs.append(((float(M[s, L - 1]) + float(penalty)) + float(best[s]), L))
        least = min([v for v, _ in vs] + [INF])
        best[e + 1] = least
        out.append([L for v, L in vs if v == least] if least < INF else [])
    return out


def cross_lane_ties(tied):
    """(ends where the least v is attained by two lengths in different lanes of the wave -- lane (L - 1) % 64 --, those of
    them where the shortest length sits in a HIGHER lane than another tied one)."""
    across, upper = [], []
    for e, ls in enumerate(tied):
        lanes = [(L - 1) % 64 for L in ls]
        if len(set(lanes)) > 1:
            across.append(e)
            if any(lane < lanes[0] for lane in lanes[1:]):
                upper.append(e)
    return across, upper


# -- live cover ----------------------------------------------------------------------------------------------------------

LANES = 300
LANES_LENS = [3, 1, 8, 2, 5, 4, 7, 1, 6, 8, 2, 3]        # Fmax 8: W = 16
LANES_DIM = 3


class Schedule:
    """A seeded schedule of calls on a coverer of LANES lanes: .segs, .ops -- ("push", [chunk per lane]), ("flush", lane),
    ("reset", lane) --, and after the last op .whole[l], everything lane l consumed since its last reset."""

    def __init__(self, seed=0x300, calls=25):
        rng = np.random.default_rng(seed)
        W = 2 * max(LANES_LENS)
        self.segs = [_real(rng, n, LANES_DIM) for n in LANES_LENS]
        self.never = {int(l) for l in rng.choice(np.arange(1, 250), size=12, replace=False)}      # lanes never fed
        self.ops, self.pushes = [], 0
        self.whole = [np.zeros((0, LANES_DIM)) for _ in range(LANES)]
        ended = set()
        for call in range(calls):
            chunks = []
            for l in range(LANES):
                often = l in (256, LANES - 1)
                fed = l not in self.never and l not in ended and rng.random() < (0.95 if often else 0.5)
                chunks.append(self._stream(rng, int(rng.integers(0, 2 * W + 4))) if fed else np.zeros((0, LANES_DIM)))
                self.whole[l] = np.concatenate([self.whole[l], chunks[-1]], axis=0)
            self.ops.append(("push", chunks))
            self.pushes += 1
            if call % 4 == 3:
                # a handful of lanes end; every second one starts over with a new sequence, the others stay ended
                for k, l in enumerate(int(v) for v in rng.choice(LANES - 1, size=6, replace=False)):
                    if l == 256:
                        continue                     # (lanes 256 and 299 go on to the end)
                    if l in ended:
                        continue
                    self.ops.append(("flush", l))
                    ended.add(l)
                    if k % 2 == 0:
                        self.ops.append(("reset", l))
                        ended.discard(l)
                        self.whole[l] = np.zeros((0, LANES_DIM))
        self.ended = ended

    def _stream(self, rng, frames):
        """`frames` frames made of segments, some with every frame doubled, with noise on top."""
        parts, have = [], 0
        while have < frames:
            a = self.segs[int(rng.integers(len(self.segs)))]
            parts.append(np.repeat(a, 2, axis=0) if rng.integers(3) == 0 else a)
            have += parts[-1].shape[0]
        if not parts:
            return np.zeros((0, LANES_DIM))
        x = np.concatenate(parts, axis=0)[:frames]
        return (x + 0.25 * rng.standard_normal(x.shape)).astype(np.float32).astype(np.float64)
