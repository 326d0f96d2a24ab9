"""The case set tests/cpp/test_mirror_dtw.cpp reads and tests/test_gpu_mirror_dtw.py compares it on, and the container both
sides pass arrays in -- TEST INFRASTRUCTURE.

The container: named little-endian arrays, nothing else.

    8 bytes   b"SSYMARR1"
    u32       number of entries
    entry     u8 name length (1 ... 255), the name (ASCII), u8 dtype (0 f64, 1 u32, 2 u64), u64 element count, the elements

The cases are a pure function of the seed (build()): three lists of sounds -- recordings (the dictionary spot, spot_all, the
span calls and the Spotter are run on), targets, and segments (the dictionary match_indices_step, pair_matrix_step,
candidates, chain_indices, align and warp are run on) -- and the arguments of the calls that are data (index lists, distances,
thresholds, hand-made spans, push schedules).  What each of them is there for is said where it is built and is checked from
the restatements, on the CPU, by tests/test_mirror_cases.py."""
import struct

import numpy as np

MAGIC = b"SSYMARR1"
DTYPES = {0: np.dtype("<f8"), 1: np.dtype("<u4"), 2: np.dtype("<u8")}
CODES = {v: k for k, v in DTYPES.items()}
MAX_NAME = 255

HOP, NCOEFFS, RATE = 256, 12, 44100.0
NO_MATCH = 0xFFFFFFFF
SEED = 0x3D7C

REC_FRAMES = (300, 70, 1, 40, 40)                 # the last two are one recording twice: spot_all's tie
REC_SAMPLES = (300 * HOP + 768, 70 * HOP - 100, HOP, 40 * HOP, 40 * HOP)   # what analysis leaves; a short last frame; exact
TGT_FRAMES = (1, 2, 8, 33, 65, 0)
TGT_SAMPLES = (HOP, 1, 8 * HOP, 33 * HOP, 65 * HOP, 0)
SEG_FRAMES = (4, 17, 33, 66, 130, 0)
SEG_SAMPLES = (4 * HOP, 17 * HOP + 768, 33 * HOP, 66 * HOP, 130 * HOP, 500)   # (the frameless one has samples: a length fit)

PLANT33, PLANT65 = 100, 200                       # targets 3 and 4 are noisy copies of recording 0 from these frames on
PLANT8 = (5, 25)                                  # target 2 is recordings 3 and 4 at both of these frames, exactly
MOVED33 = 50                                      # ... and where the replacement of recording 0 (case k) holds target 3

# align / warp: target t against segment INDICES[x][t].  "a": the frameless segment and the frameless target, a 130-frame
# segment too long for the paced pattern; "b": the paced pattern's shortest admissible sources (4 for 8, 17 for 33)
INDICES = {"a": (0, 1, 5, 2, 4, 3), "b": (0, 0, 0, 1, 3, 5)}
# spot / spot_all with indices: the recording of every target (33 frames in the one-frame recording: no paced spot)
SPOT_INDICES = (2, 0, 3, 2, 1, 4)
# spans by hand: one ending on the last frame of a recording of each sample-count kind (exact, long, short), an empty Spot
HAND = ((2, 0, 0), (0, 280, 299), (3, 30, 39), (NO_MATCH, NO_MATCH, NO_MATCH), (1, 5, 69), (0, 0, 10))
# Spotter: frames per push and lane.  One lane watches recording 0, three lanes recordings 0, 1 and 3
PUSH1 = (0, 1, 63, 64, 65, 107)
PUSH3 = ((0, 1, 40), (1, 0, 0), (63, 5, 0), (64, 64, 0), (65, 0, 0), (107, 0, 0))
LANES3 = (0, 1, 3)
AGAIN = {1: 0, 3: 1}                              # the lane that is reset and fed a second time
# follow: samples per push and lane of a two-lane stream fed the samples of recordings 0 and 1
FOLLOW = ((1000, 0), (40000, REC_SAMPLES[1]), (REC_SAMPLES[0] - 41000, 0))


def write_arrays(path, arrays):
    """arrays: a mapping name -> array of dtype float64, uint32 or uint64 (written flat)."""
    with open(path, "wb") as f:
        f.write(MAGIC + struct.pack("<I", len(arrays)))
        for name, a in arrays.items():
            raw = name.encode("ascii")
            a = np.asarray(a)
            if not 1 <= len(raw) <= MAX_NAME:
                raise ValueError("a name has 1 ... 255 bytes")
            if a.dtype.newbyteorder("<") not in CODES:
                raise ValueError("%s: dtype %s is none of f64, u32, u64" % (name, a.dtype))
            flat = np.ascontiguousarray(a, dtype=a.dtype.newbyteorder("<")).reshape(-1)
            f.write(struct.pack("<B", len(raw)) + raw + struct.pack("<BQ", CODES[flat.dtype], flat.size))
            f.write(flat.tobytes())


def read_arrays(path):
    """The mapping write_arrays wrote, in its order; ValueError on anything else."""
    with open(path, "rb") as f:
        buf = f.read()
    if buf[:8] != MAGIC or len(buf) < 12:
        raise ValueError("not an array container")
    (n,), at, out = struct.unpack_from("<I", buf, 8), 12, {}
    for _ in range(n):
        ln = buf[at]
        name = buf[at + 1:at + 1 + ln].decode("ascii")
        code, count = struct.unpack_from("<BQ", buf, at + 1 + ln)
        at += 1 + ln + 9
        dt = DTYPES[code]
        if ln == 0 or at + count * dt.itemsize > len(buf):
            raise ValueError("truncated array container")
        if name in out:
            raise ValueError("the name %s twice" % name)
        out[name] = np.frombuffer(buf, dtype=dt, count=count, offset=at).astype(dt.newbyteorder("="))
        at += count * dt.itemsize
    if at != len(buf):
        raise ValueError("bytes after the last array")
    return out


def spotter_lanes(n_lanes):
    """(the recording every lane watches, frames per push and lane [pushes][lanes]) of the Spotter cases."""
    if n_lanes == 1:
        return (0,), [(f,) for f in PUSH1]
    return LANES3, [tuple(row) for row in PUSH3]


def expected_events(cases, n_lanes, step="symmetric", max_cost=None):
    """The Spotter case of n_lanes lanes from the restatement (watch_ref, or paced_watch_ref under "paced"): (events per
    push, bests per push, events of the flush of every lane after the last push).  Events are (lane, target, cost, start,
    end) ordered by (lane, target, end); bests[p][lane][target] is (cost, start, end)."""
    import paced_watch_ref
    import watch_ref
    ref = paced_watch_ref if step == "paced" else watch_ref
    recs, pushes = spotter_lanes(n_lanes)
    n_push = len(pushes)
    per_push, bests, flushed = [[] for _ in range(n_push)], [[] for _ in range(n_push)], [[] for _ in range(n_lanes)]
    for lane, r in enumerate(recs):
        cuts = np.concatenate([[0], np.cumsum([row[lane] for row in pushes])])
        for p in range(n_push):
            bests[p].append([])
        for t, (_, tgt) in enumerate(cases.tgts):
            limit = None if max_cost is None else float(max_cost[t])
            ev, best, fl, _ = ref.watch(cases.recs[r][1], tgt, cuts, limit, flush_after=(n_push - 1,))
            for p in range(n_push):
                per_push[p] += [(lane, t) + e for e in ev[p]]
                bests[p][lane].append(best[p])
            flushed[lane] += [(lane, t) + e for e in fl.get(n_push - 1, [])]
    order = lambda evs: sorted(evs, key=lambda e: (e[0], e[1], e[4]))
    return [order(x) for x in per_push], bests, [order(x) for x in flushed]


def _features(rng, frames):
    return rng.normal(size=(frames, NCOEFFS)) * (4.0 / (1.0 + np.arange(NCOEFFS)))


def _samples(rng, n, freq):
    t = np.arange(n)
    return 0.4 * np.sin(2.0 * np.pi * freq * t / RATE + rng.uniform(0.0, 6.0)) + 0.05 * rng.normal(size=n)


class Cases:
    """recs, tgts, segs: lists of (samples f64 [n], features f64 [frames, NCOEFFS]); args: name -> array."""

    def __init__(self, recs, tgts, segs, repl, args):
        self.recs, self.tgts, self.segs, self.repl, self.args = recs, tgts, segs, repl, args

    def arrays(self):
        """What the case file holds."""
        out = {}
        for kind, sounds in (("rec", self.recs), ("tgt", self.tgts), ("seg", self.segs), ("repl", self.repl)):
            for i, (smp, feats) in enumerate(sounds):
                out["%s%d.samples" % (kind, i)] = smp
                out["%s%d.mfccs" % (kind, i)] = feats.reshape(-1)
        out.update(self.args)
        return out


def build(seed=SEED):
    rng = np.random.default_rng(seed)
    rf = [_features(rng, f) for f in REC_FRAMES]
    rf[3][PLANT8[1]:PLANT8[1] + 8] = rf[3][PLANT8[0]:PLANT8[0] + 8]
    rf[4] = rf[3].copy()
    tf = [_features(rng, f) for f in TGT_FRAMES]
    tf[1] = tf[1] + 50.0                                                  # far from everything
    tf[2] = rf[3][PLANT8[0]:PLANT8[0] + 8].copy()
    tf[3] = rf[0][PLANT33:PLANT33 + 33] + 0.05 * rng.normal(size=(33, NCOEFFS))
    tf[4] = rf[0][PLANT65:PLANT65 + 65] + 0.05 * rng.normal(size=(65, NCOEFFS))
    sf = [_features(rng, f) for f in SEG_FRAMES]
    rs = [_samples(rng, n, 180.0 + 70.0 * i) for i, n in enumerate(REC_SAMPLES)]
    rs[4] = rs[3].copy()
    ts = [_samples(rng, n, 300.0 + 45.0 * i) for i, n in enumerate(TGT_SAMPLES)]
    ss = [_samples(rng, n, 240.0 + 90.0 * i) for i, n in enumerate(SEG_SAMPLES)]
    # case k: recording 0 replaced by one that holds target 3 elsewhere; segment 2 replaced by target 3 itself
    r0 = _features(rng, REC_FRAMES[0])
    r0[MOVED33:MOVED33 + 33] = tf[3] + 0.05 * rng.normal(size=(33, NCOEFFS))
    repl = [(_samples(rng, REC_SAMPLES[0], 410.0), r0), (_samples(rng, SEG_SAMPLES[2], 520.0), tf[3].copy())]
    hand = np.array(HAND, dtype=np.uint32)
    args = {
        "distances": np.array([0.0, 3.0, 0.0, 40.0, 10.0, 1.0]),          # per target: match_indices_step, candidates
        "chain.distances": np.array([0.0, 30.0, 5.0, 0.0, 60.0]),
        "indices.a": np.array(INDICES["a"], dtype=np.uint32), "indices.b": np.array(INDICES["b"], dtype=np.uint32),
        "spot.indices": np.array(SPOT_INDICES, dtype=np.uint32),
        "hand.src": hand[:, 0].copy(), "hand.start": hand[:, 1].copy(), "hand.end": hand[:, 2].copy(),
        # spot_all's threshold: the noisy copies cost about 0.05 * sqrt(12) a frame, anything else about 6 a frame
        "spot_all.max_cost": np.array([30.0]),
        "spotter.max_cost": np.array([3.0, 1.0, 0.5, 30.0, 60.0, 1.0]),
        "push1": np.array(PUSH1, dtype=np.uint64), "push3": np.array(PUSH3, dtype=np.uint64).reshape(-1),
        "lanes3": np.array(LANES3, dtype=np.uint32),
        "follow": np.array(FOLLOW, dtype=np.uint64).reshape(-1),
    }
    return Cases(list(zip(rs, rf)), list(zip(ts, tf)), list(zip(ss, sf)), repl, args)
