"""Plain restatements of the three steps a caller runs right after a match, for the shape tests of
ssym_chain, ssym_reconstruct and ssym_merge_shards (test_gpu_chain_shapes.py, test_gpu_reconstruct_shapes.py,
test_gpu_merge_shapes.py).

Written from the reference's lines and the header, not from the kernels:
  first_min / chain   SoundDictionary::at_distance's fold (src/sound.rs:361-367) and SoundSequence::from_distances'
                      loop around it (:405-417)
  reconstruct         clone_from_dictionary's length fit (:456-465) and to_sound's concatenation (:475-480)
  pcm32               Sound::write_file's `(i32::max_value() as f64 * sample) as i32` (:139)
  merge               include/soundsym_amd.h, ssym_merge_shards_at: "the same first-minimum rule as src/sound.rs:361-367"
Python floats are IEEE f64 and every operation below is one rounded operation.  tests/test_tail_ref.py holds these
against the C oracle, which was written separately.
"""
import math

import numpy as np


def first_min(values, distance, init):
    """The fold of src/sound.rs:361-367 over |value - distance|: start (0, init), strict '<'.  Returns
    (index, found); found is False when no key was below `init` (the index is then the fold's start, 0).
    A NaN key compares false and never wins."""
    distance = float(distance)
    min_idx, min_key, found = 0, float(init), False
    for idx, v in enumerate(values):
        key = abs(float(v) - distance)
        if key < min_key:
            min_idx, min_key, found = idx, key, True
    return min_idx, found


def chain(matrix_fn, start_col, distances, init, report):
    """from_distances (src/sound.rs:405-417): the entry matched at one step is the query of the next.
    start_col    the values (similarities / costs) of every dictionary entry against the start sound
    matrix_fn    i -> the values of every dictionary entry against dictionary entry i
    report       "key": a step reports |value - distance| (refcos); "value": the value itself (dtw);
                 `init` where nothing was found
    Returns (idx int64 [steps], val f64 [steps])."""
    assert report in ("key", "value")
    col = np.asarray(start_col, dtype=np.float64)
    out_idx, out_val = [], []
    for d in distances:
        i, found = first_min(col, d, init)
        if not found:
            v = float(init)
        elif report == "key":
            v = abs(float(col[i]) - float(d))
        else:
            v = float(col[i])
        out_idx.append(i)
        out_val.append(v)
        col = np.asarray(matrix_fn(i), dtype=np.float64)
    return np.array(out_idx, dtype=np.int64), np.array(out_val, dtype=np.float64)


def best_two_keys(values, distance):
    """The two smallest non-NaN keys |value - distance| of a column (inf where there are fewer): what decides whether
    an index comparison under a cost tolerance is a fair demand."""
    with np.errstate(invalid="ignore"):
        keys = np.abs(np.asarray(values, dtype=np.float64) - float(distance))
    keys = np.sort(keys[~np.isnan(keys)])
    pad = [float("inf")] * 2
    return tuple((list(keys[:2]) + pad)[:2])


def reconstruct(samples, offsets, idx, out_offsets):
    """For target t the samples of sound idx[t], cut to the target's length or padded with +0.0 up to it
    (src/sound.rs:456-465), one after the other (:475-480).  Bit patterns are carried over untouched."""
    samples = np.asarray(samples, dtype=np.float64)
    out = np.zeros(int(out_offsets[-1]), dtype=np.float64)
    for t, s in enumerate(idx):
        o0, o1 = int(out_offsets[t]), int(out_offsets[t + 1])
        sound = samples[int(offsets[int(s)]):int(offsets[int(s) + 1])]
        diff = (o1 - o0) - sound.size
        if diff > 0:
            out[o0:o0 + sound.size] = sound          # the rest stays 0.0
        elif diff < 0:
            out[o0:o1] = sound[:o1 - o0]
        else:
            out[o0:o1] = sound
    return out


I32_MAX, I32_MIN = 2147483647, -2147483648


def pcm32(x):
    """`(i32::max_value() as f64 * sample) as i32`: one f64 product, then Rust's float-to-int cast: toward zero,
    saturating, NaN -> 0.  Integer arithmetic on Python ints, no numpy cast."""
    p = 2147483647.0 * float(x)
    if p != p:
        return 0
    if p == math.inf:
        return I32_MAX
    if p == -math.inf:
        return I32_MIN
    return max(I32_MIN, min(I32_MAX, math.trunc(p)))


def pcm32_array(xs):
    return np.array([pcm32(v) for v in np.asarray(xs, dtype=np.float64).reshape(-1)], dtype=np.int32)


def merge(costs, idx, distance=None):
    """Per target the shard entry with the smallest key |cost - distance| (distance None = 0), the lowest global index
    among equal keys.  The first-minimum rule of src/sound.rs:361-367 lets no NaN key win, so a NaN key never beats
    a key that is not NaN, whichever shard holds it; a column of NaN keys only keeps shard 0's entry (the fold never
    moved).  Returns (idx [m], cost [m]) with the dtypes of the inputs."""
    costs, idx = np.asarray(costs, dtype=np.float64), np.asarray(idx)
    g_n, m = costs.shape
    d = np.zeros(m) if distance is None else np.asarray(distance, dtype=np.float64)
    best = np.full(m, -1, dtype=np.int64)            # the shard whose entry is held, -1 = none yet
    best_key, best_idx = np.full(m, np.nan), np.zeros(m, dtype=np.int64)
    for g in range(g_n):                             # one step for all targets at once; indices compare unsigned
        i = idx[g].astype(np.uint32).astype(np.int64)
        with np.errstate(invalid="ignore"):
            key = np.abs(costs[g] - d)
            take = ~np.isnan(key) & ((best < 0) | (key < best_key) | ((key == best_key) & (i < best_idx)))
        best[take], best_key[take], best_idx[take] = g, key[take], i[take]
    best[best < 0] = 0
    cols = np.arange(m)
    return idx[best, cols], costs[best, cols]
