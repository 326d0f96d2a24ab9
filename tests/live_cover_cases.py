"""Cases of the live cover's tests -- TEST INFRASTRUCTURE shared by tests/test_live_cover_ref.py (CPU) and the GPU tests of
the coverer.  A case is (segments, target): segments a list of [frames][dim] f64 arrays, target [T][dim].  Every value is
an f32 value, so both engine dtypes hold it."""
import numpy as np

import cover_ref


def _real(rng, shape):
    return rng.standard_normal(shape).astype(np.float32).astype(np.float64)


def _ints(rng, shape):
    return rng.integers(-1, 2, size=shape).astype(np.float64)          # {-1, 0, 1}: costs tie, the tie rules decide


def random_case(seed, lens, T, dim=3, ints=False, noise=0.25):
    """Segments of the given lengths; the target is a run of randomly chosen segments, some with every frame doubled, with
    noise on top (real cases) -- so that long pieces win and commits happen -- cut or padded to T frames."""
    rng = np.random.default_rng(seed)
    draw = _ints if ints else _real
    segs = [draw(rng, (n, dim)) for n in lens]
    parts, have = [], 0
    usable = [a for a in segs if a.shape[0]]
    while have < T:
        a = usable[int(rng.integers(len(usable)))]
        part = np.repeat(a, 2, axis=0) if rng.integers(3) == 0 else a
        parts.append(part)
        have += part.shape[0]
    x = np.concatenate(parts, axis=0)[:T]
    if not ints:
        x = (x + noise * rng.standard_normal(x.shape)).astype(np.float32).astype(np.float64)
    return segs, x


def small_cases():
    """name -> (segments, target): real and tying cases on segments of 0 ... 8 frames, a dictionary whose shortest segment
    has 5 frames (frames 0 and 1 have no cover), and the planted case with noise."""
    return {
        "real": random_case(0xA1, [3, 0, 8, 1, 5, 2, 7, 4, 6, 8, 2, 3], 90),
        "ints": random_case(0xA2, [3, 0, 8, 1, 5, 2, 7, 4, 6, 8, 2, 3], 90, ints=True),
        "ints_short": random_case(0xA3, [1, 2, 2, 3, 1], 60, dim=2, ints=True),
        "shortest5": random_case(0xA4, [5, 8, 6, 7, 5], 80),
        "planted": cover_ref.planted_case(1e-3)[:2],
    }


def random_cuts(rng, T, mean):
    """[0, ..., T]: pushes of 0 ... 2 mean frames."""
    cuts = [0]
    while cuts[-1] < T:
        cuts.append(min(T, cuts[-1] + int(rng.integers(0, 2 * mean + 1))))
    return cuts


def even_cuts(T, step):
    return list(range(0, T, step)) + [T]
