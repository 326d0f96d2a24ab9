"""Numpy restatement of the paced watching definition ("Paced watching") -- TEST INFRASTRUCTURE, the
reference ssym_spotter_* is held to under SSYM_STEP_PACED.  Row i of the paced recurrence depends on rows i - 1 and i - 2
alone, so the first n rows of the whole's paced profile are the paced profile of the first n frames; the best, the report
rule and the flush are watch_ref's, unchanged, on that profile."""
import numpy as np

import paced_ref
import watch_ref


def whole_profile(source, target, squared=False):
    """(delta f64 [Fa], s int64 [Fa]) of a lane's whole source under the paced pattern; empty arrays when either side has
    no frames."""
    a, b = np.asarray(source, dtype=np.float64), np.asarray(target, dtype=np.float64)
    if a.shape[0] == 0 or b.shape[0] == 0:
        return np.zeros(0), np.zeros(0, dtype=np.int64)
    return paced_ref.profile(a, b, squared)


def watch(source, target, cuts, max_cost=None, squared=False, flush_after=()):
    """watch_ref.drive() on the paced profile of (source, target)."""
    delta, s = whole_profile(source, target, squared)
    return watch_ref.drive(delta, s, cuts, max_cost, flush_after)


def planted(seed=0x9ACED):
    """The three planted copies of the definition's examples: (lane [400][13], targets of 9, 11 and 10 frames, the spans
    they must be reported at).  Target 0 is every second frame of lane frames 50 ... 66 (a span of 2 Fb - 1), target 1 is
    lane frames 120 ... 130 as they are, target 2 is lane frames 300 ... 304 with each frame doubled (a span of Fb / 2)."""
    rng = np.random.default_rng(seed)
    lane = rng.standard_normal((400, 13)).astype(np.float32).astype(np.float64)
    targets = [lane[50:67:2].copy(), lane[120:131].copy(), np.repeat(lane[300:305], 2, axis=0)]
    return lane, targets, [(0.0, 50, 66), (0.0, 120, 130), (0.0, 300, 304)]


def nan_case(seed=0x9A9):
    """(lane [400][13] with a NaN in frame 100 and a copy of the target at 120 ... 130, the 11-frame target)."""
    rng = np.random.default_rng(seed)
    lane = rng.standard_normal((400, 13)).astype(np.float32).astype(np.float64)
    target = rng.standard_normal((11, 13)).astype(np.float32).astype(np.float64)
    lane[120:131] = target
    lane[100, 4] = np.nan
    return lane, target
