#!/usr/bin/env python3
"""tools/span_timing.py -- spot -> warp on the resident dictionary against spot -> cut -> warp on a second one (DESIGN.md
5.22, LAB.md 5.22).

Two routes through the public interface, on one GPU, for the same recordings and targets:
  * cut:   spots = dictionary.spot(targets); dictionary.cut(spots).warp(targets, indices=arange) -- one Python Sound per
           spot, a second dictionary and a second sample store packed and uploaded, then ssym_dtw_align and
           ssym_reconstruct_warped on them (what examples/spot.py did before spans);
  * spans: spots = dictionary.spot(targets); dictionary.warp(targets, spans=spots) -- ssym_dtw_align_spans and
           ssym_reconstruct_warped_spans on the dictionary and the samples that are resident already.
Two shapes: 4 recordings of 16 384 frames against 1024 ragged targets of 5 ... 40 frames, and against 4096 targets of 128
frames.  Every target is a stretch of a recording with noise on it, so the spans have about the targets' lengths.  Per
route and shape: the host clock around the whole flow and, per library call, the host clock and ssym_get_timings'
total_ms, all as the median of --runs flows after --warmup; the bytes the cut route uploads that the span route does not;
and whether the two routes gave the same samples.

    python tools/span_timing.py [--runs 10] [--warmup 3] [--search 0] [--paced]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from soundsym_amd import Engine, Sound, SoundDictionary  # noqa: E402
from soundsym_amd.api import HOP, NCOEFFS  # noqa: E402

TIMED = ("dictionary", "samples", "queries", "spot_queries", "dtw_align_device", "reconstruct_warped", "reconstruct_wsola")


class TimedEngine(Engine):
    """An Engine that keeps, per call of the methods a flow goes through, the host time and the library's own total_ms."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.log = []


def _timed(name):
    inner = getattr(Engine, name)

    def call(self, *a, **kw):
        t0 = time.perf_counter()
        out = inner(self, *a, **kw)
        host = (time.perf_counter() - t0) * 1e3
        own = self.timings()["total_ms"] if name in ("spot_queries", "reconstruct_warped", "reconstruct_wsola") else 0.0
        self.log.append((name, host, own))
        return out
    return call


for _name in TIMED:
    setattr(TimedEngine, _name, _timed(_name))


def make(shape, rng):
    recs = [rng.normal(size=(16384, NCOEFFS)) * (4.0 / (1.0 + np.arange(NCOEFFS))) for _ in range(4)]
    lengths = rng.integers(5, 41, size=1024) if shape == "ragged" else np.full(4096, 128)
    sounds = [Sound(rng.uniform(-0.5, 0.5, size=r.shape[0] * HOP + 768), 44100.0, r.reshape(-1), "rec%d" % k)
              for k, r in enumerate(recs)]
    targets = []
    for n in lengths:
        r = recs[int(rng.integers(0, 4))]
        at = int(rng.integers(0, r.shape[0] - int(n)))
        feats = r[at:at + int(n)] + rng.normal(size=(int(n), NCOEFFS)) * 0.05
        targets.append(Sound(rng.uniform(-0.5, 0.5, size=int(n) * HOP), 44100.0, feats.reshape(-1)))
    return sounds, targets


def flow(route, d, targets, kw):
    spots = d.spot(targets, **({"step": kw["step"]} if kw["step"] != "symmetric" else {}))
    if route == "cut":
        return spots, d.cut(spots).warp(targets, indices=np.arange(len(targets)), **kw)
    return spots, d.warp(targets, spans=spots, **kw)


def run(shape, args):
    rng = np.random.default_rng(0x59A2)
    sounds, targets = make(shape, rng)
    e = TimedEngine(metric="dtw", dtype="f64")
    d = SoundDictionary(engine=e)
    d.sounds = sounds
    kw = dict(search=args.search, step="paced" if args.paced else "symmetric")
    result = {"shape": shape, "targets": len(targets), "runs": args.runs, "warmup": args.warmup, **kw}
    outs = {}
    for route in ("cut", "spans"):
        walls, calls = [], {}
        for k in range(args.warmup + args.runs):
            e.log.clear()
            t0 = time.perf_counter()
            spots, outs[route] = flow(route, d, targets, kw)
            wall = (time.perf_counter() - t0) * 1e3
            if k < args.warmup:
                continue
            walls.append(wall)
            seen = {}
            for name, host, own in e.log:
                n = seen[name] = seen.get(name, 0) + 1
                calls.setdefault("%s#%d" % (name, n), []).append((host, own))
        result[route] = {"wall_ms": float(np.median(walls)), "wall_min_max": [float(min(walls)), float(max(walls))],
                         "calls": {k: {"host_ms": float(np.median([h for h, _ in v])), "total_ms": float(np.median([o for _, o in v]))}
                                   for k, v in calls.items()}}
    frames = sum(sp.num_frames() for sp in spots)
    samples = sum(b - a for a, b in (sp.sample_span(sounds[sp.source_index].samples().size) for sp in spots if sp))
    result["spotted"] = sum(1 for sp in spots if sp)
    result["span_frames_mean"] = frames / max(len(spots), 1)
    result["bytes_not_uploaded"] = int(samples * 8 + frames * NCOEFFS * 8)
    result["same_samples"] = bool(np.array_equal(np.asarray(outs["cut"]).view(np.uint64), np.asarray(outs["spans"]).view(np.uint64)))
    result["spans_over_cut"] = result["spans"]["wall_ms"] / result["cut"]["wall_ms"]
    e.close()
    return result


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--search", type=int, default=0)
    ap.add_argument("--paced", action="store_true")
    ap.add_argument("--shapes", default="ragged,128")
    args = ap.parse_args(argv)
    for shape in args.shapes.split(","):
        print(json.dumps(run(shape, args)), flush=True)


if __name__ == "__main__":
    main()
