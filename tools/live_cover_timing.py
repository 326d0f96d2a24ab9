#!/usr/bin/env python3
"""tools/live_cover_timing.py -- the coverer (ssym_coverer_*) at the reference's shape against the offline cover of the same
target (LAB.md).

    4096 ragged sources of 5 ... 40 frames x 13 values (W = 80), targets of 4096 frames.

    one lane    the target pushed P frames at a time, P in --pushes (1, 16, 64, 256, 4096): ms per push (the median over the
                pushes after the first --warmup, at most --reps of them spread over the stream for P = 1), the sum over
                the stream against ONE ssym_dtw_cover call on the same target timed in the same process between the passes,
                the device time's split into forward (gather, forward, fold: main_ms) and chain + commit (reduce_ms), and
                the latency: the largest n - committed over the stream, in frames and in W.  The pieces from first push to
                flush must be the offline cover's, piece for piece and bit for bit.
    real time   a push of 16 frames carries 16 x 256 / 44 100 s = 92.9 ms of audio: ms per push of 16 frames on 1 lane and on
                16 lanes (16 different targets).

One MI355X, one process.  A host clock around each call, which ends in its own synchronisation.

    python tools/live_cover_timing.py [--reps 10] [--warmup 3] [--pushes 1,16,64,256,4096] [--frames 4096]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from soundsym_amd import Engine  # noqa: E402
from soundsym_amd.engine import pack_segments  # noqa: E402

AUDIO_MS_PER_FRAME = 256.0 / 44100.0 * 1e3


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return 1e3 * (time.perf_counter() - t0), out


def offline(e, d, target, penalty, reps, warmup):
    q = e.queries(*pack_segments([target], 13, np.float32), 13)
    for _ in range(warmup):
        e.dtw_cover(d, q, penalty)
    ts = [timed(lambda: e.dtw_cover(d, q, penalty)) for _ in range(reps)]
    q.close()
    return [t for t, _ in ts], ts[-1][1]


def stream_pass(e, cv, targets, P):
    """Every lane's target pushed P frames at a time, then flushed: per-push host ms, device ms (main, reduce), the
    largest n - committed, and the pieces of lane 0."""
    lanes, T = len(targets), targets[0].shape[0]
    for l in range(lanes):
        cv.reset(l)
    host, main, reduce_, lag, pieces = [], [], [], 0, []
    off = np.arange(lanes + 1, dtype=np.uint64)
    for at in range(0, T, P):
        m = min(P, T - at)
        block = np.concatenate([x[at:at + m] for x in targets]).astype(np.float64)
        t, n = timed(lambda: cv.push(block, off * m))
        tm = e.timings()
        host.append(t)
        main.append(tm["main_ms"])
        reduce_.append(tm["reduce_ms"])
        if n:
            lane, src, start, end, cost = cv.pieces()
            pieces += [(int(src[k]), int(start[k]), int(end[k]), float(cost[k])) for k in range(lane.size) if lane[k] == 0]
        lag = max(lag, int((at + m - cv.best()[2].astype(np.int64)).max()))
    for l in range(lanes):
        if cv.flush(l) and l == 0:
            lane, src, start, end, cost = cv.pieces()
            pieces += [(int(src[k]), int(start[k]), int(end[k]), float(cost[k])) for k in range(lane.size)]
    return np.array(host), np.array(main), np.array(reduce_), lag, pieces


def steady(x, warmup, reps, P, W):
    """The pushes that count: after the warm-up and after the tail has filled (W - 1 frames)."""
    skip = max(warmup, -(-W // P))
    x = x[skip:] if x.size > skip else x
    if x.size > reps and P == 1:
        x = x[np.linspace(0, x.size - 1, reps).astype(int)]
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pushes", default="1,16,64,256,4096")
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--penalty", type=float, default=0.0)
    args = ap.parse_args()
    rng = np.random.default_rng(0x5EED0C07)
    mk = lambda f: rng.standard_normal((f, 13)).astype(np.float32)
    src = [mk(int(f)) for f in rng.integers(5, 41, size=4096)]
    W = 2 * max(s.shape[0] for s in src)
    targets = [mk(args.frames) for _ in range(16)]
    e = Engine(metric="dtw", dtype="f32")
    d = e.dictionary(*pack_segments(src, 13, np.float32), 13)
    cv1, cv16 = e.coverer(d, 1, args.penalty), e.coverer(d, 16, args.penalty)
    off_ms = []
    for P in [int(p) for p in args.pushes.split(",")]:
        ts, out = offline(e, d, targets[0], args.penalty, args.reps, args.warmup)
        off_ms += ts
        count = int(out[0][0])
        want = [(int(out[2][k]), int(out[3][k]), int(out[4][k]), float(out[5][k])) for k in range(count)]
        host, main_, red, lag, pieces = stream_pass(e, cv1, targets[:1], P)
        same = len(pieces) == len(want) and all(
            a[:3] == b[:3] and np.float64(a[3]).view(np.uint64) == np.float64(b[3]).view(np.uint64) for a, b in zip(pieces, want))
        st = steady(host, args.warmup, args.reps, P, W)
        row = dict(lanes=1, push_frames=P, pushes=int(host.size), ms_per_push_median=float(np.median(st)), ms_per_push_min=float(st.min()),
                   ms_per_push_max=float(st.max()), stream_ms=float(host.sum()), offline_ms=float(np.median(ts)),
                   stream_over_offline=float(host.sum() / np.median(ts)), cell_model=(P + W - 1) / P,
                   forward_share=float(main_.sum() / max(main_.sum() + red.sum(), 1e-9)),
                   device_forward_ms=float(main_.sum()), device_chain_commit_ms=float(red.sum()),
                   latency_frames=lag, latency_in_w=lag / W, pieces=len(pieces), same_as_offline=bool(same))
        print(json.dumps(row), flush=True)
        if not same:
            raise SystemExit("the live cover differs from the offline cover")
    for lanes, cv in ((1, cv1), (16, cv16)):
        host, main_, red, lag, _ = stream_pass(e, cv, targets[:lanes], 16)
        st = steady(host, args.warmup, 1 << 30, 16, W)
        print(json.dumps(dict(real_time=True, lanes=lanes, push_frames=16, audio_ms_per_push=16 * AUDIO_MS_PER_FRAME,
                              ms_per_push_median=float(np.median(st)), ms_per_push_max=float(st.max()),
                              device_forward_ms_per_push=float(np.median(main_[3:])),
                              device_chain_commit_ms_per_push=float(np.median(red[3:])),
                              holds=bool(st.max() < 16 * AUDIO_MS_PER_FRAME), latency_frames=lag, latency_in_w=lag / W)), flush=True)
    print(json.dumps(dict(offline_ms_median=float(np.median(off_ms)), offline_ms_min=float(min(off_ms)),
                          offline_ms_max=float(max(off_ms)), W=W, sources=len(src), frames=args.frames)), flush=True)
    for h in (cv1, cv16, d):
        h.close()
    e.close()


if __name__ == "__main__":
    main()
