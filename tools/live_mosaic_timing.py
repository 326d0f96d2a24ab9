#!/usr/bin/env python3
"""tools/live_mosaic_timing.py -- the mosaicker (ssym_mosaicker_*) against the offline mosaic of the same target (DESIGN.md
5.26, LAB.md).

    one recording of 16 384 source frames x 13 values, targets of --frames (4096) frames.

    (a) real time  a push of 16 frames carries 16 x 256 / 44 100 s = 92.9 ms of audio: ms per push of 16 frames on 1 lane and
                   on 16 lanes (16 different targets), the median over the pushes after the first --warmup, and the largest
                   n - committed over the stream.
    (b) long       one target through SoundDictionary.mosaic_long(block_frames=--block (4096)) -- the method itself, from
                   the Sound to the Mosaic: it creates and closes its mosaicker, converts the features, copies every
                   block's frames to the host and cuts the pieces -- against ONE ssym_dtw_mosaic call (Engine.dtw_mosaic) on
                   the same cells in the same process; and, beside it, the C calls alone: the same target pushed --block
                   frames at a time into a one-lane mosaicker that exists already, and flushed.  The frames of both must be
                   the offline mosaic's, bit for bit.
    (c) split      the device time of (b) and of (a)'s pushes: forward (main_ms) against commit + emission (reduce_ms), from
                   ssym_get_timings.

One MI355X, one process.  A host clock around each call, which ends in its own synchronisation.

    python tools/live_mosaic_timing.py [--reps 5] [--warmup 2] [--frames 4096] [--block 4096] [--penalty 1] [--stream 512]
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
from soundsym_amd.engine import pack_segments  # noqa: E402

AUDIO_MS_PER_FRAME = 256.0 / 44100.0 * 1e3
REC_FRAMES = 16384


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return 1e3 * (time.perf_counter() - t0), out


def stream_pass(e, mk, targets, P):
    """Every lane's target pushed P frames at a time, then flushed: per-push host ms, device ms (main, reduce), the largest
    n - committed, and lane 0's frames (src, frame, cost, start)."""
    lanes, T = len(targets), targets[0].shape[0]
    for l in range(lanes):
        mk.reset(l)
    host, main, reduce_, lag, parts = [], [], [], 0, []
    off = np.arange(lanes + 1, dtype=np.uint64)

    def take():
        lane, _, src, frame, cost, start = mk.frames()
        keep = lane == 0
        parts.append((src[keep], frame[keep], cost[keep], start[keep]))
    for at in range(0, T, P):
        m = min(P, T - at)
        block = np.concatenate([x[at:at + m] for x in targets]).astype(np.float64)
        t, n = timed(lambda: mk.push(block, off * m))
        tm = e.timings()
        host.append(t)
        main.append(tm["main_ms"])
        reduce_.append(tm["reduce_ms"])
        if n:
            take()
        lag = max(lag, int((at + m - mk.best()[2].astype(np.int64)).max()))
    flush_ms = 0.0
    for l in range(lanes):
        t, n = timed(lambda: mk.flush(l))
        flush_ms += t
        if n and l == 0:
            take()
    frames = tuple(np.concatenate(x) for x in zip(*parts)) if parts else None
    return np.array(host), np.array(main), np.array(reduce_), flush_ms, lag, frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--block", type=int, default=4096)
    ap.add_argument("--stream", type=int, default=512, help="frames per lane of the real-time pass")
    ap.add_argument("--penalty", type=float, default=1.0)
    args = ap.parse_args()
    rng = np.random.default_rng(0x5EED0C26)
    mkf = lambda f: rng.standard_normal((f, 13)).astype(np.float32)
    rec = mkf(REC_FRAMES)
    targets = [mkf(args.frames) for _ in range(16)]
    for k, t in enumerate(targets):                       # spans of the recording, so that pieces form
        for a in range(0, args.frames - 64, 256):
            t[a:a + 64] = rec[(977 * (a + k)) % (REC_FRAMES - 64):][:64]
    e = Engine(metric="dtw", dtype="f32")
    d = e.dictionary(*pack_segments([rec], 13, np.float32), 13)
    mk1, mk16 = e.mosaicker(d, 1, args.penalty), e.mosaicker(d, 16, args.penalty)

    # (b), (c): the long target -- offline, mosaic_long itself and the mosaicker's calls alone, taking turns
    q = e.queries(*pack_segments(targets[:1], 13, np.float32), 13)
    sound = lambda x: Sound(np.zeros(1024 + 256 * (x.shape[0] - 1)), 44100.0, x.astype(np.float64).reshape(-1), ncoeffs=13)
    sd = SoundDictionary(engine=e)
    sd.sounds = [sound(rec)]
    target = sound(targets[0])
    off_ms, long_ms, live_ms, fwd, com = [], [], [], [], []
    same = True
    for rep in range(args.warmup + args.reps):
        t, out = timed(lambda: e.dtw_mosaic(d, q, args.penalty))
        t_long, mosaic = timed(lambda: sd.mosaic_long(target, args.penalty, args.block))
        host, main_, red, flush_ms, lag, frames = stream_pass(e, mk1, targets[:1], args.block)
        if rep >= args.warmup:
            off_ms.append(t)
            long_ms.append(t_long)
            live_ms.append(float(host.sum() + flush_ms))
            fwd.append(float(main_.sum()))
            com.append(float(red.sum()))
        count = int(out[0][0])
        src, frame, cost, start = frames
        same = same and (np.flatnonzero(start).tolist() == out[2][:count].tolist() and src.tolist() == out[3].tolist() and
                         frame.tolist() == out[4].tolist() and cost.tobytes() == out[5].tobytes())
        same = same and (mosaic.frame_costs.tobytes() == out[5].tobytes() and
                         [p.start_frame for p in mosaic.pieces] == out[2][:count].tolist() and
                         np.float64(mosaic.total).tobytes() == np.float64(out[1][0]).tobytes())
    q.close()
    sd.invalidate()
    row = dict(long=True, frames=args.frames, block=args.block, source_frames=REC_FRAMES, offline_ms=float(np.median(off_ms)),
               offline_ms_min=float(min(off_ms)), offline_ms_max=float(max(off_ms)),
               mosaic_long_ms=float(np.median(long_ms)), mosaic_long_ms_min=float(min(long_ms)),
               mosaic_long_ms_max=float(max(long_ms)), mosaic_long_over_offline=float(np.median(long_ms) / np.median(off_ms)),
               live_ms=float(np.median(live_ms)),
               live_ms_min=float(min(live_ms)), live_ms_max=float(max(live_ms)),
               live_over_offline=float(np.median(live_ms) / np.median(off_ms)), device_forward_ms=float(np.median(fwd)),
               device_commit_ms=float(np.median(com)), commit_share=float(np.median(com) / (np.median(fwd) + np.median(com))),
               latency_frames=lag, same_as_offline=bool(same))
    print(json.dumps(row), flush=True)
    if not same:
        raise SystemExit("the live mosaic differs from the offline mosaic")

    # (a), (c): pushes of 16 frames
    for lanes, mk in ((1, mk1), (16, mk16)):
        host, main_, red, _, lag, _ = stream_pass(e, mk, [t[:args.stream] for t in targets[:lanes]], 16)
        st = host[args.warmup:]
        print(json.dumps(dict(real_time=True, lanes=lanes, push_frames=16, pushes=int(host.size),
                              audio_ms_per_push=16 * AUDIO_MS_PER_FRAME, ms_per_push_median=float(np.median(st)),
                              ms_per_push_min=float(st.min()), ms_per_push_max=float(st.max()),
                              device_forward_ms_per_push=float(np.median(main_[args.warmup:])),
                              device_commit_ms_per_push=float(np.median(red[args.warmup:])),
                              holds=bool(st.max() < 16 * AUDIO_MS_PER_FRAME), latency_frames=lag, ring_columns=mk.counts()[1])),
              flush=True)
    for h in (mk1, mk16, d):
        h.close()
    e.close()


if __name__ == "__main__":
    main()
