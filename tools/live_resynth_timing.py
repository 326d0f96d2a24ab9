#!/usr/bin/env python3
"""tools/live_resynth_timing.py -- the resynthesiser (ssym_resynth_*) behind the mosaicker, against the mosaicker alone and
against the offline resynthesis of the finished mosaic (LAB.md).

    one recording of 16 384 source frames x 13 values with 256 samples per frame, targets of --frames (4096) frames:
    tools/live_mosaic_timing.py's shape, and its feed -- ssym_mosaicker_push of host frames (a follow differs by the upload of
    16 x 13 values per lane).

    (a) per push   a push of 16 frames carries 92.9 ms of audio.  On 1 lane and on 16 lanes, the median of --reps (10) pushes
                   after --warmup (3), one process: the mosaicker's push alone (the parent's figure, measured here again), and
                   push + ssym_resynth_take + ssym_resynth_samples (f64 and pcm to the host) for search 0 and 256, with the
                   device time of the take split into search (main_ms) and staging + synthesis (reduce_ms).
    (b) whole      the 4096-frame target on one lane in pushes of 16 frames: the sum of the live calls (take + samples + the
                   flush; and with the mosaicker's pushes) against SoundDictionary.reconstruct_mosaic on the finished mosaic.
                   The two must give the same samples, bit for bit.

One MI355X, one process.  A host clock around each call, which ends in its own synchronisation.

    python tools/live_resynth_timing.py [--reps 10] [--warmup 3] [--frames 4096] [--penalty 1]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from soundsym_amd import HOP, Engine, Sound, SoundDictionary  # noqa: E402
from soundsym_amd.api import Mosaic, _mosaic_tiles  # noqa: E402

AUDIO_MS_PER_FRAME = 256.0 / 44100.0 * 1e3
REC_FRAMES = 16384
PUSH = 16


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return 1e3 * (time.perf_counter() - t0), out


def live_pass(e, mk, rs, targets, total_samples=None):
    """Every lane's target pushed 16 frames at a time; with a resynthesiser every log is taken and its samples copied out.
    Per push: host ms of the push, of take + samples, the take's device ms (main, reduce), the hops held; and with
    total_samples the flushes, lane 0's frames and its samples from reset to flush."""
    lanes, T = len(targets), targets[0].shape[0]
    for l in range(lanes):
        mk.reset(l)
        if rs is not None:
            rs.reset(l)
    off = np.arange(lanes + 1, dtype=np.uint64)
    push_ms, audio_ms, main, red, held, rows, smp, pcm = [], [], [], [], 0, [], [], []

    def audio():
        def call():
            rs.take(mk)
            return rs.samples(want_pcm32=True)
        t, (o, s, p) = timed(call)
        tm = e.timings()
        smp.append(s[int(o[0]):int(o[1])]), pcm.append(p[int(o[0]):int(o[1])])
        return t, tm["main_ms"], tm["reduce_ms"]

    for at in range(0, T, PUSH):
        m = min(PUSH, T - at)
        block = np.concatenate([x[at:at + m] for x in targets]).astype(np.float64)
        t, n = timed(lambda: mk.push(block, off * m))
        push_ms.append(t)
        if total_samples is not None and n:
            lane = mk.frames()
            rows.append([a[lane[0] == 0] for a in lane])
        if rs is not None:
            t, a, b = audio()
            audio_ms.append(t), main.append(a), red.append(b)
            frames, released = rs.counts()
            held = max(held, int((frames.astype(np.int64) - released.astype(np.int64) // HOP).max()))
    end_ms = 0.0
    if total_samples is not None:
        for l in range(lanes):
            t, n = timed(lambda: mk.flush(l))
            push_ms.append(t)
            if n and l == 0:
                lane = mk.frames()
                rows.append([a[lane[0] == 0] for a in lane])
            t, _, _ = audio()
            end_ms += t

            def end():
                rs.flush(l, total_samples)
                return rs.samples(want_pcm32=True)
            t, (o, s, p) = timed(end)
            end_ms += t
            if l == 0:
                smp.append(s), pcm.append(p)
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dtype=dt)
    frames0 = [np.concatenate([r[k] for r in rows]) for k in range(6)] if rows else None
    return dict(push=np.array(push_ms), audio=np.array(audio_ms), main=np.array(main), reduce=np.array(red), held=held,
                end_ms=end_ms, frames=frames0, samples=cat(smp, np.float64), pcm=cat(pcm, np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--penalty", type=float, default=1.0)
    args = ap.parse_args()
    rng = np.random.default_rng(0x5EED0C27)
    mkf = lambda f: rng.standard_normal((f, 13)).astype(np.float32)
    rec = mkf(REC_FRAMES)
    targets = [mkf(args.frames) for _ in range(16)]
    for k, t in enumerate(targets):                       # spans of the recording, so that pieces form
        for a in range(0, args.frames - 64, 256):
            t[a:a + 64] = rec[(977 * (a + k)) % (REC_FRAMES - 64):][:64]
    n_samples = lambda frames: 1024 + 256 * (frames - 1)
    e = Engine(metric="dtw", dtype="f32")
    sd = SoundDictionary(engine=e)
    sd.sounds = [Sound(rng.uniform(-1, 1, size=n_samples(REC_FRAMES)), 44100.0, rec.astype(np.float64).reshape(-1), ncoeffs=13)]
    target = Sound(rng.uniform(-1, 1, size=n_samples(args.frames)), 44100.0, targets[0].astype(np.float64).reshape(-1), ncoeffs=13)
    d, store = sd.resident(), sd.resident_samples()
    short = args.warmup + args.reps

    # (a) per push
    for lanes in (1, 16):
        mk = e.mosaicker(d, lanes, args.penalty)
        heads = [t[:short * PUSH] for t in targets[:lanes]]
        alone = live_pass(e, mk, None, heads)["push"][args.warmup:]
        row = dict(per_push=True, lanes=lanes, push_frames=PUSH, pushes=int(alone.size), audio_ms_per_push=PUSH * AUDIO_MS_PER_FRAME,
                   push_alone_ms=float(np.median(alone)), push_alone_ms_min=float(alone.min()), push_alone_ms_max=float(alone.max()))
        for search in (0, 256):
            rs = e.resynth(store, lanes, search)
            r = live_pass(e, mk, rs, heads)
            both = (r["push"] + r["audio"])[args.warmup:]
            dev = (r["main"] + r["reduce"])[args.warmup:]
            row["search_%d" % search] = dict(
                push_take_samples_ms=float(np.median(both)), ms_min=float(both.min()), ms_max=float(both.max()),
                over_push_alone=float(np.median(both) / np.median(alone)), take_samples_ms=float(np.median(r["audio"][args.warmup:])),
                device_search_ms=float(np.median(r["main"][args.warmup:])), device_synth_ms=float(np.median(r["reduce"][args.warmup:])),
                search_share=float(np.median(r["main"][args.warmup:]) / max(np.median(dev), 1e-9)), hops_held=r["held"])
            rs.close()
        mk.close()
        print(json.dumps(row), flush=True)

    # (b) the whole target
    mk = e.mosaicker(d, 1, args.penalty)
    for search in (0, 256):
        rs = e.resynth(store, 1, search)
        live_ms, with_push_ms, off_ms, steps_ms = [], [], [], []
        same = True
        for rep in range(3):
            r = live_pass(e, mk, rs, targets[:1], target.samples().size)
            lane, col, src, frame, cost, start = r["frames"]
            mosaic = Mosaic(_mosaic_tiles(np.flatnonzero(start), src, frame, cost), 0.0, col.size, cost)
            t, out = timed(lambda: sd.reconstruct_mosaic(target, search=search, want_pcm32=True, mosaic=mosaic))
            same = same and out[1].tobytes() == r["samples"].tobytes() and out[2].tobytes() == r["pcm"].tobytes()
            if rep:
                live_ms.append(float(r["audio"].sum() + r["end_ms"]))
                with_push_ms.append(float(r["audio"].sum() + r["end_ms"] + r["push"].sum()))
                off_ms.append(t)
                steps_ms.append(float(r["main"].sum()) / max(col.size, 1))
        print(json.dumps(dict(whole=True, frames=args.frames, search=search, pushes=-(-args.frames // PUSH),
                              live_resynth_ms=float(np.median(live_ms)), live_with_pushes_ms=float(np.median(with_push_ms)),
                              reconstruct_mosaic_ms=float(np.median(off_ms)),
                              live_over_offline=float(np.median(live_ms) / np.median(off_ms)),
                              device_search_ms_per_frame=float(np.median(steps_ms)), same_as_offline=bool(same))), flush=True)
        rs.close()
        if not same:
            raise SystemExit("the live resynthesis differs from reconstruct_mosaic")
    mk.close()
    sd.invalidate()
    e.close()


if __name__ == "__main__":
    main()
