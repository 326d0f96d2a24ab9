#!/usr/bin/env python3
"""tools/live_follow_timing.py -- the live envelope follower (ssym_follower_*) behind the mosaicker and the resynthesiser,
against the two alone and against ssym_follow_envelope on the finished samples (LAB.md).

    tools/live_resynth_timing.py's shape: one recording of 16 384 source frames x 13 values with 256 samples per frame,
    targets of --frames (4096) frames, ssym_mosaicker_push of 16 host frames per lane and push.

    (a) per push   a push of 16 frames carries 92.9 ms of audio.  On 1 lane and on 16 lanes, search 0 and 256, the median of
                   --reps (10) pushes after --warmup (3), one process: push + ssym_resynth_take + ssym_resynth_samples (the
                   parent's figure, measured here again) and the same with ssym_follower_push of what that released beside
                   the target's own samples + ssym_follower_samples (f64, pcm and gains to the host) behind it; the
                   follower's device time split into the gain kernel (main_ms) and append + apply (reduce_ms).
    (b) whole      the 4096-frame target on one lane: the 256 live follower calls and the flush (push + samples each) against
                   one ssym_follow_envelope on the finished resynthesis in the same session.  The two must give the same
                   samples and gains, bit for bit; the tool stops if they do not.

One MI355X, one process.  A host clock around each call, which ends in its own synchronisation.

    python tools/live_follow_timing.py [--reps 10] [--warmup 3] [--frames 4096] [--penalty 1] [--max-gain 8]
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

AUDIO_MS_PER_FRAME = 256.0 / 44100.0 * 1e3
REC_FRAMES = 16384
PUSH = 16


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return 1e3 * (time.perf_counter() - t0), out


def offsets(parts):
    return np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)


def live_pass(e, mk, rs, fl, targets, refs, flush=False):
    """Every lane's target pushed 16 frames at a time, every frame log taken and its samples copied out; with a follower what
    that released goes into it beside the lane's own samples, and its logs are copied out.  Per push: host ms of push + take
    + samples, of the follower's push + samples, its device ms (main, reduce); with flush the ends, and lane 0's resynthesis,
    followed samples and gains from reset to flush."""
    lanes, T = len(targets), targets[0].shape[0]
    for l in range(lanes):
        mk.reset(l)
        rs.reset(l)
        if fl is not None:
            fl.reset(l)
    off = np.arange(lanes + 1, dtype=np.uint64)
    base, follow, main, red, settled = [], [], [], [], []
    at_ref = [0] * lanes
    y0, out0, g0 = [], [], []

    def resynth(call):
        def both():
            call()
            return rs.samples(want_pcm32=True)
        t, (o, s, _) = timed(both)
        return t, [s[int(a):int(b)] for a, b in zip(o[:-1], o[1:])]

    def followed(parts, end_lane=None):
        xs = [r[a:a + p.size] for r, a, p in zip(refs, at_ref, parts)]

        def both():
            if end_lane is None:
                fl.push(np.concatenate(parts), offsets(parts), np.concatenate(xs), offsets(xs))
            else:
                fl.flush(end_lane)
            tm = e.timings()
            return tm, fl.samples(want_pcm32=True, want_gains=True)
        t, (tm, (o, s, _, go, g)) = timed(both)
        for l, p in enumerate(parts):
            at_ref[l] += p.size
        out0.append(s[int(o[0]):int(o[1])]), g0.append(g[int(go[0]):int(go[1])])
        return t, tm

    for at in range(0, T, PUSH):
        m = min(PUSH, T - at)
        block = np.concatenate([x[at:at + m] for x in targets]).astype(np.float64)
        t_push, _ = timed(lambda: mk.push(block, off * m))
        t, parts = resynth(lambda: rs.take(mk))
        base.append(t_push + t)
        y0.append(parts[0])
        if fl is not None:
            t, tm = followed(parts)
            follow.append(t), main.append(tm["main_ms"]), red.append(tm["reduce_ms"]), settled.append(tm["n_pairs"])
    end_ms = 0.0
    if flush:
        none = [np.zeros(0)] * lanes
        for l in range(lanes):
            mk.flush(l)
            _, parts = resynth(lambda: rs.take(mk))
            _, tail = resynth(lambda: rs.flush(l, refs[l].size))
            parts = [np.concatenate([a, b]) for a, b in zip(parts, tail)]
            y0.append(parts[0])
            if fl is not None:
                t, _ = followed(parts)
                end_ms += t
                t, _ = followed(none, end_lane=l)
                end_ms += t
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0)      # noqa: E731
    return dict(base=np.array(base), follow=np.array(follow), main=np.array(main), reduce=np.array(red), settled=np.array(settled),
                end_ms=end_ms, y=cat(y0), out=cat(out0), gains=cat(g0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--penalty", type=float, default=1.0)
    ap.add_argument("--max-gain", type=float, default=8.0)
    args = ap.parse_args()
    rng = np.random.default_rng(0x5EED0C29)
    mkf = lambda f: rng.standard_normal((f, 13)).astype(np.float32)      # noqa: E731
    rec = mkf(REC_FRAMES)
    targets = [mkf(args.frames) for _ in range(16)]
    for k, t in enumerate(targets):                       # spans of the recording, so that pieces form
        for a in range(0, args.frames - 64, 256):
            t[a:a + 64] = rec[(977 * (a + k)) % (REC_FRAMES - 64):][:64]
    n_samples = lambda frames: 1024 + 256 * (frames - 1)      # noqa: E731
    e = Engine(metric="dtw", dtype="f32")
    sd = SoundDictionary(engine=e)
    sd.sounds = [Sound(rng.uniform(-1, 1, size=n_samples(REC_FRAMES)), 44100.0, rec.astype(np.float64).reshape(-1), ncoeffs=13)]
    refs = [0.3 * rng.uniform(-1, 1, size=n_samples(args.frames)) * (1.0 + 0.5 * np.sin(np.arange(n_samples(args.frames)) / 5000.0 + k))
            for k in range(16)]                            # the targets' own samples: another level, moving
    d, store = sd.resident(), sd.resident_samples()
    short = args.warmup + args.reps
    med = lambda a: float(np.median(a))      # noqa: E731

    # (a) per push
    for lanes in (1, 16):
        mk = e.mosaicker(d, lanes, args.penalty)
        heads = [t[:short * PUSH] for t in targets[:lanes]]
        for search in (0, 256):
            rs, fl = e.resynth(store, lanes, search), e.follower(lanes, args.max_gain)
            alone = live_pass(e, mk, rs, None, heads, refs[:lanes])["base"][args.warmup:]
            r = live_pass(e, mk, rs, fl, heads, refs[:lanes])
            w = args.warmup
            both = (r["base"] + r["follow"])[w:]
            print(json.dumps(dict(
                per_push=True, lanes=lanes, search=search, push_frames=PUSH, pushes=int(alone.size),
                audio_ms_per_push=PUSH * AUDIO_MS_PER_FRAME, push_take_samples_ms=med(alone), ms_min=float(alone.min()),
                ms_max=float(alone.max()), with_follower_ms=med(both), with_follower_ms_min=float(both.min()),
                with_follower_ms_max=float(both.max()), follower_push_samples_ms=med(r["follow"][w:]),
                follower_share=med(r["follow"][w:]) / max(med(both), 1e-9), over_without=med(both) / max(med(alone), 1e-9),
                device_gain_ms=med(r["main"][w:]), device_append_apply_ms=med(r["reduce"][w:]),
                boundaries_per_push=med(r["settled"][w:]))), flush=True)
            fl.close()
            rs.close()
        mk.close()

    # (b) the whole target
    mk, rs, fl = e.mosaicker(d, 1, args.penalty), e.resynth(store, 1, 0), e.follower(1, args.max_gain)
    live_ms, off_ms, dev_ms = [], [], []
    for rep in range(3):
        r = live_pass(e, mk, rs, fl, targets[:1], refs[:1], flush=True)
        n = r["y"].size
        t, (want, want_g) = timed(lambda: e.follow_envelope(r["y"], [0, n], refs[0], [0, refs[0].size], args.max_gain, want_gains=True))
        if want.tobytes() != r["out"].tobytes() or want_g.tobytes() != r["gains"].tobytes():
            raise SystemExit("the live follower differs from ssym_follow_envelope")
        if rep:
            live_ms.append(float(r["follow"].sum() + r["end_ms"]))
            dev_ms.append(float((r["main"] + r["reduce"]).sum()))
            off_ms.append(t)
    print(json.dumps(dict(whole=True, frames=args.frames, samples=int(n), calls=int(r["follow"].size) + 2,
                          live_follower_ms=med(live_ms), live_follower_device_ms=med(dev_ms), follow_envelope_ms=med(off_ms),
                          live_over_offline=med(live_ms) / med(off_ms), same_as_offline=True)), flush=True)
    fl.close()
    rs.close()
    mk.close()
    sd.invalidate()
    e.close()


if __name__ == "__main__":
    main()
