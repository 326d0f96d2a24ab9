#!/usr/bin/env python3
"""tools/align_timing.py -- ssym_dtw_align against the exact re-scoring of the same number of pairs (DESIGN.md 5.12,
LAB.md 5.12).

For each shape a dictionary of 512 sounds is matched by M targets (ssym_match_queries); the match's exact re-scoring
step (ssym_timings.refine_ms over n_refined pairs, device time between events, as tools/exact_timing.py reads it) gives
the parent's cost per re-scored pair, scaled to P pairs.  Then the P matched pairs are aligned with ssym_dtw_align, with
and without the frame map: a host clock around the call, which ends in its own synchronisation (uploads of the pair
list and offsets and the copies back included), median of --reps calls after one warm-up call.  The same with device
outputs (no copies back) is the nearest thing to the kernel's own time.  Last: one pair of 4096 x 4096 frames, and
SoundDictionary.align against match_indices alone on the recordings of BASELINE configs[0].

    python tools/align_timing.py [--reps 9] [--skip-big]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from soundsym_amd import Engine, Sound, SoundDictionary, synth  # noqa: E402
from soundsym_amd import _native as nat  # noqa: E402
from soundsym_amd.engine import pack_segments  # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), out


def device_call(e, d, q, idx, want_map):
    """ssym_dtw_align with SSYM_OUT_DEVICE outputs: returns a callable for timed()."""
    import torch
    p_off, m_off = e.dtw_align_sizes(d, q, idx)
    n = idx.size
    cost = torch.zeros(n, dtype=torch.float64, device="cuda")
    length = torch.zeros(n, dtype=torch.int32, device="cuda")
    path = torch.zeros(2 * int(p_off[-1]), dtype=torch.int32, device="cuda")
    fmap = torch.zeros(max(1, int(m_off[-1])), dtype=torch.int32, device="cuda")

    def call():
        nat.check(nat.lib().ssym_dtw_align(e.ctx, d.ptr, q.ptr, idx.ctypes.data, None, n, 0, cost.data_ptr(),
                                           length.data_ptr(), p_off.ctypes.data, path.data_ptr(), m_off.ctypes.data,
                                           fmap.data_ptr() if want_map else None, nat.OUT_DEVICE), e.ctx)
    return call


def shape(name, src, tgt, dim, band, counts, reps):
    e = Engine(metric="dtw", dtype="f32", band=band)
    sf, so = pack_segments(src, dim, np.float32)
    d = e.dictionary(sf, so, dim)
    for p in counts:
        tf, to = pack_segments(tgt[:p], dim, np.float32)
        q = e.queries(tf, to, dim)
        e.match(d, q)
        refine, nref = [], 0
        for _ in range(reps):
            idx, _ = e.match(d, q)
            tm = e.timings()
            refine.append(tm["refine_ms"])
            nref = tm["n_refined"]
        per_pair = float(np.median(refine)) / max(nref, 1)
        ms_map, out = timed(lambda: e.dtw_align(d, q, idx), reps)
        ms_nomap, _ = timed(lambda: e.dtw_align(d, q, idx, want_map=False), reps)
        ms_dev, _ = timed(device_call(e, d, q, idx, True), reps)
        ms_dev_nomap, _ = timed(device_call(e, d, q, idx, False), reps)
        rescore = per_pair * p
        print(f"{name:26s} P {p:5d}  re-score {np.median(refine):7.3f} ms / {nref:6d} pairs = {rescore:7.3f} ms for P  |  "
              f"align host {ms_map:7.3f} ms, no map {ms_nomap:7.3f}  device outputs {ms_dev:7.3f}, no map {ms_dev_nomap:7.3f}"
              f"  |  ratio (device outputs / re-score) {ms_dev / rescore if rescore else float('nan'):6.2f}"
              f"  mean L {float(np.mean(out[1])):.1f}", flush=True)
        q.close()
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--skip-big", action="store_true")
    args = ap.parse_args()
    counts = [1, 64, 512, 4096]

    g = synth.make_grid(512, 4096, 128, 13, 0x5EED0003)
    shape("128 f x 13 d", list(g.sources), list(g.targets), 13, -1, counts, args.reps)
    src, tgt, _ = synth.make_ragged(512, 4096, 5, 40, 12, 0x5EED0041, planted=True)
    shape("ragged 5..40 f x 12 d", src, tgt, 12, -1, counts, args.reps)
    g = synth.make_grid(512, 4096, 256, 40, 0x5EED0005)
    shape("256 f x 40 d, r = 32", list(g.sources), list(g.targets), 40, 32, counts, args.reps)

    if not args.skip_big:
        rng = np.random.default_rng(7)
        a = rng.standard_normal((4096, 13)).astype(np.float32)
        b = rng.standard_normal((4096, 13)).astype(np.float32)
        e = Engine(metric="dtw", dtype="f32")
        d, q = e.dictionary(a.reshape(-1), np.array([0, 4096], np.uint64), 13), e.queries(b.reshape(-1), np.array([0, 4096], np.uint64), 13)
        ms_pm, _ = timed(lambda: e.pair_matrix(d, q, exact=True), 3)
        ms, out = timed(lambda: e.dtw_align(d, q, [0]), 3)
        print(f"one pair 4096 x 4096 f x 13 d: exact cost alone (ssym_pair_matrix) {ms_pm:8.3f} ms, align {ms:8.3f} ms "
              f"(L = {int(out[1][0])}, direction matrix in global scratch)", flush=True)
        e.close()

    # the line a user sees: the recordings of configs[0] (284 x 55 segments)
    from soundsym_amd.api import HOP, frame_features
    from soundsym_amd.io import audacity_labels_to_timestamps, read_wav
    gold = os.path.join(ROOT, "tests", "golden")
    e = Engine(metric="dtw", dtype="f64")
    s_smp, srate = read_wav(os.path.join(gold, "audio", "sample.wav"))
    t_smp, rate = read_wav(os.path.join(gold, "audio", "Section_7_1.wav"))
    seg = 16 * HOP
    lens = [seg] * (s_smp.size // seg) + ([s_smp.size % seg] if s_smp.size % seg else [])
    dictionary = SoundDictionary.from_segments(Sound(s_smp, srate, frame_features(s_smp, srate, engine=e)), lens, engine=e)
    dictionary.sounds = [x for x in dictionary.sounds if x.num_frames() > 0]
    targets = []
    for a0, b0, label in audacity_labels_to_timestamps(os.path.join(gold, "vowel.txt")):
        piece = t_smp[int(round(a0 * rate)):int(round(b0 * rate)) + 1]
        if piece.size >= HOP:
            targets.append(Sound(piece, rate, frame_features(piece, rate, engine=e), label))
    ms_m, _ = timed(lambda: dictionary.match_indices(targets), args.reps)
    ms_a, al = timed(lambda: dictionary.align(targets), args.reps)
    print(f"configs[0] recordings {len(dictionary.sounds)} x {len(targets)}: match_indices {ms_m:7.3f} ms, "
          f"SoundDictionary.align (match + align) {ms_a:7.3f} ms, mean diagonal share "
          f"{float(np.mean([x.diagonal_share() for x in al])):.2f}", flush=True)
    e.close()


if __name__ == "__main__":
    main()
