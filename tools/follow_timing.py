#!/usr/bin/env python3
"""tools/follow_timing.py -- the two kernels of ssym_follow_envelope beside ssym_reconstruct_warped's synthesis kernel on the
same samples (LAB.md E1).

The two shapes of tools/warp_timing.py: a dictionary of 512 sounds matched by 4096 targets (ssym_match_queries), the pairs
aligned with the outputs left on the device (ssym_dtw_align), every sound carrying frames x 256 samples -- 4096 targets of
128 frames, and ragged ones of 5 ... 40 frames.  The warp writes its samples into a device buffer; the follower reads that
buffer (SSYM_FOLLOW_SAMPLES_DEVICE) and the targets' own samples, resident on the device (SSYM_FOLLOW_REF_DEVICE), and writes
samples and gains back to the device (SSYM_OUT_DEVICE), as a chain of the two calls would run.  In the same run, the two
calls alternating so that both see the same machine:
  * warp_kernel as ssym_get_timings reports it after ssym_reconstruct_warped (main_ms);
  * follow_gain_kernel (main_ms), follow_apply_kernel (reduce_ms) and both (total_ms) after ssym_follow_envelope;
each the median of --reps calls after a warm-up call, device time between events around the launches.  Rates count 16 bytes
per sample for the gain kernel (y and x read once) and 16 for the apply kernel (y read, out written).

    python tools/follow_timing.py [--reps 9] [--pcm]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from soundsym_amd import Engine, synth  # noqa: E402
from soundsym_amd import _native as nat  # noqa: E402
from soundsym_amd.api import HOP  # noqa: E402
from soundsym_amd.engine import follow_boundaries, pack_segments  # noqa: E402


def shape(name, src, tgt, dim, reps, with_pcm):
    import torch
    rng = np.random.default_rng(0x3A9)
    e = Engine(metric="dtw", dtype="f32")
    sf, so = pack_segments(src, dim, np.float32)
    tf, to = pack_segments(tgt, dim, np.float32)
    d, q = e.dictionary(sf, so, dim), e.queries(tf, to, dim)
    n = len(tgt)
    s_frames = np.diff(so.astype(np.int64))
    t_frames = np.diff(to.astype(np.int64))
    s_off = np.concatenate([[0], np.cumsum(s_frames * HOP)]).astype(np.uint64)
    out_off = np.concatenate([[0], np.cumsum(t_frames * HOP)]).astype(np.uint64)
    smp = e.samples(rng.uniform(-1, 1, size=int(s_off[-1])), s_off)
    total = int(out_off[-1])
    n_gains = int(follow_boundaries(out_off)[-1])
    frames = t_frames.astype(np.uint32)
    # the targets' own samples: another level in every target, moving inside it
    level = np.repeat(np.exp(rng.uniform(-3.0, 1.0, size=n)), t_frames * HOP) * (1.0 + 0.8 * np.sin(np.arange(total) / 977.0))
    ref = torch.from_numpy(rng.uniform(-1, 1, size=total) * level).cuda()
    warped = torch.empty(total, dtype=torch.float64, device="cuda")
    out = torch.empty(total, dtype=torch.float64, device="cuda")
    pcm = torch.empty(total, dtype=torch.int32, device="cuda") if with_pcm else None
    gains = torch.empty(n_gains, dtype=torch.float64, device="cuda")
    L = nat.lib()
    idx, _ = e.match(d, q)
    _, lengths, _, maps, _, m_off = e.dtw_align_device(d, q, idx)

    def warp_kernel():
        nat.check(L.ssym_reconstruct_warped(e.ctx, smp.ptr, idx.ctypes.data, out_off.ctypes.data, n, maps.data_ptr(),
                                            m_off.ctypes.data, frames.ctypes.data, lengths.data_ptr(),
                                            nat.WARP_MAP_DEVICE | nat.OUT_DEVICE, warped.data_ptr(), None), e.ctx)
        return e.timings()["main_ms"]

    def follow_kernels():
        nat.check(L.ssym_follow_envelope(e.ctx, warped.data_ptr(), out_off.ctypes.data, n, ref.data_ptr(), out_off.ctypes.data, 8.0,
                                         nat.FOLLOW_SAMPLES_DEVICE | nat.FOLLOW_REF_DEVICE | nat.OUT_DEVICE, out.data_ptr(),
                                         pcm.data_ptr() if with_pcm else None, gains.data_ptr()), e.ctx)
        tm = e.timings()
        return tm["main_ms"], tm["reduce_ms"], tm["total_ms"]

    warp_kernel(), follow_kernels()
    ms_w, ms_f = [], []
    for _ in range(reps):
        ms_w.append(warp_kernel())
        ms_f.append(follow_kernels())
    ms_w = float(np.median(ms_w))
    ms_g, ms_a, ms_t = (float(v) for v in np.median(np.array(ms_f), axis=0))
    clipped = float((gains == 8.0).double().mean().item())
    nominal = 16.0 * total
    print(f"{name:24s} {n} targets, {total} samples, {n_gains} gains ({100 * clipped:.1f}% at max_gain)"
          f"{', pcm' if with_pcm else ''}  |  warp kernel {ms_w:7.3f} ms  |  gain kernel {ms_g:7.3f} ms "
          f"({nominal / ms_g / 1e9:5.2f} TB/s)  apply kernel {ms_a:7.3f} ms ({nominal / ms_a / 1e9:5.2f} TB/s)  both {ms_t:7.3f} ms"
          f"  |  follow / warp {ms_t / ms_w:5.2f} (gain {ms_g / ms_w:4.2f}, apply {ms_a / ms_w:4.2f})", flush=True)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--pcm", action="store_true", help="also write out_pcm32")
    args = ap.parse_args()
    g = synth.make_grid(512, 4096, 128, 13, 0x5EED0003)
    shape("128 f x 13 d", list(g.sources), list(g.targets), 13, args.reps, args.pcm)
    src, tgt, _ = synth.make_ragged(512, 4096, 5, 40, 12, 0x5EED0041, planted=True)
    shape("ragged 5..40 f x 12 d", src, tgt, 12, args.reps, args.pcm)


if __name__ == "__main__":
    main()
