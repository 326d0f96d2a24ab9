#!/usr/bin/env python3
"""tools/warp_timing.py -- the ssym_reconstruct_warped kernel against the ssym_reconstruct kernel for the same targets
(LAB.md 5.13).

For each shape a dictionary of 512 sounds is matched by 4096 targets (ssym_match_queries) and the matched pairs are
aligned with the outputs left on the device (ssym_dtw_align, SSYM_OUT_DEVICE).  Every sound carries frames x 256 samples.
Then, in the same run and for the same indices and output offsets:
  * ssym_reconstruct's gather kernel and ssym_reconstruct_warped's synthesis kernel, both as ssym_get_timings reports
    them (device time between two events around the one launch), median of --reps calls after a warm-up call, outputs
    left on the device for the warp and copied back for the gather (the events do not see the copies);
  * the rate both reach counted as 16 bytes per output sample (one f64 read, one f64 written: the gather's traffic; the
    warp reads up to four taps per sample, three of them from lines a neighbouring wave has just fetched);
  * the three-call chain match + align + warp against match + align alone: a host clock around the calls, each of which
    ends in its own synchronisation, outputs left on the device.

    python tools/warp_timing.py [--reps 9]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from soundsym_amd import Engine, synth  # noqa: E402
from soundsym_amd import _native as nat  # noqa: E402
from soundsym_amd.api import HOP  # noqa: E402
from soundsym_amd.engine import pack_segments  # noqa: E402


def median_of(fn, reps):
    fn()
    vals = [fn() for _ in range(reps)]
    return float(np.median(vals))


def shape(name, src, tgt, dim, reps):
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
    frames = t_frames.astype(np.uint32)
    dout = torch.empty(total, dtype=torch.float64, device="cuda")
    L = nat.lib()

    def match_align():
        idx, _ = e.match(d, q)
        return (idx,) + e.dtw_align_device(d, q, idx)

    def warp(idx, lengths, maps, m_off):
        nat.check(L.ssym_reconstruct_warped(e.ctx, smp.ptr, idx.ctypes.data, out_off.ctypes.data, n, maps.data_ptr(),
                                            m_off.ctypes.data, frames.ctypes.data, lengths.data_ptr(),
                                            nat.WARP_MAP_DEVICE | nat.OUT_DEVICE, dout.data_ptr(), None), e.ctx)

    idx, _, lengths, _, maps, _, m_off = match_align()

    def warp_kernel():
        warp(idx, lengths, maps, m_off)
        return e.timings()["main_ms"]

    def gather_kernel():
        e.reconstruct(smp, idx, out_off)
        return e.timings()["main_ms"]

    def chain(with_warp):
        def run():
            t0 = time.perf_counter()
            i, _, ln, _, mp, _, mo = match_align()
            if with_warp:
                warp(i, ln, mp, mo)
            return 1e3 * (time.perf_counter() - t0)
        return run

    # alternate the two kernels so that both see the same machine
    ms_w, ms_g = [], []
    warp_kernel(), gather_kernel()
    for _ in range(reps):
        ms_w.append(warp_kernel())
        ms_g.append(gather_kernel())
    ms_w, ms_g = float(np.median(ms_w)), float(np.median(ms_g))
    ms_ma = median_of(chain(False), reps)
    ms_maw = median_of(chain(True), reps)
    valid = int(np.count_nonzero(lengths.cpu().numpy()))
    nominal = 16.0 * total
    print(f"{name:24s} {n} targets, {total} samples, {valid} with a path  |  gather kernel {ms_g:7.3f} ms "
          f"({nominal / ms_g / 1e9:6.2f} TB/s)  warp kernel {ms_w:7.3f} ms ({nominal / ms_w / 1e9:6.2f} TB/s at 16 B/sample, "
          f"{nominal / 2 / ms_w / 1e9:5.2f} TB/s written)"
          f"  ratio {ms_w / ms_g:5.2f}  |  match + align {ms_ma:8.3f} ms, + warp {ms_maw:8.3f} ms "
          f"(+{ms_maw - ms_ma:7.3f})", flush=True)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    g = synth.make_grid(512, 4096, 128, 13, 0x5EED0003)
    shape("128 f x 13 d", list(g.sources), list(g.targets), 13, args.reps)
    src, tgt, _ = synth.make_ragged(512, 4096, 5, 40, 12, 0x5EED0041, planted=True)
    shape("ragged 5..40 f x 12 d", src, tgt, 12, args.reps)


if __name__ == "__main__":
    main()
