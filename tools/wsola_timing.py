#!/usr/bin/env python3
"""tools/wsola_timing.py -- the two kernels of ssym_reconstruct_wsola beside ssym_reconstruct_warped's one, for the same
targets in the same run (LAB.md 5.14).

The shapes are tools/warp_timing.py's: a dictionary of 512 sounds matched by 4096 targets (ssym_match_queries), the
matched pairs aligned with the outputs left on the device (ssym_dtw_align, SSYM_OUT_DEVICE); every sound carries frames x
256 samples.  Then, for the same indices, maps and output offsets, outputs left on the device:
  * the search kernel and the synthesis kernel of ssym_reconstruct_wsola at --search samples, and warp_kernel, all as
    ssym_get_timings reports them (device time between events around the one launch); the calls alternate so that all
    see the same machine; one warm-up round, then the median and the spread (min ... max) of --reps rounds;
  * the search's arithmetic as the definition counts it: targets x (frames - 1) x (2 S + 1) x 1024 x 2 multiply-add
    pairs (a lag outside the source costs nothing and is not counted either), as a rate; every pair is one v_mul_f64 and
    one v_add_f64, since the definition forbids the fused form;
  * the chain match + align by a host clock around the calls, each of which ends in its own synchronisation.

    python tools/wsola_timing.py [--reps 9] [--search 256] [--once SHAPE]

--once SHAPE (grid or ragged) makes one wsola call on that shape after the set-up and exits: the body of a profiler run.
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

BIN = 1024


def shape(name, src, tgt, dim, reps, search, once):
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

    idx, _, lengths, _, maps, _, m_off = match_align()
    dpos = torch.empty(max(int(m_off[-1]), 1), dtype=torch.int64, device="cuda")

    def wsola():
        nat.check(L.ssym_reconstruct_wsola(e.ctx, smp.ptr, idx.ctypes.data, out_off.ctypes.data, n, maps.data_ptr(),
                                           m_off.ctypes.data, frames.ctypes.data, lengths.data_ptr(), search,
                                           nat.WARP_MAP_DEVICE | nat.OUT_DEVICE, dpos.data_ptr(), dout.data_ptr(), None),
                  e.ctx)
        tm = e.timings()
        return tm["main_ms"], tm["reduce_ms"]

    def warp():
        nat.check(L.ssym_reconstruct_warped(e.ctx, smp.ptr, idx.ctypes.data, out_off.ctypes.data, n, maps.data_ptr(),
                                            m_off.ctypes.data, frames.ctypes.data, lengths.data_ptr(),
                                            nat.WARP_MAP_DEVICE | nat.OUT_DEVICE, dout.data_ptr(), None), e.ctx)
        return e.timings()["main_ms"]

    def chain():
        t0 = time.perf_counter()
        match_align()
        return 1e3 * (time.perf_counter() - t0)

    if once:
        print(name, "search %.3f ms, synthesis %.3f ms" % wsola(), flush=True)
        e.close()
        return
    wsola(), warp()
    ms_s, ms_y, ms_w = [], [], []
    for _ in range(reps):
        a, b = wsola()
        ms_s.append(a)
        ms_y.append(b)
        ms_w.append(warp())
    chain()
    ms_c = [chain() for _ in range(reps)]
    valid = lengths.cpu().numpy() > 0
    steps = int(np.sum(np.maximum(t_frames[valid] - 1, 0)))
    pairs = steps * (2 * search + 1) * BIN * 2
    pos = dpos.cpu().numpy()[:int(m_off[-1])]
    mp = maps.cpu().numpy().view(np.uint32)[:int(m_off[-1])].astype(np.int64) * HOP
    slot = np.concatenate([np.arange(int(m_off[t]), int(m_off[t]) + int(frames[t])) for t in np.flatnonzero(valid)])
    moved = int(np.count_nonzero(pos[slot] != mp[slot]))

    def stat(v):
        return "%8.3f ms (%.3f ... %.3f)" % (float(np.median(v)), min(v), max(v))

    med = float(np.median(ms_s))
    print(f"{name:24s} {n} targets, {total} samples, {int(valid.sum())} with a path, S = {search}, "
          f"{moved} of {slot.size} frames moved\n"
          f"    search kernel    {stat(ms_s)}   {pairs / 1e9:.1f} G multiply-add pairs: {pairs / med / 1e9:.2f} T pairs/s, "
          f"{2 * pairs / med / 1e9:.2f} TFLOP/s f64\n"
          f"    synthesis kernel {stat(ms_y)}\n"
          f"    warp_kernel      {stat(ms_w)}   synthesis / warp {float(np.median(ms_y)) / float(np.median(ms_w)):.3f}\n"
          f"    match + align    {stat(ms_c)}   (host clock)", flush=True)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--search", type=int, default=256)
    ap.add_argument("--once", choices=["grid", "ragged"])
    args = ap.parse_args()
    if args.once != "ragged":
        g = synth.make_grid(512, 4096, 128, 13, 0x5EED0003)
        shape("128 f x 13 d", list(g.sources), list(g.targets), 13, args.reps, args.search, args.once)
    if args.once != "grid":
        src, tgt, _ = synth.make_ragged(512, 4096, 5, 40, 12, 0x5EED0041, planted=True)
        shape("ragged 5..40 f x 12 d", src, tgt, 12, args.reps, args.search, args.once)


if __name__ == "__main__":
    main()
