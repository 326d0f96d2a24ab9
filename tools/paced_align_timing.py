#!/usr/bin/env python3
"""tools/paced_align_timing.py -- the paced alignment kernel against ssym_dtw_align on the same pairs (DESIGN.md 5.19,
LAB.md 5.20).

Three workloads, pair p = (source p, target p): 4096 pairs of 128 f x 13 d; 4096 ragged pairs with Fb 5 ... 40 and Fa drawn
inside the paced bounds of Fb (floor((Fb-1)/2) + 1 ... 2 Fb - 1), so that every pair has a paced path; 512 pairs of 256 f x
40 d.  The yardstick is ssym_dtw_align, the symmetric kernel; beside it ssym_dtw_align_step(SSYM_STEP_PACED) on the same
pairs in the same process.  Both with SSYM_OUT_DEVICE outputs (no copies back), warm, a host clock around the call, which
ends in its own synchronisation (the uploads of the pair list and the offsets included, as tools/align_timing.py's "device
outputs" column has them): median of --reps calls after --warmup calls.

    python tools/paced_align_timing.py [--reps 10] [--warmup 3]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from soundsym_amd import Engine  # noqa: E402
from soundsym_amd import _native as nat  # noqa: E402
from soundsym_amd.engine import pack_segments  # noqa: E402


def median_ms(call, reps, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(1e3 * (time.perf_counter() - t0))
    ts = np.array(ts)
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def device_calls(e, d, q, idx):
    """(symmetric, paced, lengths of the paced call): ssym_dtw_align and ssym_dtw_align_step(SSYM_STEP_PACED) into the
    same device outputs."""
    import torch
    p_off, m_off = e.dtw_align_sizes(d, q, idx)
    n = idx.size
    cost = torch.zeros(n, dtype=torch.float64, device="cuda")
    length = torch.zeros(n, dtype=torch.int32, device="cuda")
    path = torch.zeros(2 * int(p_off[-1]), dtype=torch.int32, device="cuda")
    fmap = torch.zeros(max(1, int(m_off[-1])), dtype=torch.int32, device="cuda")

    def args(*step):        # (the closures keep idx, the offsets and the tensors alive: the call takes their addresses)
        return (e.ctx, d.ptr, q.ptr, idx.ctypes.data, None, n, 0, *step, cost.data_ptr(), length.data_ptr(),
                p_off.ctypes.data, path.data_ptr(), m_off.ctypes.data, fmap.data_ptr(), nat.OUT_DEVICE)

    def symmetric():
        nat.check(nat.lib().ssym_dtw_align(*args()), e.ctx)

    def paced():
        nat.check(nat.lib().ssym_dtw_align_step(*args(nat.STEP_PACED)), e.ctx)

    return symmetric, paced, lambda: length.cpu().numpy()


def shape(name, src, tgt, dim, reps, warmup):
    e = Engine(metric="dtw", dtype="f32")
    sf, so = pack_segments(src, dim, np.float32)
    tf, to = pack_segments(tgt, dim, np.float32)
    d, q = e.dictionary(sf, so, dim), e.queries(tf, to, dim)
    idx = np.arange(len(src), dtype=np.uint32)
    symmetric, paced, lengths = device_calls(e, d, q, idx)
    sym = median_ms(symmetric, reps, warmup)
    pac = median_ms(paced, reps, warmup)
    found = int(np.count_nonzero(lengths()))
    cells = float(sum(a.shape[0] * b.shape[0] for a, b in zip(src, tgt)))
    print(f"{name:30s} P {len(src):5d}  cells {cells:.3e}  align {sym[0]:8.3f} ms [{sym[1]:.3f} ... {sym[2]:.3f}]  "
          f"paced {pac[0]:8.3f} ms [{pac[1]:.3f} ... {pac[2]:.3f}]  paced / align {pac[0] / sym[0]:5.2f}  "
          f"{cells / pac[0] * 1e-6:7.2f} Gcell/s  paced paths {found}", flush=True)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    rng = np.random.default_rng(0x5EED0191)
    mk = lambda f, dim: rng.standard_normal((f, dim)).astype(np.float32)
    shape("4096 x 128 f x 13 d", [mk(128, 13) for _ in range(4096)], [mk(128, 13) for _ in range(4096)], 13, args.reps,
          args.warmup)
    fbs = [int(rng.integers(5, 41)) for _ in range(4096)]
    fas = [int(rng.integers((fb - 1) // 2 + 1, 2 * fb)) for fb in fbs]
    shape("4096 x ragged Fb 5..40 x 13 d", [mk(f, 13) for f in fas], [mk(f, 13) for f in fbs], 13, args.reps, args.warmup)
    shape("512 x 256 f x 40 d", [mk(256, 40) for _ in range(512)], [mk(256, 40) for _ in range(512)], 40, args.reps,
          args.warmup)


if __name__ == "__main__":
    main()
