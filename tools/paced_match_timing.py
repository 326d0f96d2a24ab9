#!/usr/bin/env python3
"""tools/paced_match_timing.py -- the paced search (ssym_match_queries_step with SSYM_STEP_PACED) against what gave the
same answer before it, against itself without packing, and beside the paced spot kernel (LAB.md).

    (a)  ssym_dtw_align_step(SSYM_STEP_PACED) over the full N x M pair list (device outputs) and a host argmin of its costs:
         the only earlier route to the answer.  1024 x 1024 ragged 5 ... 40 f x 13 d and 512 x 512 x 128 f x 13 d.
    (b)  the search itself with SSYM_PACED_MATCH_PACK=0 (one pair per wave): what packing buys.  Ragged, 1024^2 and 4096^2.
    (c)  ssym_dtw_spot_step(SSYM_STEP_PACED) over the same pair list, i.e. the same number of cells: the same recurrence with
         a start word.  Context for the rate per cell, not a gate.
    and  configs[0]'s shape (284 x 55 segments of the reference's recordings, tests/golden/audio/) beside the symmetric
         search on the same sets.

One MI355X, one process.  A host clock around each call, which ends in its own synchronisation: median of --reps calls
after --warmup calls; beside it the device time of the new call's two kernels (ssym_get_timings: main_ms, reduce_ms).

    python tools/paced_match_timing.py [--reps 10] [--warmup 3] [--skip-4096]
"""
import argparse
import os
import sys
import time

os.environ.setdefault("SSYM_TEST_HOOKS", "1")          # (b)'s knob is read only with the hooks on; it is read at every launch
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


def fmt(t):
    return f"{t[0]:9.3f} ms [{t[1]:.3f} ... {t[2]:.3f}]"


def feasible_cells(fa, fb):
    fa, fb = np.asarray(fa)[:, None], np.asarray(fb)[None, :]
    ok = (fa >= (fb - 1) // 2 + 1) & (fa <= 2 * fb - 1) & (fa > 0) & (fb > 0)
    return float((fa * fb * ok).sum()), float((fa * fb).sum()), float(ok.mean())


def unpacked(call):
    def run():
        os.environ["SSYM_PACED_MATCH_PACK"] = "0"
        try:
            return call()
        finally:
            del os.environ["SSYM_PACED_MATCH_PACK"]
    return run


def shape(name, src, tgt, dim, reps, warmup, with_align=True, with_spot=True, dtype="f32"):
    npd = np.float32 if dtype == "f32" else np.float64
    e = Engine(metric="dtw", dtype=dtype)
    d, q = e.dictionary(*pack_segments(src, dim, npd), dim), e.queries(*pack_segments(tgt, dim, npd), dim)
    n, m = len(src), len(tgt)
    cells, all_cells, share = feasible_cells([s.shape[0] for s in src], [t.shape[0] for t in tgt])
    print(f"{name}: {n} x {m} pairs, {share:.1%} with a paced shape, {cells:.3e} of {all_cells:.3e} cells", flush=True)

    search = lambda: e.match(d, q, step="paced")
    new = median_ms(search, reps, warmup)
    idx, cost = search()
    tm = e.timings()
    print(f"  paced search           {fmt(new)}  forward {tm['main_ms']:.3f} ms  fold {tm['reduce_ms']:.3f} ms  "
          f"{cells / tm['main_ms'] * 1e-6:7.2f} Gcell/s", flush=True)
    one = median_ms(unpacked(search), reps, warmup)
    idx1, cost1 = unpacked(search)()
    tm1 = e.timings()
    assert np.array_equal(idx, idx1) and np.array_equal(cost.view(np.uint64), cost1.view(np.uint64))
    print(f"  (b) one pair per wave  {fmt(one)}  forward {tm1['main_ms']:.3f} ms  unpacked / packed {one[0] / new[0]:5.2f} "
          f"(forward alone {tm1['main_ms'] / tm['main_ms']:5.2f})", flush=True)
    sym = median_ms(lambda: e.match(d, q), reps, warmup)
    print(f"  symmetric search       {fmt(sym)}  (another cost: for scale)", flush=True)
    if with_align or with_spot:
        si = np.repeat(np.arange(n, dtype=np.uint32), m)
        ti = np.tile(np.arange(m, dtype=np.uint32), n)
    if with_align:
        # the outputs are allocated once, outside the clock: the call, the copy of the costs and the argmin are timed
        import torch
        p_off, m_off = e.dtw_align_sizes(d, q, si, ti)
        dcost = torch.zeros(n * m, dtype=torch.float64, device="cuda")
        dlen = torch.zeros(n * m, dtype=torch.int32, device="cuda")
        dpath = torch.zeros(2 * int(p_off[-1]), dtype=torch.int32, device="cuda")
        dmap = torch.zeros(max(1, int(m_off[-1])), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def old():
            nat.check(nat.lib().ssym_dtw_align_step(e.ctx, d.ptr, q.ptr, si.ctypes.data, ti.ctypes.data, n * m, 0, nat.STEP_PACED,
                                                    dcost.data_ptr(), dlen.data_ptr(), p_off.ctypes.data, dpath.data_ptr(),
                                                    m_off.ctypes.data, dmap.data_ptr(), nat.OUT_DEVICE), e.ctx)
            c = dcost.cpu().numpy().reshape(n, m)
            best = np.where(np.isfinite(c), c, np.inf).argmin(axis=0)
            return best, c[best, np.arange(m)]
        prev = median_ms(old, reps, warmup)
        best, c = old()
        won = np.isfinite(cost)
        assert np.array_equal(best[won], idx[won]) and np.array_equal(c[won].view(np.uint64), cost[won].view(np.uint64))
        print(f"  (a) align list + argmin{fmt(prev)}  new / (a) {new[0] / prev[0]:6.3f}", flush=True)
    if with_spot:
        spot = lambda: e.dtw_spot_device(d, q, si, ti, step="paced")
        sp = median_ms(spot, max(3, reps // 2), 2)
        ts = e.timings()
        print(f"  (c) paced spot, same pairs {fmt(sp)}  kernel {ts['main_ms']:.3f} ms  {all_cells / ts['main_ms'] * 1e-6:7.2f} Gcell/s "
              f"(every cell: a spot has no shape rule)", flush=True)
    e.close()


def config0(reps, warmup):
    import bench
    r = Engine(metric="refcos", dtype="f64")
    (sflat, soff), (tflat, toff) = bench.config0_features(r)
    r.close()
    e = Engine(metric="dtw", dtype="f64")
    d, q = e.dictionary(sflat, soff, 12), e.queries(tflat, toff, 12)
    fa, fb = np.diff(np.asarray(soff).astype(np.int64)), np.diff(np.asarray(toff).astype(np.int64))
    cells, all_cells, share = feasible_cells(fa, fb)
    new = median_ms(lambda: e.match(d, q, step="paced"), reps, warmup)
    idx, cost = e.match(d, q, step="paced")
    tm = e.timings()
    sym = median_ms(lambda: e.match(d, q), reps, warmup)
    sidx, _ = e.match(d, q)
    alen = e.dtw_align(d, q, sidx, step="paced")[1]
    print(f"configs[0] {d.n} x {q.n} (frames {fa.min()} ... {fa.max()} x {fb.min()} ... {fb.max()}), {share:.1%} with a paced shape: "
          f"paced search {fmt(new)} (forward {tm['main_ms']:.3f}, fold {tm['reduce_ms']:.3f})  symmetric search {fmt(sym)}; "
          f"{int(np.isfinite(cost).sum())} targets matched, {int((np.asarray(alen) == 0).sum())} symmetric matches without a paced path, "
          f"{int((idx != sidx).sum())} matches differ", flush=True)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-4096", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(0x5EED0211)
    mk = lambda f, dim: rng.standard_normal((f, dim)).astype(np.float32)
    ragged = lambda count: [mk(int(f), 13) for f in rng.integers(5, 41, size=count)]
    shape("ragged 5...40 f x 13 d", ragged(1024), ragged(1024), 13, args.reps, args.warmup)
    shape("128 f x 13 d", [mk(128, 13) for _ in range(512)], [mk(128, 13) for _ in range(512)], 13, args.reps, args.warmup)
    if not args.skip_4096:
        shape("ragged 5...40 f x 13 d", ragged(4096), ragged(4096), 13, args.reps, args.warmup, with_align=False, with_spot=False)
    config0(args.reps, args.warmup)


if __name__ == "__main__":
    main()
