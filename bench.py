#!/usr/bin/env python3
"""bench.py -- segment-pairs/sec of the DTW matching hot path (BASELINE.json metric).

One step = one pass of the hot path over one batch: every (source, target) pair's DTW cost on the
f16-MFMA filter kernel, candidate selection, exact f64 re-scoring of the candidates and the
per-target argmin (ssym_match_queries) -- with more than one GPU ONE call of ssym_match_sharded per
rank: the same on the rank's source shard plus the RCCL all-reduce(MIN) of the per-target bounds,
the RCCL all-gather of the per-target (cost, index) and the merge kernel, all on the library's
stream.  Features are resident in HBM before the timed region.

Workloads (BASELINE.json `configs`), picked with --workload:
  c3 (default)  configs[2]: 4096 x 4096 segments, 128 frames x 13 dims, f32 -- the configuration the
                metric is quoted on ("the roofline run").  With N GPUs the 4096 sources are split N
                ways (STRONG scaling: "4096x4096 ... 1/2/4/8 GPU").
  c4            configs[3]: 16384 x 4096 segments, 128 frames x 13 dims, source-sharded (2048 per GPU at 8)
  c5            configs[4]: 4096 x 4096 segments, 256 frames x 40 dims, Sakoe-Chiba r = 32, source-sharded
  c2            configs[1]: 1024 x 1024 segments, 64 frames x 13 dims
--src-per-gpu K switches to WEAK scaling (K sources per GPU, the round-1 mode), --targets / --frames /
--dim / --band override single fields for experiments.  --replay-world G (one GPU) measures the step ONE rank of a G-GPU
run would make: its shard through ssym_match_sharded with the full dictionary's bounds replayed into the bound exchange
(DESIGN.md section 7); never a multi-GPU result.

A plain run sets up, warms up, times --steps steps and prints the line.  With --full the line also carries
`early_abandon`, `cpu_baseline` and `secondary`: the reference's own metric (refcos), the chain, one query at a time, the
MFCC front-end, host-resident targets, and `secondary.ragged` -- the reference's REAL segment shape (4096 x 4096 segments
of 5...40 frames, src/sound.rs:330-343) in both metrics with rates on TRUE cells, and BASELINE's configs[0] on the
reference's recordings.  --dump-outputs DIR writes what the last timed step returned (per-target index and cost) as .npy
files, so that two builds can be compared output for output on the same seeded inputs.
"""
import argparse
import glob
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    "c2": dict(n_src=1024, n_tgt=1024, frames=64, dim=13, band=-1, config="configs[1]"),
    "c3": dict(n_src=4096, n_tgt=4096, frames=128, dim=13, band=-1, config="configs[2]"),
    "c4": dict(n_src=16384, n_tgt=4096, frames=128, dim=13, band=-1, config="configs[3]"),
    "c5": dict(n_src=4096, n_tgt=4096, frames=256, dim=40, band=32, config="configs[4]"),
}
# seed 0x5EED0000 + config number (configs[i] is config i + 1); tests/test_gpu_fullsize.py draws the
# same grids from the same generator
SEEDS = {"c2": 0x5EED0002, "c3": 0x5EED0003, "c4": 0x5EED0004, "c5": 0x5EED0005}
PEAK_F16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16/f16 MFMA peak (the cost block runs on the f16 pipe)
PEAK_HBM_GBPS = 8000.0         # MI355X_MICROARCH.md: HBM3E ~8 TB/s


def _oracle_sample(o, grid, gpu_idx, n_src, n_tgt, threads, band):
    tsel = np.arange(n_tgt)
    # keep each sampled target's planted source inside the sampled source block
    planted = grid.planted[tsel]
    rest = np.setdiff1d(np.arange(grid.sources.shape[0]), planted)[:max(0, n_src - planted.size)]
    ssel = np.sort(np.concatenate([planted, rest]))
    sf = np.ascontiguousarray(grid.sources[ssel], dtype=np.float64).reshape(-1)
    tf = np.ascontiguousarray(grid.targets[tsel], dtype=np.float64).reshape(-1)
    so = np.arange(ssel.size + 1, dtype=np.uint64) * grid.frames
    to = np.arange(tsel.size + 1, dtype=np.uint64) * grid.frames
    t0 = time.perf_counter()
    idx, _ = o.dtw_match_all(sf, so, tf, to, grid.dim, band=band, nthreads=threads)
    dt = time.perf_counter() - t0
    ok = bool(np.array_equal(ssel[idx], gpu_idx[tsel])) if gpu_idx is not None else None
    return ssel.size * tsel.size, dt, ok


def cpu_baseline(grid, gpu_idx, band, budget_s=10.0, budget_1core_s=5.0):
    """The CPU oracle (a port: the reference is Rust and cannot be built here) on bounded samples of
    the same workload: OpenMP over targets on all host cores (the headline baseline) and a single
    thread ("separately against 1 core and against all cores").  A small probe sizes
    each sample so that it takes about its budget on whatever host this is."""
    import oracle
    o = oracle.load()
    threads = max(1, min(o.max_threads(), os.cpu_count() or 1))
    n_all_s, n_all_t = grid.sources.shape[0], grid.targets.shape[0]

    def leg(nthreads, budget):
        pairs, dt, _ = _oracle_sample(o, grid, None, 16 if nthreads == 1 else 64,
                                      min(n_all_t, 8 if nthreads == 1 else 4 * nthreads), nthreads, band)
        rate = pairs / max(dt, 1e-6)
        want = max(pairs, rate * budget)
        n_tgt = int(min(n_all_t, max(nthreads, 32 if nthreads == 1 else 256)))
        n_src = int(min(n_all_s, max(n_tgt, want // n_tgt)))
        if n_src == n_all_s:
            n_tgt = int(min(n_all_t, max(n_tgt, want // n_src)))
        pairs, dt, ok = _oracle_sample(o, grid, gpu_idx, n_src, n_tgt, nthreads, band)
        return pairs, dt, ok, n_src, n_tgt

    pairs, dt, ok, n_src, n_tgt = leg(threads, budget_s)
    out = {
        "value": pairs / dt,
        "unit": "segment-pairs/s",
        "cores": threads,
        "kind": "port",
        "sample": f"{n_src}x{n_tgt} sub-grid of the workload ({pairs} pairs, {dt:.1f} s, f64 oracle, "
                  f"OpenMP over targets); indices equal the GPU's: {ok}",
    }
    p1, d1, ok1, s1, t1 = leg(1, budget_1core_s)
    out["one_core"] = {"value": p1 / d1, "unit": "segment-pairs/s", "cores": 1, "kind": "port",
                       "sample": f"{s1}x{t1} sub-grid ({p1} pairs, {d1:.1f} s, one thread); indices equal the GPU's: {ok1}"}
    return out


def secondary_metrics(device: int) -> dict:
    """Outside the timed region: the reference's own metric (refcos, SURVEY.md 8(d) "also report")
    and the neighbouring rows (chain F4, MFCC F3), each one short measurement.  GPU legs only; the
    CPU baseline of refcos is timed by secondary_cpu() after every GPU leg is done."""
    from soundsym_amd import Engine, synth
    out = {}
    n, f, dd = 4096, 128, 12
    g = synth.make_grid(n, n, f, dd, 0x5EED0103)
    off = np.arange(n + 1, dtype=np.uint64) * f
    e = Engine(metric="refcos", dtype="f64", device=device)
    d = e.dictionary(g.sources.astype(np.float64).reshape(-1), off, dd)
    q = e.queries(g.targets.astype(np.float64).reshape(-1), off, dd)
    def leg():
        e.match(d, q)
        t0 = time.perf_counter()
        kms = []
        for _ in range(5):
            e.match(d, q)
            kms.append(e.timings()["main_ms"])
        return (time.perf_counter() - t0) / 5, float(np.mean(kms)) * 1e-3, e.timings()

    # The search's filter is the integer one (csrc/refcos_q8.hip: six exact int8 GEMMs on v_mfma_i32_32x32x32_i8) where
    # the sets' values allow it, the f64 matrix pipe (csrc/refcos_mfma.hip) otherwise; both are timed, the default first.
    dt, k_s, tmr = leg()
    had_hooks = os.environ.get("SSYM_TEST_HOOKS")
    os.environ["SSYM_TEST_HOOKS"] = "1"          # (the library reads its measurement knobs only when asked to)
    os.environ["SSYM_REFCOS_Q8"] = "0"
    dt64, k64, tm64 = leg()
    del os.environ["SSYM_REFCOS_Q8"]
    if had_hooks is None:
        del os.environ["SSYM_TEST_HOOKS"]
    # algorithmic work of the reference's metric: 2 L f64 flops per pair, L = F d, as one zero-padded GEMM.
    # f64 filter: v_mfma_f64_16x16x4_f64, 64 cycles per instruction on MI355X (measured: profiles/r02_refcos_1gpu.md), i.e.
    # 2048 flops / 64 cycles x 1024 SIMDs x 2.4 GHz = 78.6 TFLOP/s.  Integer filter: the same dot as SIX int8 GEMMs (digit
    # products of three 8-bit digits per value), 12 L integer operations per pair, on v_mfma_i32_32x32x32_i8: 65536
    # operations / 32 cycles x 1024 SIMDs x 2.4 GHz = 5033 TOP/s dense.
    flops = 2.0 * n * n * f * dd
    roof64 = {"bound": "mfma", "kernel": "refcos_mfma_kernel" if tm64["used_filter"] else "refcos_sims8_kernel",
              "kernel_ms": k64 * 1e3, "achieved": flops / k64 / 1e12, "peak": 78.6, "unit": "TFLOP/s",
              "frac": flops / k64 / 1e12 / 78.6,
              "model": "2*F*d f64 flops per pair (SURVEY.md 8(d)) over the main kernel's time -- device wall-clock stamps "
                       "written by the search's own kernels (capi.hip useStamps): from the first thread of its init kernel to the "
                       "first thread of the kernel after the main one, i.e. the init kernel and one launch gap included; "
                       "peak = dense f64 MFMA rate, v_mfma_f64_16x16x4_f64 at 64 cycles per instruction"}
    if tmr["refcos_filter"] == 2:
        roof = {"bound": "mfma", "kernel": "refcos_q8_kernel", "kernel_ms": k_s * 1e3, "achieved": 6.0 * flops / k_s / 1e12,
                "peak": 5033.0, "unit": "TFLOP/s", "frac": 6.0 * flops / k_s / 1e12 / 5033.0,
                "model": "six int8 GEMMs (12*F*d integer operations per pair) over the main kernel's time (device wall-clock "
                         "stamps, init kernel and one launch gap included); peak = dense i8 MFMA rate, v_mfma_i32_32x32x32_i8 "
                         "at 32 cycles per instruction x 1024 SIMDs x the nominal 2.4 GHz (tools/mfma_i8_rate.hip measures 33-38 "
                         "cycles per instruction for the chunk's own MFMA stream); what binds the kernel is operand delivery, "
                         "not the pipe (DESIGN.md 5.5)"}
    else:
        roof = roof64
    out["refcos"] = {"value": n * n / dt, "unit": "segment-pairs/s", "ms_per_step": dt * 1e3,
                     "workload": f"{n}x{n} segments, {f} frames x {dd} dims, f64, reference metric "
                                 "(cosine_sim + at_distance, bit-exact)",
                     "phase_ms": {k: round(float(v), 3) for k, v in tmr.items() if k.endswith("_ms")},
                     "through_matrix_pipe": bool(tmr["used_filter"]),
                     "filter": {0: "none (exact tile kernel)", 1: "f64 matrix pipe", 2: "int8 matrix pipe"}[int(tmr["refcos_filter"])],
                     "pairs_rescored_exactly": int(tmr["n_refined"]), "roofline": roof,
                     "f64_filter": {"value": n * n / dt64, "unit": "segment-pairs/s", "ms_per_step": dt64 * 1e3,
                                    "pairs_rescored_exactly": int(tm64["n_refined"]), "roofline": roof64,
                                    "note": "the same search with SSYM_REFCOS_Q8=0: what sets with values the integer "
                                            "records cannot hold (not finite, far out of range) take"}}
    dist_ = np.linspace(0.2, 1.2, 256)
    e.chain(d, g.targets[0].astype(np.float64).reshape(-1), dist_[:2])
    t0 = time.perf_counter()
    e.chain(d, g.targets[0].astype(np.float64).reshape(-1), dist_)
    out["chain"] = {"value": (time.perf_counter() - t0) / dist_.size * 1e6, "unit": "us/step",
                    "workload": f"from_distances, 256 steps on the {n}-entry dictionary (refcos)"}
    # the reference's own call pattern: at_distance / match_sound ONE query at a time (src/sound.rs:453-454), against a
    # 1024-entry dictionary of 5...40-frame segments (through the Python binding, a few us of ctypes included)
    from soundsym_amd.engine import pack_segments
    rsrc, rtgt = synth.make_ragged(1024, 32, 5, 40, dd, 0x5EED0700)
    sf1, so1 = pack_segments([s_.astype(np.float64) * 0.05 for s_ in rsrc], dd)
    d1 = e.dictionary(sf1, so1, dd)
    qs = [t_.astype(np.float64).reshape(-1) * 0.05 for t_ in rtgt]
    e.match_one(d1, qs[0], 1.0)
    t0 = time.perf_counter()
    for _ in range(8):
        for q1 in qs:
            e.match_one(d1, q1, 1.0)
    out["match_one"] = {"value": (time.perf_counter() - t0) / (8 * len(qs)) * 1e6, "unit": "us/query",
                        "workload": "ssym_match_one (refcos), 1024-entry dictionary, queries of 5...40 frames x 12 dims"}
    rate = 44100.0
    x = np.sin(2 * np.pi * 440.0 * np.arange(int(rate * 120)) / rate)
    e.mfcc(x[:44100], rate)
    t0 = time.perf_counter()
    fr = e.mfcc(x, rate).shape[0]
    dt = time.perf_counter() - t0
    out["mfcc"] = {"value": fr / dt, "unit": "frames/s", "workload": "120 s of 44.1 kHz audio, host to host"}
    e.close()
    return out


RAGGED_SEED = 0x5EED0A28          # 4096 x 4096 segments of 5...40 frames: the shape SoundDictionary::add_segments emits


def ragged_metrics(device: int) -> dict:
    """The reference's REAL segment shape (src/sound.rs:330-343: a segment holds seg / HOP frames, seg = letters x 256
    samples, src/lib.rs:137 -- short and ragged, compared over the common prefix by refcos, src/sound.rs:24-28): 4096 x 4096
    segments of 5...40 frames, dtw x 13 values f32 and refcos x 12 values f64, plus BASELINE's configs[0] (the reference's
    two recordings, 284 x 55 segments) end to end.  Rates on TRUE cells (sum of source frames x sum of target frames):
    the padding the kernels add is reported as a ratio, never counted as work."""
    from soundsym_amd import Engine, synth
    from soundsym_amd.engine import pack_segments
    out = {}
    n, lo, hi = 4096, 5, 40
    valu_peak_cells = 1024 * 64 / 16.0 * 2.4e9
    e = Engine(metric="dtw", dtype="f32", device=device)

    def dtw_leg(src, tgt, planted=None, steps=20):
        sf, so = pack_segments(src, 13, np.float32)
        tf, to = pack_segments(tgt, 13, np.float32)
        d, q = e.dictionary(sf, so, 13), e.queries(tf, to, 13)
        for _ in range(5):
            idx, _ = e.match(d, q)
        kms, tot = [], []
        t0 = time.perf_counter()
        for _ in range(steps):
            idx, _ = e.match(d, q)
            tmx = e.timings()
            kms.append(tmx["main_ms"])
            tot.append(tmx["total_ms"])
        dt = (time.perf_counter() - t0) / steps
        true_cells = float(np.diff(so).astype(np.float64).sum()) * float(np.diff(to).astype(np.float64).sum())
        k_s = float(np.mean(kms)) * 1e-3
        leg = {"value": len(src) * len(tgt) / dt, "unit": "segment-pairs/s", "ms_per_step": dt * 1e3,
               "phase_ms": {k: round(float(v), 3) for k, v in tmx.items() if k.endswith("_ms")},
               "filter_ms": k_s * 1e3, "filter_launches": int(tmx["main_launches"]),
               "true_cells_per_s": true_cells / k_s, "true_cells": true_cells,
               "padded_over_true_cells": tmx["n_filter_cells"] / true_cells if tmx["n_filter_cells"] else None,
               "pairs_refined_f64": int(tmx["n_refined"]),
               "valu": {"achieved": true_cells / k_s, "unit": "true DP cells/s", "peak": valu_peak_cells,
                        "frac": true_cells / k_s / valu_peak_cells,
                        "note": "16 VALU cycles per cell per SIMD x 1024 SIMDs at 2.4 GHz, as the headline's roofline.valu; "
                                "cells of the pairs' own matrices only (sum fa x sum fb), over the filter launches' time"}}
        if planted is not None:
            leg["indices_equal_planted"] = bool(np.array_equal(idx.astype(np.int64), planted))
        d.close()
        q.close()
        return leg

    src, tgt = synth.make_ragged(n, n, lo, hi, 13, RAGGED_SEED)
    out["dtw"] = dtw_leg(src, tgt)
    out["dtw"]["workload"] = (f"{n}x{n} segments of {lo}...{hi} frames x 13 dims, f32, dtw, synth.make_ragged seed "
                              f"0x{RAGGED_SEED:X}: unrelated targets (the selection's worst case)")
    srcp, tgtp, pi = synth.make_ragged(n, n, lo, hi, 13, RAGGED_SEED + 1, planted=True)
    out["dtw_planted"] = dtw_leg(srcp, tgtp, pi)
    out["dtw_planted"]["workload"] = ("the same shape, every target a source resampled to another length plus noise "
                                      "(synth.make_ragged planted=True)")
    # the same shape at a dictionary's size: the three class launches' ramp and drain are a tenth of the 1.3 ms search
    # above and nothing of this one
    nl = 16384
    srcl, tgtl = synth.make_ragged(nl, nl, lo, hi, 13, RAGGED_SEED + 3)
    out["dtw_16384"] = dtw_leg(srcl, tgtl, steps=8)
    out["dtw_16384"]["workload"] = f"{nl}x{nl} segments of {lo}...{hi} frames x 13 dims, f32, dtw, unrelated targets"
    del srcl, tgtl
    e.close()

    r = Engine(metric="refcos", dtype="f64", device=device)
    src12, tgt12 = synth.make_ragged(n, n, lo, hi, 12, RAGGED_SEED + 2)
    sf, so = pack_segments([a.astype(np.float64) * 0.05 for a in src12], 12)
    tf, to = pack_segments([a.astype(np.float64) * 0.05 for a in tgt12], 12)
    d, q = r.dictionary(sf, so, 12), r.queries(tf, to, 12)
    for _ in range(3):
        r.match(d, q)
    t0 = time.perf_counter()
    for _ in range(10):
        r.match(d, q)
    dt = (time.perf_counter() - t0) / 10
    tmr = r.timings()
    out["refcos"] = {"value": n * n / dt, "unit": "segment-pairs/s", "ms_per_step": dt * 1e3,
                     "workload": f"{n}x{n} segments of {lo}...{hi} frames x 12 dims, f64, the reference's metric over the "
                                 "common prefix (bit-exact)",
                     "filter": {0: "none (exact tile kernel)", 1: "f64 matrix pipe", 2: "int8 matrix pipe"}[int(tmr["refcos_filter"])],
                     "phase_ms": {k: round(float(v), 3) for k, v in tmr.items() if k.endswith("_ms")},
                     "pairs_rescored_exactly": int(tmr["n_refined"])}

    # BASELINE configs[0]: tests/sample.wav in 16-frame chunks (284) as the dictionary, tests/Section_7_1.wav cut by the 55
    # labels of tests/vowel.txt as targets (data files of the reference's tests, committed under tests/golden/), features
    # from ssym_mfcc.  One ssym_match_batch per metric on host targets -- what clone_from_dictionary becomes.
    feats = config0_features(r)
    if feats is not None:
        (sflat, soff), (tflat, toff) = feats
        leg0 = {"workload": f"configs[0]: {soff.size - 1} x {toff.size - 1} segments of the reference's recordings, 12 MFCCs per frame"}
        for metric, eng in (("refcos", r), ("dtw", Engine(metric="dtw", dtype="f64", device=device))):
            d0 = eng.dictionary(sflat, soff, 12)
            for _ in range(3):
                eng.match_batch(d0, tflat, toff)
            t0 = time.perf_counter()
            for _ in range(20):
                eng.match_batch(d0, tflat, toff)
            leg0[metric + "_ms_per_call"] = (time.perf_counter() - t0) / 20 * 1e3
            d0.close()
            if eng is not r:
                eng.close()
        out["config0"] = leg0
        out["_config0_feats"] = feats
    r.close()
    return out


def config0_features(engine):
    """Features of BASELINE configs[0]'s two recordings (tests/golden/audio): ((source flat, offsets), (target flat, offsets))
    or None when the fixtures are not there."""
    from soundsym_amd import io as sio
    from soundsym_amd.api import HOP, NCOEFFS, frame_features
    gold = os.path.join(ROOT, "tests", "golden")
    ps, pt, pl = (os.path.join(gold, "audio", "sample.wav"), os.path.join(gold, "audio", "Section_7_1.wav"),
                  os.path.join(gold, "vowel.txt"))
    if not all(os.path.exists(x) for x in (ps, pt, pl)):
        return None
    s_smp, srate = sio.read_wav(ps)
    t_smp, trate = sio.read_wav(pt)
    sfe = frame_features(s_smp, srate, engine=engine)
    seg = 16 * HOP
    lens = [seg] * (s_smp.size // seg)
    rest = (s_smp.size - sum(lens)) // HOP * HOP
    lens += [rest] if rest else []
    sft, fpos = [], 0
    for L in lens:
        nf = L // HOP
        sft.append(sfe[fpos:fpos + nf * NCOEFFS].reshape(nf, NCOEFFS))
        fpos += nf * NCOEFFS
    tft = []
    for a, b, _ in sio.audacity_labels_to_timestamps(pl):
        piece = t_smp[int(round(a * trate)):int(round(b * trate)) + 1]
        if piece.size >= HOP:
            tft.append(frame_features(piece, trate, engine=engine).reshape(-1, NCOEFFS))
    from soundsym_amd.engine import pack_segments
    return pack_segments([x for x in sft if x.shape[0] > 0], NCOEFFS), pack_segments(tft, NCOEFFS)


def secondary_cpu(out: dict) -> None:
    """refcos as the reference runs it: one thread, norms recomputed per pair (the oracle), on a sub-grid."""
    import oracle as oracle_pkg
    from soundsym_amd import synth
    o = oracle_pkg.load()
    n, f, dd, k = 4096, 128, 12, 192
    g = synth.make_grid(n, n, f, dd, 0x5EED0103)
    offk = np.arange(k + 1, dtype=np.uint64) * f
    sf = g.sources[:k].astype(np.float64).reshape(-1)
    tf = g.targets[:k].astype(np.float64).reshape(-1)
    t0 = time.perf_counter()
    o.refcos_match_all(sf, offk, tf, offk, dd)
    dt = time.perf_counter() - t0
    out["refcos"]["cpu_baseline"] = {"value": k * k / dt, "unit": "segment-pairs/s", "cores": 1, "kind": "port",
                                     "sample": f"{k}x{k} sub-grid, single thread as the reference runs it"}
    feats = out.get("ragged", {}).pop("_config0_feats", None)
    if feats is not None:          # configs[0] on the host: the oracle, one thread, the same features
        (sflat, soff), (tflat, toff) = feats
        t0 = time.perf_counter()
        o.refcos_match_all(sflat, soff, tflat, toff, 12)
        t1 = time.perf_counter()
        o.dtw_match_all(sflat, soff, tflat, toff, 12, nthreads=1)
        t2 = time.perf_counter()
        out["ragged"]["config0"]["cpu_oracle_one_thread_ms"] = {"refcos": (t1 - t0) * 1e3, "dtw": (t2 - t1) * 1e3}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path: str, arrays: dict) -> None:
    """--dump-outputs: every array (one value per target) as <path>/<name>.npy in float64 (indices included: exact below
    2^53).  Above DUMP_LIMIT_BYTES in all, the same fixed, seeded sample of targets is kept of each, and its target numbers
    are written as rows.npy."""
    os.makedirs(path, exist_ok=True)
    n = len(next(iter(arrays.values())))
    if 8 * n * len(arrays) > DUMP_LIMIT_BYTES:
        rows = np.sort(np.random.default_rng(0).choice(n, DUMP_LIMIT_BYTES // (8 * (len(arrays) + 1)), replace=False))
        arrays = dict({k: v[rows] for k, v in arrays.items()}, rows=rows)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.asarray(a, dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="c3",
                    help="BASELINE.json config: c3 = configs[2] (default, the metric's), c4 = configs[3], c5 = configs[4]")
    ap.add_argument("--full", action="store_true",
                    help="also measure what is reported beside the headline: early abandoning, the secondary legs "
                         "(refcos, chain, mfcc, host batch, ragged) and the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true",
                    help="with --full: skip the refcos / chain / mfcc / early-abandon measurements")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's per-target index and cost to DIR/<name>.npy (float64)")
    ap.add_argument("--src-per-gpu", type=int, default=0, help="WEAK scaling: this many sources per GPU (default: "
                    "the workload's sources split over the GPUs, strong scaling)")
    ap.add_argument("--sources", type=int, default=0)
    ap.add_argument("--targets", type=int, default=0)
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--dim", type=int, default=0)
    ap.add_argument("--band", type=int, default=None, help="Sakoe-Chiba radius, -1 = none")
    ap.add_argument("--replay-world", type=int, default=0,
                    help="MEASUREMENT on one GPU: the step rank --replay-rank of a run over this many GPUs would make -- its "
                         "shard of the sources through ssym_match_sharded on a world-1 RCCL communicator, with the bounds of the "
                         "FULL dictionary (what the larger run's all-reduce returns) replayed into the bound exchange "
                         "(ssym_comm_replay_bounds), so that selection and re-scoring see what that rank would see")
    ap.add_argument("--replay-rank", type=int, default=0)
    args = ap.parse_args()
    if not args.full:
        args.no_secondary = args.no_cpu_baseline = True
    if args.replay_world:
        if args.gpus != 1 or not (0 <= args.replay_rank < args.replay_world):
            sys.exit("--replay-world G needs --gpus 1 and 0 <= --replay-rank < G")
        os.environ["SSYM_BENCH_FORCE_DIST"] = "1"
        os.environ["SSYM_TEST_HOOKS"] = "1"
        args.no_secondary = args.no_cpu_baseline = True
    wl = dict(WORKLOADS[args.workload])
    custom = []
    for key, val in (("n_src", args.sources), ("n_tgt", args.targets), ("frames", args.frames), ("dim", args.dim)):
        if val:
            wl[key] = val
            custom.append(key)
    if args.band is not None:
        wl["band"] = args.band
        custom.append("band")

    SEED = SEEDS[args.workload]
    # `python bench.py --gpus N` with N > 1 and no launcher around it: start the N ranks here, one process per GPU, with
    # the launcher the driver would have used.  This parent has made no GPU call (nothing above imports torch or the
    # library), it only waits: rank 0's record reaches stdout through the inherited descriptor, and the exit code is
    # the launcher's (non-zero when any rank failed).
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and os.environ.get("SSYM_BENCH_FORCE_DIST") != "1":
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.setdefault("OMP_NUM_THREADS", "1")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        print("bench.py: launching %d ranks: %s" % (args.gpus, " ".join(cmd)), file=sys.stderr, flush=True)
        sys.exit(subprocess.call(cmd, env=env))

    # stdout carries ONE line, the JSON record of rank 0: libraries write there too (RCCL prints a five-line version
    # banner on the first communicator of a process), so file descriptor 1 is pointed at stderr for the run and the
    # record goes to the saved descriptor at the end
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    import torch
    import torch.distributed as dist
    from soundsym_amd import Engine, sharding, synth

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # SSYM_BENCH_FORCE_DIST=1: run the collective code path (RCCL communicator, all-reduce, all-gather, merge)
    # with one rank -- a smoke check of the N > 1 plumbing on a single-GPU box
    force_dist = os.environ.get("SSYM_BENCH_FORCE_DIST") == "1"
    if world > 1 or force_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if os.environ.get("SSYM_BENCH_FAIL_RANK") == str(rank) and world > 1:
        sys.exit(f"rank {rank}: SSYM_BENCH_FAIL_RANK (tests/test_gpu_bench.py: a dying rank must fail the whole run)")
    if args.gpus != world and not force_dist:
        sys.exit(f"bench.py --gpus {args.gpus} inside a launcher with WORLD_SIZE={world}: the two must agree")
    # SSYM_BENCH_BACKEND=gloo rehearses the N > 1 code path on a box with fewer GPUs than ranks: the exchange
    # then runs as torch.distributed collectives over gloo around the two-phase C-ABI calls (RCCL cannot put
    # two ranks on one device); the judged path is the default, RCCL inside the library
    backend = os.environ.get("SSYM_BENCH_BACKEND", "nccl")
    local_rank = local_rank % max(torch.cuda.device_count(), 1) if backend == "gloo" else local_rank
    torch.cuda.set_device(local_rank)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world,
                                    device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    n_gpus = max(world, 1)
    weak = args.src_per_gpu > 0
    n_src_total = args.src_per_gpu * n_gpus if weak else wl["n_src"]
    m, frames, DIM_, band = wl["n_tgt"], wl["frames"], wl["dim"], wl["band"]

    # synthetic workload (seeded; the generator is counter-based, so each rank materialises only its
    # own source shard of the one global grid -- the targets and planted indices are the same on all)
    lo, hi = sharding.shard_range(n_src_total, n_gpus, rank)
    if args.replay_world:
        lo, hi = sharding.shard_range(n_src_total, args.replay_world, args.replay_rank)
    if n_gpus > 1 or args.replay_world:
        grid = synth.make_grid(n_src_total, m, frames, DIM_, SEED, src_range=(lo, hi))
        shard = grid.sources
    else:
        grid = synth.make_grid(n_src_total, m, frames, DIM_, SEED)
        shard = grid.sources[lo:hi]
    eng = Engine(metric="dtw", dtype="f32", device=local_rank, band=band)
    src_dev = torch.from_numpy(np.ascontiguousarray(shard).reshape(-1)).cuda()
    tgt_dev = torch.from_numpy(np.ascontiguousarray(grid.targets).reshape(-1)).cuda()
    so = np.arange(hi - lo + 1, dtype=np.uint64) * frames
    to = np.arange(m + 1, dtype=np.uint64) * frames
    d = eng.dictionary(src_dev, so, DIM_)
    q = eng.queries(tgt_dev, to, DIM_)
    out_idx = torch.empty(m, dtype=torch.int32, device="cuda")
    out_cost = torch.empty(m, dtype=torch.float64, device="cuda")
    bounds = torch.empty(m, dtype=torch.float64, device="cuda")
    sharded = world > 1 or force_dist
    comm = None
    if sharded and backend == "nccl":
        # RCCL communicator behind the C ABI (collective).  Every rank first says whether it can bind RCCL at all: a rank
        # that could not would leave the others waiting inside ncclCommInitRank.  If any cannot, ALL ranks run the same
        # exchange as torch.distributed collectives around the two-phase C-ABI calls (match_sharded_torch) and say so.
        # The probe is the library's own (ssym_comm_available: every RCCL symbol comm.hip calls was bound), not Python's.
        from soundsym_amd.engine import comm_available
        ok = 1 if comm_available() else 0
        if not ok:
            print(f"rank {rank}: RCCL not bound by the library; torch.distributed collectives instead", file=sys.stderr)
        if world > 1:
            t = torch.tensor([ok], dtype=torch.int32, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            ok = int(t.item())
        if ok:
            comm = sharding.init_comm(eng, rank, world)

    replay = None
    if args.replay_world:
        if comm is None:
            sys.exit("--replay-world needs the library's RCCL communicator")
        # the bounds of the FULL dictionary: the minimum over the shards' offers, i.e. the larger run's all-reduce result
        full = synth.make_grid(n_src_total, m, frames, DIM_, SEED)
        dfull = eng.dictionary(torch.from_numpy(np.ascontiguousarray(full.sources).reshape(-1)).cuda(),
                               np.arange(n_src_total + 1, dtype=np.uint64) * frames, DIM_)
        replay = torch.empty(m, dtype=torch.float64, device="cuda")
        eng.match_begin(dfull, q, replay)
        tmp_i, tmp_c = torch.empty_like(out_idx), torch.empty_like(out_cost)
        eng.match_finish(replay.clone(), tmp_i, tmp_c)           # (a begun match has to be finished)
        torch.cuda.synchronize()
        dfull.close()
        del full
        comm.replay_bounds(replay)

    def run_step(oi, oc, prune=False, queries=None):
        qq = q if queries is None else queries
        if comm is not None:
            return sharding.match_sharded(eng, comm, d, qq, lo, out_idx=oi, out_cost=oc, prune=prune)
        if sharded:
            return sharding.match_sharded_torch(eng, d, qq, lo, oi, oc, bounds, prune=prune)
        eng.match(d, qq, index_base=lo, out_idx=oi, out_cost=oc, prune=prune)
        return oi, oc

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(fn, steps, warmup, per_step=None):
        for _ in range(warmup):
            fn()
        fence()
        t0 = time.perf_counter()
        res = None
        for _ in range(steps):
            res = fn()
            if per_step:
                per_step()
        fence()
        elapsed = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        return elapsed, res

    stats = {k: [] for k in ("main_ms", "select_ms", "refine_ms", "reduce_ms", "collective_ms", "total_ms")}
    last = {}

    def note():
        tm = eng.timings()
        for k in stats:
            stats[k].append(tm[k])
        last.update(tm)

    elapsed, (fin_idx, fin_cost) = timed(lambda: run_step(out_idx, out_cost), args.steps, args.warmup, note)
    pairs_per_step = (hi - lo) * m if args.replay_world else n_src_total * m
    value = pairs_per_step * args.steps / elapsed
    idx_host = fin_idx.cpu().numpy().view(np.uint32).astype(np.int64)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"match_idx": idx_host, "match_cost": fin_cost.cpu().numpy()})
    planted_ok = bool(np.array_equal(idx_host, grid.planted))
    if args.replay_world:      # one rank of a larger world: it answers the targets whose neighbour its shard holds
        mine = (grid.planted >= lo) & (grid.planted < hi)
        planted_ok = bool(np.array_equal(idx_host[mine], grid.planted[mine]))

    # per-rank figures of the timed steps (rank 0 prints them)
    mine = [float(np.mean(stats[k])) for k in ("main_ms", "select_ms", "refine_ms", "collective_ms", "total_ms")] + \
           [float(last.get("n_refined", 0)), float(last.get("attempts", 1))]
    per_rank = [mine]
    if world > 1:
        t = torch.tensor(mine, dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        allt = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(allt, t)
        per_rank = [x.cpu().tolist() for x in allt]

    # Beside the headline (which fills the whole cost matrix): the same search with early abandoning
    # (SSYM_DTW_PRUNE) -- identical indices and costs, but the time depends on the data: this
    # planted grid is its BEST case, so the worst case (targets with no close source: nothing can be cut)
    # is measured beside it.  Reported separately and never as `value`.
    early = None
    if not args.no_secondary:
        p_idx, p_cost = torch.empty_like(out_idx), torch.empty_like(out_cost)
        full_idx, full_cost = fin_idx.clone(), fin_cost.clone()
        p_elapsed, (pf_idx, pf_cost) = timed(lambda: run_step(p_idx, p_cost, prune=True), args.steps, args.warmup)
        ptm = eng.timings()
        identical = bool(torch.equal(pf_idx, full_idx) and torch.equal(pf_cost, full_cost))
        rows = 16 * 4 * ((frames + 63) // 64) if frames > 48 else 16 * ((frames + 15) // 16)
        full_cells = float(((hi - lo + 7) // 8 * 8)) * ((m + 31) // 32 * 32) * rows * frames
        early = {
            "value": pairs_per_step * args.steps / p_elapsed, "unit": "segment-pairs/s",
            "ms_per_step": p_elapsed / args.steps * 1e3,
            "identical_to_full_search": identical,
            "filter_cells_swept_frac": (ptm["n_filter_cells"] / full_cells if ptm["pruned"] and band < 0 else None),
            "phase_ms": {k: round(float(v), 3) for k, v in ptm.items() if k.endswith("_ms")},
            "rank0_only": ["filter_cells_swept_frac", "phase_ms"] if world > 1 else [],
            "note": "one centroid-nearest candidate per target scored exactly, then the filter stops row passes and drops "
                    "64-pair tasks that are provably above it; planted grid = best case, see no_close_pair for the worst",
        }
        # worst case: the same dictionary against targets that are nobody's neighbour (another seed's sources)
        other = synth.make_grid(m, 1, frames, DIM_, SEED ^ 0x77777).sources
        q2 = eng.queries(torch.from_numpy(np.ascontiguousarray(other).reshape(-1)).cuda(), to, DIM_)
        u_idx, u_cost = torch.empty_like(out_idx), torch.empty_like(out_cost)
        ksteps = max(2, args.steps // 4)
        uf_elapsed, (uf_idx, uf_cost) = timed(lambda: run_step(u_idx, u_cost, queries=q2), ksteps, 1)
        uf_idx, uf_cost = uf_idx.clone(), uf_cost.clone()
        up_elapsed, (up_idx, up_cost) = timed(lambda: run_step(p_idx, p_cost, prune=True, queries=q2), ksteps, 1)
        early["no_close_pair"] = {
            "full_ms_per_step": uf_elapsed / ksteps * 1e3, "pruned_ms_per_step": up_elapsed / ksteps * 1e3,
            "pruned_over_full": up_elapsed / uf_elapsed,
            "identical_to_full_search": bool(torch.equal(up_idx, uf_idx) and torch.equal(up_cost, uf_cost)),
            "workload": f"the same {n_src_total} sources against {m} unrelated targets (no planted neighbour)",
        }
        q2.close()

    secondary = None
    if rank == 0 and n_gpus == 1 and not args.no_secondary:
        # SURVEY.md 8(d) "H2D of inputs reported separately": the same step through ssym_match_batch, the targets in
        # (pageable) HOST memory -- upload, packing, records, match, results back, release: what a drop-in
        # clone_from_dictionary pays per batch.  Never `value`.
        tflat = np.ascontiguousarray(grid.targets).reshape(-1)
        for _ in range(2):
            eng.match_batch(d, tflat, to)
        hb_n = 5
        t0 = time.perf_counter()
        packs = []
        for _ in range(hb_n):
            hb_idx, _ = eng.match_batch(d, tflat, to)
            packs.append(eng.timings()["pack_ms"])
        hb_dt = (time.perf_counter() - t0) / hb_n
        host_batch = {"value": pairs_per_step / hb_dt, "unit": "segment-pairs/s", "ms_per_call": hb_dt * 1e3,
                      "pack_ms": float(np.mean(packs)), "target_bytes": int(tflat.nbytes),
                      "indices_equal_planted": bool(np.array_equal(hb_idx.astype(np.int64) + 0, grid.planted)),
                      "resident_ms_per_step": elapsed / args.steps * 1e3,
                      "note": "ssym_match_batch: targets handed over as host memory every call (PCIe upload + packing = "
                              "pack_ms, device time), against the same step on resident targets"}
        secondary = secondary_metrics(local_rank)
        secondary["host_batch"] = host_batch
        secondary["ragged"] = ragged_metrics(local_rank)

    if rank == 0:
        # Roofline of the dominant kernel (dtw_filter_kernel / dtw_band_kernel).  Its duration is measured live
        # with HIP events on the library's own stream (ssym_get_timings).  Algorithmic work per pair is
        # SURVEY.md 8(d)'s: bytes 2*F*d*4 (per-pair operand-streaming model -- the model the
        # north star's ">= 60 % HBM roofline" is stated in), matrix flops 2*cells*d, DP cells F^2 (band: in-band cells).
        k_ms = float(np.mean(stats["main_ms"]))
        k_s = k_ms * 1e-3
        pairs_launch = (hi - lo) * m
        f, dd, r = frames, DIM_, band
        cells_pair = float(f) * f if r < 0 else float(f * (2 * r + 1) - r * (r + 1))
        stream_gbps = pairs_launch * 2 * f * dd * 4 / k_s / 1e9
        flops_tf = pairs_launch * 2.0 * cells_pair * dd / k_s / 1e12
        cells_per_s = pairs_launch * cells_pair / k_s
        recorded = None
        prof_name = {"c3": "*bench_1gpu.json", "c5": "*bench_c5_1gpu.json"}.get(args.workload)
        prof = sorted(glob.glob(os.path.join(ROOT, "profiles", prof_name))) if prof_name else []
        if prof and n_gpus == 1 and not custom and not weak:
            pj = json.load(open(prof[-1]))           # rocprofv3 PMC passes over this same command (tools/profile_bench.sh)
            recorded = {"file": os.path.relpath(prof[-1], ROOT),
                        "hbm_traffic_bytes_per_launch": pj.get("hbm_traffic_bytes_per_launch"),
                        "kernel_ms_in_profile": pj.get("dominant_kernel_avg_ms"),
                        "mfma_pipe_busy_frac": pj.get("mfma_busy_fraction"),
                        "valu_busy_frac": pj.get("valu_busy_fraction"),
                        "note": "RECORDED by an earlier rocprofv3 --pmc run of this command (counters cannot be read "
                                "inside an unprofiled run); not measured by the run that printed this line"}
        traffic = recorded["hbm_traffic_bytes_per_launch"] if recorded else None
        # VALU floor measured on MI355X (profiles/): v_sqrt_f32 8 + v_min3_f32 4 + v_add_f32 4
        # cycles per wave-instruction = 16 cycles per 64 cells per SIMD, 1024 SIMDs
        valu_peak_cells = 1024 * 64 / 16.0 * 2.4e9
        # operand planes (K = 16 each) a 32x32 tile multiplies: 2 for frames of up to 13 values (record layout 3 of
        # csrc/ssym_internal.hpp), 3 otherwise; every MFMA also holds the SIMD's vector issue for 8 of its 32 cycles
        # (MI355X_MICROARCH.md, 'vector-instruction ISSUE cost'), which the 16-cycle cell model leaves out
        planes = 2 if ((dd <= 13 and not os.environ.get("SSYM_FILTER_K48")) or 14 <= dd <= 26) else 3
        tiles_per_cell = 1.0 / 16 if r < 0 else float((2 * r + 1 + 15) // 16) / (2 * r + 1)
        issue_cycles = 16.0 + 8.0 * planes * tiles_per_cell
        scaling = "n/a" if n_gpus == 1 else ("weak" if weak else "strong")
        names = ("main_ms", "select_ms", "refine_ms", "collective_ms", "total_ms", "n_refined", "attempts")
        line = {
            "metric": "segment-pairs/sec (DTW cost+argmin)",
            "value": value,
            "unit": "segment-pairs/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": scaling,
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": f"{wl['config'] if not custom and not weak else 'custom'}: {n_src_total}x{m} segments, "
                            f"{f} frames x {dd} dims, f32, "
                            f"dtw (L2 local cost, {'full matrix' if r < 0 else f'Sakoe-Chiba r={r}'}), "
                            f"planted neighbours, seed 0x{SEED:X}",
                "workload_key": args.workload,
                "sources_per_gpu": hi - lo,
                "parallelism": (f"source-shard x{n_gpus}, RCCL all-reduce(MIN) of bounds + all-gather of (cost, index) "
                                f"inside the library" if comm is not None and n_gpus > 1 else
                                (f"source-shard x{n_gpus}, {backend} collectives of torch.distributed around the two-phase "
                                 f"C-ABI calls" if sharded else "single GPU")),
                "indices_equal_planted": planted_ok,
                "replay": ({"world": args.replay_world, "rank": args.replay_rank,
                            "note": "ONE GPU: this rank's shard through ssym_match_sharded (world-1 RCCL) with the full "
                                    "dictionary's bounds replayed into the bound exchange; `value` counts this shard's pairs "
                                    "only; a measurement for the strong-scaling prediction, not a multi-GPU result"}
                           if args.replay_world else None),
                "pairs_refined_f64": int(last.get("n_refined", 0)),
                "phase_ms": {k: round(float(np.mean(v)), 3) for k, v in stats.items()},
                "collective_ms": round(float(np.mean(stats["collective_ms"])), 4),
                "per_rank": [{k: (round(v, 4) if k.endswith("_ms") else int(v)) for k, v in zip(names, row)}
                             for row in per_rank],
            },
            "roofline": {
                "bound": "hbm",
                "kernel": "dtw_filter_kernel" if r < 0 else "dtw_band_kernel",
                "model": "SURVEY.md 8(d) per-pair operand-streaming bytes 2*F*d*4 x pairs per launch / kernel time.  The "
                         "kernel keeps operands on chip: the bytes it really moves are in 'hbm_measured', and what "
                         "binds it is VALU issue ('binding_limit', 'valu')",
                "achieved": stream_gbps,
                "peak": PEAK_HBM_GBPS,
                "unit": "GB/s",
                "frac": stream_gbps / PEAK_HBM_GBPS,
                "traffic": traffic,
                "traffic_note": "bytes per launch at the L2-fabric boundary (rocprofv3 FETCH_SIZE x2 + WRITE_SIZE), RECORDED "
                                "in profiles/ (see 'recorded_pmc'), not measured by this run",
                "algorithmic_bytes_per_launch": pairs_launch * 2 * f * dd * 4,
                "kernel_ms": k_ms,
                "binding_limit": "valu",
                "hbm_measured": ({"achieved": traffic / k_s / 1e9, "unit": "GB/s", "frac": traffic / k_s / 1e9 / PEAK_HBM_GBPS,
                                  "note": "recorded traffic / live kernel time"} if traffic else None),
                "mfma": {"achieved": flops_tf, "unit": "TFLOP/s", "algorithmic_flops_per_pair": 2 * cells_pair * dd,
                         "peak_f16_mfma": PEAK_F16_MFMA_TFLOPS, "frac_of_f16_mfma_peak": flops_tf / PEAK_F16_MFMA_TFLOPS,
                         "mfmas_per_tile": planes,
                         "note": f"cost block on the f16 matrix pipe ({planes} x v_mfma_f32_32x32x16_f16 per 32x32 tile: K = "
                                 f"{16 * planes} slots for d values and both squared norms, f16-split operands); ALGORITHMIC "
                                 "flops 2*cells*d over the dense f16 peak -- utilisation of the pipe itself is "
                                 "recorded_pmc.mfma_pipe_busy_frac"},
                "valu": {"achieved": cells_per_s, "unit": "DP cells/s", "peak": valu_peak_cells,
                         "frac": cells_per_s / valu_peak_cells,
                         "note": "16 VALU cycles per cell per SIMD (v_sqrt_f32 8 + v_min3_f32 4 + v_add_f32 4, measured "
                                 "issue costs) x 1024 SIMDs at 2.4 GHz",
                         "issue_cycles_per_cell_with_mfma": issue_cycles,
                         "frac_with_mfma_issue": cells_per_s / (1024 * 64 / issue_cycles * 2.4e9),
                         "note_mfma_issue": "the same model plus the 8 vector-issue cycles each MFMA of a tile holds the SIMD "
                                            "for: the floor of the instruction stream as written, still at the nominal 2.4 GHz "
                                            "(the kernel runs power-limited at 2.1-2.2 GHz, profiles/)"},
                "recorded_pmc": recorded,
            },
        }
        if r >= 0:
            # Banded workloads: the per-pair operand-streaming byte model exceeds the HBM peak several times over (the
            # operands never leave the chip), so it is kept as a labelled sub-object and the top-level object names the
            # nearer of the two hardware ceilings the schema allows, the matrix pipe; what binds is 'valu' either way.
            rl = line["roofline"]
            rl["hbm_streaming_model"] = {"achieved": rl["achieved"], "peak": rl["peak"], "unit": rl["unit"], "frac": rl["frac"],
                                         "note": "2*F*d*4 bytes per pair x pairs / kernel time: above 1 because nothing is re-streamed"}
            rl.update({"bound": "mfma", "achieved": flops_tf, "peak": PEAK_F16_MFMA_TFLOPS, "unit": "TFLOP/s",
                       "frac": flops_tf / PEAK_F16_MFMA_TFLOPS,
                       "model": "SURVEY.md 8(d) in-band matrix flops 2*d*cells per pair x pairs per launch / kernel time over "
                                "the dense f16 MFMA peak; the binding limit is VALU issue ('valu')"})
        if early is not None:
            line["early_abandon"] = early
        # the CPU legs come last: every GPU figure above is measured before the host cores are loaded
        if n_gpus == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(grid, idx_host, band)
            line["vs_cpu_all_cores"] = value / line["cpu_baseline"]["value"]
            line["vs_cpu_one_core"] = value / line["cpu_baseline"]["one_core"]["value"]
        if secondary is not None:
            if not args.no_cpu_baseline:
                secondary_cpu(secondary)
            secondary.get("ragged", {}).pop("_config0_feats", None)
            line["secondary"] = secondary
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(line) + "\n").encode())
    if comm is not None:
        comm.close()
    eng.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
