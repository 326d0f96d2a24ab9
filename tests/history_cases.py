"""The cases of tests/test_gpu_history.py as data and functions -- TEST INFRASTRUCTURE (tests/test_history_cases.py checks
this module on the CPU; nothing here touches the GPU at import).

A context (ssym_ctx) carries state from call to call: the block cache of dev_alloc / dev_free, the DeviceBufs that
ensure() keeps while they are large enough, caches inside handles, host flags ("What a context carries
between calls").  A *probe* is one call family at the smallest shape at which its routes still differ; a *prelude* makes
a context dirty before the probe runs on it.  The tests hold the probe's outputs on the dirty context to the same
probe's outputs on a fresh one, bit for bit.

    Probe.run(engine, variant)   -> (outputs: tuple of host numpy arrays, route: dict of the route-naming timings)
    Probe.shape(variant)         -> n, m, dim, total frames and the length vector of what run() would feed (CPU)
    PLAIN                        the probe's own data
    twin(fill)                   the same n, m, dim and total frames, the lengths rotated by one, every value `fill`:
                                 every block the probe will allocate is in the cache and was last written by this
    larger(fill)                 three times the segments, frames and (where the call takes it) values per frame
    PRELUDES                     name -> function(engine, probe) that dirties the engine

Every probe creates its own handles and closes them; a hostile call that the library refuses (SsymError) counts as
history like any other."""
import os
from collections import namedtuple

import numpy as np

from soundsym_amd import Engine, SsymError
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

NAN, INF = float("nan"), float("inf")
RATE = 44100.0

DTW64 = dict(metric="dtw", dtype="f64")
DTW32 = dict(metric="dtw", dtype="f32")
BAND8 = dict(metric="dtw", dtype="f32", band=8)
BAND6 = dict(metric="dtw", dtype="f64", band=6)
REFCOS = dict(metric="refcos", dtype="f64")

ROUTE_KEYS = ("used_filter", "refcos_filter", "pruned", "n_pairs")

Variant = namedtuple("Variant", "fill permute grow")
PLAIN = Variant(None, False, 1)
FILLS = ("nan", "inf", "big", "same")


def twin(fill):
    return Variant(fill, True, 1)


def larger(fill):
    return Variant(fill, True, 3)


def ctx_key(ctx):
    return tuple(sorted(ctx.items()))


def new_engine(ctx):
    return Engine(**ctx)


# -- data -------------------------------------------------------------------------------------------------------------
def _values(rng, shape, fill, scale, f32):
    if fill is None:
        return rng.normal(size=shape) * scale
    if fill == "same":                                   # one frame, everywhere: every cost and every key ties
        if len(shape) == 1:
            return np.full(shape, 0.25)
        row = np.random.default_rng(0x5A3E).normal(size=shape[-1:]) * (scale if np.ndim(scale) else float(scale))
        return np.broadcast_to(row, shape).copy()
    return np.full(shape, {"nan": NAN, "inf": INF, "big": 3e38 if f32 else 1e300}[fill])


def variant_lengths(lengths, variant):
    """A set's lengths under a variant: rotated by one (the same multiset, other places), then three times as many of
    three times the length."""
    ls = list(lengths)
    if variant.permute:
        ls = ls[1:] + ls[:1]
    if variant.grow > 1:
        ls = [f * variant.grow for f in ls] * variant.grow
    return ls


class Data:
    """What one run of a probe feeds: per set a list of arrays ([frames][dim] for frame sets, [samples] for sample sets,
    None for a set that is lengths only), drawn from the probe's seed (the twin draws nothing: it is all one value)."""

    def __init__(self, probe, variant):
        self.variant = variant
        self.dim = probe.dim * (variant.grow if probe.grow_dim else 1)
        self.lengths, self.sets = {}, {}
        f32 = probe.ctx.get("dtype") == "f32"
        rng = np.random.default_rng(probe.seed)
        for name, (kind, lengths) in probe.sets.items():
            ls = self.lengths[name] = variant_lengths(lengths, variant)
            if kind == "frames":
                scale = probe.scale if np.ndim(probe.scale) == 0 else np.resize(probe.scale, self.dim)
                segs = [_values(rng, (f, self.dim), variant.fill, scale, f32) for f in ls]
                if f32:
                    with np.errstate(over="ignore"):
                        segs = [s.astype(np.float32).astype(np.float64) for s in segs]
                self.sets[name] = segs
            elif kind == "samples":
                self.sets[name] = [_values(rng, (f,), variant.fill, 0.3, False) for f in ls]
            else:
                self.sets[name] = None

    def __getitem__(self, name):
        return self.sets[name]

    def flat(self, name, dtype=np.float64):
        """(values, frame offsets) of a frame set as the engine takes them."""
        return pack_segments(self.sets[name], self.dim, dtype)

    def samples(self, name):
        """(samples, sample offsets) of a sample set."""
        xs = self.sets[name]
        off = np.concatenate([[0], np.cumsum([x.size for x in xs])]).astype(np.uint64)
        return (np.concatenate(xs) if xs else np.zeros(0)), off


class Handles:
    """The handles of one run, closed in reverse order of creation whatever happens."""

    def __init__(self):
        self.items = []

    def add(self, h):
        self.items.append(h)
        return h

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for h in reversed(self.items):
            h.close()
        return False


class Probe:
    """One call family: `call(engine, data, handles)` runs it on `ctx` engines and returns its outputs (and, where the
    timings name it, its route); `sets` maps a name to ("frames" | "samples" | "lengths", lengths); `entry_points` are
    the ssym_* calls it runs; `takes_dict`: call() accepts dictionary=, a handle that holds the probe's sources."""

    def __init__(self, name, ctx, call, entry_points, sets, dim, seed, scale=1.0, grow_dim=True, env=None,
                 takes_dict=False, ragged=True):
        self.name, self.ctx, self.call, self.entry_points = name, ctx, call, tuple(entry_points)
        self.sets, self.dim, self.seed, self.scale, self.grow_dim = sets, dim, seed, scale, grow_dim
        self.env, self.takes_dict, self.ragged = env or {}, takes_dict, ragged

    def data(self, variant=PLAIN):
        return Data(self, variant)

    def shape(self, variant=PLAIN):
        """(n, m, dim, total, lengths): segments of the first and of the second set, values per frame, the frames (or
        samples) of all sets together, and all the lengths in order -- host arithmetic."""
        names = list(self.sets)
        if not names:
            return 0, 0, self.dim, 0, []
        ls = {name: variant_lengths(lengths, variant) for name, (_, lengths) in self.sets.items()}
        n = len(ls[names[0]])
        m = len(ls[names[1]]) if len(names) > 1 else 0
        dim = self.dim * (variant.grow if self.grow_dim else 1)
        every = [f for name in names for f in ls[name]]
        return n, m, dim, sum(every), every

    def run(self, engine, variant=PLAIN, **kw):
        old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        try:
            with Handles() as h:
                out = self.call(engine, self.data(variant), h, **kw)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        outs, route = out if isinstance(out, tuple) and len(out) == 2 and isinstance(out[1], dict) else (out, {})
        return tuple(np.array(x) for x in outs), route


def dirty_run(engine, probe, variant):
    """A prelude's run of a probe: the outputs are dropped, a refusal is as good as an answer."""
    try:
        probe.run(engine, variant)
    except SsymError:
        pass


def route_of(e):
    tm = e.timings()
    return {k: tm[k] for k in ROUTE_KEYS}


def _sets(e, D, h, dictionary=None, src="src", tgt="tgt"):
    if dictionary is None:
        sf, so = D.flat(src, e.np_dtype)
        dictionary = h.add(e.dictionary(sf, so, D.dim))
    tf, to = D.flat(tgt, e.np_dtype)
    return dictionary, h.add(e.queries(tf, to, D.dim))


def _edge_distances(m, lo, hi, far, seed=0xD157):
    d = np.random.default_rng(seed).uniform(lo, hi, size=m)
    for i, v in enumerate([NAN, INF, -INF, far]):
        if i + 1 < m:
            d[i + 1] = v
    return d


# -- the search -------------------------------------------------------------------------------------------------------
def _search(e, D, h, dictionary=None):
    d, q = _sets(e, D, h, dictionary)
    idx, cost = e.match(d, q)
    return (idx, cost), route_of(e)


def _search_distances(e, D, h, dictionary=None):
    d, q = _sets(e, D, h, dictionary)
    far = 1e6 if e.metric == "dtw" else 1e301
    idx, cost = e.match(d, q, _edge_distances(q.n, 0.0, 60.0 if e.metric == "dtw" else 1.2, far), index_base=3)
    return (idx, cost), route_of(e)


def _topk(k):
    def call(e, D, h, dictionary=None):
        d, q = _sets(e, D, h, dictionary)
        idx, cost = e.match_topk(d, q, k)
        return (idx, cost), route_of(e)
    return call


def _match_one(e, D, h, dictionary=None):
    d, _ = _sets(e, D, h, dictionary)
    outs = []
    for t, dist in zip(D["tgt"], (0.0 if e.metric == "dtw" else 1.0, 7.5 if e.metric == "dtw" else 0.4)):
        i, c = e.match_one(d, t.astype(e.np_dtype), dist)
        outs += [np.array([i], dtype=np.uint32), np.array([c])]
    return tuple(outs), route_of(e)


def _batches(counts, with_distance):
    """ssym_match_batch on the first counts[0], counts[1], ... targets: either side of the few-targets shortcut."""
    def call(e, D, h, dictionary=None):
        sf, so = D.flat("src", e.np_dtype)
        d = dictionary if dictionary is not None else h.add(e.dictionary(sf, so, D.dim))
        outs, routes = [], {}
        for c in counts:
            c = c * D.variant.grow
            tf, to = pack_segments(D["tgt"][:c], D.dim, e.np_dtype)
            dist = _edge_distances(c, 0.0, 60.0 if e.metric == "dtw" else 1.2, 1e6) if with_distance else None
            idx, cost = e.match_batch(d, tf, to, dist)
            tm = e.timings()
            outs += [idx, cost]
            routes.update({"%s/%d" % (k, c): tm[k] for k in ROUTE_KEYS})
            routes["packed/%d" % c] = int(tm["pack_ms"] > 0)
        return tuple(outs), routes
    return call


def _pruned_step(e, D, h, dictionary=None):
    """ssym_match_candidates -> ssym_match_begin_pruned -> ssym_match_finish, then the one-call pruned search."""
    import torch
    d, q = _sets(e, D, h, dictionary)
    dev = torch.device("cuda", e.device)
    cand = torch.full((q.n,), -1.0, dtype=torch.float64, device=dev)
    bounds = torch.full((q.n,), -1.0, dtype=torch.float64, device=dev)
    oi = torch.full((q.n,), 12345, dtype=torch.int32, device=dev)
    oc = torch.full((q.n,), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)                      # (the fills ran on torch's stream, the library writes on its own)
    e.match_candidates(d, q, cand)
    e.match_begin_pruned(d, q, bounds, cand, index_base=2)
    pruned = e.timings()["pruned"]
    e.match_finish(bounds, oi, oc)
    route = route_of(e)
    route["begin_pruned"] = pruned
    e.synchronize()
    step = (oi.cpu().numpy().view(np.uint32), oc.cpu().numpy(), bounds.cpu().numpy(), cand.cpu().numpy())
    idx, cost = e.match(d, q, prune=True)
    route["call_pruned"] = e.timings()["pruned"]
    return step + (idx, cost), route


def _begin_finish(e, D, h, dictionary=None):
    import torch
    d, q = _sets(e, D, h, dictionary)
    dev = torch.device("cuda", e.device)
    bounds = torch.full((q.n,), -1.0, dtype=torch.float64, device=dev)
    oi = torch.full((q.n,), 12345, dtype=torch.int32, device=dev)
    oc = torch.full((q.n,), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    e.match_begin(d, q, bounds, distance=_edge_distances(q.n, 0.0, 60.0, 1e6), index_base=1)
    e.match_finish(bounds, oi, oc)
    route = route_of(e)
    e.synchronize()
    return (oi.cpu().numpy().view(np.uint32), oc.cpu().numpy(), bounds.cpu().numpy()), route


CHAIN_DISTANCES = {"dtw": [20.0, 35.0, 0.0, 50.0, 27.5], "refcos": [0.9, 1.1, 0.8, 1.2, 1.0]}


def _chain(append):
    def call(e, D, h, dictionary=None):
        src = D["src"]
        if dictionary is not None:
            d = dictionary
        elif append:                                     # a prefix, its self-similarities built by a chain, then the rest
            cut = max(len(src) // 2, 1)
            d = h.add(e.dictionary(*pack_segments(src[:cut], D.dim, e.np_dtype), D.dim))
            e.chain(d, D["start"][0].astype(e.np_dtype), CHAIN_DISTANCES[e.metric][:2])
            e.dictionary_append(d, *pack_segments(src[cut:], D.dim, e.np_dtype))
        else:
            d = h.add(e.dictionary(*D.flat("src", e.np_dtype), D.dim))
        idx, cost = e.chain(d, D["start"][0].astype(e.np_dtype), CHAIN_DISTANCES[e.metric])
        return (idx, cost)
    return call


def _pair_matrix(e, D, h, dictionary=None):
    d, q = _sets(e, D, h, dictionary)
    if e.metric == "dtw":
        return (e.pair_matrix(d, q, exact=False), e.pair_matrix(d, q, exact=True))
    return (e.pair_matrix(d, q, exact=True),)


# -- the wavefront family ---------------------------------------------------------------------------------------------
def _pairs(D):
    return np.arange(len(D.lengths["src"]), dtype=np.uint32)


def _align(step):
    def call(e, D, h):
        d, q = _sets(e, D, h)
        cost, length, paths, maps = e.dtw_align(d, q, _pairs(D), step=step)
        return (cost, length, np.concatenate([np.zeros((0, 2), dtype=np.uint32)] + [np.asarray(x).reshape(-1, 2) for x in paths]),
                np.concatenate([np.zeros(0, dtype=np.uint32)] + [np.asarray(x).reshape(-1) for x in maps]))
    return call


def _all_pairs(D):
    n, m = len(D.lengths["src"]), len(D.lengths["tgt"])
    return np.repeat(np.arange(n, dtype=np.uint32), m), np.tile(np.arange(m, dtype=np.uint32), n)


SPOT_K = 3


def spot_limit(costs):
    """The one threshold of the occurrences: the median of the pairs' finite best costs (it admits some)."""
    fin = costs[np.isfinite(costs)]
    return float(np.median(fin)) if fin.size else 0.0


def _spot(step):
    def call(e, D, h):
        d, q = _sets(e, D, h)
        src, tgt = _all_pairs(D)
        cost, start, end = e.dtw_spot(d, q, src, tgt, step=step)
        qi, qc, qs, qe = e.spot_queries(d, q, index_base=4, step=step)
        count, ac, as_, ae = e.dtw_spot_all(d, q, src, tgt, max_spots=SPOT_K, max_cost=spot_limit(cost), step=step)
        return (cost, start, end, qi, qc, qs, qe, count, ac, as_, ae)
    return call


SPOTTER_CUTS = (0, 1, 71, 200)           # pushes of 1, 70 and 129 rows
SPOTTER_RESET_LANE, SPOTTER_RESET_AFTER = 1, 1


def spotter_cuts(frames, grow=1):
    return [min(c * grow, frames) for c in SPOTTER_CUTS[:-1]] + [frames]


def _spotter(step):
    def call(e, D, h):
        tf, to = D.flat("tgt", e.np_dtype)
        q = h.add(e.queries(tf, to, D.dim))
        lanes = D["src"]
        sp = h.add(e.spotter(q, len(lanes), step=step))
        cuts = [spotter_cuts(x.shape[0], D.variant.grow) for x in lanes]
        outs = []
        for p in range(len(SPOTTER_CUTS) - 1):
            chunks = [x[c[p]:c[p + 1]] for x, c in zip(lanes, cuts)]
            off = np.concatenate([[0], np.cumsum([c.shape[0] for c in chunks])])
            n, pd, ps = sp.push(np.concatenate(chunks), off, want_profile=True)
            outs += [np.array([n])] + pd + ps + list(sp.events()) + list(sp.best())
            if p == SPOTTER_RESET_AFTER:
                sp.reset(SPOTTER_RESET_LANE)
        outs.append(sp.counts())
        for lane in range(len(lanes)):
            outs += [np.array([sp.flush(lane)])] + list(sp.events())
        outs += list(sp.best())
        return tuple(outs)
    return call


# -- analysis, reconstruction, partition, merge -----------------------------------------------------------------------
def _mfcc(e, D, h):
    outs = []
    for i, x in enumerate(D["snd"]):
        m, mean = e.mfcc(x, RATE, (12, 40)[i % 2], want_mean=True)
        outs += [m, mean]
    return tuple(outs)


def _mfcc_batch(e, D, h):
    x, off = D.samples("snd")
    feats, fo, mean = e.mfcc_batch(x, off, RATE, 12, want_mean=True)
    return (feats, fo, mean)


def _sequence(e, D, h):
    f, off = D.flat("blk")
    dist, mean, sim = e.sequence_distances(f, off, D.dim, want_mean=True, want_sim=True)
    return (dist, mean, sim)


def _descriptors(e, D, h):
    x, off = D.samples("snd")
    mp, pc = e.sound_descriptors(x, off, RATE)
    mv, pv = e.sound_descriptors(x, off, RATE, voiced_only=True)
    return (mp, pc, mv, pv) + tuple(e.pitch_track(x, off, RATE))


STREAM_CUTS = (0, 1500, 2530, 2530)      # pushes of 1500, 1030, 0 and the rest (3470 of 6000 samples)


def _stream(e, D, h):
    lanes = D["snd"]
    g = D.variant.grow
    st = h.add(e.stream(len(lanes), RATE, 12))
    cuts = [[min(c * g, x.size) for c in STREAM_CUTS] + [x.size] for x in lanes]
    outs = []
    for p in range(len(STREAM_CUTS)):
        chunks = [x[c[p]:c[p + 1]] for x, c in zip(lanes, cuts)]
        off = np.concatenate([[0], np.cumsum([c.size for c in chunks])])
        new, frames = st.push(np.concatenate(chunks), off, want_frames=True)
        outs += [new, frames]
    outs += list(st.counts()) + [st.read(l) for l in range(len(lanes))] + list(st.descriptors())
    if e.metric == "dtw":       # a spotter follows the stream's resident frames in place
        tf, to = D.flat("tgt", e.np_dtype)
        q = h.add(e.queries(tf, to, D.dim))
        sp = h.add(e.spotter(q, len(lanes)))
        outs += [np.array([sp.follow(st)])] + list(sp.events()) + list(sp.best())
    st.reset(0)                                               # the lane starts again: nothing of the old sound is left
    again = lanes[0][:1100 * g]
    st.push(again, [0] + [again.size] * len(lanes))
    outs += list(st.counts()) + [st.read(0)] + list(st.descriptors())
    one = h.add(e.stream(1, RATE, 12))                        # a seeded lane: the next push analyses what the seed left
    one.seed(0, lanes[1])
    outs += [one.push(np.zeros(0), [0, 0]), one.read(0)] + list(one.descriptors())
    return tuple(outs)


RECON_IDX = (1, 3, 0, 5)
HOP = 256


def recon_maps(D):
    """(idx, out offsets, maps, map offsets, map frames, pair_len) of the four matches: maps over any u32 values (the
    header: no map content can cause an out-of-range read), one pair without a path (pair_len 0: the length fit)."""
    sounds, out_len = D["snd"], D.lengths["out"]
    idx = np.array([RECON_IDX[t % len(RECON_IDX)] for t in range(len(out_len))], dtype=np.uint32)
    rng = np.random.default_rng(0x3A95 + sum(out_len))
    ooff = np.concatenate([[0], np.cumsum(out_len)]).astype(np.uint64)
    frames = np.array([max(n // HOP, 1) for n in out_len], dtype=np.uint32)
    moff = np.concatenate([[0], np.cumsum(frames + 2)]).astype(np.uint64)       # (two slack slots per target)
    maps = np.zeros(int(moff[-1]), dtype=np.uint32)
    for t, f in enumerate(frames):
        s_frames = sounds[int(idx[t])].size // HOP + 2
        base = np.arange(f) * s_frames // max(int(f), 1)
        maps[int(moff[t]):int(moff[t]) + f] = np.clip(base + rng.integers(-1, 2, size=f), 0, s_frames)
    pair_len = frames.copy()
    pair_len[1] = 0
    return idx, ooff, maps, moff, frames, pair_len


WSOLA_SEARCH = 40


def _reconstruct(e, D, h):
    x, off = D.samples("snd")
    smp = h.add(e.samples(x, off))
    idx, ooff, maps, moff, frames, pair_len = recon_maps(D)
    out, pcm = e.reconstruct(smp, idx, ooff, want_pcm32=True)
    w, wpcm = e.reconstruct_warped(smp, idx, ooff, maps, moff, frames, pair_len, want_pcm32=True)
    s, spcm, pos = e.reconstruct_wsola(smp, idx, ooff, maps, moff, frames, pair_len, search=WSOLA_SEARCH, want_pcm32=True,
                                       want_pos=True)
    return (out, pcm, w, wpcm, s, spcm, pos)


GMM_K = 8


def gmm_rows(n):
    return np.sort(np.random.default_rng(0x6A1).choice(n, size=GMM_K, replace=False)).astype(np.uint64)


def _partition(e, D, h):
    train, other = D["trn"][0], np.concatenate(D["oth"])
    std = e.standardize(train, D.dim)
    g = h.add(e.gmm_train(train, D.dim, gmm_rows(train.shape[0]), max_iters=5))
    letters, post = e.gmm_predict(g, other, want_post=True)
    seg = e.partition(g, other)
    vseg, votes = e.vote_segments(letters, GMM_K, want_votes=True)
    return (std, g.weights, g.means, g.covs, np.array([g.log_lik]), np.array([g.iters]), letters, post, seg, vseg, votes)


MERGE_SHARDS, MERGE_TARGETS = 3, 7


def merge_inputs(variant):
    rng = np.random.default_rng(0x3E6)
    g, m = MERGE_SHARDS * variant.grow, MERGE_TARGETS * variant.grow
    costs = rng.integers(0, 5, size=(g, m)).astype(np.float64)              # small integers: ties between the shards
    if variant.fill is not None:
        costs[:] = {"nan": NAN, "inf": INF, "big": 1e300, "same": 1.0}[variant.fill]
    idx = rng.integers(0, 1000, size=(g, m)).astype(np.int32)
    dist = rng.integers(0, 5, size=m).astype(np.float64)
    return costs, idx, dist


def _merge(e, D, h):
    import torch
    costs, idx, dist = merge_inputs(D.variant)
    dev = torch.device("cuda", e.device)
    c, i = torch.from_numpy(costs).to(dev), torch.from_numpy(idx).to(dev)
    g, m = costs.shape
    outs = []
    for which in ("plain", "at_none", "at"):
        oi = torch.full((m,), 12345, dtype=torch.int32, device=dev)
        oc = torch.full((m,), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        if which == "plain":
            nat.check(nat.lib().ssym_merge_shards(e.ctx, g, m, c.data_ptr(), i.data_ptr(), oi.data_ptr(), oc.data_ptr()), e.ctx)
        else:
            e.merge_shards(c, i, oi, oc, dist if which == "at" else None)
        e.synchronize()
        outs += [oi.cpu().numpy(), oc.cpu().numpy()]
    return tuple(outs)


# -- the probes -------------------------------------------------------------------------------------------------------
def _sigma(dim):
    return 4.0 / (1.0 + np.arange(dim, dtype=np.float64))


SRC33 = [(7 * i + 64) % 65 for i in range(33)]            # 0 ... 64 frames, one empty (i = 28); 33 pad to 64 slots
TGT65 = [(11 * i + 3) % 65 for i in range(65)]            # every length 0 ... 64 once
SRC_LONG = [130, 97, 130, 64, 129, 130, 33, 1]            # 130 frames: several row passes of the filter
TGT5 = [20, 33, 5, 64, 47]
SRC_BAND = [64 - (i % 5) for i in range(16)]              # 16 x 33 x 64 frames, lengths within the band of each other
TGT_BAND = [64 - (i % 7) for i in range(33)]              # 33 targets pad to 256 slots in the banded filter
SRC_WIDE = [40 - (i % 11) for i in range(20)]             # 64-value frames: the lower-bound cascade
TGT_WIDE = [40 - (3 * i % 9) for i in range(12)]
SRC_FEW = [3 + (5 * i) % 18 for i in range(100)]          # 100 sources of 3 ... 20 frames
TGT_FEW = [20, 7, 13, 3, 16]                              # 4 targets: the one-launch kernel; 5: packed
SRC_PRUNE = [10 + (7 * i) % 21 for i in range(96)]
TGT_PRUNE = [10 + (5 * i) % 21 for i in range(40)]
ALIGN_SRC, ALIGN_TGT = [64, 65, 257], [64, 130, 256]      # (257, 256): past the 16 KiB of LDS directions, the slab
PACED_SRC, PACED_TGT = [64, 65, 257, 10], [64, 130, 256, 64]      # (10, 64): no slope-bounded path
SPOT_SRC, SPOT_TGT = [130, 300], [5, 65]
WATCH_TGT, WATCH_LANES = [1, 65, 0], [200, 187]
SRC_R70 = [1 + (7 * i) % 30 for i in range(70)]           # 70 x 45 ragged 1 ... 30 frames (3 150 pairs: the tile kernel)
TGT_R45 = [1 + (11 * i) % 30 for i in range(45)]
SRC_R300 = [1 + (7 * i) % 30 for i in range(300)]         # 300 x 220 = 66 000 pairs: from 65 536 on the filters take it
TGT_R220 = [1 + (11 * i) % 30 for i in range(220)]
SRC_R129 = [1 + (5 * i) % 30 for i in range(129)]
TGT_R5 = [30, 1, 17, 8, 25]
TGT_R65 = [1 + (3 * i) % 8 for i in range(65)]            # 64 queries: refcos_match_one_kernel; 65: packed


def _unholdable(e, D, h, dictionary=None):
    """Values the integer records cannot hold: one source beyond 2^120, one with a NaN -- the f64 filter takes the set."""
    src = [s.copy() for s in D["src"]]
    if D.variant.fill is None:
        src[5] *= 1e40
        src[9][0, 3] = NAN
    sf, so = pack_segments(src, D.dim, e.np_dtype)
    d = h.add(e.dictionary(sf, so, D.dim))
    tf, to = D.flat("tgt", e.np_dtype)
    idx, cost = e.match(d, h.add(e.queries(tf, to, D.dim)))
    return (idx, cost), route_of(e)


F = "frames"
S = "samples"
SEARCH_EP = ("ssym_match_queries",)


def _probe_list():
    dtw = lambda name, call, ep, src, tgt, seed, **kw: Probe(name, kw.pop("ctx", DTW64), call, ep, {"src": (F, src), "tgt": (F, tgt)},
                                                             kw.pop("dim", 13), seed, scale=kw.pop("scale", _sigma(13)), **kw)
    ref = lambda name, call, ep, src, tgt, seed, **kw: Probe(name, REFCOS, call, ep, {"src": (F, src), "tgt": (F, tgt)}, 12, seed,
                                                             scale=0.3, **kw)
    return [
        # dtw context: the search
        dtw("dtw_search", _search, SEARCH_EP, SRC33, TGT65, 0x4101, takes_dict=True),
        dtw("dtw_search_f32", _search, SEARCH_EP, SRC33, TGT65, 0x4102, ctx=DTW32, takes_dict=True),
        dtw("dtw_long_rows", _search, SEARCH_EP, SRC_LONG, TGT5, 0x4103, takes_dict=True),
        dtw("dtw_band8", _search, SEARCH_EP, SRC_BAND, TGT_BAND, 0x4104, ctx=BAND8, takes_dict=True),
        dtw("dtw_wide64", _search, SEARCH_EP, SRC_WIDE, TGT_WIDE, 0x4105, dim=64, scale=_sigma(64), takes_dict=True),
        dtw("dtw_distances", _search_distances, SEARCH_EP, SRC33, TGT65, 0x4101, takes_dict=True),
        dtw("dtw_topk3", _topk(3), ("ssym_match_topk",), SRC33, TGT65, 0x4101, takes_dict=True),
        dtw("dtw_topk64", _topk(64), ("ssym_match_topk",), SRC33, TGT65, 0x4101, takes_dict=True),
        dtw("dtw_match_one", _match_one, ("ssym_match_one",), SRC33, [40, 9], 0x4106, takes_dict=True),
        dtw("dtw_few_batch", _batches((4, 5), False), ("ssym_match_batch",), SRC_FEW, TGT_FEW, 0x4107, ctx=DTW32, takes_dict=True),
        dtw("dtw_match_batch", _batches((65,), True), ("ssym_match_batch",), SRC33, TGT65, 0x4101, takes_dict=True),
        dtw("dtw_pruned_step", _pruned_step, ("ssym_match_candidates", "ssym_match_begin_pruned", "ssym_match_finish",
                                              "ssym_match_queries"), SRC_PRUNE, TGT_PRUNE, 0x4108, takes_dict=True),
        dtw("dtw_begin_finish", _begin_finish, ("ssym_match_begin", "ssym_match_finish"), SRC33, TGT65, 0x4101, takes_dict=True),
        Probe("dtw_chain", DTW64, _chain(False), ("ssym_chain",), {"src": (F, [f or 9 for f in SRC33]), "start": (F, [40])}, 13,
              0x4109, scale=_sigma(13), takes_dict=True),
        dtw("dtw_pair_matrix", _pair_matrix, ("ssym_pair_matrix",), SRC33, TGT65, 0x4101, takes_dict=True),
        # dtw context: the wavefront family
        dtw("align", _align("symmetric"), ("ssym_dtw_align", "ssym_dtw_align_sizes"), ALIGN_SRC, ALIGN_TGT, 0x4201),
        dtw("align_lds", _align("symmetric"), ("ssym_dtw_align",), [64, 31], [64, 60], 0x4202),
        dtw("align_slab", _align("symmetric"), ("ssym_dtw_align",), [257, 300], [256, 290], 0x4203),
        dtw("align_paced", _align("paced"), ("ssym_dtw_align_step",), PACED_SRC, PACED_TGT, 0x4201),
        dtw("align_band6", _align("symmetric"), ("ssym_dtw_align",), ALIGN_SRC, [64, 67, 256], 0x4204, ctx=BAND6),
        dtw("spot_sym", _spot("symmetric"), ("ssym_dtw_spot", "ssym_spot_queries", "ssym_dtw_spot_all"), SPOT_SRC, SPOT_TGT, 0x4205),
        dtw("spot_paced", _spot("paced"), ("ssym_dtw_spot_step", "ssym_spot_queries_step", "ssym_dtw_spot_all_step"), SPOT_SRC,
            SPOT_TGT, 0x4205),
        dtw("spotter_sym", _spotter("symmetric"), ("ssym_spotter_push", "ssym_spotter_events", "ssym_spotter_flush",
                                                   "ssym_spotter_best", "ssym_spotter_reset"), WATCH_LANES, WATCH_TGT, 0x4206),
        dtw("spotter_paced", _spotter("paced"), ("ssym_spotter_push", "ssym_spotter_events", "ssym_spotter_flush",
                                                 "ssym_spotter_best", "ssym_spotter_reset"), WATCH_LANES, WATCH_TGT, 0x4206),
        # refcos context
        ref("refcos_70x45", _search, SEARCH_EP, SRC_R70, TGT_R45, 0x4301, takes_dict=True),
        ref("refcos_q8", _search, SEARCH_EP, SRC_R300, TGT_R220, 0x4302, takes_dict=True),
        ref("refcos_f64", _search, SEARCH_EP, SRC_R300, TGT_R220, 0x4302, env={"SSYM_REFCOS_Q8": "0"}, takes_dict=True),
        ref("refcos_tile", _search, SEARCH_EP, SRC_R129, TGT_R5, 0x4303, takes_dict=True),
        ref("refcos_unholdable", _unholdable, SEARCH_EP, SRC_R300, TGT_R220, 0x4302),
        ref("refcos_distances", _search_distances, SEARCH_EP, SRC_R300, TGT_R220, 0x4302, takes_dict=True),
        ref("refcos_topk8", _topk(8), ("ssym_match_topk",), SRC_R300, TGT_R220, 0x4302, takes_dict=True),
        ref("refcos_match_one", _match_one, ("ssym_match_one",), SRC_R70, [30, 4], 0x4304, takes_dict=True),
        ref("refcos_few_batch", _batches((64, 65), False), ("ssym_match_batch",), SRC_R70, TGT_R65, 0x4305, takes_dict=True),
        Probe("refcos_chain", REFCOS, _chain(False), ("ssym_chain",), {"src": (F, SRC_R70), "start": (F, [17])}, 12, 0x4306,
              scale=0.3, takes_dict=True),
        Probe("refcos_chain_append", REFCOS, _chain(True), ("ssym_chain", "ssym_dict_append"),
              {"src": (F, SRC_R70), "start": (F, [17])}, 12, 0x4306, scale=0.3),
        ref("refcos_pair_matrix", _pair_matrix, ("ssym_pair_matrix",), SRC_R70, TGT_R45, 0x4301, takes_dict=True),
        # either context (here: the dtw one, which warped reconstruction and the spotter that follows a stream need)
        Probe("mfcc", DTW64, _mfcc, ("ssym_mfcc",), {"snd": (S, [6000, 4500])}, 1, 0x4401, grow_dim=False),
        Probe("mfcc_batch", DTW64, _mfcc_batch, ("ssym_mfcc_batch",), {"snd": (S, [0, 1023, 5000])}, 1, 0x4402, grow_dim=False),
        Probe("sequence", DTW64, _sequence, ("ssym_sequence_distances",), {"blk": (F, [5, 0, 35])}, 12, 0x4403, scale=2.0),
        Probe("descriptors", DTW64, _descriptors, ("ssym_sound_descriptors", "ssym_pitch_track"),
              {"snd": (S, [9000, 1500, 5000])}, 1, 0x4404, grow_dim=False),
        Probe("stream", DTW64, _stream, ("ssym_stream_push", "ssym_stream_read", "ssym_stream_descriptors", "ssym_stream_reset",
                                         "ssym_stream_seed", "ssym_spotter_follow"),
              {"snd": (S, [6000, 5200]), "tgt": (F, [5, 9])}, 12, 0x4405, grow_dim=False),
        Probe("reconstruct", DTW64, _reconstruct, ("ssym_reconstruct", "ssym_reconstruct_warped", "ssym_reconstruct_wsola"),
              {"snd": (S, [3000, 5000, 2100, 4096, 1, 2600]), "out": ("lengths", [2500, 4096, 3100, 2000])}, 1, 0x4406,
              grow_dim=False),
        Probe("partition", DTW64, _partition, ("ssym_standardize", "ssym_gmm_train", "ssym_gmm_predict", "ssym_partition",
                                               "ssym_vote_segments"),
              {"trn": (F, [300]), "oth": (F, [170, 130])}, 12, 0x4407, scale=2.0, grow_dim=False),
        Probe("merge", DTW64, _merge, ("ssym_merge_shards", "ssym_merge_shards_at"), {}, 1, 0x4408, grow_dim=False, ragged=False),
    ]


PROBES = {p.name: p for p in _probe_list()}

# the sequence probe's offsets are [0, 5, 5, 40]
assert np.cumsum([0] + PROBES["sequence"].sets["blk"][1]).tolist() == [0, 5, 5, 40]


def by_ctx():
    """ctx key -> (ctx, the probes that run on it), in the order of the list."""
    out = {}
    for p in PROBES.values():
        out.setdefault(ctx_key(p.ctx), (p.ctx, []))[1].append(p)
    return out


# -- preludes ---------------------------------------------------------------------------------------------------------
def _twin(fill):
    return lambda e, probe: dirty_run(e, probe, twin(fill))


def _larger(fill):
    return lambda e, probe: dirty_run(e, probe, larger(fill))


def refused_calls(e, probe=None):
    """Calls that the library refuses after part of their host work; returns what each answered.  Every one must be a
    refusal (the test asserts it): decreasing offsets in the second set, k = 0, an unknown step, a paced target of 2049
    frames, a lane out of range."""
    dim = 12
    rng = np.random.default_rng(0x4EF)
    got = {}

    def refusal(what, fn):
        try:
            fn()
            got[what] = None
        except (SsymError, ValueError) as err:
            got[what] = err

    with Handles() as h:
        feats = rng.normal(size=(40, dim)).astype(e.np_dtype)
        d = h.add(e.dictionary(feats, [0, 10, 25, 40], dim))
        q = h.add(e.queries(feats, [0, 20, 40], dim))
        refusal("decreasing offsets", lambda: h.add(e.queries(feats, [0, 30, 20, 40], dim)))
        refusal("k = 0", lambda: e.match_topk(d, q, 0))
        pair = np.zeros(1, dtype=np.uint32)
        out = np.zeros(4)
        u32 = np.zeros(4, dtype=np.uint32)
        refusal("unknown step", lambda: nat.check(nat.lib().ssym_dtw_spot_step(
            e.ctx, d.ptr, q.ptr, pair.ctypes.data, pair.ctypes.data, 1, 0, 99, out.ctypes.data, u32.ctypes.data,
            u32.ctypes.data, 0), e.ctx))
        long_q = h.add(e.queries(rng.normal(size=(2049, dim)).astype(e.np_dtype), [0, 2049], dim))
        refusal("paced target of 2049 frames", lambda: h.add(e.spotter(long_q, 1, step="paced")))
        st = h.add(e.stream(2, RATE, 12))
        refusal("lane out of range", lambda: nat.check(nat.lib().ssym_stream_reset(e.ctx, st.ptr, 7), e.ctx))
    return got


def unfinished_begin(e, probe=None):
    """A ssym_match_begin that is never finished: its handles are closed, its pending step is left behind (the header: any
    other matching call on the context ends the pair)."""
    import torch
    rng = np.random.default_rng(0xBE61)
    dim = 13
    with Handles() as h:
        src = [rng.normal(size=(int(f), dim)) * _sigma(dim) for f in rng.integers(5, 40, size=96)]
        tgt = [rng.normal(size=(int(f), dim)) * _sigma(dim) for f in rng.integers(5, 40, size=40)]
        d = h.add(e.dictionary(*pack_segments(src, dim, e.np_dtype), dim))
        q = h.add(e.queries(*pack_segments(tgt, dim, e.np_dtype), dim))
        bounds = torch.zeros(40, dtype=torch.float64, device=torch.device("cuda", e.device))
        torch.cuda.synchronize()
        e.match_begin(d, q, bounds, distance=np.linspace(0.0, 50.0, 40))
        e.synchronize()


def used_dictionary(e, probe, h):
    """The probe's own dictionary, not new: grown by ssym_dict_append from a prefix after that prefix was searched, and
    then matched against queries scaled x 300 and x 1e-3 (its filter records are rebuilt at another scale), searched
    with top-k and pruned (centroids)."""
    D = probe.data()
    src = D["src"]
    cut = max(len(src) // 2, 1)
    d = h.add(e.dictionary(*pack_segments(src[:cut], D.dim, e.np_dtype), D.dim))
    second = [name for name in probe.sets if name != "src"][0]
    with Handles() as mine:
        for scale in (300.0, 1e-3):
            q = mine.add(e.queries(*pack_segments([t * scale for t in D[second]], D.dim, e.np_dtype), D.dim))
            e.match(d, q)
            if scale == 300.0:
                e.dictionary_append(d, *pack_segments(src[cut:], D.dim, e.np_dtype))
            e.match_topk(d, q, 5)
            if e.metric == "dtw":
                e.match(d, q, prune=True)
    return d


PRELUDES = {}
for _fill in FILLS:
    PRELUDES["twin_" + _fill] = _twin(_fill)
PRELUDES["larger_nan"] = _larger("nan")
PRELUDES["larger_same"] = _larger("same")
PRELUDES["refused"] = refused_calls
PRELUDES["unfinished"] = unfinished_begin

# "other route first": the first probe runs on its own data, then the second is held to its fresh answer -- both orders
OTHER_ROUTES = [
    ("dtw_topk64", "dtw_search"),                # top-k 64 before k = 1
    ("refcos_topk8", "refcos_q8"),
    ("dtw_pruned_step", "dtw_search"),           # pruned before plain
    ("dtw_distances", "dtw_search"),             # with distances before without
    ("refcos_distances", "refcos_q8"),
    ("align_paced", "align"),                    # paced before symmetric
    ("spot_paced", "spot_sym"),
    ("spotter_paced", "spotter_sym"),
    ("align_slab", "align_lds"),                 # an alignment that needs the slab before one in LDS
    ("dtw_match_one", "dtw_search"),             # ssym_match_one before a batched search
    ("refcos_match_one", "refcos_q8"),
    ("refcos_f64", "refcos_q8"),                 # the f64 filter before the integer one
]

# ssym_* calls no probe has to run: lifecycle and accessors, the communicator family (sharded search is out of scope)
LIFECYCLE = {
    "ssym_abi_version", "ssym_last_error", "ssym_ctx_create", "ssym_ctx_destroy", "ssym_ctx_synchronize", "ssym_get_timings",
    "ssym_dict_create", "ssym_dict_create_device", "ssym_dict_size", "ssym_dict_destroy",
    "ssym_queries_create", "ssym_queries_create_device", "ssym_queries_destroy",
    "ssym_samples_create", "ssym_samples_destroy", "ssym_gmm_get", "ssym_gmm_destroy",
    "ssym_stream_create", "ssym_stream_destroy", "ssym_stream_counts", "ssym_stream_frames_device", "ssym_stream_samples_device",
    "ssym_spotter_create", "ssym_spotter_create_step", "ssym_spotter_destroy", "ssym_spotter_counts",
    "ssym_mfcc_num_frames", "ssym_pitch_num_windows",
    "ssym_comm_unique_id", "ssym_comm_create", "ssym_comm_create_local", "ssym_comm_destroy", "ssym_comm_available",
    "ssym_comm_set_timeout", "ssym_comm_is_dead", "ssym_comm_inject_fault", "ssym_comm_replay_bounds",
    "ssym_local_group_create", "ssym_local_group_destroy", "ssym_match_sharded",
}
