"""Inputs on which a target's two nearest keys lie closer than the dtw filter resolves (TEST INFRASTRUCTURE ONLY, CPU).

The dtw search scores every pair with the f16-split MFMA filter into an f32 matrix, keeps the pairs whose key interval
can still hold the first minimum (csrc/certify.hip, csrc/select.hip, csrc/dtw_margin.hpp) and re-scores those in f64.
Where two keys of a target lie closer than the filter resolves, its order is noise, and only the margin and the exact
re-scoring give the right index.  The cases here are built so that a wrong selection gives a wrong ANSWER.

    gap     of a target: the difference of its two smallest unequal keys |cost - distance| (topk_ref.keys), relative to
            the larger of those two keys and the two costs behind them -- topk_ref.assert_separated's scale
    blind   1e-9 < gap < 2^-25: above the suite's separation floor, below half an ulp of the filter's f32 matrix
    inside  2^-25 <= gap < the pair's filter bound (bounds.pair_bound_matrix) / cost: the intervals overlap
    resolved gap >= 1e-2: a control (inside ends there at the latest)
    reach   frames wider than the filter's 42 values, twins equal in values 0...41: the filter is blind whatever the gap

How contenders are made (every perturbation is calibrated against oracle.dtw, grown or shrunk until the oracle's gap
lands in the wanted range; the same seed gives the same bits):
    twins   of a target's planted source: f32 sets move some values by 2^b units in the last place (b = 0: the last
            mantissa bit), f64 sets multiply them by 1 +- 2^(b-30); first more values, then a higher bit
    riders  targets without a planted neighbour: unrelated segments, re-drawn until the twins of their nearest source --
            calibrated for another target -- give them a gap on a rung
    quads   a planted source with three twins, all six gaps of the four in one range (top-k)
    tied    no twin: the per-target distance lies between two costs adjacent in the target's sorted column, nudged so
            that the two keys differ by a rung's gap; the smaller key on either side in equal shares

Sources are laid out as whole blocks [originals | twins 1 | twins 2 (| twins 3)]: a set split into shards has every
near-tie across a shard boundary, and which contender is nearer is decided per target.  Twins 2 of the first-minimum
cases lie farther than both (a third, resolved contender).

Built cases are cached in-process (functools.lru_cache); no fixture is committed.
"""
import functools
import math
from dataclasses import dataclass

import numpy as np

import bounds
import topk_ref as ref
from soundsym_amd import synth

FLOOR = 1e-9                     # topk_ref.assert_separated's rel
HALF_ULP = 2.0 ** -25            # half an ulp of the filter's f32 cost matrix
RESOLVED = 1e-2
FILTER_DIM = 42                  # values of a frame the filter takes in
_LO = 2.0 * FLOOR                # what the builder aims above, so that the floor holds with room
_HI = 0.9 * HALF_ULP

# name -> how the case is built.  kind: ragged (synth.make_ragged, planted), grid (synth.make_grid), long (grids of 150
# and 300 frames); riders: targets replaced by unrelated segments; bmax: highest bit (f32) / exponent step (f64) a twin
# may be moved by; decades: the inside decades the case claims, each [d, 10 d); tied: keys tied across a distance
SPECS = {
    "sp":        dict(kind="ragged", lo=16, hi=40, n0=64, m=64, riders=8, dim=13, seed=0x5EED7101),
    "mid":       dict(kind="ragged", lo=49, hi=128, n0=48, m=64, riders=16, dim=13, seed=0x5EED7102),
    "long":      dict(kind="long", n0=32, m=32, riders=0, dim=13, seed=0x5EED7103, half=True),
    "f64":       dict(kind="ragged", lo=16, hi=40, n0=64, m=64, riders=8, dim=12, seed=0x5EED7104, dtype="f64"),
    "squared":   dict(kind="ragged", lo=16, hi=40, n0=64, m=64, riders=8, dim=13, seed=0x5EED7105, squared=True),
    "single":    dict(kind="grid", frames=30, n0=48, m=64, riders=16, dim=40, seed=0x5EED7106, bmax=11,
                      decades=(1e-7, 1e-6, 1e-5), resolved=0, far=(2e-5, 2e-4)),
    "single_b32": dict(kind="grid", frames=30, n0=48, m=64, riders=16, dim=40, seed=0x5EED7106, bmax=11, band=32,
                       decades=(1e-7, 1e-6, 1e-5), resolved=0, far=(2e-5, 2e-4)),
    "band3":     dict(kind="ragged", lo=16, hi=40, n0=64, m=64, riders=8, dim=13, seed=0x5EED7107, band=3),
    "band8":     dict(kind="ragged", lo=16, hi=40, n0=64, m=64, riders=8, dim=13, seed=0x5EED7108, band=8),
    "reach64":   dict(kind="ragged", lo=30, hi=70, n0=32, m=32, riders=0, dim=64, seed=0x5EED7109, reach=True),
    "reach100_b3": dict(kind="ragged", lo=30, hi=70, n0=32, m=32, riders=0, dim=100, seed=0x5EED710A, reach=True, band=3),
    "tied":      dict(kind="ragged", lo=16, hi=40, n0=192, m=64, riders=0, dim=13, seed=0x5EED710B, tied=True,
                      decades=(1e-7, 1e-6, 1e-5, 1e-4)),
    "tied64":    dict(kind="ragged", lo=30, hi=70, n0=144, m=64, riders=0, dim=64, seed=0x5EED710C, tied=True,
                      decades=(1e-7, 1e-6, 1e-5, 1e-4)),
    "quads":     dict(kind="ragged", lo=16, hi=40, n0=48, m=48, riders=0, dim=13, seed=0x5EED710D, quads=True, resolved=0,
                      decades=(1e-7, 1e-6, 1e-5, 1e-4)),
}
FIRST_MINIMUM = tuple(n for n, s in SPECS.items() if not s.get("quads"))
REACH_DECADES = (1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4)


@dataclass
class Case:
    name: str
    dim: int
    dtype: str
    band: int
    squared: bool
    k: int                        # the largest k the case is used with
    n0: int                       # sources per block
    blocks: int
    src: list
    tgt: list
    distance: object              # None, or [m] f64
    contenders: list              # per target: the source indices meant to tie nearly (ascending)
    rung: list                    # per target: blind / inside / resolved / reach, as MEASURED on the oracle's matrix
    gap: np.ndarray               # per target, measured
    ceiling: np.ndarray           # per target: the inside rung's upper end
    mat: np.ndarray               # the oracle's [n][m] costs
    bound: np.ndarray             # the filter's [n][m] error bound
    decades: tuple
    half: bool = False            # half the placement minimums (the long case)
    reach: bool = False
    tied: bool = False
    quads: bool = False

    @property
    def np_dtype(self):
        return np.float64 if self.dtype == "f64" else np.float32

    def nearer_is_higher(self):
        """per target: True where the contender with the smaller key sits at the higher index."""
        key = ref.keys(self.mat, self.distance, 0.0)
        out = np.zeros(len(self.tgt), dtype=bool)
        for t, c in enumerate(self.contenders):
            ks = [key[s, t] for s in c]
            out[t] = c[int(np.argmin(ks))] == max(c)
        return out

    def counts(self):
        r = np.array(self.rung)
        hi = self.nearer_is_higher()
        return {g: (int((r == g).sum()), int(((r == g) & hi).sum()), int(((r == g) & ~hi).sum()))
                for g in ("blind", "inside", "resolved", "reach") if (r == g).any()}

    def decade_counts(self):
        return {d: int(sum(1 for t, g in enumerate(self.gap) if self.rung[t] in ("inside", "reach") and d <= g < 10 * d))
                for d in self.decades}


# ---- measuring ------------------------------------------------------------------------------------------------------
def measure_gaps(mat, distance=None):
    """per target: (gap, the two sources behind it) -- the two smallest unequal keys, on assert_separated's scale."""
    key = ref.keys(mat, distance, 0.0)
    m = key.shape[1]
    gap, pair = np.full(m, np.inf), [None] * m
    for t in range(m):
        col = key[:, t]
        fin = np.flatnonzero(col < np.inf)
        order = fin[np.argsort(col[fin], kind="stable")]
        for j in range(1, order.size):
            a, b = order[0], order[j]
            if col[b] != col[a]:
                scale = max(col[a], col[b], abs(mat[a, t]), abs(mat[b, t]))
                gap[t], pair[t] = (col[b] - col[a]) / scale, (int(a), int(b))
                break
    return gap, pair


def bound_matrix(src, tgt, dim, squared):
    """the filter's [n][m] error bound: bounds.pair_bound_matrix; the squared cost's cell error (csrc/dtw_margin.hpp,
    mp.squared) restated here, since tests/bounds.py states the plain cost's only."""
    used = min(dim, FILTER_DIM)
    b, ra, rb, na, nb = bounds.pair_bound_matrix(src, tgt, used)
    if not squared:
        return b
    full = lambda a: float((np.asarray(a, dtype=np.float64) ** 2).sum(-1).max()) * 1.000002
    vmax = max(max(float(np.abs(a).max()) for a in src), max(float(np.abs(a).max()) for a in tgt)) * 1.000001
    s = bounds.common_scale(vmax, max(max(full(a) for a in src), max(full(a) for a in tgt)))
    in_a, in_b = bounds.input_rounding(used)
    tot = na[:, None] + nb[None, :]
    cell = 256 * 2.0 ** -24 * tot + 2.0 ** -12 / s ** 2 + 4.1 * max(in_a, in_b) * tot + 2.0 ** -20 / s
    fa = np.array([a.shape[0] for a in src])
    fb = np.array([a.shape[0] for a in tgt])
    return 1.02 * (fa[:, None] + fb[None, :] - 1) * cell


def classify(gap, ceiling):
    if FLOOR < gap < HALF_ULP:
        return "blind"
    if gap >= RESOLVED:
        return "resolved"
    if HALF_ULP <= gap < ceiling:
        return "inside"
    return "other"


# ---- perturbing -----------------------------------------------------------------------------------------------------
def _perturb(a, pos, b, k, st):
    """A copy of `a` with k of the flat positions `pos` moved: f32 by 2^b units in the last place, up or down; f64 by
    the factor 1 +- 2^(b-30)."""
    out = a.copy().reshape(-1)
    pick = pos[st.permutation(pos.size)[:k]]
    sgn = 1 - 2 * st.integers(pick.size, 2)
    if a.dtype == np.float64:
        out[pick] *= 1.0 + sgn * 2.0 ** (b - 30)
        return out.reshape(a.shape)
    bits = out.view(np.uint32)
    mag = (bits[pick] & np.uint32(0x7FFFFFFF)).astype(np.int64) + sgn * (1 << b)
    ok = (mag >= 0x00800000) & (mag < 0x7F000000)                  # stays a normal number
    pick, mag = pick[ok], mag[ok]
    bits[pick] = (bits[pick] & np.uint32(0x80000000)) | mag.astype(np.uint32)
    return out.reshape(a.shape)


def _calibrate(cost, a, c0, pos, lo, hi, accept, seed, bmax, trials=400):
    """A twin of `a` whose cost c1 has lo <= |c1 - c0| / max(c1, c0) < hi and accept(twin, c1).  The strength
    2^b sqrt(k) is steered to the range's geometric middle: first more values (k), then a higher bit (b)."""
    P = pos.size
    b, k = 0, max(1, P // 16)
    mid = math.sqrt(lo * hi)
    for trial in range(trials):
        tw = _perturb(a, pos, b, k, synth.Stream((seed * 0x9E3779B1 + trial) & 0xFFFFFFFFFFFF))
        c1 = cost(tw)
        g = abs(c1 - c0) / max(c1, c0)
        if lo <= g < hi:
            if accept(tw, c1):
                return tw, c1
            continue
        s = 2.0 ** b * math.sqrt(k) * min(max(mid / max(g, 1e-16), 1.0 / 64), 64.0) ** 0.6    # (damped: large moves add in quadrature)
        b = 0 if s <= math.sqrt(P) else min(bmax, int(math.ceil(math.log2(s / math.sqrt(P)))))
        k = int(min(P, max(1, round((s / 2.0 ** b) ** 2))))
    raise RuntimeError("no twin with a gap in [%g, %g) after %d trials: change the seed" % (lo, hi, trials))


# ---- base sets ------------------------------------------------------------------------------------------------------
def _base(spec):
    """(originals, planted targets, planted index per target) of the case's own dtype."""
    n0, dim, seed = spec["n0"], spec["dim"], spec["seed"]
    m0 = min(spec["m"], n0)
    if spec["kind"] == "ragged":
        src, tgt, pi = synth.make_ragged(n0, m0, spec["lo"], spec["hi"], dim, seed, planted=True)
    elif spec["kind"] == "grid":
        g = synth.make_grid(n0, m0, spec["frames"], dim, seed)
        src, tgt, pi = list(g.sources), list(g.targets), g.planted
    else:                                                    # long: 150 and 300 frames, several row passes
        g1 = synth.make_grid(n0 // 2, m0 // 2, 150, dim, seed)
        g2 = synth.make_grid(n0 // 2, m0 // 2, 300, dim, seed + 1)
        src, tgt = list(g1.sources) + list(g2.sources), list(g1.targets) + list(g2.targets)
        pi = np.concatenate([g1.planted, g2.planted + n0 // 2])
    if spec.get("dtype") == "f64":                           # values no f32 holds
        st = synth.Stream(seed ^ 0xF64)
        wob = lambda a: a.astype(np.float64) * (1.0 + 1e-9 * st.normal(a.size).reshape(a.shape))
        src, tgt = [wob(a) for a in src], [wob(a) for a in tgt]
    return src, tgt, np.asarray(pi, dtype=np.int64)


def _matrix(oracle, src, tgt, spec):
    from oracle.oracle import pack_segments
    sf, so = pack_segments([a.astype(np.float64) for a in src], spec["dim"])
    tf, to = pack_segments([a.astype(np.float64) for a in tgt], spec["dim"])
    return oracle.dtw_match_all(sf, so, tf, to, spec["dim"], band=spec.get("band", -1), squared=spec.get("squared", False),
                                nthreads=min(oracle.max_threads(), 16), want_matrix=True)[2]


def _plan(spec, n):
    """The wanted (range, nearer) per planted target: blind and inside in turn, a few resolved; the nearer contender at
    the higher (True) and at the lower index in equal shares."""
    decades = spec.get("decades", (1e-7, 1e-6, 1e-5, 1e-4, 1e-3))
    if spec.get("reach"):
        return [((max(REACH_DECADES[i % 6], _LO), 10 * REACH_DECADES[i % 6]), (i // 6) % 2 == 0) for i in range(n)]
    n_res = spec.get("resolved", 4)
    out = []
    for i in range(n):
        if i >= n - n_res:
            out.append(((RESOLVED, 3 * RESOLVED), i % 2 == 0))
        elif i % 2 == 0:
            out.append(((_LO, _HI), (i // 2) % 2 == 0))
        else:
            d = decades[(i // 2) % len(decades)]
            out.append(((max(d, 1.05 * HALF_ULP), 10 * d), (i // 2 // len(decades)) % 2 == 0))
    return out


# ---- the builder ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def build(name):
    import oracle as _o
    oracle = _o.load()
    spec = SPECS[name]
    dim, band, squared = spec["dim"], spec.get("band", -1), spec.get("squared", False)
    src, tgt, pi = _base(spec)
    if spec.get("tied"):
        return _build_tied(name, spec, oracle, src, tgt)
    n0, m = spec["n0"], spec["m"]
    blocks = 4 if spec.get("quads") else 3
    bmax = spec.get("bmax", 22 if spec.get("dtype") != "f64" else 28)
    dtw = lambda a, b: oracle.dtw(a, b, dim, band=band, squared=squared)
    base = _matrix(oracle, src, tgt, spec)
    ceil0 = 0.5 * bound_matrix(src, tgt, dim, squared) / np.where(base > 0, base, 1.0)
    twins = [[None] * n0 for _ in range(blocks - 1)]
    first_rider = m - spec.get("riders", 0)
    plan = _plan(spec, first_rider)
    contenders = [None] * m
    for t in range(first_rider):
        p = int(pi[t])
        a, y = src[p], tgt[t]
        cols = np.arange(a.size).reshape(a.shape)
        pos = (cols[:, FILTER_DIM:] if spec.get("reach") else cols).reshape(-1)
        c0 = dtw(a, y)
        (lo, hi), higher = plan[t]
        if lo >= HALF_ULP and hi <= RESOLVED and not spec.get("reach"):      # an inside range ends below the pair's bound
            hi = min(hi, ceil0[p, t])
            assert hi > 2 * lo, "target %d: the bound %g leaves no room above %g" % (t, ceil0[p, t], lo)
        fam_cost = [c0]
        for j in range(blocks - 1):
            if spec.get("quads"):                           # all gaps of the family in the one range
                acc = lambda tw, c1: all(lo <= abs(c1 - x) / max(c1, x) < hi for x in fam_cost)
                rng = (lo, hi)
            elif j == 0:                                    # the near twin
                acc = lambda tw, c1: True
                rng = (lo, hi)
            else:                                           # the far twin: behind both
                acc = lambda tw, c1: c1 > max(fam_cost)
                far = spec.get("far", (1e-4, 1e-3) if spec.get("reach") else (3 * RESOLVED, 10 * RESOLVED))
                rng = (max(far[0], 3 * fam_gap), max(far[1], 30 * fam_gap))
            tw, c1 = _calibrate(lambda x: dtw(x, y), a, c0, pos, rng[0], rng[1], acc, spec["seed"] * 64 + t * 4 + j, bmax,
                                trials=3000 if spec.get("quads") else 400)
            if j == 0:
                fam_gap = abs(c1 - c0) / max(c1, c0)
                if not spec.get("quads") and (c1 < c0) != higher:      # the nearer one at the planned index: swap the roles
                    src[p], tw = tw, src[p]
            fam_cost.append(c1)
            twins[j][p] = tw
        contenders[t] = tuple([p] + [p + n0 * (j + 1) for j in range(blocks - 1 if spec.get("quads") else 1)])
    # sources no target is planted on (a rider took their target's place): they get twins too, of any strength
    st = synth.Stream(spec["seed"] ^ 0x71DE)
    for j in range(blocks - 1):
        for p in range(n0):
            if twins[j][p] is None:
                twins[j][p] = _perturb(src[p], np.arange(src[p].size), 3 + 4 * j, src[p].size, st)
    allsrc = src + [x for blk in twins for x in blk]
    if spec.get("quads"):
        # ranks 5 and 6 of a column: two runners-up per source (noisy copies, far from the four and from each other), so
        # that no other family's twins -- closer than 1e-9 in a column they were not made for -- stand there
        for lvl in (0.10, 0.16):
            allsrc = allsrc + [(a + lvl * synth.sigma(dim) * st.normal(a.size).reshape(a.shape)).astype(a.dtype) for a in src]
    # riders: unrelated targets, re-drawn until the twins of their nearest source give them a rung
    tgt = list(tgt[:first_rider]) + [None] * (m - first_rider)
    contenders = contenders[:first_rider] + [None] * (m - first_rider)
    sig = synth.sigma(dim)
    for t in range(first_rider, m):
        want = "inside" if (t - first_rider) % 2 == 0 else "blind"
        for trial in range(200):
            f = allsrc[int(st.integers(1, n0)[0])].shape[0]
            y = (st.normal(f * dim).reshape(f, dim) * sig).astype(src[0].dtype)
            if spec.get("dtype") == "f64":
                y = y * (1.0 + 1e-9 * st.normal(y.size).reshape(y.shape))
            col = _matrix(oracle, allsrc, [y], spec)
            g, pr = measure_gaps(col)
            if pr[0] is None or (pr[0][0] % n0) != (pr[0][1] % n0) or g[0] <= _LO:
                continue
            cl = 0.5 * bound_matrix(allsrc, [y], dim, squared)[pr[0][0], 0] / col[pr[0][0], 0]
            if classify(g[0], cl) == want or (trial >= 100 and classify(g[0], cl) in ("blind", "inside")):
                break
        else:
            raise RuntimeError("no rider for target %d: change the seed" % t)
        tgt[t] = y
        contenders[t] = tuple(sorted(pr[0]))
    return _finish(name, spec, oracle, allsrc, tgt, None, contenders, n0, blocks)


def _build_tied(name, spec, oracle, src, tgt0):
    """Keys tied across a distance: no twin, the planted set as it is."""
    n0, m, dim = spec["n0"], spec["m"], spec["dim"]
    tgt = list(tgt0)[:m]
    mat = _matrix(oracle, src, tgt, spec)
    bnd = bound_matrix(src, tgt, dim, spec.get("squared", False))
    decades = spec["decades"]          # (no wider: the planted pair's runner-up has a third cost close behind it)
    st = synth.Stream(spec["seed"] ^ 0x71ED)
    dist = np.zeros(m)
    contenders = [None] * m
    for t in range(m):
        col = mat[:, t]
        order = np.argsort(col, kind="stable")
        r = 0 if t % 4 == 0 else int(1 + st.integers(1, n0 - 2)[0])      # the two nearest sources, or deeper in the column
        u1, u2 = float(st.uniform24(1)[0]), float(st.uniform24(1)[0])
        if t % 2 == 1 and decades[(t // 2) % len(decades)] >= 1e-4:
            r = 0                                                        # a wide gap needs costs far apart: the planted pair
        higher = (t // 2) % 2 == 0                                       # the nearer contender at the higher index?
        for _ in range(n0):
            a, b = int(order[r]), int(order[r + 1])
            ca, cb = col[a], col[b]
            if t % 2 == 0:
                g = _LO * (_HI / _LO) ** u1
            else:
                d = max(decades[(t // 2) % len(decades)], 1.05 * HALF_ULP)
                top = min(10 * decades[(t // 2) % len(decades)], 0.5 * min(bnd[a, t], bnd[b, t]) / cb)
                g = d * max(top / d, 1.0) ** u2
            near_b = (b > a) == higher
            dist[t] = 0.5 * (ca + cb) + (0.5 if near_b else -0.5) * g * cb
            key = np.abs(col - dist[t])
            ko = np.argsort(key, kind="stable")
            if g * cb < 0.25 * (cb - ca) and {int(ko[0]), int(ko[1])} == {a, b} and key[ko[2]] - key[ko[1]] > 1e-3 * cb:   # those two, no third key near
                break
            r = (r + 1) % (n0 - 1)
        else:
            raise RuntimeError("no pair of adjacent costs for target %d: change the seed" % t)
        contenders[t] = (min(a, b), max(a, b))
    return _finish(name, spec, oracle, src, tgt, dist, contenders, n0, 1)


def _finish(name, spec, oracle, src, tgt, dist, contenders, n0, blocks):
    dim, squared = spec["dim"], spec.get("squared", False)
    mat = _matrix(oracle, src, tgt, spec)
    bnd = bound_matrix(src, tgt, dim, squared)
    gap, pair = measure_gaps(mat, dist)
    m = len(tgt)
    ceiling = np.array([min(bnd[s, t] for s in pair[t]) / max(abs(mat[s, t]) for s in pair[t]) for t in range(m)])
    reach = bool(spec.get("reach"))
    rung = ["reach" if reach else classify(gap[t], ceiling[t]) for t in range(m)]
    decades = REACH_DECADES if reach else tuple(spec.get("decades", (1e-7, 1e-6, 1e-5, 1e-4, 1e-3)))
    return Case(name=name, dim=dim, dtype=spec.get("dtype", "f32"), band=spec.get("band", -1), squared=squared,
                k=5 if spec.get("quads") else 1, n0=n0, blocks=blocks, src=src, tgt=tgt, distance=dist,
                contenders=contenders, rung=rung, gap=gap, ceiling=ceiling, mat=mat, bound=bnd, decades=decades,
                half=bool(spec.get("half")), reach=reach, tied=bool(spec.get("tied")), quads=bool(spec.get("quads")))
