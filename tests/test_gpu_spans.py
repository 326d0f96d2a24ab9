"""ssym_dtw_align_spans on the GPU against the cut route -- the existing call on a dictionary built from the sliced frames,
in the same context -- bit for bit: cost, length, path and map, both step patterns, every edge of the kernels (64-row
chunks, the LDS / slab boundary of the direction matrix, both ends of the paced shape rule), spans inside a recording the
existing call refuses, frames outside the spans poisoned, spots fed straight in, and the limits and errors of the header."""
import numpy as np
import pytest

import span_ref
from soundsym_amd import Engine
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

NO = nat.NO_MATCH
SENT32, SENTF = 0xDEADBEEF, -12345.5
REC_FRAMES = (300, 70, 1, 4200)
TGT_FRAMES = (1, 2, 33, 64, 65, 130, 256, 0, 8)          # (0: a target without frames, 8: the limit case's)
T = {f: i for i, f in enumerate(TGT_FRAMES)}

# (recording, first, last, target frames)
SYMMETRIC = [(0, 0, 0, 1), (0, 299, 299, 2), (0, 0, 299, 130), (0, 17, 80, 64), (0, 17, 81, 65), (0, 100, 228, 130),
             (0, 0, 256, 256),                             # 257 x 256: the direction matrix goes to the global slabs
             (0, 17, 80, 1), (0, 17, 81, 2), (0, 100, 228, 33), (1, 0, 69, 33), (1, 3, 66, 64),
             (2, 0, 0, 33), (2, 0, 0, 1), (3, 4135, 4199, 65), (3, 4135, 4199, 130), (0, 5, 9, 0)]
# the paced shape rule admits Fa' in floor((Fb - 1) / 2) + 1 ... 2 Fb - 1: 33 -> 17 ... 65, 65 -> 33 ... 129
PACED = [(0, 0, 0, 1), (0, 299, 299, 2), (0, 298, 299, 1),                      # Fb = 1: one frame only; Fb = 2: 1 ... 3
         (0, 17, 32, 33), (0, 17, 33, 33), (0, 17, 81, 33), (0, 17, 82, 33),    # 16 (too short), 17, 65, 66 (too long)
         (0, 100, 228, 65), (0, 100, 229, 65), (0, 17, 80, 64), (0, 17, 81, 65), (0, 0, 256, 130),
         (0, 0, 256, 256),                                 # the slab
         (0, 0, 299, 256), (1, 0, 69, 64), (2, 0, 0, 1), (2, 0, 0, 2), (3, 4135, 4199, 65), (3, 4135, 4199, 33), (0, 5, 9, 0)]


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _data(dim, seed=0x59A7):
    rng = np.random.default_rng(seed)
    sigma = 4.0 / (1.0 + np.arange(dim))
    recs = [rng.normal(size=(f, dim)) * sigma for f in REC_FRAMES]
    tgts = [rng.normal(size=(f, dim)) * sigma for f in TGT_FRAMES]
    return recs, tgts


def _call(e, d, q, src, tgt, first, last, step="symmetric", base=0, device=False, offsets=None):
    """ssym_dtw_align_spans through ctypes into sentinel-filled outputs: (rc, cost, len, path [cells, 2], map, p_off, m_off)."""
    src, tgt, first, last = (np.ascontiguousarray(x, dtype=np.uint32) for x in (src, tgt, first, last))
    n = src.size
    L = nat.lib()
    if offsets is None:
        p_off, m_off = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
        rc = L.ssym_dtw_align_spans_sizes(d.ptr, q.ptr, src.ctypes.data, tgt.ctypes.data, first.ctypes.data, last.ctypes.data, n,
                                          base, p_off.ctypes.data, m_off.ctypes.data)
        if rc != nat.SSYM_OK:
            return (rc,) + (None,) * 6
    else:
        p_off, m_off = offsets
    cost = np.full(n, SENTF)
    length = np.full(n, SENT32, dtype=np.uint32)
    path = np.full((int(p_off[-1]), 2), SENT32, dtype=np.uint32)
    fmap = np.full(int(m_off[-1]), SENT32, dtype=np.uint32)
    which = nat.STEP_PACED if step == "paced" else nat.STEP_SYMMETRIC
    head = (e.ctx, d.ptr, q.ptr, src.ctypes.data, tgt.ctypes.data, first.ctypes.data, last.ctypes.data, n, base, which)
    if device:
        import torch
        dcost, dlen = torch.from_numpy(cost).cuda(), torch.from_numpy(length.view(np.int32)).cuda()
        dpath, dmap = torch.from_numpy(path.view(np.int32).reshape(-1)).cuda(), torch.from_numpy(fmap.view(np.int32)).cuda()
        torch.cuda.synchronize()
        rc = L.ssym_dtw_align_spans(*head, dcost.data_ptr(), dlen.data_ptr(), p_off.ctypes.data, dpath.data_ptr(),
                                    m_off.ctypes.data, dmap.data_ptr(), nat.OUT_DEVICE)
        torch.cuda.synchronize()
        cost, length = dcost.cpu().numpy(), dlen.cpu().numpy().view(np.uint32)
        path, fmap = dpath.cpu().numpy().view(np.uint32).reshape(-1, 2), dmap.cpu().numpy().view(np.uint32)
    else:
        rc = L.ssym_dtw_align_spans(*head, cost.ctypes.data, length.ctypes.data, p_off.ctypes.data, path.ctypes.data,
                                    m_off.ctypes.data, fmap.ctypes.data, 0)
    return rc, cost, length, path, fmap, p_off, m_off


def _cut_route(e, recs, q, cases, dim, step):
    """The existing call on a dictionary built from the sliced frames: (cost, len, paths, maps)."""
    cut = [recs[r][a:b + 1].copy() for r, a, b, _ in cases]
    d = e.dictionary(*pack_segments(cut, dim, np.float64), dim)
    try:
        return e.dtw_align(d, q, np.arange(len(cases)), [T[f] for _, _, _, f in cases], step=step)
    finally:
        d.close()


def _assert_same(got, want, cases, what):
    rc, cost, length, path, fmap, p_off, m_off = got
    w_cost, w_len, w_paths, w_maps = want
    assert rc == nat.SSYM_OK, what
    assert np.array_equal(_bits(cost), _bits(w_cost)), (what, cost, w_cost)
    assert np.array_equal(length, w_len), (what, length, w_len)
    for p, (r, a, b, f) in enumerate(cases):
        n = int(length[p])
        cells = path[int(p_off[p]):int(p_off[p + 1])]
        assert int(p_off[p + 1] - p_off[p]) == (b - a + f if f else 0) and int(m_off[p + 1] - m_off[p]) == f, (what, p)
        assert np.array_equal(cells[:n], w_paths[p]), (what, p)
        assert (cells[n:] == SENT32).all(), (what, p)                          # beyond the path: unwritten
        slot = fmap[int(m_off[p]):int(m_off[p + 1])]
        if n:
            assert np.array_equal(slot, w_maps[p]) and slot[0] == 0 and cells[n - 1][0] == b - a, (what, p)
        else:
            assert (slot == SENT32).all(), (what, p)


class _Ctx:
    """An f64 dtw engine with the recordings as its dictionary and the targets as its queries."""

    def __init__(self, dim=13, **kw):
        self.dim = dim
        self.recs, self.tgts = _data(dim)
        self.e = Engine(metric="dtw", dtype="f64", **kw)
        self.d = self.e.dictionary(*pack_segments(self.recs, dim, np.float64), dim)
        self.q = self.e.queries(*pack_segments(self.tgts, dim, np.float64), dim)

    def spans(self, cases, step="symmetric", d=None, src=None, **kw):
        r, a, b, f = (np.array(x) for x in zip(*cases))
        return _call(self.e, self.d if d is None else d, self.q, r if src is None else src, [T[x] for x in f], a, b, step, **kw)

    def close(self):
        self.e.close()


@pytest.fixture(scope="module")
def ctx():
    c = _Ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def answers(ctx):
    """The cut route's answers, computed once: step -> (cost, len, paths, maps)."""
    return {step: _cut_route(ctx.e, ctx.recs, ctx.q, cases, ctx.dim, step)
            for step, cases in (("symmetric", SYMMETRIC), ("paced", PACED))}


def test_the_cases_sit_where_the_kernels_change_their_path():
    fa = lambda c: c[2] - c[1] + 1
    assert {64, 65, 129, 257, 300, 1} <= {fa(c) for c in SYMMETRIC}
    assert any(fa(c) * ((c[3] + 15) // 16) * 4 > 16384 for c in SYMMETRIC) and any(fa(c) * ((c[3] + 15) // 16) * 4 > 16384 for c in PACED)
    assert {fa(c) for c in PACED if c[3] == 33} >= {16, 17, 65, 66} and {fa(c) for c in PACED if c[3] == 65} >= {129, 130}
    assert {c[3] for c in SYMMETRIC} >= {1, 2, 33, 64, 65, 130, 256}
    assert REC_FRAMES[3] > 4096                                                 # ssym_dtw_align itself refuses that recording


@pytest.mark.parametrize("step,cases", [("symmetric", SYMMETRIC), ("paced", PACED)])
def test_spans_equal_the_cut_route_bit_for_bit(ctx, answers, step, cases):
    got = ctx.spans(cases, step)
    _assert_same(got, answers[step], cases, step)
    finite = np.isfinite(got[1])
    if step == "paced":
        want = [span_ref.align_status([REC_FRAMES[r]], [f], [(a, b)], 13, "paced") == span_ref.OK and f > 0 and
                (f - 1) // 2 + 1 <= b - a + 1 <= 2 * f - 1 for r, a, b, f in cases]
        assert finite.tolist() == want
    else:
        assert finite.tolist() == [f > 0 for _, _, _, f in cases]
    # the recording of 4200 frames: the existing call refuses it, the span call does not mind
    with pytest.raises(nat.SsymError) as err:
        ctx.e.dtw_align(ctx.d, ctx.q, [3], [T[65]], step=step)
    assert err.value.code == nat.SSYM_E_UNSUPPORTED


@pytest.mark.parametrize("step,cases", [("symmetric", SYMMETRIC), ("paced", PACED)])
def test_device_outputs_and_an_index_base(ctx, answers, step, cases):
    got = ctx.spans(cases, step, device=True, src=np.array([c[0] for c in cases]) + 7, base=7)
    _assert_same(got, answers[step], cases, step + ", SSYM_OUT_DEVICE")
    # the Engine's spelling of both
    r, a, b, f = (np.array(x) for x in zip(*cases))
    cost, length, paths, maps = ctx.e.dtw_align(ctx.d, ctx.q, r, [T[x] for x in f], step=step, spans=(a, b))
    assert np.array_equal(_bits(cost), _bits(answers[step][0])) and np.array_equal(length, answers[step][1])
    assert all(np.array_equal(x, y) for x, y in zip(paths, answers[step][2]))
    assert all(np.array_equal(x, y) for x, y in zip(maps, answers[step][3]))
    dcost, dlen, _, dmap, _, m_off = ctx.e.dtw_align_device(ctx.d, ctx.q, r, [T[x] for x in f], step=step, spans=(a, b))
    assert np.array_equal(_bits(dcost.cpu().numpy()), _bits(cost)) and np.array_equal(dlen.cpu().numpy().view(np.uint32), length)
    hmap = dmap.cpu().numpy().view(np.uint32)
    assert all(np.array_equal(hmap[int(m_off[p]):int(m_off[p + 1])], maps[p]) for p in range(len(cases)) if length[p])


@pytest.mark.parametrize("step,cases", [("symmetric", SYMMETRIC), ("paced", PACED)])
def test_frames_outside_the_spans_are_never_read(ctx, answers, step, cases):
    """One copy of its recording per case, every frame outside the case's span NaN: all outputs keep their bits."""
    copies = []
    for r, a, b, _ in cases:
        x = ctx.recs[r].copy()
        x[:a] = np.nan
        x[b + 1:] = np.nan
        copies.append(x)
    d = ctx.e.dictionary(*pack_segments(copies, ctx.dim, np.float64), ctx.dim)
    try:
        got = ctx.spans(cases, step, d=d, src=np.arange(len(cases)))
    finally:
        d.close()
    _assert_same(got, answers[step], cases, step + ", poisoned")


@pytest.mark.parametrize("kw,dim", [({}, 16), ({}, 40), ({}, 64), ({"band": 8}, 13), ({"squared": True}, 13)],
                         ids=["dim16", "dim40", "dim64", "band8", "squared"])
def test_other_frame_widths_a_band_and_the_squared_cost(kw, dim):
    c = _Ctx(dim, **kw)
    try:
        steps = ("symmetric",) if "band" in kw else ("symmetric", "paced")
        cases = [(0, 17, 80, 64), (0, 17, 81, 65), (1, 5, 40, 33), (0, 0, 256, 256)]
        for step in steps:
            want = _cut_route(c.e, c.recs, c.q, cases, dim, step)
            _assert_same(c.spans(cases, step), want, cases, "%s %r dim %d" % (step, kw, dim))
            assert np.isfinite(want[0]).all()
            # ... and the restatement, slice by slice (the costs bit for bit where the sum is the reference's)
            for p, (r, a, b, f) in enumerate(cases[:3]):
                ref = span_ref.align_one(c.recs[r], c.tgts[T[f]], a, b, step, kw.get("band", -1), kw.get("squared", False))
                assert np.array_equal(want[2][p], ref[1]) and np.array_equal(want[3][p], ref[2])
    finally:
        c.close()


@pytest.mark.parametrize("step", ["symmetric", "paced"])
def test_spots_go_straight_into_the_span_alignment(ctx, step):
    src = np.array([0, 1, 3, 0, 0, 2], dtype=np.uint32)
    tgt = np.array([T[33], T[33], T[65], T[2], T[0], T[1]], dtype=np.uint32)       # (T[0]: no frames, a spot without a span)
    s_cost, start, end = ctx.e.dtw_spot(ctx.d, ctx.q, src, tgt, step=step)
    assert end[4] == NO and start[4] == NO and (end[[0, 1, 2, 3, 5]] != NO).all()
    rc, cost, length, path, fmap, p_off, m_off = _call(ctx.e, ctx.d, ctx.q, src, tgt, start, end, step)
    assert rc == nat.SSYM_OK
    assert np.array_equal(_bits(cost), _bits(s_cost))                              # the spot's bits (+inf for the one without)
    for p in range(src.size):
        if end[p] == NO:
            assert length[p] == 0 and cost[p] == np.inf
            continue
        n = int(length[p])
        assert n > 0 and fmap[int(m_off[p])] == 0
        assert tuple(path[int(p_off[p])]) == (0, 0)
        assert path[int(p_off[p]) + n - 1][0] == end[p] - start[p]                 # the last cell's source: last - first


def test_limits(ctx):
    # 4097 frames of the 4200: beyond the limit; 4096 frames with an 8-frame target run, and equal the cut route
    rc = _call(ctx.e, ctx.d, ctx.q, [3], [T[8]], [100], [100 + 4096])[0]
    assert rc == nat.SSYM_E_UNSUPPORTED
    cases = [(3, 100, 100 + 4095, 8)]
    _assert_same(ctx.spans(cases), _cut_route(ctx.e, ctx.recs, ctx.q, cases, ctx.dim, "symmetric"), cases, "4096 frames")
    # the full set of statuses against the table of tests/span_ref.py
    for step in ("symmetric", "paced"):
        for r, a, b, f in ((3, 0, 4096, 8), (3, 0, 4095, 8), (0, 0, 299, 256), (3, 4199, 4199, 1)):
            p_off, m_off = span_ref.sizes([f], [(a, b)])
            got = _call(ctx.e, ctx.d, ctx.q, [r], [T[f]], [a], [b], step, offsets=(p_off, m_off))
            assert got[0] == span_ref.align_status([REC_FRAMES[r]], [f], [(a, b)], 13, step), (step, r, a, b, f)


@pytest.mark.parametrize("first,last", [(81, 80), (0, 300), (299, 300), (NO, 5), (5, NO), (NO - 1, NO - 1)])
def test_invalid_spans_are_refused_with_the_outputs_unwritten(ctx, first, last):
    src, tgt = [0, 0], [T[33], T[33]]
    assert span_ref.align_status([300, 300], [33, 33], [(17, 60), (first, last)], 13) == span_ref.E_INVALID
    assert _call(ctx.e, ctx.d, ctx.q, src, tgt, [17, first], [60, last])[0] == nat.SSYM_E_INVALID      # the sizes call
    offsets = (np.array([0, 100, 200], dtype=np.uint64), np.array([0, 40, 80], dtype=np.uint64))
    for step in ("symmetric", "paced"):
        rc, cost, length, path, fmap, _, _ = _call(ctx.e, ctx.d, ctx.q, src, tgt, [17, first], [60, last], step, offsets=offsets)
        assert rc == nat.SSYM_E_INVALID and b"span 1" in nat.lib().ssym_last_error(ctx.e.ctx)
        assert (cost == SENTF).all() and (length == SENT32).all() and (path == SENT32).all() and (fmap == SENT32).all()


def test_the_existing_error_cases_keep_their_codes(ctx):
    ok = ([0], [T[33]], [17], [60])
    assert _call(ctx.e, ctx.d, ctx.q, *ok, step="symmetric")[0] == nat.SSYM_OK
    L = nat.lib()
    u32 = lambda *v: np.array(v, dtype=np.uint32)
    s, t, a, b = u32(0), u32(T[33]), u32(17), u32(60)
    p_off, m_off = span_ref.sizes([33], [(17, 60)])
    cost, length = np.full(1, SENTF), np.full(1, SENT32, dtype=np.uint32)
    path, fmap = np.full((int(p_off[-1]), 2), SENT32, dtype=np.uint32), np.full(33, SENT32, dtype=np.uint32)
    tail = (cost.ctypes.data, length.ctypes.data, p_off.ctypes.data, path.ctypes.data, m_off.ctypes.data, fmap.ctypes.data, 0)
    call = lambda src, first, last, step=0, d=ctx.d: L.ssym_dtw_align_spans(
        ctx.e.ctx, d.ptr, ctx.q.ptr, src.ctypes.data, t.ctypes.data, first, last, 1, 0, step, *tail)
    assert call(s, None, b.ctypes.data) == nat.SSYM_E_INVALID                     # a NULL span array
    assert call(s, a.ctypes.data, None) == nat.SSYM_E_INVALID
    assert call(u32(9), a.ctypes.data, b.ctypes.data) == nat.SSYM_E_INVALID        # a source outside the dictionary
    assert call(s, a.ctypes.data, b.ctypes.data, step=9) == nat.SSYM_E_INVALID     # an unknown step
    small = np.array([0, 10], dtype=np.uint64)                                     # offsets with too little room
    assert L.ssym_dtw_align_spans(ctx.e.ctx, ctx.d.ptr, ctx.q.ptr, s.ctypes.data, t.ctypes.data, a.ctypes.data, b.ctypes.data,
                                  1, 0, 0, cost.ctypes.data, length.ctypes.data, small.ctypes.data, path.ctypes.data,
                                  m_off.ctypes.data, fmap.ctypes.data, 0) == nat.SSYM_E_INVALID
    assert (cost == SENTF).all() and (length == SENT32).all() and (path == SENT32).all() and (fmap == SENT32).all()
    # src_idx = SSYM_NO_MATCH: no path, whatever its span says
    assert call(u32(NO), u32(7000).ctypes.data, u32(3).ctypes.data) == nat.SSYM_OK and cost[0] == np.inf and length[0] == 0
    # a refcos context and a band under the paced pattern: SSYM_E_UNSUPPORTED
    for kw, step in (({"metric": "refcos"}, 0), ({"metric": "dtw", "band": 8}, 1)):
        e = Engine(dtype="f64", **kw)
        try:
            d = e.dictionary(*pack_segments(ctx.recs[:2], 13, np.float64), 13)
            q = e.queries(*pack_segments(ctx.tgts, 13, np.float64), 13)
            assert _call(e, d, q, *ok, step="paced" if step else "symmetric", offsets=(p_off, m_off))[0] == nat.SSYM_E_UNSUPPORTED
        finally:
            e.close()
