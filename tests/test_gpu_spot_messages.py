"""The refusals of the spot family word for word: ssym_dtw_spot, ssym_spot_queries, ssym_dtw_spot_all, their three _step
forms and ssym_spotter_create.  Every refusal's code and exact ssym_last_error text, the entry point's own name in it
(the _step forms name themselves), and for each adjacent pair of the order in which a call with two faults reports them

    step, metric, band, handles, (an empty list succeeds), src_idx, empty dictionary / dim, list entries, max_spots,
    NULL outputs, NaN threshold, target limit, source limit

one call with both faults that reports the earlier one.  Outputs are sentinel-filled and stay untouched on every
refusal.  Every call here is refused on the host before any launch; the sets are the smallest on which every check can
be reached (2 sources of 4 and 3 frames, 2 targets of 2 and 3 frames, dim 2), plus one target over each limit (2049
frames for the paced pattern; 4097 frames at dim 1) and, at dim 1, one source over ssym_dtw_spot_all's 2^24 frames."""
import ctypes

import numpy as np
import pytest

from soundsym_amd import Engine
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

SENT32, SENTF = 0xDEADBEEF, -12345.5
NO = nat.NO_MATCH
PACED, SYMMETRIC = nat.STEP_PACED, nat.STEP_SYMMETRIC
INV, UNS, EMPTY = nat.SSYM_E_INVALID, nat.SSYM_E_UNSUPPORTED, nat.SSYM_E_EMPTY_DICT

LIST_CALLS = ("ssym_dtw_spot", "ssym_dtw_spot_step", "ssym_dtw_spot_all", "ssym_dtw_spot_all_step")
QUERY_CALLS = ("ssym_spot_queries", "ssym_spot_queries_step")

STEP = "{fn}: step must be SSYM_STEP_SYMMETRIC or SSYM_STEP_PACED"
METRIC = "{fn}: the context's metric is refcos, which has no alignment to spot"
BAND = "{fn}: a Sakoe-Chiba band has no meaning with a free start; use a context without one"
HANDLES = "{fn}: dictionary or queries handle is NULL"
SRC_NULL = "{fn}: src_idx is NULL"
NO_DICT = "empty dictionary"
DIM = "dim mismatch between dictionary and targets"
TGT_NULL = "{fn}: tgt_idx is NULL and n_pairs exceeds the number of targets"
SRC_OUT = "{fn}: src_idx[1] is outside the dictionary"
TGT_OUT = "{fn}: tgt_idx[0] is outside the targets"
MAX_SPOTS = "{fn}: max_spots must be 1 ... 64"
OUTPUTS = {"ssym_dtw_spot": "{fn}: out_cost, out_start and out_end must not be NULL",
           "ssym_dtw_spot_all": "{fn}: out_count, out_cost, out_start and out_end must not be NULL",
           "ssym_spot_queries": "{fn}: out_idx, out_cost, out_start and out_end must not be NULL"}
NAN = "{fn}: max_cost[1] is NaN"
TARGET = "{fn}: a target has more than {frames} frames, or frames have more than 64 values"
SOURCE = "{fn}: a listed source has more than 16777216 frames (the end-column profile takes 12 bytes of scratch per source frame)"


def _base(name):
    return name[:-len("_step")] if name.endswith("_step") else name


class _Sets:
    """An engine with a resident dictionary and query set made from lists of frame counts (all-zero frames)."""

    def __init__(self, src, tgt, dim=2, tgt_dim=None, **kw):
        self.e = Engine(dtype="f64", **kw)
        sf, so = pack_segments([np.zeros((f, dim)) for f in src], dim, np.float64)
        self.d = self.e.dictionary(sf, so, dim)
        tgt_dim = tgt_dim or dim
        tf, to = pack_segments([np.zeros((f, tgt_dim)) for f in tgt], tgt_dim, np.float64)
        self.q = self.e.queries(tf, to, tgt_dim)
        self.n_tgt = len(tgt)

    def close(self):
        self.e.close()


def _refused(s, name, code, text, step=PACED, d=True, q=True, src=(0, 1), tgt=None, n=None, k=2, max_cost=None, null=(),
             ok=False):
    """One call of entry point `name` on the sets s into sentinel-filled outputs; it returns `code` with the message `text`
    (a pattern that takes the entry point's name as {fn}) and leaves every output alone.  d / q False, src None and the names in
    `null` pass NULL.  ok: the call succeeds instead, the outputs of an empty call untouched as well."""
    L = nat.lib()
    ctx = s.e.ctx
    # whatever the context's last message was, it is another one now
    assert L.ssym_spotter_flush(ctx, None, 0, None) == INV
    assert L.ssym_last_error(ctx) == b"ssym_spotter_flush: the spotter handle is NULL"
    stepped = name.endswith("_step")
    step_arg = [step] if stepped else []
    dp, qp = (s.d.ptr if d else None), (s.q.ptr if q else None)
    if _base(name) == "ssym_spot_queries":
        m = s.n_tgt
        outs = {"idx": np.full(m, SENT32, dtype=np.uint32), "cost": np.full(m, SENTF),
                "start": np.full(m, SENT32, dtype=np.uint32), "end": np.full(m, SENT32, dtype=np.uint32)}
        ptr = lambda key: None if key in null else outs[key].ctypes.data
        rc = getattr(L, name)(ctx, dp, qp, 0, *step_arg, ptr("idx"), ptr("cost"), ptr("start"), ptr("end"), 0)
    else:
        si = None if src is None else np.ascontiguousarray(src, dtype=np.uint32)
        ti = None if tgt is None else np.ascontiguousarray(tgt, dtype=np.uint32)
        n = n if n is not None else (si.size if si is not None else 2)
        head = [ctx, dp, qp, None if si is None else si.ctypes.data, None if ti is None else ti.ctypes.data, n, 0] + step_arg
        rows = max(n, 1)
        if _base(name) == "ssym_dtw_spot":
            outs = {"cost": np.full(rows, SENTF), "start": np.full(rows, SENT32, dtype=np.uint32),
                    "end": np.full(rows, SENT32, dtype=np.uint32)}
            ptr = lambda key: None if key in null else outs[key].ctypes.data
            rc = getattr(L, name)(*head, ptr("cost"), ptr("start"), ptr("end"), 0)
        else:
            cols = max(k, 1)
            outs = {"count": np.full(rows, SENT32, dtype=np.uint32), "cost": np.full((rows, cols), SENTF),
                    "start": np.full((rows, cols), SENT32, dtype=np.uint32), "end": np.full((rows, cols), SENT32, dtype=np.uint32)}
            ptr = lambda key: None if key in null else outs[key].ctypes.data
            mc = None if max_cost is None else np.ascontiguousarray(max_cost, dtype=np.float64)
            rc = getattr(L, name)(*head, k, None if mc is None else mc.ctypes.data, ptr("count"), ptr("cost"), ptr("start"),
                                  ptr("end"), 0)
    for x in outs.values():
        assert ((x == SENTF) if x.dtype == np.float64 else (x == SENT32)).all(), name
    if ok:
        assert rc == nat.SSYM_OK, (name, rc, L.ssym_last_error(ctx))
        return
    want = text.format(fn=name, frames=2048 if stepped and step == PACED else 4096)
    assert (rc, L.ssym_last_error(ctx).decode()) == (code, want), name


def _outputs(name):
    return OUTPUTS[_base(name)]


@pytest.fixture(scope="module")
def sets():
    made = {"plain": _Sets([4, 3], [2, 3]),
            "refcos": _Sets([4, 3], [2, 3], metric="refcos"),
            "refcos_band": _Sets([4, 3], [2, 3], metric="refcos", band=0),
            "band": _Sets([4, 3], [2, 3], band=0),
            "no_dict": _Sets([], [2, 3]),
            "dim": _Sets([4, 3], [2, 3], tgt_dim=3),
            "no_targets": _Sets([4, 3], []),
            "nothing": _Sets([], []),
            "paced_limit": _Sets([4, 3], [2, 3, 2049]),
            # dim 1: the symmetric pattern's target limit, and one source over ssym_dtw_spot_all's (128 MiB, made once)
            "limit": _Sets([4, 3, 2 ** 24 + 1], [2, 3, 4097], dim=1)}
    yield made
    for s in made.values():
        s.close()


@pytest.mark.parametrize("name", LIST_CALLS)
def test_every_refusal_of_the_pair_list_calls_word_for_word(sets, name):
    plain, stepped, spot_all = sets["plain"], name.endswith("_step"), "spot_all" in name
    if stepped:
        _refused(plain, name, INV, STEP, step=7)
        _refused(plain, name, INV, STEP, step=2)
    _refused(sets["refcos"], name, UNS, METRIC)
    _refused(sets["band"], name, UNS, BAND)
    _refused(plain, name, INV, HANDLES, d=False)
    _refused(plain, name, INV, HANDLES, q=False)
    _refused(plain, name, 0, "", n=0, ok=True)
    _refused(plain, name, INV, SRC_NULL, src=None)
    _refused(sets["no_dict"], name, EMPTY, NO_DICT)
    _refused(sets["dim"], name, INV, DIM)
    _refused(plain, name, INV, TGT_NULL, src=(0, 1, 0))
    _refused(plain, name, INV, SRC_OUT, src=(0, 2))
    _refused(plain, name, INV, SRC_OUT, src=(1, 0xfffffffe))
    _refused(plain, name, INV, TGT_OUT, tgt=(2, 0))
    if spot_all:
        _refused(plain, name, INV, MAX_SPOTS, k=0)
        _refused(plain, name, INV, MAX_SPOTS, k=65)
        _refused(plain, name, INV, NAN, max_cost=(1.0, float("nan")))
    for out in ("cost", "start", "end") + (("count",) if spot_all else ()):
        _refused(plain, name, INV, _outputs(name), null=(out,))
    if stepped:
        _refused(sets["paced_limit"], name, UNS, TARGET, src=(0, 1), tgt=(0, 2))
        _refused(sets["paced_limit"], name, 0, "", src=(0, 1), tgt=(0, 2), n=0, ok=True)
    _refused(sets["limit"], name, UNS, TARGET, step=SYMMETRIC, src=(0, 1), tgt=(0, 2))
    if spot_all:
        _refused(sets["limit"], name, UNS, SOURCE, step=SYMMETRIC, src=(0, 2), tgt=(0, 1))


@pytest.mark.parametrize("name", LIST_CALLS)
def test_of_two_faults_the_pair_list_calls_report_the_earlier(sets, name):
    plain, stepped, spot_all = sets["plain"], name.endswith("_step"), "spot_all" in name
    if stepped:
        _refused(sets["refcos"], name, INV, STEP, step=7)                                  # step, metric
    _refused(sets["refcos_band"], name, UNS, METRIC)                                       # metric, band
    _refused(sets["band"], name, UNS, BAND, d=False)                                       # band, handles
    _refused(plain, name, INV, HANDLES, q=False, n=0)                                      # handles, the empty list
    _refused(plain, name, 0, "", src=None, n=0, null=("cost", "start", "end", "count"), ok=True)     # the empty list, src_idx
    _refused(sets["no_dict"], name, 0, "", n=0, ok=True)
    _refused(sets["no_dict"], name, INV, SRC_NULL, src=None)                               # src_idx, empty dictionary
    _refused(sets["dim"], name, INV, SRC_NULL, src=None)
    _refused(sets["no_dict"], name, EMPTY, NO_DICT, src=(0, 2), tgt=(2, 0))               # empty dictionary / dim, list entries
    _refused(sets["dim"], name, INV, DIM, src=(0, 2), tgt=(2, 0))
    if spot_all:
        _refused(plain, name, INV, SRC_OUT, src=(0, 2), k=0)                               # list entries, max_spots
        _refused(plain, name, INV, MAX_SPOTS, k=65, null=("count",))                       # max_spots, NULL outputs
        _refused(plain, name, INV, _outputs(name), null=("end",), max_cost=(1.0, float("nan")))      # NULL outputs, NaN
        _refused(sets["limit"], name, INV, NAN, step=SYMMETRIC, tgt=(0, 2), max_cost=(1.0, float("nan")))       # NaN, target limit
        _refused(sets["limit"], name, UNS, TARGET, step=SYMMETRIC, src=(0, 2), tgt=(0, 2))           # target limit, source limit
        if stepped:
            _refused(sets["paced_limit"], name, INV, NAN, tgt=(0, 2), max_cost=(1.0, float("nan")))
    else:
        _refused(plain, name, INV, TGT_OUT, tgt=(2, 0), null=("cost",))                    # list entries, NULL outputs
        _refused(sets["limit"], name, INV, _outputs(name), step=SYMMETRIC, tgt=(0, 2), null=("start",))         # NULL outputs, target limit
        if stepped:
            _refused(sets["paced_limit"], name, INV, _outputs(name), tgt=(0, 2), null=("start",))


@pytest.mark.parametrize("name", QUERY_CALLS)
def test_every_refusal_of_spot_queries_word_for_word_and_the_earlier_of_two(sets, name):
    plain, stepped = sets["plain"], name.endswith("_step")
    if stepped:
        _refused(plain, name, INV, STEP, step=7)
        _refused(sets["refcos"], name, INV, STEP, step=7)                                  # step, metric
    _refused(sets["refcos"], name, UNS, METRIC)
    _refused(sets["refcos_band"], name, UNS, METRIC)                                       # metric, band
    _refused(sets["band"], name, UNS, BAND)
    _refused(sets["band"], name, UNS, BAND, q=False)                                       # band, handles
    _refused(plain, name, INV, HANDLES, d=False)
    _refused(plain, name, INV, HANDLES, q=False)
    _refused(sets["no_targets"], name, INV, HANDLES, d=False)                              # handles, no targets
    _refused(sets["no_targets"], name, 0, "", ok=True)
    _refused(sets["nothing"], name, 0, "", null=("idx", "cost", "start", "end"), ok=True)  # no targets, empty dictionary
    _refused(sets["no_dict"], name, EMPTY, NO_DICT)
    _refused(sets["dim"], name, INV, DIM)
    _refused(sets["no_dict"], name, EMPTY, NO_DICT, null=("idx",))                         # empty dictionary / dim, NULL outputs
    _refused(sets["dim"], name, INV, DIM, null=("idx",))
    for out in ("idx", "cost", "start", "end"):
        _refused(plain, name, INV, _outputs(name), null=(out,))
    if stepped:
        _refused(sets["paced_limit"], name, UNS, TARGET)
        _refused(sets["paced_limit"], name, INV, _outputs(name), null=("cost",))           # NULL outputs, target limit
    _refused(sets["limit"], name, UNS, TARGET, step=SYMMETRIC)
    _refused(sets["limit"], name, INV, _outputs(name), step=SYMMETRIC, null=("cost",))


def test_every_refusal_of_spotter_create_word_for_word_and_the_earlier_of_two(sets):
    L, fn = nat.lib(), "ssym_spotter_create"
    nan = np.array([1.0, float("nan"), float("nan")])

    def refused(s, code, text, q=True, lanes=1, max_cost=None, out=True):
        ctx = s.e.ctx
        assert L.ssym_spotter_flush(ctx, None, 0, None) == INV
        handle = ctypes.c_void_p(5)
        rc = L.ssym_spotter_create(ctx, s.q.ptr if q else None, lanes, None if max_cost is None else max_cost.ctypes.data,
                                   ctypes.byref(handle) if out else None)
        assert (rc, L.ssym_last_error(ctx).decode()) == (code, text.format(fn=fn))
        assert handle.value == (None if out else 5)               # a refusal leaves NULL where there is somewhere to leave it

    plain, limit = sets["plain"], sets["limit"]
    refused(plain, INV, "{fn}: out is NULL", out=False)
    refused(sets["refcos"], INV, "{fn}: out is NULL", out=False)                             # out, metric
    refused(sets["refcos"], UNS, METRIC)
    refused(sets["refcos_band"], UNS, METRIC)                                              # metric, band
    refused(sets["band"], UNS, BAND)
    refused(sets["band"], UNS, BAND, q=False)                                              # band, handle
    refused(plain, INV, "{fn}: the queries handle is NULL or n_lanes is 0", q=False)
    refused(plain, INV, "{fn}: the queries handle is NULL or n_lanes is 0", lanes=0)
    refused(plain, INV, "{fn}: the queries handle is NULL or n_lanes is 0", lanes=0, max_cost=nan)       # lanes, NaN threshold
    refused(plain, INV, "{fn}: max_cost[1] is NaN", max_cost=nan)
    refused(limit, INV, "{fn}: max_cost[1] is NaN", max_cost=nan)                            # NaN threshold, target limit
    refused(limit, UNS, "{fn}: a target has more than 4096 frames, or frames have more than 64 values")
    refused(limit, UNS, "{fn}: a target has more than 4096 frames, or frames have more than 64 values", lanes=2 ** 31)       # limit, pairs
    refused(plain, UNS, "{fn}: more than 2^32 - 2 (lane, target) pairs", lanes=2 ** 31)
