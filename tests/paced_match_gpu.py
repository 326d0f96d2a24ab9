"""What tests/test_gpu_paced_match.py and tests/test_gpu_paced_match_shapes.py share -- TEST INFRASTRUCTURE: sets on an
engine, the two calls through ctypes into sentinel-filled outputs, and the comparisons against tests/paced_match_ref.py."""
import numpy as np

import paced_match_ref as ref
from dtw_path_ref import same_floats
from soundsym_amd import Engine
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

SENT32, SENTF = 0xDEADBEEF, -12345.5
PACED, SYMMETRIC = nat.STEP_PACED, nat.STEP_SYMMETRIC
INF, NAN = float("inf"), float("nan")


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def same_bits(got, want):
    """Equal bit for bit, a NaN matching any NaN (dtw_path_ref.same_floats), and every other entry its exact bits."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not same_floats(got, want):
        return False
    ok = ~np.isnan(want)
    return bool((bits(got)[ok] == bits(want)[ok]).all())


def real(rng, frames, dim, scale=1.0):
    """Values both dtypes hold exactly."""
    return (rng.standard_normal((frames, dim)) * scale).astype(np.float32).astype(np.float64)


class Sets:
    """An engine with a resident dictionary and query set made from lists of [frames, dim] arrays."""

    def __init__(self, src, tgt, dim, dtype="f64", squared=False, band=-1, metric="dtw"):
        self.src, self.tgt, self.dim, self.squared = src, tgt, dim, squared
        npd = np.float32 if dtype == "f32" else np.float64
        self.e = Engine(metric=metric, dtype=dtype, band=band, squared=squared)
        self.d = self.e.dictionary(*pack_segments(src, dim, npd), dim)
        self.q = self.e.queries(*pack_segments(tgt, dim, npd), dim)

    def close(self):
        self.e.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def matrix(sets, step=PACED):
    """ssym_pair_matrix_step into a sentinel-filled matrix with one entry more than it needs: (rc, matrix, untouched)."""
    n, m = len(sets.src), len(sets.tgt)
    out = np.full(n * m + 1, SENTF)
    rc = nat.lib().ssym_pair_matrix_step(sets.e.ctx, sets.d.ptr, sets.q.ptr, step, out.ctypes.data)
    return rc, out[:n * m].reshape(n, m), bool(out[n * m] == SENTF and (rc == nat.SSYM_OK or (out == SENTF).all()))


def match(sets, distance=None, base=0, step=PACED, device=False, flags=0, want_cost=True):
    """ssym_match_queries_step into sentinel-filled outputs with one entry more than the targets: (rc, idx, cost, untouched)."""
    m = len(sets.tgt)
    idx = np.full(m + 1, SENT32, dtype=np.uint32)
    cost = np.full(m + 1, SENTF)
    dist = None if distance is None else np.ascontiguousarray(distance, dtype=np.float64)
    head = [sets.e.ctx, sets.d.ptr, sets.q.ptr, None if dist is None else dist.ctypes.data, base, step]
    if device:
        import torch
        didx = torch.from_numpy(idx.view(np.int32)).cuda()
        dcost = torch.from_numpy(cost).cuda()
        torch.cuda.synchronize()
        rc = nat.lib().ssym_match_queries_step(*head, didx.data_ptr(), dcost.data_ptr() if want_cost else None,
                                               flags | nat.OUT_DEVICE)
        torch.cuda.synchronize()
        idx, cost = didx.cpu().numpy().view(np.uint32), dcost.cpu().numpy()
    else:
        rc = nat.lib().ssym_match_queries_step(*head, idx.ctypes.data, cost.ctypes.data if want_cost else None, flags)
    untouched = idx[m] == SENT32 and cost[m] == SENTF
    if rc != nat.SSYM_OK:
        untouched = untouched and (idx == SENT32).all() and (cost == SENTF).all()
    return rc, idx[:m], cost[:m], bool(untouched)


def error(sets):
    return (nat.lib().ssym_last_error(sets.e.ctx) or b"").decode()


def check_matrix(sets, want):
    rc, mat, untouched = matrix(sets)
    assert rc == nat.SSYM_OK, error(sets)
    assert untouched
    want = np.asarray(want, dtype=np.float64)
    assert mat.shape == want.shape
    # same_bits entry by entry, on the whole matrix at once (a matrix may have half a million entries)
    differ = ~((bits(mat) == bits(want)) | (np.isnan(mat) & np.isnan(want)))
    bad = [(int(s), int(t), mat[s, t], want[s, t]) for s, t in np.argwhere(differ)[:5]]
    assert not bad, bad
    return mat


def _first(a, b):
    """The first entries at which two arrays differ, for a message that stays readable with 65 600 targets."""
    at = np.flatnonzero(~((a == b) | ((a != a) & (b != b))))[:5]
    return at.tolist(), a[at].tolist(), b[at].tolist()


def check_match(sets, want, distance=None, base=0, folded=None, **kw):
    """The call against the restatement's fold of `want` (the restatement's matrix).  folded: that fold, (idx, cost) of
    ref.fold(want, distance, base), where the caller has it already (a fold is a plain loop over every pair)."""
    rc, idx, cost, untouched = match(sets, distance, base, **kw)
    assert rc == nat.SSYM_OK, error(sets)
    assert untouched
    widx, wcost = ref.fold(want, distance, base) if folded is None else folded
    assert np.array_equal(idx, widx), _first(idx, widx)
    if kw.get("want_cost", True):
        assert same_bits(cost, wcost), _first(cost, wcost)
    else:
        assert (cost == SENTF).all()
    return idx, cost


def full_pair_list(n, m):
    src = np.repeat(np.arange(n, dtype=np.uint32), m)
    tgt = np.tile(np.arange(m, dtype=np.uint32), n)
    return src, tgt


def align_costs(sets, n=None, m=None):
    """ssym_dtw_align_step(SSYM_STEP_PACED)'s (out_cost, out_len) over the full pair list, as [n][m] arrays."""
    n, m = len(sets.src) if n is None else n, len(sets.tgt) if m is None else m
    src, tgt = full_pair_list(n, m)
    cost, length, _, _ = sets.e.dtw_align(sets.d, sets.q, src, tgt, step="paced")
    return np.asarray(cost).reshape(n, m), np.asarray(length).reshape(n, m)


def same_as_align(mat, acost):
    """Contract point 1: the bits of ssym_dtw_align_step's out_cost; where one is not finite, neither is the other."""
    fin = np.isfinite(acost)
    assert np.array_equal(np.isfinite(mat), fin)
    assert (bits(mat)[fin] == bits(acost)[fin]).all()
