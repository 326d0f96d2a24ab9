"""The partitioner's internal boundaries, read from csrc/partition.hip (CPU only).

tests/test_gpu_partition_shapes.py picks its cases to fall on both sides of every branch of the kernels: the E-step's
model in LDS or in global memory, the E-step grid capped by the slab budget, the lane splits of the column statistics,
frame counts around the tile.  This file reads the constants that place those branches from the source, restates the
host-side decisions in Python and checks that the case lists still straddle each of them, so that a moved constant
moves the case list with it.  It also checks that the restatement itself is a valid reference for unstandardised data.
"""
import os
import re

import numpy as np
import pytest

import partition_ref as ref
from soundsym_amd.api import init_rows
from test_gpu_partition import _close, _mixture
from test_gpu_partition_shapes import GMM_CASES, STD_DIMS, STD_NS, VOTE_CASES

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(os.path.dirname(HERE), "soundsym_amd", "csrc", "partition.hip")
NUM_CUS = 256                       # MI355X
BLOCK = 256                         # threads of colstats_kernel and gmm_estep_kernel


def _constants():
    text = open(SRC).read()
    out = {}
    for name in ("kTile", "kMaxDim", "kMaxK", "kModelLdsBytes", "kPartialBudget"):
        m = re.search(r"\b%s\s*=\s*([^,;]+)[,;]" % name, text)
        assert m, name
        expr = re.sub(r"size_t\((\w+)\)", r"(\1)", m.group(1))
        assert re.fullmatch(r"[0-9\s()*<+]+", expr), expr
        out[name] = int(eval(expr, {"__builtins__": {}}))
    return out


C = _constants()


def model_fits_lds(K, d):
    P = d * (d + 1) // 2
    return (K * d + K * P + K) * 8 <= C["kModelLdsBytes"]


def chunking(n, slab_doubles, cus=NUM_CUS):
    """(blocks, frames per block, capped by the slab budget) as the host's chunking() decides them."""
    t = C["kTile"]
    g0 = min(-(-n // t), 2 * cus)
    cap = max(1, C["kPartialBudget"] // (slab_doubles * 8))
    g = max(min(g0, cap), 1)
    c = -(-n // g)
    c = -(-c // t) * t
    return max(1, -(-n // max(c, 1))), max(c, t), cap < g0


def train_slab(K, d):
    return K * (d + 1) * (d + 2) // 2 + 1


def colstats_split(E):
    """(lanes per entry, entry rounds) of colstats_kernel for E entries."""
    S = BLOCK // E if E <= BLOCK // 2 else 1
    per = BLOCK // S
    return S, -(-E // per)


def test_constants_are_read():
    assert C["kTile"] == 32 and C["kMaxDim"] == 64 and C["kMaxK"] == 64
    assert C["kModelLdsBytes"] > 0 and C["kPartialBudget"] > 0


def test_cases_are_in_range():
    for K, d, n, _ in GMM_CASES:
        assert 1 <= K <= C["kMaxK"] and 1 <= d <= C["kMaxDim"] and n >= K
    assert max(K for K, *_ in GMM_CASES) == C["kMaxK"] and max(d for _, d, *_ in GMM_CASES) == C["kMaxDim"]
    assert max(STD_DIMS) == C["kMaxDim"]
    for A, d in VOTE_CASES:
        assert A ** d < 2 ** 63 and A <= 256


def test_lds_boundary_is_straddled():
    shapes = {(K, d) for K, d, *_ in GMM_CASES}
    # along K at d = 12, and along d at K = 26: the last shape that fits and the first that does not
    k_edge = max(K for K in range(1, C["kMaxK"] + 1) if model_fits_lds(K, 12))
    assert k_edge < C["kMaxK"]
    assert (k_edge, 12) in shapes and (k_edge + 1, 12) in shapes
    d_edge = max(d for d in range(1, C["kMaxDim"] + 1) if model_fits_lds(26, d))
    assert (26, d_edge) in shapes and (26, d_edge + 1) in shapes
    # the largest model is read from global memory
    assert not model_fits_lds(C["kMaxK"], C["kMaxDim"])


def test_slab_budget_boundary_is_straddled():
    capped = {(K, d): chunking(n, train_slab(K, d))[2] for K, d, n, _ in GMM_CASES}
    assert any(capped.values()) and not all(capped.values())
    # at K = kMaxK the first dimension whose slab caps the grid, and the one before it
    K = C["kMaxK"]
    d_edge = min(d for d in range(1, C["kMaxDim"] + 1) if chunking(20000, train_slab(K, d))[2])
    assert capped.get((K, d_edge - 1)) is False and capped.get((K, d_edge)) is True
    assert capped[(C["kMaxK"], C["kMaxDim"])] and not model_fits_lds(C["kMaxK"], C["kMaxDim"])
    # the capped grid still covers every frame with whole tiles and its slabs stay within the budget
    for K, d, n, _ in GMM_CASES:
        G, chunk, _ = chunking(n, train_slab(K, d))
        assert chunk % C["kTile"] == 0 and (G - 1) * chunk < n <= G * chunk
        assert G * train_slab(K, d) * 8 <= max(C["kPartialBudget"], train_slab(K, d) * 8)


def test_colstats_splits_are_straddled():
    # the start covariance pass has E = d (d + 1) / 2 entries; the standardiser's passes E = d
    dims = {d for _, d, *_ in GMM_CASES}
    E = lambda d: d * (d + 1) // 2                                        # noqa: E731
    one_lane = min(d for d in range(1, C["kMaxDim"] + 1) if colstats_split(E(d))[0] == 1)
    assert one_lane - 1 in dims and one_lane in dims                    # several lanes per entry -> one
    two_rounds = min(d for d in range(1, C["kMaxDim"] + 1) if colstats_split(E(d))[1] > 1)
    assert two_rounds - 1 in dims and two_rounds in dims                # one round of entries -> several
    assert colstats_split(E(C["kMaxDim"]))[1] > 2
    # the standardiser: all lanes on one entry, and lanes that leave part of the block idle (S E < 256)
    assert colstats_split(1) == (BLOCK, 1) and 1 in STD_DIMS and 1 in dims
    assert any(colstats_split(d)[0] * d < BLOCK for d in STD_DIMS)


def test_tile_edges_are_covered():
    t = C["kTile"]
    ns = {n for K, d, n, _ in GMM_CASES if (K, d) == (26, 12)}
    assert {26, t - 1, t, t + 1, 2 * t + 1} <= ns                      # n = K, around one tile, past two
    assert any(n >= 1 << 20 for n in ns)
    assert {1, 2, t + 1} <= set(STD_NS) and max(STD_NS) >= 1 << 20


@pytest.mark.parametrize("iters", [5, 10])
def test_restatement_is_shift_invariant(iters):
    # the reference the GPU's unstandardised cases are held to: EM on x + 1e3 is EM on x moved by 1e3.  The residue
    # (up to about 1e-10 here) is EM amplifying the rounding of x + 1e3, so 1e-9 is the bound, not a tighter one.
    x = _mixture()
    rows = init_rows(len(x), 26, seed=3)
    a = ref.gmm_train(x, rows, 0.1, iters)
    b = ref.gmm_train(x + 1e3, rows, 0.1, iters)
    assert a["iters"] == b["iters"] == iters
    assert _close(b["covs"], a["covs"], 1e-9)
    assert _close(b["means"] - 1e3, a["means"], 1e-9)
    assert _close(b["weights"], a["weights"], 1e-9)
    assert np.isclose(b["log_lik"], a["log_lik"], rtol=1e-9, atol=0)
