"""What the GPU tests of the cover share -- TEST INFRASTRUCTURE: ssym_dtw_cover through ctypes into sentinel-filled outputs
and the comparison against tests/cover_ref.py, on paced_match_gpu's Sets."""
import numpy as np

import cover_ref as ref
from paced_match_gpu import SENT32, SENTF, Sets, bits, error, real  # noqa: F401
from soundsym_amd import _native as nat

INF = float("inf")
NAMES = ("count", "total", "src", "start", "end", "cost")


def call(sets, penalty=0.0, device=False, flags=0):
    """ssym_dtw_cover into sentinel-filled outputs with one entry more than each needs:
    (rc, (count, total, src, start, end, cost), untouched)."""
    m, frames = len(sets.tgt), int(sum(np.asarray(x).shape[0] for x in sets.tgt))
    sizes = (m, m, frames, frames, frames, frames)
    outs = [np.full(n + 1, SENTF) if k in (1, 5) else np.full(n + 1, SENT32, dtype=np.uint32) for k, n in enumerate(sizes)]
    head = (sets.e.ctx, sets.d.ptr, sets.q.ptr, float(penalty))
    if device:
        import torch
        dev = [torch.from_numpy(o if o.dtype == np.float64 else o.view(np.int32)).cuda() for o in outs]
        torch.cuda.synchronize()
        rc = nat.lib().ssym_dtw_cover(*head, flags | nat.OUT_DEVICE, *(d.data_ptr() for d in dev))
        torch.cuda.synchronize()
        outs = [d.cpu().numpy() if o.dtype == np.float64 else d.cpu().numpy().view(np.uint32) for d, o in zip(dev, outs)]
    else:
        rc = nat.lib().ssym_dtw_cover(*head, flags, *(o.ctypes.data for o in outs))
    sent = lambda o: SENTF if o.dtype == np.float64 else SENT32
    untouched = all(o[n] == sent(o) for o, n in zip(outs, sizes))
    if rc != nat.SSYM_OK:
        untouched = untouched and all((o == sent(o)).all() for o in outs)
    return rc, tuple(o[:n] for o, n in zip(outs, sizes)), bool(untouched)


def same(got, want):
    """The six arrays bit for bit; the first difference otherwise."""
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (name, g.shape, w.shape)
        eq = bits(g) == bits(w) if w.dtype == np.float64 else g == w
        assert eq.all(), (name, int(np.flatnonzero(~eq)[0]), g[~eq][:4].tolist(), w[~eq][:4].tolist())


def check(sets, penalty=0.0, want=None, **kw):
    """The call against the restatement: counts, totals, the four piece arrays and the padding of the unused slots."""
    rc, got, untouched = call(sets, penalty, **kw)
    assert rc == nat.SSYM_OK, error(sets)
    assert untouched
    if want is None:
        want = ref.arrays(sets.src, sets.tgt, penalty, sets.squared)
    same(got, want)
    return got


def pieces_of(got, tgt, t):
    """[(src, start, end, cost)] of target t."""
    off = int(sum(np.asarray(x).shape[0] for x in tgt[:t]))
    return [(int(got[2][k]), int(got[3][k]), int(got[4][k]), float(got[5][k])) for k in range(off, off + int(got[0][t]))]
