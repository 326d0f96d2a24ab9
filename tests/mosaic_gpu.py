"""What the GPU tests of the mosaic share -- TEST INFRASTRUCTURE: ssym_dtw_mosaic through ctypes into sentinel-filled outputs
one entry too long, host and SSYM_OUT_DEVICE, and the comparison against tests/mosaic_ref.py, on paced_match_gpu's Sets."""
import numpy as np

import mosaic_ref as ref
from paced_match_gpu import SENT32, SENTF, Sets, bits, error, real  # noqa: F401
from soundsym_amd import _native as nat

INF, NAN = float("inf"), float("nan")
GAP, NONE = ref.GAP, ref.NONE
NAMES = ("count", "total", "start", "src", "frame", "frame_cost")


def offsets(tgt):
    return np.concatenate([[0], np.cumsum([np.asarray(x).shape[0] for x in tgt])]).astype(np.int64)


def call(sets, penalty=0.0, gap_cost=INF, device=False, flags=0, keep=(True,) * 6):
    """ssym_dtw_mosaic into sentinel-filled outputs with one entry more than each needs; keep[k] False passes NULL for
    output k: (rc, (count, total, start, src, frame, frame_cost), untouched)."""
    m, frames = len(sets.tgt), int(offsets(sets.tgt)[-1])
    sizes = (m, m, frames, frames, frames, frames)
    outs = [np.full(n + 1, SENTF) if k in (1, 5) else np.full(n + 1, SENT32, dtype=np.uint32) for k, n in enumerate(sizes)]
    head = (sets.e.ctx, sets.d.ptr, sets.q.ptr, float(penalty), float(gap_cost))
    if device:
        import torch
        dev = [torch.from_numpy(o if o.dtype == np.float64 else o.view(np.int32)).cuda() for o in outs]
        torch.cuda.synchronize()
        rc = nat.lib().ssym_dtw_mosaic(*head, flags | nat.OUT_DEVICE, *(d.data_ptr() if k else None for d, k in zip(dev, keep)))
        torch.cuda.synchronize()
        outs = [d.cpu().numpy() if o.dtype == np.float64 else d.cpu().numpy().view(np.uint32) for d, o in zip(dev, outs)]
    else:
        rc = nat.lib().ssym_dtw_mosaic(*head, flags, *(o.ctypes.data if k else None for o, k in zip(outs, keep)))
    sent = lambda o: SENTF if o.dtype == np.float64 else SENT32
    untouched = all(o[n] == sent(o) for o, n in zip(outs, sizes))
    untouched = untouched and all((o == sent(o)).all() for o, k in zip(outs, keep) if not k)
    if rc != nat.SSYM_OK:
        untouched = untouched and all((o == sent(o)).all() for o in outs)
    return rc, tuple(o[:n] for o, n in zip(outs, sizes)), bool(untouched)


def same(got, want, keep=(True,) * 6):
    """The six arrays bit for bit; the first difference otherwise."""
    for name, g, w, k in zip(NAMES, got, want, keep):
        if not k:
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (name, g.shape, w.shape)
        eq = bits(g) == bits(w) if w.dtype == np.float64 else g == w
        assert eq.all(), (name, int(np.flatnonzero(~eq)[0]), g[~eq][:4].tolist(), w[~eq][:4].tolist())


def check(sets, penalty=0.0, gap_cost=INF, want=None, **kw):
    """The call against the restatement: all six outputs and the padding of the unused slots."""
    rc, got, untouched = call(sets, penalty, gap_cost, **kw)
    assert rc == nat.SSYM_OK, error(sets)
    assert untouched
    if want is None:
        want = ref.arrays(sets.src, sets.tgt, penalty, gap_cost, sets.squared)
    same(got, want, kw.get("keep", (True,) * 6))
    return got


def pieces_of(got, tgt, t):
    return ref.pieces_of(got, offsets(tgt), t)
