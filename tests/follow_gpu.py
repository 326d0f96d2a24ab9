"""ssym_follow_envelope through ctypes into sentinel-filled outputs -- what the GPU tests of envelope following share.  Test
infrastructure; needs the GPU only when called."""
import numpy as np

import follow_ref as fr
from soundsym_amd import _native as nat

SENTF, SENT32, SENTG = -12345.5, -559038737, -777.25
SLACK = 7                    # values of sentinel past every output's end


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Result:
    """What one call left behind: code, message, the three outputs up to their ends (None where the pointer was NULL), whether
    the sentinels past every end are intact and whether every output is still all sentinel."""

    def __init__(self, rc, message, out, pcm, gain, total, n_gains):
        self.rc, self.message = rc, message
        sent = {"out": SENTF, "pcm": SENT32, "gain": SENTG}
        full = {"out": out, "pcm": pcm, "gain": gain}
        ends = {"out": total, "pcm": total, "gain": n_gains}
        self.slack_intact = all(np.all(full[k][ends[k]:] == sent[k]) for k in full if full[k] is not None)
        self.untouched = all(np.all(full[k] == sent[k]) for k in full if full[k] is not None)
        self.out, self.pcm, self.gain = (None if full[k] is None else full[k][:ends[k]] for k in ("out", "pcm", "gain"))


def call(e, y, off, x, r_off, max_gain=8.0, y_dev=False, x_dev=False, out_dev=False, want=("out", "pcm", "gain"), flags=None,
         null=(), in_place=False, n_targets=None, room=None):
    """One call.  y_dev / x_dev / out_dev: that side in device memory (torch tensors).  want: the outputs given a pointer.
    in_place (with y_dev and out_dev): out_samples is the samples' own device buffer.  null: "ctx", "samples", "ref", "off",
    "r_off" passed as NULL.  flags: instead of the ones the placement asks for.  room: (total, gains) to size the outputs by
    when the offsets are not to be trusted."""
    y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    off = np.ascontiguousarray(off, dtype=np.uint64).reshape(-1)
    r_off = np.ascontiguousarray(r_off, dtype=np.uint64).reshape(-1)
    n = off.size - 1 if n_targets is None else n_targets
    total, n_gains = room if room is not None else (int(off[-1]), int(fr.gain_offsets(off)[-1]))
    out = np.full(total + SLACK, SENTF)
    pcm = np.full(total + SLACK, SENT32, dtype=np.int32)
    gain = np.full(n_gains + SLACK, SENTG)
    keep = []
    if y_dev or x_dev or out_dev:
        import torch

        def dev(a):
            t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            keep.append(t)
            return t
    fl = (nat.FOLLOW_SAMPLES_DEVICE if y_dev else 0) | (nat.FOLLOW_REF_DEVICE if x_dev else 0) | (nat.OUT_DEVICE if out_dev else 0)
    if in_place:
        assert y_dev and out_dev and y.size == total
        d_y = dev(np.concatenate([y, np.full(SLACK, SENTF)]))
        y_p = d_y.data_ptr()
    else:
        d_y = dev(y if y.size else np.zeros(1)) if y_dev else None
        y_p = d_y.data_ptr() if y_dev else (y.ctypes.data if y.size else None)
    d_x = dev(x if x.size else np.zeros(1)) if x_dev else None
    x_p = d_x.data_ptr() if x_dev else (x.ctypes.data if x.size else None)
    if out_dev:
        d_out, d_pcm, d_gain = (d_y if in_place else dev(out)), dev(pcm), dev(gain)
        torch.cuda.synchronize()
        ptr = {"out": d_out.data_ptr(), "pcm": d_pcm.data_ptr(), "gain": d_gain.data_ptr()}
    else:
        ptr = {"out": out.ctypes.data, "pcm": pcm.ctypes.data, "gain": gain.ctypes.data}
    p = lambda key, value: None if key in null else value      # noqa: E731
    rc = nat.lib().ssym_follow_envelope(p("ctx", e.ctx), p("samples", y_p), p("off", off.ctypes.data), n, p("ref", x_p),
                                        p("r_off", r_off.ctypes.data), float(max_gain), fl if flags is None else flags,
                                        *(ptr[k] if k in want else None for k in ("out", "pcm", "gain")))
    message = (nat.lib().ssym_last_error(e.ctx) or b"").decode()
    if out_dev:
        torch.cuda.synchronize()
        out, pcm, gain = d_out.cpu().numpy(), d_pcm.cpu().numpy(), d_gain.cpu().numpy()
    full = {"out": out, "pcm": pcm, "gain": gain}
    return Result(rc, message, *(full[k] if k in want else None for k in ("out", "pcm", "gain")), total, n_gains)


def assert_matches(res, want_out, want_pcm, want_gain, what=""):
    """The outputs the call was given, bit for bit, and the sentinels past their ends."""
    assert res.rc == nat.SSYM_OK, (what, res.rc, res.message)
    assert res.slack_intact, what
    if res.out is not None:
        assert same_bits(res.out, want_out), (what, "out_samples")
    if res.pcm is not None:
        assert np.array_equal(res.pcm, want_pcm), (what, "out_pcm32")
    if res.gain is not None:
        assert same_bits(res.gain, want_gain), (what, "out_gain")
