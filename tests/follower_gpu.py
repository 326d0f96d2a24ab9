"""ssym_follower_* through ctypes into sentinel-filled outputs -- what the GPU tests of live envelope following share.  Test
infrastructure; needs the GPU only when called.

A Follower here is the bare handle: push / flush return the code, the message and the count the call left; read() fetches the
call's logs into outputs filled with sentinels, with slack behind every end.  Live pairs a handle with the restatement
(tests/live_follow_ref.py LiveFollower) and holds every call's samples, pcm and gains to it, bit for bit."""
import ctypes

import numpy as np

import follow_ref as fr
import live_follow_ref as lf
from follow_gpu import SENT32, SENTF, SENTG, SLACK, same_bits  # noqa: F401
from soundsym_amd import _native as nat

SENTN = 0xDEADBEEFCAFEF00D       # what out_n_samples holds before a call
SENTO = 0xABABABABABABABAB       # ... and the offset outputs


class Call:
    def __init__(self, rc, message, n):
        self.rc, self.message, self.n = rc, message, n
        self.untouched = n == SENTN


class Logs:
    """What ssym_follower_samples left: code, message, offsets, the three logs up to their ends (None where the pointer was
    NULL), whether the sentinels past every end are intact and whether every output is still all sentinel."""

    def __init__(self, rc, message, off, g_off, out, pcm, gain, held):
        self.rc, self.message, self.off, self.g_off = rc, message, off, g_off
        total, n_gains = held if rc == nat.SSYM_OK else (0, 0)       # held: what the logs hold, by the object's own offsets
        sent = {"out": SENTF, "pcm": SENT32, "gain": SENTG}
        full = {"out": out, "pcm": pcm, "gain": gain}
        ends = {"out": total, "pcm": total, "gain": n_gains}
        self.slack_intact = all(np.all(full[k][ends[k]:] == sent[k]) for k in full if full[k] is not None)
        self.untouched = all(np.all(full[k] == sent[k]) for k in full if full[k] is not None) and \
            all(np.all(o == SENTO) for o in (off, g_off) if o is not None)
        self.out, self.pcm, self.gain = (None if full[k] is None else full[k][:ends[k]] for k in ("out", "pcm", "gain"))


def _message(e):
    return (nat.lib().ssym_last_error(e.ctx) or b"").decode()


class Follower:
    def __init__(self, e, n_lanes=1, max_gain=fr.MAX_GAIN):
        self.e, self.n_lanes = e, n_lanes
        out = ctypes.c_void_p()
        self.rc = nat.lib().ssym_follower_create(e.ctx, n_lanes, float(max_gain), ctypes.byref(out))
        self.message = _message(e)
        self.ptr = out.value

    def push(self, ys, xs, y_dev=False, x_dev=False, flags=None, null=(), off=None, r_off=None, ctx=None, ptr="own"):
        """ys, xs: per lane the new samples (None: nothing).  y_dev / x_dev: that side in device memory.  null: "samples",
        "ref", "off", "r_off", "count" passed as NULL.  off / r_off: offsets instead of the ones the amounts give."""
        arr = lambda parts: np.concatenate([np.zeros(0)] + [np.asarray(p, dtype=np.float64).reshape(-1) for p in parts if p is not None])  # noqa: E731
        sizes = lambda parts: np.concatenate([[0], np.cumsum([0 if p is None else np.asarray(p).size for p in parts])]).astype(np.uint64)  # noqa: E731
        y, x = arr(ys), arr(xs)
        off = sizes(ys) if off is None else np.ascontiguousarray(off, dtype=np.uint64)
        r_off = sizes(xs) if r_off is None else np.ascontiguousarray(r_off, dtype=np.uint64)
        keep = []

        def place(a, dev):
            if not dev:
                return a.ctypes.data if a.size else None
            import torch
            t = torch.from_numpy(a if a.size else np.zeros(1)).cuda()
            torch.cuda.synchronize()
            keep.append(t)
            return t.data_ptr()
        fl = (nat.FOLLOW_SAMPLES_DEVICE if y_dev else 0) | (nat.FOLLOW_REF_DEVICE if x_dev else 0)
        n = ctypes.c_uint64(SENTN)
        p = lambda key, value: None if key in null else value      # noqa: E731
        rc = nat.lib().ssym_follower_push(self.e.ctx if ctx is None else ctx, self.ptr if ptr == "own" else ptr,
                                          p("samples", place(y, y_dev)), p("off", off.ctypes.data), p("ref", place(x, x_dev)),
                                          p("r_off", r_off.ctypes.data), fl if flags is None else flags,
                                          p("count", ctypes.byref(n)))
        return Call(rc, _message(self.e), int(n.value))

    def flush(self, lane, null=(), ptr="own"):
        n = ctypes.c_uint64(SENTN)
        rc = nat.lib().ssym_follower_flush(self.e.ctx, self.ptr if ptr == "own" else ptr, lane,
                                           None if "count" in null else ctypes.byref(n))
        return Call(rc, _message(self.e), int(n.value))

    def read(self, out_dev=False, want=("off", "out", "pcm", "g_off", "gain"), flags=None, room=None, ptr="own"):
        """The last call's logs.  room: (samples, gains) to size the outputs by; default: what the offsets say."""
        lib = nat.lib()
        o, g = np.zeros(self.n_lanes + 1, dtype=np.uint64), np.zeros(self.n_lanes + 1, dtype=np.uint64)
        assert lib.ssym_follower_samples(self.e.ctx, self.ptr, o.ctypes.data, None, None, g.ctypes.data, None, 0) == nat.SSYM_OK
        held = int(o[-1]), int(g[-1])
        total, n_gains = held if room is None else room
        off, g_off = (np.full(self.n_lanes + 1, SENTO, dtype=np.uint64) for _ in range(2))
        out, pcm, gain = np.full(total + SLACK, SENTF), np.full(total + SLACK, SENT32, dtype=np.int32), np.full(n_gains + SLACK, SENTG)
        if out_dev:
            import torch
            d = {k: torch.from_numpy(v).cuda() for k, v in (("out", out), ("pcm", pcm), ("gain", gain))}
            torch.cuda.synchronize()
            ptrs = {k: t.data_ptr() for k, t in d.items()}
        else:
            ptrs = {"out": out.ctypes.data, "pcm": pcm.ctypes.data, "gain": gain.ctypes.data}
        ptrs.update(off=off.ctypes.data, g_off=g_off.ctypes.data)
        rc = lib.ssym_follower_samples(self.e.ctx, self.ptr if ptr == "own" else ptr,
                                       *(ptrs[k] if k in want else None for k in ("off", "out", "pcm", "g_off", "gain")),
                                       (nat.OUT_DEVICE if out_dev else 0) if flags is None else flags)
        message = _message(self.e)
        if out_dev:
            torch.cuda.synchronize()
            out, pcm, gain = (d[k].cpu().numpy() for k in ("out", "pcm", "gain"))
        have = dict(off=off, g_off=g_off, out=out, pcm=pcm, gain=gain)
        return Logs(rc, message, *(have[k] if k in want else None for k in ("off", "g_off", "out", "pcm", "gain")), held)

    def counts(self):
        ny, nx, rel = (np.zeros(self.n_lanes, dtype=np.uint64) for _ in range(3))
        assert nat.lib().ssym_follower_counts(self.ptr, ny.ctypes.data, nx.ctypes.data, rel.ctypes.data) == nat.SSYM_OK
        return [int(v) for v in ny], [int(v) for v in nx], [int(v) for v in rel]

    def reset(self, lane):
        rc = nat.lib().ssym_follower_reset(self.e.ctx, self.ptr, lane)
        return Call(rc, _message(self.e), SENTN)

    def close(self):
        if self.ptr:
            assert nat.lib().ssym_follower_destroy(self.e.ctx, self.ptr) == nat.SSYM_OK
        self.ptr = None


def assert_logs(logs, want, what=""):
    """want: per lane (samples, gains), the restatement's answer for the call."""
    assert logs.rc == nat.SSYM_OK, (what, logs.rc, logs.message)
    assert logs.slack_intact, what
    want_off = np.concatenate([[0], np.cumsum([o.size for o, _ in want])]).astype(np.uint64)
    want_g_off = np.concatenate([[0], np.cumsum([g.size for _, g in want])]).astype(np.uint64)
    want_out = np.concatenate([np.zeros(0)] + [o for o, _ in want])
    want_gain = np.concatenate([np.zeros(0)] + [g for _, g in want])
    if logs.off is not None:
        assert np.array_equal(logs.off, want_off), (what, "out_lane_offsets", logs.off, want_off)
    if logs.g_off is not None:
        assert np.array_equal(logs.g_off, want_g_off), (what, "out_gain_offsets", logs.g_off, want_g_off)
    if logs.out is not None:
        assert same_bits(logs.out, want_out), (what, "out_samples")
    if logs.pcm is not None:
        assert np.array_equal(logs.pcm, fr.pcm32(want_out)), (what, "out_pcm32")
    if logs.gain is not None:
        assert same_bits(logs.gain, want_gain), (what, "out_gain")


class Live:
    """A handle and the restatement side by side: every call goes to both and is held, bit for bit; the released samples and
    the settled gains are collected lane by lane."""

    def __init__(self, e, n_lanes=1, max_gain=fr.MAX_GAIN):
        self.fl, self.ref = Follower(e, n_lanes, max_gain), lf.LiveFollower(n_lanes, max_gain)
        assert self.fl.rc == nat.SSYM_OK, self.fl.message
        self.outs, self.gains = [[] for _ in range(n_lanes)], [[] for _ in range(n_lanes)]

    def _held(self, call, want, what, **read_kw):
        assert call.rc == nat.SSYM_OK, (what, call.rc, call.message)
        assert call.n == sum(o.size for o, _ in want), (what, call.n)
        assert_logs(self.fl.read(**read_kw), want, what)
        assert self.fl.counts() == self.ref.counts(), what
        for l, (o, g) in enumerate(want):
            self.outs[l].append(o)
            self.gains[l].append(g)

    def push(self, ys, xs, what="", out_dev=False, **kw):
        self._held(self.fl.push(ys, xs, **kw), self.ref.push(ys, xs), what, out_dev=out_dev)

    def flush(self, lane, what="", out_dev=False):
        want = [(np.zeros(0), np.zeros(0))] * len(self.ref.lanes)
        want[lane] = self.ref.flush(lane)
        self._held(self.fl.flush(lane), want, what, out_dev=out_dev)

    def reset(self, lane):
        assert self.fl.reset(lane).rc == nat.SSYM_OK
        self.ref.reset(lane)
        self.outs[lane], self.gains[lane] = [], []

    def total(self, lane):
        return (np.concatenate([np.zeros(0)] + self.outs[lane]), np.concatenate([np.zeros(0)] + self.gains[lane]))

    def close(self):
        self.fl.close()


def feed(live, lane_pairs, cuts, what="", **kw):
    """Every lane of `live` fed its (y, x) by the same cuts (a list of (my, mx); the rest goes in with a last push)."""
    at = [[0, 0] for _ in lane_pairs]
    for i, (my, mx) in enumerate(list(cuts) + [(1 << 60, 1 << 60)]):
        ys = [y[a[0]:a[0] + my] for (y, _), a in zip(lane_pairs, at)]
        xs = [x[a[1]:a[1] + mx] for (_, x), a in zip(lane_pairs, at)]
        for a, y, x in zip(at, ys, xs):
            a[0], a[1] = a[0] + len(y), a[1] + len(x)
        if i < len(cuts) or any(len(v) for v in ys + xs):
            live.push(ys, xs, "%s push %d" % (what, i), **kw)
