"""A LiveMosaic whose poll the mosaicker refuses after some slices (the uncommitted stretch fills the memory it may own):
the frames those slices committed are kept, and the flush the message asks for then gives the mosaic of what was consumed.
The frames are the test's own (tests/live_mosaic_ref.py decides where the refusal falls), fed through push in place of
follow; everything else is the LiveMosaic and the Mosaicker as they are."""
import numpy as np
import pytest

import live_mosaic_ref as ref
import mosaic_ref
import mosaicker_gpu as mg
from soundsym_amd import LiveMosaic, SsymError
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu


class _Fed:
    """a Mosaicker whose follow pushes the next block of the test's frames"""

    def __init__(self, mk, blocks):
        self.mk, self.blocks = mk, list(blocks)

    def follow(self, stream):
        return self.mk.push(self.blocks.pop(0))

    def __getattr__(self, name):
        return getattr(self.mk, name)


def test_a_refused_poll_keeps_what_it_committed_and_a_flush_then_works():
    rng = np.random.default_rng(0x7A61)
    segs = [mosaic_ref._real(rng, (n, 3)) for n in (30, 25)]
    x = np.concatenate([segs[0][5:25], mosaic_ref._real(rng, (96, 3))])[:96]    # a span that commits, then nothing like anything
    penalty, G, dim, ring = 20.0, 55, 3, 16
    # where a ring that cannot grow refuses one push of x: a slice is what the ring leaves beside the uncommitted stretch
    c = ref.commits(segs, x, penalty)
    n, done = 0, -1
    while n - (done + 1) < ring:
        n += ring - (n - (done + 1))
        done = c[n - 1]
    assert n < 96 and done >= 0, (n, done)                                       # refused part-way, with frames committed
    col = G + 4 + 8 * dim
    budget = G * (1 + 8 * dim) + 16 + (56 * G + 24 + 128) + 20 * col            # room for a ring of 16 columns, not of 32
    with mg.Dict(segs, dim) as D, mg.hooks(SSYM_MOSAICKER_SCRATCH_BYTES=budget):
        mk = D.e.mosaicker(D.d, 1, penalty)
        assert mk.counts()[1] == ring
        live = LiveMosaic([None], None, _Fed(mk, [x[:3], x[3:]]), penalty)
        assert live.poll() == []
        with pytest.raises(SsymError) as err:
            live.poll()
        assert err.value.code == nat.SSYM_E_UNSUPPORTED and "flush" in str(err.value)
        consumed, covered, committed, total = live.pending()
        assert (int(consumed[0]), int(committed[0])) == (n, done + 1)
        src, frame, cost, start = live.committed()[0]
        assert src.size == done + 1                                              # the refused poll's frames were taken
        got = live.flush()
        assert [l for l, _ in got] == [0] * len(got) and got[0][1].start_frame == 0 and got[-1][1].end_frame == n - 1
        assert all(a[1].end_frame + 1 == b[1].start_frame for a, b in zip(got, got[1:]))
        src, frame, cost, start = live.committed()[0]
        frames = [(j, int(src[j]), int(frame[j]), float(cost[j]), int(start[j])) for j in range(src.size)]
        mg.same_as_offline(D, frames, x[:n], penalty)
        mosaic = live.mosaics()[0]
        assert mosaic.num_frames == n and [p.start_frame for p in mosaic.pieces] == [p.start_frame for _, p in got]
        assert np.float64(mosaic.total).tobytes() == np.float64(total[0]).tobytes()
        live.close()
