"""The refusals of the three lane-fed objects word for word: ssym_spotter_*, ssym_coverer_* and ssym_mosaicker_* push,
follow, flush, reset, events / pieces / frames and best.  Every refusal's code and exact ssym_last_error text, the entry
point's own name and the object's noun in it, and for every two faults one call can have, in the order of the checks

    push   : handle, NULL frame_offsets / count, (coverer, mosaicker) dictionary appended to, then lane by lane: offsets
             decrease, (coverer, mosaicker) the lane has ended, lane limit; then NULL feats
    follow : handle, NULL stream / count, (coverer, mosaicker) dictionary appended to, the stream's context, the stream's
             shape, then lane by lane: holds fewer than consumed (an ended lane too), lane limit
    flush  : handle, lane / NULL count     reset : handle, lane     events / pieces / frames, best : handle

one call with both that reports the earlier one.  The count output is sentinel-filled and stays untouched on every refusal,
and so do the object's counts and best; the accepted calls after the refusals give, bit for bit, what they give an object
that was never refused anything.  Every refusal is made on the host before any device work (the lane limit by an offsets
array [0, 2^31]).  2 lanes, dim 3, targets of 4 and 6 frames, a dictionary of 3 segments of 3 to 5 frames, pushes of at
most 11 frames, streams of (3 lanes, 3 coefficients) and (2 lanes, 12 coefficients) for the shape refusals."""
import ctypes

import numpy as np
import pytest

from soundsym_amd import Engine
from soundsym_amd import _native as nat
from soundsym_amd.engine import pack_segments

pytestmark = pytest.mark.gpu

OK, INV, UNS = nat.SSYM_OK, nat.SSYM_E_INVALID, nat.SSYM_E_UNSUPPORTED
SENT = 77
LANES, DIM = 2, 3
COUNT = {"spotter": "out_n_events", "coverer": "out_n_pieces", "mosaicker": "out_n_frames"}
READ = {"spotter": "events", "coverer": "pieces", "mosaicker": "frames"}
TILINGS = ["coverer", "mosaicker"]                       # a flushed lane has ended, and push and follow read the dictionary

# {fn}: the entry point, {noun}: spotter / coverer / mosaicker, {count}: out_n_events / out_n_pieces / out_n_frames
NULL_HANDLE = "{fn}: the {noun} handle is NULL"
FOREIGN = "{fn}: the {noun} belongs to another context"
PUSH_NULL = "{fn}: frame_offsets and {count} must not be NULL"
APPENDED = "{fn}: the dictionary was appended to after the {noun} was created; create a new {noun}"
DECREASE = "{fn}: frame_offsets decrease"
ENDED = "{fn}: lane {lane} was flushed and has ended; call ssym_{noun}_reset"
LIMIT = "{fn}: lane {lane} would consume more than 2^31 - 1 = 2147483647 frames"
FEATS = "{fn}: feats is NULL"
FOLLOW_NULL = "{fn}: stream and {count} must not be NULL"
STREAM_CTX = "{fn}: the stream belongs to another context"
SHAPE = "{fn}: the stream has {lanes} lanes of {nc} coefficients, the {noun} 2 lanes of 3 values"
FEWER = ("{fn}: lane {lane} of the stream holds {held} frames, fewer than the {consumed} consumed: "
         "after ssym_stream_reset call ssym_{noun}_reset")
FLUSH_LANE = "{fn}: lane outside the {noun}'s lanes, or {count} is NULL"
RESET_LANE = "{fn}: lane outside the {noun}'s lanes"


def _off(*v):
    return np.array(v, dtype=np.uint64)


class _World:
    """Two engines; on the first the query set, two dictionaries (the second is there to be appended to), the frames that are
    pushed and the streams; on the second a stream of a foreign context."""

    def __init__(self):
        rng = np.random.default_rng(0x1A9EFEED)
        self.e, self.other = Engine(dtype="f64"), Engine(dtype="f64")
        segs = [rng.standard_normal((n, DIM)) for n in (3, 4, 5)]
        self.segs = pack_segments(segs, DIM, np.float64)
        self.d, self.d2 = self.e.dictionary(*self.segs, DIM), self.e.dictionary(*self.segs, DIM)
        self.q = self.e.queries(*pack_segments([rng.standard_normal((n, DIM)) for n in (4, 6)], DIM, np.float64), DIM)
        # the recordings pass through the segments, so that there is something to spot and something to cover
        self.x = np.ascontiguousarray(np.concatenate([segs[1], segs[0], rng.standard_normal((4, DIM)), segs[2], segs[1],
                                                      segs[2], segs[0]]))
        self.waves = [rng.standard_normal(1024 + 256 * 9) * 0.3, np.sin(0.03 * np.arange(1024 + 256 * 7))]    # 10 and 8 frames
        self.st3, self.st12 = self.e.stream(3, 44100.0, 3), self.e.stream(2, 44100.0, 12)
        self.foreign = self.other.stream(3, 44100.0, 3)

    def make(self, noun, d=None):
        if noun == "spotter":
            return self.e.spotter(self.q, LANES)
        return getattr(self.e, noun)(d or self.d, LANES, 0.5)

    def fill(self, st):
        st.push(np.concatenate(self.waves), _off(0, self.waves[0].size, self.waves[0].size + self.waves[1].size))

    def close(self):
        self.e.close()
        self.other.close()


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.close()


class _Calls:
    """The entry points of one object by their short names, every one into a sentinel-filled count."""

    def __init__(self, w, noun, obj):
        self.w, self.noun, self.obj, self.L = w, noun, obj, nat.lib()
        self.n = ctypes.c_uint64(SENT)
        self.u, self.f = np.full(64, SENT, dtype=np.uint32), np.full(64, -1.5)
        self.fill, self.last, self.total = {}, 0, 0      # what a message's {lane}, {held} ... stand for; the counts given

    def fn(self, name):
        return getattr(self.L, "ssym_%s_%s" % (self.noun, name))

    def push(self, off, ctx=True, obj=True, feats=True, count=True):
        x = self.w.x
        tail = (None, None) if self.noun == "spotter" else ()
        return self.fn("push")(self._ctx(ctx), self.obj.ptr if obj else None, x.ctypes.data if feats else None,
                               None if off is None else off.ctypes.data, 0, ctypes.byref(self.n) if count else None, *tail)

    def follow(self, st, ctx=True, obj=True, count=True):
        tail = (None, None) if self.noun == "spotter" else ()
        return self.fn("follow")(self._ctx(ctx), self.obj.ptr if obj else None, None if st is None else st.ptr, 0,
                                 ctypes.byref(self.n) if count else None, *tail)

    def flush(self, lane, ctx=True, obj=True, count=True):
        return self.fn("flush")(self._ctx(ctx), self.obj.ptr if obj else None, lane, ctypes.byref(self.n) if count else None)

    def reset(self, lane, ctx=True, obj=True):
        return self.fn("reset")(self._ctx(ctx), self.obj.ptr if obj else None, lane)

    def read(self, ctx=True, obj=True):
        u, f = self.u.ctypes.data, self.f.ctypes.data
        words = {"spotter": (u, u, f, u, u), "coverer": (u, u, u, u, f), "mosaicker": (u, u, u, u, f, u)}[self.noun]
        return self.fn(READ[self.noun])(self._ctx(ctx), self.obj.ptr if obj else None, *words, 0)

    def best(self, ctx=True, obj=True):
        u, f = self.u.ctypes.data, self.f.ctypes.data
        return self.fn("best")(self._ctx(ctx), self.obj.ptr if obj else None, f, u, u, 0)

    def _ctx(self, own):
        return self.w.e.ctx if own else self.w.other.ctx

    def refused(self, name, code, text, ctx=True, **kw):
        """Call `name`: it returns `code`, leaves `text` as the last error of the context it was called on, and every
        output alone."""
        other = "coverer" if self.noun == "spotter" else "spotter"
        c = self._ctx(ctx)
        # whatever the context's last message was, it is another one now
        assert getattr(self.L, "ssym_%s_reset" % other)(c, None, 0) == INV
        assert self.L.ssym_last_error(c) == ("ssym_%s_reset: the %s handle is NULL" % (other, other)).encode()
        entry = READ[self.noun] if name == "read" else name
        rc = getattr(self, name)(ctx=ctx, **kw) if name in ("read", "best") else getattr(self, name)(kw.pop("arg"), ctx=ctx, **kw)
        want = text.format(fn="ssym_%s_%s" % (self.noun, entry), noun=self.noun, count=COUNT[self.noun], **self.fill)
        assert (rc, self.L.ssym_last_error(c)) == (code, want.encode()), (name, kw)
        assert self.n.value == SENT and (self.u == SENT).all() and (self.f == -1.5).all()

    def accept(self, name, *args):
        """Call `name`: it succeeds; the count it gave (push, follow, flush) is kept for `state`."""
        assert getattr(self, name)(*args) == OK, (name, self.L.ssym_last_error(self.w.e.ctx))
        if name != "reset":
            self.last = self.n.value
            self.total += self.last
        self.n.value = SENT

    def counts(self):
        counts = self.obj.counts()
        return (counts if self.noun == "spotter" else counts[0]).tolist()

    def state(self):
        """Everything the object answers about itself, as bytes: the frames consumed, best, and the events / pieces / frames of
        the last accepted call with their number."""
        if self.noun == "spotter":
            self.obj.n_events = self.last
            log = self.obj.events()
        elif self.noun == "coverer":
            self.obj.n_pieces = self.last
            log = self.obj.pieces()
        else:
            self.obj.n_frames = self.last
            log = self.obj.frames()
        return self.counts(), self.last, [a.tobytes() for a in self.obj.best()], [a.tobytes() for a in log]


def _handle_refusals(c, name, **kw):
    """The two refusals that come before every other, alone and in front of a second fault."""
    c.refused(name, INV, NULL_HANDLE, obj=False, **kw)
    c.refused(name, INV, FOREIGN, ctx=False, **kw)


@pytest.mark.parametrize("noun", ["spotter"] + TILINGS)
def test_every_refusal_of_push_flush_reset_and_the_reads_word_for_word_and_the_earlier_of_two(world, noun):
    w = world
    objs = [w.make(noun), w.make(noun)]                  # the second is never refused anything
    calls = [_Calls(w, noun, o) for o in objs]
    c = calls[0]
    first, second, third = _off(0, 6, 11), _off(11, 15, 15), _off(15, 19, 26)
    for k in calls:
        k.accept("push", first)
        k.accept("flush", 1)                             # lane 1 of a tiling has ended now; a spotter's goes on
    before = c.state()
    assert before == calls[1].state()
    big = 2 ** 31

    good = dict(arg=_off(0, 2, 2))
    _handle_refusals(c, "push", **good)
    c.refused("push", INV, NULL_HANDLE, obj=False, arg=None, count=False, feats=False)       # handle, NULL arguments
    c.refused("push", INV, FOREIGN, ctx=False, arg=None)                                     # another context, NULL frame_offsets
    c.refused("push", INV, PUSH_NULL, arg=None)
    c.refused("push", INV, PUSH_NULL, count=False, **good)
    c.refused("push", INV, PUSH_NULL, arg=_off(0, 4, 2), count=False)                        # NULL count, offsets decrease
    c.refused("push", INV, DECREASE, arg=_off(3, 2, 2))
    c.refused("push", INV, DECREASE, arg=_off(0, 2, 1))
    c.refused("push", INV, DECREASE, arg=_off(3, 2, 2 + big))                                # decrease on lane 0, limit on lane 1
    c.refused("push", INV, DECREASE, arg=_off(3, 2, 2), feats=False)                         # decrease, NULL feats
    c.fill = dict(lane=0)
    c.refused("push", UNS, LIMIT, arg=_off(0, big, big))
    c.refused("push", UNS, LIMIT, arg=_off(0, big - 6, big - 6))                             # 6 consumed + 2^31 - 6
    c.refused("push", UNS, LIMIT, arg=_off(0, big, 5))                                       # limit on lane 0, decrease on lane 1
    c.refused("push", UNS, LIMIT, arg=_off(0, big, big), feats=False)                        # limit, NULL feats
    c.fill = dict(lane=1)
    if noun in TILINGS:
        c.refused("push", INV, ENDED, arg=_off(0, 0, 3))
        c.refused("push", INV, ENDED, arg=_off(0, 0, big))                                   # ended and over the limit, one lane
        c.refused("push", INV, ENDED, arg=_off(0, 0, 3), feats=False)                        # ended, NULL feats
        c.refused("push", INV, DECREASE, arg=_off(3, 2, 4))                                  # decrease on lane 0, lane 1 ended
        c.fill = dict(lane=0)
        c.refused("push", UNS, LIMIT, arg=_off(0, big, big + 1))                             # limit on lane 0, lane 1 ended
    else:
        c.refused("push", UNS, LIMIT, arg=_off(0, 0, big))
        c.refused("push", UNS, LIMIT, arg=_off(0, 0, big - 5))                               # 5 consumed + 2^31 - 5
    c.refused("push", INV, FEATS, feats=False, **good)
    c.refused("push", INV, FEATS, arg=_off(7, 7, 8) if noun == "spotter" else _off(7, 8, 8), feats=False)

    _handle_refusals(c, "flush", arg=0)
    c.refused("flush", INV, NULL_HANDLE, obj=False, arg=2, count=False)                      # handle, lane / count
    c.refused("flush", INV, FOREIGN, ctx=False, arg=2)
    c.refused("flush", INV, FLUSH_LANE, arg=2)
    c.refused("flush", INV, FLUSH_LANE, arg=0xffffffff)
    c.refused("flush", INV, FLUSH_LANE, arg=0, count=False)
    _handle_refusals(c, "reset", arg=0)
    c.refused("reset", INV, NULL_HANDLE, obj=False, arg=2)                                   # handle, lane
    c.refused("reset", INV, FOREIGN, ctx=False, arg=2)
    c.refused("reset", INV, RESET_LANE, arg=2)
    c.refused("reset", INV, RESET_LANE, arg=0xffffffff)
    _handle_refusals(c, "read")
    _handle_refusals(c, "best")

    assert c.state() == before
    # on as if nothing had been asked: the same calls on both objects, the same answers
    steps = [[("push", _off(4, 4, 4), True, True, False)],                                   # no frames: feats is not looked at
             [("push", second)], [("reset", 1), ("push", third)], [("flush", 0)]]
    for step in steps:
        for k in calls:
            for call in step:
                k.accept(*call)
        assert c.state() == calls[1].state()
    assert c.counts() == [14, 7] and c.total > 0         # (and there was something to compare)
    for o in objs:
        o.close()


@pytest.mark.parametrize("noun", ["spotter"] + TILINGS)
def test_every_refusal_of_follow_word_for_word_and_the_earlier_of_two(world, noun):
    w = world
    st = w.e.stream(LANES, 44100.0, DIM)
    w.fill(st)
    obj = w.make(noun)
    c = _Calls(w, noun, obj)
    c.accept("follow", st)
    c.accept("flush", 1)                                 # 10 and 8 frames consumed; lane 1 of a tiling has ended
    before = c.state()
    assert c.counts() == [10, 8]

    _handle_refusals(c, "follow", arg=st)
    c.refused("follow", INV, NULL_HANDLE, obj=False, arg=None, count=False)                  # handle, NULL arguments
    c.refused("follow", INV, FOREIGN, ctx=False, arg=None)
    c.refused("follow", INV, FOLLOW_NULL, arg=None)
    c.refused("follow", INV, FOLLOW_NULL, arg=st, count=False)
    c.refused("follow", INV, FOLLOW_NULL, arg=w.foreign, count=False)                        # NULL count, the stream's context
    c.refused("follow", INV, STREAM_CTX, arg=w.foreign)                                      # the stream's context, its shape
    c.fill = dict(lanes=3, nc=3)
    c.refused("follow", INV, SHAPE, arg=w.st3)                                               # shape, holds fewer than consumed
    c.fill = dict(lanes=2, nc=12)
    c.refused("follow", INV, SHAPE, arg=w.st12)
    st.reset(1)
    c.fill = dict(lane=1, held=0, consumed=8)
    c.refused("follow", INV, FEWER, arg=st)                                                  # (a tiling's ended lane as well)
    st.reset(0)
    c.fill = dict(lane=0, held=0, consumed=10)
    c.refused("follow", INV, FEWER, arg=st)                                                  # fewer on both lanes: the first
    assert c.state() == before

    # both lanes reset and the stream filled again: what an object that was never refused anything gives
    fresh = _Calls(w, noun, w.make(noun))
    w.fill(st)
    c.accept("reset", 0)
    c.accept("reset", 1)
    for call in (("follow", st), ("flush", 0)):
        c.accept(*call)
        fresh.accept(*call)
        assert c.state() == fresh.state()
    assert c.counts() == [10, 8] and fresh.total > 0
    for h in (obj, fresh.obj, st):
        h.close()


def _appended_to_is_reported_in_its_place(w, noun):
    obj = w.make(noun, w.d2)
    c = _Calls(w, noun, obj)
    c.accept("push", _off(0, 3, 6))
    c.accept("flush", 1)
    before = c.state()
    w.e.dictionary_append(w.d2, *pack_segments([w.x[:4]], DIM, np.float64))
    good = _off(6, 8, 8)
    c.refused("push", INV, APPENDED, arg=good)
    c.refused("push", INV, PUSH_NULL, arg=None)                                              # NULL frame_offsets, appended to
    c.refused("push", INV, PUSH_NULL, arg=good, count=False)
    c.refused("push", INV, NULL_HANDLE, arg=good, obj=False)
    c.refused("push", INV, APPENDED, arg=_off(3, 2, 2))                                      # appended to, offsets decrease
    c.refused("push", INV, APPENDED, arg=_off(0, 0, 3))                                      # appended to, the lane has ended
    c.refused("push", INV, APPENDED, arg=_off(0, 2 ** 31, 2 ** 31))                          # appended to, lane limit
    c.refused("push", INV, APPENDED, arg=good, feats=False)                                  # appended to, NULL feats
    c.refused("push", INV, APPENDED, arg=_off(4, 4, 4))                                      # ... and a push of no frames
    c.refused("follow", INV, FOLLOW_NULL, arg=None)                                          # NULL stream, appended to
    c.refused("follow", INV, APPENDED, arg=w.foreign)                                        # appended to, the stream's context
    c.refused("follow", INV, APPENDED, arg=w.st3)                                            # appended to, the stream's shape
    # flush, reset, pieces / frames and best do not read the dictionary
    assert c.state() == before
    for call in (("flush", 0), ("reset", 0), ("reset", 1)):
        c.accept(*call)
    assert c.counts() == [0, 0]
    obj.close()


def test_a_dictionary_appended_to_is_reported_in_its_place(world):
    """The coverer's own check: behind the NULL checks of push and follow, in front of the offsets and the stream."""
    _appended_to_is_reported_in_its_place(world, "coverer")


def test_a_dictionary_appended_to_is_reported_in_its_place_by_a_mosaicker(world):
    """The mosaicker's own check is the coverer's, at the same place and in the same words."""
    _appended_to_is_reported_in_its_place(world, "mosaicker")
