"""What the four resynthesis entry points -- ssym_reconstruct_warped, ssym_reconstruct_wsola and their _spans forms -- say
when they refuse a call, and which refusal wins when a call has two faults: the messages word for word, the order of the
checks pair by neighbouring pair, host and device maps and outputs, the outputs untouched.  Every faulty call here is refused
on the host, before any device work; the one call per entry point that is accepted is the arguments all of them start from.

The order: (_spans) NULL windows; NULL pointers; (WSOLA) the search width; out_offsets[0]; the flags; an empty store; per
target t its out_offsets / index, then its map room; a NULL map; (_spans) the windows against their sounds.  The one refusal
not reached is "more than 2^31 - 1 windows in one call": it takes arrays of that many targets."""
import numpy as np
import pytest

from soundsym_amd import Engine
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu

ENTRIES = ("ssym_reconstruct_warped", "ssym_reconstruct_warped_spans", "ssym_reconstruct_wsola", "ssym_reconstruct_wsola_spans")
SOUNDS = (3000, 0, 900)
SENTF, SENT32, SENTP = -12345.5, -559038737, np.uint64(0xDEADBEEFCAFEF00D)
TOTAL, SLOTS = 3000, 20
GOOD = dict(idx=[0, 2, 1], off=[0, 2000, 2600, 3000], maps=np.arange(20, dtype=np.uint32) % 5, m_off=[0, 8, 12, 20],
            frames=[8, 3, 0], plen=[9, 0, 4], search=32, win_first=[0, 100, 0], win_len=[3000, 800, 0], flags=None, null=())
INVALID, EMPTY = nat.SSYM_E_INVALID, nat.SSYM_E_EMPTY_DICT

NULL_WINDOWS = "%s: win_first and win_len must not be NULL"
NULL_POINTERS = "%s: s, idx, out_offsets, map_offsets and map_frames must not be NULL"
SEARCH = "%s: search must not exceed 512 samples"
START = "%s: out_offsets must start at 0"
FLAGS = "%s: unknown flag bits"
EMPTY_STORE = "empty dictionary"
OFFSETS = "%s: out_offsets decrease or an index is outside the sample store (target %d)"
MAP_ROOM = "%s: map_offsets decrease or leave less room than map_frames (target %d)"
NULL_MAP = "%s: frame_map is NULL although a target has map frames"
WINDOW = "%s: window %d reaches beyond its sound's samples"


@pytest.fixture(scope="module")
def eng():
    e = Engine(metric="dtw", dtype="f64")
    yield e
    e.close()


@pytest.fixture(scope="module")
def stores(eng):
    """(the three sounds, a store without a sound)."""
    rng = np.random.default_rng(0xE46)
    off = np.concatenate([[0], np.cumsum(SOUNDS)]).astype(np.uint64)
    return eng.samples(rng.uniform(-1, 1, size=int(off[-1])), off), eng.samples(np.zeros(0), np.zeros(1, dtype=np.uint64))


def _call(e, store, name, device, **change):
    """One call of entry point `name` into sentinel-filled outputs: (code, message, outputs untouched)."""
    import torch
    a = dict(GOOD)
    a.update(change)
    u32 = lambda key: np.ascontiguousarray(a[key], dtype=np.uint32)
    u64 = lambda key: np.ascontiguousarray(a[key], dtype=np.uint64)
    idx, frames, maps, plen = u32("idx"), u32("frames"), u32("maps"), u32("plen")
    off, m_off, wf, wl = u64("off"), u64("m_off"), u64("win_first"), u64("win_len")
    out, pcm, pos = np.full(TOTAL, SENTF), np.full(TOTAL, SENT32, dtype=np.int32), np.full(SLOTS, SENTP, dtype=np.uint64)
    fl = 0
    if device:
        fl = nat.WARP_MAP_DEVICE | nat.OUT_DEVICE
        dmaps, dlen = torch.from_numpy(maps.view(np.int32)).cuda(), torch.from_numpy(plen.view(np.int32)).cuda()
        dout, dpcm, dpos = torch.from_numpy(out).cuda(), torch.from_numpy(pcm).cuda(), torch.from_numpy(pos.view(np.int64)).cuda()
        torch.cuda.synchronize()
        map_p, len_p, out_p, pcm_p, pos_p = dmaps.data_ptr(), dlen.data_ptr(), dout.data_ptr(), dpcm.data_ptr(), dpos.data_ptr()
    else:
        map_p, len_p, out_p, pcm_p, pos_p = maps.ctypes.data, plen.ctypes.data, out.ctypes.data, pcm.ctypes.data, pos.ctypes.data
    p = lambda key, ptr: None if key in a["null"] else ptr
    wsola = "wsola" in name
    args = [e.ctx, p("s", store.ptr), p("idx", idx.ctypes.data)]
    if name.endswith("_spans"):
        args += [p("win_first", wf.ctypes.data), p("win_len", wl.ctypes.data)]
    args += [p("off", off.ctypes.data), idx.size, p("map", map_p), p("moff", m_off.ctypes.data), p("frames", frames.ctypes.data),
             len_p]
    args += ([a["search"]] if wsola else []) + [fl if a["flags"] is None else a["flags"]] + ([pos_p] if wsola else [])
    rc = getattr(nat.lib(), name)(*args, out_p, pcm_p)
    message = (nat.lib().ssym_last_error(e.ctx) or b"").decode()
    if device:
        torch.cuda.synchronize()
        out, pcm, pos = dout.cpu().numpy(), dpcm.cpu().numpy(), dpos.cpu().numpy().view(np.uint64)
    return rc, message, bool((out == SENTF).all() and (pcm == SENT32).all() and (pos == SENTP).all())


def _cases(name):
    """(the arguments changed, the code, the message) of every refusal alone, then of every neighbouring pair of the order,
    the first fault's message expected."""
    spans, wsola = name.endswith("_spans"), "wsola" in name
    alone, pairs = [], []
    if spans:
        alone += [(dict(null=(key,)), INVALID, NULL_WINDOWS % name) for key in ("win_first", "win_len")]
        alone += [(dict(null=("win_first", "win_len")), INVALID, NULL_WINDOWS % name)]
        pairs += [(dict(null=("win_len", "idx")), INVALID, NULL_WINDOWS % name)]
    alone += [(dict(null=(key,)), INVALID, NULL_POINTERS % name) for key in ("s", "idx", "off", "moff", "frames")]
    if wsola:
        alone += [(dict(search=s), INVALID, SEARCH % name) for s in (513, 0xFFFFFFFF)]
        pairs += [(dict(null=("frames",), search=513), INVALID, NULL_POINTERS % name),
                  (dict(search=513, off=[1, 2000, 2600, 3000]), INVALID, SEARCH % name)]
    else:
        pairs += [(dict(null=("idx",), off=[1, 2000, 2600, 3000]), INVALID, NULL_POINTERS % name)]
    alone += [(dict(off=[1, 2000, 2600, 3000]), INVALID, START % name)]
    pairs += [(dict(off=[1, 2000, 2600, 3000], flags=4), INVALID, START % name)]
    alone += [(dict(flags=f), INVALID, FLAGS % name) for f in (2, 4, 8, 64, 0x80000000, nat.WARP_MAP_DEVICE | 16)]
    pairs += [(dict(flags=64, empty=True), INVALID, FLAGS % name)]
    alone += [(dict(empty=True), EMPTY, EMPTY_STORE)]
    pairs += [(dict(empty=True, off=[0, 2600, 2000, 3000]), EMPTY, EMPTY_STORE)]
    alone += [(dict(off=[0, 2600, 2000, 3000]), INVALID, OFFSETS % (name, 1)),
              (dict(idx=[0, 2, 3]), INVALID, OFFSETS % (name, 2)),
              (dict(idx=[nat.NO_MATCH, 2, 1]), INVALID, OFFSETS % (name, 0)),
              (dict(m_off=[0, 12, 8, 20]), INVALID, MAP_ROOM % (name, 1)),
              (dict(m_off=[0, 7, 12, 20]), INVALID, MAP_ROOM % (name, 0))]                # room for 7 frames, 8 asked
    pairs += [(dict(idx=[0, 3, 1], m_off=[0, 8, 10, 20]), INVALID, OFFSETS % (name, 1)),   # target 1: its index before its room
              (dict(idx=[0, 3, 1], m_off=[0, 7, 12, 20]), INVALID, MAP_ROOM % (name, 0)),  # target 0's room before target 1's index
              (dict(off=[0, 2000, 2600, 2500], m_off=[0, 8, 10, 20]), INVALID, MAP_ROOM % (name, 1)),
              (dict(m_off=[0, 8, 12, 11], null=("map",)), INVALID, MAP_ROOM % (name, 2))]  # the last target's room before the map
    alone += [(dict(null=("map",)), INVALID, NULL_MAP % name)]
    if spans:
        alone += [(dict(win_len=[3001, 800, 0]), INVALID, WINDOW % (name, 0)),
                  (dict(win_first=[0, 100, 1]), INVALID, WINDOW % (name, 2)),             # sound 1 has no samples
                  (dict(win_first=[0, 2 ** 64 - 1, 0], win_len=[3000, 2, 0]), INVALID, WINDOW % (name, 1))]
        pairs += [(dict(null=("map",), win_len=[3000, 801, 0]), INVALID, NULL_MAP % name)]
    return alone, pairs


def _assert_refused(eng, stores, name, device, cases):
    for change, code, message in cases:
        change = dict(change)
        store = stores[1] if change.pop("empty", False) else stores[0]
        rc, said, untouched = _call(eng, store, name, device, **change)
        assert (rc, said) == (code, message), (change, rc, said)
        assert untouched, change
        assert message == EMPTY_STORE or message.startswith(name + ": ")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ENTRIES)
def test_every_refusal_alone_says_what_it_said(eng, stores, name, device):
    alone, _ = _cases(name)
    assert len(alone) == 19 + (6 if name.endswith("_spans") else 0) + (2 if "wsola" in name else 0)
    _assert_refused(eng, stores, name, device, alone)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ENTRIES)
def test_of_two_faults_the_first_in_the_order_wins(eng, stores, name, device):
    _, pairs = _cases(name)
    assert len(pairs) == 8 + (2 if name.endswith("_spans") else 0) + (1 if "wsola" in name else 0)
    _assert_refused(eng, stores, name, device, pairs)


@pytest.mark.parametrize("name", ENTRIES)
def test_the_unchanged_call_is_accepted(eng, stores, name):
    """The arguments every case above changes are themselves in order: the call succeeds and writes every sample."""
    rc, _, untouched = _call(eng, stores[0], name, False)
    assert rc == nat.SSYM_OK and not untouched
