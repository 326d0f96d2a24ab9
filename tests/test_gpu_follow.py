"""ssym_follow_envelope through ctypes against tests/follow_ref.py, bit for bit: out_samples, out_pcm32 and out_gain into
sentinel-filled outputs; host and device inputs in all four combinations, host and device outputs, each output alone and
all three NULL, in place on a device buffer, the sentinels past every output's end; every refusal the header lists with
its code, its message and the outputs unwritten; a refcos context; the call between ssym_match_begin and
ssym_match_finish; Engine.follow_envelope over the same call."""
import numpy as np
import pytest

import follow_gpu as fg
import follow_ref as fr
from soundsym_amd import Engine, synth
from soundsym_amd import _native as nat

pytestmark = pytest.mark.gpu

# a batch that has a target of several blocks' worth of chunk edges, short ones, an empty one and references of other lengths
LENGTHS = (4097, 0, 1, 300, 513, 9000, 256)
REF_LENGTHS = (4097, 5, 0, 310, 400, 9000, 255)
INVALID, UNSUPPORTED = nat.SSYM_E_INVALID, nat.SSYM_E_UNSUPPORTED
NAME = "ssym_follow_envelope: "


@pytest.fixture(scope="module")
def eng():
    e = Engine(metric="dtw", dtype="f64")
    yield e
    e.close()


@pytest.fixture(scope="module")
def case():
    """(samples, out_offsets, ref, ref_offsets) and the restatement's (out, pcm, gain) at max_gain 8, computed once."""
    args = fr.ragged_case(LENGTHS, ref_lengths=REF_LENGTHS)
    args[0][100:1500] *= 1e-3                       # a stretch far too quiet: its gains meet max_gain
    return args, fr.follow(*args, 8.0)


@pytest.mark.parametrize("out_dev", [False, True], ids=["host_out", "device_out"])
@pytest.mark.parametrize("x_dev", [False, True], ids=["host_ref", "device_ref"])
@pytest.mark.parametrize("y_dev", [False, True], ids=["host_samples", "device_samples"])
def test_every_placement_gives_the_restatements_bits(eng, case, y_dev, x_dev, out_dev):
    args, want = case
    res = fg.call(eng, *args, 8.0, y_dev, x_dev, out_dev)
    assert res.out is not None and res.pcm is not None and res.gain is not None
    fg.assert_matches(res, *want)
    assert np.any(want[2] == 8.0) and np.any((want[2] > 0.0) & (want[2] < 8.0))      # the clip is taken and is not all there is


@pytest.mark.parametrize("out_dev", [False, True], ids=["host_out", "device_out"])
@pytest.mark.parametrize("want_outputs", [("out",), ("pcm",), ("gain",), ("out", "gain"), ("pcm", "gain"), ("out", "pcm")])
def test_each_output_alone(eng, case, want_outputs, out_dev):
    args, want = case
    res = fg.call(eng, *args, 8.0, out_dev=out_dev, y_dev=out_dev, want=want_outputs)
    assert [k for k in ("out", "pcm", "gain") if getattr(res, k) is not None] == list(want_outputs)
    fg.assert_matches(res, *want, what=want_outputs)


def test_all_three_outputs_null_and_the_other_no_op_cases(eng, case):
    args, _ = case
    y, off, x, r_off = args
    assert fg.call(eng, *args, 8.0, want=()).rc == nat.SSYM_OK
    res = fg.call(eng, y, off, x, r_off, 8.0, n_targets=0, room=(int(off[-1]), 40))
    assert res.rc == nat.SSYM_OK and res.untouched
    zeros = np.zeros(4, dtype=np.uint64)
    res = fg.call(eng, np.zeros(0), zeros, x, r_off[:4], 8.0, room=(16, 16))              # no samples: nothing to follow
    assert res.rc == nat.SSYM_OK and res.untouched
    res = fg.call(eng, np.zeros(0), zeros, x, r_off[:4], 8.0, null=("samples", "ref"), room=(16, 16))
    assert res.rc == nat.SSYM_OK and res.untouched


def test_in_place_on_a_device_buffer(eng, case):
    args, want = case
    res = fg.call(eng, *args, 8.0, y_dev=True, x_dev=True, out_dev=True, in_place=True)
    fg.assert_matches(res, *want)
    res = fg.call(eng, *args, 8.0, y_dev=True, out_dev=True, in_place=True, want=("out",))
    fg.assert_matches(res, *want)


def test_the_timings_name_the_two_kernels(eng, case):
    args, _ = case
    assert fg.call(eng, *args, 8.0).rc == nat.SSYM_OK
    tm = eng.timings()
    assert tm["main_ms"] > 0 and tm["reduce_ms"] > 0 and tm["total_ms"] >= tm["main_ms"] and tm["main_launches"] == 1
    assert fg.call(eng, *args, 8.0, want=("gain",)).rc == nat.SSYM_OK
    tm = eng.timings()
    assert tm["main_ms"] > 0 and tm["reduce_ms"] == 0


# ---- refusals ----------------------------------------------------------------------------------------------------------

FLAGS = NAME + "unknown flag bits"
GAIN = NAME + "max_gain must be a finite number, 1 or more"
TARGETS = NAME + "2^31 targets or more"
NULL_OFFSETS = NAME + "out_offsets and ref_offsets must not be NULL"
START = NAME + "out_offsets and ref_offsets must start at 0"
DECREASE = NAME + "out_offsets or ref_offsets decrease (target %d)"
LENGTH = NAME + "a target of 2^40 samples or more (target %d)"
BLOCKS = NAME + "more than 2^31 - 1 blocks of 32 boundaries"
NULL_SAMPLES = NAME + "samples and ref must not be NULL while they hold samples"
# 2^40 - 1 samples pass the length check: 2^32 + 1 boundaries, 2^27 + 1 blocks; seventeen such targets pass 2^31 - 1 blocks
LONG = 2 ** 40
MANY_BLOCKS = [k * (LONG - 1) for k in range(18)]

GOOD_OFF, GOOD_ROFF = [0, 700, 700, 1000], [0, 700, 900, 1200]
REFUSALS = [
    (dict(flags=2), INVALID, FLAGS), (dict(flags=4), INVALID, FLAGS), (dict(flags=32), INVALID, FLAGS),
    (dict(flags=256), INVALID, FLAGS), (dict(flags=0x80000000), INVALID, FLAGS), (dict(flags=64 | 16), INVALID, FLAGS),
    (dict(max_gain=float("nan")), INVALID, GAIN), (dict(max_gain=0.999), INVALID, GAIN), (dict(max_gain=0.0), INVALID, GAIN),
    (dict(max_gain=-8.0), INVALID, GAIN), (dict(max_gain=float("inf")), INVALID, GAIN),
    (dict(n_targets=0x80000000), UNSUPPORTED, TARGETS), (dict(n_targets=0xFFFFFFFF), UNSUPPORTED, TARGETS),
    (dict(null=("off",)), INVALID, NULL_OFFSETS), (dict(null=("r_off",)), INVALID, NULL_OFFSETS),
    (dict(off=[1, 700, 700, 1000]), INVALID, START), (dict(r_off=[3, 700, 900, 1200]), INVALID, START),
    (dict(off=[0, 700, 600, 1000]), INVALID, DECREASE % 1), (dict(r_off=[0, 700, 900, 899]), INVALID, DECREASE % 2),
    (dict(off=[0, LONG, LONG, LONG]), UNSUPPORTED, LENGTH % 0), (dict(off=[0, 700, 700, 700 + LONG]), UNSUPPORTED, LENGTH % 2),
    (dict(off=[0, 700, 700, 701 + LONG]), UNSUPPORTED, LENGTH % 2), (dict(off=[0, 2 ** 63, 2 ** 63, 2 ** 64 - 1]), UNSUPPORTED, LENGTH % 0),
    (dict(off=MANY_BLOCKS, r_off=[0] * 18), UNSUPPORTED, BLOCKS),
    (dict(null=("samples",)), INVALID, NULL_SAMPLES), (dict(null=("ref",)), INVALID, NULL_SAMPLES),
    # of two faults the first in the header's order wins
    (dict(flags=2, max_gain=0.5), INVALID, FLAGS), (dict(max_gain=0.5, n_targets=0x80000000), INVALID, GAIN),
    (dict(n_targets=0x80000000, null=("off",)), UNSUPPORTED, TARGETS), (dict(null=("off",), r_off=[1, 2, 3, 4]), INVALID, NULL_OFFSETS),
    (dict(off=[1, 700, 600, 1000]), INVALID, START), (dict(off=[0, 700, 600, 1000], null=("samples",)), INVALID, DECREASE % 1),
    # target by target, its decrease before its length; then the blocks; then the NULL samples
    (dict(off=[0, LONG, LONG, LONG], r_off=[0, 700, 600, 1200]), UNSUPPORTED, LENGTH % 0),
    (dict(off=[0, 700, 700 + LONG, 700 + LONG], r_off=[0, 700, 600, 1200]), INVALID, DECREASE % 1),
    (dict(off=[0, 700, 600, 600 + LONG]), INVALID, DECREASE % 1),
    (dict(off=MANY_BLOCKS + [MANY_BLOCKS[-1] + LONG], r_off=[0] * 19), UNSUPPORTED, LENGTH % 17),
    (dict(off=MANY_BLOCKS[:-1] + [MANY_BLOCKS[-2] - 1], r_off=[0] * 18), INVALID, DECREASE % 16),
    (dict(off=[0, LONG, LONG, LONG], null=("samples",)), UNSUPPORTED, LENGTH % 0),
    (dict(off=MANY_BLOCKS, r_off=[0] * 18, null=("samples", "ref")), UNSUPPORTED, BLOCKS),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_every_refusal_its_code_its_message_the_outputs_unwritten(eng, device):
    rng = np.random.default_rng(0xF0110)
    y, x = rng.standard_normal(1000), rng.standard_normal(1200)
    for change, code, message in REFUSALS:
        a = dict(off=GOOD_OFF, r_off=GOOD_ROFF, max_gain=8.0, flags=None, null=(), n_targets=None)
        a.update(change)
        res = fg.call(eng, y, a["off"], x, a["r_off"], a["max_gain"], device, device, device, flags=a["flags"], null=a["null"],
                      n_targets=a["n_targets"], room=(1000, 8))
        assert (res.rc, res.message) == (code, message), (change, res.rc, res.message)
        assert res.untouched, change
    res = fg.call(eng, y, GOOD_OFF, x, GOOD_ROFF, 8.0, device, device, device, null=("ctx",), room=(1000, 8))
    assert res.rc == INVALID and res.untouched
    good = fg.call(eng, y, GOOD_OFF, x, GOOD_ROFF, 8.0, device, device, device)           # what every case above changes
    fg.assert_matches(good, *fr.follow(y, GOOD_OFF, x, GOOD_ROFF, 8.0))
    assert not good.untouched


def test_a_reference_of_no_samples_may_be_null(eng):
    y = fr.sounding(700)
    res = fg.call(eng, y, [0, 700], np.zeros(0), [0, 0], 8.0, null=("ref",))
    fg.assert_matches(res, *fr.follow(y, [0, 700], np.zeros(0), [0, 0], 8.0))
    assert np.all(res.gain == 0.0) and np.all(res.out == 0.0)


# ---- beside the other calls of a context -------------------------------------------------------------------------------

def test_a_refcos_context(case):
    args, want = case
    e = Engine(metric="refcos", dtype="f64")
    try:
        fg.assert_matches(fg.call(e, *args, 8.0), *want)
        fg.assert_matches(fg.call(e, *args, 8.0, True, True, True), *want)
        out, pcm, gains = e.follow_envelope(*args, 8.0, want_pcm32=True, want_gains=True)
        assert fg.same_bits(out, want[0]) and np.array_equal(pcm, want[1]) and fg.same_bits(gains, want[2])
    finally:
        e.close()


def test_between_begin_and_finish(case):
    torch = pytest.importorskip("torch")
    args, want = case
    g = synth.make_grid(256, 96, 32, 13, 0x5EED0A00)
    m = 96
    e = Engine(metric="dtw", dtype="f32")
    try:
        so, to = np.arange(257, dtype=np.uint64) * 32, np.arange(m + 1, dtype=np.uint64) * 32
        d, q = e.dictionary(g.sources.reshape(-1), so, 13), e.queries(g.targets.reshape(-1), to, 13)
        want_idx, want_cost = e.match(d, q, index_base=3)
        bounds = torch.empty(m, dtype=torch.float64, device="cuda")
        oi = torch.empty(m, dtype=torch.int32, device="cuda")
        oc = torch.empty(m, dtype=torch.float64, device="cuda")
        first = fg.call(e, *args, 8.0)
        e.match_begin(d, q, bounds, index_base=3)
        between = fg.call(e, *args, 8.0)
        e.match_finish(bounds, oi, oc)
        assert np.array_equal(oi.cpu().numpy().astype(np.int64), want_idx.astype(np.int64))
        assert np.array_equal(fg.bits(oc.cpu().numpy()), fg.bits(want_cost))
        after = fg.call(e, *args, 8.0)
        for res in (first, between, after):
            fg.assert_matches(res, *want)
    finally:
        e.close()


# ---- Engine.follow_envelope ----------------------------------------------------------------------------------------------

def test_the_engine_method_host_and_device(eng, case):
    torch = pytest.importorskip("torch")
    (y, off, x, r_off), want = case
    out = eng.follow_envelope(y, off, x, r_off)
    assert isinstance(out, np.ndarray) and fg.same_bits(out, want[0])
    out, pcm = eng.follow_envelope(y, off, x, r_off, 8.0, want_pcm32=True)
    assert fg.same_bits(out, want[0]) and pcm.dtype == np.int32 and np.array_equal(pcm, want[1])
    out, gains = eng.follow_envelope(torch.from_numpy(y).cuda(), off, x, r_off, want_gains=True)
    assert fg.same_bits(out, want[0]) and fg.same_bits(gains, want[2])
    d_out, d_pcm, d_gains = eng.follow_envelope(torch.from_numpy(y).cuda(), off, torch.from_numpy(x).cuda(), r_off, 8.0, True, True,
                                                on_device=True)
    assert d_out.is_cuda and d_pcm.is_cuda and d_gains.is_cuda
    assert fg.same_bits(d_out.cpu().numpy(), want[0]) and np.array_equal(d_pcm.cpu().numpy(), want[1])
    assert fg.same_bits(d_gains.cpu().numpy(), want[2])
    out2 = eng.follow_envelope(y, off, x, r_off, 2.0)
    assert fg.same_bits(out2, fr.follow(y, off, x, r_off, 2.0)[0]) and not fg.same_bits(out2, want[0])
    empty = eng.follow_envelope(np.zeros(0), [0], np.zeros(0), [0], want_gains=True)
    assert empty[0].size == 0 and empty[1].size == 0
