"""soundsym_amd/csrc/follower_plan.hpp against its restatement in tests/live_follow_ref.py (CPU only).

The plan is the one place that decides what a call of the live envelope follower consumes, settles and releases; follower.hip
runs it.  This file builds tests/cpp/follower_plan_dump.cpp -- a host program over the plan's header alone -- and holds every
call it prints against the restatement, field by field: calls worked out by hand (the block edges the GPU tests settle in
one call among them), seeded random sequences of pushes, flushes and resets over 1 ... 70 lanes, and single calls at the
ring's and the length's limits.
The restatement's counts are in turn what tests/test_live_follow_ref.py holds against the offline render."""
import json
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import live_follow_ref as lf
from follow_ref import HOP

HERE = os.path.dirname(os.path.abspath(__file__))


def _sequence(rng, n_lanes, calls, top):
    """A run of calls against the restatement's arithmetic: (state before, my, mx, flush lane) per call; resets in between."""
    lanes = [(0, 0, 0, 0)] * n_lanes
    out = []
    for _ in range(calls):
        kind = rng.random()
        live = [l for l, s in enumerate(lanes) if not s[3]]
        if kind < 0.12 and live:
            l = int(rng.choice(live))
            call = (list(lanes), None, None, l)
        elif kind < 0.2:
            l = int(rng.integers(0, n_lanes))
            lanes = lanes[:l] + [(0, 0, 0, 0)] + lanes[l + 1:]
            continue
        else:
            feed = lambda s: 0 if s[3] or rng.random() < 0.3 else int(rng.integers(0, top + 1))      # noqa: E731
            call = (list(lanes), [feed(s) for s in lanes], [feed(s) for s in lanes], lf.NO_LANE)
        out.append(call)
        lanes = lf.plan(*call)["after"]
    return out


def _hand_calls():
    z = (0, 0, 0, 0)
    return {
        "first_hops": ([z], [511], [511], lf.NO_LANE),
        "two_hops": ([z], [512], [600], lf.NO_LANE),
        "three_hops": ([(512, 600, 0, 0)], [256], [168], lf.NO_LANE),
        "x_behind": ([(10000, 0, 0, 0)], [0], [10000], lf.NO_LANE),
        "flush_mid": ([(5220, 5220, 18 * HOP, 0)], None, None, 0),
        "flush_empty": ([z, (300, 0, 0, 0)], None, None, 0),
        "flush_short_x": ([z, (300, 0, 0, 0)], None, None, 1),
        "ended_idle": ([(300, 0, 300, 1), (600, 900, 0, 0)], [0, 700], [0, 0], lf.NO_LANE),
        "blocks": ([z] * 7, [(c + 1) * HOP if c else 0 for c in (0, 1, 31, 32, 33, 64, 65)],
                   [(c + 1) * HOP + 5 if c else 0 for c in (0, 1, 31, 32, 33, 64, 65)], lf.NO_LANE),
        "ring_full_16384": ([(5 * HOP, 5 * HOP, 3 * HOP, 0)] * 3, [768 + HOP] * 3, [0] * 3, lf.NO_LANE),
        "ring_limit_1_lane": ([z], [1 << 25], [0], lf.NO_LANE),
        "ring_beyond_1_lane": ([z], [(1 << 25) + 1], [0], lf.NO_LANE),
        "long_lane": ([((1 << 40) - 1000, (1 << 40) - 1000, ((1 << 40) - 1000) // HOP * HOP - 2 * HOP, 0)], [999], [999], lf.NO_LANE),
    }


def _all_calls():
    rng = np.random.default_rng(0xF0110E)
    calls = dict(_hand_calls())
    for k in range(60):
        n_lanes = int(rng.choice([1, 2, 3, 5, 70]))
        top = int(rng.choice([1, 255, 256, 257, 700, 3000, 20000]))
        for i, call in enumerate(_sequence(rng, n_lanes, 25, top)):
            calls["random_%02d_%02d" % (k, i)] = call
    return calls


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("follower_plan")
    make = ["make", "-s", "-C", os.path.join(HERE, "cpp"), "-f", "follower_plan.mk"]
    exe = str(tmp / "follower_plan_dump")
    subprocess.run(make + ["OUT=" + exe], check=True, timeout=300)
    calls = _all_calls()
    cases = str(tmp / "cases.txt")
    with open(cases, "w") as f:
        for name, (lanes, my, mx, flush) in calls.items():
            my, mx = my or [0] * len(lanes), mx or [0] * len(lanes)
            f.write("call %s %d %d %s\n" % (name, len(lanes), -1 if flush == lf.NO_LANE else flush,
                                            " ".join("%d %d %d %d %d %d" % (*s, a, b) for s, a, b in zip(lanes, my, mx))))
    stdout = subprocess.run([exe, cases], check=True, capture_output=True, text=True, timeout=300).stdout
    lines = stdout.splitlines()
    return SimpleNamespace(consts=json.loads(lines[0]), got={r["id"]: r for r in map(json.loads, lines[1:])}, calls=calls,
                           exe=exe, cases=cases, make=make, stdout=stdout)


def test_the_plan_has_the_constants_the_restatement_names(planner):
    assert planner.consts == dict(kFollowerHop=HOP, kFollowerBlock=lf.BLOCK, kFollowerRingMin=lf.RING_MIN,
                                  kFollowerRingBytes=lf.RING_BYTES, kFollowerMaxLanes=lf.MAX_LANES, kFollowerMaxLen=lf.MAX_LEN,
                                  kFollowerNoLane=lf.NO_LANE)


def test_the_plan_plans_what_the_restatement_does(planner):
    assert len(planner.got) == len(planner.calls) > 1000
    flushes = grown = 0
    for name, call in planner.calls.items():
        want, got = lf.plan(*call), planner.got[name]
        assert got["steps"] == want["steps"], name
        assert [tuple(e) for e in got["table"]] == want["table"], name
        assert [tuple(a) for a in got["after"]] == want["after"], name
        for key in ("samples", "gains", "maxAppend", "maxReleased", "maxBlock", "ringCap", "fits"):
            assert got[key] == want[key], (name, key)
        flushes += call[3] != lf.NO_LANE
        grown += want["ringCap"] > lf.RING_MIN
    assert flushes > 50 and grown > 100


def test_plan_by_hand(planner):
    got = planner.got
    s, = got["first_hops"]["steps"]                     # 511 samples of both: one hop, nothing settled
    assert (s["setCount"], s["relCount"], got["first_hops"]["table"]) == (0, 0, [])
    s, = got["two_hops"]["steps"]                       # min(512, 600): h = 2, boundary 0 settled, no hop released
    assert (s["setFirst"], s["setCount"], s["relCount"], got["two_hops"]["table"]) == (0, 1, 0, [[0, 0, 1]])
    s, = got["three_hops"]["steps"]                     # 768 of both: h = 3, boundary 1 settled, hop 0 released
    assert (s["setFirst"], s["setCount"], s["relFirst"], s["relCount"]) == (1, 1, 0, HOP)
    assert got["three_hops"]["after"] == [[768, 768, HOP, 0]]
    s, = got["x_behind"]["steps"]                       # x arrives 10 000 at once: h = 39
    assert (s["setCount"], s["relCount"], got["x_behind"]["ringCap"]) == (38, 37 * HOP, 16384)
    assert got["x_behind"]["table"] == [[0, 0, 32], [0, 32, 6]]
    s, = got["flush_mid"]["steps"]                      # 20 hops + 100: h = 20, settled 19, released 18 hops; J = 21
    assert (s["setFirst"], s["setCount"], s["relFirst"], s["relCount"]) == (19, 3, 18 * HOP, 5220 - 18 * HOP)
    assert got["flush_mid"]["after"] == [[5220, 5220, 5220, 1]]
    assert got["flush_empty"]["samples"] == got["flush_empty"]["gains"] == 0 and got["flush_empty"]["after"][0] == [0, 0, 0, 1]
    s = got["flush_short_x"]["steps"][1]                # 300 samples of y alone: boundaries 0, 1, 2
    assert (s["setFirst"], s["setCount"], s["relCount"], s["outAt"], s["gainAt"]) == (0, 3, 300, 0, 0)
    a, b = got["ended_idle"]["steps"]
    assert (a["setCount"], a["relCount"], b["yAt"], b["ny"], b["setCount"], b["outAt"]) == (0, 0, 0, 1300, 1, 0)
    # one call settling 0, 1, 31, 32, 33, 64 and 65 boundaries on different lanes
    assert [s["setCount"] for s in got["blocks"]["steps"]] == [0, 1, 31, 32, 33, 64, 65]
    assert [(e[0], e[2]) for e in got["blocks"]["table"]] == [(1, 1), (2, 31), (3, 32), (4, 32), (4, 1), (5, 32), (5, 32), (6, 32),
                                                             (6, 32), (6, 1)]
    assert got["blocks"]["maxBlock"] == 32 and got["blocks"]["gains"] == 226
    # a lane that has released 3 hops holds from hop 1: 256 ... 1280 + 1024 is exactly 2048
    assert got["ring_full_16384"]["ringCap"] == 2048
    assert (got["ring_limit_1_lane"]["ringCap"], got["ring_limit_1_lane"]["fits"]) == (1 << 25, True)
    assert (got["ring_beyond_1_lane"]["ringCap"], got["ring_beyond_1_lane"]["fits"]) == (1 << 26, False)
    s, = got["long_lane"]["steps"]
    assert s["ny"] == (1 << 40) - 1 and s["setFirst"] + s["setCount"] == ((1 << 40) - 1) // HOP - 1 < 1 << 32


def test_the_plan_is_clean_under_the_sanitizers(planner, tmp_path):
    """The dump program once more with -fsanitize=address,undefined, as the stand-alone program it is, over the same cases:
    the same output, nothing reported."""
    exe = str(tmp_path / "follower_plan_dump_san")
    subprocess.run(planner.make + ["OUT=" + exe, "EXTRA=-fsanitize=address,undefined -fno-sanitize-recover=all"], check=True,
                   timeout=300)
    r = subprocess.run([exe, planner.cases], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    assert r.stdout == planner.stdout
