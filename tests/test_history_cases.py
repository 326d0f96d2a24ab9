"""tests/history_cases.py on the CPU: every compute entry point of include/soundsym_amd.h is run by a probe (a call added
later without one fails here), every probe has a hostile twin of the same size classes under other lengths, and the
tables of tests/test_gpu_history.py name probes that exist."""
import os
import re

import numpy as np
import pytest

import history_cases as hc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "soundsym_amd.h")


def api_functions():
    text = open(HEADER).read()
    return re.findall(r"^SSYM_API\s+[\w\s\*]+?\b(ssym_\w+)\s*\(", text, flags=re.M)


def test_the_header_is_parsed():
    names = api_functions()
    assert len(names) == len(set(names)) > 80
    assert len(names) == len(re.findall(r"^SSYM_API\b", open(HEADER).read(), flags=re.M))
    for known in ("ssym_match_queries", "ssym_last_error", "ssym_spotter_create_step", "ssym_abi_version"):
        assert known in names


def test_every_compute_entry_point_is_run_by_a_probe():
    names = set(api_functions())
    probed = {ep for p in hc.PROBES.values() for ep in p.entry_points}
    assert probed <= names, sorted(probed - names)                     # no probe claims a call the header does not have
    assert hc.LIFECYCLE <= names, sorted(hc.LIFECYCLE - names)
    assert not probed & hc.LIFECYCLE, sorted(probed & hc.LIFECYCLE)
    missing = names - probed - hc.LIFECYCLE
    assert not missing, "no probe of tests/history_cases.py runs %s" % sorted(missing)


def test_the_lifecycle_list_holds_lifecycle_and_accessor_calls_only():
    kinds = re.compile(r"_(create|create_device|create_step|create_local|destroy|size|counts|get|synchronize|last_error|"
                       r"abi_version|get_timings|frames_device|samples_device|num_frames|num_windows)$|^ssym_comm_|"
                       r"^ssym_match_sharded$|^ssym_last_error$|^ssym_abi_version$|^ssym_get_timings$")
    assert all(kinds.search(name) for name in hc.LIFECYCLE), [n for n in hc.LIFECYCLE if not kinds.search(n)]


@pytest.mark.parametrize("name", sorted(hc.PROBES))
def test_every_probe_has_a_hostile_twin_of_its_size_classes(name):
    probe = hc.PROBES[name]
    n, m, dim, total, lengths = probe.shape()
    for fill in hc.FILLS:
        tn, tm, tdim, ttotal, tlengths = probe.shape(hc.twin(fill))
        assert (tn, tm, tdim, ttotal) == (n, m, dim, total)
        if probe.ragged:
            assert tlengths != lengths and sorted(tlengths) == sorted(lengths)
        else:
            assert name == "merge" and lengths == []           # a merge has no segments: its twin differs in its values alone
        D = probe.data(hc.twin(fill))
        assert [f for name_ in probe.sets for f in D.lengths[name_]] == tlengths
        for name_, (kind, _) in probe.sets.items():
            for x, f in zip(D[name_] or [], D.lengths[name_]):
                assert x.shape[0] == f and (kind != "frames" or x.shape[1] == dim)
                if x.size and fill != "same":
                    assert not np.isfinite(x).any() or (fill == "big" and np.all(np.abs(x) >= 3e38))
                elif x.size:
                    assert np.isfinite(x).all() and np.all(x == x[0])
    ln, lm, ldim, ltotal, _ = probe.shape(hc.larger("nan"))
    assert (ln, lm, ltotal) == (3 * n, 3 * m, 9 * total) and ldim in (dim, 3 * dim)


def test_the_plain_data_is_the_same_on_every_draw_and_finite():
    for probe in hc.PROBES.values():
        a, b = probe.data(), probe.data()
        for name in probe.sets:
            for x, y in zip(a[name] or [], b[name] or []):
                assert np.array_equal(x, y) and np.isfinite(x).all()


def test_the_shapes_the_routes_need():
    p = hc.PROBES
    assert p["dtw_search"].shape()[:3] == (33, 65, 13) and min(hc.SRC33) == 0 and max(hc.SRC33) == 64 == max(hc.TGT65)
    assert max(hc.SRC_LONG) == 130 and len(hc.TGT5) == 5
    assert p["dtw_band8"].shape()[:2] == (16, 33) and p["dtw_band8"].ctx["band"] == 8
    assert p["dtw_wide64"].dim == 64 and max(hc.SRC_WIDE) == 40
    assert p["refcos_q8"].shape()[0] * p["refcos_q8"].shape()[1] >= 65536 > p["refcos_tile"].shape()[0] * 5
    assert p["refcos_70x45"].shape()[:3] == (70, 45, 12) and (min(hc.SRC_R70), max(hc.SRC_R70)) == (1, 30)
    assert list(zip(hc.ALIGN_SRC, hc.ALIGN_TGT)) == [(64, 64), (65, 130), (257, 256)]
    assert sorted(hc.WATCH_TGT) == [0, 1, 65] and np.diff(hc.SPOTTER_CUTS).tolist() == [1, 70, 129]
    assert p["mfcc_batch"].sets["snd"][1] == [0, 1023, 5000]
    assert np.diff(list(hc.STREAM_CUTS) + [6000]).tolist() == [1500, 1030, 0, 3470]
    assert (hc.MERGE_SHARDS, hc.MERGE_TARGETS, hc.GMM_K) == (3, 7, 8) and p["partition"].sets["trn"][1] == [300]


def test_the_tables_name_probes_on_one_context():
    for a, b in hc.OTHER_ROUTES:
        assert hc.ctx_key(hc.PROBES[a].ctx) == hc.ctx_key(hc.PROBES[b].ctx), (a, b)
    assert sum(len(ps) for _, ps in hc.by_ctx().values()) == len(hc.PROBES)
    for probe in hc.PROBES.values():
        assert not probe.takes_dict or "src" in probe.sets
