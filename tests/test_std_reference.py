"""CPU checks of the loop search's specification (tests/std_cases.py): the scalar restatement of
candidate_selector against the all-pairs cross-check, the recovered transform against the generator's
ground truth, what each edge case is built to show, and the measured solver deviation behind the
device tolerance."""
import numpy as np
import pytest

import std_cases as S

NAMES = list(S.cases())


@pytest.mark.parametrize("name", NAMES)
def test_selector_equals_the_all_pairs_cross_check(name):
    c = S.cases()[name]
    db = c.db()
    got = S.selector(db, c.query, {**c.prm, "candidate_num": 64})
    cross = S.selector_cross(db, c.query, c.prm)
    want = sorted(((len(v), -f) for f, v in cross.items() if len(v) >= 5), reverse=True)
    assert [(len(m), -f) for f, m in got] == want[:64]
    for f, m in got:
        assert m == cross[f], (name, f)


def test_revisit_recovers_the_ground_truth():
    c = S.cases()["revisit"]
    e = c.expected()
    R, t = c.truth
    assert e["frame"] == 10 and e["score"] > 0.9 and len(e["pairs"]) == S.N_TRI
    assert np.abs(e["rot"] - R).max() < 0.05  # 1 cm of vertex noise over sides >= 2 m
    far = max(np.linalg.norm(d["center"]) for d in c.query)
    assert np.linalg.norm(e["t"] - t) < 0.05 * far + 0.05
    assert S.cases()["no_revisit"].expected()["frame"] == -1


def _cands(name):
    return [(k["frame"], k["votes"]) for k in S.cases()[name].expected()["candidates"]]


def test_edge_cases_show_what_they_are_built_for():
    assert _cands("runs_65_130") == [(0, 10), (1, 10), (2, 10)]          # ties: the lower frame; 39 frames qualify
    assert len(S.selector_cross(S.cases()["runs_65_130"].db(), S.cases()["runs_65_130"].query,
                                S.cases()["runs_65_130"].prm)) == 39
    assert _cands("skip_len") == [(4, 100), (3, 99), (2, 51), (1, 50), (0, 49)]
    assert [k["use_size"] for k in S.cases()["skip_len"].expected()["candidates"]] == [33, 49, 25, 25, 49]
    assert _cands("votes_4_5") == [(1, 5)]
    assert _cands("gap_5_6") == [(14, 5)]                                 # 20 - 15 = 5 is not > 5
    assert _cands("gap_wraps") == [(10, 5)]                               # 3 - 10 wraps
    assert _cands("frac_49_51") == [(0, 5), (1, 5)]
    assert _cands("trunc_twice") == [(0, 6)]                              # 3 entries, cell 0 visited twice
    assert _cands("centre_exact") == [] and _cands("centre_inside") == [(0, 5)]
    e3, e4 = S.cases()["max_vote_3"].expected(), S.cases()["max_vote_4"].expected()
    assert e3["candidates"][0]["max_vote"] == 3 and e3["candidates"][0]["score"] == -1.0 and e3["frame"] == -1
    assert e4["candidates"][0]["max_vote"] == 4 and e4["frame"] == 0 and len(e4["pairs"]) == 4
    assert S.cases()["normal_flipped"].expected()["score"] == 1.0
    e2, e3 = S.cases()["score_2_of_4"].expected(), S.cases()["score_3_of_4"].expected()
    assert e2["candidates"][0]["score"] == 0.5 and e2["frame"] == -1      # 0.5 > 0.5 is false
    assert e3["score"] == 0.75 and e3["frame"] == 0
    assert S.cases()["target_2_planes"].expected()["candidates"][0]["score"] >= 0.0
    assert np.isnan(S.cases()["empty_source_cloud"].expected()["candidates"][0]["score"])
    assert S.cases()["empty_source_cloud"].expected()["frame"] == -1
    assert S.cases()["empty_descs"].expected()["candidates"] == []


def test_generated_cases_keep_their_margins():
    for name in ("revisit", "no_revisit"):
        c = S.cases()[name]
        c.expected()
        assert c.generated and min(m[1] for m in c.margins) >= S.MARGIN


def test_the_tolerance_constants_are_the_measured_deviation():
    pytest.importorskip("mpmath")
    dev_r, dev_t = S.measure_solver_deviation()
    # (numpy's BLAS picks its kernels by CPU, which moves the last bits: twice the recorded value at most here;
    # the device tolerance is fixed at 8 x the recorded one either way)
    assert dev_r <= 2 * S.ROT_DEV and dev_t <= 2 * S.T_DEV
    assert S.ROT_TOL == 8 * S.ROT_DEV and S.T_TOL == 8 * S.T_DEV
