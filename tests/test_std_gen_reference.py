"""The restatement of GenerateSTDescs (tests/std_gen_cases.py) on the CPU: the edge cases show what they are built
for, the margins hold, what the issue calls order-free is unchanged under random visiting orders, the per-voxel greedy
membership equals corner_extractor's sequential walk, and the room's loop is found."""
import math

import numpy as np
import pytest

import std_gen_cases as G

NAMES = list(G.cases())


def _exp(name):
    return G.cases()[name].expected()


@pytest.mark.parametrize("name", NAMES)
def test_margins_hold(name):
    e = _exp(name)  # (expected() asserts them)
    assert all(m >= G.MARGIN for m in e["worst_margins"].values())


def test_voxel_keys():
    assert G.voxel_key((-2.0, 0.5, 0.5), 2.0) == (-2, 0, 0)     # an exact negative multiple: -1 - 1
    assert G.voxel_key((-0.0, -0.0, 0.5), 2.0) == (0, 0, 0)     # -0.0 is not < 0
    assert G.voxel_key((-0.5, -3.9, -4.0), 2.0) == (-1, -2, -3)
    assert G.voxel_key((np.float32(1.9999999), np.float32(-1e-7), 7.0), 2.0) == (0, -1, 3)
    e = _exp("keys")
    by_count = {int(c): int(p) for _, c, p in e["voxels"]}
    assert by_count[10] == 0 and by_count[11] == 1                # voxel_init_num is exclusive


def test_planes_case():
    e = _exp("planes")
    vox = e["vox"]
    thin, thick = vox[(0, 0, 0)], vox[(3, 0, 0)]
    assert thin.is_plane and 0.005 < thin.min_eig < 0.01 and not thick.is_plane and 0.01 < thick.min_eig < 0.02
    down = vox[(6, 0, 0)]
    assert down.is_plane and down.normal[2] > 0.9                 # given as (0.2, -0.1, -1): the pin turns it
    assert G.pin_sign((0.2, -0.1, -0.9)) == (-0.2, 0.1, 0.9) and G.pin_sign((0.5, -0.5, 0.1)) == (0.5, -0.5, 0.1)
    assert G.pin_sign((-0.5, 0.5, 0.1)) == (0.5, -0.5, -0.1)      # equal magnitudes: the first decides
    assert vox[(0, 4, 0)].normal == (1.0, 0.0, 0.0) and vox[(4, 0, 3)].normal == (0.0, 1.0, 0.0)
    assert sorted(j["branch"] for j in e["jobs"]) == [1, 2] and all(j["projected"] > 5 for j in e["jobs"])
    assert any(j["branch"] == 0 for j in _exp("room")["jobs"])


def test_connect_case():
    e = _exp("connect")
    vox = e["vox"]
    a = vox[(0, 0, 0)]
    assert a.connect[0] and vox[(1, 0, 0)].connect[3]             # 0.095 apart: merged, both sides
    assert not a.connect[1] and a.checked[1] and not vox[(0, 1, 0)].connect[4]  # 0.105 apart
    assert a.checked[3] and not a.connect[3]                      # a missing neighbour
    up = vox[(0, 0, 1)]
    assert not a.connect[2] and up.connect[5] and up.tree[5] is a  # a non-plane neighbour is written by the plane
    assert G.same_normal((0.0, 0.6, 0.8), (-0.0, -0.6, -0.8), 0.1)  # antipodal normals are the same plane
    lone = vox[(5, 0, 0)]
    assert lone.is_plane and not any(lone.connect) and vox[(5, 0, 1)].connect[5]
    assert [(j["v"], j["c"]) for j in e["jobs"]] == [(3, 0)]      # through (0,0,0) only: the lone plane gives no job


def test_job_cases():
    e = _exp("v_10_11")
    assert e["stats"]["jobs"] == 1 and e["voxels"][e["jobs"][0]["v"]][1] == 11
    once, twice = _exp("w_once"), _exp("w_twice")
    w = 1  # W is the first voxel: rank 0, stored as rank + 1
    assert [w in j["members"] for j in once["jobs"]] == [True, False]
    assert [w in j["members"] for j in twice["jobs"]] == [True, True]


def test_chain_depends_on_the_visiting_order():
    case = G.cases()["chain"]
    e = case.expected()
    assert [1 in j["members"] for j in e["jobs"]] == [True, False, False]
    back = G.generate(case.pts, case.prm, order=list(reversed(e["order"])))
    w = back["order"].index((0, 0, 0)) + 1
    got = {back["order"][j["v"]]: w in j["members"] for j in back["jobs"]}
    assert got == {(0, 0, -1): True, (0, -1, 0): True, (-1, 0, 0): False}
    n = G.CHAIN_NORMALS
    assert G.same_normal(n[0], n[1], 0.5) and G.same_normal(n[0], n[2], 0.5) and not G.same_normal(n[1], n[2], 0.5)


@pytest.mark.parametrize("name", NAMES)
def test_order_free_parts_and_greedy_membership(name):
    case = G.cases()[name]
    rng = np.random.default_rng(5)
    pts = np.asarray(case.pts, np.float32).reshape(-1, 3)
    vox0 = G.init_voxel_map(pts, case.prm)
    G.build_connection(vox0, list(vox0), case.prm)
    state0 = G.connection_state(vox0)
    assert G.members_greedy(vox0, list(vox0)) == G.members_sequential(vox0, list(vox0))
    for _ in range(3):
        order = [list(vox0)[i] for i in rng.permutation(len(vox0))]
        vox = G.init_voxel_map(pts, case.prm)
        G.build_connection(vox, order, case.prm)
        assert G.connection_state(vox) == state0
        assert G.members_greedy(vox, order) == G.members_sequential(vox, order)


def test_suppression_is_order_free_and_its_edges():
    prm = G.DEFAULTS
    c = [(0.0, 0.0, 0.0, 12.0, 0, 0, 1), (1.0, 0.0, 0.0, 12.0, 0, 0, 1),      # equal counts within the radius: both die
         (10.0, 0.0, 0.0, 15.0, 0, 0, 1), (11.0, 0.0, 0.0, 12.0, 0, 0, 1),    # unequal: the weaker dies
         (20.0, 0.0, 0.0, 12.0, 0, 0, 1), (22.001, 0.0, 0.0, 30.0, 0, 0, 1)]  # just outside: both live
    assert G.non_maxi_suppression(c, prm) == [2, 4, 5]
    rng = np.random.default_rng(3)
    raw = _exp("room_fine")["raw"]
    want = {raw[i] for i in G.non_maxi_suppression(raw, prm)}
    for _ in range(3):
        sh = [raw[i] for i in rng.permutation(len(raw))]
        assert {sh[i] for i in G.non_maxi_suppression(sh, prm)} == want


@pytest.mark.parametrize("n", [99, 100, 101])
def test_cut_ties(n):
    cor = [(float(i), 0.0, 0.0, float(10 + i % 3), 0, 0, 1) for i in range(n)]
    out = G.corner_cut(cor, G.DEFAULTS)
    if n == 99:
        assert out == cor                                          # maximum_corner_num > size: as it is
    else:
        assert len(out) == 100 and out == sorted(cor, key=lambda c: (-c[3], c[0]))[:100]
        assert out[0][3] == 12.0 and out[-1][3] == 10.0 and out[-1][0] == (99.0 if n == 100 else 96.0)


def test_descriptor_edges():
    prm = G.DEFAULTS
    e2, e3, e9 = _exp("room_cut_2"), _exp("room_cut_3"), _exp("room_cut_9")
    assert (e2["stats"]["triangles_tried"], e3["stats"]["triangles_tried"], e9["stats"]["triangles_tried"]) == (0, 3, 252)
    # one triangle from each of its vertices: two of them share a key, the third comes out as (b, a, c) (below)
    assert len(e3["descs"]) == 2 and len(e2["descs"]) == 0
    tri = [(0.0, 0.0, 0.0, 11.0, 0, 0, 1), (3.0, 0.0, 0.0, 12.0, 0, 0, 1), (0.0, 4.0, 0.0, 13.0, 0, 0, 1)]
    d = G.build_stdesc(tri, prm, 7)
    # vertices 0 and 1 reach one key; from vertex 2 (a, b, c) = (4, 5, 3) and the three swaps as written, which are
    # not a full sort, leave (4, 3, 5): the reference's second descriptor of this triangle
    assert len(d) == 2 and (d["frame_id"] == 7).all()
    assert d["side_length"].tolist() == [[15.0, 20.0, 25.0], [20.0, 15.0, 25.0]]
    assert d["vertex_attached"][0].tolist() == [11.0, 12.0, 13.0]  # A opposite the longest side
    assert len(G.build_stdesc(tri, dict(prm, descriptor_min_len=3.5), 0)) == 0   # a side under the gate
    assert len(G.build_stdesc(tri, dict(prm, descriptor_max_len=4.5), 0)) == 0   # a side over it
    # two different triangles with one key: the mirror image comes later and is dropped
    both = tri + [(100.0, 0.0, 0.0, 21.0, 0, 0, 1), (103.0, 0.0, 0.0, 22.0, 0, 0, 1), (100.0, -4.0, 0.0, 23.0, 0, 0, 1)]
    d = G.build_stdesc(both, dict(prm, descriptor_near_num=3), 0)
    assert len(d) == 2 and d["vertex_attached"].max() == 13.0
    swaps = set().union(*(_exp(n)["swaps"] for n in ("room", "room_fine")))
    assert {s[1] for s in swaps} == {True, False}                  # the second swap taken and not taken
    # behind the first two swaps c = max(a, b, c), so the third (a > c) can never be taken, here or in the reference
    assert {s[2] for s in swaps} == {False}
    # the neighbours come sorted by distance, so a <= b and the first swap is dead code behind the k-NN search;
    # the restated triangle takes it when it is handed the farther neighbour first
    assert {s[0] for s in swaps} == {False}
    assert G.triangle(tri[0], tri[2], tri[1], prm)[3][0] is True
    short = _exp("room_short_sides")
    assert 0 < len(short["descs"]) < len(_exp("room")["descs"])
    assert short["descs"]["side_length"].min() >= 4.0 / 0.2 and short["descs"]["side_length"].max() <= 7.0 / 0.2


@pytest.mark.parametrize("axis", [0, 1])
def test_corner_cells(axis):
    e = _exp(f"cells_{axis}")
    job = e["jobs"][0]
    assert job["branch"] == (2 if axis == 0 else 1) and job["segments"] == 6
    assert {c: n for c, n in job["cells"].items() if n > 3} == {(1, 2): 10, (2, 1): 10, (2, 6): 9, (6, 6): 11, (10, 2): 10}
    assert job["projected"] == 53                                  # the ten points behind proj_dis_max are not among them
    raw = e["raw"]
    assert [c[3] for c in raw] == [10.0, 11.0, 10.0]               # the cell of 9 and the two empty segments give none
    # the tie inside segment (0, 0) goes to cell (1, 2), the first in x-then-y order: px = 0.75, py = 1.25 from the
    # image's minimum at (-1.9, -1.9) (axis 0: px = z, py = y; axis 1: px = -z from 3.9, py = x)
    want = (2.0, -0.65, -1.15) if axis == 0 else (-0.65, 2.0, 3.15)
    assert np.abs(np.array(raw[0][:3]) - want).max() < 1e-3
    assert raw[0][4:7] == ((1.0, 0.0, 0.0) if axis == 0 else (0.0, 1.0, 0.0))
    assert e["stats"]["corners"] == 3 and len(e["descs"]) == 2


def test_projected_5_against_6():
    a, b = _exp("projected_5"), _exp("projected_6")
    assert a["jobs"][0]["projected"] == 5 and a["stats"]["corners_raw"] == 0   # the return at 5 or fewer
    assert b["jobs"][0]["projected"] == 6 and [c[3] for c in b["raw"]] == [6.0]


@pytest.mark.parametrize("axis", [0, 1])
def test_suppression_case(axis):
    e = _exp(f"nms_{axis}")
    assert [c[3] for c in e["raw"]] == [12.0, 15.0, 15.0, 12.0, 12.0, 12.0]
    # 12 | 12 at 1.5: both die; 15 | 12 at 2.02: both live; 15 | 12 at 1.5: the 12 dies
    assert e["keep"] == [1, 2, 4]
    d = math.sqrt(G.d2f(e["raw"][1], e["raw"][4]))
    assert 2.0 < d < 2.05


@pytest.mark.parametrize("n", [99, 100, 101])
def test_cut_cases(n):
    e = _exp(f"cut_{n}")
    att = e["corners"]["attached"].tolist()
    assert e["stats"]["corners_suppressed"] == n and len(att) == min(n, 100)
    if n == 99:
        assert att == [15.0, 15.0, 12.0] * 33                      # below the cut: the suppressed list as it is
    else:
        assert att == [15.0] * 66 + [13.0] * (n - 99) + [12.0] * (34 - (n - 99))
        twelves = [tuple(c) for c in e["corners"]["xyz"][-(34 - (n - 99)):]]
        assert twelves == sorted(twelves, key=lambda c: c[1])      # ties keep the suppressed list's order


def test_empty_and_planeless_clouds():
    for name in ("empty", "no_plane"):
        e = _exp(name)
        assert e["stats"]["descs"] == 0 and e["stats"]["plane_voxels"] == 0 and len(e["planes"]) == 0


def test_the_rooms_loop_is_found():
    r = G.room_loop()
    assert r["frame"] == 0 and r["score"] > 0.5 and len(r["pairs"]) >= 4
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    # SearchLoop's transform takes the source (frame 1) onto the target (frame 0)
    # from one triangle whose corners are cell means: a corner sits within a cell (0.5) of its place and a side
    # is at least 2 long, so the rotation is within 0.25 rad and, over the room's 10 m, t within 2.5
    assert np.abs(np.asarray(r["rot"]) - R.T).max() < 0.25
    assert np.abs(np.asarray(r["t"]) - (-R.T @ np.array([2.0, -4.0, 0.0]))).max() < 2.5


def test_tolerances_are_the_measured_deviations():
    dev = G.measure_deviation()
    for k, v in dev.items():
        assert v <= G.DEV[k] <= 1.05 * v, (k, v, G.DEV[k])   # the constant is the measured value, rounded up
        assert G.TOL[k] == 8 * G.DEV[k]
