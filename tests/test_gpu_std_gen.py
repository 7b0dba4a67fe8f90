"""GenerateSTDescs on the device (livo_std_key_*, livo_std_generate, livo_std_staged) against the scalar
restatement (tests/std_gen_cases.py): every count, the plane flags and plane-cloud order, the jobs and their
members, the corner order and attached counts, the descriptors' order, frame_id and vertex_attached exactly;
centres, normals, corner coordinates, side lengths and vertices within 8 x the restatement's own measured
deviation from a 60-digit evaluation (std_gen_cases.TOL).  Clouds of at most 10k points.

Measured on the MI355X: see DESIGN.md 8.17."""
import ctypes as C

import numpy as np
import pytest

import std_cases as S
import std_gen_cases as G

pytestmark = pytest.mark.gpu
E_INVALID, E_RANGE = -1, -6
NAMES = list(G.cases())


def _gen(ctx, case, reset=True):
    import livo_amd
    if reset:
        ctx.std_reset(livo_amd.std_params(**G.LOOP_PRM), 4096, 8, 4096)
        for _ in range(case.frame_id):  # empty key frames in front, so that the frame's index is its frame_id
            ctx.std_stage(np.zeros(0, S.DESC), np.zeros(0, S.PLANE))
            ctx.std_commit()
    ctx.std_key_clear()
    ctx.std_key_add_host(case.pts)
    return ctx.std_generate(livo_amd.std_gen_params(**case.prm))


@pytest.mark.parametrize("name", NAMES)
def test_generate_equals_the_restatement(gpu_ctx, name):
    case = G.cases()[name]
    exp = case.expected()
    stats = _gen(gpu_ctx, case)
    assert stats == exp["stats"], (name, stats, exp["stats"])
    vox, jobs = gpu_ctx.std_gen_debug()
    assert np.array_equal(vox, exp["voxels"])                      # visiting order, counts, plane flags
    assert len(jobs) == len(exp["jobs"])
    for j, e in zip(jobs, exp["jobs"]):
        assert (j[0], j[1], j[2]) == (e["v"], e["c"], e["projected"]) and j[3:].tolist() == e["members"], (name, e)
    descs, planes, corners = gpu_ctx.std_staged()
    ep, ec, ed = exp["planes"], exp["corners"], exp["descs"]
    assert len(planes) == len(ep) and len(corners) == len(ec) and len(descs) == len(ed)
    dev = dict(center=0.0, normal=0.0, corner=0.0, side=0.0, vertex=0.0)
    if len(ep):
        # the plane cloud is cast to float: the tolerance, and the spacing of floats at the value for the cast
        for f, k in (("xyz", "center"), ("normal", "normal")):
            d = np.abs(planes[f].astype(np.float64) - ep[f].astype(np.float64))
            dev[k] = float(d.max())
            assert (d <= G.TOL[k] + np.spacing(np.abs(ep[f]))).all(), (name, f, d.max())
    if len(ec):
        assert np.array_equal(corners["attached"], ec["attached"])
        d = np.abs(corners["xyz"].astype(np.float64) - ec["xyz"].astype(np.float64))
        dev["corner"] = float(d.max())
        assert (d <= G.TOL["corner"] + np.spacing(np.abs(ec["xyz"]))).all(), (name, d.max())
        dn = np.abs(corners["normal"].astype(np.float64) - ec["normal"].astype(np.float64))
        assert (dn <= G.TOL["normal"] + np.spacing(np.abs(ec["normal"]))).all(), (name, dn.max())
    if len(ed):
        assert np.array_equal(descs["frame_id"], ed["frame_id"]) and (descs["frame_id"] == case.frame_id).all()
        assert np.array_equal(descs["vertex_attached"], ed["vertex_attached"])
        dev["side"] = float(np.abs(descs["side_length"] - ed["side_length"]).max())
        dev["vertex"] = float(max(np.abs(descs[f] - ed[f]).max() for f in ("vertex_A", "vertex_B", "vertex_C", "center")))
        assert dev["side"] <= G.TOL["side"]
        # a vertex is a corner's float coordinates: the corner's allowance, element by element; the centre adds its own
        for f in ("vertex_A", "vertex_B", "vertex_C"):
            lim = G.TOL["corner"] + np.spacing(np.abs(ed[f]).astype(np.float32)).astype(np.float64)
            assert (np.abs(descs[f] - ed[f]) <= lim).all(), (name, f)
        lim = G.TOL["corner"] + G.TOL["vertex"] + np.spacing(np.abs(ed["center"]).astype(np.float32)).astype(np.float64)
        assert (np.abs(descs["center"] - ed["center"]) <= lim).all(), name
    print(name, "device deviation", {k: f"{v:.2e}" for k, v in dev.items()}, "tol", {k: f"{v:.2e}" for k, v in G.TOL.items()})
    assert gpu_ctx.std_key_count() == 0                            # laser_mapping.cpp:1249
    info = gpu_ctx.std_info()
    assert info["staged_descs"] == len(ed) and info["staged_planes"] == len(ep)
    res = gpu_ctx.std_search()                                     # nothing committed that could match
    if len(ed) == 0:
        assert (res["frame"], res["score"]) == (-1, 0.0)


def test_room_loop_through_search_and_commit(gpu_ctx):
    cs = G.cases()
    a, b = cs["room"], cs["room_again"]
    _gen(gpu_ctx, a)
    da, pa, _ = gpu_ctx.std_staged()
    assert gpu_ctx.std_commit() == 0
    _gen(gpu_ctx, b, reset=False)
    db_, pb, _ = gpu_ctx.std_staged()
    assert (db_["frame_id"] == 1).all()
    res = gpu_ctx.std_search()
    cands = gpu_ctx.std_candidates()
    # the existing restatement of SearchLoop on the device's own products
    db = S.Db()
    db.add(da, pa)
    exp = S.search_loop(db, db_, pb, G.LOOP_PRM)
    assert res["frame"] == exp["frame"] == 0 and res["score"] == exp["score"]
    assert len(cands) == len(exp["candidates"])
    for k, (c, e) in enumerate(zip(cands, exp["candidates"])):
        assert (int(c["frame"]), int(c["votes"]), int(c["max_vote"])) == (e["frame"], e["votes"], e["max_vote"])
        m = gpu_ctx.std_matches(k)
        assert list(zip(m["src"].tolist(), m["db_index"].tolist())) == e["matches"]
    assert list(zip(res["pairs"]["src"].tolist(), res["pairs"]["db_index"].tolist())) == exp["pairs"]
    assert np.abs(res["rot"] - exp["rot"]).max() <= S.ROT_TOL and np.abs(res["t"] - exp["t"]).max() <= S.T_TOL
    # ... and on the restatement's: the same loop
    want = G.room_loop()
    assert want["frame"] == 0 and len(want["pairs"]) == len(exp["pairs"])
    assert gpu_ctx.std_commit() == 1


def test_two_generates_give_the_same_bytes(gpu_ctx):
    case = G.cases()["room_fine"]
    out = []
    for _ in range(2):
        st = _gen(gpu_ctx, case)
        d, p, c = gpu_ctx.std_staged()
        v, j = gpu_ctx.std_gen_debug()
        out.append((tuple(st.items()), d.tobytes(), p.tobytes(), c.tobytes(), v.tobytes(), j.tobytes()))
    assert out[0] == out[1] and len(out[0][1]) > 0


def test_key_add_of_the_published_cloud_equals_the_host_points(gpu_ctx):
    import livo_amd
    from livo_amd import synth
    case = G.cases()["room"]
    L = synth.make_state(2)
    sid = gpu_ctx.scan_upload(np.asarray(case.pts, np.float32))
    try:
        world = gpu_ctx.frame_to_world(L, sid)                      # what livo_cloud_publish keeps, point for point
        gpu_ctx.cloud_publish(L, sid, match_leaf=0.0)
    finally:
        gpu_ctx.scan_release(sid)
    prm = livo_amd.std_gen_params(**case.prm)
    out = []
    for device in (False, True):
        gpu_ctx.std_reset(livo_amd.std_params(**G.LOOP_PRM), 4096, 8, 4096)
        gpu_ctx.std_key_clear()
        if device:
            gpu_ctx.std_key_add(livo_amd.CLOUD_WORLD)
            gpu_ctx.std_key_add(livo_amd.CLOUD_WORLD)               # appended behind the first
        else:
            gpu_ctx.std_key_add_host(world)                         # rows of five floats: the stride
            gpu_ctx.std_key_add_host(world[:, :3])
        assert gpu_ctx.std_key_count() == 2 * len(world)
        st = gpu_ctx.std_generate(prm)
        out.append((tuple(st.items()),) + tuple(a.tobytes() for a in gpu_ctx.std_staged()))
    assert out[0] == out[1] and out[0][0][0] == ("points", 2 * len(world)) and len(out[0][2]) > 0


def test_refusals_come_back_as_codes(gpu_ctx):
    import livo_amd
    L, h = gpu_ctx._L, gpu_ctx.h
    p = livo_amd.std_gen_params()
    gpu_ctx.std_reset(livo_amd.std_params(), 64, 4, 64)
    gpu_ctx.std_key_clear()
    far = np.array([[2.0 * (2 ** 20), 0.0, 0.0], [1.0, 1.0, 1.0]], np.float32)
    gpu_ctx.std_key_add_host(far)
    assert L.livo_std_generate(h, C.byref(p), None) == E_RANGE      # a voxel coordinate past the packed key
    assert gpu_ctx.std_key_count() == 2                             # a refused call keeps the key cloud
    gpu_ctx.std_key_clear()
    assert gpu_ctx.std_key_count() == 0
    assert L.livo_std_key_add(h, 12345) == -4                       # LIVO_E_NOSCAN, as livo_frame_to_world
    bad = livo_amd.std_gen_params(voxel_size=2.5)
    assert L.livo_std_generate(h, C.byref(bad), None) == E_RANGE
    n = C.c_int64()
    assert L.livo_std_staged(h, None, 0, C.byref(n), None, 0, None, None, 0, None) == E_INVALID   # nothing staged


def test_a_generate_before_a_reset_is_refused():
    import livo_amd
    ctx = livo_amd.Context()
    try:
        ctx.std_key_add_host(np.ones((3, 3), np.float32))
        p = livo_amd.std_gen_params()
        assert ctx._L.livo_std_generate(ctx.h, C.byref(p), None) == E_INVALID
        assert ctx.std_key_count() == 3
    finally:
        ctx.close() if hasattr(ctx, "close") else None
