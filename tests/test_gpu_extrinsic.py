"""The scan-to-map update on the device under a LiDAR-IMU extrinsic other than the identity.

livo_params.R_LI (the reference's Lidar_rot_to_IMU) enters every stage that turns a body point into a
world point: the k-NN queries of the IEKF loop (both query_point overloads), the fused evaluation's
residual and its Jacobian row (p_I = R_LI p_b + t_LI, laser_mapping.cpp:573), the iVox searches,
both map_incremental branches and the frame stages' shared cloud source.  Everywhere else in the
suite it is the identity; here it is tests/extrinsic_cases.py's `tilt` (35 degrees about (1, 2, 3): a
transposed matrix shows) and `flip` (diag(1, -1, -1): a sign or axis mix-up shows), on scans
re-expressed (body_for) so that they still land on the map.

Bars: the ones the suite applies to the same quantities with R_LI = I, imported from the tests that
own them: world points, neighbour indices, squared distances, normals, flags, counts and maps bit
for bit; HTH and HTL 1e-9 relative; each evaluation's state delta 1e-5 relative; the covariance
1e-9 of the prior's norm.  The oracle's side of every case is held on the CPU (test_oracle.py,
test_ivox_oracle.py, test_ikd_incr_oracle.py); its floors (extrinsic_cases.oracle_floors) are
asserted here on the oracle's result alone.  Each test prints the errors it measured.
"""
import numpy as np
import pytest

import extrinsic_cases as xc
from test_gpu_parity import REL_HTH, REL_STATE, _hshare_compare, _iekf_bars, _rel

pytestmark = pytest.mark.gpu

N = 1000   # the oracle-checked scan
SID = 3


def _synth():
    from livo_amd import synth
    return synth


def _bits(x):
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_bits(v) for v in x]
    return np.asarray(x).tobytes()


def _same_bits(a, b):
    assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.fixture(scope="module")
def ctxs(built, map100k):
    """One context per extrinsic, created with it, the 100k-point map built."""
    import livo_amd
    made = {}
    for name in ("ident", "tilt", "flip"):
        R, t = xc.ext(name)
        made[name] = livo_amd.Context(0, R_LI=R, t_LI=t, max_iterations=4)
        made[name].map_build(map100k)
    yield made
    for c in made.values():
        c.close()


def _errors(tag, stg, str_, sg=None, sr=None, st0=None):
    worst = max(_rel(stg["solution"][e], str_["solution"][e]) for e in range(stg["iterations"]))
    cov = np.linalg.norm(sg["cov"] - sr["cov"]) / np.linalg.norm(st0["cov"]) if sg is not None else float("nan")
    print(f"ERR {tag}: effct {str_['effct_feat_num']} evaluations {str_['iterations']} "
          f"state delta {worst:.2e} (bar {REL_STATE:g}) cov {cov:.2e} (bar 1e-09)")


# ------------------------------------------------------------------------------- a. h_share ----
@pytest.mark.parametrize("ext", ["tilt", "flip"])
def test_h_share(ctxs, tree100k, ext):
    import oracle
    ctx = ctxs[ext]
    R_LI, t_LI = xc.ext(ext)
    body, st = xc.scan(N, SID, ext)
    sid = ctx.scan_upload(body)
    try:
        g = ctx.h_share(sid, st, search_en=True)
        r = tree100k.h_share(body, st["rot"], st["pos"], R_LI, t_LI, True)
        assert r["effct"] >= 0.9 * N, r["effct"]
        _same_bits(g["world"], oracle.to_world(body, st, R_LI, t_LI)[:, :3])
        print(f"ERR h_share {ext}: effct {r['effct']} HTH {_rel(g['HTH'], r['HTH']):.2e} "
              f"HTL {_rel(g['HTL'], r['HTL']):.2e} (bar {REL_HTH:g})")
        _hshare_compare(g, r, N, body)
        assert g["visits"] == r["visits"]
        # the evaluation without a search, at a moved state
        st2 = dict(st)
        st2["pos"] = st["pos"] + np.array([0.01, -0.02, 0.005])
        st2["rot"] = st["rot"] @ _synth().so3_exp(np.array([0.002, -0.001, 0.003]))
        g2 = ctx.h_share(sid, st2, search_en=False)
        r2 = tree100k.h_share(body, st2["rot"], st2["pos"], R_LI, t_LI, False, cache=r["cache"])
        assert r2["effct"] >= 0.9 * N
        _same_bits(g2["world"], oracle.to_world(body, st2, R_LI, t_LI)[:, :3])
        print(f"ERR h_share {ext} no search: effct {r2['effct']} HTH {_rel(g2['HTH'], r2['HTH']):.2e} "
              f"HTL {_rel(g2['HTL'], r2['HTL']):.2e}")
        _hshare_compare(g2, r2, N, body)
    finally:
        ctx.scan_release(sid)


# --------------------------------------------------------------- b. the update by search path ----
KINDS = {"static": {}, "gen": {"LIVO_EVAL_GEN": "1"}, "leaf": {"LIVO_KNN_KIND": "leaf"},
         "grid": {"LIVO_KNN_KIND": "grid"}, "tile": {"LIVO_KNN_KIND": "tile"}, "novruns": {"LIVO_VRUNS": "0"}}


@pytest.mark.parametrize("kind", list(KINDS))
def test_iekf_by_search_path(built, map100k, tree100k, kind, monkeypatch):
    """The fused static kernel (the staged pose's query_point), the generic kernel, the leaf, grid and tile
    searches (the slot's query_point) and the map without vertex runs, at max_iterations 4 and 0.  After
    the single evaluation of max_iterations 0 the scan's neighbour record is the k-NN of
    oracle.to_world's points, bit for bit."""
    import livo_amd
    import oracle
    R_LI, t_LI = xc.ext("tilt")
    body, st = xc.scan(N, SID, "tilt")
    for k in ("LIVO_EVAL_GEN", "LIVO_KNN_KIND", "LIVO_VRUNS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in KINDS[kind].items():
        monkeypatch.setenv(k, v)
    with livo_amd.Context(0, R_LI=R_LI, t_LI=t_LI, max_iterations=4) as ctx:
        ctx.map_build(map100k)
        sid = ctx.scan_upload(body)
        for mi in (4, 0):
            ctx.set_params(max_iterations=mi)
            sg, stg = ctx.iekf_update(sid, st)
            sr, str_ = tree100k.iekf_update(body, st, R_LI=R_LI, t_LI=t_LI, max_iter=mi)
            xc.oracle_floors(str_, N, mi)
            _errors(f"iekf {kind} max_iterations {mi}", stg, str_, sg, sr, st)
            _iekf_bars(sg, stg, sr, str_, st)
        assert str_["iterations"] == 1
        gi, gd = ctx.scan_neighbors(sid)
        ri, rd, _ = tree100k.knn(oracle.to_world(body, st, R_LI, t_LI)[:, :3])
        assert np.array_equal(gi, ri)
        _same_bits(gd, rd)


# ------------------------------------------------------------------ c. prior differs from state ----
def test_iekf_prior_differs(ctxs, tree100k):
    """state_propagat != state under tilt (tests/test_gpu_parity.py's case): the prior term is exercised."""
    synth = _synth()
    ctx = ctxs["tilt"]
    R_LI, t_LI = xc.ext("tilt")
    body, st0 = xc.scan(5_000, 2, "tilt")
    prior = dict(st0)
    prior["pos"] = st0["pos"] + np.array([0.02, 0.0, -0.01])
    prior["rot"] = st0["rot"] @ synth.so3_exp(np.array([0.002, -0.001, 0.003]))
    prior["vel"] = np.array([0.5, 0.1, 0.0])
    sid = ctx.scan_upload(body)
    try:
        sg, stg = ctx.iekf_update(sid, st0, prior)
    finally:
        ctx.scan_release(sid)
    sr, str_ = tree100k.iekf_update(body, st0, prior, R_LI=R_LI, t_LI=t_LI, max_iter=4)
    xc.oracle_floors(str_, 5_000)
    _errors("iekf prior differs", stg, str_)
    assert stg["iterations"] == str_["iterations"]
    assert stg["effct_feat_num"] == str_["effct_feat_num"]
    for e in range(stg["iterations"]):
        assert _rel(stg["solution"][e], str_["solution"][e]) < REL_STATE
    assert _rel(sg["vel"], sr["vel"]) < REL_STATE


# -------------------------------------------------------------------------------------- d. batch ----
def _ragged(ext):
    """The oracle-checked scan and its companions of 0, 1, 63, 64 and 257 points, with their states."""
    synth = _synth()
    R, t = xc.ext(ext)
    scans, states = [xc.scan(N, SID, ext)[0]], [synth.make_state(SID)]
    for k, n in enumerate(xc.RAGGED):
        scans.append(xc.body_for(synth.make_scan(max(n, 1), 10 + k)[0][:n], R, t))
        states.append(synth.make_state(10 + k))
    return scans, states


def test_batch(ctxs, tree100k):
    ctx = ctxs["tilt"]
    R_LI, t_LI = xc.ext("tilt")
    scans, states = _ragged("tilt")
    assert [len(s) for s in scans] == [N, *xc.RAGGED]
    sids = [ctx.scan_upload(s) for s in scans]
    try:
        b, bst = ctx.iekf_update_batch(sids, states)
        for i, sid in enumerate(sids):
            one, st1 = ctx.iekf_update(sid, states[i])
            assert _bits(one) == _bits(b[i]), i
            assert _bits(st1) == _bits(bst[i]), i
        t = ctx.iekf_update_batch_submit(sids, states)
        w, wst = ctx.iekf_update_batch_wait(t, len(sids))
        assert _bits(w) == _bits(b) and _bits(wst) == _bits(bst)
    finally:
        for sid in sids:
            ctx.scan_release(sid)
    sr, str_ = tree100k.iekf_update(scans[0], states[0], R_LI=R_LI, t_LI=t_LI, max_iter=4)
    xc.oracle_floors(str_, N)
    _errors("batch scan 0", bst[0], str_, b[0], sr, states[0])
    _iekf_bars(b[0], bst[0], sr, str_, states[0])


# ----------------------------------------------------------------------- e. live parameter change ----
def test_set_params_changes_every_parameter_block(ctxs, map100k):
    """One context, the map built once and the scans uploaded once; set_params(R_LI, t_LI) in the order
    ident, tilt, flip, ident.  Every update (the scan made for that extrinsic and the two that are not)
    and its neighbour record equal, bit for bit, those of the context created with that extrinsic: a
    parameter block staged once and not refreshed would show."""
    import livo_amd
    bodies = {name: xc.scan(N, SID, name) for name in ("ident", "tilt", "flip")}
    want = {}
    for name, ctx in ctxs.items():
        for made_for, (body, st) in bodies.items():
            sid = ctx.scan_upload(body)
            try:
                want[name, made_for] = (ctx.iekf_update(sid, st), ctx.scan_neighbors(sid), ctx.h_share(sid, st, True))
            finally:
                ctx.scan_release(sid)
    assert _bits(want["ident", "ident"][0]) != _bits(want["tilt", "ident"][0])  # (the extrinsic matters)
    assert want["tilt", "tilt"][0][1]["effct_feat_num"][0] >= 0.9 * N
    assert want["flip", "flip"][0][1]["effct_feat_num"][0] >= 0.9 * N
    with livo_amd.Context(0, max_iterations=4) as ctx:
        ctx.map_build(map100k)
        sids = {made_for: ctx.scan_upload(body) for made_for, (body, _) in bodies.items()}
        for name in ("ident", "tilt", "flip", "ident"):
            R, t = xc.ext(name)
            ctx.set_params(R_LI=R, t_LI=t)
            for made_for, (_, st) in bodies.items():
                got = (ctx.iekf_update(sids[made_for], st), ctx.scan_neighbors(sids[made_for]),
                       ctx.h_share(sids[made_for], st, True))
                assert _bits(got) == _bits(want[name, made_for]), (name, made_for)


# -------------------------------------------------------------------------------- f. iVox backend ----
def test_ivox_backend(built):
    import livo_amd
    import oracle
    from test_gpu_ivox import _dump_by_grid, _hs_equal, _iekf_check, _oracle_by_grid
    synth = _synth()
    R_LI, t_LI = xc.ext("tilt")
    m = synth.make_map(100_000)
    with livo_amd.Context(0, R_LI=R_LI, t_LI=t_LI, max_iterations=4) as ctx:
        ctx.set_backend(livo_amd.BACKEND_IVOX)
        ctx.ivox_init()
        iv = oracle.Ivox()
        ctx.ivox_add_points(m)
        iv.add_points(m)
        # h_share with and without a search, then the update, on scans of their own
        body, st = xc.scan(N, SID, "tilt")
        sid = ctx.scan_upload(body)
        g = ctx.h_share(sid, st, search_en=True)
        r = iv.h_share(body, st["rot"], st["pos"], R_LI, t_LI, True, oracle.new_cache(N))
        # (on the 100k-point map the iVox search, confined to the 18 nearby 0.2 m grids, finds five neighbours
        # for about 0.6 N points whatever the extrinsic: the floor here is the identity-extrinsic scan's count)
        bi, sti = xc.scan(N, SID, "ident")
        ri = iv.h_share(bi, sti["rot"], sti["pos"], *xc.ident(), True, oracle.new_cache(N))
        assert abs(r["effct"] - ri["effct"]) <= 0.01 * N and r["effct"] >= 0.5 * N, (r["effct"], ri["effct"])
        print(f"ERR ivox h_share: effct {r['effct']} HTH {_rel(g['HTH'], r['HTH']):.2e} HTL {_rel(g['HTL'], r['HTL']):.2e}")
        _hs_equal(g, r)
        st2 = dict(st)
        st2["pos"] = st["pos"] + np.array([0.02, 0.01, -0.01])
        _hs_equal(ctx.h_share(sid, st2, search_en=False),
                  iv.h_share(body, st2["rot"], st2["pos"], R_LI, t_LI, False, r["cache"]))
        ctx.scan_release(sid)
        sid = ctx.scan_upload(body)
        sg, stg = ctx.iekf_update(sid, st)
        ctx.scan_release(sid)
        sr, str_ = iv.iekf_update(body, st, oracle.new_cache(N), R_LI=R_LI, t_LI=t_LI, max_iter=4)
        assert str_["iterations"] >= 2 and str_["effct_feat_num"][0] == r["effct"]
        _errors("ivox iekf", stg, str_, sg, sr, st)
        _iekf_check(stg, sg, str_, sr, st)
        # two scans of the odometry sequence: neighbours carried over, update, map_incremental
        prev_sid, cache = None, oracle.new_cache(0)
        for k, n in enumerate((1500, 1000)):
            body, st0 = xc.scan(n, 21 + k, "tilt")
            sid = ctx.scan_upload(body)
            if prev_sid is not None:
                ctx.scan_inherit_neighbors(sid, prev_sid)
                ctx.scan_release(prev_sid)
            cache = oracle.resize_cache(cache, n)
            sg, stg = ctx.iekf_update(sid, st0)
            sr, str_ = iv.iekf_update(body, st0, cache, R_LI=R_LI, t_LI=t_LI)
            _iekf_check(stg, sg, str_, sr, st0)
            gi, _ = ctx.scan_neighbors(sid)
            assert np.array_equal(gi, cache["idx"])
            cat_g, cnt_g = ctx.map_incremental(sid, sr, filter_size_map=0.5)
            cat_r, cnt_r = iv.map_incremental(body, sr, cache, R_LI=R_LI, t_LI=t_LI, filter_size_map=0.5)
            assert np.array_equal(cat_g, cat_r) and cnt_g == cnt_r
            assert cnt_r["added"] > 0
            prev_sid = sid
        ctx.scan_release(prev_sid)
        assert ctx.ivox_info()["num_points"] == iv.info()["num_points"]
        assert _dump_by_grid(*ctx.ivox_dump()) == _oracle_by_grid(iv)


# ----------------------------------------------------------------------- g. ikd incremental map ----
def test_ikd_map_incremental(built, map100k):
    import livo_amd
    import oracle
    from test_gpu_ikd_incr import _same_add, _same_map
    R_LI, t_LI = xc.ext("tilt")
    dm = oracle.DynMap(map100k)
    with livo_amd.Context(0, R_LI=R_LI, t_LI=t_LI, max_iterations=4) as ctx:
        ctx.map_build(map100k)
        body, st = xc.scan(5_000, 0, "tilt")
        sid = ctx.scan_upload(body)
        cat, g = ctx.map_incremental(sid, st, filter_size_map=0.3)
        ctx.scan_release(sid)
        assert np.all(cat == 1)
        r = dm.map_incremental(body, st, R_LI=R_LI, t_LI=t_LI, filter_size_map=0.3)
        assert r["added"] > 0 and r["events"] > 0
        _same_add(g, r)
        _same_map(ctx, dm)
        body, st = xc.scan(N, 1, "tilt")
        sid = ctx.scan_upload(body)
        gs, gst = ctx.iekf_update(sid, st)
        ctx.scan_release(sid)
    rs, rst = dm.iekf_update(body, st, R_LI=R_LI, t_LI=t_LI, max_iter=4)
    xc.oracle_floors(rst, N)
    _errors("iekf on the updated map", gst, rst, gs, rs, st)
    assert gst["iterations"] == rst["iterations"] and gst["effct_feat_num"] == rst["effct_feat_num"]
    for e in range(gst["iterations"]):
        assert _rel(gst["solution"][e], rst["solution"][e]) < REL_STATE, e


# --------------------------------------------------------------------------------------- h. IKFoM ----
def test_ikfom_reads_the_state_extrinsic_only(ctxs, tree100k):
    """The IKFoM h-model takes its extrinsic from the state (offset_R_L_I, offset_T_L_I), not from
    livo_params: a context created with the tilt extrinsic gives the identity context's bytes, and both
    meet the oracle at the bars of tests/test_gpu_ikfom.py."""
    from test_gpu_ikfom import _compare
    synth = _synth()
    body = synth.make_scan(N, 7)[0]
    st0 = synth.make_ikfom_state(7)
    out = {}
    for name in ("ident", "tilt"):
        sid = ctxs[name].scan_upload(body)
        try:
            out[name] = ctxs[name].ikfom_update(sid, st0)
        finally:
            ctxs[name].scan_release(sid)
    assert _bits(out["tilt"]) == _bits(out["ident"])
    r, rs = tree100k.ikfom_update(body, st0, max_iter=4)
    assert rs["effct_feat_num"][0] >= 0.9 * N and rs["iterations"] >= 2
    _compare(out["tilt"][0], out["tilt"][1], r, rs, st0)


# -------------------------------------------------------------------------------- i. frame stages ----
def _cloud_is_restated(ctx, sid, body, st, R_LI, t_LI):
    """livo_frame_to_world of the scan = the restatement of pointBodyToWorld under (R_LI, t_LI), bit for bit:
    the cloud source every frame stage reads."""
    from test_vis_select_abi import restate_world
    world = ctx.frame_to_world(st, sid)
    _same_bits(world[:, :3], restate_world(body, st["rot"], st["pos"], R_LI, t_LI))
    return world


def test_colorize(ctxs):
    """tests/test_gpu_rgb_cloud.py's wide camera on a 5,000-point frame re-expressed under tilt."""
    from test_gpu_rgb_cloud import _cameras, _check_parity
    from test_rgb_cloud_abi import BEHIND, KEPT, OUT_OF_FRAME, random_image
    synth = _synth()
    ctx = ctxs["tilt"]
    R_LI, t_LI = xc.ext("tilt")
    n = 5000
    raw = synth.make_raw_scan(n, n % 7)[0].copy()
    raw[:, :3] = xc.body_for(raw[:, :3], R_LI, t_LI)
    st = synth.make_state(n % 7)
    image = random_image()
    sid, und, down = ctx.scan_preprocess(raw, leaf_size=0.5)  # (no poses: the points as they are)
    try:
        _cloud_is_restated(ctx, -1, und[:, :3], st, R_LI, t_LI)
        _cloud_is_restated(ctx, sid, down[:, :3], st, R_LI, t_LI)
        fate = _check_parity(ctx, st, _cameras()["wide"], image, -1)
        assert len(fate) == n and 0.2 < np.mean(fate == KEPT) < 0.8
        assert np.sum(fate == OUT_OF_FRAME) > 0 and np.sum(fate == BEHIND) > 0
        assert len(_check_parity(ctx, st, _cameras()["wide"], image, sid)) == len(down)
    finally:
        ctx.scan_release(sid)


def test_vio_select(ctxs):
    """tests/test_gpu_vis_select.py's 160 x 152, grid 40 frame (the one with the cell overflow) at 3,000 points."""
    from test_gpu_vis_select import _params
    from test_vis_select_abi import case_worth, frame_case, restate_case
    ctx = ctxs["tilt"]
    R_LI, t_LI = xc.ext("tilt")
    name, n = "160x152-g40", 3000
    st, body = frame_case(name, n, R_LI, t_LI)
    img, vp, grid = _params(name)
    sid = ctx.scan_upload(body)
    try:
        world = _cloud_is_restated(ctx, sid, body, st, R_LI, t_LI)
        pts, pat, stats = ctx.vio_select(st, img, vp, grid, sid)
    finally:
        ctx.scan_release(sid)
    rec, want_pat, want_stats, info = restate_case(name, world[:, :3], st)
    case_worth(name, n, want_stats, info)
    assert stats == want_stats
    assert pts.tobytes() == rec.tobytes()
    assert pat.shape == want_pat.shape and np.array_equal(pat.view(np.uint32), want_pat.view(np.uint32))


def test_vio_match(ctxs):
    """tests/test_gpu_vmatch.py's closed loop: select on frame A, store, match on frame B, on clouds
    expressed under tilt."""
    from test_gpu_vmatch import Rig
    from test_vmatch_abi import Scene, moved, small_cam
    synth = _synth()
    ctx = ctxs["tilt"]
    R_LI, t_LI = xc.ext("tilt")
    cam = small_cam()
    A = synth.make_state(1)
    sc = Scene(A, cam)
    imgA = sc.render(A)
    B = moved(A, [0.03, -0.02, 0.015], [0.2, -0.15, 0.1])
    imgB = sc.render(B)
    rig = Rig(ctx, cam)
    bodyA = sc.cloud(A, 4000, 1, R_LI=R_LI, t_LI=t_LI)
    sid = ctx.scan_upload(bodyA)
    try:
        _cloud_is_restated(ctx, sid, bodyA, A, R_LI, t_LI)
        pts, pat, _ = ctx.vio_select(A, imgA, rig.vp, 16, sid)
    finally:
        ctx.scan_release(sid)
    assert len(pts) >= 30
    rig.add_frame(0, A, imgA, upload=False)
    rig.add(0, pts, pat)
    rig.check_dump()
    dev, ref = rig.match_equal(B, imgB, sc.cloud(B, 4000, 2, R_LI=R_LI, t_LI=t_LI), 16)
    assert ref[4]["n_out"] >= 20 and ref[4]["warp_shared"] >= 1
