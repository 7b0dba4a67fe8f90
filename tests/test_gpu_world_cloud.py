"""GPU checks of the LiDAR-to-camera hand-off: livo_cloud_publish stores pcl_wait_pub (the LiDAR frame's world
cloud at the LIO state) and pg_down (its 0.2 m VoxelGrid) on the device, and livo_frame_to_world,
livo_cloud_colorize, livo_vio_select, livo_vio_match and livo_vio_detect read them through LIVO_CLOUD_WORLD and
LIVO_CLOUD_WORLD_DOWN at a camera state of their own.

Bars: byte equality everywhere, against calls on the source scan or against the restatements of
test_rgb_cloud_abi.py, test_vis_select_abi.py and test_vmatch_abi.py fed the published points and the camera's
pose.  The one exception is pg_down's centroids: voxel set, order and count exact, the values within the
front-end's own bars for the same filter (2e-6 relative against oracle.voxel_grid as in test_gpu_frontend.py, and
frontend_cases.check_voxels with the device's summation bound as in test_gpu_frontend_edges.py), both taken on the
device's own world points.  Sizes 1, 255, 256, 257 around the stage kernels' blocks of 256 points, and clouds of
4,000 points on the walls of test_vmatch_abi.Scene; 160 x 128 images, patch_size 4.
"""
import ctypes as C

import numpy as np
import pytest

import frontend_cases as fc
from test_gpu_vdetect import GRID, PS, assert_same_map, new_ctx, state_bytes, vio_params
from test_gpu_vmatch import Rig, side, world0  # noqa: F401  (world0: a module fixture, the wall with the board)
from test_gpu_vobserve import unpack, world  # noqa: F401  (world: a module fixture, the bare wall)
from test_rgb_cloud_abi import KEPT, restate_colorize, restate_stats
from test_vis_select_abi import restate_select
from test_vmatch_abi import moved

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
WORLD, DOWN = 0x40000000, 0x40000001  # LIVO_CLOUD_WORLD, LIVO_CLOUD_WORLD_DOWN (test_world_cloud_abi.py)
INVALID, NOSCAN = -1, -4
SIZES = (1, 255, 256, 257, 4000)


@pytest.fixture(scope="module")
def wctx(built):
    ctx = new_ctx()
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def ictx(built):
    """No lever arm: at the state IDENT a published point is its body point (rounded through double)."""
    import livo_amd
    ctx = livo_amd.Context(0, t_LI=np.zeros(3))
    yield ctx
    ctx.close()


def ident():
    from livo_amd import synth
    st = synth.make_state(0)
    st["rot"], st["pos"] = np.eye(3), np.zeros(3)
    return st


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def raw_publish(ctx, sid, st, leaf=0.2):
    import livo_amd
    info = livo_amd.CloudInfo()
    s = None if st is None else C.byref(livo_amd.state_to_c(st))
    return ctx._L.livo_cloud_publish(ctx.h, sid, s, C.c_float(leaf), C.byref(info)), info


def gray3(img):
    return np.ascontiguousarray(np.stack([img, 255 - img, img // 2 + 60], axis=2))


def source(ctx, kind, n, seed):
    """-> (src id for livo_cloud_publish, the resident scan to release)."""
    from livo_amd import synth
    if kind == "scan":  # a resident scan: stored in Morton order, read in the caller's (random) order
        body = (np.random.default_rng(seed).normal(size=(n, 3)) * [6.0, 4.0, 2.0]).astype(F32)
        sid = ctx.scan_upload(body)
        return sid, sid
    raw, poses, Re, pe = synth.make_raw_scan(n, seed)
    sid, _, _ = ctx.scan_preprocess(raw, poses, Re, pe, leaf_size=0.5)
    return -1, sid


# ------------------------------------------------------- 1. published bytes ----
@pytest.mark.parametrize("kind", ["scan", "frame"])
@pytest.mark.parametrize("n", SIZES)
def test_published_bytes(wctx, n, kind):
    from livo_amd import synth
    L, X = synth.make_state(2), synth.make_state(5)
    src, sid = source(wctx, kind, n, 3)
    try:
        want = wctx.frame_to_world(L, src)
        info = wctx.cloud_publish(L, src, match_leaf=0.0)
    finally:
        wctx.scan_release(sid)
    assert want.shape == (n, 5) and info["n"] == n and info["n_down"] == -1 and info["down_filtered"] == 0
    assert info["device_bytes"] >= 20 * n and wctx.cloud_info() == info
    got = wctx.frame_to_world(X, WORLD)  # an unrelated state: ignored
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    if kind == "scan":
        assert not np.any(want[:, 3:])  # a resident scan keeps x, y, z only
    else:
        assert not np.any(want[:, 4])  # (intensity copied; the curvature of a fresh point)


def test_negative_zero_survives(ictx):
    """A world x of -0.0f: -1e-30 times cos(pi / 2) = 6e-17 underflows the float.  An identity transform of the
    stored point would give +0.0 (-0.0 + 0.0)."""
    L = ident()
    c = np.cos(np.pi / 2)
    L["rot"] = np.array([[c, -1.0, 0.0], [1.0, c, 0.0], [0.0, 0.0, 1.0]])
    body = (np.random.default_rng(1).normal(size=(257, 3)) * 3.0).astype(F32)
    body[100] = [-1e-30, 0.0, 2.0]
    sid = ictx.scan_upload(body)
    try:
        want = ictx.frame_to_world(L, sid)
        ictx.cloud_publish(L, sid, match_leaf=0.0)
    finally:
        ictx.scan_release(sid)
    assert bits(want)[100, 0] == 0x80000000
    got = ictx.frame_to_world(ident(), WORLD)
    assert np.array_equal(bits(got), bits(want))


# --------------------------------------------------------------- 2. lifetime ----
def test_lifetime(built):
    import livo_amd
    from livo_amd import synth
    ctx = new_ctx()
    try:
        L, X = synth.make_state(2), synth.make_state(6)
        raw, poses, Re, pe = synth.make_raw_scan(4000, 2)
        sid, _, _ = ctx.scan_preprocess(raw, poses, Re, pe, leaf_size=0.5)
        want = ctx.frame_to_world(L, -1)
        info = ctx.cloud_publish(L, -1, match_leaf=0.2)
        down = ctx.frame_to_world(X, DOWN)
        assert info["n"] == 4000 and 0 < info["n_down"] == len(down) < 4000 and info["down_filtered"] == 1

        def intact():
            return (np.array_equal(bits(ctx.frame_to_world(X, WORLD)), bits(want)) and
                    np.array_equal(bits(ctx.frame_to_world(X, DOWN)), bits(down)) and ctx.cloud_info() == info)

        raw2, poses2, Re2, pe2 = synth.make_raw_scan(3000, 4)  # feats_undistort is overwritten ...
        sid2, _, _ = ctx.scan_preprocess(raw2, poses2, Re2, pe2, leaf_size=0.5)
        assert len(ctx.frame_to_world(L, -1)) == 3000 and intact()
        ctx.scan_release(sid)  # ... the frame's resident scan released ...
        ctx.map_build(synth.make_map(20_000))
        ctx.map_add_points(synth.make_map(3_000, seed=5) + F32(0.3))  # ... and the map changed
        assert intact()
        # refused publishes leave both clouds
        for rc in (raw_publish(ctx, 77, L)[0], raw_publish(ctx, sid, L)[0]):  # unknown, released
            assert rc == NOSCAN
        for rc in (raw_publish(ctx, sid2, L, float("nan"))[0], raw_publish(ctx, sid2, None)[0],
                   raw_publish(ctx, WORLD, L)[0], raw_publish(ctx, DOWN, L)[0]):
            assert rc == INVALID
        assert intact()
        # a second publish replaces both
        L2 = synth.make_state(4)
        want2 = ctx.frame_to_world(L2, sid2)
        info2 = ctx.cloud_publish(L2, sid2, match_leaf=0.3)
        assert info2["n"] == len(want2) != 4000 and 0 < info2["n_down"] < info2["n"]
        assert np.array_equal(bits(ctx.frame_to_world(X, WORLD)), bits(want2))
        down2 = ctx.frame_to_world(X, DOWN)
        assert len(down2) == info2["n_down"]
        fc.check_voxels(down2, want2, 0.3, fc.device_adds)
        ctx.scan_release(sid2)
        assert np.array_equal(bits(ctx.frame_to_world(X, DOWN)), bits(down2))
        assert (livo_amd.CLOUD_WORLD, livo_amd.CLOUD_WORLD_DOWN) == (WORLD, DOWN)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 3. pg_down ----
def _close(a, b, rel=2e-6):  # test_gpu_frontend.py's bar for the same filter
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return np.all(np.abs(a - b) <= rel * np.maximum(np.abs(b), 1.0))


def check_down(ctx, L, src, leaf):
    """Publishes twice; pg_down against both references on the device's own world points.  -> world, down, info"""
    import oracle
    import frontend_ref as fr
    outs = []
    for _ in range(2):
        info = ctx.cloud_publish(L, src, match_leaf=leaf)
        outs.append((ctx.frame_to_world(L, WORLD), ctx.frame_to_world(L, DOWN), info))
    (world_pts, down, info), again = outs
    assert np.array_equal(bits(again[0]), bits(world_pts)) and np.array_equal(bits(again[1]), bits(down))
    assert again[2] == info and info["n"] == len(world_pts) and info["n_down"] == len(down)
    v = fr.voxel_grid(world_pts, leaf)
    assert info["down_filtered"] == int(v.filtered)
    frac = fc.check_voxels(down, world_pts, leaf, fc.device_adds)  # set, order and count; the summation bound
    dref = oracle.voxel_grid(world_pts, leaf)
    assert down.shape == dref.shape and _close(down, dref)
    print(f"FRAC pg_down n={len(world_pts)} leaf={leaf} voxels={len(down)} {frac:.4f}")
    return world_pts, down, info


VOXEL_CASES = [("one_voxel", 1), ("one_voxel", 65), ("one_per_voxel", 257), ("lattice", 0.2), ("negative", 3000)]


@pytest.mark.parametrize("case", VOXEL_CASES, ids=fc.case_id)
def test_pg_down_constructed(ictx, case):
    """frontend_cases' clouds as the full-resolution frame, published at the identity: one point, 65 points in one
    voxel, one point per voxel, the lattice on the leaf boundaries either side of 0 on every axis (with -0.0), a
    frame near -1000 m.  All five columns: the tags ride in column 3, column 4 is the fresh point's 0."""
    raw, leaf = fc.voxel_frame(case)
    sid, und, _ = ictx.scan_preprocess(raw, leaf_size=0.0)
    try:
        assert np.array_equal(bits(und), bits(raw))
        world_pts, down, info = check_down(ictx, ident(), -1, leaf)
    finally:
        ictx.scan_release(sid)
    assert np.array_equal(world_pts[:, :4], raw[:, :4]) and not np.any(world_pts[:, 4])
    want = {"one_voxel": 1, "one_per_voxel": len(raw)}.get(case[0])
    assert want is None or len(down) == want
    if case[0] == "lattice":
        xyz = world_pts[:, :3]
        assert np.all(xyz.min(0) < 0) and np.all(xyz.max(0) > 0) and np.any(xyz == 0)


def test_pg_down_of_a_rotated_cloud(wctx, world0):  # noqa: F811
    """4,000 points on the wall and the board at a real state, as a resident scan (the caller's order)."""
    sc, A = world0["sc"], world0["A"]
    L = moved(A, [0.03, -0.02, 0.015], [0.2, -0.15, 0.1])
    sid = wctx.scan_upload(sc.cloud(L, 4000, 2))
    try:
        want = wctx.frame_to_world(L, sid)
        world_pts, down, info = check_down(wctx, L, sid, 0.2)
    finally:
        wctx.scan_release(sid)
    assert np.array_equal(bits(world_pts), bits(want)) and 100 < len(down) < 4000


def test_pg_down_leaf_too_small_keeps_input(ictx):
    from livo_amd import synth
    raw, _, _, _ = synth.make_raw_scan(1000, 5)
    raw[0, :3] = [-3000, -3000, -3000]
    raw[1, :3] = [3000, 3000, 3000]
    sid, _, _ = ictx.scan_preprocess(raw, leaf_size=0.0)
    try:
        info = ictx.cloud_publish(ident(), -1, match_leaf=0.01)
    finally:
        ictx.scan_release(sid)
    assert info["n"] == info["n_down"] == 1000 and info["down_filtered"] == 0
    world_pts = ictx.frame_to_world(ident(), WORLD)
    assert np.array_equal(world_pts[:, :4], raw[:, :4])
    assert np.array_equal(bits(ictx.frame_to_world(ident(), DOWN)), bits(world_pts))


def test_no_pg_down_without_a_leaf(ictx):
    import livo_amd
    raw, _ = fc.voxel_frame(("one_per_voxel", 257))
    sid, _, _ = ictx.scan_preprocess(raw, leaf_size=0.0)
    try:
        ictx.cloud_publish(ident(), -1, match_leaf=0.2)
        assert ictx.cloud_info()["n_down"] == 257
        for leaf in (0.0, -1.0):
            info = ictx.cloud_publish(ident(), -1, match_leaf=leaf)
            assert info["n"] == 257 and info["n_down"] == -1 and info["down_filtered"] == 0
            with pytest.raises(livo_amd.LivoError) as e:
                ictx.frame_to_world(ident(), DOWN)
            assert e.value.code == NOSCAN
            assert len(ictx.frame_to_world(ident(), WORLD)) == 257
    finally:
        ictx.scan_release(sid)


# ------------------------------------------------ 4. same state, same answer ----
def seeded_pair(world_fx):
    """Two contexts with the same one-frame visual map: livo_vio_select's points of frame A."""
    cam, A, sc, imgA = (world_fx[k] for k in ("cam", "A", "sc", "imgA"))
    pair, vp = (new_ctx(), new_ctx()), vio_params(cam)
    for c in pair:
        c.vmap_reset(1200, 8, PS)
        sid = c.scan_upload(sc.cloud(A, 4000, 1))
        pts, pat, _ = c.vio_select(A, imgA, vp, GRID, sid)
        c.scan_release(sid)
        c.vmap_add_frame(0, A, vp, imgA)
        c.vmap_add(0, pts, pat)
    assert_same_map(*pair)
    return pair, vp


def match_bytes(m):
    return [m["records"].tobytes(), m["pos"].tobytes(), m["levels"].tobytes(), m["patches"].tobytes(), repr(m["stats"])]


def test_same_state_same_answer(built, world0):  # noqa: F811
    """With the camera at the publish's state and no pg_down, every stage on LIVO_CLOUD_WORLD gives the bytes of
    the same call on the source scan (twin contexts: match and detect rewrite the map)."""
    cam, A, sc, imgA = (world0[k] for k in ("cam", "A", "sc", "imgA"))
    (a, b), vp = seeded_pair(world0)
    try:
        L = moved(A, [0.03, -0.02, 0.015], [0.2, -0.15, 0.1])
        img, body = sc.render(L), sc.cloud(L, 4000, 2)
        sa, sb = a.scan_upload(body), b.scan_upload(body)
        info = b.cloud_publish(L, sb, match_leaf=0.0)
        b.scan_release(sb)
        assert info["n"] == 4000 and info["n_down"] == -1
        pa, ia, ca = a.colorize(L, gray3(img), vp, sa)
        pb, ib, cb = b.colorize(L, gray3(img), vp, WORLD)
        assert pa.tobytes() == pb.tobytes() and ia.tobytes() == ib.tobytes() and ca == cb and ca["n_out"] >= 20
        qa, ta, za = a.vio_select(L, img, vp, GRID, sa)
        qb, tb, zb = b.vio_select(L, img, vp, GRID, WORLD)
        assert qa.tobytes() == qb.tobytes() and ta.tobytes() == tb.tobytes() and za == zb and za["n_out"] >= 20
        ma = a.vio_match(L, img, vp, GRID, scan_id=sa)
        mb = b.vio_match(L, img, vp, GRID, scan_id=WORLD)
        assert match_bytes(ma) == match_bytes(mb) and ma["stats"]["n_out"] >= 20
        assert_same_map(a, b)
        st_a, stats_a = a.vio_detect(1, L, img, vp, GRID, scan_id=sa)
        st_b, stats_b = b.vio_detect(1, L, img, vp, GRID, scan_id=WORLD)
        a.scan_release(sa)
        assert stats_a == stats_b and state_bytes(st_a) == state_bytes(st_b)
        assert stats_a["n_matched"] >= 20 and stats_a["n_new"] > 0 and stats_a["update"]["n_meas"] > 0
        assert_same_map(a, b)
    finally:
        a.close()
        b.close()


# --------------------------------------------------------- 5. different states ----
def test_camera_state_differs_from_the_clouds(wctx, world0):  # noqa: F811
    """The cloud is published at the LIO state L; the image is taken at C, a few cm and tenths of a degree on.
    Every stage equals its restatement fed the cloud at L and the pose of C."""
    cam, A, sc, imgA = (world0[k] for k in ("cam", "A", "sc", "imgA"))
    rig = Rig(wctx, cam)
    sid = wctx.scan_upload(sc.cloud(A, 4000, 1))
    pts, pat, _ = wctx.vio_select(A, imgA, rig.vp, GRID, sid)
    wctx.scan_release(sid)
    rig.add_frame(0, A, imgA)
    rig.add(0, pts, pat)
    L = moved(A, [0.03, -0.02, 0.015], [0.2, -0.15, 0.1])
    Cs = moved(L, [0.04, 0.03, -0.02], [0.3, -0.2, 0.25])
    imgC = sc.render(Cs)
    sid = wctx.scan_upload(sc.cloud(L, 4000, 2))
    world_L = wctx.frame_to_world(L, sid)
    at_C = wctx.frame_to_world(Cs, sid)
    wctx.cloud_publish(L, sid, match_leaf=0.0)
    wctx.scan_release(sid)
    assert not np.array_equal(bits(world_L), bits(at_C))  # the two states place the cloud differently
    xyz, (Rcw, Pcw) = world_L[:, :3], rig.pose(Cs)
    # livo_vio_match, as Rig.match_equal
    dev = wctx.vio_match(Cs, imgC, rig.vp, GRID, scan_id=WORLD)
    rec, pos, lev, mpat, stats, info = rig.model.match(xyz, Rcw, Pcw, imgC, GRID, False, 0.0, 100.0, quirk=True)
    print(stats)
    assert dev["stats"] == stats and dev["records"].tobytes() == rec.tobytes()
    assert dev["pos"].tobytes() == pos.tobytes() and np.array_equal(dev["levels"], lev)
    assert dev["patches"].shape == mpat.shape and np.array_equal(bits(dev["patches"]), bits(mpat))
    rig.check_dump()
    assert stats["n_out"] >= 20 and stats["n_in"] == 4000
    # livo_vio_select
    got, gpat, gstats = wctx.vio_select(Cs, imgC, rig.vp, GRID, WORLD)
    want, wpat, wstats, _ = restate_select(xyz, cam, Rcw, Pcw, imgC, PS, GRID)
    assert gstats == wstats and got.tobytes() == want.tobytes()
    assert gpat.shape == wpat.shape and np.array_equal(bits(gpat), bits(wpat)) and len(got) >= 20
    # livo_cloud_colorize
    bgr = gray3(imgC)
    cpts, idx, cstats = wctx.colorize(Cs, bgr, rig.vp, WORLD)
    fate, rgb, edge = restate_colorize(xyz, cam, Rcw, Pcw, bgr)
    keep = np.flatnonzero(fate == KEPT)
    assert np.array_equal(idx, keep) and cstats == restate_stats(fate, edge) and len(keep) >= 20
    assert np.array_equal(np.stack([cpts["r"], cpts["g"], cpts["b"]], axis=1), rgb[keep])
    assert np.array_equal(bits(np.stack([cpts["x"], cpts["y"], cpts["z"]], axis=1)), bits(xyz[idx]))


# ------------------------------------------------------ 6. detect reads pg_down ----
def chain_ids(ctx, vp, fid, st, img):
    """livo_vio_detect(LIVO_CLOUD_WORLD)'s definition: the six public calls with the two ids."""
    m = ctx.vio_match(st, img, vp, GRID, scan_id=DOWN)
    pts, pat, sstats = ctx.vio_select(st, img, vp, GRID, WORLD)
    st1, ustats, _ = ctx.vio_update(dict(m, image=img), st, max_iter=vp.max_iterations, img_point_cov=vp.img_point_cov)
    ctx.vmap_add_frame(fid, st1, vp, img)
    rec, ostats = ctx.vio_observe(fid, m["records"]["point_id"], m["records"]["search_level"])
    first = ctx.vmap_info()["n_points"]
    ctx.vmap_add(fid, pts, pat)
    stats = {"match": m["stats"], "select": sstats, "update": ustats, "observe": ostats, "n_matched": len(rec),
             "n_new": len(pts), "first_new_id": first if len(pts) else -1}
    return st1, stats


def test_detect_matches_on_pg_down_and_selects_on_the_full_cloud(built, world):  # noqa: F811
    """Three frames of a closed loop on twin contexts: each LiDAR frame is published at its LIO state with leaf
    0.2, the camera frame follows a few cm later."""
    cam, A, sc, imgA = unpack(world)
    one, chain, vp = new_ctx(), new_ctx(), vio_params(cam)
    try:
        for c in (one, chain):
            c.vmap_reset(1200, 8, PS)
        matched = []
        for k in range(3):
            L = side(sc, A, 0.3 * k)
            Cs = moved(L, [0.02, -0.015, 0.01], [0.15, 0.1, -0.1])
            img, body = sc.render(Cs), sc.cloud(L, 4000, 10 + k)
            infos = []
            for c in (one, chain):
                sid = c.scan_upload(body)
                infos.append(c.cloud_publish(L, sid, match_leaf=0.2))
                c.scan_release(sid)
            info = infos[0]
            assert infos[1] == info and info["n"] == 4000 and 0 < info["n_down"] < 4000 and info["down_filtered"] == 1
            want_state, want = chain_ids(chain, vp, k, Cs, img)
            got_state, got = one.vio_detect(k, Cs, img, vp, GRID, scan_id=WORLD)
            print(k, info, {f: v for f, v in want.items() if f.startswith("n_")})
            assert got == want and state_bytes(got_state) == state_bytes(want_state)
            assert_same_map(chain, one)
            assert got["match"]["n_in"] == info["n_down"] and got["select"]["n_in"] == info["n"]
            matched.append(got["n_matched"])
        assert matched[0] == 0 and min(matched[1:]) >= 5
        # LIVO_CLOUD_WORLD_DOWN: pg_down for both stages
        L = side(sc, A, 0.9)
        st, got = one.vio_detect(3, L, sc.render(L), vp, GRID, scan_id=DOWN)
        assert got["match"]["n_in"] == got["select"]["n_in"] == info["n_down"]
    finally:
        one.close()
        chain.close()


# ------------------------------------------------------------------ 7. errors ----
def test_errors(built, world):  # noqa: F811
    import livo_amd
    from livo_amd import synth
    cam, A, sc, imgA = unpack(world)
    ctx, vp = new_ctx(), vio_params(cam)
    try:
        L = ctx._L
        ctx.vmap_reset(400, 4, PS)
        ctx.map_build(synth.make_map(20_000))
        s, n, info = livo_amd.state_to_c(A), C.c_int64(-7), livo_amd.CloudInfo()

        def stages(sid):
            d, vs = livo_amd.VdetectParams(GRID, 0, 0.0, 100.0), livo_amd.VdetectStats()
            return [L.livo_frame_to_world(ctx.h, sid, C.byref(s), None, 0, C.byref(n)),
                    L.livo_cloud_colorize(ctx.h, sid, C.byref(s), C.byref(vp), livo_amd._ptr(gray3(imgA)), 160, 128,
                                          None, None, 0, C.byref(n), None),
                    L.livo_vio_select(ctx.h, sid, C.byref(s), C.byref(vp), GRID, livo_amd._ptr(imgA), 160, 128, None,
                                      None, 0, C.byref(n), None),
                    L.livo_vio_match(ctx.h, sid, C.byref(s), C.byref(vp), GRID, 0, 0.0, 100.0, livo_amd._ptr(imgA), 160,
                                     128, None, None, None, None, 0, C.byref(n), None),
                    L.livo_vio_detect(ctx.h, sid, 0, C.byref(s), None, C.byref(vp), C.byref(d), livo_amd._ptr(imgA),
                                      160, 128, C.byref(vs))]

        # before any publish
        assert L.livo_cloud_info_get(ctx.h, C.byref(info)) == NOSCAN
        for sid in (WORLD, DOWN):
            assert stages(sid) == [NOSCAN] * 5
        assert ctx.vmap_info()["n_frames"] == 0
        # refused sources and arguments
        body = sc.cloud(A, 300, 1)
        src = ctx.scan_upload(body)
        assert raw_publish(ctx, WORLD, A)[0] == INVALID and raw_publish(ctx, DOWN, A)[0] == INVALID
        assert raw_publish(ctx, src, A, float("nan"))[0] == INVALID and raw_publish(ctx, src, A, float("inf"))[0] == INVALID
        assert raw_publish(ctx, src, None)[0] == INVALID and raw_publish(ctx, 77, A)[0] == NOSCAN
        assert L.livo_cloud_info_get(ctx.h, C.byref(info)) == NOSCAN
        assert L.livo_frame_to_world(ctx.h, WORLD, None, None, 0, C.byref(n)) == INVALID  # state: ignored, required
        # a published cloud is no scan to any other entry point
        ctx.cloud_publish(A, src, match_leaf=0.2)
        stats, hth, htl = livo_amd.IterStats(), np.zeros(81, F64), np.zeros(9, F64)
        cnt, idx, d2 = C.c_int64(), np.zeros((300, 5), np.int32), np.zeros((300, 5), F32)
        for sid in (WORLD, DOWN):
            assert L.livo_iekf_update(ctx.h, sid, C.byref(s), None, C.byref(stats)) == NOSCAN
            assert L.livo_h_share(ctx.h, sid, C.byref(s), 1, livo_amd._ptr(hth), livo_amd._ptr(htl), C.byref(cnt),
                                  None) == NOSCAN
            assert L.livo_scan_release(ctx.h, sid) == NOSCAN
            assert L.livo_map_incremental(ctx.h, sid, C.byref(s), 0.5, 1, None, None) == NOSCAN
            assert L.livo_scan_neighbors(ctx.h, sid, livo_amd._ptr(idx), livo_amd._ptr(d2)) == NOSCAN
        assert ctx.cloud_info()["n"] == 300 and len(ctx.frame_to_world(A, WORLD)) == 300
        # an empty source: an empty cloud, and the stages' answers for an empty scan
        empty = ctx.scan_upload(np.zeros((0, 3), F32))
        want = stages(empty)
        got_n = []
        for leaf, n_down in ((0.2, 0), (0.0, -1)):
            info2 = ctx.cloud_publish(A, empty, match_leaf=leaf)
            assert info2["n"] == 0 and info2["n_down"] == n_down and info2["down_filtered"] == 0
            assert ctx.frame_to_world(A, WORLD).shape == (0, 5)
            pts, idx2, cs = ctx.colorize(A, gray3(imgA), vp, WORLD)
            sel, pat, ss = ctx.vio_select(A, imgA, vp, GRID, WORLD)
            got_n.append((len(pts), cs["n_in"], len(sel), ss["n_in"]))
        assert got_n == [(0, 0, 0, 0)] * 2 and want[:3] == [0, 0, 0]
        ctx.scan_release(empty)
        ctx.scan_release(src)
    finally:
        ctx.close()
