"""GPU parity of livo_cloud_colorize (LaserMapping::publish_frame_world_rgb,
src/laser_mapping.cpp:1351-1381) against the numpy restatement of tests/test_rgb_cloud_abi.py
applied to livo_frame_to_world's float x, y, z.

Bars: everything exact.  The kept set, its order, r, g, b and every statistic equal the
restatement; x, y, z equal livo_frame_to_world's bit for bit; two calls give the same bytes.
Cloud sizes 1, 63, 64, 65, 257 and 5,000 cross the wave (64) and block (256) boundaries of the
compaction; the cameras are aimed so that a good part of the cloud is kept and the rest dropped
(checked below for the frames of 63 points and more).
"""
import ctypes as C

import numpy as np
import pytest
from test_rgb_cloud_abi import (BEHIND, CAM_DIST, CAM_PLAIN, H, KEPT, OUT_OF_FRAME, W, edge_points, random_image,
                                restate_colorize, restate_pose, restate_stats)

pytestmark = pytest.mark.gpu


def _yawed(deg):
    from livo_amd import synth
    return synth.R_CI @ synth.so3_exp(np.array([0.0, 0.0, -np.radians(deg)]))


def _cameras():
    """name -> (cam, Rci, Pci).  The LiDAR looks along +x of the IMU with a 70 x 77 degree field of view.
    half: a narrow camera yawed by 30 degrees sees about half of it, the rest is out of frame; wide: a wide
    one yawed by 65 degrees has a part of it behind; away: all of it behind; all: every point in frame."""
    from livo_amd import synth
    return {"half": (dict(CAM_DIST, fx=48.0 * 1.03, fy=48.0 * 0.99), _yawed(30.0), synth.P_CI),
            "wide": (dict(CAM_DIST, fx=14.0 * 1.03, fy=14.0 * 0.99), _yawed(65.0), synth.P_CI),
            "away": (CAM_DIST, _yawed(180.0), synth.P_CI),
            "all": (dict(CAM_PLAIN, fx=12.0, fy=12.0), synth.R_CI, synth.P_CI)}


@pytest.fixture(scope="module")
def rctx(built):
    import livo_amd
    from livo_amd import synth
    ctx = livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=4)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def image():
    return random_image()


def _xyz_bits(pts):
    return np.stack([pts["x"], pts["y"], pts["z"]], axis=1).view(np.uint32)


def _check_parity(ctx, st, camera, img, sid):
    """colorize against the restatement on frame_to_world's points; returns the restatement's fates."""
    import livo_amd
    cam, Rci, Pci = camera
    vp = livo_amd.vio_params(cam, Rci, Pci)
    world = ctx.frame_to_world(st, sid)
    pts, idx, stats = ctx.colorize(st, img, vp, sid)
    Rcw, Pcw = restate_pose(Rci, Pci, st["rot"], st["pos"])
    fate, rgb, edge = restate_colorize(world[:, :3], cam, Rcw, Pcw, img)
    want = np.flatnonzero(fate == KEPT)
    assert np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, want)
    assert np.array_equal(np.stack([pts["r"], pts["g"], pts["b"]], axis=1), rgb[want])
    assert np.all(pts["a"] == 255)
    assert stats == restate_stats(fate, edge)
    assert np.array_equal(_xyz_bits(pts), np.ascontiguousarray(world[idx, :3]).view(np.uint32))
    return fate


@pytest.mark.parametrize("camera", ["half", "wide"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_parity_frame_and_resident_scan(rctx, image, n, camera):
    from livo_amd import synth
    raw, poses, Re, pe = synth.make_raw_scan(n, n % 7)
    sid, _, down = rctx.scan_preprocess(raw, poses, Re, pe, leaf_size=0.5)
    try:
        st = synth.make_state(n % 7)
        cam = _cameras()[camera]
        fate = _check_parity(rctx, st, cam, image, -1)  # the full-resolution frame
        assert len(fate) == n
        if n >= 63:
            assert 0.2 < np.mean(fate == KEPT) < 0.8
            assert np.sum(fate == OUT_OF_FRAME) > 0
        if camera == "wide" and n >= 63:
            assert np.sum(fate == BEHIND) > 0
        fate_d = _check_parity(rctx, st, cam, image, sid)  # the resident scan, caller's order
        assert len(fate_d) == len(down)
    finally:
        rctx.scan_release(sid)


def test_edges(built, image):
    """The constructed edge points as a resident scan under the identity state and extrinsics (world =
    body = camera): flat-offset wraps, last-row and row -1 points kept with 0 taps, NaN / inf / z <= 0."""
    import livo_amd
    from livo_amd import synth
    pts = edge_points()
    st = synth.make_state(0)
    st["rot"], st["pos"] = np.eye(3), np.zeros(3)
    with livo_amd.Context(0) as ctx:  # R_LI = I, t_LI = 0
        sid = ctx.scan_upload(pts)
        world = ctx.frame_to_world(st, sid)
        finite = np.isfinite(pts).all(axis=1)
        assert np.array_equal(world[finite, :3], pts[finite])  # (as values: the transform turns -0 into +0)
        fate = _check_parity(ctx, st, (CAM_PLAIN, np.eye(3), np.zeros(3)), image, sid)
        out, idx, stats = ctx.colorize(st, None, livo_amd.vio_params(CAM_PLAIN, np.eye(3), np.zeros(3)), sid)
    rgb = np.stack([out["r"], out["g"], out["b"]], axis=1)
    at = {int(i): k for k, i in enumerate(idx)}
    half = np.float32(0.5)
    bgr = lambda r, c: image[r, c].astype(np.float32)  # noqa: E731
    trunc = lambda v: (v.astype(np.int32) & 255)[::-1]  # noqa: E731
    # u = -0.5 and u = width - 0.5 at v = 10: the neighbouring row's pixel
    assert np.array_equal(rgb[at[5]], trunc(half * bgr(9, 63) + half * bgr(10, 0)))
    assert np.array_equal(rgb[at[7]], trunc(half * bgr(10, 63) + half * bgr(11, 0)))
    # v = height - 0.5: kept, the lower taps read 0
    assert np.array_equal(rgb[at[9]], trunc(half * bgr(47, 10)))
    assert 9 in at and 10 in at and 11 in at and 12 in at and 13 in at
    # (_check_parity held every statistic against the restatement; here: the cases are all present.  The
    # identity body -> world transform turns the point with z = inf into NaNs, 0 * inf: it counts as behind)
    assert stats["edge_reads"] >= 8 and stats["behind"] >= 9 and stats["out_of_frame"] >= 5
    assert stats["n_in"] == len(pts) and stats["n_out"] == int(np.sum(fate == KEPT))


def test_all_dropped_and_all_kept(rctx, image):
    import livo_amd
    from livo_amd import synth
    raw, poses, Re, pe = synth.make_raw_scan(700, 2)
    sid, _, _ = rctx.scan_preprocess(raw, poses, Re, pe, leaf_size=0.5)
    try:
        st = synth.make_state(2)
        cams = _cameras()
        fate = _check_parity(rctx, st, cams["away"], image, -1)
        assert np.all(fate == BEHIND)
        pts, idx, stats = rctx.colorize(st, image, livo_amd.vio_params(*cams["away"]), -1)
        assert len(pts) == 0 and len(idx) == 0 and stats["n_out"] == 0 and stats["behind"] == 700
        fate = _check_parity(rctx, st, cams["all"], image, -1)
        assert np.all(fate == KEPT)
        pts, idx, stats = rctx.colorize(st, image, livo_amd.vio_params(*cams["all"]), -1)
        assert stats["n_out"] == stats["n_in"] == 700 and np.array_equal(idx, np.arange(700))
    finally:
        rctx.scan_release(sid)


def _raw_call(ctx, st, vp, img, sid, out, idx, cap, stats=None, w=W, h=H):
    import livo_amd
    n = C.c_int64(-7)
    s = livo_amd.state_to_c(st)
    rc = ctx._L.livo_cloud_colorize(ctx.h, sid, C.byref(s), C.byref(vp), livo_amd._ptr(img), w, h,
                                    livo_amd._ptr(out), livo_amd._ptr(idx), cap, C.byref(n),
                                    C.byref(stats) if stats is not None else None)
    return rc, n.value


def test_contract(built, image):
    import livo_amd
    from livo_amd import synth
    cam, Rci, Pci = _cameras()["half"]
    vp = livo_amd.vio_params(cam, Rci, Pci)
    st = synth.make_state(3)
    with livo_amd.Context(0, t_LI=synth.T_LI) as ctx:
        # a fresh context: no frame (*n = 0), no image to reuse, unknown scan ids
        assert _raw_call(ctx, st, vp, image, -1, None, None, 0) == (0, 0)
        with livo_amd.Context(0, t_LI=synth.T_LI) as fresh:
            assert _raw_call(fresh, st, vp, None, -1, None, None, 0)[0] == -1  # LIVO_E_INVALID
        assert _raw_call(ctx, st, vp, image, 5, None, None, 0)[0] == -4  # LIVO_E_NOSCAN
        raw, poses, Re, pe = synth.make_raw_scan(1500, 3)
        sid, _, down = ctx.scan_preprocess(raw, poses, Re, pe, leaf_size=0.5)
        pts, idx, stats = ctx.colorize(st, image, vp, -1)
        k = len(pts)
        assert 2 < k < 1500
        # a count-only call gives the same *n
        assert _raw_call(ctx, st, vp, image, -1, None, None, 0) == (0, k)
        # cap = n_out - 1: LIVO_E_RANGE, *n set, the buffers untouched
        out = np.full(1500, 0xA5, np.uint8).repeat(16).view(livo_amd.RGB_POINT_DTYPE)
        ind = np.full(1500, -12345, np.int32)
        rs = livo_amd.RgbStats()
        assert _raw_call(ctx, st, vp, image, -1, out, ind, k - 1, rs) == (-6, k)
        assert np.all(out.view(np.uint8) == 0xA5) and np.all(ind == -12345)
        assert _raw_call(ctx, st, vp, image, -1, out, None, k - 1) == (-6, k)
        assert _raw_call(ctx, st, vp, image, -1, None, ind, k - 1) == (-6, k)
        assert np.all(out.view(np.uint8) == 0xA5) and np.all(ind == -12345)
        # cap = n_out is enough, and either output alone is filled
        assert _raw_call(ctx, st, vp, image, -1, out, None, k) == (0, k)
        assert _raw_call(ctx, st, vp, image, -1, None, ind, k) == (0, k)
        assert np.array_equal(out[:k], pts) and np.array_equal(ind[:k], idx)
        assert np.all(out[k:].view(np.uint8) == 0xA5) and np.all(ind[k:] == -12345)
        # image = None reuses the uploaded image: the frame, then the downsampled scan with one upload
        p2, i2, s2 = ctx.colorize(st, None, vp, -1)
        assert np.array_equal(p2, pts) and np.array_equal(i2, idx) and s2 == stats
        pd, idd, sd = ctx.colorize(st, image, vp, sid)
        pd2, idd2, sd2 = ctx.colorize(st, None, vp, sid)
        assert np.array_equal(pd, pd2) and np.array_equal(idd, idd2) and sd == sd2 and sd["n_in"] == len(down)
        # a size that differs from cam.width / height, with and without an image
        small = np.ascontiguousarray(image[:H - 1])
        assert _raw_call(ctx, st, vp, small, -1, None, None, 0, h=H - 1)[0] == -1
        assert _raw_call(ctx, st, vp, None, -1, None, None, 0, h=H - 1)[0] == -1
        vp2 = livo_amd.vio_params(dict(cam, height=H - 1), Rci, Pci)
        assert _raw_call(ctx, st, vp2, None, -1, None, None, 0, h=H - 1)[0] == -1  # the resident image is 64 x 48
        assert _raw_call(ctx, st, vp2, small, -1, None, None, 0, h=H - 1)[0] == 0
        assert _raw_call(ctx, st, vp, None, -1, None, None, 0)[0] == -1  # ... and now it is 64 x 47
        ctx.scan_release(sid)
        assert _raw_call(ctx, st, vp, image, sid, None, None, 0)[0] == -4


def test_determinism_and_isolation(rctx, image, map100k):
    """Two calls give byte-equal outputs, and the call leaves a resident scan's neighbour cache and a later
    update alone: livo_iekf_update of the scan gives the same state and statistics before and after."""
    import livo_amd
    from livo_amd import synth
    rctx.map_build(map100k)
    body, _, _ = synth.make_scan(3000, 1)
    sid = rctx.scan_upload(body)
    try:
        st = synth.make_state(1)
        vp = livo_amd.vio_params(*_cameras()["half"])
        s1, t1 = rctx.iekf_update(sid, st)
        i1, d1 = rctx.scan_neighbors(sid)
        a = rctx.colorize(st, image, vp, sid)
        b = rctx.colorize(st, image, vp, sid)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
        assert 0 < len(a[0]) < 3000
        i2, d2 = rctx.scan_neighbors(sid)
        assert np.array_equal(i1, i2) and np.array_equal(d1, d2)
        s2, t2 = rctx.iekf_update(sid, st)
        for key in ("rot", "pos", "vel", "bias_g", "bias_a", "gravity", "cov"):
            assert np.array_equal(s1[key], s2[key])
        assert t1["iterations"] == t2["iterations"] and t1["effct_feat_num"] == t2["effct_feat_num"]
        assert np.array_equal(t1["solution"], t2["solution"]) and t1["res_mean"] == t2["res_mean"]
    finally:
        rctx.scan_release(sid)


@pytest.mark.slow
def test_full_size_frame(rctx):
    """200k points, 1280 x 1024: the same parity, once."""
    from livo_amd import synth
    w, h = 1280, 1024
    img = random_image(w, h, seed=5)
    cam = dict(CAM_DIST, width=w, height=h, fx=960.0 * 1.03, fy=960.0 * 0.99, cx=631.2, cy=507.6)
    raw, _, _, _ = synth.make_raw_scan(200_000, 4)
    sid, _, _ = rctx.scan_preprocess(raw, leaf_size=0.5)
    try:
        fate = _check_parity(rctx, synth.make_state(4), (cam, _yawed(30.0), synth.P_CI), img, -1)
        assert len(fate) == 200_000 and 0.2 < np.mean(fate == KEPT) < 0.8
    finally:
        rctx.scan_release(sid)
