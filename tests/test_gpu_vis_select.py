"""GPU parity of livo_vio_select (LidarSelector::addSparseMap, src/lidar_selection.cpp:140-193)
against the numpy restatement of tests/test_vis_select_abi.py applied to livo_frame_to_world's
float x, y, z.

Bars: everything exact.  The records (every field, as bytes), the patches (as uint32), their order
and every statistic equal the restatement; two calls give the same bytes.  The frames and what each
can show are listed in test_vis_select_abi.py; the clouds are resident scans of 0, 1, 63, 257 and
3,000 points (20,000 on the 640 x 512 frame), and the cases of 3,000 points and more must show,
in the restatement on the device's points, the ties, behind-camera winners, empty and occupied
cells and the overflow they are built for (case_worth).
"""
import ctypes as C

import numpy as np
import pytest
from test_vis_select_abi import (BIG_N, FRAMES, SIZES, case_worth, frame_case, frame_image, restate_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sctx(built):
    import livo_amd
    from livo_amd import synth
    ctx = livo_amd.Context(0, t_LI=synth.T_LI)
    yield ctx
    ctx.close()


def _params(name):
    import livo_amd
    img, cam, Rci, Pci = frame_image(name)
    vp = livo_amd.vio_params(cam, Rci, Pci)
    vp.patch_size = FRAMES[name][2]
    return img, vp, FRAMES[name][3]


def _check_parity(ctx, name, n):
    st, body = frame_case(name, n)
    img, vp, grid = _params(name)
    sid = ctx.scan_upload(body)
    try:
        world = ctx.frame_to_world(st, sid)
        pts, pat, stats = ctx.vio_select(st, img, vp, grid, sid)
    finally:
        ctx.scan_release(sid)
    assert len(world) == n
    rec, want_pat, want_stats, info = restate_case(name, world[:, :3], st)
    print(name, n, stats, info)
    assert stats == want_stats
    assert np.array_equal(pts["cell"], rec["cell"]) and np.array_equal(pts["src_index"], rec["src_index"])
    assert pts.tobytes() == rec.tobytes()
    assert pat.shape == want_pat.shape and np.array_equal(pat.view(np.uint32), want_pat.view(np.uint32))
    case_worth(name, n, want_stats, info)
    return pts, pat, stats


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", [k for k in FRAMES if k != "640x512-g40"])
def test_parity_small_frames(sctx, name, n):
    _check_parity(sctx, name, n)


def test_parity_distorted_frame(sctx):
    pts, _, stats = _check_parity(sctx, "640x512-g40", BIG_N)
    assert stats["n_cells"] == 192 and len(pts) > 96


def _raw_call(ctx, st, vp, grid, img, sid, out, pat, cap, stats=None):
    import livo_amd
    n = C.c_int64(-7)
    s = livo_amd.state_to_c(st)
    rc = ctx._L.livo_vio_select(ctx.h, sid, C.byref(s), C.byref(vp), grid, livo_amd._ptr(img), vp.cam.width,
                                vp.cam.height, livo_amd._ptr(out), livo_amd._ptr(pat), cap, C.byref(n),
                                C.byref(stats) if stats is not None else None)
    return rc, n.value


def test_determinism_and_image_reuse(sctx):
    name = "160x152-g40"
    st, body = frame_case(name, 3000)
    img, vp, grid = _params(name)
    sid = sctx.scan_upload(body)
    try:
        a = sctx.vio_select(st, img, vp, grid, sid)
        b = sctx.vio_select(st, img, vp, grid, sid)
        c = sctx.vio_select(st, None, vp, grid, sid)  # the uploaded image again
        assert len(a[0]) > 0
        for other in (b, c):
            assert a[0].tobytes() == other[0].tobytes() and a[1].tobytes() == other[1].tobytes() and a[2] == other[2]
        # another image in between, then the first one again
        other_img, other_vp, other_grid = _params("160x128-g20")
        sctx.vio_select(st, other_img, other_vp, other_grid, sid)
        assert _raw_call(sctx, st, vp, grid, None, sid, None, None, 0)[0] == -1  # the resident image is 160 x 128
        d = sctx.vio_select(st, img, vp, grid, sid)
        assert a[0].tobytes() == d[0].tobytes() and a[1].tobytes() == d[1].tobytes()
    finally:
        sctx.scan_release(sid)


def test_contract(built):
    import livo_amd
    from livo_amd import synth
    name = "160x128-g20"
    st, body = frame_case(name, 3000)
    img, vp, grid = _params(name)
    with livo_amd.Context(0, t_LI=synth.T_LI) as ctx:
        # a fresh context: no frame (*n = 0), no image to reuse, unknown scan ids
        assert _raw_call(ctx, st, vp, grid, img, -1, None, None, 0) == (0, 0)
        with livo_amd.Context(0, t_LI=synth.T_LI) as fresh:
            assert _raw_call(fresh, st, vp, grid, None, -1, None, None, 0)[0] == -1  # LIVO_E_INVALID
        assert _raw_call(ctx, st, vp, grid, img, 5, None, None, 0)[0] == -4  # LIVO_E_NOSCAN
        sid = ctx.scan_upload(body)
        pts, pat, stats = ctx.vio_select(st, img, vp, grid, sid)
        k = len(pts)
        assert 2 < k < stats["n_cells"]
        vs = livo_amd.VisStats()
        assert _raw_call(ctx, st, vp, grid, img, sid, None, None, 0, vs) == (0, k)  # the sizing call
        assert vs.n_out == k and vs.n_in == 3000 and vs.n_cells == stats["n_cells"]
        # cap = n_out - 1: LIVO_E_CAPACITY, *n set, the buffers untouched
        cells = stats["n_cells"]
        out = np.full(cells * 64, 0xA5, np.uint8).view(livo_amd.VIS_POINT_DTYPE)
        buf = np.full((cells, 48), -12345.0, np.float32)
        assert _raw_call(ctx, st, vp, grid, img, sid, out, buf, k - 1) == (-7, k)
        assert _raw_call(ctx, st, vp, grid, img, sid, out, buf, 0) == (-7, k)
        assert np.all(out.view(np.uint8) == 0xA5) and np.all(buf == -12345.0)
        # out without patches, a negative cap, cap without out: LIVO_E_INVALID
        assert _raw_call(ctx, st, vp, grid, img, sid, out, None, cells)[0] == -1
        assert _raw_call(ctx, st, vp, grid, img, sid, out, buf, -1)[0] == -1
        assert _raw_call(ctx, st, vp, grid, img, sid, None, None, 5)[0] == -1
        # cap = n_out is enough; nothing past the result is written
        assert _raw_call(ctx, st, vp, grid, None, sid, out, buf, k) == (0, k)
        assert out[:k].tobytes() == pts.tobytes() and np.array_equal(buf[:k], pat)
        assert np.all(out[k:].view(np.uint8) == 0xA5) and np.all(buf[k:] == -12345.0)
        ctx.scan_release(sid)
        assert _raw_call(ctx, st, vp, grid, img, sid, None, None, 0)[0] == -4


def test_selected_points_drive_the_photometric_update(built):
    """End to end on a make_vio_frame image and pose: points selected from a cloud at the true state, then
    livo_vio_update from make_state's perturbed state with the selected positions, level 0 and patches."""
    import livo_amd
    import oracle
    from livo_amd import synth
    fr, st, truth = synth.make_vio_frame(3000, 0)
    vp = livo_amd.vio_params(fr["cam"], fr["Rci"], fr["Pci"])
    vp.patch_size = fr["patch_size"]
    # the frame's visual points as a LiDAR cloud: body = R^T (p_w - p) - t_LI at the true pose (R_LI = I)
    body = ((fr["pos"] - truth["pos"]) @ truth["rot"] - synth.T_LI).astype(np.float32)
    with livo_amd.Context(0, t_LI=synth.T_LI) as ctx:
        sid = ctx.scan_upload(body)
        pts, pat, stats = ctx.vio_select(truth, fr["image"], vp, 20, sid)
        assert stats["n_out"] == len(pts) > 100
        sel = dict(fr)
        sel["pos"] = np.stack([pts["x"], pts["y"], pts["z"]], axis=1).astype(np.float64)
        sel["levels"] = np.zeros(len(pts), np.int32)
        sel["patches"] = pat
        g = ctx.vio_update(sel, st)
    r = oracle.vio_update(sel, st)
    gs, gst, gerr = g
    rs, rst, rerr = r
    assert gst["iterations"] == rst["iterations"] and gst["updates"] == rst["updates"]
    assert gst["cov_updated"] == rst["cov_updated"] and gst["n_meas"] == rst["n_meas"]
    assert np.array_equal(np.float32(gst["last_error"]), np.float32(rst["last_error"]))
    assert np.array_equal(gerr.view(np.uint32), rerr.view(np.uint32))
    assert np.abs(gs["pos"] - rs["pos"]).max() < 1e-9
    assert np.abs(gs["rot"] - rs["rot"]).max() < 1e-9
    assert np.abs(gs["cov"] - rs["cov"]).max() < 1e-12
    e0, e1 = np.linalg.norm(st["pos"] - truth["pos"]), np.linalg.norm(gs["pos"] - truth["pos"])
    print("position error", e0, "->", e1)
    assert e1 < 0.2 * e0
