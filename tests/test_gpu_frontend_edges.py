"""The device scan front-end (livo_scan_preprocess, livo_frame_to_world) off its trivial points,
against the plain reference oracle/frontend_ref.py.  tests/test_gpu_frontend.py holds it to the
C++ oracle on synth.make_raw_scan alone (sorted times, no point on a segment boundary,
identity R_LI); here:

  * segment assignment on unsorted times (the suffix minimum, across many scan blocks), points
    exactly on, just below and just above a pose offset, zero-length segments, points later
    than the last pose, two poses, the first point's chain of 1 to 20 moves, n = 1;
  * Exp's small-angle branch either side of its 1e-7 threshold, and 0.6 rad;
  * all of that again under a 35-degree R_LI with a lever arm of decimetres, and
    livo_frame_to_world under it;
  * VoxelGrid membership on leaf boundaries (negative, -0.0, one float either side), voxels of
    1 to 5000 members, 3 to 1025 voxels, dx dy dz either side of INT32_MAX (31-bit sort keys),
    a frame near -1000 m, and the filter behind a real de-skew;
  * resident scans with a 300 m box (the 511 / extent Morton scale), of identical points and
    of one point, built by livo_scan_preprocess, livo_scan_upload and
    livo_scan_upload_batch_async: the same update and neighbours bit for bit.

Inputs, bars and their derivation (K = 192 float64 roundings; half a float32 ulp; the voxel
summation bound): tests/frontend_cases.py, shared with tests/test_frontend_reference.py, which
holds the CPU oracle to the same reference.  Each test prints its largest error as a fraction of
its bar.
"""
import numpy as np
import pytest

import frontend_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs(built):
    import livo_amd
    made = {ext: livo_amd.Context(0, R_LI=R, t_LI=t, max_iterations=4) for ext, (R, t) in fc.EXTRINSICS.items()}
    yield made
    for c in made.values():
        c.close()


def _preprocess(ctx, frame, leaf=0.0):
    sid, und, down = ctx.scan_preprocess(frame.raw, frame.poses, frame.rot_end, frame.pos_end, leaf_size=leaf)
    ctx.scan_release(sid)
    return und, down


@pytest.mark.parametrize("ext", ["ident", "tilt"])
@pytest.mark.parametrize("case", fc.DESKEW_CASES, ids=fc.case_id)
def test_deskew(ctxs, case, ext):
    frame = fc.deskew_frame(case, ext)
    ref0 = fc.deskew_reference(frame, ext)  # (rejects a frame that does not separate adjacent heads)
    und, down = _preprocess(ctxs[ext], frame)
    assert np.array_equal(down.view(np.uint32), und.view(np.uint32))  # leaf 0: no filter
    ref = fc.deskew_reference(frame, ext, und)
    frac = fc.check_deskew(und, frame, ref)
    exact = float(np.mean(und.view(np.uint32) == ref0.cloud.view(np.uint32)))
    print(f"FRAC deskew-{case[0]} {fc.case_id(case)}-{ext} {frac:.4f} bits-equal {exact:.6f}")


@pytest.mark.parametrize("n", [0, 1, 257, 30000])
def test_frame_to_world_extrinsics(ctxs, n):
    import oracle
    from livo_amd import synth
    ctx = ctxs["tilt"]
    R_LI, t_LI = fc.EXTRINSICS["tilt"]
    f = fc.deskew_frame(("segment", "random", 70001), "tilt")
    frame = fc.Frame(f.raw[:n], f.poses, f.rot_end, f.pos_end)
    st = synth.make_state(3)
    st["rot"] = fc.rot_axis_angle([3.0, -1.0, 2.0], 110.0)
    sid, und, down = ctx.scan_preprocess(frame.raw, frame.poses, frame.rot_end, frame.pos_end, leaf_size=0.5)
    try:
        assert down.shape[0] <= n and (n == 0 or down.shape[0] > 0)
        worst = 0.0
        for pts, got in ((und, ctx.frame_to_world(st)), (down[:, :3], ctx.frame_to_world(st, sid))):
            assert got.shape == (len(pts), 5)
            want = oracle.to_world(pts, st, R_LI=R_LI, t_LI=t_LI)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
            ref, bar = fc.to_world_bar(pts, st, "tilt", got)
            err = np.abs(got[:, :3].astype(np.float64) - ref)
            assert (err <= bar).all()
            worst = max(worst, float((err / bar).max()) if n else 0.0)
        print(f"FRAC to_world n={n} {worst:.4f}")
    finally:
        ctx.scan_release(sid)


@pytest.mark.parametrize("case", fc.VOXEL_CASES, ids=fc.case_id)
def test_voxel_grid(ctxs, case):
    raw, leaf = fc.voxel_frame(case)
    ctx = ctxs["ident"]
    sid, und, down = ctx.scan_preprocess(raw, leaf_size=leaf)
    ctx.scan_release(sid)
    assert np.array_equal(und.view(np.uint32), raw.view(np.uint32))
    frac = fc.check_voxels(down, raw, leaf, fc.device_adds)
    print(f"FRAC voxel {fc.case_id(case)} {frac:.4f}")


def test_voxel_grid_after_deskew(ctxs):
    """The filter behind a real de-skew: unsorted times, tilted extrinsics, leaf 0.2, against the
    reference's filter of the device's own de-skewed cloud."""
    frame = fc.deskew_frame(("segment", "random", 4097), "tilt")
    und, down = _preprocess(ctxs["tilt"], frame, leaf=0.2)
    fc.check_deskew(und, frame, fc.deskew_reference(frame, "tilt", und))
    frac = fc.check_voxels(down, und, 0.2, fc.device_adds, tags=False)
    print(f"FRAC voxel after-deskew {frac:.4f}")


def _resident_scan(kind):
    from livo_amd import synth
    body = synth.make_scan(6000, 31)[0][:, :3].astype(np.float64)
    body[:, 0] *= 11.0  # the scan reaches 28 m in x: a box 300 m wide, 1200 cells of 0.25 m (> 512)
    body = body.astype(np.float32)
    if kind == "identical":
        body = np.repeat(body[1234:1235], 500, axis=0)
    elif kind == "single":
        body = body[4321:4322]
    return np.ascontiguousarray(body)


@pytest.fixture(scope="module")
def resident_ctx(built):
    import livo_amd
    import frontend_ref as fr
    from livo_amd import synth
    wide = _resident_scan("wide")
    assert 290.0 < np.ptp(wide[:, 0]) < 320.0
    R, p, _ = synth.true_pose(31)
    world = fr.to_world(wide, {"rot": R, "pos": p}, np.eye(3), synth.T_LI).astype(np.float32)
    ctx = livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=4)
    ctx.map_build(world)  # a small map: the scan's own world points
    yield ctx
    ctx.close()


@pytest.mark.parametrize("kind", fc.RESIDENT_KINDS)
def test_resident_scan_three_builders(resident_ctx, kind):
    """One scan stored by the three builders (the device front-end's k_fe_morton, livo_scan_upload,
    and the batch's k_fe_morton_seg): the same update and the same neighbour records."""
    from livo_amd import synth
    ctx = resident_ctx
    body = _resident_scan(kind)
    raw = np.ascontiguousarray(np.concatenate([body, np.zeros((len(body), 2), np.float32)], 1))
    st = synth.make_state(31, rot_deg=0.3, trans_m=0.03)
    sids = [ctx.scan_preprocess(raw, leaf_size=0.0)[0], ctx.scan_upload(body), ctx.scan_upload_batch_async([body])[0]]
    try:
        got = [(ctx.iekf_update(s, st), ctx.scan_neighbors(s)) for s in sids]
    finally:
        for s in sids:
            ctx.scan_release(s)
    (s0, t0), (i0, d0) = got[0]
    if kind == "wide":
        assert t0["effct_feat_num"][0] > 1000  # a real update: the order of the sums matters
    for (s, t), (i, d) in got[1:]:
        for k in ("rot", "pos", "vel", "bias_g", "bias_a", "gravity", "cov"):
            assert np.array_equal(s[k], s0[k]), k
        assert t["iterations"] == t0["iterations"] and t["effct_feat_num"] == t0["effct_feat_num"]
        assert t["converged"] == t0["converged"] and t["res_mean"] == t0["res_mean"]
        assert np.array_equal(t["solution"], t0["solution"])
        assert np.array_equal(i, i0) and np.array_equal(d.view(np.uint32), d0.view(np.uint32))
