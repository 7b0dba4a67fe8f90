"""CPU tests of the VIO photometric-update restatement (oracle/livo_oracle.cpp,
VIO section; SURVEY.md §8f row 4: LidarSelector::UpdateState / ComputeJ,
src/lidar_selection.cpp:748-978).

Parity status: "parity unpinned" against the reference itself (OpenCV, vikit,
Sophus, Eigen, ROS absent; no fixtures).  Pinned against an independent numpy
restatement of the same update (float32 weights / residual sums, float64
Jacobians and algebra), and by its behaviour: on synthetic frames whose
reference patches were sampled at the true pose, the update converges to it.
"""
import numpy as np
import pytest


def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def _exp(v):
    n = np.linalg.norm(v)
    if n <= 1e-5:
        return np.eye(3)
    K = _skew(v / n)
    return np.eye(3) + np.sin(n) * K + (1 - np.cos(n)) * K @ K


def _log(R):
    tr = np.trace(R)
    th = 0.0 if tr > 3 - 1e-6 else np.arccos(0.5 * (tr - 1))
    k = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return 0.5 * k if abs(th) < 0.001 else 0.5 * th / np.sin(th) * k


def _vio_np(fr, st, max_iter=4, cov_img=10.0):
    """The update in numpy.  Image reads are clamped to the frame (the project's
    convention: the reference reads out of bounds there) and every patch pixel
    whose 4x4-tap footprint leaves the frame counts once per iteration in
    out_of_frame.  Returns (state, stats, per-point errors of the last iteration)."""
    from livo_amd import synth
    img = fr["image"].astype(np.float32)
    H_, W = img.shape
    cam, ps = fr["cam"], fr["patch_size"]
    pst, ph = ps * ps, ps // 2
    Rci, Pci = fr["Rci"], fr["Pci"]
    Pic = -Rci.T @ Pci
    Jdphi_dR, Jdp_dR = Rci, -Rci @ _skew(Pic)
    st = {k: np.array(v, copy=True) for k, v in st.items()}
    prior = {k: np.array(v, copy=True) for k, v in st.items()}
    G = np.zeros((18, 18))
    n = len(fr["pos"])
    stats = {"iterations": [0, 0, 0], "updates": [0, 0, 0], "last_error": [np.float32(1e10)] * 3, "out_of_frame": 0,
             "n_meas": 0}
    perr = np.zeros(n, np.float32)
    f32 = np.float32

    def minus(a, b):
        return np.concatenate([_log(b["rot"].T @ a["rot"]), a["pos"] - b["pos"], a["vel"] - b["vel"],
                               a["bias_g"] - b["bias_g"], a["bias_a"] - b["bias_a"], a["gravity"] - b["gravity"]])

    def update_state(level, total):
        nonlocal G
        li = 2 - level
        old = {k: v.copy() for k, v in st.items()}
        last = f32(total)
        for it in range(max_iter):
            stats["iterations"][li] += 1
            Rcw = Rci @ st["rot"].T
            Pcw = -Rcw @ st["pos"] + Pci
            rows, zs = [], []
            err = f32(0)
            for i in range(n):
                scale = 1 << (level + int(fr["levels"][i]))
                pf = Rcw @ fr["pos"][i] + Pcw
                pc = synth._world2cam(cam, pf[None])[0]
                Jdpi = np.array([[cam["fx"] / pf[2], 0, -cam["fx"] * pf[0] / pf[2] ** 2],
                                 [0, cam["fy"] / pf[2], -cam["fy"] * pf[1] / pf[2] ** 2]])
                ui = int(np.floor(f32(pc[0] / scale)) * f32(scale))
                vi = int(np.floor(f32(pc[1] / scale)) * f32(scale))
                su = (f32(pc[0]) - f32(ui)) / f32(scale)
                sv = (f32(pc[1]) - f32(vi)) / f32(scale)
                # the weights are products in double, rounded once
                su_d, sv_d = float(su), float(sv)
                w = [f32((1.0 - su_d) * (1.0 - sv_d)), f32(su_d * (1.0 - sv_d)), f32((1.0 - su_d) * sv_d),
                     f32(su_d * sv_d)]
                P = fr["patches"][i]
                pe = f32(0)
                s = scale
                for x in range(ps):
                    for y in range(ps):
                        r0, c0 = vi + x * scale - ph * scale, ui - ph * scale + y * scale
                        if r0 - s < 0 or r0 + 2 * s >= H_ or c0 - s < 0 or c0 + 2 * s >= W:
                            stats["out_of_frame"] += 1

                        def I(dr, dc):
                            return img[min(max(r0 + dr, 0), H_ - 1), min(max(c0 + dc, 0), W - 1)]
                        bl = lambda a, b, c, d: ((w[0] * a + w[1] * b) + w[2] * c) + w[3] * d  # noqa: E731
                        du = f32(0.5) * (bl(I(0, s), I(0, 2 * s), I(s, s), I(s, 2 * s)) -
                                         bl(I(0, -s), I(0, 0), I(s, -s), I(s, 0)))
                        dv = f32(0.5) * (bl(I(s, 0), I(s, s), I(2 * s, 0), I(2 * s, s)) -
                                         bl(I(-s, 0), I(-s, s), I(0, 0), I(0, s)))
                        J = np.array([du, dv], np.float64) * (1.0 / scale)
                        Jdphi = J @ Jdpi @ _skew(pf)
                        Jdp = -J @ Jdpi
                        rows.append(np.concatenate([Jdphi @ Jdphi_dR + Jdp @ Jdp_dR, Jdp @ Rcw]))
                        res = float(bl(I(0, 0), I(0, s), I(s, 0), I(s, s)) - P[pst * level + x * ps + y])
                        zs.append(res)
                        pe = f32(float(pe) + res * res)
                perr[i] = pe
                err = f32(err + pe)
            err = f32(err / f32(len(zs)))
            stats["n_meas"] = len(zs)
            if err <= last:
                stats["updates"][li] += 1
                old = {k: v.copy() for k, v in st.items()}
                last = err
                Hs, z = np.array(rows), np.array(zs)
                HTH = np.zeros((18, 18))
                HTH[:6, :6] = Hs.T @ Hs
                K1 = np.linalg.inv(HTH + np.linalg.inv(st["cov"] / cov_img))
                G = np.zeros((18, 18))
                G[:, :6] = K1[:, :6] @ HTH[:6, :6]
                vec = minus(prior, st)
                sol = -K1[:, :6] @ (Hs.T @ z) + vec - G[:, :6] @ vec[:6]
                st["rot"] = st["rot"] @ _exp(sol[:3])
                for k, sl in (("pos", 3), ("vel", 6), ("bias_g", 9), ("bias_a", 12), ("gravity", 15)):
                    st[k] = st[k] + sol[sl:sl + 3]
                if np.linalg.norm(sol[:3]) * 57.3 < 0.001 and np.linalg.norm(sol[3:6]) * 100 < 0.001:
                    break
            else:
                st.update({k: v.copy() for k, v in old.items()})
                break
        stats["last_error"][li] = last
        return last

    err0 = f32(1e10)
    now = err0
    for level in (2, 1, 0):
        now = update_state(level, err0)
    stats["cov_updated"] = int(now < err0)
    if now < err0:
        st["cov"] = st["cov"] - G @ st["cov"]
    return st, stats, perr


def _same(got, exp):
    """oracle.vio_update against _vio_np: state to the file's bars, everything that
    steers control flow (counts, per-level float errors, per-point errors) exact."""
    (gs, gst, gerr), (es, est, eerr) = got, exp
    for k in ("iterations", "updates", "cov_updated", "n_meas", "out_of_frame"):
        assert gst[k] == est[k], (k, gst[k], est[k])
    assert np.array_equal(np.float32(gst["last_error"]).view(np.uint32), np.float32(est["last_error"]).view(np.uint32))
    assert np.array_equal(gerr.view(np.uint32), eerr.view(np.uint32))
    assert np.allclose(gs["pos"], es["pos"], rtol=0, atol=1e-9)
    assert np.allclose(gs["rot"], es["rot"], rtol=0, atol=1e-9)
    assert np.allclose(gs["cov"], es["cov"], rtol=0, atol=1e-12)


def test_vio_update_matches_numpy(built):
    import oracle
    from livo_amd import synth
    fr, st, truth = synth.make_vio_frame(150, 1)
    got, stats, err = oracle.vio_update(fr, st)
    _same((got, stats, err), _vio_np(fr, st))
    assert stats["cov_updated"] == 1 and stats["out_of_frame"] == 0


@pytest.fixture(scope="module")
def frame257(built):
    from livo_amd import synth
    return synth.make_vio_frame(257, 8)


def test_vio_border_is_clamped_and_counted(frame257):
    """A window of the image: points near and beyond its border read clamped pixels,
    each such patch pixel counted once per iteration; the error grows at every level."""
    import oracle
    from livo_amd import synth
    fr, st, _ = frame257
    fr = synth.crop_vio_frame(fr, 90, 90, 550, 422)
    assert fr["image"].shape == (332, 460) and fr["image"].flags.c_contiguous
    got = oracle.vio_update(fr, st)
    assert got[1]["out_of_frame"] > 0 and got[1]["cov_updated"] == 1
    assert all(i > u for i, u in zip(got[1]["iterations"], got[1]["updates"]))
    _same(got, _vio_np(fr, st))


def test_vio_point_levels_to_eight(frame257):
    """Point levels 0..8 (scale up to 1024 at pyramid level 2: every tap of the
    coarse points is clamped)."""
    import oracle
    fr, st, _ = frame257
    fr = dict(fr, levels=(np.arange(len(fr["pos"])) % 9).astype(np.int32))
    got = oracle.vio_update(fr, st)
    assert got[1]["out_of_frame"] > 0
    _same(got, _vio_np(fr, st))


def test_vio_points_behind_the_camera(frame257):
    """Every 16th point mirrored through the camera centre: negative depth, a finite
    pixel, the projection Jacobian's sign flipped."""
    import oracle
    from livo_amd import synth
    fr, st, truth = frame257
    fr = synth.mirror_vio_points(fr, truth, 16)
    got = oracle.vio_update(fr, st)
    assert all(np.isfinite(v).all() for v in got[0].values()) and np.isfinite(got[2]).all()
    _same(got, _vio_np(fr, st))


def test_vio_undistorted_camera(built):
    """d0 = 0 switches vikit's world2cam to the plain pinhole."""
    import oracle
    from livo_amd import synth
    fr, st, _ = synth.make_vio_frame(120, 11)
    fr["cam"] = dict(fr["cam"], d=[0.0] * 5)
    got = oracle.vio_update(fr, st)
    assert got[1]["cov_updated"] == 1
    _same(got, _vio_np(fr, st))


def test_vio_update_converges_to_truth(built):
    import oracle
    from livo_amd import synth
    for fid in (0, 2):
        fr, st, truth = synth.make_vio_frame(1500, fid)
        got, stats, err = oracle.vio_update(fr, st)
        assert np.linalg.norm(got["pos"] - truth["pos"]) < 0.1 * np.linalg.norm(st["pos"] - truth["pos"])
        assert np.linalg.norm(_log(got["rot"].T @ truth["rot"])) < 0.1 * np.linalg.norm(_log(st["rot"].T @ truth["rot"]))
        assert sum(stats["updates"]) >= 3 and np.all(err >= 0)


def test_vio_no_points_is_a_no_op(built):
    import oracle
    from livo_amd import synth
    fr, st, _ = synth.make_vio_frame(10, 3)
    for k in ("pos", "levels", "patches"):
        fr[k] = fr[k][:0]
    got, stats, _ = oracle.vio_update(fr, st)
    assert np.array_equal(got["pos"], st["pos"]) and stats["iterations"] == [0, 0, 0]
