"""livo_lio_frame (one LiDAR frame in one call) against the seven-call chain it replaces.

Two contexts are built from the same inputs: one runs Context.lio_frame, the other imu_propagate,
frame_take, (inherit,) release, iekf_update, map_incremental, cloud_publish.  The two run the same
kernels on the same bytes -- the one call only keeps the state on the device and stages the IEKF
slot there (k_lio_stage_slot, which must reproduce the host's cov_factor bit for bit) -- so every
comparison is np.array_equal on bytes: there is no error to allow for.
"""
import os

import numpy as np
import pytest

import imu_cases as imc
import ingest_cases as ic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
LEAF, FS_MAP, MATCH = 0.2, 0.5, 0.2
E_NOMAP, E_NOSCAN, E_BUSY = -3, -4, -8  # LIVO_E_*


@pytest.fixture(scope="module")
def gold(built):
    g = np.load(os.path.join(ROOT, "tests", "golden", "config1_small.npz"))
    st0 = {k[6:]: g[k] for k in g.files if k.startswith("state_")}
    return {"map": np.asarray(g["map"], F), "scan": np.asarray(g["scan"], F)[:, :3], "st0": st0}


def _frame(gold, k, t_beg, blind=0.01):
    """Frame k: the golden scan nudged, as an Avia message, with 21 IMU samples behind t_beg."""
    st0 = gold["st0"]
    rng = np.random.default_rng(11 + k)
    scan = gold["scan"] + F(0.01 * k)
    n = len(scan)
    m = np.zeros(n + 1, ic.LIVOX)
    m["x"][1:], m["y"][1:], m["z"][1:] = scan.T
    m["tag"], m["line"] = 0x10, rng.integers(0, 6, n + 1)
    m["offset_time"] = rng.integers(500_000, 99_000_000, n + 1)
    t = t_beg + 0.005 * np.arange(22)
    f_body = st0["rot"].T @ (-st0["gravity"]) + st0["bias_a"]
    acc = f_body + rng.normal(0, 0.02, (22, 3))
    gyr = st0["bias_g"] + np.array([0.01, -0.02, 0.015]) + rng.normal(0, 0.002, (22, 3))
    imu = np.concatenate([t[1:, None], acc[1:], gyr[1:]], 1)
    return {"msg": m, "imu": imu, "t": t, "acc": acc, "gyr": gyr, "blind": blind,
            "params": imc.inited_params({**imc.default_params(), "mean_acc": f_body})}


def _start(gold, fr, cov=None):
    st0 = gold["st0"]
    carry = {"last_imu": np.concatenate([[fr["t"][0]], fr["acc"][0], fr["gyr"][0]]), "acc_s_last": np.zeros(3),
             "angvel_last": fr["gyr"][0] - st0["bias_g"], "last_lidar_end_time": fr["t"][0]}
    return dict(st0, vel=np.zeros(3), cov=np.eye(18) * 0.01 if cov is None else cov), carry


def _ctx(gold, ivox=False, with_map=True):
    import livo_amd
    from livo_amd import synth
    c = livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=4)
    if ivox:
        c.set_backend(livo_amd.BACKEND_IVOX)
        c.ivox_init(resolution=0.5, nearby_type=18, capacity=1_000_000)
        if with_map:
            c.ivox_add_points(gold["map"])
    elif with_map:
        c.map_build(gold["map"])
    return c


def _ingest(c, fr):
    import livo_amd
    p = livo_amd.ingest_params(lidar_type=ic.AVIA, n_scans=16, point_filter_num=1, blind=fr["blind"])
    info = c.frame_ingest_livox(fr["msg"], p)
    t0 = fr["t"][0]
    return t0, t0 + float(info["end_curvature"]) / 1000.0, ic.take_limit(t0, info["end_curvature"], True)


def _one(c, fr, state, carry, prev, n_imu=None, **kw):
    t0, end, lim = _ingest(c, fr)
    imu = fr["imu"] if n_imu is None else fr["imu"][:n_imu]
    return c.lio_frame(imu, t0, end, fr["params"], carry, state, lim, filter_size_surf=LEAF,
                       filter_size_map_min=FS_MAP, match_leaf=MATCH, prev_scan_id=prev, **kw)


def _chain(c, fr, state, carry, prev, n_imu=None, ekf_inited=True, first_scan=False, dense_map_en=True):
    """The seven calls; the same tuple as Context.lio_frame."""
    import livo_amd
    t0, end, lim = _ingest(c, fr)
    imu = fr["imu"] if n_imu is None else fr["imu"][:n_imu]
    st, cy, _ = c.imu_propagate(imu, t0, end, fr["params"], carry, state, want_poses=False)
    prop = st
    nt, sid, _, down = c.frame_take(lim, True, leaf_size=LEAF)
    S = {"stage": livo_amd.LIO_EMPTY, "scan_id": sid, "n_taken": nt, "n_down": len(down), "map_built": 0,
         "iter": None, "map_counts": [0, 0], "cloud": None}
    if nt == 0:
        return st, prop, cy, S
    if first_scan:
        S["stage"] = livo_amd.LIO_FIRST_SCAN
        if len(down) > 5:
            if getattr(c, "backend", 0) == livo_amd.BACKEND_IVOX:
                c.ivox_add_points(down[:, :3])
            else:
                c.map_build(down[:, :3])
            S["map_built"] = 1
        return st, prop, cy, S
    if prev >= 0:
        if getattr(c, "backend", 0) == livo_amd.BACKEND_IVOX:
            c.scan_inherit_neighbors(sid, prev)
        c.scan_release(prev)
    if ekf_inited:
        st, S["iter"] = c.iekf_update(sid, st, prop)
    counts = np.zeros(2, np.int64)
    s = livo_amd.state_to_c(st)
    rc = c._L.livo_map_incremental(c.h, sid, s, FS_MAP, int(ekf_inited), None, counts.ctypes.data)
    assert rc == 0
    S["map_counts"] = [int(counts[0]), int(counts[1])]
    S["cloud"] = c.cloud_publish(st, -1 if dense_map_en else sid, MATCH)
    S["stage"] = livo_amd.LIO_UPDATED
    return st, prop, cy, S


def _eq_state(a, b, what):
    for k in a:
        x, y = np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (what, k)


def _eq_carry(a, b, what):
    for k in a:
        assert np.array_equal(np.asarray(a[k], np.float64).view(np.uint64),
                              np.asarray(b[k], np.float64).view(np.uint64)), (what, k)


def _eq_iter(a, b, what):
    if b is None:
        assert a["iterations"] == 0 and a["knn_passes"] == 0, what
        return
    for k in b:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)


def _world(c, which):
    return c.frame_to_world(imc_identity(), which).view(np.uint32)


def imc_identity():
    return {"rot": np.eye(3), "pos": np.zeros(3), "vel": np.zeros(3), "bias_g": np.zeros(3), "bias_a": np.zeros(3),
            "gravity": np.zeros(3), "cov": np.zeros((18, 18))}


def _eq_device(c1, c2, what, ivox=False, sid=None):
    import livo_amd
    if ivox:
        for a, b in zip(c1.ivox_dump(), c2.ivox_dump()):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, "ivox_dump")
    else:
        for a, b in zip(c1.map_dump(), c2.map_dump()):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, "map_dump")
    assert c1.cloud_info() == c2.cloud_info(), what
    for which in (livo_amd.CLOUD_WORLD, livo_amd.CLOUD_WORLD_DOWN):
        assert np.array_equal(_world(c1, which), _world(c2, which)), (what, which)
    if sid is not None:
        # (an ikd-Tree map_incremental that rebuilt the grid invalidates every scan's records:
        # livo_scan_neighbors then answers LIVO_E_NOSCAN, on both contexts alike)
        got = []
        for c, s in ((c1, sid[0]), (c2, sid[1])):
            try:
                got.append(c.scan_neighbors(s))
            except livo_amd.LivoError as e:
                got.append(e.code)
        if isinstance(got[1], int):
            assert got[0] == got[1] == E_NOSCAN, (what, got)
        else:
            for a, b in zip(*got):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, "neighbours")


def _eq_result(r1, r2, what, nonvacuous=True):
    (s1, p1, c1, S1), (s2, p2, c2, S2) = r1, r2
    _eq_state(s1, s2, what + " state")
    _eq_state(p1, p2, what + " state_propagat")
    _eq_carry(c1, c2, what + " carry")
    for k in ("stage", "n_taken", "n_down", "map_built", "map_counts"):
        assert S1[k] == S2[k], (what, k, S1[k], S2[k])
    _eq_iter(S1["iter"], S2["iter"], what)
    if S2["cloud"] is not None:
        assert S1["cloud"] == S2["cloud"], what
    if nonvacuous and S2["iter"] is not None:
        assert S1["iter"]["iterations"] >= 1 and S1["iter"]["effct_feat_num"][0] > 100, (what, S1["iter"])


@pytest.mark.parametrize("ivox", [False, True], ids=["ikd", "ivox"])
def test_three_frames_equal_the_chain(gold, ivox):
    """Three consecutive frames (different messages and IMU segments), carry and prev_scan_id threaded."""
    import livo_amd
    a, b = _ctx(gold, ivox), _ctx(gold, ivox)
    try:
        fr0 = _frame(gold, 0, imc.T0)
        sa, ca = _start(gold, fr0)
        sb, cb = dict(sa), dict(ca)
        pa = pb = -1
        t = imc.T0
        for k in range(3):
            fr = _frame(gold, k, t)
            ra = _one(a, fr, sa, ca, pa)
            rb = _chain(b, fr, sb, cb, pb)
            _eq_result(ra, rb, f"frame {k}")
            assert ra[3]["stage"] == livo_amd.LIO_UPDATED
            pa, pb = ra[3]["scan_id"], rb[3]["scan_id"]
            _eq_device(a, b, f"frame {k}", ivox, (pa, pb))
            sa, ca, sb, cb = ra[0], ra[2], rb[0], rb[2]
            t = fr["t"][-1]
        # the hand-off to the camera: a propagation to an image time, then the published cloud read back
        fr = _frame(gold, 3, t)
        ha = a.imu_propagate(fr["imu"][:5], t, fr["imu"][4, 0], fr["params"], ca, sa, want_poses=True)
        hb = b.imu_propagate(fr["imu"][:5], t, fr["imu"][4, 0], fr["params"], cb, sb, want_poses=True)
        _eq_state(ha[0], hb[0], "hand-off state")
        assert np.array_equal(ha[2], hb[2])
        # addSparseMap on the published cloud at the camera's state: the consumer of pcl_wait_pub
        from livo_amd import synth
        cam = {"fx": 100.0, "fy": 100.0, "cx": 80.0, "cy": 64.0, "d": [0.0] * 5, "width": 160, "height": 128}
        vp = livo_amd.vio_params(cam, synth.R_CI, synth.P_CI)
        vp.patch_size = 4
        img = np.random.default_rng(3).integers(0, 256, (128, 160)).astype(np.uint8)
        va = a.vio_select(ha[0], img, vp, 16, livo_amd.CLOUD_WORLD)
        vb = b.vio_select(hb[0], img, vp, 16, livo_amd.CLOUD_WORLD)
        print("hand-off select", va[2])
        assert va[2] == vb[2] and va[2]["n_in"] == ra[3]["cloud"]["n"] > 0
        assert va[0].tobytes() == vb[0].tobytes() and va[1].tobytes() == vb[1].tobytes()
        _eq_device(a, b, "hand-off", ivox)
    finally:
        a.close()
        b.close()


def _cov_cases():
    rng = np.random.default_rng(5)
    A = rng.normal(0, 0.05, (18, 18))
    dense = A @ A.T + np.eye(18) * 0.01
    asym = dense.copy()
    asym[0, 1] *= 1.0 + 1e-9
    nspd = dense.copy()
    nspd[2, 2] = -1e-6
    near = dense.copy()
    near[0, 1] += 0.5e-12 * np.abs(dense[:, :6]).max()  # under 1e-12 * amax: still factored
    return {"dense": dense, "asym": asym, "not_spd": nspd, "near_sym": near}


@pytest.mark.parametrize("case", ["dense", "asym", "not_spd", "near_sym", "n_imu0"])
def test_factor_branches(gold, case):
    """Start covariances that take every exit of cov_factor: the device must choose the same solve
    path with the same factors.  n_imu = 0 passes P through the propagation unchanged."""
    a, b = _ctx(gold), _ctx(gold)
    try:
        fr = _frame(gold, 0, imc.T0)
        cov = _cov_cases().get(case, _cov_cases()["asym"] if case == "n_imu0" else None)
        st, cy = _start(gold, fr, cov)
        n_imu = 0 if case == "n_imu0" else None
        ra = _one(a, fr, st, cy, -1, n_imu=n_imu)
        rb = _chain(b, fr, dict(st), dict(cy), -1, n_imu=n_imu)
        print(case, "iterations", ra[3]["iter"]["iterations"], "effct", ra[3]["iter"]["effct_feat_num"][:1])
        _eq_result(ra, rb, case)
        _eq_device(a, b, case, False, (ra[3]["scan_id"], rb[3]["scan_id"]))
    finally:
        a.close()
        b.close()


def test_ekf_not_inited(gold):
    a, b = _ctx(gold), _ctx(gold)
    try:
        fr = _frame(gold, 0, imc.T0)
        st, cy = _start(gold, fr)
        ra = _one(a, fr, st, cy, -1, ekf_inited=False, dense_map_en=False)
        rb = _chain(b, fr, dict(st), dict(cy), -1, ekf_inited=False, dense_map_en=False)
        _eq_result(ra, rb, "ekf_inited=0")
        _eq_state(ra[0], ra[1], "state == state_propagat")
        assert not ra[3]["iter_raw"].any()
        _eq_device(a, b, "ekf_inited=0")
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("ivox", [False, True], ids=["ikd", "ivox"])
def test_first_scan_then_update(gold, ivox):
    import livo_amd
    a, b = _ctx(gold, ivox, with_map=False), _ctx(gold, ivox, with_map=False)
    try:
        fr = _frame(gold, 0, imc.T0)
        st, cy = _start(gold, fr)
        ra = _one(a, fr, st, cy, -1, first_scan=True)
        rb = _chain(b, fr, dict(st), dict(cy), -1, first_scan=True)
        _eq_result(ra, rb, "first scan")
        assert ra[3]["stage"] == livo_amd.LIO_FIRST_SCAN and ra[3]["map_built"] == 1
        for c in (a, b):
            with pytest.raises(livo_amd.LivoError) as e:
                c.cloud_info()
            assert e.value.code == E_NOSCAN
        fr1 = _frame(gold, 1, fr["t"][-1])
        ra2 = _one(a, fr1, ra[0], ra[2], ra[3]["scan_id"])
        rb2 = _chain(b, fr1, rb[0], rb[2], rb[3]["scan_id"])
        _eq_result(ra2, rb2, "after first scan", nonvacuous=False)
        _eq_device(a, b, "after first scan", ivox, (ra2[3]["scan_id"], rb2[3]["scan_id"]))
    finally:
        a.close()
        b.close()


def test_first_scan_too_small_builds_nothing(gold):
    import livo_amd
    a = _ctx(gold, with_map=False)
    try:
        fr = _frame(gold, 0, imc.T0)
        fr["msg"] = fr["msg"][:5]  # point 0 is never emitted: four points, n_down <= 5
        st, cy = _start(gold, fr)
        r = _one(a, fr, st, cy, -1, first_scan=True)
        assert r[3]["stage"] == livo_amd.LIO_FIRST_SCAN and r[3]["map_built"] == 0 and 0 < r[3]["n_down"] <= 5
        _ingest(a, fr)  # no map was built: the next frame is refused for the lack of one
        with pytest.raises(livo_amd.LivoError) as e:
            _one_no_ingest(a, fr, r[0], r[2], prev=r[3]["scan_id"])
        assert e.value.code == E_NOMAP
    finally:
        a.close()


def test_empty_frame(gold):
    import livo_amd
    a, b = _ctx(gold), _ctx(gold)
    try:
        fr0 = _frame(gold, 0, imc.T0)
        st, cy = _start(gold, fr0)
        ra = _one(a, fr0, st, cy, -1)
        rb = _chain(b, fr0, dict(st), dict(cy), -1)
        prev = ra[3]["scan_id"]
        before = [x.copy() for x in a.map_dump()], a.cloud_info(), _world(a, livo_amd.CLOUD_WORLD).copy()
        fr = _frame(gold, 1, fr0["t"][-1], blind=1e9)  # every point fails the handler
        ea = _one(a, fr, ra[0], ra[2], prev)
        assert ea[3]["stage"] == livo_amd.LIO_EMPTY and ea[3]["scan_id"] == -1 and ea[3]["n_taken"] == 0
        _ingest(b, fr)
        pb, cb, _ = b.imu_propagate(fr["imu"], fr["t"][0], fr["t"][0], fr["params"], rb[2], rb[0], want_poses=False)
        _eq_state(ea[0], pb, "empty state")
        _eq_state(ea[1], pb, "empty state_propagat")
        _eq_carry(ea[2], cb, "empty carry")
        after = a.map_dump(), a.cloud_info(), _world(a, livo_amd.CLOUD_WORLD)
        assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0]))
        assert before[1] == after[1] and np.array_equal(before[2], after[2])
        assert len(a.frame_to_world(imc_identity(), prev)) == ra[3]["n_down"]  # prev_scan_id is still resident
    finally:
        a.close()
        b.close()


def test_refusals_on_a_live_context(gold):
    import livo_amd
    a = _ctx(gold)
    try:
        fr = _frame(gold, 0, imc.T0)
        st, cy = _start(gold, fr)
        sid = a.scan_upload(gold["scan"])
        _ingest(a, fr)
        info, minfo = a.frame_info(), a.map_info()

        def refused(code, prev, c=a, minfo=minfo):
            rc, same = _raw_call(c, fr, st, cy, prev)
            assert rc == code, (rc, code)
            assert same, "a refusal changed the caller's state, state_propagat, carry or stats"
            assert c.frame_info() == info
            if minfo is not None:
                assert c.map_info() == minfo

        refused(E_NOSCAN, prev=12345)
        ticket = a.iekf_update_batch_submit([sid], [st])
        refused(E_BUSY, prev=-1)
        a.iekf_update_batch_wait(ticket, 1)
        r = _one_no_ingest(a, fr, st, cy, prev=-1)
        assert r[3]["stage"] == livo_amd.LIO_UPDATED
    finally:
        a.close()
    e = _ctx(gold, with_map=False)
    try:
        _ingest(e, fr)
        info = e.frame_info()
        refused(E_NOMAP, -1, c=e, minfo=None)
    finally:
        e.close()


def _raw_call(c, fr, state, carry, prev):
    """livo_lio_frame on ctypes structures the caller keeps -> (code, whether their bytes stayed)."""
    import ctypes as C

    import livo_amd
    t0 = fr["t"][0]
    info = c.frame_info()
    imu = np.ascontiguousarray(fr["imu"], np.float64)
    job = livo_amd.ImuJob(imu.ctypes.data, imu.shape[0], t0, t0 + float(info["end_curvature"]) / 1000.0)
    q, cy, s = livo_amd.imu_params_to_c(fr["params"]), livo_amd.imu_carry_to_c(carry), livo_amd.state_to_c(state)
    sp, ls = livo_amd.state_to_c(state), livo_amd.LioStats()
    lp = livo_amd.LioParams(LEAF, MATCH, FS_MAP, 1, 0, 1, prev)
    keep = [bytes(x) for x in (cy, s, sp, ls)]
    rc = c._L.livo_lio_frame(c.h, C.byref(job), C.byref(q), C.byref(cy), ic.take_limit(t0, info["end_curvature"], True),
                             C.byref(lp), C.byref(s), C.byref(sp), C.byref(ls))
    return rc, keep == [bytes(x) for x in (cy, s, sp, ls)]


def _one_no_ingest(c, fr, state, carry, prev):
    t0 = fr["t"][0]
    info = c.frame_info()
    end = t0 + float(info["end_curvature"]) / 1000.0
    return c.lio_frame(fr["imu"], t0, end, fr["params"], carry, state, ic.take_limit(t0, info["end_curvature"], True),
                       filter_size_surf=LEAF, filter_size_map_min=FS_MAP, match_leaf=MATCH, prev_scan_id=prev)


def test_determinism(gold):
    a, b = _ctx(gold), _ctx(gold)
    try:
        fr = _frame(gold, 0, imc.T0)
        st, cy = _start(gold, fr)
        ra = _one(a, fr, st, cy, -1)
        rb = _one(b, fr, dict(st), dict(cy), -1)
        _eq_state(ra[0], rb[0], "state")
        assert np.array_equal(ra[3]["iter_raw"], rb[3]["iter_raw"])
        _eq_device(a, b, "determinism", False, (ra[3]["scan_id"], rb[3]["scan_id"]))
    finally:
        a.close()
        b.close()
