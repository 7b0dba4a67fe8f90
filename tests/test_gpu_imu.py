"""GPU checks of the IMU forward propagation (livo_imu_propagate, livo_imu_propagate_batch,
livo_scan_preprocess_imu) against the restatements of tests/imu_cases.py.

Trajectory, Pose6D rows and carry: held to the longdouble restatement within the bars derived in
imu_cases (float64 roundings per quantity and per propagated sample).  Covariance:
max(100 x the float64 restatement's own error against longdouble, 1e-11) x |P_out|.  Every test
prints its largest error as a fraction of its bar (FRAC ...) and the share of float64 values
equal bit for bit to the float64 restatement.
"""
import os

import numpy as np
import pytest

import frontend_cases as fc
import imu_cases as ic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ictx(built):
    import livo_amd
    from livo_amd import synth
    ctx = livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=4)
    yield ctx
    ctx.close()


def _equal_share(got_state, got_poses, r64):
    a = np.concatenate([got_poses.ravel()] + [np.ravel(got_state[k]) for k in ("rot", "pos", "vel")])
    b = np.concatenate([r64["poses"].ravel()] + [np.ravel(r64["state"][k]) for k in ("rot", "pos", "vel")])
    return float((a == b).mean())


def _hold(name, st, cy, poses, r64, rld):
    """-> (trajectory fraction, covariance fraction, bit-equal share) of one job's results."""
    f = ic.trajectory_frac(st, cy, poses, rld, ic.trajectory_bars(rld))
    assert np.array_equal(cy["last_imu"], r64["carry"]["last_imu"]), name
    assert cy["last_lidar_end_time"] == r64["carry"]["last_lidar_end_time"], name
    for k in ("bias_g", "bias_a", "gravity"):
        assert np.array_equal(st[k], r64["state"][k]), (name, k)
    fp = ic.cov_error(st["cov"], rld["state"]["cov"]) / ic.cov_bar(r64, rld)
    return f, fp, _equal_share(st, poses, r64)


@pytest.fixture(scope="module")
def batch_results(ictx):
    """The ragged batch of every edge case, once per |mean_acc|: one launch each."""
    out = {}
    for acc_norm in (9.79, 1.0):
        _, jobs, params, carries, states = ic.batch(acc_norm)
        out[acc_norm] = ictx.imu_propagate_batch(list(jobs), params, list(carries), list(states))
    return out


@pytest.mark.parametrize("acc_norm", [9.79, 1.0])
def test_ragged_batch_against_the_restatements(batch_results, acc_norm):
    names = ic.batch(acc_norm)[0]
    sts, cys, tabs = batch_results[acc_norm]
    worst, worst_p, share = 0.0, 0.0, 1.0
    for k, (name, (r64, rld)) in enumerate(zip(names, ic.batch_refs(acc_norm))):
        f, fp, eq = _hold(name, sts[k], cys[k], tabs[k], r64, rld)
        print(f"FRAC imu-batch acc_norm={acc_norm} {name} traj {f:.4f} cov {fp:.4f} bits-equal {eq:.4f}")
        assert f <= 1.0 and fp <= 1.0, (name, f, fp)
        worst, worst_p, share = max(worst, f), max(worst_p, fp), min(share, eq)
    print(f"FRAC imu-batch acc_norm={acc_norm} worst traj {worst:.4f} cov {worst_p:.4f} bits-equal>= {share:.4f}")


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def test_single_jobs_equal_the_batch_bit_for_bit(ictx, batch_results):
    names, jobs, params, carries, states = ic.batch(9.79)
    sts, cys, tabs = batch_results[9.79]
    for k, name in enumerate(names):
        st, cy, tab = ictx.imu_propagate(jobs[k][0], jobs[k][1], jobs[k][2], params, carries[k], states[k])
        assert _same(st, sts[k]) and _same(cy, cys[k]) and np.array_equal(tab, tabs[k]), name
    # job order does not matter
    order = np.random.default_rng(5).permutation(len(names))
    s2, c2, t2 = ictx.imu_propagate_batch([jobs[i] for i in order], params, [carries[i] for i in order],
                                          [states[i] for i in order])
    for pos, i in enumerate(order):
        assert _same(s2[pos], sts[i]) and _same(c2[pos], cys[i]) and np.array_equal(t2[pos], tabs[i]), names[i]
    # no table asked for: the same states and carries
    s3, c3, t3 = ictx.imu_propagate_batch(list(jobs), params, list(carries), list(states), want_poses=False)
    assert t3 is None and all(_same(a, b) for a, b in zip(s3, sts)) and all(_same(a, b) for a, b in zip(c3, cys))


def test_table_that_does_not_fit_is_refused(ictx):
    import livo_amd
    job, params, carry, state = ic.make_case(20)
    with pytest.raises(livo_amd.LivoError) as e:
        ictx.imu_propagate_batch([job], params, [carry], [state], pose_cap=20)
    assert e.value.code == -6
    sts, _, tabs = ictx.imu_propagate_batch([job], params, [carry], [state], pose_cap=21)
    assert len(tabs[0]) == 21


def test_frame_split_at_an_image_chains_through_the_carry(ictx):
    """A camera call ending mid-frame, then the LiDAR call ending at the last point: the second
    call starts from the first one's carry and state, as the restatement does."""
    job, params, carry, state = ic.make_case(20)
    imu, beg, end = job
    t_img = imu[9, 0] + 0.002  # between two samples
    cam = (imu[:10], beg, t_img)
    st1, cy1, tab1 = ictx.imu_propagate(cam[0], cam[1], cam[2], params, carry, state)
    lid = (imu[10:], t_img, end)  # pcl_beg_time = max(lidar_beg_time, last_update_time)
    st2, cy2, tab2 = ictx.imu_propagate(lid[0], lid[1], lid[2], params, cy1, st1)
    a64, ald = ic.propagate(cam, params, carry, state), ic.propagate(cam, params, carry, state, ic.LD)
    f1, p1, e1 = _hold("camera", st1, cy1, tab1, a64, ald)
    # the second leg's restatements start where the device's first leg ended: the leg alone is held
    b64, bld = ic.propagate(lid, params, cy1, st1), ic.propagate(lid, params, cy1, st1, ic.LD)
    f2, p2, e2 = _hold("lidar", st2, cy2, tab2, b64, bld)
    worst = max(f1, f2, p1, p2)
    print(f"FRAC imu-carry traj {max(f1, f2):.4f} cov {max(p1, p2):.4f} bits-equal {min(e1, e2):.4f}")
    assert worst <= 1.0
    assert cy1["last_lidar_end_time"] == t_img and len(tab1) == 11
    # the first tail of the second leg lies after t_img, its head before: the partial dt
    assert len(tab2) == 11 and tab2[1, 0] == imu[10, 0] - t_img
    # what the second leg started from is what the first one left, as in the restatement's chain
    assert cy2["last_lidar_end_time"] == end and np.array_equal(cy2["last_imu"], imu[-1])
    assert np.array_equal(tab2[0, 7:22], np.concatenate([st1["vel"], st1["pos"], st1["rot"].ravel()]))
    assert np.array_equal(tab2[0, 1:7], np.concatenate([cy1["acc_s_last"], cy1["angvel_last"]]))


def _frame_job(frame):
    """IMU samples whose propagation gives a table at the frame's pose times: 5 ms apart from T0."""
    job, params, carry, state = ic.make_case(20, key="frame")
    return job, params, carry, state


@pytest.mark.parametrize("n", [30_000, 1, 0])
def test_resident_table_equals_host_poses(ictx, n):
    raw = fc.deskew_frame(("segment", "random", 70001), "ident").raw[:n].copy()
    job, params, carry, state = _frame_job(raw)
    st, _, tab = ictx.imu_propagate(job[0], job[1], job[2], params, carry, state)
    sid, und, down = ictx.scan_preprocess_imu(raw, leaf_size=0.5)
    sid2, und2, down2 = ictx.scan_preprocess(raw, tab, st["rot"], st["pos"], leaf_size=0.5)
    ictx.scan_release(sid)
    ictx.scan_release(sid2)
    assert np.array_equal(und, und2) and np.array_equal(down, down2)
    if n > 1:
        assert not np.array_equal(und[:, :3], raw[:, :3])  # the walk moved the points


def test_no_table_then_replaced_table(built):
    import livo_amd
    from livo_amd import synth
    raw = fc.deskew_frame(("segment", "random", 4097), "ident").raw
    with livo_amd.Context(0, t_LI=synth.T_LI) as ctx:
        with pytest.raises(livo_amd.LivoError) as e:
            ctx.scan_preprocess_imu(raw)
        assert e.value.code == -1
        job, params, carry, state = ic.make_case(20, key="frame")
        st1, cy1, tab1 = ctx.imu_propagate(job[0], job[1], job[2], params, carry, state)
        _, und1, _ = ctx.scan_preprocess_imu(raw, leaf_size=0.0)
        # a second propagate (another frame, a faster turn) replaces the table and the end pose
        job2, params2, carry2, state2 = ic.make_case(20, rate="6", key="frame2")
        st2, _, tab2 = ctx.imu_propagate(job2[0], job2[1], job2[2], params2, carry2, state2)
        _, und2, _ = ctx.scan_preprocess_imu(raw, leaf_size=0.0)
        _, ref2, _ = ctx.scan_preprocess(raw, tab2, st2["rot"], st2["pos"], leaf_size=0.0)
        assert np.array_equal(und2, ref2) and not np.array_equal(und2, und1)
        # a camera-frame propagate with no samples leaves a one-row table: nothing to walk
        ctx.imu_propagate(np.zeros((0, 7)), job2[2], job2[2] + 0.01, params2, cy1, st1)
        _, und3, _ = ctx.scan_preprocess_imu(raw, leaf_size=0.0)
        assert np.array_equal(und3, raw)


def test_loop_propagate_preprocess_update(ictx):
    """imu_propagate -> scan_preprocess_imu -> iekf_update(prior = the propagated state) on
    config1_small's map, against the same chain fed from the float64 restatement through the host:
    the same iteration counts and the same state, within test_gpu_frontend.py's bar for a chain fed
    from host poses (1e-6 relative)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "config1_small.npz"))
    st0 = {k[6:]: g[k] for k in g.files if k.startswith("state_")}
    rng = np.random.default_rng(11)
    scan = np.asarray(g["scan"], np.float32)[:, :3]
    n = len(scan)
    raw = np.concatenate([scan, rng.uniform(0, 255, (n, 1)), np.sort(rng.uniform(0.5, 99.0, (n, 1)), 0)],
                         1).astype(np.float32)
    # an IMU nearly at rest at st0: the specific force cancels gravity, a slow turn, 21 samples over 100 ms
    t = ic.T0 + 0.005 * np.arange(22)
    f_body = st0["rot"].T @ (-st0["gravity"]) + st0["bias_a"]
    acc = f_body + rng.normal(0, 0.02, (22, 3))
    gyr = st0["bias_g"] + np.array([0.01, -0.02, 0.015]) + rng.normal(0, 0.002, (22, 3))
    imu = np.concatenate([t[1:, None], acc[1:], gyr[1:]], 1)
    carry = {"last_imu": np.concatenate([[t[0]], acc[0], gyr[0]]), "acc_s_last": np.zeros(3),
             "angvel_last": gyr[0] - st0["bias_g"], "last_lidar_end_time": t[0]}
    start = dict(st0, vel=np.zeros(3), cov=np.eye(18) * 0.01)
    params = ic.inited_params({**ic.default_params(), "mean_acc": f_body})
    job = (imu, t[0], t[0] + 0.0995)
    ctx = ictx
    ctx.map_build(g["map"])
    prior, _, _ = ctx.imu_propagate(job[0], job[1], job[2], params, carry, start)
    sid, _, down = ctx.scan_preprocess_imu(raw, leaf_size=0.2)
    s1, t1 = ctx.iekf_update(sid, prior, prior)
    r64 = ic.propagate(job, params, carry, start)
    sid2, _, down2 = ctx.scan_preprocess(raw, r64["poses"], r64["state"]["rot"], r64["state"]["pos"], leaf_size=0.2)
    s2, t2 = ctx.iekf_update(sid2, r64["state"], r64["state"])
    ctx.scan_release(sid)
    ctx.scan_release(sid2)
    print("loop iterations", t1["iterations"], t2["iterations"], "effct", t1["effct_feat_num"], t2["effct_feat_num"],
          "down", len(down), len(down2))
    assert t1["iterations"] == t2["iterations"] and t1["iterations"] >= 1 and t1["effct_feat_num"][0] > 100
    assert len(down) == len(down2)
    for k in ("rot", "pos", "vel", "cov"):
        a, b = np.asarray(s1[k], np.float64), np.asarray(s2[k], np.float64)
        assert np.all(np.abs(a - b) <= 1e-6 * np.maximum(np.abs(b), 1.0)), k
