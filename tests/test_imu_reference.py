"""CPU checks of the IMU restatements in tests/imu_cases.py (no GPU): the float64 walk of
IMU_Processing.cpp:236-338 against the longdouble one within the bars the GPU test uses, closed
forms of the propagation, and IMU_init (the restatement and livo_imu_init, which is host code).
"""
import numpy as np
import pytest

import imu_cases as ic

LD = np.longdouble


@pytest.mark.parametrize("acc_norm", [9.79, 1.0])
def test_float64_restatement_within_the_bars(acc_norm):
    names, jobs, params, carries, states = ic.batch(acc_norm)
    worst = 0.0
    for name, (r64, rld) in zip(names, ic.batch_refs(acc_norm)):
        bars = ic.trajectory_bars(rld)
        f = ic.trajectory_frac(r64["state"], r64["carry"], r64["poses"], rld, bars)
        assert f <= 1.0, (name, f)
        assert ic.cov_error(r64["state"]["cov"], rld["state"]["cov"]) < 1e-12, name
        assert r64["carry"]["last_lidar_end_time"] == rld["carry"]["last_lidar_end_time"]
        worst = max(worst, f)
    print(f"FRAC restatement-64 acc_norm={acc_norm} {worst:.4f}")


def _rest_state():
    st = {"rot": np.eye(3), "pos": np.array([1.0, 2.0, 3.0]), "vel": np.array([0.5, -0.25, 0.125]),
          "bias_g": np.zeros(3), "bias_a": np.zeros(3), "gravity": np.array([0.0, 0.0, -ic.G]),
          "cov": ic.dense_cov(ic._rng("closed"))}
    return st


def _job(n, acc, gyr, step=0.005):
    t = ic.T0 + step * np.arange(n + 1)
    imu = np.concatenate([t[1:, None], np.tile(acc, (n, 1)), np.tile(gyr, (n, 1))], 1)
    carry = {"last_imu": np.concatenate([[t[0]], acc, gyr]), "acc_s_last": np.zeros(3), "angvel_last": np.zeros(3),
             "last_lidar_end_time": t[0]}
    return (imu, t[0], t[-1]), carry, t[-1] - t[0]


def test_constant_rate_about_one_axis():
    """Constant rate about z, the accelerometer cancelling gravity: R = Exp(w T), v and p on a line."""
    st = _rest_state()
    w = np.array([0.0, 0.0, 0.8])
    job, carry, T = _job(40, np.array([0.0, 0.0, ic.G]), w)
    p = ic.inited_params({**ic.default_params(), "mean_acc": np.array([0.0, 0.0, ic.G])})
    r = ic.propagate(job, p, carry, st)
    assert np.abs(r["state"]["rot"] - ic.exp_so3(w, T, np.float64)).max() < 1e-13
    assert np.abs(r["state"]["vel"] - st["vel"]).max() < 1e-12
    assert np.abs(r["state"]["pos"] - (st["pos"] + st["vel"] * T)).max() < 1e-12


def test_zero_rate_constant_force_is_the_parabola():
    st = _rest_state()
    f = np.array([0.4, -0.3, ic.G + 0.2])
    job, carry, T = _job(40, f, np.zeros(3))
    p = ic.inited_params({**ic.default_params(), "mean_acc": np.array([0.0, 0.0, ic.G])})
    r = ic.propagate(job, p, carry, st)
    a = f + st["gravity"]
    assert np.array_equal(r["state"]["rot"], np.eye(3))
    assert np.abs(r["state"]["vel"] - (st["vel"] + a * T)).max() < 1e-12
    assert np.abs(r["state"]["pos"] - (st["pos"] + st["vel"] * T + 0.5 * a * T * T)).max() < 1e-12


def test_zero_dt_segments_change_nothing():
    st = _rest_state()
    job, carry, _ = _job(5, np.array([0.1, 0.2, 9.7]), np.array([0.3, -0.2, 0.1]), step=0.0)
    p = ic.inited_params({**ic.default_params(), "mean_acc": np.array([0.0, 0.0, ic.G])})
    r = ic.propagate(job, p, carry, st)
    for k in ("rot", "pos", "vel", "cov"):
        assert np.array_equal(r["state"][k], st[k]), k
    assert len(r["poses"]) == 6 and np.all(r["poses"][:, 0] == 0.0)


def test_no_noise_and_identity_transition_keep_the_covariance():
    """cov_w = 0 with F = I (dt = 0): P unchanged; and cov_w = 0 alone keeps a zero P at zero."""
    st = _rest_state()
    z = {k: np.zeros(3) for k in ("cov_acc", "cov_gyr", "cov_bias_gyr", "cov_bias_acc")}
    p = {**z, "mean_acc": np.array([0.0, 0.0, ic.G])}
    job, carry, _ = _job(4, np.array([0.1, 0.2, 9.7]), np.array([0.3, -0.2, 0.1]), step=0.0)
    assert np.array_equal(ic.propagate(job, p, carry, st)["state"]["cov"], st["cov"])
    job, carry, _ = _job(4, np.array([0.1, 0.2, 9.7]), np.array([0.3, -0.2, 0.1]))
    st0 = {**st, "cov": np.zeros((18, 18))}
    assert np.array_equal(ic.propagate(job, p, carry, st0)["state"]["cov"], np.zeros((18, 18)))


# ------------------------------------------------------------------------------- IMU_init ----
def _still(n, acc, gyr, rng, noise=1e-3):
    t = ic.T0 + 0.005 * np.arange(n)
    return np.concatenate([t[:, None], acc + rng.normal(0, noise, (n, 3)), gyr + rng.normal(0, noise, (n, 3))], 1)


def _init_both(built, imu, params, it, mg, st):
    import livo_amd
    a = ic.imu_init(imu, params, it, mg, st)
    b = livo_amd.imu_init(imu, params, it, mg, st)
    assert a[0] == b[0] and a[2] == b[2]
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k]), k
    assert np.array_equal(a[3], b[3])
    for k in ("gravity", "bias_g"):
        assert np.array_equal(a[4][k], b[4][k]), k
    return a


def test_imu_init(built):
    rng = ic._rng("init")
    st = _rest_state()
    tilt = ic.rot_axis_angle([1.0, 0.3, 0.0], 0.25) @ np.array([0.0, 0.0, 9.79])
    gyr = np.array([0.01, -0.02, 0.005])
    imu = _still(60, tilt, gyr, rng)
    # fewer than 50 samples: still collecting (init_iter_num starts at 1 and counts 1 + samples)
    s, p, it, mg, st1 = _init_both(built, imu[:48], ic.default_params(), 1, np.zeros(3), st)
    assert (s, it) == (0, 49) and np.array_equal(st1["gravity"], st["gravity"])
    assert np.array_equal(p["cov_bias_gyr"], np.full(3, 0.1))
    # exactly the 50th count: done
    s, p, it, mg, st2 = _init_both(built, imu[48:49], p, it, mg, st1)
    assert (s, it) == (2, 50)
    m = p["mean_acc"]
    assert np.allclose(m, imu[:49, 1:4].mean(0), atol=1e-12)
    assert np.array_equal(st2["gravity"], -m / np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]) * ic.G)
    assert np.array_equal(st2["bias_g"], mg) and np.allclose(mg, imu[:49, 4:7].mean(0), atol=1e-12)
    assert np.array_equal(p["cov_acc"], np.full(3, 0.01)) and np.array_equal(p["cov_bias_acc"], np.full(3, 1e-4))
    assert abs(np.linalg.norm(st2["gravity"]) - ic.G) < 1e-12
    # a moving IMU resets, with Reset()'s values
    s, p, it, mg, _ = _init_both(built, _still(10, tilt * 1.2, gyr, rng), ic.default_params(), 1, np.zeros(3), st)
    assert (s, it) == (1, 1) and np.array_equal(p["mean_acc"], [0.0, 0.0, -1.0]) and np.array_equal(mg, np.zeros(3))
    s, _, it, _, _ = _init_both(built, _still(10, tilt, gyr + 0.5, rng), ic.default_params(), 1, np.zeros(3), st)
    assert (s, it) == (1, 1)
    # no samples: nothing changes
    s, p, it, mg, _ = _init_both(built, imu[:0], ic.default_params(), 7, gyr, st)
    assert (s, it) == (0, 7) and np.array_equal(mg, gyr)
