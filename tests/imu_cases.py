"""Inputs, restatements and bars of the IMU forward propagation (ImuProcess::IMU_init /
detectZeroVelocity / UndistortPcl's first half, IMU_Processing.cpp:92-338), shared by
tests/test_imu_reference.py (CPU) and tests/test_gpu_imu.py (livo_imu_propagate*).

Restatements.  propagate(job, params, carry, state, T) walks :236-338 in number type T:
numpy.float64 in the reference's expression order (3 x 3 products summed left to right, as the
device kernels write them; the covariance as the dense F @ P @ F.T + Q, a stand-in for Eigen's
product, whose summation order the reference does not pin), or numpy.longdouble, the yardstick.
imu_init(...) is :92-197 in float64.

Trajectory bars (rows of the Pose6D table, the end state, the carry), against the longdouble
run.  u = 2^-53 is one float64 rounding (relative); every bound is a norm over the three
components (a componentwise rounding of relative size u moves the vector's norm by <= u times
its norm) and is carried from sample to sample as a running sum, so it is per quantity and per
propagated sample.  Stamps are exact inputs on both sides and their differences are exact in
float64 (operands within a factor two of each other), so dt carries no error.

    angvel = 0.5 (h + t) - bg           add, sub (the halving is exact)          e_w = 2 u (|0.5 (h + t)| + |bg|)
    acc    = 0.5 (h + t) G / |m| - ba   add, mul, div, sub and |m| (3 mul, 2 add,
                                        sqrt: <= 3 u relative)                   e_b = 7 u (|.| + |ba|)
    Exp(angvel, dt)                     tests/frontend_cases.py's count: 37 u an entry, Frobenius 111 u
                                        (sin and cos at the device library's documented 2 ulp), and the
                                        rate's own error turned by dt: e_w dt
    R = R Exp                           product 15 u (Frobenius)           e_R += (111 + 15) u + e_w dt = K_R u + e_w dt
    acc_imu = R acc + g                 product 6 u, add 1 u               e_a = e_R |acc| + e_b + 7 u (|acc| + |g|)
    pos = (pos + vel dt) + ((0.5 acc_imu) dt) dt    5 roundings            e_p += e_v dt + 0.5 e_a dt^2
                                                                                  + 2 u (|pos| + |vel| dt + |acc_imu| dt^2)
    vel = vel + acc_imu dt              2 roundings                        e_v += e_a dt + 2 u (|vel| + |acc_imu| dt)
    offset_time = stamp - pcl_beg_time  1 rounding                         u |offset|

(pos uses the velocity before its update, so e_p takes the old e_v; |.| are the longdouble
run's magnitudes, the larger of before and after a step.)  The frame end is one more step of
the same kind with |dt| = |pcl_end_time - imu_end_time| (the factors note = +-1 are exact).
Each bar gets 2^-1074-free slack of one more rounding of the quantity itself (the comparison
rounds the longdouble value to float64): + u |x|.

Covariance bar: max(100 x the float64 restatement's own error against longdouble, 1e-11) x
|P_out| (Frobenius), errors as the Frobenius norm of the difference -- tests/test_gpu_solve.py's
rule: the device applies F's blocks in another order of the same sums.
"""
from __future__ import annotations

import functools

import numpy as np

G = 9.81
U = 2.0 ** -53
K_R = 126.0
T0 = 1.7e9  # absolute stamps: seconds since the epoch, as sensor_msgs stamps are
LD = np.longdouble


# ------------------------------------------------------------------------------ restatements ----
def _mm(A, B):
    """3 x 3 (or 3 x n) product, each entry summed left to right."""
    return (A[:, 0:1] * B[0:1, :] + A[:, 1:2] * B[1:2, :]) + A[:, 2:3] * B[2:3, :]


def _mv(A, v):
    return (A[:, 0] * v[0] + A[:, 1] * v[1]) + A[:, 2] * v[2]


def skew(v, T):
    z = T(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=T)


def exp_so3(w, dt, T):
    """Exp(ang_vel, dt) (so3_math.h:31-52)."""
    nrm = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    R = np.eye(3, dtype=T)
    if nrm > T(0.0000001):
        K = skew(w / nrm, T)
        ang = nrm * dt
        s, c1 = np.sin(ang), T(1) - np.cos(ang)
        R = (R + s * K) + _mm(c1 * K, K)
    return R


def new_carry():
    return {"last_imu": np.zeros(7), "acc_s_last": np.zeros(3), "angvel_last": np.zeros(3),
            "last_lidar_end_time": 0.0}


def default_params():
    return {"cov_acc": np.full(3, 0.1), "cov_gyr": np.full(3, 0.1), "cov_bias_gyr": np.full(3, 0.1),
            "cov_bias_acc": np.full(3, 0.1), "mean_acc": np.array([0.0, 0.0, -1.0])}


def inited_params(p=None):
    p = dict(default_params() if p is None else p)
    p.update(cov_acc=np.full(3, 0.01), cov_gyr=np.full(3, 0.01), cov_bias_gyr=np.full(3, 0.0001),
             cov_bias_acc=np.full(3, 0.0001))
    return p


def propagate(job, params, carry, state, T=np.float64, dense=True):
    """:236-338.  job = (imu (n, 7: stamp, acc, gyr), pcl_beg_time, pcl_end_time).
    -> dict(state, carry, poses (rows, 22), steps: per propagated sample the magnitudes the bars use)."""
    imu, beg, end = job
    c = lambda x: np.array(x, dtype=T)  # noqa: E731
    v_imu = np.concatenate([np.asarray(carry["last_imu"], np.float64).reshape(1, 7),
                            np.asarray(imu, np.float64).reshape(-1, 7)]).astype(T)
    beg, end, last_end = T(beg), T(end), T(carry["last_lidar_end_time"])
    acc_imu, angvel = c(carry["acc_s_last"]), c(carry["angvel_last"])
    vel, pos, R = c(state["vel"]), c(state["pos"]), c(state["rot"])
    bg, ba, grav = c(state["bias_g"]), c(state["bias_a"]), c(state["gravity"])
    P = c(state["cov"])
    cov = {k: c(params[k]) for k in ("cov_acc", "cov_gyr", "cov_bias_gyr", "cov_bias_acc")}
    m = c(params["mean_acc"])
    m_norm = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
    row = lambda t: np.concatenate([[t], acc_imu, angvel, vel, pos, R.reshape(9)])  # noqa: E731
    poses, steps = [row(T(0))], []
    half, one = T(0.5), T(1)
    for k in range(len(v_imu) - 1):
        head, tail = v_imu[k], v_imu[k + 1]
        if tail[0] < last_end:
            continue
        mid_w, mid_a = half * (head[4:7] + tail[4:7]), half * (head[1:4] + tail[1:4])
        angvel = mid_w - bg
        raw_a = mid_a * T(G) / m_norm
        acc = raw_a - ba
        dt = tail[0] - last_end if head[0] < last_end else tail[0] - head[0]
        Exp_f, A = exp_so3(angvel, dt, T), exp_so3(angvel, -dt, T)
        F = np.eye(18, dtype=T)
        Q = np.zeros((18, 18), dtype=T)
        F[0:3, 0:3] = A
        F[0:3, 9:12] = -np.eye(3, dtype=T) * dt
        F[3:6, 6:9] = np.eye(3, dtype=T) * dt
        F[6:9, 0:3] = _mm(-R, skew(acc, T)) * dt
        F[6:9, 12:15] = (-R) * dt
        F[6:9, 15:18] = np.eye(3, dtype=T) * dt
        Q[0:3, 0:3] = np.diag(cov["cov_gyr"] * dt * dt)
        Q[6:9, 6:9] = _mm(R * cov["cov_acc"][None, :], R.T.copy()) * dt * dt
        Q[9:12, 9:12] = np.diag(cov["cov_bias_gyr"] * dt * dt)
        Q[12:15, 12:15] = np.diag(cov["cov_bias_acc"] * dt * dt)
        P = F @ P @ F.T + Q
        before = (np.linalg.norm(vel.astype(LD)), np.linalg.norm(pos.astype(LD)))
        R = _mm(R, Exp_f)
        acc_imu = _mv(R, acc) + grav
        pos = (pos + vel * dt) + ((half * acc_imu) * dt) * dt
        vel = vel + acc_imu * dt
        poses.append(row(tail[0] - beg))
        n = lambda x: float(np.linalg.norm(np.asarray(x, LD)))  # noqa: E731
        steps.append(dict(dt=float(dt), w_in=n(mid_w) + n(bg), a_in=n(raw_a) + n(ba), acc=n(acc), g=n(grav),
                          acc_imu=n(acc_imu), vel=max(float(before[0]), n(vel)), pos=max(float(before[1]), n(pos)),
                          off=abs(float(tail[0] - beg))))
    imu_end = v_imu[-1][0]
    frm = imu_end if imu_end > beg else beg
    note = one if end > frm else -one
    dt = note * (end - frm)
    out = dict(state)
    out["vel"] = vel + (note * acc_imu) * dt
    out["rot"] = _mm(R, exp_so3(note * angvel, dt, T))
    out["pos"] = (pos + (note * vel) * dt) + (((note * half) * acc_imu) * dt) * dt
    out["cov"] = P
    for k in ("bias_g", "bias_a", "gravity"):
        out[k] = c(state[k])
    cy = {"last_imu": v_imu[-1].copy(), "acc_s_last": acc_imu, "angvel_last": angvel, "last_lidar_end_time": end}
    n = lambda x: float(np.linalg.norm(np.asarray(x, LD)))  # noqa: E731
    end_step = dict(dt=abs(float(dt)), acc_imu=n(acc_imu), vel=max(n(vel), n(out["vel"])),
                    pos=max(n(pos), n(out["pos"])), w_err_in=0.0)
    return {"state": out, "carry": cy, "poses": np.array(poses, dtype=T).reshape(-1, 22), "steps": steps,
            "end_step": end_step}


def imu_init(imu, params, init_iter_num, mean_gyr, state):
    """IMU_init + detectZeroVelocity (:92-197) in float64 -> (status, params, init_iter_num, mean_gyr, state);
    status 0 collecting, 1 reset, 2 done."""
    imu = np.asarray(imu, np.float64).reshape(-1, 7)
    p = {k: np.array(v, np.float64) for k, v in params.items()}
    mg = np.array(mean_gyr, np.float64)
    st = dict(state)
    if len(imu) == 0:
        return 0, p, init_iter_num, mg, st
    N = init_iter_num
    for s in imu:
        ca, cg = s[1:4], s[4:7]
        if N == 1:
            p["mean_acc"], mg = ca.copy(), cg.copy()
        p["mean_acc"] = p["mean_acc"] + (ca - p["mean_acc"]) / N
        mg = mg + (cg - mg) / N
        da, dg = ca - p["mean_acc"], cg - mg
        p["cov_acc"] = p["cov_acc"] * (N - 1.0) / N + da * da * (N - 1.0) / (N * N)
        p["cov_gyr"] = p["cov_gyr"] * (N - 1.0) / N + dg * dg * (N - 1.0) / (N * N)
        N += 1
    nrm = lambda v: np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])  # noqa: E731
    if not (abs(nrm(p["mean_acc"]) - G) < 0.1 and abs(nrm(mg)) < 0.1):
        p["mean_acc"] = np.array([0.0, 0.0, -1.0])
        return 1, p, 1, np.zeros(3), st
    if N < 50:
        return 0, p, N, mg, st
    st["gravity"] = -p["mean_acc"] / nrm(p["mean_acc"]) * G
    st["bias_g"] = mg.copy()
    return 2, inited_params(p), N, mg, st


# -------------------------------------------------------------------------------------- bars ----
def trajectory_bars(ref):
    """Bars of the module docstring from a longdouble run `ref`: dict(rows: (rows, 22) bars of the
    Pose6D table, rot, pos, vel: the end state's, acc_s_last, angvel_last: the carry's)."""
    rows = np.zeros((len(ref["poses"]), 22))
    eR = ev = ep = ew = ea = 0.0
    for k, s in enumerate(ref["steps"]):
        dt = abs(s["dt"])
        ew = 2 * U * s["w_in"]
        eb = 7 * U * s["a_in"]
        eR = eR + K_R * U + ew * dt
        ea = eR * s["acc"] + eb + 7 * U * (s["acc"] + s["g"])
        ep = ep + ev * dt + 0.5 * ea * dt * dt + 2 * U * (s["pos"] + s["vel"] * dt + s["acc_imu"] * dt * dt)
        ev = ev + ea * dt + 2 * U * (s["vel"] + s["acc_imu"] * dt)
        r = rows[k + 1]
        r[0] = U * s["off"]
        r[1:4] = ea + U * s["acc_imu"]
        r[4:7] = ew + U * s["w_in"]
        r[7:10] = ev + U * s["vel"]
        r[10:13] = ep + U * s["pos"]
        r[13:22] = eR + U
    e = ref["end_step"]
    dt = e["dt"]
    out = {"rows": rows, "acc_s_last": ea + U * e["acc_imu"], "angvel_last": ew + (U * ref["steps"][-1]["w_in"] if ref["steps"] else 0.0),
           "rot": eR + K_R * U + ew * dt + U,
           "vel": ev + ea * dt + 2 * U * (e["vel"] + e["acc_imu"] * dt) + U * e["vel"],
           "pos": ep + ev * dt + 0.5 * ea * dt * dt + 2 * U * (e["pos"] + e["vel"] * dt + e["acc_imu"] * dt * dt)
           + U * e["pos"]}
    return out


def cov_error(P, P_ld):
    """|P - P_ld|_F / |P_ld|_F, in longdouble."""
    P_ld = np.asarray(P_ld, LD)
    return float(np.linalg.norm(np.asarray(P, LD) - P_ld) / np.linalg.norm(P_ld))


def cov_bar(ref64, ref_ld):
    return max(100.0 * cov_error(ref64["state"]["cov"], ref_ld["state"]["cov"]), 1e-11)


def _frac(err, bar):
    """err / bar; a bar of 0 (an exact quantity: a zero rate with zero bias) asks for err == 0."""
    err, bar = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bar, np.float64), np.shape(err))
    out = np.where(err == 0.0, 0.0, np.inf)
    np.divide(err, bar, out=out, where=bar > 0.0)
    return float(out.max()) if out.size else 0.0


def trajectory_frac(got_state, got_carry, got_poses, ref, bars):
    """Largest |got - longdouble| / bar over the table, the end state and the carry; the share
    of float64 values equal bit for bit to `ref64` is the caller's."""
    worst = 0.0
    P = np.asarray(ref["poses"], LD)
    assert got_poses.shape == P.shape, (got_poses.shape, P.shape)
    d = np.abs(np.asarray(got_poses, LD) - P).astype(np.float64)
    assert np.array_equal(got_poses[0], np.asarray(P[0], np.float64))  # row 0: copies of the inputs
    if len(P) > 1:
        worst = _frac(d[1:], bars["rows"][1:])
    for k in ("rot", "pos", "vel"):
        e = float(np.abs(np.asarray(got_state[k], LD) - np.asarray(ref["state"][k], LD)).max())
        worst = max(worst, e / bars[k])
    if ref["steps"]:
        for k in ("acc_s_last", "angvel_last"):
            e = float(np.abs(np.asarray(got_carry[k], LD) - np.asarray(ref["carry"][k], LD)).max())
            worst = max(worst, _frac(e, bars[k]))
    return worst


# ------------------------------------------------------------------------------------ inputs ----
def _rng(*key):
    return np.random.default_rng([0x1A0, *[sum(ord(ch) * 131 ** i for i, ch in enumerate(str(k))) % (2 ** 31) for k in key]])


def rot_axis_angle(axis, rad):
    a = np.asarray(axis, np.float64)
    return exp_so3(a / np.sqrt((a * a).sum()), rad, np.float64)


def dense_cov(rng, asym=1e-6):
    """Dense, correlated, asymmetric by `asym` relative (the reference never symmetrises)."""
    A = rng.normal(size=(18, 18))
    s = 10.0 ** rng.uniform(-3, -1, size=18)
    P = (A @ A.T / 18 + np.eye(18)) * s[:, None] * s[None, :]
    return P * (1.0 + asym * rng.uniform(-1, 1, size=(18, 18)))


def make_state(rng, biases=True):
    g = rot_axis_angle(rng.normal(size=3), 0.2) @ np.array([0.0, 0.0, -G])
    return {"rot": rot_axis_angle(rng.normal(size=3), rng.uniform(0.3, 2.5)), "pos": rng.normal(0, 20.0, 3),
            "vel": rng.normal(0, 3.0, 3), "bias_g": rng.normal(0, 0.02, 3) if biases else np.zeros(3),
            "bias_a": rng.normal(0, 0.1, 3) if biases else np.zeros(3), "gravity": g, "cov": dense_cov(rng)}


def make_params(rng, acc_norm=9.79):
    d = rng.normal(size=3)
    return {"cov_acc": 10.0 ** rng.uniform(-3, -1, 3), "cov_gyr": 10.0 ** rng.uniform(-3, -1, 3),
            "cov_bias_gyr": 10.0 ** rng.uniform(-5, -3, 3), "cov_bias_acc": 10.0 ** rng.uniform(-5, -3, 3),
            "mean_acc": acc_norm * d / np.sqrt((d * d).sum())}


SIZES = (0, 1, 2, 63, 64, 65, 200)
LAYOUTS = ("later", "skip3", "partial", "dup")
ENDS = ("after", "before", "else", "equal")
RATES = ("zero", "0.9e-7", "1.1e-7", "6")


def make_case(n_imu, layout="later", end="after", rate="mid", acc_norm=9.79, key=0):
    """One job with its params, carry and state.  Samples 5 ms apart near T0."""
    rng = _rng("case", n_imu, layout, end, rate, acc_norm, key)
    step = 0.005
    t_last = T0 + 0.0123                     # last_imu_'s stamp
    stamps = t_last + step * np.arange(1, n_imu + 1)
    if layout == "dup" and n_imu >= 2:
        stamps[1::3] = stamps[0::3][:len(stamps[1::3])]  # dt = 0 segments
    last_end = t_last - 0.001                # every sample later
    if layout == "skip3":
        last_end = (stamps[min(3, n_imu) - 1] + 0.001) if n_imu else t_last + 0.001  # the first tails earlier
    elif layout == "partial":
        last_end = t_last + 0.002            # head earlier, first tail later: the partial dt
    beg = last_end
    imu_end = stamps[-1] if n_imu else t_last
    if end == "after":
        pcl_end = imu_end + 0.0031
    elif end == "before":
        pcl_end = imu_end - 0.0017
    elif end == "else":                      # imu_end_time <= pcl_beg_time
        beg = imu_end + 0.004
        pcl_end = beg + 0.0021
    else:                                    # pcl_end_time == pcl_beg_time
        pcl_end = beg
    u = np.array([2.0, -1.0, 2.0]) / 3.0
    state = make_state(rng, biases=rate not in ("zero", "0.9e-7", "1.1e-7"))
    mag = {"zero": 0.0, "0.9e-7": 0.9e-7, "1.1e-7": 1.1e-7, "6": 6.0, "mid": 0.7}[rate]
    gyr = mag * u + (rng.normal(0, 0.05, (n_imu + 1, 3)) if rate in ("6", "mid") else 0.0) * np.ones((n_imu + 1, 3))
    scale = acc_norm / G
    acc = (np.array([0.3, -0.2, 9.7]) + rng.normal(0, 0.5, (n_imu + 1, 3))) * scale
    imu = np.concatenate([stamps[:, None], acc[1:], gyr[1:]], 1) if n_imu else np.zeros((0, 7))
    carry = {"last_imu": np.concatenate([[t_last], acc[0], gyr[0]]), "acc_s_last": rng.normal(0, 0.5, 3),
             "angvel_last": mag * u if rate != "mid" else rng.normal(0, 0.3, 3), "last_lidar_end_time": last_end}
    return (imu, float(beg), float(pcl_end)), make_params(rng, acc_norm), carry, state


@functools.lru_cache(maxsize=None)
def edge_cases():
    """The ragged set: (name, job, params-key, carry, state).  One params per acc_norm (a batch shares
    its params), so the set is two batches."""
    out = []
    for n in SIZES:
        for lay in LAYOUTS:
            out.append((f"n{n}-{lay}", n, lay, "after", "mid"))
    for e in ENDS:
        for n in (0, 1, 20):
            out.append((f"n{n}-end-{e}", n, "later", e, "mid"))
    for r in RATES:
        out.append((f"n20-rate-{r}", 20, "later", "after", r))
        out.append((f"n20-rate-{r}-before", 20, "partial", "before", r))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def batch(acc_norm):
    """-> (names, jobs, params, carries, states) of edge_cases() at one |mean_acc| (1.0: g units)."""
    names, jobs, carries, states = [], [], [], []
    params = make_params(_rng("params", acc_norm), acc_norm)
    for name, n, lay, e, r in edge_cases():
        job, _, cy, st = make_case(n, lay, e, r, acc_norm)
        names.append(name)
        jobs.append(job)
        carries.append(cy)
        states.append(st)
    return names, jobs, params, carries, states


@functools.lru_cache(maxsize=None)
def batch_refs(acc_norm):
    """The two restatements of every job of batch(acc_norm), computed once: [(ref64, ref_ld)]."""
    _, jobs, params, carries, states = batch(acc_norm)
    return [(propagate(j, params, c, s, np.float64), propagate(j, params, c, s, LD))
            for j, c, s in zip(jobs, carries, states)]
