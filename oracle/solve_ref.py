"""High-precision restatement of one IEKF evaluation's solve, and the inputs that exercise it.

TEST INFRASTRUCTURE ONLY (like oracle.py).  solve() restates laser_mapping.cpp:187-227 literally
in mpmath at DPS digits, for any invertible covariance and with no symmetry assumed:

    K1 = (H18 + P^-1)^-1            H18(0:6, 0:6) = HTH (it carries 1 / LASER_POINT_COV already)
    G(:, 0:6) = K1(:, 0:6) HTH
    vec = prior [-] state           (common_lib.h:576-587)
    solution = K1(:, 0:6) HTL + vec - G(:, 0:6) vec(0:6)
    state [+] solution              (common_lib.h:565-574)
    cov = (I - G) P

Log / Exp follow so3_math.h:55-81: each branch is evaluated at full precision and the branch is
chosen at full precision.  The inputs are taken exactly from their doubles; the results are rounded
to float64 once, at the end.  The CPU oracle (two 18x18 pivoted LU inverses in double) and the
device solve (a factored 6x6 form) are both held against it.

dense_cov / full_prior / asym / indef / angle_cov build the covariances and priors of the sweep,
block_errors / cov_error / rot_error are its metrics.
"""
from __future__ import annotations

import mpmath as mp
import numpy as np

DPS = 60
DIM = 18
BLOCKS = ("rot", "pos", "vel", "bias_g", "bias_a", "gravity")  # solution rows 3 b .. 3 b + 2
ADDITIVE = BLOCKS[1:]

# standard deviations of a filter that has run: rot 1e-2 rad, pos 3e-2 m, vel 0.1 m/s,
# gyro bias 3e-4, accelerometer bias 3e-3, gravity 1e-3
VARIANCES = np.array([1e-4] * 3 + [1e-3] * 3 + [1e-2] * 3 + [1e-7] * 3 + [1e-5] * 3 + [1e-6] * 3)


def _mat(a, rows, cols):
    a = np.asarray(a, np.float64).reshape(rows, cols)
    return mp.matrix([[mp.mpf(float(a[i, j])) for j in range(cols)] for i in range(rows)])  # exact


def _np(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


def _hat(v):
    return mp.matrix([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def so3_log(R):
    """Log(R), so3_math.h:76-81."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    theta = mp.mpf(0) if tr > 3 - mp.mpf(1e-6) else mp.acos((tr - 1) / 2)
    K = [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]
    f = mp.mpf(0.5) if abs(theta) < mp.mpf(0.001) else theta / mp.sin(theta) / 2
    return [f * k for k in K]


def so3_exp(v):
    """Exp(v1, v2, v3), so3_math.h:55-72."""
    norm = mp.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    E = mp.eye(3)
    if norm > mp.mpf(0.00001):
        K = _hat([x / norm for x in v])
        E = E + mp.sin(norm) * K + (1 - mp.cos(norm)) * (K * K)
    return E


def solve(state: dict, prior: dict, HTH, HTL) -> dict:
    """One evaluation's solve.  HTH (6 x 6 or the oracle's 9 x 9) and HTL (6 or 9) as h_share returns them.
    Returns float64 arrays: solution (18), vec (18), rot (3 x 3), pos .. gravity (3), cov (18 x 18),
    and cond, the 2-norm condition number of H18 + P^-1."""
    with mp.workdps(DPS):
        C = _mat(np.asarray(HTH, np.float64)[:6, :6], 6, 6)
        h = _mat(np.asarray(HTL, np.float64).reshape(-1)[:6], 6, 1)
        P = _mat(state["cov"], DIM, DIM)
        A = P ** -1
        for i in range(6):
            for j in range(6):
                A[i, j] += C[i, j]
        K1 = A ** -1
        K6 = K1[:, 0:6]
        G6 = K6 * C
        Rs, Rp = _mat(state["rot"], 3, 3), _mat(prior["rot"], 3, 3)
        vec = so3_log(Rs.T * Rp)
        for k in ADDITIVE:
            a, b = _mat(prior[k], 3, 1), _mat(state[k], 3, 1)
            vec += [a[i] - b[i] for i in range(3)]
        vec = mp.matrix(vec)
        sol = K6 * h + vec - G6 * vec[0:6, 0]
        rot = Rs * so3_exp([sol[0], sol[1], sol[2]])
        cov = P - G6 * P[0:6, :]  # (I - G) P: G is zero outside its first six columns
        out = {"solution": _np(sol).ravel(), "vec": _np(vec).ravel(), "rot": _np(rot), "cov": _np(cov)}
        for b, k in enumerate(ADDITIVE, 1):
            s = _mat(state[k], 3, 1)
            out[k] = np.array([float(s[i] + sol[3 * b + i]) for i in range(3)])
        out["cond"] = float(np.linalg.norm(_np(A), 2) * np.linalg.norm(_np(K1), 2))
    return out


# ------------------------------------------------------------------ inputs ----
def dense_cov(seed: int, rho: float, variances=VARIANCES) -> np.ndarray:
    """A covariance with the scales of `variances` and the correlation (1 - rho) I + rho corr(A A^T),
    A ~ N(0, 1)^(n x n); exactly symmetric."""
    n = len(variances)
    A = np.random.default_rng(seed).standard_normal((n, n))
    S = A @ A.T
    d = np.sqrt(np.diag(S))
    corr = (1.0 - rho) * np.eye(n) + rho * (S / np.outer(d, d))
    sd = np.sqrt(np.asarray(variances, np.float64))
    P = corr * np.outer(sd, sd)
    return (P + P.T) / 2


def _rotvec(w):
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(w, np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


SKEW_AXIS = np.array([0.36, -0.48, 0.8])  # unit, no zero component


def full_prior(state: dict, angle: float = 0.037, axis=SKEW_AXIS) -> dict:
    """A prior that differs from the state in all six blocks: rotated by `angle` about `axis`
    (angle 0: the same rotation matrix), pos a few cm, vel 0.5, bias_g 1e-4, bias_a 1e-3, gravity 1e-3."""
    pr = {k: np.array(v, np.float64) for k, v in state.items()}
    axis = np.asarray(axis, np.float64)
    pr["rot"] = state["rot"] @ _rotvec(angle * axis / np.linalg.norm(axis))
    pr["pos"] = state["pos"] + np.array([0.031, -0.024, 0.017])
    pr["vel"] = state["vel"] + np.array([0.5, -0.37, 0.21])
    pr["bias_g"] = state["bias_g"] + np.array([1.0e-4, -0.6e-4, 0.8e-4])
    pr["bias_a"] = state["bias_a"] + np.array([-1.0e-3, 0.7e-3, 0.4e-3])
    pr["gravity"] = state["gravity"] + np.array([0.9e-3, 1.0e-3, -0.5e-3])
    return pr


def asym(P: np.ndarray, rel: float = 1e-6, seed: int = 1) -> np.ndarray:
    """P plus an antisymmetric perturbation E, |E_ij| = rel * (0.5 .. 1) * sqrt(P_ii P_jj), on the first
    six rows and columns: still a well-posed system, but not one a symmetric factorisation may take."""
    n = P.shape[0]
    U = np.triu(np.random.default_rng(seed).uniform(0.5, 1.0, size=(n, n)), 1)
    E = (U - U.T) * rel * np.sqrt(np.outer(np.diag(P), np.diag(P)))
    E[6:, 6:] = 0.0
    return P + E


def indef(P: np.ndarray) -> np.ndarray:
    """P with the pose block's smallest eigenvalue pushed just below zero (P66 - 1.0001 lmin v v^T):
    symmetric, no Cholesky factor, H18 + P^-1 still invertible."""
    lam, V = np.linalg.eigh(P[:6, :6])
    v = V[:, 0]
    Q = P.copy()
    Q[:6, :6] = P[:6, :6] - 1.0001 * lam[0] * np.outer(v, v)
    return (Q + Q.T) / 2


def angle_cov(seed: int = 3, rho: float = 0.5) -> np.ndarray:
    """dense_cov with the rotation block 1e-12 I and no rotation cross terms: the rotation rows of
    the gain vanish, solution(0:3) ~ vec(0:3), so Exp sees the angle Log returned."""
    P = dense_cov(seed, rho)
    P[:3, :] = 0.0
    P[:, :3] = 0.0
    P[:3, :3] = 1e-12 * np.eye(3)
    return P


VARIANTS = {"sym": lambda P: P, "asym": asym, "indef": indef}
_workload = None


def workload() -> dict:
    """The sweep's one scan: the smallest workload that still gives a well-posed 6 x 6 HTH (a 20k-point
    map, 1000 points of scan 60, about 900 of them effective).  map, body, state, the oracle's tree and
    its HTH / HTL at the state; built once."""
    global _workload
    if _workload is None:
        import oracle
        from livo_amd import synth
        m = synth.make_map(20_000)
        body, _, _ = synth.make_scan(1000, 60)
        st = synth.make_state(60)
        tree = oracle.Tree(m)
        r = tree.h_share(body, st["rot"], st["pos"], np.eye(3), synth.T_LI, True)
        _workload = {"map": m, "body": body, "state": st, "tree": tree, "HTH": r["HTH"], "HTL": r["HTL"],
                     "effct": r["effct"], "t_LI": synth.T_LI}
    return _workload


_cases = {}


def case(cov: np.ndarray, prior_angle=None) -> dict:
    """The workload's state with covariance `cov`, its prior (the state itself, or full_prior at
    prior_angle) and the reference solve of that input; cached by content, never modified."""
    key = (np.asarray(cov, np.float64).tobytes(), prior_angle)
    if key not in _cases:
        w = workload()
        st = dict(w["state"])
        st["cov"] = np.array(cov, np.float64)
        prior = st if prior_angle is None else full_prior(st, prior_angle)
        _cases[key] = {"state": st, "prior": prior, "ref": solve(st, prior, w["HTH"], w["HTL"])}
    return _cases[key]


def errors(sol, out: dict, c: dict) -> dict:
    """Every metric of one result (solution of the evaluation, the state after it) against c["ref"]."""
    ref = c["ref"]
    e = {"sol_" + k: v for k, v in block_errors(sol, ref["solution"]).items()}
    e["rot"] = rot_error(out["rot"], ref["rot"])
    e["cov"] = cov_error(out["cov"], ref["cov"], c["state"]["cov"])
    return e


# ----------------------------------------------------------------- metrics ----
def block_errors(sol, ref) -> dict:
    """Relative error of the solution per 3-block; a block whose reference is exactly 0 is skipped."""
    sol, ref = np.asarray(sol, np.float64).reshape(DIM), np.asarray(ref, np.float64).reshape(DIM)
    out = {}
    for b, k in enumerate(BLOCKS):
        n = np.linalg.norm(ref[3 * b:3 * b + 3])
        if n != 0.0:
            out[k] = float(np.linalg.norm(sol[3 * b:3 * b + 3] - ref[3 * b:3 * b + 3]) / n)
    return out


def cov_error(cov, ref, P) -> float:
    """max_ij |cov_ij - ref_ij| / sqrt(P_ii P_jj): every block at its own scale."""
    d = np.sqrt(np.abs(np.diag(np.asarray(P, np.float64))))
    return float((np.abs(np.asarray(cov) - np.asarray(ref)) / np.outer(d, d)).max())


def rot_error(rot, ref) -> float:
    return float(np.abs(np.asarray(rot) - np.asarray(ref)).max())
