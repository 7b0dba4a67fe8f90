"""The CPU oracle's IEKF solve against a 60-digit restatement (oracle/solve_ref.py), before anyone
trusts the oracle on the device: correlated covariances with scales from 1e-2 (velocity) to 1e-7
(gyro bias), a prior that differs from the state in every block, and covariances that no symmetric
factorisation may take.  One evaluation (max_iter = 0), which then stops and writes the covariance.

Metrics (solve_ref.errors): the solution's relative error per 3-block, max |d rot|, and the
covariance as max_ij |d cov_ij| / sqrt(P_ii P_jj).

Bar: 1e-12 on every metric: a few tens of times the symmetric sweep's worst error, which leaves
room for another libm or compiler without hiding a wrong formula.  The asym and indef covariances
are held to the same bar.  Measured here (g++ -O2, worst over the sweep, solution / covariance):
symmetric 1.6e-13 / 3.3e-14, asym 1.4e-13 / 3.2e-14, indef 3.3e-13 / 3.5e-13 with
cond(H18 + P^-1) up to 1.4e7.
"""
import numpy as np
import pytest

BAR = 1e-12
RHOS = (0.0, 0.5, 0.9, 0.99)
PRIORS = {"state": None, "full": 0.037}


def _oracle(c, w):
    out, stats = w["tree"].iekf_update(w["body"], c["state"], prior=c["prior"], R_LI=np.eye(3), t_LI=w["t_LI"],
                                       max_iter=0)
    assert stats["iterations"] == 1 and stats["effct_feat_num"][0] == w["effct"]
    return out, stats


@pytest.fixture(scope="module")
def work(built):
    import solve_ref
    w = solve_ref.workload()
    assert w["effct"] > 800
    return w


def test_reference_matches_numpy_on_diagonal_cov(work):
    """The restatement itself, where float64 is enough: P = 1e-3 I and prior = state, the form
    test_iekf_first_step_vs_numpy uses."""
    import solve_ref
    st = work["state"]
    ref = solve_ref.case(st["cov"])["ref"]
    H18 = np.zeros((18, 18))
    H18[:6, :6] = work["HTH"][:6, :6]
    K1 = np.linalg.inv(H18 + np.linalg.inv(st["cov"]))
    assert np.allclose(ref["solution"], K1[:, :6] @ work["HTL"][:6], rtol=1e-9, atol=1e-16)
    assert np.allclose(ref["cov"], (np.eye(18) - K1 @ H18) @ st["cov"], rtol=1e-9, atol=1e-16)
    assert np.all(ref["vec"] == 0)


@pytest.mark.parametrize("theta", [0.0, 5e-4, 0.9e-3, 1.1e-3, 0.05, 0.49, 0.51, 1.0, 3.0])
def test_reference_log_inverts_exp(theta):
    """Log(Exp(v)) in each branch of so3_math.h:55-81: v, or sin(t) / t of it from the small-angle
    branches, which return 0.5 K."""
    import mpmath as mp
    import solve_ref
    with mp.workdps(solve_ref.DPS):
        axis = [mp.mpf(float(x)) for x in solve_ref.SKEW_AXIS]
        n = mp.sqrt(sum(a * a for a in axis))
        v = [mp.mpf(theta) * a / n for a in axis]
        E = solve_ref.so3_exp(v)
        assert mp.norm(E.T * E - mp.eye(3)) < mp.mpf(10) ** -50
        got = solve_ref.so3_log(E)
        t = mp.mpf(theta)
        # below 1e-3 (the trace gate and the |theta| gate nearly coincide): 0.5 K = sin(t) / t * v
        f = mp.sin(t) / t if 0 < theta < 1e-3 else mp.mpf(1)
        assert max(abs(got[i] - f * v[i]) for i in range(3)) < mp.mpf(10) ** -45


def test_variants_leave_the_factored_class(work):
    """asym: the first six rows and columns differ from their transpose by ~1e-6 relative (cov_factor's
    gate is 1e-12).  indef: numpy's Cholesky of the pose block raises; the reference's system stays
    well conditioned."""
    import solve_ref
    for rho in RHOS:
        P = solve_ref.dense_cov(7, rho)
        assert np.array_equal(P, P.T) and np.all(np.linalg.eigvalsh(P) > 0)
        np.linalg.cholesky(P[:6, :6])
        A = solve_ref.asym(P)
        d = np.sqrt(np.diag(P))
        rel = np.abs(A - A.T) / np.outer(d, d)
        assert 0.9e-6 < rel[:6, 6:].min() and rel.max() < 2.1e-6 and np.all(rel[6:, 6:] == 0)
        assert np.abs(A - A.T)[:, :6].max() > 1e-12 * np.abs(A[:, :6]).max()
        Q = solve_ref.indef(P)
        assert np.array_equal(Q, Q.T)
        with pytest.raises(np.linalg.LinAlgError):
            np.linalg.cholesky(Q[:6, :6])
        assert solve_ref.case(Q)["ref"]["cond"] < 1e10


@pytest.mark.parametrize("variant", ["sym", "asym", "indef"])
@pytest.mark.parametrize("prior", list(PRIORS))
@pytest.mark.parametrize("rho", RHOS)
def test_oracle_solve_vs_reference(work, rho, prior, variant):
    import solve_ref
    P = solve_ref.VARIANTS[variant](solve_ref.dense_cov(7, rho))
    c = solve_ref.case(P, PRIORS[prior])
    out, stats = _oracle(c, work)
    err = solve_ref.errors(stats["solution"][0], out, c)
    print(f"rho={rho} prior={prior} {variant}: cond={c['ref']['cond']:.2e} "
          + " ".join(f"{k}={v:.1e}" for k, v in err.items()))
    if prior == "full":  # every block of vec is in play
        assert np.all(c["ref"]["vec"].reshape(6, 3).any(axis=1))
    diagonal = rho == 0 and prior == "state" and variant != "asym"  # solution rows 6..17 are exactly 0
    assert len(err) == (4 if diagonal else 8)
    for k in solve_ref.ADDITIVE:
        assert np.abs(out[k] - c["ref"][k]).max() <= BAR * max(np.abs(c["ref"][k]).max(), 1.0), k
    bad = {k: v for k, v in err.items() if not v < BAR}
    assert not bad, (bad, c["ref"]["cond"])
