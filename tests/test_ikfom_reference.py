"""The 60-digit restatement of the IKFoM update (oracle/ikfom_ref.py) against independent facts, and
the CPU oracle's IKFoM path against it, before anyone trusts the oracle on the device.

The facts: boxplus / boxminus invert each other and keep gravity on its sphere; A_matrix is the
derivative of Exp; S2_Nx_yy * S2_Mx is the derivative of delta -> (x_prop [+] delta) [-] x once
exp_delta gets the scale 1 / 2 its author meant (as written, scalar(1 / 2) is 0 and the factor is
missing: the restatement, the oracle and the kernel keep what is written); the two gain forms are
one update.  The finite difference of Exp uses a step of 1e-20, which 60 digits allow.

The sweep (ikfom_ref.CASES) leaves the points where the manifold code degenerates: offset_R 20
degrees about a skew axis, gravity in a generic direction and exactly at the S2_Bx pole (-L, 0, 0),
dense and asymmetric covariances that move gravity and the extrinsics by 1e-3 .. 1e-2 rad, a first
rotation step on either side of the Taylor switch of cos_sinc_sqrt (0.0221 rad), non-zero vel / bg /
ba, and 1 / 22 / 23 / 24 effective rows around the switch of the gain form.  Each case is evaluated
twice: max_iter = 0 (x = x_prop, dx_new = 0) and the second evaluation of max_iter = 1, entered from
the oracle's own first step, where dx_new != 0 drives A_matrix, S2_Nx_yy and S2_Mx off the identity.

Bar for the oracle (_bound): rounding of its double algebra through the condition number the
reference returns, 8 N eps cond((P_ / R)^-1 + HTH) (two N x N inversions and three products of
N-term sums), times |dx_new| / |block| for dx_ = K_h + (K_x - I) dx_new, which cancels when the
filter has nearly converged.

Measured here (g++ -O2; worst over the sweep and both evaluations, cond up to 3.0e5):
    dx_pos 2.7e-10  dx_rot 5.1e-11  dx_offset_R 1.1e-10  dx_offset_T 1.0e-11  dx_vel 4.9e-11
    dx_bg 4.7e-11  dx_ba 1.1e-11  dx_grav 1.4e-11  q_rot 8.3e-14  q_offset_R 1.2e-13  grav 3.0e-14
    cov 3.1e-10
These maxima are the floors of tests/test_gpu_ikfom_manifold.py (FLOOR); the last test here holds
the two together.
"""
import mpmath as mp
import numpy as np
import pytest

EPS = 2.0 ** -52


def _ir():
    import ikfom_ref
    return ikfom_ref


@pytest.fixture(scope="module")
def work(built):
    import solve_ref
    return solve_ref.workload()


def _unit(rng, n):
    v = rng.normal(size=n)
    return v / np.linalg.norm(v)


def _steps(ir):
    s = ir.TAYLOR_SWITCH
    return (1e-3, 0.99 * s, 1.01 * s, 0.5)


# ------------------------------------------------------ the manifold pieces ----
@pytest.mark.parametrize("grav", ["generic", "down", "pole"])
def test_boxplus_boxminus_roundtrip_and_s2_length(grav):
    """(x [+] dx) [-] x = dx and |grav| = L, with the SO3 and S2 steps on both sides of the Taylor
    switch.  The Taylor side is a polynomial of degree 3 in x2 <= 2^-13: it misses cos and sinc by
    x2^4 / 8! ~ 5e-21, so that side is held to 1e-18 and the library side to 1e-50."""
    ir = _ir()
    from livo_amd import synth
    rng = np.random.default_rng(5)
    st = synth.make_ikfom_state(2, offset_R=ir.quat_about(ir.TILT_AXIS, 20.0), grav=ir.grav_of(grav))
    with mp.workdps(ir.DPS):
        x = ir._state(st)
        x["grav"] = [v * ir._L / ir._norm(x["grav"]) for v in x["grav"]]  # on the sphere to 60 digits, not 16
        for step in _steps(ir):
            dx = rng.normal(size=23) * 0.05
            dx[3:6], dx[6:9], dx[21:23] = step * _unit(rng, 3), step * _unit(rng, 3), step * _unit(rng, 2)
            tol = mp.mpf(10) ** (-50 if step >= ir.TAYLOR_SWITCH else -18)
            y = ir.boxplus(x, ir._vec(dx))
            back = ir.boxminus(y, x)
            assert max(abs(b - mp.mpf(float(d))) for b, d in zip(back, dx)) < tol, step
            assert abs(ir._norm(y["grav"]) - ir._L) < tol * 10, step
            if step < ir.TAYLOR_SWITCH:  # the truncation is there: the branch was taken
                assert abs(ir._norm(y["rot"]) - 1) > mp.mpf(10) ** -40


@pytest.mark.parametrize("theta", [0.05, 0.7, 3.0])
def test_A_matrix_is_the_derivative_of_exp(theta):
    """Exp(v + d) Exp(v)^-1 = Exp(A(v) d) + O(d^2), |d| = 1e-20 (library side of the switch)."""
    ir = _ir()
    rng = np.random.default_rng(3)
    with mp.workdps(ir.DPS):
        v = ir._vec(theta * _unit(rng, 3))
        A = ir.A_matrix(v)
        for _ in range(3):
            u = ir._vec(_unit(rng, 3))
            d = [mp.mpf(10) ** -20 * c for c in u]
            q = ir.qmul(ir.so3_exp([a + b for a, b in zip(v, d)]), ir.qconj(ir.so3_exp(v)))
            want = A * ir._col(d)
            assert max(abs(2 * q[1 + i] - want[i]) for i in range(3)) < mp.mpf(10) ** -38
        assert ir.A_matrix([mp.mpf(0)] * 3) == mp.eye(3)


@pytest.mark.parametrize("grav", ["generic", "down", "pole"])
@pytest.mark.parametrize("step", [0.0, 2e-3, 0.3])
def test_Nx_Mx_against_finite_difference(grav, step):
    """J = S2_Nx_yy(x) S2_Mx(x_prop, seg) at x = x_prop [+] seg against the finite difference of
    delta -> (x_prop [+] delta) [-] x at delta = seg.  With exp_delta at scale 1 / 2 the two agree to
    the step; as written (scale 0) J lacks the rotation Exp(Bx seg) between hat(vec)
    and Nx, exactly, and agrees only at seg = 0."""
    ir = _ir()
    rng = np.random.default_rng(9)
    with mp.workdps(ir.DPS):
        xp = ir._vec(ir.grav_of(grav))
        xp = [v * ir._L / ir._norm(xp) for v in xp]  # on the sphere to 60 digits
        seg = ir._vec(step * _unit(rng, 2))
        x = ir.s2_boxplus(xp, seg)
        N = ir.s2_Nx_yy(x)
        # boxminus returns 0 below v_sin = L^2 sin(theta) = 1e-11 (its tolerance branch, taken at x [-] x):
        # a step of 1e-20 never leaves it, so this is a central difference at 1e-8, good to ~1e-16
        assert ir.s2_boxminus(x, x) == [0, 0]
        hstep = mp.mpf(10) ** -8
        fd = mp.zeros(2, 2)
        for j in range(2):
            lo, hi = list(seg), list(seg)
            lo[j] -= hstep
            hi[j] += hstep
            a, b = ir.s2_boxminus(ir.s2_boxplus(xp, lo), x), ir.s2_boxminus(ir.s2_boxplus(xp, hi), x)
            for i in range(2):
                fd[i, j] = (b[i] - a[i]) / (2 * hstep)
        meant = N * ir.s2_Mx(xp, seg, mp.mpf(1) / 2)
        assert mp.norm(meant - fd, mp.inf) < mp.mpf(10) ** -14
        written = N * ir.s2_Mx(xp, seg)
        if step == 0.0:
            assert written == meant
        else:
            Bu = list(ir.s2_Bx(xp) * ir._col(seg))
            E = ir.qmat(ir.mtk_exp(Bu, mp.mpf(1) / 2))
            assert mp.norm(N * E * (-ir.hat(xp)) * ir.A_matrix(Bu).T * ir.s2_Bx(xp) - meant, mp.inf) < mp.mpf(10) ** -50
            assert mp.norm(N * (-ir.hat(xp)) * ir.A_matrix(Bu).T * ir.s2_Bx(xp) - written, mp.inf) < mp.mpf(10) ** -50
            assert mp.norm(written - meant, mp.inf) > mp.mpf(step) ** 2 / 100  # the missing factor shows


@pytest.mark.parametrize("name", ["rows22", "rows24"])
def test_gain_forms_are_one_update(work, name):
    """The measurement-space and the information form on one input: the same dx_ and K_x to the
    reference's precision (60 digits less the condition number)."""
    ir = _ir()
    c = ir.case(name)
    st = c["state"]
    entry = _oracle_case(name, work)["entry"]  # dx_new != 0
    H, h, _ = ir.rows(entry, c["body"], work["tree"])
    a = ir.evaluate(entry, st, st["cov"], H, h, form="meas")
    b = ir.evaluate(entry, st, st["cov"], H, h, form="info")
    assert a["form"] == "meas" and b["form"] == "info" and np.linalg.norm(a["dx_new"]) > 1e-3
    # (both are rounded to float64 once: equal to an ulp of the largest entry)
    assert np.abs(a["dx"] - b["dx"]).max() <= np.spacing(np.abs(a["dx"]).max())
    assert np.abs(a["K_x"] - b["K_x"]).max() <= np.spacing(np.abs(a["K_x"]).max())
    assert np.abs(a["cov"] - b["cov"]).max() <= np.spacing(np.abs(a["cov"]).max())


# ------------------------------------------------- oracle against reference ----
_cache = {}
_maxima = {}


def _oracle_case(name, work):
    """The oracle's max_iter = 0 and 1 runs of case `name`, the reference at the same inputs (the
    second evaluation entered from the oracle's own first step) and the oracle's errors; once."""
    if name not in _cache:
        ir = _ir()
        c = ir.case(name)
        st, body, tree = c["state"], c["body"], work["tree"]
        o0, s0 = tree.ikfom_update(body, st, max_iter=0)
        o1, s1 = tree.ikfom_update(body, st, max_iter=1)
        ref0 = ir.reference(st, st, body, tree)
        entry = dict(o0)
        entry["cov"] = st["cov"]
        ref1 = ir.reference(entry, st, body, tree)
        e0 = ir.errors(s0["dx"][0], o0, ref0, st["cov"])
        e1 = ir.errors(s1["dx"][1], o1, ref1, st["cov"])
        for e in (e0, e1):
            for k, v in e.items():
                _maxima[k] = max(_maxima.get(k, 0.0), v)
        _cache[name] = {"case": c, "o0": o0, "s0": s0, "o1": o1, "s1": s1, "ref0": ref0, "ref1": ref1,
                        "entry": entry, "e0": e0, "e1": e1}
    return _cache[name]


def _bound(ir, ref, metric):
    """See the module docstring."""
    base = 8 * ir.N * EPS * ref["cond"]
    if metric == "cov":
        return base
    moved = np.linalg.norm(ref["dx_new"]) + np.linalg.norm(ref["dx"])
    if not metric.startswith("dx_"):  # a distance between states: the step's error, and the state's own rounding
        return base * moved + 4 * EPS
    a, b = next((a, b) for k, a, b in ir.BLOCKS if "dx_" + k == metric)
    own, whole = np.linalg.norm(ref["dx"][a:b]), np.linalg.norm(ref["dx"])
    return base * moved / (own if own >= 1e-6 * whole else whole)


@pytest.mark.parametrize("name", list(_ir().CASES))
def test_oracle_vs_reference(work, name):
    ir = _ir()
    r = _oracle_case(name, work)
    c, s0, s1, ref0, ref1 = r["case"], r["s0"], r["s1"], r["ref0"], r["ref1"]
    offR, grav, cov, rot_deg, vbb, want = ir.CASES[name]
    # the case is what it says
    assert s0["iterations"] == 1 and s1["iterations"] == 2 and s1["knn_passes"] == 2
    assert np.array_equal(s1["dx"][0], s0["dx"][0])
    assert s0["effct_feat_num"] == [ref0["effct"]] and s1["effct_feat_num"] == [ref0["effct"], ref1["effct"]]
    if want is None:
        assert len(c["body"]) == 1000 and ref0["effct"] > 800
    else:
        assert ref0["effct"] == want
    assert ref0["form"] == ("meas" if ref0["effct"] < 23 else "info")
    step = np.linalg.norm(ref0["dx"][3:6])
    assert (step > 1.2 * ir.TAYLOR_SWITCH) if rot_deg == 5.0 and want is None else (step < 0.99 * ir.TAYLOR_SWITCH), step
    assert np.all(ref0["dx_new"] == 0) and np.linalg.norm(ref1["dx_new"]) > 1e-4
    moved = cov != "diag"  # cross terms: gravity, vel and the biases move
    assert (np.linalg.norm(ref0["dx"][21:23]) > 1e-4) == moved
    assert (np.linalg.norm(ref0["dx"][12:21]) > 1e-4) == moved
    if moved:
        assert 1e-3 < np.linalg.norm(ref0["dx"][6:9]) < 3e-2
    if grav == "generic":
        with mp.workdps(ir.DPS):
            assert all(abs(v) > 0.05 for v in ir.s2_Bx(ir._vec(c["state"]["grav"])))
    for tag, e, ref in (("eval 0", r["e0"], ref0), ("eval 1", r["e1"], ref1)):
        print(f"{name} {tag}: rows={ref['effct']} {ref['form']} cond={ref['cond']:.1e} "
              + " ".join(f"{k}={v:.1e}" for k, v in e.items()))
        bad = {k: (v, _bound(ir, ref, k)) for k, v in e.items() if not v <= _bound(ir, ref, k)}
        assert len(e) == 12 and not bad, (tag, bad, ref["cond"])
    print("maxima so far: " + " ".join(f"{k}={v:.1e}" for k, v in _maxima.items()))


def test_recorded_maxima(work):
    """The oracle's worst errors over the whole sweep against the floors the GPU test uses: a floor is
    the measured maximum, rounded up (it may not drift above 4 x what is measured here, nor the
    measurement above 2 x the floor)."""
    from test_gpu_ikfom_manifold import FLOOR
    for name in _ir().CASES:
        _oracle_case(name, work)
    print("oracle against reference, maxima over the sweep:")
    for k, v in _maxima.items():
        print(f"    {k:14s} {v:.2e}   floor {FLOOR[k]:.1e}")
    assert set(FLOOR) == set(_maxima)
    bad = {k: (v, FLOOR[k]) for k, v in _maxima.items() if not (v <= 2 * FLOOR[k] and FLOOR[k] <= 4 * v)}
    assert not bad, bad
