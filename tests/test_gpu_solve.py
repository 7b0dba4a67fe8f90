"""The device's IEKF solve (solve_scan) against the 60-digit restatement of
oracle/solve_ref.py, on the inputs a diagonal covariance never produces: correlated covariances
with scales from 1e-2 to 1e-7 (the lower rows of B, the triangles of C L and L^T C L), covariances
the host cannot factor (the pivoted 6x6 LU branch), priors that differ from the state in every
block, and rotation angles on both sides of every threshold of sincos_short, acos_near1 and Log.

Workload: solve_ref.workload() -- a 20k-point map and 1000 points of scan 60, one evaluation
(max_iterations = 0) unless a test says otherwise.

Metrics (solve_ref.errors): the solution's relative error per 3-block, max |d rot|, the covariance
as max_ij |d cov_ij| / sqrt(P_ii P_jj).  The bar for the device, per metric and per case, is

    max(100 x the oracle's own error against the reference on that input, 1e-11)

1e-11 is the agreement DESIGN.md claims; the factor 100 is there because the device's algebra is a
different form (a 6x6 factored system), not the oracle's two 18x18 inverses re-ordered.  The
oracle's error is computed here and printed with the device's when a case fails.

Later evaluations of a multi-evaluation update (the mixed batch) have no reference of their own:
the device and the oracle enter them from states that already differ by the first evaluation's
error, and the evaluation maps a state difference to a solution difference of the same size, with
the lever arm of the scan (up to 30 m over a 0.1 m step) between the rotation and position blocks.
They are held to the oracle at BAR_LATER = 1e-9 = 100 x 1e-11 of the largest norm the block's
solution has had so far (the scale of the state's change); counts are exact.  (World points are
rounded to float32: a state difference of 1e-12 m flips such a rounding with probability ~1e-6 per
coordinate; a flip would show as ~1e-7 here and is not allowed for.)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLOOR = 1e-11
BAR_LATER = 1e-9
RHOS = (0.0, 0.5, 0.9, 0.99)
PRIORS = {"state": None, "full": 0.037}
# both sides of: Log's trace gate and |theta| < 1e-3, acos_near1's 0.99 (theta = 0.14154), sincos_short's
# 0.5, with the library branches beyond; each at least 1e-3 relative away from its threshold
ANGLES = (0.0, 5e-4, 0.9e-3, 1.1e-3, 0.05, 0.141, 0.142, 0.49, 0.51, 1.0, 3.0)


def _sr():
    import solve_ref
    return solve_ref


def _bits(x):
    return np.asarray(x).tobytes()


@pytest.fixture(scope="module")
def work(built):
    return _sr().workload()


def _ctx(max_iter=0):
    import livo_amd
    from livo_amd import synth
    return livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=max_iter)


@pytest.fixture(scope="module")
def sctx(work):
    """One context on the static map, the scan resident, one evaluation per update."""
    with _ctx() as ctx:
        ctx.map_build(work["map"])
        yield ctx, ctx.scan_upload(work["body"])


_orc = {}


def _oracle_errors(c, work):
    """The oracle's own errors on case c (computed once per case)."""
    key = id(c)
    if key not in _orc:
        out, stats = work["tree"].iekf_update(work["body"], c["state"], prior=c["prior"], R_LI=np.eye(3),
                                              t_LI=work["t_LI"], max_iter=0)
        _orc[key] = (c, _sr().errors(stats["solution"][0], out, c))
    return _orc[key][1]


def _bars(orc_err):
    return {k: max(100.0 * v, FLOOR) for k, v in orc_err.items()}


def _ulp2(x):
    return 2 * np.spacing(np.abs(np.asarray(x, np.float64)).max())


def _hold(out, stats, c, work, bars=None):
    """One device evaluation against c["ref"] at the bars; returns (errors, bars)."""
    sr = _sr()
    assert stats["iterations"] == 1 and stats["effct_feat_num"] == [work["effct"]]
    orc = _oracle_errors(c, work)
    bars = bars or _bars(orc)
    err = sr.errors(stats["solution"][0], out, c)
    assert set(err) == set(orc)
    print("device/oracle " + " ".join(f"{k}={err[k]:.1e}/{orc[k]:.1e}" for k in err))
    bad = {k: (err[k], bars[k], orc[k]) for k in err if not err[k] <= bars[k]}
    assert not bad, f"metric: (device, bar, oracle) {bad}; cond {c['ref']['cond']:.2e}"
    ref = c["ref"]
    for b, k in enumerate(sr.ADDITIVE, 1):  # state [+] solution, both sums rounded once
        tol = bars.get("sol_" + k, 0.0) * np.linalg.norm(ref["solution"][3 * b:3 * b + 3]) + _ulp2(ref[k])
        assert np.abs(out[k] - ref[k]).max() <= tol, k
    return err, bars


# ------------------------------------------------------ dense covariance ----
@pytest.mark.parametrize("prior", list(PRIORS))
@pytest.mark.parametrize("rho", RHOS)
def test_dense_covariance(sctx, work, rho, prior):
    """The factored path on a correlated covariance, default kernel, against the reference."""
    sr = _sr()
    ctx, sid = sctx
    c = sr.case(sr.dense_cov(7, rho), PRIORS[prior])
    out, stats = ctx.iekf_update(sid, c["state"], c["prior"])
    err, bars = _hold(out, stats, c, work)
    if rho > 0:  # B's lower rows are in play: rows 6..17 of the solution are not vec alone
        sol, ref = stats["solution"][0], c["ref"]
        for b in range(2, 6):
            k, s = "sol_" + sr.BLOCKS[b], slice(3 * b, 3 * b + 3)
            moved = np.linalg.norm(sol[s] - ref["vec"][s]) / np.linalg.norm(ref["solution"][s])
            assert moved > 100 * bars[k], (k, moved)
    else:
        assert np.array_equal(stats["solution"][0][6:], c["ref"]["vec"][6:])


# ---------------------------------------------------------- the LU path ----
@pytest.mark.parametrize("variant", ["sym", "asym", "indef"])
@pytest.mark.parametrize("rho", (0.5, 0.99))
def test_lu_path(sctx, work, rho, variant):
    """asym / indef: cov_factor refuses the covariance and the device takes the pivoted 6x6 LU.
    asym differs from its symmetric part by 1e-6: a solve that took the factored path would miss
    the bar by five orders.  The same symmetric P through the factored path agrees with its own
    reference, so the two branches are pinned on one dataset."""
    sr = _sr()
    ctx, sid = sctx
    P = sr.dense_cov(7, rho)
    c = sr.case(sr.VARIANTS[variant](P), PRIORS["full"])
    out, stats = ctx.iekf_update(sid, c["state"], c["prior"])
    err, bars = _hold(out, stats, c, work)
    if variant == "asym":  # the two references are apart by far more than the bars
        sym = sr.case(P, PRIORS["full"])["ref"]
        apart = sr.block_errors(c["ref"]["solution"], sym["solution"])
        assert max(apart.values()) > 1e3 * max(bars.values()), apart
    if variant == "indef":
        with pytest.raises(np.linalg.LinAlgError):
            np.linalg.cholesky(c["state"]["cov"][:6, :6])
        assert c["ref"]["cond"] < 1e10


# --------------------------------------------------------------- angles ----
@pytest.mark.parametrize("theta", ANGLES)
def test_angles(sctx, work, theta):
    """The prior rotated by theta about a skew axis, the covariance's rotation block 1e-12 I:
    solution(0:3) ~ vec(0:3), so Exp sees the angle Log returned."""
    sr = _sr()
    ctx, sid = sctx
    c = sr.case(sr.angle_cov(), theta)
    ref = c["ref"]
    assert abs(np.linalg.norm(ref["vec"][:3]) - (theta if theta >= 1e-3 else np.sin(theta))) <= 1e-12
    assert abs(np.linalg.norm(ref["solution"][:3]) - np.linalg.norm(ref["vec"][:3])) < 1e-6 + 2e-5 * theta
    out, stats = ctx.iekf_update(sid, c["state"], c["prior"])
    _hold(out, stats, c, work)
    assert np.abs(out["rot"].T @ out["rot"] - np.eye(3)).max() < 1e-14


# --------------------------------------------------- every caller of it ----
def _one(work, c, **env):
    def run(monkeypatch):
        for k in ("LIVO_EVAL_GEN", "LIVO_FUSED"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with _ctx() as ctx:
            ctx.map_build(work["map"])
            return ctx.iekf_update(ctx.scan_upload(work["body"]), c["state"], c["prior"])
    return run


def test_callers_static_map(sctx, work, monkeypatch):
    """solve_scan<true> in the static kernel (default), in the generic kernel (LIVO_EVAL_GEN=1) and
    solve_scan<false> behind k_reduce_solve (LIVO_FUSED=0, lane 0 forms vec): bit-equal, and within
    the bars of the reference."""
    sr = _sr()
    ctx, sid = sctx
    c = sr.case(sr.dense_cov(7, 0.9), PRIORS["full"])
    base = ctx.iekf_update(sid, c["state"], c["prior"])
    _hold(base[0], base[1], c, work)
    for env in ({"LIVO_EVAL_GEN": "1"}, {"LIVO_FUSED": "0"}):
        out, stats = _one(work, c, **env)(monkeypatch)
        assert _bits(stats["solution"]) == _bits(base[1]["solution"]), env
        for k in base[0]:
            assert _bits(out[k]) == _bits(base[0][k]), (env, k)


def _hold_to_oracle(out, stats, r_out, r_stats, c, bars):
    """A caller whose map is not the workload's: the device against that map's own oracle."""
    sr = _sr()
    assert stats["iterations"] == r_stats["iterations"] == 1
    assert stats["effct_feat_num"] == r_stats["effct_feat_num"] and stats["effct_feat_num"][0] > 300
    err = {"sol_" + k: v for k, v in sr.block_errors(stats["solution"][0], r_stats["solution"][0]).items()}
    err["rot"] = sr.rot_error(out["rot"], r_out["rot"])
    err["cov"] = sr.cov_error(out["cov"], r_out["cov"], c["state"]["cov"])
    bad = {k: (err[k], bars[k]) for k in err if not err[k] <= bars[k]}
    assert len(err) == 8 and not bad, bad


def test_caller_incremental_map(work):
    """A map made incremental by map_add_points (the generic kernel, the dynamic search) against
    DynMap's update.  Bars: those of the same covariance and prior on the static map."""
    import oracle
    sr = _sr()
    from livo_amd import synth
    c = sr.case(sr.dense_cov(7, 0.9), PRIORS["full"])
    bars = _bars(_oracle_errors(c, work))
    add, _, _ = synth.make_scan(2000, 61)
    st1 = synth.make_state(61)
    W = ((add.astype(np.float64) + synth.T_LI) @ st1["rot"].T + st1["pos"]).astype(np.float32)
    dm = oracle.DynMap(work["map"])
    with _ctx() as ctx:
        ctx.map_build(work["map"])
        g = ctx.map_add_points(W, 0.5)
        r = dm.add_points(W, 0.5)
        assert {k: g[k] for k in r} == r and r["added"] > 0
        out, stats = ctx.iekf_update(ctx.scan_upload(work["body"]), c["state"], c["prior"])
    r_out, r_stats = dm.iekf_update(work["body"], c["state"], prior=c["prior"], t_LI=synth.T_LI, max_iter=0)
    _hold_to_oracle(out, stats, r_out, r_stats, c, bars)


def test_caller_ivox(work):
    """The iVox backend's iekf_update: its own oracle gives HTH / HTL at the state, so the device
    and that oracle are both held against the reference of this input."""
    import livo_amd
    import oracle
    sr = _sr()
    from livo_amd import synth
    kw = {"resolution": 1.0, "nearby_type": 18}  # (the 20k-point map is sparse: metre cells)
    iv = oracle.Ivox(**kw)
    iv.add_points(work["map"])
    body = work["body"]
    c0 = sr.case(sr.dense_cov(7, 0.9), PRIORS["full"])
    st, prior = c0["state"], c0["prior"]
    hs = iv.h_share(body, st["rot"], st["pos"], np.eye(3), synth.T_LI, True, oracle.new_cache(len(body)))
    assert hs["effct"] > 300
    c = {"state": st, "prior": prior, "ref": sr.solve(st, prior, hs["HTH"], hs["HTL"])}
    r_out, r_stats = iv.iekf_update(body, st, oracle.new_cache(len(body)), prior=prior, t_LI=synth.T_LI, max_iter=0)
    bars = _bars(sr.errors(r_stats["solution"][0], r_out, c))
    with _ctx() as ctx:
        ctx.set_backend(livo_amd.BACKEND_IVOX)
        ctx.ivox_init(**kw)
        ctx.ivox_add_points(work["map"])
        out, stats = ctx.iekf_update(ctx.scan_upload(body), st, prior)
    assert stats["iterations"] == 1 and stats["effct_feat_num"] == [hs["effct"]]
    err = sr.errors(stats["solution"][0], out, c)
    bad = {k: (err[k], bars[k]) for k in err if not err[k] <= bars[k]}
    assert len(err) == 8 and not bad, bad


# ----------------------------------------------------------- mixed batch ----
def test_mixed_batch(work):
    """Six scans (sizes of test_gpu_eval_kinds.SIZES, the empty and the one-point scan among them),
    their slots alternating among a diagonal, a dense, an asym and an indef covariance, four
    iterations: per-slot cov_ok, the host-slot writeback of a dense cov, vec over several
    evaluations.  Synchronous and submitted batches are bit-equal to the single updates; the first
    evaluation is held against the reference, the later ones against the oracle (BAR_LATER)."""
    from livo_amd import synth
    from test_gpu_eval_kinds import SIZES
    sr = _sr()
    dense = sr.dense_cov(7, 0.9)
    # 1000 points dense, 0 indef, 1 diagonal, 63 asym, 64 dense, 257 indef
    covs = [dense, sr.indef(sr.dense_cov(7, 0.99)), np.eye(18) * 1e-3, sr.asym(sr.dense_cov(7, 0.5))]
    scans, states, priors = [], [], []
    for k, n in enumerate(SIZES):
        scans.append(synth.make_scan(n, 60 + k)[0])
        st = synth.make_state(60 + k)
        st["cov"] = covs[k % 4]
        states.append(st)
        priors.append(sr.full_prior(st))
    assert [len(s) for s in scans] == list(SIZES) and np.array_equal(scans[0], work["body"])
    with _ctx(4) as ctx:
        ctx.map_build(work["map"])
        sids = [ctx.scan_upload(s) for s in scans]
        single = [ctx.iekf_update(s, st, pr) for s, st, pr in zip(sids, states, priors)]
        sync = ctx.iekf_update_batch(sids, states, priors)
        t = ctx.iekf_update_batch_submit(sids, states, priors)
        sub = ctx.iekf_update_batch_wait(t, len(sids))
    for name, (b_out, b_stats) in (("sync", sync), ("submit", sub)):
        for k, (out, stats) in enumerate(single):
            for key in out:
                assert _bits(b_out[k][key]) == _bits(out[key]), (name, k, key)
            for key in ("iterations", "knn_passes", "converged", "rematch_num", "effct_feat_num"):
                assert b_stats[k][key] == stats[key], (name, k, key)
            assert _bits(b_stats[k]["solution"]) == _bits(stats["solution"]), (name, k)
    tree = work["tree"]
    for k, (out, stats) in enumerate(single):
        st, pr, body = states[k], priors[k], scans[k]
        r_out, r_stats = tree.iekf_update(body, st, prior=pr, R_LI=np.eye(3), t_LI=synth.T_LI, max_iter=4)
        for key in ("iterations", "knn_passes", "converged", "rematch_num", "effct_feat_num"):
            assert stats[key] == r_stats[key], (k, key)
        # the first evaluation: device and oracle against the reference of this slot's input
        hs = tree.h_share(body, st["rot"], st["pos"], np.eye(3), synth.T_LI, True)
        assert hs["effct"] == stats["effct_feat_num"][0]
        ref = sr.solve(st, pr, hs["HTH"], hs["HTL"])
        e_orc = sr.block_errors(r_stats["solution"][0], ref["solution"])
        e_dev = sr.block_errors(stats["solution"][0], ref["solution"])
        bad = {b: (e_dev[b], e_orc[b]) for b in e_dev if not e_dev[b] <= max(100 * e_orc[b], FLOOR)}
        assert len(e_dev) == 6 and not bad, (k, bad)
        # later evaluations and the state they leave: against the oracle, per block, at the
        # scale of the block's change so far
        scale = np.zeros(6)
        for e in range(stats["iterations"]):
            rs = r_stats["solution"][e].reshape(6, 3)
            scale = np.maximum(scale, np.linalg.norm(rs, axis=1))
            d = np.linalg.norm(stats["solution"][e].reshape(6, 3) - rs, axis=1)
            assert np.all(d <= BAR_LATER * scale), (k, e, d / scale)
        assert sr.rot_error(out["rot"], r_out["rot"]) <= BAR_LATER * max(scale[0], 1e-3), k
        for b, key in enumerate(sr.ADDITIVE, 1):
            assert np.abs(out[key] - r_out[key]).max() <= BAR_LATER * scale[b] + _ulp2(r_out[key]), (k, key)
        assert sr.cov_error(out["cov"], r_out["cov"], st["cov"]) <= BAR_LATER, k
        if stats["effct_feat_num"][-1] > 0:  # (the stopping evaluation wrote it)
            assert not np.array_equal(out["cov"], st["cov"])


# ------------------------------------------------------- VIO and IKFoM ----
def test_vio_dense_covariance(built):
    """wave_lu_to_lds<6> of the photometric update on a correlated covariance and a prior that
    differs in every block; device against oracle at test_gpu_vio's bars."""
    import livo_amd
    import oracle
    from livo_amd import synth
    from test_gpu_vio import _check
    sr = _sr()
    fr, st, _ = synth.make_vio_frame(1500, 4)
    with livo_amd.Context(0) as ctx:
        for rho in (0.5, 0.99):
            st = dict(st)
            st["cov"] = sr.dense_cov(11, rho)
            prior = sr.full_prior(st, 0.004)
            _check(ctx.vio_update(fr, st, prior), oracle.vio_update(fr, st, prior))


@pytest.mark.parametrize("n", [12, 40, 1000])
def test_ikfom_dense_covariance(work, n):
    """wave_lu_to_lds<22> / <23> (the only users of the pivot search's cross-row step) on a
    correlated 23x23 covariance: 12 points take the measurement-space gain, 40 and 1000 the
    information form; device against oracle at test_gpu_ikfom's bars."""
    from livo_amd import synth
    from test_gpu_ikfom import _compare
    sr = _sr()
    body = work["body"][:n]
    st0 = synth.make_ikfom_state(60)
    st0["cov"] = sr.dense_cov(13, 0.9, np.diag(synth.ikfom_cov()))
    with _ctx(4) as ctx:
        ctx.map_build(work["map"])
        g, gs = ctx.ikfom_update(ctx.scan_upload(body), st0)
    r, rs = work["tree"].ikfom_update(body, st0, max_iter=4)
    assert gs["effct_feat_num"][0] > 0
    _compare(g, gs, r, rs, st0)
