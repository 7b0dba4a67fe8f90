"""The device's IKFoM update (k_hshare_ik, ik_prep, ik_solve and the s2_* / so3_* pieces of
livo_kernels.hip) against the 60-digit restatement of oracle/ikfom_ref.py, on the sweep of
tests/test_ikfom_reference.py: a tilted offset_R, gravity in a generic direction and at the S2_Bx
pole, dense and asymmetric covariances, rotation steps on both sides of the Taylor switch, non-zero
vel / bg / ba, and 1 / 22 / 23 / 24 effective rows around the switch of the gain form.
(test_gpu_ikfom.py holds the device to the oracle, at inputs where every one of these is trivial.)

Workload: solve_ref.workload() -- a 20k-point map and (a prefix of) 1000 points of scan 60.

Evaluation 0: max_iterations = 0.  x = x_prop, dx_new = 0, the covariance is written at dx_.
Evaluation 1: max_iterations = 1.  The device is deterministic, so its first evaluation is bitwise
that of the max_iterations = 0 run (asserted), and its second one enters from that run's output
state; the reference evaluates at exactly that state, with rows formed there (both evaluations
search).  Only there is dx_new != 0: the A_matrix branch of s2_J_d, a non-trivial S2_Nx_yy, so3_J_d
away from the identity in the prep.

Metrics (ikfom_ref.errors): dx_ per block relative to the reference's block, quaternion and gravity
distance of the output state, max_ij |d cov_ij| / sqrt(P_ii P_jj).  Counts, iterations, knn_passes,
converged and t are exact against the oracle.  The bar, per metric and case:

    max(100 x the oracle's own error against the reference on that input, FLOOR[metric])

100 as in test_gpu_solve.py: the device's wave LU pivots differently from the oracle's inverse.
FLOOR is the oracle's largest error against the reference over the whole sweep, both evaluations,
measured on the CPU by tests/test_ikfom_reference.py (which prints the table and checks these
numbers against what it measures); nothing here comes from the device's output:

    measured  dx_pos 2.7e-10  dx_rot 5.1e-11  dx_offset_R 1.1e-10  dx_offset_T 1.0e-11
              dx_vel 4.9e-11  dx_bg 4.7e-11  dx_ba 1.1e-11  dx_grav 1.4e-11
              q_rot 8.3e-14  q_offset_R 1.2e-13  grav 3.0e-14  cov 3.1e-10
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLOOR = {"dx_pos": 3.0e-10, "dx_rot": 6.0e-11, "dx_offset_R": 1.2e-10, "dx_offset_T": 1.1e-11,
         "dx_vel": 5.0e-11, "dx_bg": 5.0e-11, "dx_ba": 1.2e-11, "dx_grav": 1.5e-11,
         "q_rot": 9.0e-14, "q_offset_R": 1.3e-13, "grav": 3.1e-14, "cov": 3.2e-10}
EXACT = ("iterations", "knn_passes", "converged", "t", "effct_feat_num")


def _ir():
    import ikfom_ref
    return ikfom_ref


def _bits(x):
    return np.asarray(x).tobytes()


@pytest.fixture(scope="module")
def work(built):
    import solve_ref
    return solve_ref.workload()


@pytest.fixture(scope="module")
def ctx(work):
    import livo_amd
    from livo_amd import synth
    with livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=0) as c:
        c.map_build(work["map"])
        yield c


def _run(ctx, body, st, max_iter):
    ctx.set_params(max_iterations=max_iter)
    sid = ctx.scan_upload(body)
    try:
        return ctx.ikfom_update(sid, st)
    finally:
        ctx.scan_release(sid)
        ctx.set_params(max_iterations=0)


def _ulp2(x):
    return 2 * np.spacing(np.abs(np.asarray(x, np.float64)).max())


def _hold(tag, dx, out, ref, orc, st):
    """One device evaluation against its reference at the bars; prints device / bar / oracle on failure."""
    ir = _ir()
    err = ir.errors(dx, out, ref, st["cov"])
    assert set(err) == set(orc) == set(FLOOR)
    bars = {k: max(100.0 * orc[k], FLOOR[k]) for k in err}
    print(f"{tag} device/oracle " + " ".join(f"{k}={err[k]:.1e}/{orc[k]:.1e}" for k in err))
    bad = {k: (err[k], bars[k], orc[k]) for k in err if not err[k] <= bars[k]}
    assert not bad, f"{tag} metric: (device, bar, oracle) {bad}; cond {ref['cond']:.2e}"
    for k, a, b in ir.BLOCKS:  # the additive members: x + dx_, both sums rounded once
        if k in ir.ADDITIVE:
            tol = bars["dx_" + k] * max(np.linalg.norm(ref["dx"][a:b]), 1e-6 * np.linalg.norm(ref["dx"])) + _ulp2(ref["x"][k])
            assert np.abs(out[k] - ref["x"][k]).max() <= tol, (tag, k)
    assert abs(np.linalg.norm(out["grav"]) - ir.S2_LEN) < 1e-12
    return err


@pytest.mark.parametrize("name", list(_ir().CASES))
def test_device_vs_reference(ctx, work, name):
    from test_ikfom_reference import _oracle_case
    ir = _ir()
    r = _oracle_case(name, work)
    c, st, body, tree = r["case"], r["case"]["state"], r["case"]["body"], work["tree"]
    want = c["want"]
    g0, gs0 = _run(ctx, body, st, 0)
    g1, gs1 = _run(ctx, body, st, 1)
    for k in EXACT:
        assert gs0[k] == r["s0"][k] and gs1[k] == r["s1"][k], k
    assert gs0["iterations"] == 1 and gs1["iterations"] == 2 and gs1["knn_passes"] == 2
    assert gs0["effct_feat_num"][0] == (want if want is not None else r["ref0"]["effct"])
    assert _bits(gs1["dx"][0]) == _bits(gs0["dx"][0])  # evaluation 1 enters from g0
    _hold(name + " eval 0", gs0["dx"][0], g0, r["ref0"], r["e0"], st)
    entry = dict(g0)
    entry["cov"] = st["cov"]
    ref1 = ir.reference(entry, st, body, tree)
    assert gs1["effct_feat_num"][1] == ref1["effct"]
    assert np.linalg.norm(ref1["dx_new"]) > 1e-4
    _hold(name + " eval 1", gs1["dx"][1], g1, ref1, r["e1"], st)


def test_batch_equals_single(ctx, work):
    """The sweep's generic cases (1000, 22- and 24-row prefixes, two covariance classes) in one batch:
    bitwise the single updates, synchronous and submitted."""
    ir = _ir()
    cases = [ir.case(n) for n in ir.GENERIC]
    assert len({len(c["body"]) for c in cases}) >= 3
    states = [c["state"] for c in cases]
    ctx.set_params(max_iterations=1)
    sids = [ctx.scan_upload(c["body"]) for c in cases]
    try:
        single = [ctx.ikfom_update(s, st) for s, st in zip(sids, states)]
        sync = ctx.ikfom_update_batch(sids, states)
        sub = ctx.ikfom_update_batch_wait(ctx.ikfom_update_batch_submit(sids, states), len(sids))
    finally:
        for s in sids:
            ctx.scan_release(s)
        ctx.set_params(max_iterations=0)
    for tag, (b_out, b_stats) in (("sync", sync), ("submit", sub)):
        for i, (out, stats) in enumerate(single):
            for k in out:
                assert _bits(b_out[i][k]) == _bits(out[k]), (tag, i, k)
            for k in EXACT:
                assert b_stats[i][k] == stats[k], (tag, i, k)
            assert _bits(b_stats[i]["dx"]) == _bits(stats["dx"]) and stats["iterations"] == 2, (tag, i)
