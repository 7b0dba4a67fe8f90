"""The fused first search on a static map leaves out the neighbour records that the
scan's second search is sure to rewrite (DESIGN.md §3 "Dead first records").  Nothing
a caller can see may change: states, statistics and the records after an update.

References.  States and iteration statistics: the oracle, at test_gpu_parity's bars.
Records: the oracle's search bit for bit where it defines them so -- one evaluation
(max_iterations 0) at the identity pose, where world point = body point.  After a
longer loop the oracle returns no neighbours and not the pose of its last search, so
the records are compared (a) bit for bit with a full-record context
(LIVO_REC_COMPACT=0), in which every search stores every record as it always did, and
(b) with the oracle's own search at the pose rebuilt from the oracle's solutions, at
the tolerance the parity bars leave between the two poses (_oracle_last_search)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 700)  # wave and block edges, a ragged last block
REL_STATE = 1e-5  # test_gpu_parity's bars


def _synth():
    from livo_amd import synth
    return synth


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _bits(x):
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_bits(v) for v in x]
    return np.asarray(x).tobytes()


ID_STATE = {"rot": np.eye(3), "pos": np.zeros(3), "vel": np.zeros(3), "bias_g": np.zeros(3),
            "bias_a": np.zeros(3), "gravity": np.array([0.0, 0.0, -9.81]), "cov": np.eye(18) * 1e-3}


@pytest.fixture(scope="module")
def map5k():
    return _synth().make_map(5_000)


@pytest.fixture(scope="module")
def tree5k(built, map5k):
    import oracle
    return oracle.Tree(map5k)


@pytest.fixture(scope="module")
def scans():
    synth = _synth()
    out = {}
    for k, n in enumerate(SIZES):
        out[n] = (np.ascontiguousarray(synth.make_scan(max(n, 64), 20 + k)[0][:n]), synth.make_state(20 + k))
    return out


def _run(m, bodies, states, max_iter, env, monkeypatch, t_LI=None, pipelined=False, prof=False):
    """One batched update in a fresh context: (states, stats, records, replays)."""
    import livo_amd
    for k in ("LIVO_FUSED", "LIVO_REC_COMPACT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t_LI = _synth().T_LI if t_LI is None else t_LI
    with livo_amd.Context(0, t_LI=t_LI, max_iterations=max_iter) as ctx:
        ctx.map_build(m)
        if prof:
            ctx.set_profiling(2)  # (the level that reads the replay counter back)
        sids = [ctx.scan_upload(b) for b in bodies]
        if pipelined:
            t = ctx.iekf_update_batch_submit(sids, states)
            st, stats = ctx.iekf_update_batch_wait(t, len(sids))
        else:
            st, stats = ctx.iekf_update_batch(sids, states)
        replays = ctx.last_timings()["knn_replays"] if prof else None
        nn = [ctx.scan_neighbors(s) for s in sids]
    for k in env:
        monkeypatch.delenv(k, raising=False)
    return st, stats, nn, replays


def _oracle_bars(tree, body, st0, sg, stg, max_iter, t_LI):
    sr, str_ = tree.iekf_update(body, st0, R_LI=np.eye(3), t_LI=t_LI, max_iter=max_iter)
    assert stg["iterations"] == str_["iterations"]
    assert stg["knn_passes"] == str_["knn_passes"]
    assert stg["converged"] == str_["converged"]
    assert list(stg["effct_feat_num"]) == list(str_["effct_feat_num"])
    for e in range(stg["iterations"]):
        assert _rel(stg["solution"][e], str_["solution"][e]) < REL_STATE, e
    dth = np.linalg.norm(st0["rot"].T @ sg["rot"] - st0["rot"].T @ sr["rot"])
    assert dth < REL_STATE * max(np.linalg.norm(str_["solution"][:, :3]), 1e-12)
    assert _rel(sg["pos"] - st0["pos"], sr["pos"] - st0["pos"]) < REL_STATE
    assert np.linalg.norm(sg["cov"] - sr["cov"]) / np.linalg.norm(st0["cov"]) < 1e-9
    return str_


def _oracle_last_search(m, tree, body, st0, ref_stats, max_iter, t_LI, nn):
    """The device's records against the oracle's own search at the pose of the oracle's
    last searching evaluation, rebuilt from the oracle's solutions and the control law
    (laser_mapping.cpp:217-227).

    Tolerance, from the parity bars and the number formats, not from a run.  _oracle_bars
    holds each device solution to REL_STATE of the oracle's (18-vector norm), so before the
    last search the two poses differ by at most
        dp = REL_STATE * sum_e |sol_e| * (1 + lever)   (position part + rotation part x lever arm)
    with lever the largest distance of a scan point from the sensor, plus F32 = 2e-6 m for the
    float32 rounding of a world point at up to 16 m (ulp 1.9e-6, three coordinates).  A
    neighbour at distance r then has a squared distance within 2 r dp + dp^2.  Indices must be
    equal for every point whose six nearest squared distances are apart by more than twice
    that (a nearer tie may order either way); such points must be most of the scan."""
    import oracle
    F32 = 2e-6
    synth = _synth()
    n_ev = ref_stats["iterations"]
    it, rematch, search = -1, 0, [True]
    rot, pos = np.array(st0["rot"], np.float64), np.array(st0["pos"], np.float64)
    poses, norms = [(rot, pos)], []
    for e in range(n_ev):
        sol = np.asarray(ref_stats["solution"][e], np.float64)
        conv = np.linalg.norm(sol[:3]) * 180 / 3.14159265358 < 0.01 and np.linalg.norm(sol[3:6]) * 100 < 0.015
        nxt = False
        if conv or (rematch == 0 and it == max_iter - 2):
            nxt, rematch = True, rematch + 1
        search.append(nxt)
        it += 1
        rot, pos = rot @ synth.so3_exp(sol[:3]), pos + sol[3:6]
        poses.append((rot, pos))
        norms.append(np.linalg.norm(sol))
    assert sum(search[:n_ev]) == ref_stats["knn_passes"]
    last = max(e for e in range(n_ev) if search[e])
    rot, pos = poses[last]
    t = np.asarray(t_LI, np.float64)
    world = np.ascontiguousarray(oracle.to_world(body, {"rot": rot, "pos": pos}, np.eye(3), t)[:, :3])
    lever = float(np.linalg.norm(np.asarray(body, np.float64)[:, :3] + t, axis=1).max())
    dp = REL_STATE * sum(norms[:last]) * (1.0 + lever) + F32
    idx5, d5, _ = tree.knn(world, 5)
    # the six nearest squared distances (brute force: the tree answers k <= 5)
    dd = ((world[:, None, :].astype(np.float64) - np.asarray(m, np.float64)[None, :, :3]) ** 2).sum(axis=2)
    d6 = np.sort(np.partition(dd, 5, axis=1)[:, :6], axis=1)
    tol = 2.0 * np.sqrt(d6) * dp + dp * dp  # per neighbour
    clear = (np.diff(d6, axis=1) > 2.0 * tol[:, 5:6]).all(axis=1)
    idx, d = nn
    err = np.abs(d.astype(np.float64) - d5)
    print(f"last search: evaluation {last}, lever {lever:.1f} m, dp {dp:.2e} m, clear {clear.mean():.3f}, "
          f"max sqdist error / tolerance {(err / tol[:, :5]).max():.3f}")
    assert clear.mean() >= 0.75 or len(body) < 8, clear.mean()
    np.testing.assert_array_equal(idx[clear], idx5[clear])
    assert (err <= tol[:, :5]).all(), (err / tol[:, :5]).max()
    return last


@pytest.fixture(scope="module")
def full4(built, map5k, scans):
    """The eight scans, one batch, max_iterations 4, with full records."""
    mp = pytest.MonkeyPatch()
    try:
        bodies = [scans[n][0] for n in SIZES]
        states = [scans[n][1] for n in SIZES]
        return _run(map5k, bodies, states, 4, {"LIVO_REC_COMPACT": "0"}, mp)
    finally:
        mp.undo()


@pytest.mark.parametrize("n", SIZES)
def test_sizes(built, map5k, tree5k, scans, full4, n, monkeypatch):
    """max_iterations 4: the oracle's states and statistics; every point's record after
    the update is the last search's."""
    synth = _synth()
    body, st0 = scans[n]
    st, stats, nn, _ = _run(map5k, [body], [st0], 4, {}, monkeypatch)
    ref = _oracle_bars(tree5k, body, st0, st[0], stats[0], 4, synth.T_LI)
    assert ref["knn_passes"] == 2  # (the first search's records were dead)
    assert _oracle_last_search(map5k, tree5k, body, st0, ref, 4, synth.T_LI, nn[0]) >= 1
    k = SIZES.index(n)
    assert _bits(st[0]) == _bits(full4[0][k])
    np.testing.assert_array_equal(nn[0][0], full4[2][k][0])
    np.testing.assert_array_equal(nn[0][1], full4[2][k][1])
    assert nn[0][0].shape == (n, 5) and (nn[0][0] >= 0).all() and np.isfinite(nn[0][1]).all()


@pytest.mark.parametrize("max_iter", [0, 1])
def test_short_loops(built, map5k, scans, max_iter, monkeypatch):
    """max_iterations 0 (one search: its records are the answer) and 1: the records of
    every point equal the oracle's search (0, identity pose) and the full-record context's."""
    import oracle
    m = map5k
    bodies = [np.ascontiguousarray(m[::7][:n] + np.float32(0.03)) for n in (65, 257, 700)]
    states = [ID_STATE] * 3
    zero = [0.0, 0.0, 0.0]
    st, stats, nn, _ = _run(m, bodies, states, max_iter, {}, monkeypatch, t_LI=zero)
    st_u, stats_u, nn_u, _ = _run(m, bodies, states, max_iter, {"LIVO_REC_COMPACT": "0"}, monkeypatch, t_LI=zero)
    assert _bits(st) == _bits(st_u) and _bits(nn) == _bits(nn_u)
    assert [s["knn_passes"] for s in stats] == [1 + max_iter] * 3
    tree = oracle.Tree(m)
    if max_iter == 1:  # the second search, at the pose after the first solve
        for b, sg, stg, rec in zip(bodies, st, stats, nn):
            ref = _oracle_bars(tree, b, ID_STATE, sg, stg, 1, np.zeros(3))
            assert _oracle_last_search(m, tree, b, ID_STATE, ref, 1, zero, rec) == 1
    if max_iter == 0:
        for b, (idx, d) in zip(bodies, nn):
            idx_r, d_r, _ = tree.knn(b, 5)
            np.testing.assert_array_equal(idx, idx_r)
            np.testing.assert_array_equal(d, d_r)


def _lattice(seed=7, n_base=6_000, n_q=700, n_dup=40):
    """test_gpu_parity's dyadic lattice (mirror pairs at exactly equal distances), with an
    exact duplicate for the first n_dup queries (same distance, same x: the exact replay)."""
    rng = np.random.default_rng(seed)
    g = 2.0 ** -8
    base = rng.integers(0, 16 * 256, size=(n_base, 3)) * g
    q = rng.integers(256, 15 * 256, size=(n_q, 3)) * g
    v = rng.integers(1, 4, size=(n_q, 3)) * rng.choice([-1, 1], size=(n_q, 3)) * g
    v[:, 1] = np.sign(v[:, 1]) * ((np.abs(v[:, 0]) / g) % 3 + 1) * g
    vp = v[:, [1, 0, 2]]
    four = np.arange(n_q) % 2 == 0
    extra = [q + v, q - v, (q + vp)[four], (q - vp)[four], (q + v)[:n_dup]]
    return np.concatenate([base] + extra).astype(np.float32), q.astype(np.float32)


def _dup_map():
    """test_gpu_parity's duplicate-point map: every answer hinges on PointType_CMP ties."""
    synth = _synth()
    base = synth.make_map(3_000)
    return np.concatenate([base, base[::-1]]), synth.make_scan(700, 8)[0][:700].copy(), synth.make_state(8)


@pytest.mark.parametrize("kind", ["lattice", "duplicates"])
def test_tie_replays(built, kind, monkeypatch):
    """Flagged queries replay from their own records inside the first evaluation: their
    waves keep the store.  Replays ran; planes (through the effective-point counts and
    solutions of every evaluation) and final states equal the oracle's; records equal the
    full-record context's."""
    import oracle
    synth = _synth()
    if kind == "lattice":
        m, body = _lattice()
        st0, t_LI = ID_STATE, [0.0, 0.0, 0.0]
    else:
        m, body, st0 = _dup_map()
        t_LI = synth.T_LI
    st, stats, nn, replays = _run(m, [body], [st0], 4, {}, monkeypatch, t_LI=t_LI, prof=True)
    assert replays > 0, replays
    # the first evaluation alone (one search) flags the same queries: its replay count
    _, _, _, first = _run(m, [body], [st0], 0, {}, monkeypatch, t_LI=t_LI, prof=True)
    assert first > 0, first
    _oracle_bars(oracle.Tree(m), body, st0, st[0], stats[0], 4, np.asarray(t_LI, np.float64))
    st_u, stats_u, nn_u, _ = _run(m, [body], [st0], 4, {"LIVO_REC_COMPACT": "0"}, monkeypatch, t_LI=t_LI)
    assert _bits(st) == _bits(st_u) and _bits(nn) == _bits(nn_u)
    assert _bits(stats[0]["solution"]) == _bits(stats_u[0]["solution"])


def test_mixed_batch(built, map5k, scans, full4, monkeypatch):
    """Six scans of different sizes in one batch, synchronous and pipelined: byte-identical."""
    ns = (700, 1, 257, 64, 255, 65)
    bodies = [scans[n][0] for n in ns]
    states = [scans[n][1] for n in ns]
    a = _run(map5k, bodies, states, 4, {}, monkeypatch)
    b = _run(map5k, bodies, states, 4, {}, monkeypatch, pipelined=True)
    assert _bits(a[0]) == _bits(b[0]) and _bits(a[2]) == _bits(b[2])
    assert _bits([s["solution"] for s in a[1]]) == _bits([s["solution"] for s in b[1]])
    for k, n in enumerate(ns):
        assert _bits(a[2][k]) == _bits(full4[2][SIZES.index(n)]), n


def test_no_effective_points(built, map5k, monkeypatch):
    """A scan far from the map: every 5th neighbour is beyond the gate, no point is
    effective, the solve runs on zero sums (solve_scan has no stop of its own for it: the
    control law alone ends the loop).  A scan half far, half near beside it.  Records are
    complete for every point and equal the full-record context's."""
    synth = _synth()
    near, st0 = synth.make_scan(300, 31)[0][:300].copy(), synth.make_state(31)
    far = (near + np.float32(30.0)).astype(np.float32)
    half = np.concatenate([near[:150], far[:107]])
    bodies, states = [far, half], [st0, st0]
    st, stats, nn, _ = _run(map5k, bodies, states, 4, {}, monkeypatch)
    st_u, stats_u, nn_u, _ = _run(map5k, bodies, states, 4, {"LIVO_REC_COMPACT": "0"}, monkeypatch)
    assert list(stats[0]["effct_feat_num"]) == [0] * stats[0]["iterations"]
    assert stats[0]["knn_passes"] == 2
    for (idx, d), b in zip(nn, bodies):
        assert idx.shape == (len(b), 5) and (idx >= 0).all() and (idx < len(map5k)).all()
        assert np.isfinite(d).all() and (np.diff(d, axis=1) >= 0).all()
    assert (nn[0][1][:, 4] > 5.0).all()
    assert _bits(nn) == _bits(nn_u)
    assert _bits(st[1]) == _bits(st_u[1])


@pytest.mark.parametrize("variant", ["asym", "indef"])
def test_lu_path(built, map5k, tree5k, scans, variant, monkeypatch):
    """A covariance the host cannot factor (oracle/solve_ref.py's asym / indef, as
    test_gpu_solve uses them): cov_ok == 0, the device's solve takes the pivoted 6x6 LU.
    Two such scans beside a diagonal one, max_iterations 4: two searches each, every record
    complete and equal to the full-record context's bit for bit and to the oracle's last
    search; states and statistics at the parity bars."""
    import solve_ref as sr
    synth = _synth()
    bad = {"asym": sr.asym(sr.dense_cov(7, 0.5)), "indef": sr.indef(sr.dense_cov(7, 0.99))}[variant]
    if variant == "indef":
        with pytest.raises(np.linalg.LinAlgError):
            np.linalg.cholesky(bad[:6, :6])
    else:
        assert not np.array_equal(bad, bad.T)
    ns = (700, 65, 257)
    bodies = [scans[n][0] for n in ns]
    states = [dict(scans[n][1]) for n in ns]
    states[0]["cov"] = bad
    states[2]["cov"] = bad
    st, stats, nn, _ = _run(map5k, bodies, states, 4, {}, monkeypatch)
    st_u, stats_u, nn_u, _ = _run(map5k, bodies, states, 4, {"LIVO_REC_COMPACT": "0"}, monkeypatch)
    assert _bits(st) == _bits(st_u) and _bits(nn) == _bits(nn_u)
    for k, n in enumerate(ns):
        assert stats[k]["knn_passes"] == 2, k
        idx, d = nn[k]
        assert idx.shape == (n, 5) and (idx >= 0).all() and (idx < len(map5k)).all()
        assert np.isfinite(d).all() and (np.diff(d, axis=1) >= 0).all()
        ref = _oracle_bars(tree5k, bodies[k], states[k], st[k], stats[k], 4, synth.T_LI)
        assert _oracle_last_search(map5k, tree5k, bodies[k], states[k], ref, 4, synth.T_LI, nn[k]) >= 1
