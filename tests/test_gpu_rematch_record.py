"""The fused searches after a scan's first on a static map leave out the neighbour
records that nothing in the loop reads; the library rebuilds a scan's records when a
caller first asks for them (DESIGN.md §3 "Records on demand").  Nothing a caller can see
may change: states, statistics, the records after an update and every consumer of them.

Reference: a full-record context (LIVO_REC_COMPACT=0), in which every search stores
every record as it always did, bit for bit -- as in test_gpu_first_record, whose checks
against the oracle hold for the same code.  That each branch is taken is asserted on the
reference's own results (replays, gated points, the evaluation after the last search)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 513)  # wave and block edges inside and at the end of a scan
LATE = {65: 3, 257: 6, 513: 6}               # scans that end with points in the map's hole
GATE = 5.0                                   # max_nn_sqdist
HOLE_C = np.array([10.0, 6.0, -1.6])         # a spot on the floor; the map has no point within HOLE_R of it
HOLE_R = 3.2

ID_STATE = {"rot": np.eye(3), "pos": np.zeros(3), "vel": np.zeros(3), "bias_g": np.zeros(3),
            "bias_a": np.zeros(3), "gravity": np.array([0.0, 0.0, -9.81]), "cov": np.eye(18) * 1e-3}


def _synth():
    from livo_amd import synth
    return synth


def _bits(x):
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_bits(v) for v in x]
    return np.asarray(x).tobytes()


def _searches(stats, max_iter):
    """Which evaluations searched, from the solutions and the control law
    (laser_mapping.cpp:217-227), as test_gpu_first_record rebuilds it."""
    n_ev = stats["iterations"]
    it, rematch, search = -1, 0, [True]
    for e in range(n_ev):
        sol = np.asarray(stats["solution"][e], np.float64)
        conv = np.linalg.norm(sol[:3]) * 180 / 3.14159265358 < 0.01 and np.linalg.norm(sol[3:6]) * 100 < 0.015
        nxt = False
        if conv or (rematch == 0 and it == max_iter - 2):
            nxt, rematch = True, rematch + 1
        search.append(nxt)
        it += 1
    assert sum(search[:n_ev]) == stats["knn_passes"]
    return search[:n_ev]


@pytest.fixture(scope="module")
def hole_map():
    m = _synth().make_map(6_000)
    keep = np.linalg.norm(m.astype(np.float64) - HOLE_C, axis=1) > HOLE_R
    return np.ascontiguousarray(m[keep])


@pytest.fixture(scope="module")
def scans(built, hole_map):
    """One scan per size; those of LATE end with points in the hole, whose five
    neighbours lie on its rim, beyond the gate (checked here with the oracle's search)."""
    import oracle
    synth = _synth()
    rng = np.random.default_rng(11)
    tree = oracle.Tree(hole_map)
    out = {}
    for k, n in enumerate(SIZES):
        body = np.ascontiguousarray(synth.make_scan(max(n, 64), 40 + k)[0][:n])
        st0 = synth.make_state(40 + k)
        if n in LATE:
            nl = LATE[n]
            w = HOLE_C + np.concatenate([rng.uniform(-0.3, 0.3, size=(nl, 2)), np.zeros((nl, 1))], axis=1)
            _, d_ref, _ = tree.knn(w.astype(np.float32), 5)
            assert (d_ref[:, 4] > GATE + 1.0).all(), d_ref[:, 4]  # (the poses of a loop differ by centimetres)
            R, p = np.asarray(st0["rot"]), np.asarray(st0["pos"])
            body = np.concatenate([body[:-nl], ((w - p) @ R - synth.T_LI).astype(np.float32)])
        out[n] = (np.ascontiguousarray(body), st0)
    return out


def _ctx(env, monkeypatch, max_iter=4, t_LI=None):
    import livo_amd
    for k in ("LIVO_FUSED", "LIVO_REC_COMPACT", "LIVO_REC_LAZY"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = livo_amd.Context(0, t_LI=_synth().T_LI if t_LI is None else t_LI, max_iterations=max_iter)
    for k in env:  # (read once, when the context is created)
        monkeypatch.delenv(k, raising=False)
    return ctx


def _run(m, bodies, states, max_iter, env, monkeypatch, t_LI=None, pipelined=False, prof=False):
    """One batched update in a fresh context: (states, stats, records, records asked for
    again, replays)."""
    with _ctx(env, monkeypatch, max_iter, t_LI) as ctx:
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
        nn2 = [ctx.scan_neighbors(s) for s in sids]
    return st, stats, nn, nn2, replays


FULL = {"LIVO_REC_COMPACT": "0"}


@pytest.fixture(scope="module")
def full4(built, hole_map, scans):
    """The eight scans, one batch, max_iterations 4, with full records."""
    mp = pytest.MonkeyPatch()
    try:
        return _run(hole_map, [scans[n][0] for n in SIZES], [scans[n][1] for n in SIZES], 4, FULL, mp)
    finally:
        mp.undo()


@pytest.mark.parametrize("n", SIZES)
def test_sizes(built, hole_map, scans, full4, n, monkeypatch):
    """States, statistics and every point's record after the update; the records asked
    for twice are the same bytes."""
    body, st0 = scans[n]
    st, stats, nn, nn2, _ = _run(hole_map, [body], [st0], 4, {}, monkeypatch)
    k = SIZES.index(n)
    ref_st, ref_stats, ref_nn = full4[0][k], full4[1][k], full4[2][k]
    sr = _searches(ref_stats, 4)
    assert ref_stats["knn_passes"] == 2 and max(e for e, s in enumerate(sr) if s) >= 1  # (the last search is a rematch)
    assert _bits(st[0]) == _bits(ref_st)
    assert _bits(stats[0]) == _bits(ref_stats)
    assert _bits(nn[0]) == _bits(ref_nn) and _bits(nn2[0]) == _bits(ref_nn)
    idx, d = nn[0]
    assert idx.shape == (n, 5) and (idx >= 0).all() and np.isfinite(d).all() and (np.diff(d, axis=1) >= 0).all()


def test_off_switch(built, hole_map, scans, full4, monkeypatch):
    """LIVO_REC_LAZY=0: the rematch stores its records; the same results."""
    ns = (513, 65, 1)
    got = _run(hole_map, [scans[n][0] for n in ns], [scans[n][1] for n in ns], 4, {"LIVO_REC_LAZY": "0"}, monkeypatch)
    for k, n in enumerate(ns):
        j = SIZES.index(n)
        assert _bits([got[0][k], got[1][k], got[2][k]]) == _bits([full4[0][j], full4[1][j], full4[2][j]]), n


@pytest.mark.parametrize("n", sorted(LATE))
def test_late_fit(built, hole_map, scans, full4, n, monkeypatch):
    """Points whose 5th neighbour is beyond the gate in the rematch stay at plane state 0
    and are fitted from their records by the cached-plane evaluation that follows it: their
    waves keep the store.  The reference shows the case: gated records after the loop, and an
    evaluation without a search after the last search."""
    body, st0 = scans[n]
    nl = LATE[n]
    k = SIZES.index(n)
    ref_stats, ref_nn = full4[1][k], full4[2][k]
    sr = _searches(ref_stats, 4)
    last = max(e for e, s in enumerate(sr) if s)
    assert last >= 1 and ref_stats["iterations"] > last + 1, sr  # (a cached-plane evaluation follows the rematch)
    assert (ref_nn[1][-nl:, 4] > GATE).all(), ref_nn[1][-nl:, 4]

    def run(env):
        with _ctx(env, monkeypatch) as ctx:
            ctx.map_build(hole_map)
            sid = ctx.scan_upload(body)
            b, st = ctx.iekf_update_batch([sid], [st0])
            # at the pose the late points were built for they lie on the floor: a plane fitted
            # from their rim neighbours (in the loop, or here) selects them
            r = ctx.h_share(sid, st0, search_en=False)
            return b, st, r["sel"], r["normvec"], r["HTH"], r["HTL"], r["effct"], ctx.scan_neighbors(sid)

    full, lazy = run(FULL), run({})
    for got in (full, lazy):
        assert got[2][-nl:].all(), got[2][-nl:]
        assert (np.abs(got[3][-nl:, :3]).max(axis=1) > 0.9).all(), got[3][-nl:]  # (the floor's normal)
    assert _bits(full) == _bits(lazy)
    assert _bits(lazy[1][0]) == _bits(ref_stats)  # (effct_feat_num and solution of every evaluation among them)


def _lattice(seed=7, n_base=6_000, n_q=513, n_dup=40):
    """test_gpu_parity's dyadic lattice (mirror pairs at exactly equal distances), with an
    exact duplicate for the first n_dup queries (same distance, same x whatever the pose:
    the exact replay, in the rematch too)."""
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
    return np.concatenate([base, base[::-1]]), synth.make_scan(513, 8)[0][:513].copy(), synth.make_state(8)


@pytest.mark.parametrize("kind", ["lattice", "duplicates"])
def test_tie_replays(built, kind, monkeypatch):
    """Flagged queries of the rematch replay from their own records inside its launch:
    their waves keep the store.  The reference replays more queries in the whole loop than
    in its first evaluation alone, so the rematch replayed."""
    if kind == "lattice":
        m, body = _lattice()
        st0, t_LI = ID_STATE, [0.0, 0.0, 0.0]
    else:
        m, body, st0 = _dup_map()
        t_LI = _synth().T_LI
    full = _run(m, [body], [st0], 4, FULL, monkeypatch, t_LI=t_LI, prof=True)
    first = _run(m, [body], [st0], 0, FULL, monkeypatch, t_LI=t_LI, prof=True)
    assert first[4] > 0 and full[4] > first[4], (first[4], full[4])
    assert full[1][0]["knn_passes"] == 2
    lazy = _run(m, [body], [st0], 4, {}, monkeypatch, t_LI=t_LI, prof=True)
    assert lazy[4] == full[4]
    assert _bits(lazy[:4]) == _bits(full[:4])


def test_tiny_map(built, scans, monkeypatch):
    """A map of fewer than 5 points: every list is short (d5 = +inf), every wave keeps its
    records; the rebuilt records carry the same counts and pads."""
    m = _synth().make_map(6_000)[[10, 2000, 4000]].copy()
    ns = (65, 257)
    bodies, states = [scans[n][0] for n in ns], [scans[n][1] for n in ns]
    full = _run(m, bodies, states, 4, FULL, monkeypatch)
    lazy = _run(m, bodies, states, 4, {}, monkeypatch)
    assert (full[2][0][0][:, 3:] == -1).all() and (full[2][0][0][:, :3] >= 0).all()
    assert _bits(lazy[:4]) == _bits(full[:4])


@pytest.mark.parametrize("max_iter", [1, 2, 4])
def test_mixed_batch(built, hole_map, scans, max_iter, monkeypatch):
    """Six scans of different sizes in one batch, synchronous and pipelined, at
    max_iterations 1, 2 and 4 (two searches each): byte-identical to the full records."""
    ns = (513, 1, 257, 64, 255, 65)
    bodies, states = [scans[n][0] for n in ns], [scans[n][1] for n in ns]
    full = _run(hole_map, bodies, states, max_iter, FULL, monkeypatch)
    assert [s["knn_passes"] for s in full[1]] == [2] * len(ns)
    a = _run(hole_map, bodies, states, max_iter, {}, monkeypatch)
    b = _run(hole_map, bodies, states, max_iter, {}, monkeypatch, pipelined=True)
    assert _bits(a[:4]) == _bits(full[:4])
    assert _bits(b[:4]) == _bits(full[:4])


def test_no_effective_points(built, hole_map, monkeypatch):
    """A scan far from the map (every 5th neighbour beyond the gate, no effective point,
    the solve on zero sums) and one half far, half near."""
    synth = _synth()
    near, st0 = synth.make_scan(300, 31)[0][:300].copy(), synth.make_state(31)
    far = (near + np.float32(30.0)).astype(np.float32)
    half = np.concatenate([near[:150], far[:107]])
    bodies, states = [far, half], [st0, st0]
    full = _run(hole_map, bodies, states, 4, FULL, monkeypatch)
    assert list(full[1][0]["effct_feat_num"]) == [0] * full[1][0]["iterations"]
    assert full[1][0]["knn_passes"] == 2 and (full[2][0][1][:, 4] > GATE).all()
    lazy = _run(hole_map, bodies, states, 4, {}, monkeypatch)
    assert _bits(lazy[:4]) == _bits(full[:4])


def test_lu_path(built, hole_map, scans, monkeypatch):
    """A covariance the host cannot factor (cov_ok == 0: the pivoted 6x6 LU) beside a
    diagonal one: the pose of the last search is kept on that path too."""
    import solve_ref as sr
    bad = sr.asym(sr.dense_cov(7, 0.5))
    assert not np.array_equal(bad, bad.T)
    ns = (513, 65, 257)
    bodies = [scans[n][0] for n in ns]
    states = [dict(scans[n][1]) for n in ns]
    states[0]["cov"] = bad
    states[2]["cov"] = bad
    full = _run(hole_map, bodies, states, 4, FULL, monkeypatch)
    assert [s["knn_passes"] for s in full[1]] == [2, 2, 2]
    lazy = _run(hole_map, bodies, states, 4, {}, monkeypatch)
    assert _bits(lazy[:4]) == _bits(full[:4])


def test_consumers(built, hole_map, scans, monkeypatch):
    """Every reader of the records after a static-map update: livo_h_share without a
    search, scan_inherit_neighbors, a second map_build before the old scan's records are
    asked for, and map_incremental with the update that follows it."""
    import livo_amd
    synth = _synth()
    ns = (513, 257, 65)
    bodies, states = [scans[n][0] for n in ns], [scans[n][1] for n in ns]
    second = np.ascontiguousarray(hole_map[::2])

    def hs(ctx, sid, st):
        r = ctx.h_share(sid, st, search_en=False)
        return {k: r[k] for k in ("HTH", "HTL", "effct", "normvec", "sel", "nn_idx", "nn_d")}

    def run(env):
        out = {}
        with _ctx(env, monkeypatch) as ctx:
            ctx.map_build(hole_map)
            sids = [ctx.scan_upload(b) for b in bodies]
            upd, _ = ctx.iekf_update_batch(sids, states)
            out["hs"] = [hs(ctx, sid, st) for sid, st in zip(sids, upd)]
            ctx.iekf_update_batch(sids, states)
            dst = ctx.scan_upload(synth.make_scan(300, 77)[0])
            ctx.scan_inherit_neighbors(dst, sids[0])
            out["inherit"] = [ctx.scan_neighbors(dst), hs(ctx, dst, upd[0])]
            # a second map_build: the old scans' records are rebuilt before the map goes (the
            # iVox map_incremental reads them afterwards without asking for a new search)
            ctx.ivox_init(resolution=0.5, nearby_type=18)
            ctx.ivox_add_points(hole_map)
            upd, _ = ctx.iekf_update_batch(sids, states)
            ctx.map_build(second)
            out["rebuilt_hs"] = hs(ctx, sids[2], upd[2])  # (no neighbours any more: the loop's plane cache alone)
            out["rebuilt"] = []
            for sid, st in zip(sids[:2], upd[:2]):
                ctx.set_backend(livo_amd.BACKEND_IVOX)
                cat, counts = ctx.map_incremental(sid, st)
                ctx.set_backend(livo_amd.BACKEND_IKDTREE)
                assert len(np.unique(cat)) >= 2, np.bincount(cat)  # (decided from the neighbours' coordinates)
                out["rebuilt"].append([cat, {k: np.asarray(v) for k, v in counts.items()}])
            # map_incremental on the ikd backend, and the update that follows it
            ctx.map_build(hole_map)
            upd2, _ = ctx.iekf_update_batch(sids, states)
            cat, counts = ctx.map_incremental(sids[0], upd2[0])
            out["incr"] = [cat, {k: np.asarray(v) for k, v in counts.items()}]
            out["after"] = ctx.iekf_update_batch(sids, states)
            out["after_nn"] = [ctx.scan_neighbors(s) for s in sids]
        return _bits(out)

    full, lazy = run(FULL), run({})
    for k in full:
        assert full[k] == lazy[k], k
