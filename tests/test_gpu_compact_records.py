"""Hot-only neighbour records of the fused search (LIVO_REC_COMPACT, default on)
against full records (LIVO_REC_COMPACT=0): nothing numeric changes, so every
result must be equal bit for bit -- the updates, the neighbours, and every
consumer that reads the records' coordinates afterwards (filled on demand)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 300, 1000)  # a partial wave, a partial block, more than one block
GATE = 5.0                  # max_nn_sqdist: the 5th neighbour beyond sqrt(5) m is not selected after a search
HOLE_C = np.array([10.0, 6.0, -1.6])  # a spot on the floor; the map is thinned out around it
HOLE_R = 3.2


def _synth():
    from livo_amd import synth
    return synth


def _bits(x):
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_bits(v) for v in x]
    return np.asarray(x).tobytes()


@pytest.fixture(scope="module")
def small_map():
    """About 20k points of the synthetic room with a hole of HOLE_R around HOLE_C."""
    m = _synth().make_map(20_000)
    keep = np.linalg.norm(m.astype(np.float64) - HOLE_C, axis=1) > HOLE_R
    return np.ascontiguousarray(m[keep])


def _to_body(world, st, synth):
    """Body points whose world_point at state st is `world` (up to float rounding)."""
    R, p = np.asarray(st["rot"]), np.asarray(st["pos"])
    return ((world - p) @ R - synth.T_LI).astype(np.float32)  # R_LI = I


@pytest.fixture(scope="module")
def batch(small_map):
    """Four scans; scan 2 ends with 6 points in the hole (their 5 neighbours lie on the
    hole's rim, all beyond the gate)."""
    synth = _synth()
    scans = [synth.make_scan(n, 40 + k)[0][:n].copy() for k, n in enumerate(SIZES)]
    assert [len(s) for s in scans] == list(SIZES)
    states = [synth.make_state(40 + k) for k in range(len(SIZES))]
    rng = np.random.default_rng(11)
    late_w = HOLE_C + np.concatenate([rng.uniform(-0.3, 0.3, size=(6, 2)), np.zeros((6, 1))], axis=1)
    n_late = len(late_w)
    scans[2] = np.concatenate([scans[2][:-n_late], _to_body(late_w, states[2], synth)])
    return scans, states, late_w


def _both(monkeypatch, fn):
    """fn(ctx) in a context with full records and in one with the default."""
    import livo_amd
    synth = _synth()
    out = {}
    for compact in ("0", None):
        if compact is None:
            monkeypatch.delenv("LIVO_REC_COMPACT", raising=False)
        else:
            monkeypatch.setenv("LIVO_REC_COMPACT", compact)
        with livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=4) as ctx:
            out[compact] = fn(ctx)
    return out["0"], out[None]


def test_update_results(built, small_map, batch, monkeypatch):
    """States, covariance, iteration statistics and the neighbours after a synchronous
    batch and after one through submit / wait."""
    scans, states, _ = batch

    def run(ctx):
        ctx.map_build(small_map)
        sids = [ctx.scan_upload(s) for s in scans]
        b, st = ctx.iekf_update_batch(sids, states)
        nn = [ctx.scan_neighbors(s) for s in sids]
        t = ctx.iekf_update_batch_submit(sids, states)
        b2, st2 = ctx.iekf_update_batch_wait(t, len(sids))
        nn2 = [ctx.scan_neighbors(s) for s in sids]
        return _bits([b, st, nn, b2, st2, nn2])

    full, compact = _both(monkeypatch, run)
    assert full == compact


def test_late_fit(built, small_map, batch, monkeypatch):
    """Points whose 5th neighbour is beyond the gate after the search are left at plane
    state 0 and fitted by the next evaluation without a search, from the keys."""
    import oracle
    scans, states, late_w = batch
    n_late = len(late_w)
    # the gate trips by construction: checked on the CPU with the oracle
    _, d_ref, _ = oracle.Tree(small_map).knn(late_w.astype(np.float32), 5)
    assert (d_ref[:, 4] > GATE + 1.0).all(), d_ref[:, 4]

    def run(ctx):
        ctx.map_build(small_map)
        sid = ctx.scan_upload(scans[2])
        b, st = ctx.iekf_update_batch([sid], [states[2]])
        idx, d = ctx.scan_neighbors(sid)
        # the late points at the pose they were built for: on the floor, so a plane fitted
        # from their rim neighbours (in the loop from the keys, or here) selects them
        r = ctx.h_share(sid, states[2], search_en=False)
        return b, st, idx, d, r["sel"], r["normvec"]

    full, compact = _both(monkeypatch, run)
    assert (compact[3][-n_late:, 4] > GATE).all(), compact[3][-n_late:, 4]
    for got in (full, compact):  # the late points are fitted and kept: their planes reach the compared values
        assert got[4][-n_late:].all(), got[4][-n_late:]
        assert (np.abs(got[5][-n_late:, :3]).max(axis=1) > 0.9).all(), got[5][-n_late:]  # (the floor's normal)
    assert full[1][0]["iterations"] >= 2, full[1]  # (an evaluation without a search followed a search)
    assert _bits(full) == _bits(compact)
    assert _bits(full[1][0]) == _bits(compact[1][0])  # (effct_feat_num of every evaluation among them)


def _tie_map(seed=7, n_base=20_000, n_q=2_000, n_dup=40):
    """Dyadic lattice map + queries with 2 or 4 map points at exactly the same float
    distance (mirror pairs; ordered in the search by x), and for the first n_dup queries
    an exact duplicate of one of them (same distance, same x: the exact replay)."""
    rng = np.random.default_rng(seed)
    g = 2.0 ** -8
    base = rng.integers(0, 16 * 256, size=(n_base, 3)) * g
    q = rng.integers(256, 15 * 256, size=(n_q, 3)) * g
    v = rng.integers(1, 4, size=(n_q, 3)) * rng.choice([-1, 1], size=(n_q, 3)) * g
    v[:, 1] = np.sign(v[:, 1]) * ((np.abs(v[:, 0]) / g) % 3 + 1) * g  # |vx| != |vy|: distinct x
    vp = v[:, [1, 0, 2]]
    four = np.arange(n_q) % 2 == 0
    extra = [q + v, q - v, (q + vp)[four], (q - vp)[four], (q + v)[:n_dup]]
    return np.concatenate([base] + extra).astype(np.float32), q.astype(np.float32)


def test_ties(built, monkeypatch):
    """Replayed records (full) among hot-only ones: neighbours equal to the full-record
    context's and to the oracle's."""
    import oracle
    m, q = _tie_map()
    st0 = {"rot": np.eye(3), "pos": np.zeros(3), "vel": np.zeros(3), "bias_g": np.zeros(3),
           "bias_a": np.zeros(3), "gravity": np.array([0.0, 0.0, -9.81]), "cov": np.eye(18) * 1e-3}

    def run(ctx):
        ctx.set_params(t_LI=[0.0, 0.0, 0.0], max_iterations=0)
        ctx.map_build(m)
        ctx.set_profiling(2)  # (the level that reads the replay counter back)
        sid = ctx.scan_upload(q)
        ctx.iekf_update(sid, st0)  # one evaluation: the search at the identity pose
        replays = ctx.last_timings()["knn_replays"]
        idx, d = ctx.scan_neighbors(sid)
        hs = ctx.h_share(sid, st0, search_en=False)  # (the records' coordinates, filled or stored)
        return replays, idx, d, hs

    full, compact = _both(monkeypatch, run)
    assert compact[0] > 0 and compact[0] == full[0]
    idx_r, d_r, _ = oracle.Tree(m).knn(q, 5)
    for got in (full, compact):
        np.testing.assert_array_equal(got[2], d_r)
        np.testing.assert_array_equal(got[1], idx_r)
    assert _bits(full[3]) == _bits(compact[3])


def test_consumers(built, small_map, batch, monkeypatch):
    """Everything that reads the records' coordinates after a fused update."""
    synth = _synth()
    scans, states, _ = batch
    second = np.ascontiguousarray(small_map[::2])

    def hs(ctx, sid, st):
        r = ctx.h_share(sid, st, search_en=False)
        return {k: r[k] for k in ("HTH", "HTL", "effct", "normvec", "sel")}

    def run(ctx):
        out = {}
        ctx.map_build(small_map)
        sids = [ctx.scan_upload(s) for s in scans]
        upd, _ = ctx.iekf_update_batch(sids, states)
        # cached-neighbour h_share
        out["hs"] = [hs(ctx, sid, st) for sid, st in zip(sids, upd)]
        # scan_inherit_neighbors into a second scan (a fresh batch leaves the source hot-only again)
        ctx.iekf_update_batch(sids[3:], states[3:])
        dst = ctx.scan_upload(synth.make_scan(700, 77)[0])
        ctx.scan_inherit_neighbors(dst, sids[3])
        out["inherit"] = hs(ctx, dst, upd[3])
        # a second map_build: the old scan's records are filled before the map goes
        ctx.iekf_update_batch(sids[2:3], states[2:3])
        ctx.map_build(second)
        out["rebuilt"] = hs(ctx, sids[2], upd[2])
        # map_incremental on the ikd backend, and the neighbours of a following update
        upd2, _ = ctx.iekf_update_batch(sids, states)
        cat, counts = ctx.map_incremental(sids[3], upd2[3])
        out["incr"] = [cat, {k: np.asarray(v) for k, v in counts.items()}]
        out["after"] = ctx.iekf_update_batch(sids, states)
        out["after_nn"] = [ctx.scan_neighbors(s) for s in sids]
        out["after_hs"] = [hs(ctx, sid, st) for sid, st in zip(sids, out["after"][0])]
        return _bits(out)

    full, compact = _both(monkeypatch, run)
    for k in full:
        assert full[k] == compact[k], k


def test_fill_before_map_changes(built, small_map, batch, monkeypatch):
    """Hot-only records are filled before the map they index goes: after a second
    map_build, after the first Add_Points, and at a backend change.  The iVox
    map_incremental reads the old records' coordinates afterwards (it does not ask
    for a new search), so its categories depend on that fill."""
    import livo_amd
    scans, states, _ = batch
    second = np.ascontiguousarray(small_map[::2])

    def run(ctx):
        out = {}
        ctx.map_build(small_map)
        sids = [ctx.scan_upload(s) for s in scans]
        ctx.ivox_init(resolution=0.5, nearby_type=18)
        ctx.ivox_add_points(small_map)

        def incr(sid, st):
            ctx.set_backend(livo_amd.BACKEND_IVOX)
            cat, counts = ctx.map_incremental(sid, st)
            ctx.set_backend(livo_amd.BACKEND_IKDTREE)
            return [cat, {k: np.asarray(v) for k, v in counts.items()}]

        # the backend change itself
        upd, _ = ctx.iekf_update_batch(sids, states)
        out["backend"] = incr(sids[3], upd[3])
        # a second map_build (half the points: the old keys would index other points, or none)
        upd, _ = ctx.iekf_update_batch(sids, states)
        ctx.map_build(second)
        out["rebuilt"] = incr(sids[3], upd[3])
        out["rebuilt2"] = incr(sids[2], upd[2])
        # the first Add_Points: the map becomes incremental and its grid is rebuilt
        upd, _ = ctx.iekf_update_batch(sids, states)
        ctx.map_add_points(small_map[1::2][:3000] + np.float32(0.013))
        out["added"] = incr(sids[3], upd[3])
        out["added2"] = incr(sids[2], upd[2])
        return out

    full, compact = _both(monkeypatch, run)
    for k in full:
        cat = full[k][0]
        assert len(np.unique(cat)) >= 2, (k, np.bincount(cat))  # (decided from the neighbours' coordinates)
        assert _bits(full[k]) == _bits(compact[k]), k
