"""The fused evaluation by search kind: k_iekf_eval (the static map's index runs
alone, 5 waves per SIMD) against k_iekf_eval_gen (every search, LIVO_EVAL_GEN=1).
The two run the same operations on the same data, so every result must be equal
bit for bit: states, iteration statistics, the neighbour records' indices and
squared distances.  One scan of every case is also checked against the CPU
oracle at the bars of tests/test_gpu_parity.py (counts exact, 1e-5 relative on
the state delta of each evaluation)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL_STATE = 1e-5
# an oracle-checked scan first, then an empty scan (its one block only solves), one
# point, a partial wave, a whole wave, a block and one thread (two shard rows)
SIZES = (1000, 0, 1, 63, 64, 257)
CROP = 8.0   # the map: the synthetic room within CROP m of the origin (x, y), at the 200k-point density
INNER = 7.0  # scan points are kept within INNER m, so that every one of them has map points around it


def _synth():
    from livo_amd import synth
    return synth


def _bits(x):
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_bits(v) for v in x]
    return np.asarray(x).tobytes()


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _world(body, st):
    synth = _synth()
    return (body.astype(np.float64) + synth.T_LI) @ np.asarray(st["rot"]).T + np.asarray(st["pos"])  # R_LI = I


def _to_body(world, st):
    synth = _synth()
    return ((world - np.asarray(st["pos"])) @ np.asarray(st["rot"]) - synth.T_LI).astype(np.float32)


@pytest.fixture(scope="module")
def dense_map():
    """5k-20k points: the middle of the room at the density of the 200k-point map
    (the ball runs' radius follows the density: about 1.5 m here)."""
    m = _synth().make_map(200_000)
    keep = (np.abs(m[:, 0]) <= CROP) & (np.abs(m[:, 1]) <= CROP)
    m = np.ascontiguousarray(m[keep])
    assert 5_000 <= len(m) <= 20_000, len(m)
    return m


@pytest.fixture(scope="module")
def dense_tree(built, dense_map):
    import oracle
    return oracle.Tree(dense_map)


def _scan(n, sid):
    """n points of synthetic scan `sid` that hit the room within INNER m of the origin."""
    synth = _synth()
    st = synth.make_state(sid)
    body = synth.make_scan(6 * n + 4000, sid)[0]
    w = _world(body, st)
    body = body[(np.abs(w[:, 0]) <= INNER) & (np.abs(w[:, 1]) <= INNER)]
    assert len(body) >= n, (len(body), n)
    return np.ascontiguousarray(body[:n]), st


def _both(monkeypatch, fn, **env):
    """fn(ctx) in a fresh context on the static kernel (default) and in one on the generic kernel."""
    import livo_amd
    synth = _synth()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = []
    for gen in (None, "1"):
        if gen is None:
            monkeypatch.delenv("LIVO_EVAL_GEN", raising=False)
        else:
            monkeypatch.setenv("LIVO_EVAL_GEN", gen)
        with livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=4) as ctx:
            out.append(fn(ctx))
    monkeypatch.delenv("LIVO_EVAL_GEN", raising=False)
    return out[0], out[1]


def _oracle_check(tree, body, st0, sg, stg, t_LI=None, max_iter=4):
    """tests/test_gpu_parity.py's bars for one scan's update."""
    synth = _synth()
    sr, str_ = tree.iekf_update(body, st0, R_LI=np.eye(3), t_LI=synth.T_LI if t_LI is None else t_LI,
                                max_iter=max_iter)
    assert stg["iterations"] == str_["iterations"]
    assert stg["knn_passes"] == str_["knn_passes"]
    assert stg["converged"] == str_["converged"]
    assert stg["effct_feat_num"] == str_["effct_feat_num"]
    for e in range(stg["iterations"]):
        assert _rel(stg["solution"][e], str_["solution"][e]) < REL_STATE, e
    dth = np.linalg.norm(st0["rot"].T @ sg["rot"] - st0["rot"].T @ sr["rot"])
    assert dth < REL_STATE * max(np.linalg.norm(str_["solution"][:, :3]), 1e-12)
    assert _rel(sg["pos"] - st0["pos"], sr["pos"] - st0["pos"]) < REL_STATE
    assert np.linalg.norm(sg["cov"] - sr["cov"]) / np.linalg.norm(st0["cov"]) < 1e-9


def _run_batch(m, scans, states):
    def run(ctx):
        ctx.map_build(m)
        ctx.set_profiling(2)  # (the level that reads the search counters back)
        sids = [ctx.scan_upload(s) for s in scans]
        out, stats = ctx.iekf_update_batch(sids, states)
        t = ctx.last_timings()
        nn = [ctx.scan_neighbors(s) for s, b in zip(sids, scans) if len(b)]
        # (the hash slots read are kept apart: the run tables are filled on the device by
        # concurrent inserts, so a key's place in its probe sequence, and with it the
        # slot count, differs from one context to the next; the points read do not)
        return {"state": out, "stats": stats, "nn": nn, "slots": t["knn_visits"],
                "counters": [t["knn_points"], t["knn_queries"], t["knn_replays"]]}
    return run


def _same(stat, gen):
    assert _bits({k: v for k, v in stat.items() if k != "slots"}) == _bits({k: v for k, v in gen.items() if k != "slots"})


@pytest.fixture(scope="module")
def ragged():
    pairs = [_scan(n, 60 + k) for k, n in enumerate(SIZES)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def test_ragged_batch(built, dense_map, dense_tree, ragged, monkeypatch):
    """Partial waves, partial blocks, the empty scan's solving block, two shard rows."""
    scans, states = ragged
    assert [len(s) for s in scans] == list(SIZES)
    stat, gen = _both(monkeypatch, _run_batch(dense_map, scans, states))
    _same(stat, gen)
    assert stat["stats"][0]["iterations"] >= 2, stat["stats"][0]  # (evaluations without a search ran too)
    _oracle_check(dense_tree, scans[0], states[0], stat["state"][0], stat["stats"][0])


def test_full_records(built, dense_map, dense_tree, ragged, monkeypatch):
    """LIVO_REC_COMPACT=0: the records' cold halves leave through the shared stage too."""
    scans, states = ragged
    stat, gen = _both(monkeypatch, _run_batch(dense_map, scans, states), LIVO_REC_COMPACT="0")
    _same(stat, gen)
    _oracle_check(dense_tree, scans[0], states[0], stat["state"][0], stat["stats"][0])


def _tie_map(seed=7, n_base=15_000, n_q=1_500, n_dup=40):
    """tests/test_gpu_parity.py's dyadic lattice map: every query has 2 or 4 map points at
    exactly the same float distance (mirror pairs, ordered in the search by x); the first
    n_dup queries also an exact duplicate of one of them (same distance, same x), which
    only the exact replay resolves."""
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


def test_tie_replay(built, monkeypatch):
    """Duplicated map points: replay_wave runs inside the kernel, its subtree caches on the
    evaluation's LDS; the neighbours equal the oracle's, in the reference's order."""
    import oracle
    m, q = _tie_map()
    assert 5_000 <= len(m) <= 20_000
    st0 = {"rot": np.eye(3), "pos": np.zeros(3), "vel": np.zeros(3), "bias_g": np.zeros(3),
           "bias_a": np.zeros(3), "gravity": np.array([0.0, 0.0, -9.81]), "cov": np.eye(18) * 1e-3}

    def run(ctx):
        ctx.set_params(t_LI=[0.0, 0.0, 0.0], max_iterations=0)
        ctx.map_build(m)
        ctx.set_profiling(2)
        sid = ctx.scan_upload(q)
        out, stats = ctx.iekf_update(sid, st0)  # one evaluation: the search at the identity pose
        replays = ctx.last_timings()["knn_replays"]
        idx, d = ctx.scan_neighbors(sid)
        return {"replays": replays, "idx": idx, "d": d, "state": out, "stats": stats}

    stat, gen = _both(monkeypatch, run)
    assert stat["replays"] > 0 and stat["replays"] == gen["replays"]
    _same(stat, gen)
    tree = oracle.Tree(m)
    idx_r, d_r, _ = tree.knn(q, 5)
    np.testing.assert_array_equal(stat["d"], d_r)
    np.testing.assert_array_equal(stat["idx"], idx_r)
    _oracle_check(tree, q, st0, stat["state"], stat["stats"], t_LI=np.zeros(3), max_iter=0)


def test_run_search_fallbacks(built, dense_map, dense_tree, monkeypatch):
    """Queries in mid-air, 1-3 m off every surface: their ball run does not certify them
    (the list's bound reaches past the ball), so vrun_search's cell run and its serial
    walk beyond the cube find their neighbours."""
    n, n_far = 600, 150
    body, st = _scan(n, 70)
    rng = np.random.default_rng(5)
    cand = np.stack([rng.uniform(-5, 5, 4000), rng.uniform(-5, 5, 4000), rng.uniform(0.0, 0.8, 4000)], axis=1)
    _, d_c, _ = dense_tree.knn(cand.astype(np.float32), 5)
    ok = (d_c[:, 0] >= 1.0) & (d_c[:, 4] <= 9.0)  # nearest point at 1 m or more, the 5th within 3 m
    assert ok.sum() >= n_far, ok.sum()
    far = _to_body(cand[ok][:n_far], st)
    mixed = np.concatenate([body[:200], far, body[200:]])  # (a block of them, whole waves among them)
    stat, gen = _both(monkeypatch, _run_batch(dense_map, [mixed, body], [st, st]))
    _same(stat, gen)
    visits, queries = stat["slots"], stat["counters"][1]
    assert queries == len(mixed) + len(body)
    # the ball path reads one hash slot per query (or a few of one probe sequence); a
    # query it leaves uncertified reads the cell runs' table as well: at least n_far more
    assert visits >= queries + n_far, (visits, queries)
    # against the same batch without the mid-air block: those queries account for the excess
    stat0, _ = _both(monkeypatch, _run_batch(dense_map, [body, body], [st, st]))
    v0, q0 = stat0["slots"], stat0["counters"][1]
    assert (visits - queries) - (v0 - q0) >= n_far, (visits, queries, v0, q0)
    _oracle_check(dense_tree, mixed, st, stat["state"][0], stat["stats"][0])


def test_kernel_selection(built, dense_map, dense_tree, monkeypatch):
    """The launcher's rule: a map without vertex runs (LIVO_VRUNS=0) and an incremental map
    (after livo_map_add_points) take the generic kernel; the static kernel compiles neither
    search, so the oracle's answers there prove the selection."""
    import livo_amd
    import oracle
    synth = _synth()
    body, st = _scan(1000, 71)
    monkeypatch.delenv("LIVO_EVAL_GEN", raising=False)
    monkeypatch.setenv("LIVO_VRUNS", "0")
    with livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=4) as ctx:
        ctx.map_build(dense_map)
        sid = ctx.scan_upload(body)
        sg, stg = ctx.iekf_update(sid, st)
        idx, d = ctx.scan_neighbors(sid)
    _oracle_check(dense_tree, body, st, sg, stg)
    monkeypatch.delenv("LIVO_VRUNS")
    with livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=4) as ctx:  # (the static kernel: same neighbours)
        ctx.map_build(dense_map)
        sid = ctx.scan_upload(body)
        sg1, stg1 = ctx.iekf_update(sid, st)
        idx1, d1 = ctx.scan_neighbors(sid)
        assert _bits([idx, d]) == _bits([idx1, d1])
        assert stg1["iterations"] == stg["iterations"] and stg1["effct_feat_num"] == stg["effct_feat_num"]
        # the map becomes incremental
        dm = oracle.DynMap(dense_map)
        add_body, add_st = _scan(2000, 72)
        W = _world(add_body, add_st).astype(np.float32)
        g = ctx.map_add_points(W, 0.5)
        r = dm.add_points(W, 0.5)
        assert {k: g[k] for k in ("events", "added", "deleted", "ambiguous")} == r
        sg2, stg2 = ctx.iekf_update(sid, st)
    rs, rst = dm.iekf_update(body, st, t_LI=synth.T_LI, max_iter=4)
    assert stg2["iterations"] == rst["iterations"] and stg2["effct_feat_num"] == rst["effct_feat_num"]
    for e in range(stg2["iterations"]):
        assert _rel(stg2["solution"][e], rst["solution"][e]) < REL_STATE, e
    assert _rel(sg2["pos"] - st["pos"], rs["pos"] - st["pos"]) < REL_STATE
