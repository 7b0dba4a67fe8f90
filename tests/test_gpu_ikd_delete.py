"""livo_map_delete_boxes (KD_TREE::Delete_Point_Boxes, ikd_Tree.cpp:501-521) and
what runs on the map it leaves -- the grid rebuilds (sorted, merged, fused
into Add_Points' pass), the runs' deletion marks, delta grid and rebases, the
na == 0 guards -- against the grid-free reference of tests/ikd_delete_cases.py
(pinned on the CPU in tests/test_ikd_delete_reference.py).

Every assertion is exact: after each call the returned count,
map_info()["num_points"], the dump (ids and coordinate bits) and the k-NN
(indices and distance bits, in order) of a query set holding the coordinates
of every point deleted so far, surviving points and random points.  The one
tolerance is test_gpu_ikd_incr.py's REL_STATE on IEKF states.
"""
import ctypes as C

import numpy as np
import pytest

import ikd_delete_cases as dc

pytestmark = pytest.mark.gpu
f32 = np.float32
REL_STATE = 1e-5
KEYS = ("events", "added", "deleted", "ambiguous")
FIXED_Q = np.random.default_rng(1).uniform(-5, 5, (200, 3)).astype(f32)


@pytest.fixture(scope="module")
def ictx(built):
    import livo_amd
    from livo_amd import synth
    ctx = livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=4)
    yield ctx
    ctx.close()


def _bytes(*arrays):
    return tuple(np.ascontiguousarray(a).tobytes() for a in arrays)


def _check(ctx, ref, seed, built_map=False):
    """num_points, the dump and the k-NN of the device map equal the brute force's; returns their bytes.
    built_map: before the first incremental call the search is the static map's, which orders neighbours
    within 1e-10 of each other as the reference's tree does, not by (d, x, id): only
    the random queries then, whose neighbours are no such near-ties."""
    bx, bi = ref.b.dump()
    assert ctx.map_info()["num_points"] == len(bi)
    gx, gi = ctx.map_dump()
    assert np.array_equal(gi, bi)
    assert np.array_equal(gx.view(np.uint32), bx.view(np.uint32))
    q = FIXED_Q if built_map else dc.queries(ref, seed)
    ki, kd = ctx.knn(q)
    wi, wd = ref.b.knn(q)
    assert np.array_equal(ki, wi), (seed, int((ki != wi).any(axis=1).sum()))
    assert np.array_equal(kd.view(np.uint32), wd.view(np.uint32))
    return _bytes(gx, gi, *ctx.knn(FIXED_Q))  # (one query set for all steps: equal maps give equal bytes)


def _iekf_counts(ctx, ref, body, st):
    from livo_amd import synth
    sid = ctx.scan_upload(body)
    _, gst = ctx.iekf_update(sid, st)
    ctx.scan_release(sid)
    _, rst = ref.dm.iekf_update(body, st, t_LI=synth.T_LI, max_iter=4)
    assert gst["iterations"] == rst["iterations"] and gst["effct_feat_num"] == rst["effct_feat_num"]
    return gst


def _run(ctx, case, on_step=None):
    """The case's steps on the device map and on the reference, everything compared after each."""
    ctx.map_build(case["map"])
    ref = dc.Ref(case["map"])
    rec = [_check(ctx, ref, 0, built_map=True)]
    for k, step in enumerate(case["steps"]):
        before = ctx.map_rebuilds()
        if step[0] == "delete":
            boxes = dc.resolve(step[1], ref)
            want, orc = ref.delete(boxes)
            assert orc == want
            got = ctx.map_delete_boxes(boxes)
            assert got == want, (k, got, want)
            rec.append(got)
        elif step[0] == "add":
            W = dc.resolve(step[1], ref)
            n0 = ref.b.n_ids
            r = ref.add(W, step[2], step[3])
            g = ctx.map_add_points(W, step[2], downsample=step[3])
            assert {x: g[x] for x in KEYS} == r, (k, g, r)
            assert g["map_points"] == int(ref.b.alive.sum())
            ids = ctx.map_dump()[1]
            assert np.array_equal(ids[ids >= n0], np.arange(n0, n0 + r["added"]))  # the next ids, none reused
            rec.append(tuple(g[x] for x in KEYS))
        else:
            gst = _iekf_counts(ctx, ref, step[1], step[2])
            if not ref.b.alive.any():
                assert gst["effct_feat_num"][0] == 0
        rec.append(_check(ctx, ref, k + 1))
        if on_step:
            on_step(k, step, before, ctx.map_rebuilds())
    return rec, ref


@pytest.mark.parametrize("name", ["faces", "overlap", "n_ids_1", "n_ids_255", "n_ids_256", "n_ids_257",
                                  "session_added", "cells_and_empty"])
def test_delete_cases(ictx, name):
    """faces: points on vertex_min (deleted) and vertex_max (kept) of each axis and one float32 step to
    each side, negative and positive faces, a 0.0 face with a point at -0.0; boxes with min == max,
    inverted, with NaN vertices, far outside (nothing deleted) and (-inf, +inf) (everything); no boxes
    as the first incremental call and later (0, nothing changes).
    overlap: points inside three boxes and a box listed twice count once; the same boxes again delete 0;
    300 boxes with the hits in the first, the last, and both.
    n_ids_*: 1, 255, 256 and 257 ids (the launch's blocks of 256), the first and last id deleted, twice.
    session_added: a downsampled and a plain batch added, then boxes taking base ids, added ids and
    both; Add_Points into boxes whose stored point was just deleted keeps the new points; new ids go on
    from the old n_ids.
    cells_and_empty: whole clusters (the cells of the first, the last and a middle point of the grid's
    key order) deleted, then everything (num_points 0, an empty dump, -1 / inf neighbours, an IEKF update
    with the oracle's counts), a deletion on the empty map, then adds with and without downsampling.
    (The grid's cell count has no getter; the k-NN of the deleted coordinates is what a stale cell would
    break.)"""
    rec, ref = _run(ictx, dc.STEP_CASES[name]())
    assert ref.b.n_ids > len(ref.b.dump()[1])  # something was deleted
    if name == "faces":
        assert rec[1] == 0 and rec[2] == rec[0]  # no boxes on the freshly built map: nothing changed
        assert rec[7] == 0 and rec[9] == 0 and rec[8] == rec[10] == rec[6]  # odd boxes, no boxes
        assert rec[11] == 0  # the same boxes again


def test_delete_then_fused_add(built, monkeypatch):
    """dyn_rebuild after a delete leaves the grid covering every id, so the next downsampled add may run
    the merged rebuild inside its own pass (map_rebuilds()[3]), whose survivor ranks (k_scan_flags) then
    skip the points the delete took: it did so on an add directly after a delete, the map and k-NN are
    the reference's throughout, and LIVO_DYN_MERGE=0 (a sort at every change) gives the same bytes."""
    import livo_amd
    from livo_amd import synth
    case = dc.case_fused()
    out = {}
    for merge in ("1", "0"):
        monkeypatch.setenv("LIVO_DYN_MERGE", merge)
        fused_after_delete = []

        def on_step(k, step, before, after):
            if step[0] == "add" and k > 0 and case["steps"][k - 1][0] == "delete":
                fused_after_delete.append(after[3] - before[3])

        with livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=4) as ctx:
            rec, _ = _run(ctx, case, on_step)
            out[merge] = (rec, ctx.map_rebuilds(), fused_after_delete)
    (a, ra, fa), (b, rb, fb) = out["1"], out["0"]
    assert len(fa) == 5 and max(fa) == 1, fa  # the fused pass ran directly after a delete
    assert rb[1] == 0 and rb[3] == 0 and max(fb) == 0
    assert ra[1] >= 1 and a == b


@pytest.fixture(scope="module")
def runs_expected(built):
    """case_runs on the reference, once for the four settings: per step the call's result, the scan
    (the coordinates of every point deleted so far, survivors, random points) and its brute-force k-NN."""
    case = dc.case_runs()
    ref = dc.Ref(case["map"])
    out = []
    for k, step in enumerate(case["steps"]):
        arg = dc.resolve(step[1], ref)
        if step[0] == "delete":
            want, orc = ref.delete(arg)
            assert want == orc
        else:
            want = ref.add(arg, step[2], step[3])
        q = dc.queries(ref, 50 + k, 300, 300)
        out.append((step, arg, want, ref.b.dump(), q, ref.b.knn(q)))
    return case["map"], out


@pytest.mark.parametrize("mode", ["default", "rebase_every_change", "never_rebase", "cell_walk"])
def test_runs_under_deletion(runs_expected, monkeypatch, mode):
    """The fused IEKF search on the runs of the base point set (LIVO_DYN_RUNS=1) while deletions mark base
    points (NaN tombstones), empty the delta grid and force a rebase.  The built map's cell runs exist
    for any map of at least one point (livo_map_build builds them whenever M > 0); this one has 4,000, so
    the thresholds of dyn_runs_update are whole numbers: at the default LIVO_DYN_REBASE = 0.125 the
    delta may hold 500 points and the marks 1,000.  Steps: a delete of 5% of the base (marks, no delta);
    an add (a delta grid); a delete of every point added since the base (the delta count back to 0); an
    add; a delete of 30% of the base (marks > 1,000: the tombstone rebase; with LIVO_DYN_REBASE=99 never,
    with 1e-9 at every change).  tests/test_ikd_delete_reference.py checks that arithmetic on the case.
    No counter of the ABI shows that the runs are live or that a rebase ran; the settings differ only
    in which structure serves the search, and each must give the brute force's records.
    After every step one evaluation (max_iterations 0: one search at the state, the identity, so the
    scan's world points are its own): every point's neighbour record equals the brute-force k-NN on the
    updated map, bit for bit; the scan holds the coordinates of every point deleted so far."""
    import livo_amd
    import oracle
    from livo_amd import synth
    monkeypatch.setenv("LIVO_DYN_RUNS", "0" if mode == "cell_walk" else "1")
    monkeypatch.delenv("LIVO_DYN_REBASE", raising=False)
    if mode == "rebase_every_change":
        monkeypatch.setenv("LIVO_DYN_REBASE", "1e-9")
    if mode == "never_rebase":
        monkeypatch.setenv("LIVO_DYN_REBASE", "99")
    m, steps = runs_expected
    st = synth.make_state(0)
    st["rot"], st["pos"] = np.eye(3), np.zeros(3)
    with livo_amd.Context(0, t_LI=np.zeros(3), max_iterations=0) as ctx:
        ctx.map_build(m)
        for k, (step, arg, want, (bx, bi), q, (wi, wd)) in enumerate(steps):
            if step[0] == "delete":
                assert ctx.map_delete_boxes(arg) == want
            else:
                g = ctx.map_add_points(arg, step[2], downsample=step[3])
                assert {x: g[x] for x in KEYS} == want
            assert ctx.map_info()["num_points"] == len(bi)
            gx, gi = ctx.map_dump()
            assert np.array_equal(gi, bi) and np.array_equal(gx.view(np.uint32), bx.view(np.uint32))
            assert np.array_equal(oracle.to_world(q, st, np.eye(3), np.zeros(3))[:, :3].view(np.uint32),
                                  q.view(np.uint32))
            sid = ctx.scan_upload(q)
            _, gst = ctx.iekf_update(sid, st)
            assert gst["iterations"] == 1
            ni, nd = ctx.scan_neighbors(sid)
            ctx.scan_release(sid)
            assert np.array_equal(ni, wi), (mode, k, int((ni != wi).any(axis=1).sum()))
            assert np.array_equal(nd.view(np.uint32), wd.view(np.uint32)), (mode, k)


@pytest.mark.parametrize("mode", ["cell_walk", "runs"])
def test_sliding_local_map(built, monkeypatch, mode):
    """The shape lasermap_fov_segment gives the call: six scans, before each one or two slabs behind the
    sensor deleted, then a four-iteration IEKF update against the oracle's (counts exact, state
    REL_STATE) and map_incremental of the scan at the updated state with downsampling; the map, its
    k-NN and the counts checked after every delete and every add.  With the cell walk and with the
    runs at the default rebase."""
    import livo_amd
    from livo_amd import synth
    monkeypatch.setenv("LIVO_DYN_RUNS", "1" if mode == "runs" else "0")
    monkeypatch.delenv("LIVO_DYN_REBASE", raising=False)
    case = dc.case_sliding()
    ref = dc.Ref(case["map"])
    fs = case["filter_size_map"]
    with livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=4) as ctx:
        ctx.map_build(case["map"])
        for k, (boxes, body, st0) in enumerate(case["scans"]):
            want, orc = ref.delete(boxes)
            assert orc == want and want > 0
            assert ctx.map_delete_boxes(boxes) == want
            _check(ctx, ref, 2 * k)
            sid = ctx.scan_upload(body)
            gs, gst = ctx.iekf_update(sid, st0)
            rs, rst = ref.dm.iekf_update(body, st0, t_LI=synth.T_LI, max_iter=4)
            assert gst["iterations"] == rst["iterations"] and gst["effct_feat_num"] == rst["effct_feat_num"]
            assert rst["effct_feat_num"][0] > 100
            for e in range(gst["iterations"]):
                rel = np.linalg.norm(gst["solution"][e] - rst["solution"][e]) / np.linalg.norm(rst["solution"][e])
                assert rel < REL_STATE, (k, e, rel)
            # both maps take the points at the device's updated state
            n0 = ref.b.n_ids
            cat, g = ctx.map_incremental(sid, gs, filter_size_map=fs)
            r = ref.dm.map_incremental(body, gs, t_LI=synth.T_LI, filter_size_map=fs)
            ref.adopt(n0, r["added"])
            assert {x: g[x] for x in KEYS} == r, (k, g, r)
            assert g["map_points"] == int(ref.b.alive.sum())
            ctx.scan_release(sid)
            _check(ctx, ref, 2 * k + 1)


def test_delete_boxes_contract(built):
    """nb < 0 and nb > 0 with NULL boxes: LIVO_E_INVALID; no map: LIVO_E_NOMAP; a submitted, uncollected
    batch: LIVO_E_BUSY; NULL `deleted` is accepted.  After each refused call the dump is byte-identical."""
    import livo_amd
    from livo_amd import synth
    L = livo_amd.load()
    rng = np.random.default_rng(107)
    m = rng.uniform(-3, 3, (1500, 3)).astype(f32)
    boxes = np.array([[-1, -1, -1, 1, 1, 1]], f32)
    bp = boxes.ctypes.data_as(C.c_void_p)
    n = C.c_int64(-5)
    with livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=4) as ctx:
        assert L.livo_map_delete_boxes(ctx.h, bp, 1, C.byref(n)) == -3  # LIVO_E_NOMAP
        assert L.livo_map_delete_boxes(None, bp, 1, C.byref(n)) == -1
        with pytest.raises(livo_amd.LivoError) as e:
            ctx.map_dump()
        assert e.value.code == -3
        ctx.map_build(m)
        ref = dc.Ref(m)
        ref.delete(np.array([[2, 2, 2, 3, 3, 3]], f32))
        assert ctx.map_delete_boxes(np.array([[2, 2, 2, 3, 3, 3]], f32)) > 0  # (the incremental map is live)
        d0 = _check(ctx, ref, 0)
        assert L.livo_map_delete_boxes(ctx.h, bp, -1, C.byref(n)) == -1  # LIVO_E_INVALID
        assert _check(ctx, ref, 0) == d0
        assert L.livo_map_delete_boxes(ctx.h, None, 1, C.byref(n)) == -1
        assert _check(ctx, ref, 0) == d0
        sid = ctx.scan_upload(synth.make_scan(500, 1)[0])
        st = synth.make_state(1)
        t = ctx.iekf_update_batch_submit([sid], [st])
        assert L.livo_map_delete_boxes(ctx.h, bp, 1, C.byref(n)) == -8  # LIVO_E_BUSY
        ctx.iekf_update_batch_wait(t, 1)
        ctx.scan_release(sid)
        assert _check(ctx, ref, 0) == d0
        want, _ = ref.delete(boxes)
        assert want > 0 and L.livo_map_delete_boxes(ctx.h, bp, 1, None) == 0  # NULL deleted
        assert _check(ctx, ref, 1) != d0
        assert L.livo_map_delete_boxes(ctx.h, None, 0, C.byref(n)) == 0 and n.value == 0  # no boxes, NULL: fine
