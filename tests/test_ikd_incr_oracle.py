"""CPU tests of the ikd-Tree incremental map restatement (oracle/livo_oracle.cpp,
section "ikd-Tree incremental map"): KD_TREE::Add_Points with downsampling
(ikd_Tree.cpp:382-457, called by map_incremental with USE_ikdtree,
laser_mapping.cpp:383-384), Delete_Point_Boxes (:501-521) and the k-NN of the
updated map.

Parity status: the reference ships no tests for the ikd-Tree
and its tree cannot be built here, so the restatement is pinned against an
independent numpy replay of Add_Points' per-point rules in float32: the box
and centre of :392-400, half-open Search_by_range boxes (:988-1016), the
strictly-nearer test of :403-411, same_point (:1287-1289) and the box
emptying of :413-416 -- on maps with points within a few ulps of box faces,
exact duplicates and stored points tied at the box centre.
"""
import numpy as np
import pytest

f32 = np.float32


def _box(q, ds):
    lo = (np.floor(q / ds) * ds).astype(f32)
    hi = (lo + ds).astype(f32)
    mid = (lo.astype(np.float64) + (hi - lo).astype(np.float64) / 2.0).astype(f32)
    return lo, hi, mid


def _dist(a, m):
    d = (np.asarray(a, f32) - m).astype(f32)
    return f32(f32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def py_add_points(P, alive, W, ds):
    """Add_Points(W, true) replayed point by point on the point set (P, alive)."""
    ds = f32(ds)
    base = len(P)
    kept = {}
    st = {"events": 0, "added": 0, "deleted": 0, "ambiguous": 0}
    for i, q in enumerate(W):
        lo, hi, mid = _box(q, ds)
        inside = alive & np.all((lo <= P) & (hi > P), axis=1)
        S = [(int(j), P[j]) for j in np.nonzero(inside)[0]]
        S += [(base + k, W[k]) for k in sorted(kept) if np.all((lo <= W[k]) & (hi > W[k]))]
        r, md = None, _dist(q, mid)
        for o, s in S:
            d = _dist(s, mid)
            if d < md:
                md, r = d, (o, s)
        if len(S) > 1 and r is not None:
            if any(o != r[0] and _dist(s, mid) == md and not np.array_equal(s, r[1]) for o, s in S):
                st["ambiguous"] += 1
        same = r is None or bool(np.all(np.abs(q - r[1]).astype(np.float64) < 1e-6))
        if len(S) > 1 or same:
            for o, s in S:
                if r is not None and o == r[0]:
                    continue
                if o >= base:
                    kept.pop(o - base)
                else:
                    alive[o] = False
                    st["deleted"] += 1
            if r is None:
                kept[i] = q
            st["events"] += 1
    new = np.array([W[k] for k in sorted(kept)], f32).reshape(-1, 3)
    st["added"] = len(new)
    return np.concatenate([P, new]), np.concatenate([alive, np.ones(len(new), bool)]), st


def _scene(rng, ds):
    from livo_amd import synth
    pairs, far = synth.centre_tie_points(ds)
    m = np.concatenate([rng.uniform(-6, 6, (1500, 3)), synth.boundary_points(rng, ds, 300, span=12), pairs])
    m = np.concatenate([m, m[:20]]).astype(f32)  # exact duplicates in the initial map
    return m, far


def _batch(rng, ds, m, far):
    from livo_amd import synth
    W = np.concatenate([rng.uniform(-6, 6, (500, 3)), synth.boundary_points(rng, ds, 200, span=12),
                        m[rng.choice(len(m), 30)], far]).astype(f32)
    return W[rng.permutation(len(W))]


@pytest.mark.parametrize("ds", [0.5, 0.3])
def test_add_points_matches_numpy_replay(built, ds):
    import oracle
    rng = np.random.default_rng(21)
    m, far = _scene(rng, ds)
    dm = oracle.DynMap(m)
    P, alive = m.copy(), np.ones(len(m), bool)
    amb = 0
    for _ in range(3):
        W = _batch(rng, ds, m, far)
        st = dm.add_points(W, ds)
        P, alive, rst = py_add_points(P, alive, W, ds)
        assert st == rst
        amb += st["ambiguous"]
        xyz, ids = dm.dump()
        assert np.array_equal(ids, np.nonzero(alive)[0])
        assert np.array_equal(xyz, P[alive])
    if ds == 0.5:
        assert amb > 0  # the centre ties were exercised


def test_add_points_without_downsampling(built):
    import oracle
    rng = np.random.default_rng(2)
    m = rng.uniform(-2, 2, (300, 3)).astype(f32)
    dm = oracle.DynMap(m)
    W = rng.uniform(-2, 2, (100, 3)).astype(f32)
    assert dm.add_points(W, 0.5, downsample=False) == {"events": 0, "added": 100, "deleted": 0, "ambiguous": 0}
    xyz, ids = dm.dump()
    assert np.array_equal(ids, np.arange(400)) and np.array_equal(xyz, np.concatenate([m, W]))


def _knn_numpy(P, ids, q, k=5):
    out_i, out_d = [], []
    for x in q:
        d = (P - x).astype(f32)
        dd = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(f32)
        o = np.lexsort((ids, P[:, 0], dd))[:k]
        out_i.append(ids[o])
        out_d.append(dd[o])
    return np.array(out_i), np.array(out_d)


def test_knn_on_updated_map_matches_numpy(built):
    import oracle
    rng = np.random.default_rng(4)
    m, far = _scene(rng, 0.5)
    dm = oracle.DynMap(np.concatenate([m, rng.uniform(-6, 6, (4000, 3)).astype(f32)]))
    dm.add_points(_batch(rng, 0.5, m, far), 0.5)
    dm.delete_boxes(np.array([[-1, -1, -1, 1, 1, 1]], f32))
    P, ids = dm.dump()
    q = np.concatenate([rng.uniform(-7, 7, (300, 3)), P[:50], P[:20] + f32(1e-3)]).astype(f32)
    gi, gd = dm.knn(q)
    ri, rd = _knn_numpy(P, ids, q)
    assert np.array_equal(gi, ri) and np.array_equal(gd, rd)


def test_delete_boxes_matches_numpy(built):
    import oracle
    rng = np.random.default_rng(6)
    m = rng.uniform(-5, 5, (5000, 3)).astype(f32)
    dm = oracle.DynMap(m)
    boxes = np.array([[-1, -1, -5, 1, 1, 5], [0, 0, 0, 3, 3, 3], [-5, -5, -5, -4, -4, -4]], f32)
    n = dm.delete_boxes(boxes)
    hit = np.zeros(len(m), bool)
    for b in boxes:
        hit |= np.all((b[:3] <= m) & (b[3:] > m), axis=1)
    assert n == hit.sum()
    xyz, ids = dm.dump()
    assert np.array_equal(ids, np.nonzero(~hit)[0])


def test_iekf_on_unchanged_map_equals_static_tree(built, map100k, tree100k):
    """Before any Add_Points the incremental map's search returns the ikd-Tree's neighbours
    (continuous data: no PointType_CMP ties), so the whole IEKF update is identical."""
    import oracle
    from livo_amd import synth
    body, _, _ = synth.make_scan(5_000, 2)
    st = synth.make_state(2)
    dm = oracle.DynMap(map100k)
    a, sa = dm.iekf_update(body, st, t_LI=synth.T_LI, max_iter=4)
    b, sb = tree100k.iekf_update(body, st, t_LI=synth.T_LI, max_iter=4, threads=8)
    assert sa["iterations"] == sb["iterations"] and sa["effct_feat_num"] == sb["effct_feat_num"]
    assert np.array_equal(sa["solution"], sb["solution"])
    assert np.array_equal(a["cov"], b["cov"])


def test_map_incremental_is_world_transform_then_add(built):
    import oracle
    from livo_amd import synth
    rng = np.random.default_rng(8)
    m = synth.make_map(20_000)
    body, _, _ = synth.make_scan(3_000, 1)
    st = synth.make_state(1)
    a, b = oracle.DynMap(m), oracle.DynMap(m)
    sa = a.map_incremental(body, st, t_LI=synth.T_LI, filter_size_map=0.3)
    W = ((body.astype(np.float64) + synth.T_LI) @ st["rot"].T + st["pos"]).astype(f32)
    sb = b.add_points(W, 0.3)
    assert sa == sb and sa["events"] > 0
    for x, y in zip(a.dump(), b.dump()):
        assert np.array_equal(x, y)
    del rng


@pytest.mark.parametrize("ext", ["tilt", "flip"])
def test_map_incremental_under_extrinsic_is_to_world_then_add(built, ext):
    """The same under a tilted and an upside-down LiDAR-IMU extrinsic (tests/extrinsic_cases.py): the
    points map_incremental adds are oracle.to_world's (held to the 60-digit front-end reference under
    tilt), so its counts and map equal Add_Points of them on a twin map."""
    import extrinsic_cases as xc
    import oracle
    from livo_amd import synth
    R_LI, t_LI = xc.ext(ext)
    m = synth.make_map(20_000)
    body, st = xc.scan(3_000, 1, ext)
    a, b = oracle.DynMap(m), oracle.DynMap(m)
    sa = a.map_incremental(body, st, R_LI=R_LI, t_LI=t_LI, filter_size_map=0.3)
    W = oracle.to_world(body, st, R_LI, t_LI)[:, :3]
    assert np.abs(W - xc.world_of(body, st, R_LI, t_LI)).max() < 4e-6  # (metres in float32: the same points)
    sb = b.add_points(W, 0.3)
    assert sa == sb and sa["events"] > 0 and sa["added"] > 0
    for x, y in zip(a.dump(), b.dump()):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    # the scan lands on the room: without R_LI it would not, and the add would differ
    c = oracle.DynMap(m)
    assert c.map_incremental(body, st, R_LI=np.eye(3), t_LI=t_LI, filter_size_map=0.3) != sa
