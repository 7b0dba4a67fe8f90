"""CPU pin of oracle.DynMap (the grid restatement the GPU suite compares the
device map with) against the grid-free reference of tests/ikd_delete_cases.py,
on every case tests/test_gpu_ikd_delete.py runs on the device: after every
step the delete count, the dump (ids and coordinate bits) and the k-NN
(indices and distance bits, in order) of a query set holding every deleted
point's coordinates are equal bit for bit.

Finding (settled against ikd_Tree.cpp Delete_by_range, :626-688, which prunes
on the node's own float range and compares every point with
range_min <= p && range_max > p): a box with an infinite vertex deletes what
the comparisons say, so (-inf, +inf) empties the map.  The oracle's bucket
walk turned the vertices into bucket indices with a cast that is undefined for
non-finite (and > 2^63 buckets) values and then walked an empty bucket range:
it deleted nothing on maps of 27 points or more.  The brute force was right;
ODyn::for_box now scans every id when a bucket index is not representable.
"""
import numpy as np
import pytest

import ikd_delete_cases as dc

f32 = np.float32


def _same(ref, seed):
    rx, ri = ref.dm.dump()
    bx, bi = ref.b.dump()
    assert np.array_equal(ri, bi)
    assert np.array_equal(rx.view(np.uint32), bx.view(np.uint32))
    q = dc.queries(ref, seed)
    gi, gd = ref.dm.knn(q)
    wi, wd = ref.b.knn(q)
    assert np.array_equal(gi, wi), int((gi != wi).any(axis=1).sum())
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))
    return len(bi)


@pytest.mark.parametrize("name", sorted(dc.STEP_CASES))
def test_oracle_equals_brute_force(built, name):
    from livo_amd import synth
    case = dc.STEP_CASES[name]()
    ref = dc.Ref(case["map"])
    _same(ref, 0)
    deleted = 0
    for k, step in enumerate(case["steps"]):
        if step[0] == "delete":
            boxes = dc.resolve(step[1], ref)
            want, got = ref.delete(boxes)
            assert got == want, (name, k, got, want)
            deleted += want
        elif step[0] == "add":
            n0 = ref.b.n_ids
            st = ref.add(dc.resolve(step[1], ref), step[2], step[3])
            assert ref.b.n_ids == n0 + st["added"]
        else:
            _, rst = ref.dm.iekf_update(step[1], step[2], t_LI=synth.T_LI, max_iter=4)
            if not ref.b.alive.any():
                assert rst["effct_feat_num"][0] == 0  # (no map point: no feature)
        _same(ref, k + 1)
    assert deleted > 0


def test_cases_reach_their_edges(built):
    """The builders do what their names say (so neither suite passes on a case that lost its edge)."""
    # faces: vertex_min goes, vertex_max stays, one step inside / outside each; -0.0 at a 0.0 face
    b = dc.Brute(dc.face_points(dc.BOX_A, np.random.default_rng(0), per=1))
    all_hit = b.hit_mask(dc.BOX_A[None])
    for a in range(3):
        lo, hi = dc.BOX_A[a], dc.BOX_A[a + 3]
        o = [x for x in range(3) if x != a]  # (the other two coordinates strictly inside: not the corner points)
        rows = np.all((dc.BOX_A[o] < b.P[:, o]) & (b.P[:, o] < dc.BOX_A[3:][o]), axis=1)
        col, hit = b.P[rows, a], all_hit[rows]
        for v, inside in ((dc.down(lo), False), (lo, True), (dc.up(lo), True),
                          (dc.down(hi), True), (hi, False), (dc.up(hi), False)):
            assert (col == v).any() and (hit[col == v] == inside).all(), (a, v)
    neg0 = (b.P[:, 1] == 0) & np.signbit(b.P[:, 1])
    assert neg0.any() and all_hit[neg0].all()  # 0.0 <= -0.0
    assert all_hit[np.all(b.P == dc.BOX_A[:3], axis=1)].all() and not all_hit[np.all(b.P == dc.BOX_A[3:], axis=1)].any()
    b = dc.Brute(dc.face_points(dc.BOX_B, np.random.default_rng(0), per=1))
    neg0 = (b.P[:, 0] == 0) & np.signbit(b.P[:, 0])
    assert neg0.any() and not b.hit_mask(dc.BOX_B[None])[neg0].any()  # 0.0 > -0.0 is false
    # the odd boxes delete nothing, the infinite box everything
    case = dc.case_faces()
    b = dc.Brute(case["map"])
    assert b.delete_boxes(case["steps"][3][1]) == 0
    assert b.delete_boxes(dc.EVERYTHING) == len(case["map"]) and len(b.dump()[1]) == 0
    # overlap: three points inside three boxes and a box listed twice count once; 300 boxes, few hits
    case = dc.case_overlap()
    b = dc.Brute(case["map"])
    three = case["steps"][0][1]
    per_box = sum(int(dc.Brute(case["map"]).hit_mask(x[None]).sum()) for x in three)
    n = b.delete_boxes(three)
    assert 3 <= n < per_box and b.delete_boxes(three) == 0
    # runs: the arithmetic of dyn_runs_update at the default LIVO_DYN_REBASE = 0.125
    case = dc.case_runs()
    ref = dc.Ref(case["map"])
    base, tomb, counts = dc.RUNS_BASE, 0, []
    for step in case["steps"]:
        _, ids0 = ref.b.dump()
        if step[0] == "delete":
            ref.delete(dc.resolve(step[1], ref))
        else:
            ref.add(step[1], step[2], step[3])
        _, ids1 = ref.b.dump()
        tomb += int((ids0 < base).sum() - (ids1 < base).sum())
        counts.append((tomb, int((ids1 >= base).sum())))
    (t1, d1), (t2, d2), (t3, d3), (t4, d4), (t5, d5) = counts
    assert 0.04 * base < t1 < 0.06 * base and d1 == 0
    assert 0 < d2 <= 0.125 * base and t2 <= 0.25 * base           # a delta grid, no rebase
    assert d3 == 0 and t3 == t2                                    # the delta count back at 0
    assert 0 < d4 <= 0.125 * base and t4 <= 0.25 * base
    assert t5 - t4 > 0.25 * base and t5 > 2 * 0.125 * base         # the tombstone rebase
    # sliding: every step deletes something, one or two slabs
    case = dc.case_sliding()
    b = dc.Brute(case["map"])
    assert 3000 < len(case["map"]) < 8000
    for boxes, _, _ in case["scans"]:
        assert len(boxes) in (1, 2) and b.delete_boxes(boxes) > 0


def test_sliding_map_oracle_equals_brute_force(built):
    from livo_amd import synth
    case = dc.case_sliding()
    ref = dc.Ref(case["map"])
    for k, (boxes, body, st0) in enumerate(case["scans"]):
        want, got = ref.delete(boxes)
        assert got == want and want > 0
        _same(ref, 2 * k)
        rs, rst = ref.dm.iekf_update(body, st0, t_LI=synth.T_LI, max_iter=4)
        assert rst["effct_feat_num"][0] > 100  # (a scan that matches the local map)
        n0 = ref.b.n_ids
        st = ref.dm.map_incremental(body, rs, t_LI=synth.T_LI, filter_size_map=case["filter_size_map"])
        ref.adopt(n0, st["added"])
        _same(ref, 2 * k + 1)
