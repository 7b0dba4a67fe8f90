"""The iVox search's overflow cascade and depth-limit exits, branch by branch, against the oracle.

A query moves from the team search (a list of up to 128) to k_ivox_knn_wave_list (every raw point at
once up to 512, streaming past that) to the big pass (k_ivox_knn_big_wave while the slice fits 64 KB
of LDS, k_ivox_knn_big beyond), and every parallel nth_element leaves through a fallback when
introselect's depth limit runs out.  The scenes (tests/ivox_cascade_cases.py) put a query on each
branch on purpose; tests/test_ivox_oracle.py::test_cascade_scenes_are_what_they_claim shows with numpy
alone that they do.  Everything is compared with oracle.Ivox (which calls std::nth_element) bit for
bit: counts, ids, distance bits and order.

The context is this module's own.  livo_ivox_init frees the iVox state and starts from an empty one
(ivox_free assigns IvoxDev{}), so big_slice starts again from the new map's largest grid at every
ivox_init and no earlier scene's larger slice carries over: the LDS-edge scenes get the slice they ask
for, which they assert through max_grid_points.
"""
import numpy as np
import pytest

import ivox_cascade_cases as cc

pytestmark = pytest.mark.gpu

KINDS = [None, "team", "thread", "wave"]


@pytest.fixture(scope="module")
def adv_cli(tmp_path_factory):
    return cc.build_cli(tmp_path_factory.mktemp("nth_adversary"))


@pytest.fixture(scope="module")
def cctx(built):
    import livo_amd
    ctx = livo_amd.Context(0, t_LI=np.zeros(3), max_iterations=0)
    ctx.set_backend(livo_amd.BACKEND_IVOX)
    yield ctx
    ctx.close()


def _set_kind(monkeypatch, kind):
    if kind is None:
        monkeypatch.delenv("LIVO_IVOX_KIND", raising=False)
    else:
        monkeypatch.setenv("LIVO_IVOX_KIND", kind)


def _pair(ctx, scene):
    import oracle
    ctx.ivox_init(resolution=scene["res"], nearby_type=scene["nearby_type"])
    iv = oracle.Ivox(resolution=scene["res"], nearby_type=scene["nearby_type"])
    ctx.ivox_add_points(scene["points"])
    iv.add_points(scene["points"])
    return iv


def _knn_equal(ctx, iv, q, max_num=5, max_range=5.0):
    gi, gd, gc = ctx.ivox_knn(q, max_num, max_range)
    ri, rd, _, rc = iv.knn(q, max_num, max_range)
    assert np.array_equal(gc, rc)
    assert np.array_equal(gi, ri)
    assert np.array_equal(gd.view(np.uint32), rd.view(np.uint32))
    return gc


def _run(ctx, scene):
    iv = _pair(ctx, scene)
    cnt = _knn_equal(ctx, iv, scene["queries"], scene["max_num"], scene["max_range"])
    assert np.all(cnt == scene["max_num"])
    return iv


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("first,length", cc.DEPTH_CASES)
def test_depth_limit_every_kind(cctx, adv_cli, monkeypatch, kind, first, length):
    """An adversarial grid selected at nth = first + 4.  Up to a list of 128 the team heap-selects on
    its lane 0 and the per-thread kind runs sel_nth_element's heap select; past that the wave search
    (all at once at 300, streaming at 500 / 501, beyond its staging at 600) hands the query to
    k_ivox_knn_big_wave, which runs out of depth on the same list and redoes the query on its lane 0
    in the block's global slice."""
    _set_kind(monkeypatch, kind)
    _run(cctx, cc.depth_scene(adv_cli, first, length))


_CAPACITY = cc.capacity_scenes()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("scene", _CAPACITY, ids=[s["name"] for s in _CAPACITY])
def test_capacity_edges(cctx, monkeypatch, kind, scene):
    """Lists of exactly 128 entries (one grid, or 5 survivors + 123) stay in the team and in the
    per-thread kind's private array, 129 go on; only in-range points count.  The wave search loads 512
    raw points at once and streams 513; streaming holds 5 + 507 and hands 5 + 508 to the big pass."""
    _set_kind(monkeypatch, kind)
    _run(cctx, scene)


@pytest.mark.parametrize("kind", [None, "thread", "wave"])
@pytest.mark.parametrize("over", [False, True], ids=["fits-64KB", "one-more"])
def test_lds_edge(cctx, monkeypatch, kind, over):
    """The largest grid whose slice fits 64 KB of dynamic LDS (k_ivox_knn_big_wave) and one point more
    (k_ivox_knn_big, global-memory slices), queried from the grid's own cell and from its neighbours,
    on a lattice with exact duplicate distances."""
    _set_kind(monkeypatch, kind)
    scene = cc.lds_scene(over)
    iv = _pair(cctx, scene)
    assert cctx.ivox_info()["max_grid_points"] == scene["expect"]["max_grid"] == cc.lds_edge_grid() + over
    cnt = _knn_equal(cctx, iv, scene["queries"], scene["max_num"], scene["max_range"])
    assert np.all(cnt == 5)


def _identity_state():
    from livo_amd import synth
    st = synth.make_state(0)
    st["rot"] = np.eye(3)
    st["pos"] = np.zeros(3)
    return st


@pytest.mark.parametrize("name", ["depth-0-300", "depth-5-500", "depth-0-24", "lds-edge", "lds-over"])
def test_cascade_in_iekf_evaluation(cctx, adv_cli, monkeypatch, name):
    """The job / slot form of the same kernels: one IEKF evaluation (max_iterations = 0) of a batch of
    scans whose points are the scene's queries, at the identity pose and extrinsic (world = body,
    exactly), so each stream group's overflow pass works in its own scratch.  The neighbour records
    equal the oracle's bit for bit."""
    import oracle
    monkeypatch.delenv("LIVO_IVOX_KIND", raising=False)
    if name.startswith("depth"):
        _, f, n = name.split("-")
        scene = cc.depth_scene(adv_cli, int(f), int(n))
    else:
        scene = cc.lds_scene(name == "lds-over")
    iv = _pair(cctx, scene)
    st = _identity_state()
    q = scene["queries"]
    bodies = [q, q[::-1].copy(), q[: len(q) // 2].copy(), q[1::2].copy(), q, q[::3].copy()]
    sids = [cctx.scan_upload(b) for b in bodies]
    try:
        cctx.iekf_update_batch(sids, [st] * len(sids))
        for sid, b in zip(sids, bodies):
            cache = oracle.new_cache(len(b))
            iv.iekf_update(b, st, cache, t_LI=np.zeros(3), max_iter=0)
            gi, gd = cctx.scan_neighbors(sid)
            assert np.all(cache["cnt"] == 5)
            assert np.array_equal(gi, cache["idx"])
            assert np.array_equal(gd.view(np.uint32), cache["d"].view(np.uint32))
    finally:
        for s in sids:
            cctx.scan_release(s)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("res", [0.5, 0.2])
def test_keys_and_range_edges(cctx, monkeypatch, kind, res):
    """Pos2Grid's half-away rounding at exact k + 0.5 products (both signs, one ulp either side, -0.0)
    for points (ivox_dump equals the oracle's grids) and queries; the strict d < max_range^2 with a
    point at d == range2 exactly, one ulp inside and one outside; max_num 1 and 5; queries with 1..4
    candidates, whose records are padded as the oracle pads (-1, inf)."""
    import oracle
    _set_kind(monkeypatch, kind)
    pts, exact = cc.half_product_points(res)
    assert exact.sum() >= 6
    # clusters of 1..4 points far from everything else (and from each other)
    iso = np.concatenate([np.array([[100.0 * c + 0.01 * k, 50.0, 0.0] for k in range(c)], np.float32)
                          for c in (1, 2, 3, 4)])
    # the range edge: a point e beyond the query at x = 10 (the next cell), and the floats either side
    # of it; the differences are exact, and so are e, e^2 and max_range = e: d == range2 on the first
    e = np.float32(0.375 if res == 0.5 else 0.125)
    base = np.float32(10.0)
    p = base + e
    edge = np.array([[p, 0, 0], [np.nextafter(p, np.float32(0)), 0, 0], [np.nextafter(p, np.float32(99)), 0, 0]],
                    np.float32)
    allp = np.concatenate([pts, iso, edge])
    cctx.ivox_init(resolution=res, nearby_type=18)
    iv = oracle.Ivox(resolution=res, nearby_type=18)
    cctx.ivox_add_points(allp)
    iv.add_points(allp)
    assert cc.by_grid_dev(*cctx.ivox_dump()) == cc.by_grid_oracle(iv)
    qiso = np.array([[100.0 * c, 50.0, 0.0] for c in (1, 2, 3, 4)], np.float32)
    qedge = np.array([[base, 0, 0]], np.float32)
    d_edge = cc.dist2(edge, qedge[0]).astype(np.float64)
    for max_num in (1, 5):
        cnt = _knn_equal(cctx, iv, pts, max_num, 5.0)   # queries at the half products themselves
        assert np.all(cnt >= 1)
        cnt = _knn_equal(cctx, iv, qiso, max_num, 5.0)
        assert cnt.tolist() == [min(c, max_num) for c in (1, 2, 3, 4)]
        # max_range at the middle point's distance, and the doubles either side of it
        r0 = float(e)
        assert r0 * r0 == d_edge[0]
        for r in (r0, np.nextafter(r0, 0.0), np.nextafter(r0, 1.0), float(np.sqrt(d_edge.min())),
                  float(np.sqrt(d_edge.max()))):
            cnt = _knn_equal(cctx, iv, qedge, max_num, r)
            want = int((d_edge < r * r).sum())
            assert cnt[0] == (min(want, max_num) if want else -1)
    assert int((d_edge < d_edge[0]).sum()) == 1 and int((d_edge > d_edge[0]).sum()) == 1


def test_key_limit(cctx, monkeypatch):
    """Cells at +-kIvMaxKey are stored and found; a point one cell beyond makes livo_ivox_add_points
    fail with LIVO_E_RANGE and leaves the map unchanged, as include/livo.h documents (the oracle, like
    the reference, has no such limit: the batch is not given to it).  Queries up to kIvMaxKey + 8 cells
    are answered (from kIvMaxKey + 1 the grid at the limit is a neighbour), past that nothing is found."""
    import livo_amd
    import oracle
    monkeypatch.delenv("LIVO_IVOX_KIND", raising=False)
    res = 0.5
    lim = np.float32(cc.MAX_KEY * res)  # 524256: the product with inv_resolution is kIvMaxKey exactly
    pts = np.array([[lim, 0, 0], [-lim, 0, 0], [0, lim, -lim], [lim, lim, lim], [lim - 0.5, 0, 0], [lim, 0.1, 0]],
                   np.float32)
    assert np.abs(cc.keys_of(pts, res)).max() == cc.MAX_KEY
    cctx.ivox_init(resolution=res, nearby_type=18)
    iv = oracle.Ivox(resolution=res, nearby_type=18)
    cctx.ivox_add_points(pts)
    iv.add_points(pts)
    assert cc.by_grid_dev(*cctx.ivox_dump()) == cc.by_grid_oracle(iv)
    for bad in ([lim + 0.5, 0, 0], [0, -lim - 0.5, 0], [0, 0, 3e9]):
        batch = np.array([[1, 2, 3], bad, [4, 5, 6]], np.float32)
        assert np.abs(cc.keys_of(batch, res)).max() > cc.MAX_KEY
        with pytest.raises(livo_amd.LivoError) as ei:
            cctx.ivox_add_points(batch)
        assert ei.value.code == -6  # LIVO_E_RANGE
        assert cc.by_grid_dev(*cctx.ivox_dump()) == cc.by_grid_oracle(iv)
        assert cctx.ivox_info()["ids_issued"] == iv.info()["ids_issued"] == len(pts)
    q = np.array([[lim + 0.5 * k, 0, 0] for k in range(-2, 12)] + [[-lim - 0.5 * k, 0, 0] for k in range(-2, 12)] +
                 [[3 * lim, 0, 0], [0, lim + 0.5, -lim - 0.5], [lim + 4.5, lim, lim]], np.float32)
    assert np.abs(cc.keys_of(q, res)).max() > cc.MAX_KEY + 8
    cnt = _knn_equal(cctx, iv, q, 5, 5.0)
    assert (cnt > 0).sum() >= 8 and (cnt == -1).sum() >= 8
