"""The device's three copies of the per-point plane pass on the neighbourhoods of oracle/plane_ref.py.

fit_plane / hshare_point of the unfused k_hshare, the fit inside the fused evaluation and the IKFoM
row kernel each restate esti_plane with hand-unrolled register arrays; the room scans of the other
tests take one path through it (full rank, tau != 0, four of the six permutations, no ties, finite
normals: tests/test_plane_reference.py::test_room_scan_branches).  Here they run on rank-2, rank-1
and rank-0 clusters, zero columns, tau = 0 (exact and by underflow), bit-equal column norms,
recomputed norms, fits at 200-5000 m and planes through the origin region, a cluster of denormal squares, and on four sweeps that
step a gate quantity by nextafter through its threshold; tests/test_plane_reference.py holds the
oracle's side of the same cases against an mpmath reference.

Bars: neighbours, planes, residuals and flags bit for bit (NaN through view(uint32)), HTH / HTL
1e-9, counts exact, the IEKF solution 1e-5, the IKFoM dx 1e-5 of its own norm.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL_HTH = 1e-9
REL_STATE = 1e-5
ZERO3 = np.zeros(3)
SOLVE_SHEETS = tuple(range(9))  # one sheet of every origin-bound kind; the sweep and origin-body sheets are added


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _hs_equal(g, r, tag, found=None):
    rows = slice(None) if found is None else found
    assert np.array_equal(g["nn_idx"][rows], r["cache"]["idx"][rows]), tag
    assert np.array_equal(_bits(g["nn_d"][rows]), _bits(r["cache"]["d"][rows])), tag
    assert np.array_equal(_bits(g["normvec"]), _bits(r["normvec"])), tag
    assert np.array_equal(g["sel"], r["sel"]), tag
    assert g["effct"] == r["effct"], tag
    assert _rel(g["HTH"], r["HTH"]) < REL_HTH, tag
    assert _rel(g["HTL"], r["HTL"]) < REL_HTH, tag


@pytest.fixture(scope="module")
def sheets(built):
    import plane_ref as pr
    return pr.sheets()


@pytest.fixture(scope="module")
def ctx(built):
    import livo_amd
    with livo_amd.Context(0, t_LI=ZERO3, max_iterations=4) as c:
        yield c


@pytest.fixture(scope="module")
def unfused(ctx, sheets):
    """4.1 on every sheet: (device search pass, oracle search pass, device / oracle cached pass at a moved state)."""
    import oracle
    out = []
    for sh in sheets:
        st = sh["state"]
        tree = oracle.Tree(sh["map"])
        ctx.map_build(sh["map"])
        sid = ctx.scan_upload(sh["body"])
        try:
            g = ctx.h_share(sid, st, search_en=True)
            st2 = dict(st)
            st2["pos"] = st["pos"] + np.array([0.004, -0.003, 0.002])
            g2 = ctx.h_share(sid, st2, search_en=False)
        finally:
            ctx.scan_release(sid)
        r = tree.h_share(sh["body"], st["rot"], st["pos"], np.eye(3), ZERO3, True)
        r2 = tree.h_share(sh["body"], st2["rot"], st2["pos"], np.eye(3), ZERO3, False,
                          cache={k: v.copy() for k, v in r["cache"].items()})
        out.append((g, r, g2, r2))
    return out


def test_unfused_pass(sheets, unfused):
    """4.1: k_hshare after a search, and from the cached planes at a moved state."""
    kept = 0
    for sh, (g, r, g2, r2) in zip(sheets, unfused):
        assert np.array_equal(r["cache"]["d"], sh["nn_d"])  # (the case's own neighbours)
        _hs_equal(g, r, ("search", sh["index"]))
        _hs_equal(g2, r2, ("cached", sh["index"]))
        kept += g["effct"]
    assert kept > 1500, kept


def test_unfused_planes_are_esti_plane(sheets, unfused):
    """Every plane the kernel reports is orc_esti_plane's of the map points at its nn_idx: the
    kernel against the traced function, not only against h_share."""
    import oracle
    seen = nan = 0
    for sh, (g, _, _, _) in zip(sheets, unfused):
        for i, idx in enumerate(g["nn_idx"]):
            ok, pa = oracle.esti_plane(sh["map"][idx])
            if np.isnan(pa).any():
                nan += 1
                assert not g["sel"][i] and not g["normvec"][i].any()
            if g["normvec"][i].any():  # accepted: normvec = (n, pd2)
                assert ok, (sh["index"], i)
                assert np.array_equal(_bits(g["normvec"][i, :3]), _bits(pa[:3])), (sh["index"], i)
                seen += 1
    assert seen > 1500 and nan >= 20, (seen, nan)


def _mixed(sh):
    """The sheet's clusters beside the room crop, its queries after 2,000 room points (body frame of the sheet's state)."""
    import plane_ref as pr
    room, world = pr.room_crop()
    st = sh["state"]
    body_room = ((world.astype(np.float64) - st["pos"]) @ st["rot"]).astype(np.float32)
    return np.concatenate([room, sh["map"]]), np.concatenate([body_room, sh["body"]]), len(room), len(world)


@pytest.fixture(scope="module")
def mixed_refs(built, sheets):
    """The oracle's side of 4.2 for every sheet: one evaluation, its neighbours, and the pass without
    a search that follows it (which also fits the points the search's sqdist gate left out)."""
    import oracle
    out = []
    for sh in sheets:
        m, body, _, _ = _mixed(sh)
        st = sh["state"]
        tree = oracle.Tree(m)
        _, stats = tree.iekf_update(body, st, R_LI=np.eye(3), t_LI=ZERO3, max_iter=0)
        r = tree.h_share(body, st["rot"], st["pos"], np.eye(3), ZERO3, True)
        r2 = tree.h_share(body, st["rot"], st["pos"], np.eye(3), ZERO3, False,
                          cache={k: v.copy() for k, v in r["cache"].items()})
        out.append({"tree": tree, "stats": stats, "search": r, "cached": r2})
    return out


@pytest.mark.parametrize("gen", [None, "1"], ids=["k_iekf_eval", "k_iekf_eval_gen"])
def test_fused_pass(sheets, mixed_refs, monkeypatch, gen):
    """4.2 and the sweeps of 4.5: the fit inside the fused evaluation.  effct_feat_num shows every
    case's decision (the room's 2,000 points keep the normal equations well posed); the planes the
    kernel cached (the scan's plane / pstate buffers, which livo_h_share without a search reads:
    fill_job) give the per-point view."""
    import livo_amd
    import plane_ref as pr
    if gen is None:
        monkeypatch.delenv("LIVO_EVAL_GEN", raising=False)
    else:
        monkeypatch.setenv("LIVO_EVAL_GEN", gen)
    flips = {}
    with livo_amd.Context(0, t_LI=ZERO3, max_iterations=0) as c:
        for sh, ref in zip(sheets, mixed_refs):
            m, body, n_room, n_scan = _mixed(sh)
            st = sh["state"]
            c.map_build(m)
            sid = c.scan_upload(body)
            try:
                _, stats = c.iekf_update(sid, st)
                idx, d = c.scan_neighbors(sid)
                g2 = c.h_share(sid, st, search_en=False)
            finally:
                c.scan_release(sid)
            tag = sh["index"]
            assert stats["iterations"] == ref["stats"]["iterations"] == 1, tag
            assert stats["effct_feat_num"] == ref["stats"]["effct_feat_num"], tag
            assert _rel(stats["solution"][0], ref["stats"]["solution"][0]) < REL_STATE, tag
            assert np.array_equal(idx, ref["search"]["cache"]["idx"]), tag
            assert np.array_equal(_bits(d), _bits(ref["search"]["cache"]["d"])), tag
            assert np.array_equal(np.sort(idx[n_scan:] - n_room, axis=1), np.sort(sh["nn_idx"], axis=1)), tag
            assert np.array_equal(_bits(g2["normvec"]), _bits(ref["cached"]["normvec"])), tag
            assert np.array_equal(g2["sel"], ref["cached"]["sel"]), tag
            # where the sqdist gate passed, the evaluation's own decision is the cached pass's
            gate = ~(ref["search"]["cache"]["d"][:, 4] > 5.0)
            assert np.array_equal(ref["search"]["sel"][gate], g2["sel"][gate]), tag
            flips[sh["index"]] = (g2["sel"][n_scan:], ref["search"]["sel"][n_scan:], stats["effct_feat_num"][0])
    for name, steps in pr.sweeps().items():
        if name == "edge_sqdis":  # decided by the search pass: in the counts (above), not in the cached planes
            sel = np.array([flips[s][1][i] for s, i in steps])
        else:
            sel = np.array([flips[s][0][i] for s, i in steps])
        assert sel[0] == 1 and sel[-1] == 0 and np.count_nonzero(np.diff(sel.astype(int))) == 1, (name, sel)


def test_sweeps_unfused(sheets, unfused):
    """4.5: sel at every step of the four sweeps (equal to the oracle's in test_unfused_pass); the
    flip is inside each sweep, once.  The body point at the origin is rejected (x / 0)."""
    import plane_ref as pr
    for name, steps in pr.sweeps().items():
        sel = np.array([unfused[s][0]["sel"][i] for s, i in steps], int)
        ref = np.array([unfused[s][1]["sel"][i] for s, i in steps], int)
        assert np.array_equal(sel, ref), name
        assert sel[0] == 1 and sel[-1] == 0 and np.count_nonzero(np.diff(sel)) == 1, (name, sel)
    g, r = unfused[pr.N_SHEETS + 1][:2]
    assert not np.any(sheets[pr.N_SHEETS + 1]["body"][0])
    assert np.array_equal(g["sel"], r["sel"]) and g["sel"][0] == 0
    assert g["nn_idx"][0, 0] >= 0 and not (g["nn_d"][0, 4] > 5.0)  # (it did land inside its cluster)


def test_ikfom_pass(sheets, mixed_refs):
    """4.3: the IKFoM row kernel's fit, one evaluation on the mixed scans."""
    import livo_amd
    import plane_ref as pr
    from livo_amd import synth
    with livo_amd.Context(0, t_LI=ZERO3, max_iterations=0) as c:
        for k in SOLVE_SHEETS + (pr.N_SHEETS, pr.N_SHEETS + 1):
            sh = sheets[k]
            m, body, _, _ = _mixed(sh)
            st = synth.make_ikfom_state(0)
            st["pos"] = np.asarray(sh["state"]["pos"], np.float64)
            st["rot"] = synth.rot_to_quat(np.asarray(sh["state"]["rot"], np.float64))
            st["offset_T"] = np.zeros(3)
            c.map_build(m)
            sid = c.scan_upload(body)
            try:
                _, gs = c.ikfom_update(sid, st)
            finally:
                c.scan_release(sid)
            _, rs = mixed_refs[k]["tree"].ikfom_update(body, st, max_iter=0)
            assert gs["iterations"] == rs["iterations"] == 1, k
            assert gs["effct_feat_num"] == rs["effct_feat_num"], k
            err = np.linalg.norm(gs["dx"][0] - rs["dx"][0])
            assert err <= REL_STATE * max(np.linalg.norm(rs["dx"][0]), 1e-300), (k, err)


def test_ivox_backend(sheets):
    """4.4: the same pass behind the iVox search, whose row order is nth_element's."""
    import livo_amd
    import oracle
    kept = 0
    with livo_amd.Context(0, t_LI=ZERO3, max_iterations=4) as c:
        c.set_backend(livo_amd.BACKEND_IVOX)
        for sh in sheets:
            st = sh["state"]
            c.ivox_init(resolution=0.5)
            iv = oracle.Ivox(resolution=0.5)
            c.ivox_add_points(sh["map"])
            iv.add_points(sh["map"])
            sid = c.scan_upload(sh["body"])
            try:
                g = c.h_share(sid, st, search_en=True)
                st2 = dict(st)
                st2["pos"] = st["pos"] + np.array([0.004, -0.003, 0.002])
                g2 = c.h_share(sid, st2, search_en=False)
            finally:
                c.scan_release(sid)
            r = iv.h_share(sh["body"], st["rot"], st["pos"], np.eye(3), ZERO3, True, oracle.new_cache(len(sh["body"])))
            # a query with no candidate at all (the sweep queries 2 m off their cluster): GetClosestPoint
            # leaves the point's neighbour entry untouched, which is the caller's initial content on
            # either side (a zeroed record here, new_cache's -1 there); every other field is compared
            found = r["cache"]["cnt"] > 0
            assert found.sum() >= 0.9 * len(found) or sh["index"] == len(sheets) - 2, sh["index"]
            _hs_equal(g, r, ("ivox search", sh["index"]), found)
            r2 = iv.h_share(sh["body"], st2["rot"], st2["pos"], np.eye(3), ZERO3, False, r["cache"])
            _hs_equal(g2, r2, ("ivox cached", sh["index"]), found)
            kept += g["effct"]
    assert kept > 1000, kept


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ragged_sizes(ctx, sheets, n):
    """4.6: edge cases in a partial wave and in both shard rows; the scan's last point is a rank-0 case."""
    import oracle
    sh = sheets[0]  # (the sheet of the cluster at the origin)
    zero = np.flatnonzero(sh["family"] == "coincident_origin")
    rest = np.flatnonzero(sh["family"] != "coincident_origin")
    pick = np.concatenate([np.resize(rest, n - 1), zero[:1]])
    body = np.ascontiguousarray(sh["body"][pick])
    assert len(body) == n and not np.any(sh["map"][sh["nn_idx"][pick[-1]]])
    st = sh["state"]
    ctx.map_build(sh["map"])
    sid = ctx.scan_upload(body)
    try:
        g = ctx.h_share(sid, st, search_en=True)
    finally:
        ctx.scan_release(sid)
    r = oracle.Tree(sh["map"]).h_share(body, st["rot"], st["pos"], np.eye(3), ZERO3, True)
    _hs_equal(g, r, n)
    assert g["sel"][-1] == 0
