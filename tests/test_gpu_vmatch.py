"""GPU parity of the resident visual map (livo_vmap_*) and livo_vio_match
(LidarSelector::addFromSparseMap, src/lidar_selection.cpp:332-593) against the restatement of
tests/test_vmatch_abi.py (MapModel) applied to livo_frame_to_world's float x, y, z.

Bars: everything exact.  The records (every field, as bytes), the statistics, pos, the search levels,
all three patch levels and the map's dump equal the restatement.  Unless a test says otherwise: a
160 x 128 image, patch_size 4 (border 24), grid_size 16 or 20, clouds of a few thousand points on a
textured wall with a board 2 m in front of its left half (Scene), maps of tens to hundreds of points.
Every case must show, in the restatement alone, what it is for (the floors asserted beside it).
"""
import ctypes as C

import numpy as np
import pytest
from test_rgb_cloud_abi import restate_pose
from test_vmatch_abi import MATCH_DTYPE, MapModel, Scene, fabricate, moved, small_cam

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


class Rig:
    """One context's visual map and its MapModel, driven alike."""

    def __init__(self, ctx, cam, ps=4, max_points=1200, max_frames=6):
        import livo_amd
        from livo_amd import synth
        self.ctx, self.cam, self.ps, self.synth = ctx, cam, ps, synth
        self.vp = livo_amd.vio_params(cam, synth.R_CI, synth.P_CI)
        self.vp.patch_size = ps
        ctx.vmap_reset(max_points, max_frames, ps)
        self.model = MapModel(cam, ps)

    def pose(self, st):
        return restate_pose(self.synth.R_CI, self.synth.P_CI, st["rot"], st["pos"])

    def add_frame(self, fid, st, img, upload=True):
        self.ctx.vmap_add_frame(fid, st, self.vp, img if upload else None)
        self.model.add_frame(fid, *self.pose(st), img)

    def add(self, fid, pts, pat, ids=None, levels=None):
        got = self.ctx.vmap_add(fid, pts, pat, ids, levels)
        want = self.model.add(fid, pts, pat, ids, levels)
        assert np.array_equal(got, want)
        return got

    def seen(self, fid, st, img, world, sample=True):
        """Points created from float32 world points as frame fid sees them."""
        pts, pat = fabricate(world, self.cam, *self.pose(st), img, self.ps, sample)
        return self.add(fid, pts, pat), pts, pat

    def check_dump(self):
        got, want = self.ctx.vmap_dump(), self.model.dump()
        for g, w in zip(got, want):
            assert g.shape == w.shape and g.tobytes() == w.tobytes()
        return got

    def match(self, st, img, body, grid, quirk=True, **kw):
        sid = self.ctx.scan_upload(body)
        try:
            world = self.ctx.frame_to_world(st, sid)[:, :3]
            dev = self.ctx.vio_match(st, img, self.vp, grid, scan_id=sid, **kw)
        finally:
            self.ctx.scan_release(sid)
        ref = self.model.match(world, *self.pose(st), img, grid, kw.get("ncc_en", False), kw.get("ncc_thre", 0.0),
                               kw.get("outlier_threshold", 100.0), quirk=quirk)
        return dev, ref

    def match_equal(self, *a, **kw):
        dev, ref = self.match(*a, **kw)
        rec, pos, lev, pat, stats, info = ref
        print(stats, info.get("levels_at_warp"))
        assert dev["stats"] == stats
        assert dev["records"].tobytes() == rec.tobytes()
        assert dev["pos"].tobytes() == pos.tobytes() and np.array_equal(dev["levels"], lev)
        assert dev["patches"].shape == pat.shape and np.array_equal(dev["patches"].view(np.uint32), pat.view(np.uint32))
        self.check_dump()
        return dev, ref


@pytest.fixture(scope="module")
def mctx(built):
    import livo_amd
    from livo_amd import synth
    ctx = livo_amd.Context(0, t_LI=synth.T_LI)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def world0():
    """Frame A, its scene and images, and wall points (float32, world) through a lattice of A's pixels."""
    from livo_amd import synth
    cam = small_cam()
    A = synth.make_state(1)
    sc = Scene(A, cam)
    return {"cam": cam, "A": A, "sc": sc, "imgA": sc.render(A)}


def lattice(sc, st, us, vs):
    uu, vv = np.meshgrid(np.asarray(us, F64), np.asarray(vs, F64))
    return sc._pixels(st, uu.ravel(), vv.ravel())[0].astype(F32)


def side(sc, st, dx, dz=0.0, rot=(0.0, 0.0, 0.0)):
    """`st` moved dx along its camera's x axis and dz along its optical axis."""
    return moved(st, sc.Rwc[:, 0] * dx + sc.Rwc[:, 2] * dz, rot)


def test_closed_loop_select_store_match_update(mctx, world0):
    """livo_vio_select on frame A, stored with the retained image; livo_vio_match on frame B a few cm and
    tenths of a degree away; its output drives livo_vio_update.  The board's edge rejects on depth."""
    cam, A, sc, imgA = (world0[k] for k in ("cam", "A", "sc", "imgA"))
    B = moved(A, [0.03, -0.02, 0.015], [0.2, -0.15, 0.1])
    imgB = sc.render(B)
    rig = Rig(mctx, cam)
    sid = mctx.scan_upload(sc.cloud(A, 4000, 1))
    pts, pat, _ = mctx.vio_select(A, imgA, rig.vp, 16, sid)
    mctx.scan_release(sid)
    assert len(pts) >= 30
    rig.add_frame(0, A, imgA, upload=False)  # gray == NULL: vio_select's retained image
    rig.add(0, pts, pat)
    rig.check_dump()
    dev, ref = rig.match_equal(B, imgB, sc.cloud(B, 4000, 2), 16)
    stats = ref[4]
    assert stats["n_out"] >= 20 and stats["warp_shared"] >= 1
    start = moved(B, [0.01, 0.01, -0.01], [0.1, 0.1, -0.1])
    restated = dict(dev, pos=ref[1], levels=ref[2], patches=ref[3])
    g, r = mctx.vio_update(dev, start), mctx.vio_update(restated, start)
    assert g[1] == r[1] and g[2].tobytes() == r[2].tobytes()
    assert all(np.array_equal(g[0][k], r[0][k]) for k in ("pos", "rot", "cov")) and g[1]["n_meas"] > 0


def test_depth_discontinuity_at_the_board_edge(mctx, world0):
    """Wall points one or two pixels right of the board's edge (the board is 2 m nearer) are rejected where
    the cloud left a board depth in their window; wall points away from it are kept."""
    cam, A, sc, imgA = (world0[k] for k in ("cam", "A", "sc", "imgA"))
    rig = Rig(mctx, cam)
    rig.add_frame(0, A, imgA)
    rig.seen(0, A, imgA, lattice(sc, A, [70.5, 100.5, 116.5], [32.5, 48.5, 64.5, 80.5, 96.5]))
    dev, ref = rig.match_equal(A, imgA, sc.cloud(A, 12000, 14), 16)
    assert ref[4]["depth_rejected"] >= 3 and ref[4]["n_out"] >= 3


def test_depth_last_cloud_index_wins(mctx, world0):
    """Two cloud points on one pixel beside a map point, their depths straddling the 1.5 m test, in both cloud
    orders: the later one decides."""
    cam, A, sc, imgA = (world0[k] for k in ("cam", "A", "sc", "imgA"))
    Rcw, Pcw = restate_pose(sc.synth.R_CI, sc.synth.P_CI, A["rot"], A["pos"])
    o = -Rcw.T @ Pcw
    pt = lattice(sc, A, [100.5], [60.5])
    far = lattice(sc, A, [101.5], [60.5])[0].astype(F64)
    near = o + (far - o) * (3.9 / 6.0)
    outs = []
    for order in ((near, far), (far, near)):
        rig = Rig(mctx, cam)
        rig.add_frame(0, A, imgA)
        rig.seen(0, A, imgA, pt)
        dev, ref = rig.match_equal(A, imgA, sc.body(A, np.vstack([pt.astype(F64), *order])), 20)
        outs.append((ref[4]["n_out"], ref[4]["depth_rejected"]))
    assert outs == [(1, 0), (0, 1)]


def test_view_choice(mctx, world0):
    """Points with three observations from three frames (the two last at one pose: equal cosines, the first
    of them wins), and points seen only from beyond 60 degrees."""
    cam, A, sc, imgA = (world0[k] for k in ("cam", "A", "sc", "imgA"))
    frames = [side(sc, A, 0.8), side(sc, A, 0.3), side(sc, A, 0.3), side(sc, A, 13.0)]
    imgs = [sc.render(f) for f in frames]
    rig = Rig(mctx, cam)
    for k in range(4):
        rig.add_frame(10 + k, frames[k], imgs[k])
    near = lattice(sc, A, [88.5, 104.5, 120.5], [40.5, 72.5])   # on the wall, right of the board
    ids, _, _ = rig.seen(10, frames[0], imgs[0], near)
    for k in (1, 2):
        pts, pat = fabricate(near, cam, *rig.pose(frames[k]), imgs[k], 4)
        rig.add(10 + k, pts, pat, ids, np.zeros(len(ids), np.int32))
    lone = lattice(sc, A, [88.5, 104.5, 120.5, 72.5], [56.5, 88.5])[:5]
    rig.seen(13, frames[3], imgs[3], lone, sample=False)
    dev, ref = rig.match_equal(A, imgA, sc.cloud(A, 3000, 3), 16)
    assert ref[4]["view_rejected"] >= 3 and ref[4]["n_out"] >= 3
    assert set(dev["records"]["obs_index"]) == {1} and set(dev["records"]["frame_id"]) == {11}


def test_warp_cache_is_keyed_by_the_reference_frame(mctx, world0):
    """Two cells whose observations share a frame: the later cell carries the earlier cell's matrix."""
    cam, A, sc, imgA = (world0[k] for k in ("cam", "A", "sc", "imgA"))
    F = side(sc, A, 0.6, -1.0, (0.0, 2.0, 1.0))
    imgF = sc.render(F)
    pts = lattice(sc, A, [88.5, 120.5], [40.5])
    out = []
    for quirk in (True, False):
        rig = Rig(mctx, cam)
        rig.add_frame(4, F, imgF)
        rig.seen(4, F, imgF, pts)
        sid_body = sc.cloud(A, 2000, 4)
        if quirk:
            dev, ref = rig.match_equal(A, imgA, sid_body, 16, outlier_threshold=1e9)
        else:
            dev, ref = rig.match(A, imgA, sid_body, 16, quirk=False, outlier_threshold=1e9)
        out.append((dev, ref))
    (dev, ref), (_, plain) = out
    assert ref[4]["warp_shared"] == 1 and plain[4]["warp_shared"] == 0 and ref[4]["n_out"] == 2
    assert not np.array_equal(ref[3], plain[3])  # the input exercises the quirk ...
    assert np.array_equal(dev["patches"][0], plain[3][0]) and not np.array_equal(dev["patches"][1], plain[3][1])


def test_search_levels_one_and_two(mctx, world0):
    """Reference frames 6 m and 18 m further from the wall: determinants about 4 and 16."""
    cam, A, sc, imgA = (world0[k] for k in ("cam", "A", "sc", "imgA"))
    F1, F2 = side(sc, A, 0.0, -6.0), side(sc, A, 0.0, -18.0)
    rig = Rig(mctx, cam)
    for fid, f in ((1, F1), (2, F2)):
        img = sc.render(f)
        rig.add_frame(fid, f, img)
        rig.seen(fid, f, img, lattice(sc, A, [88.5, 104.5, 120.5], [40.5 if fid == 1 else 72.5]))
    dev, ref = rig.match_equal(A, imgA, sc.cloud(A, 2000, 5), 16, outlier_threshold=1e9)
    assert sorted(set(ref[5]["own_levels"])) == [1, 2] and sorted(set(dev["records"]["search_level"])) == [1, 2]
    _, obs, pat = mctx.vmap_dump()
    for r, p in zip(dev["records"], dev["patches"]):  # the stored level-0 patch is the emitted one
        assert np.array_equal(pat[r["point_id"]][:16], p[:16])


def test_zero_branch_at_the_image_edge(mctx, world0):
    cam, A, sc, imgA = (world0[k] for k in ("cam", "A", "sc", "imgA"))
    rig = Rig(mctx, cam)
    rig.add_frame(0, A, imgA)
    pts, pat = fabricate(lattice(sc, A, [104.5, 120.5], [56.5]), cam, *rig.pose(A), imgA, 4, sample=False)
    pts["u"], pts["v"] = [1.5, 158.2], [60.0, 126.4]
    rig.add(0, pts, pat)
    dev, ref = rig.match_equal(A, imgA, sc.cloud(A, 2000, 6), 16, outlier_threshold=1e9)
    assert ref[4]["n_out"] == 2 and ref[5]["zero_samples"] >= 8
    assert np.sum(dev["patches"][:, :16] == 0) >= 8 and np.sum(dev["patches"][:, :16] > 0) >= 4


@pytest.mark.parametrize("w,h,grid", [(160, 128, 20), (160, 152, 40)])
def test_cell_rule(mctx, w, h, grid):
    """Two points at one position: the greater id; a point beyond 10,000 m marks its cell and yields nothing;
    index >= length is dropped and counted (160 x 152 with grid 40; at 160 x 128 with grid 20 the frame test
    ends before the aliasing rows, and the count is 0 on both sides)."""
    from livo_amd import synth
    cam = small_cam(w, h)
    A = synth.make_state(1)
    sc = Scene(A, cam, board=False)
    imgA = sc.render(A)
    rig = Rig(mctx, cam)
    rig.add_frame(0, A, imgA)
    wall = lattice(sc, A, np.arange(48.5, w - 24, 11.0), np.arange(48.5, h - 24, 9.0))
    rig.seen(0, A, imgA, np.vstack([wall, wall]))  # every point twice: the second copy has the greater id
    Rcw, Pcw = rig.pose(A)
    o = -Rcw.T @ Pcw
    ray = lattice(sc, A, [30.5], [30.5])[0].astype(F64) - o  # a cell of its own
    distant = (o + ray / np.linalg.norm(ray) * 10500.0).astype(F32)[None]
    rig.seen(0, A, imgA, distant, sample=False)
    body = np.vstack([sc.cloud(A, 3000, 7), sc.body(A, distant.astype(F64))])
    dev, ref = rig.match_equal(A, imgA, body, grid)
    stats = ref[4]
    ids = dev["records"]["point_id"]
    assert len(ids) >= 3 and np.all(ids >= len(wall)) and 2 * len(wall) not in ids
    assert stats["map_tested"] > len(wall)  # (a point is tested where the cloud reached its stored voxel)
    assert stats["cells_marked"] == stats["n_out"] + stats["depth_rejected"] + stats["view_rejected"] + \
        stats["error_rejected"] + 1
    assert (stats["cell_overflow"] >= 1) == (h == 152)


def test_thresholds_split_the_candidates(mctx, world0):
    cam, A, sc, imgA = (world0[k] for k in ("cam", "A", "sc", "imgA"))
    B = moved(A, [0.05, 0.03, -0.02], [0.3, 0.2, -0.2])
    imgB = sc.render(B)
    F = side(sc, A, 0.25)
    imgF = sc.render(F)
    wall = lattice(sc, A, np.arange(86.5, 130, 8.0), np.arange(30.5, 100, 8.0))

    def rig_():
        rig = Rig(mctx, cam)
        rig.add_frame(0, F, imgF)
        rig.seen(0, F, imgF, wall)
        return rig

    body = sc.cloud(B, 3000, 8)
    dev, ref = rig_().match_equal(B, imgB, body, 16, ncc_en=True, ncc_thre=-2.0, outlier_threshold=1e9)
    assert len(ref[0]) >= 8
    ncc_mid, err_mid = float(np.median(ref[0]["ncc"])), float(np.median(ref[0]["error"])) / 16.0
    dev, ref = rig_().match_equal(B, imgB, body, 16, ncc_en=True, ncc_thre=ncc_mid, outlier_threshold=1e9)
    assert ref[4]["ncc_rejected"] >= 3 and ref[4]["n_out"] >= 3 and np.all(dev["records"]["ncc"] >= ncc_mid)
    dev, ref = rig_().match_equal(B, imgB, body, 16, outlier_threshold=err_mid)
    assert ref[4]["error_rejected"] >= 3 and ref[4]["n_out"] >= 3 and np.all(dev["records"]["ncc"] == 0)


def test_sizes_that_change_the_path(mctx):
    """1,000 map points and 5,000 cloud points over 300 voxels and more (neither a multiple of the block, the
    hash set holds collisions); then patch_size 8 (64 lanes) on a 256 x 192 image."""
    from livo_amd import synth
    rng = np.random.default_rng(12)
    for (w, h, ps, grid, n_map, n_cloud) in ((160, 128, 4, 16, 1000, 5000), (256, 192, 8, 32, 150, 2000)):
        cam = small_cam(w, h)
        A = synth.make_state(1)
        sc = Scene(A, cam)
        imgA = sc.render(A)
        B = moved(A, [0.02, 0.02, 0.01], [0.1, -0.1, 0.1])
        rig = Rig(mctx, cam, ps)
        rig.add_frame(0, A, imgA)
        b = (ps // 2 + 1) * 8
        wall = sc._pixels(A, rng.uniform(b + 1, w - b - 1, n_map), rng.uniform(b + 1, h - b - 1, n_map))[0]
        rig.seen(0, A, imgA, wall.astype(F32))
        dev, ref = rig.match_equal(B, sc.render(B), sc.cloud(B, n_cloud, 13, margin=0.6), grid)
        assert ref[4]["n_out"] >= 5 and ref[4]["map_tested"] >= n_map // 2
        if n_cloud == 5000:
            assert ref[4]["n_voxels"] >= 300


def test_determinism_sizing_and_isolation(built, world0):
    """Two calls give the same bytes; the sizing call leaves the map's dump unchanged; interleaved with the
    other frame stages on one context, every stage's output equals a fresh context's."""
    import livo_amd
    from livo_amd import synth
    cam, A, sc, imgA = (world0[k] for k in ("cam", "A", "sc", "imgA"))
    B = moved(A, [0.03, -0.02, 0.015], [0.2, -0.15, 0.1])
    imgB = sc.render(B)
    bgr = np.stack([imgB, imgA, imgB], axis=2)
    raw = synth.make_raw_scan(3000, 0)
    wall = lattice(sc, A, np.arange(86.5, 130, 8.0), np.arange(30.5, 100, 8.0))
    body = sc.cloud(B, 3000, 9)

    def stages(ctx, mixed):
        rig = Rig(ctx, cam)
        rig.add_frame(0, A, imgA)
        rig.seen(0, A, imgA, wall)
        before = [a.tobytes() for a in ctx.vmap_dump()]
        sid = ctx.scan_upload(body)
        n, vs, st = C.c_int64(), livo_amd.VmatchStats(), livo_amd.state_to_c(B)
        assert ctx._L.livo_vio_match(ctx.h, sid, C.byref(st), C.byref(rig.vp), 16, 0, 0.0, 100.0, livo_amd._ptr(imgB),
                                     160, 128, None, None, None, None, 0, C.byref(n), C.byref(vs)) == 0
        assert [a.tobytes() for a in ctx.vmap_dump()] == before and n.value == vs.n_out > 0
        out = {}
        if mixed:
            out["sel"] = ctx.vio_select(A, imgA, rig.vp, 16, sid)
        out["m1"] = ctx.vio_match(B, imgB, rig.vp, 16, scan_id=sid)
        if mixed:
            out["rgb"] = ctx.colorize(B, bgr, rig.vp, sid)
            out["upd"] = ctx.vio_update(out["m1"], A)
            pre = ctx.scan_preprocess(*raw, leaf_size=0.5)
            out["pre"] = (pre[1], pre[2])
        out["m2"] = ctx.vio_match(B, None, rig.vp, 16, scan_id=sid)
        assert [a.tobytes() for a in ctx.vmap_dump()] != before  # the warped patches are in the map
        return out

    def flat(x):
        if isinstance(x, dict):
            return [flat(x[k]) for k in sorted(x)]
        if isinstance(x, (tuple, list)):
            return [flat(v) for v in x]
        return x.tobytes() if isinstance(x, np.ndarray) else x

    with livo_amd.Context(0, t_LI=synth.T_LI) as c1:
        mixed = stages(c1, True)
    with livo_amd.Context(0, t_LI=synth.T_LI) as c2:
        plain = stages(c2, False)
    m = {k: v for k, v in mixed["m1"].items() if k != "image"}
    assert flat(m) == flat({k: v for k, v in mixed["m2"].items() if k != "image"})
    assert flat(m) == flat({k: v for k, v in plain["m1"].items() if k != "image"}) and len(m["records"]) > 0
    with livo_amd.Context(0, t_LI=synth.T_LI) as c3:
        rig = Rig(c3, cam)
        sid = c3.scan_upload(body)
        assert flat(c3.vio_select(A, imgA, rig.vp, 16, sid)) == flat(mixed["sel"])
        assert flat(c3.colorize(B, bgr, rig.vp, sid)) == flat(mixed["rgb"])
        assert flat(c3.vio_update(mixed["m1"], A)) == flat(mixed["upd"])
        pre = c3.scan_preprocess(*raw, leaf_size=0.5)
        assert flat((pre[1], pre[2])) == flat(mixed["pre"])


def test_errors(built, world0):
    import livo_amd
    from livo_amd import synth
    cam, A, sc, imgA = (world0[k] for k in ("cam", "A", "sc", "imgA"))
    with livo_amd.Context(0, t_LI=synth.T_LI) as ctx:
        L, st, n = ctx._L, livo_amd.state_to_c(A), C.c_int64(-7)
        vp = livo_amd.vio_params(cam, synth.R_CI, synth.P_CI)
        sid = ctx.scan_upload(sc.cloud(A, 500, 10))

        def match(p=vp, img=imgA, w=160, h=128, out=None, cap=0, bufs=(None, None, None)):
            return L.livo_vio_match(ctx.h, sid, C.byref(st), C.byref(p), 16, 0, 0.0, 1e9, livo_amd._ptr(img), w, h,
                                    livo_amd._ptr(out), *(livo_amd._ptr(b) for b in bufs), cap, C.byref(n), None)

        assert match() == -1  # no map yet
        rig = Rig(ctx, cam, max_points=30, max_frames=2)
        assert match() == 0 and n.value == 0  # an empty map
        assert L.livo_vmap_add_frame(ctx.h, 0, C.byref(st), C.byref(vp), None, 160, 128) == -1  # no retained image
        rig.add_frame(0, A, imgA)
        assert L.livo_vmap_add_frame(ctx.h, 0, C.byref(st), C.byref(vp), livo_amd._ptr(imgA), 160, 128) == -1  # duplicate
        dist = livo_amd.vio_params(dict(cam, d=[-0.1, 0.0, 0.0, 0.0, 0.0]), synth.R_CI, synth.P_CI)
        assert L.livo_vmap_add_frame(ctx.h, 1, C.byref(st), C.byref(dist), livo_amd._ptr(imgA), 160, 128) == -1
        assert match(p=dist) == -1 and match(h=127) == -1
        wide = livo_amd.vio_params(small_cam(256, 192), synth.R_CI, synth.P_CI)
        assert match(p=wide, img=np.zeros((192, 256), np.uint8), w=256, h=192) == -1  # not the map's size
        rig.add_frame(1, A, imgA)
        assert L.livo_vmap_add_frame(ctx.h, 2, C.byref(st), C.byref(vp), livo_amd._ptr(imgA), 160, 128) == -7  # full
        wall = lattice(sc, A, [88.5, 104.5, 120.5], [40.5, 72.5])
        ids, pts, pat = rig.seen(0, A, imgA, wall)
        P = livo_amd._ptr
        assert L.livo_vmap_add(ctx.h, 5, 6, None, P(pts), None, P(pat), None) == -1  # unknown frame
        bad = np.array([0, 1, 2, 3, 4, 99], np.int32)
        assert L.livo_vmap_add(ctx.h, 0, 6, P(bad), P(pts), None, P(pat), None) == -1  # unknown id
        for _ in range(19):
            rig.add(1, pts, pat, ids, np.zeros(6, np.int32))
        assert L.livo_vmap_add(ctx.h, 1, 6, P(ids), P(pts), None, P(pat), None) == -7  # a 21st observation
        many = np.repeat(pts, 5)
        assert L.livo_vmap_add(ctx.h, 0, 30, None, P(many), None, P(np.repeat(pat, 5, axis=0)), None) == -7  # 6 + 30 > 30
        rig.check_dump()  # nothing was written by the failed calls
        assert ctx.vmap_info()["n_points"] == 6 and ctx.vmap_info()["n_obs"] == 120
        assert match() == 0 and n.value >= 2
        k = n.value
        out = np.full(80 * 48, 0xA5, np.uint8).view(MATCH_DTYPE)
        bufs = (np.full((80, 3), -5.0), np.full(80, -5, np.int32), np.full((80, 48), -5.0, F32))
        assert match(out=out, cap=k - 1, bufs=bufs) == -7 and n.value == k
        assert np.all(out.view(np.uint8) == 0xA5) and all(np.all(b == -5) for b in bufs)
        assert match(out=out, cap=k, bufs=(bufs[0], None, bufs[2])) == -1 and match(cap=3) == -1
        assert match(out=out, cap=k, bufs=bufs) == 0 and np.all(out[k:].view(np.uint8) == 0xA5)
        ctx.scan_release(sid)
