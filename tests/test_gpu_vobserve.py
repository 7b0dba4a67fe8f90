"""GPU parity of livo_vio_observe (LidarSelector::addObservation, src/lidar_selection.cpp:905-962) against the
restatement of tests/test_vobserve_abi.py (ObserveModel).

Bars: everything exact.  After every call the records (as bytes), the statistics and the map's dump equal the
restatement's, and livo_vmap_info's count equals the model's.  160 x 128 images, maps of tens of points (257
for the launch shapes) on a textured wall 6 m in front of frame A.  Every case asserts, in the restatement
alone, the floor that shows it reached what it is for.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
from test_gpu_vmatch import Rig, lattice, side
from test_vis_select_abi import restate_patch, restate_score
from test_vmatch_abi import MAX_OBS, Scene, cam2world, fabricate, small_cam
from test_vobserve_abi import ADDED, BEHIND, DELETED, OUT_OF_FRAME, PIXEL, POSE, ObserveModel

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUR = 100            # the id of the frame observed from
FAR = MAX_OBS - 1    # cap_rig: the stored frame furthest from it


class ORig(Rig):
    """Rig with the ObserveModel, and livo_vio_observe driven alike on both."""

    def __init__(self, ctx, cam, ps=4, max_points=400, max_frames=24):
        super().__init__(ctx, cam, ps, max_points, max_frames)
        self.model = ObserveModel(cam, ps)

    def observe(self, fid, ids, levels=None):
        got, got_stats = self.ctx.vio_observe(fid, ids, levels)
        rec, stats = self.model.observe(fid, ids, levels)
        print(stats)
        assert got_stats == stats
        assert got.dtype == rec.dtype and got.tobytes() == rec.tobytes()
        self.check_dump()
        assert self.ctx.vmap_info()["n_obs"] == stats["n_obs_total"]
        return rec, stats


@pytest.fixture(scope="module")
def octx(built):
    import livo_amd
    from livo_amd import synth
    ctx = livo_amd.Context(0, t_LI=synth.T_LI)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def world():
    """Frame A, the wall 6 m in front of it, and A's image."""
    from livo_amd import synth
    cam = small_cam()
    A = synth.make_state(1)
    sc = Scene(A, cam, board=False)
    return {"cam": cam, "A": A, "sc": sc, "imgA": sc.render(A)}


def unpack(world):
    return (world[k] for k in ("cam", "A", "sc", "imgA"))


def noise(rng, n, ps):
    """n patch pyramids, no two alike: a mis-shifted one shows."""
    return rng.uniform(0, 255, (n, 3 * ps * ps)).astype(F32)


def frame_order(far_pos):
    """Frames 0 .. 18 in order with frame FAR at index far_pos."""
    rest = list(range(FAR))
    return rest[:far_pos] + [FAR] + rest[far_pos:]


CAP_CASES = [(far_pos, add) for far_pos in (0, 7, FAR) for add in (True, False)]


def cap_rig(ctx, world, ps):
    """Six points at 20 observations from frames 0.02 m .. 0.4 m beside frame CUR (= A), frame FAR the furthest,
    at index 0, 7 or 19 of the point's list; observation 0's px lies 41 pixels (add) or 5 (no add) from the
    point's pixel in CUR.  No distance reaches 0.5 m: the pose flag stays off.  -> rig, {(far_pos, add): id}"""
    cam, A, sc, imgA = unpack(world)
    rig = ORig(ctx, cam, ps, max_points=16, max_frames=22)
    for k in range(MAX_OBS):
        rig.add_frame(k, side(sc, A, 0.02 * (k + 1)), imgA)  # (tiny maps: the stored frames share A's image)
    rig.add_frame(CUR, A, imgA)
    base, _ = fabricate(lattice(sc, A, [60.5, 80.5, 100.5], [50.5, 70.5]), cam, *rig.pose(A), imgA, ps, sample=False)
    rng = np.random.default_rng(30 + ps)
    order = [frame_order(far_pos) for far_pos, _ in CAP_CASES]
    ids = {}
    for k in range(MAX_OBS):
        for fid in sorted({o[k] for o in order}):
            sel = [j for j in range(len(CAP_CASES)) if order[j][k] == fid]
            pts = base[sel].copy()
            if k == 0:
                pts["u"] += [41.0 if CAP_CASES[j][1] else 5.0 for j in sel]
                for j, i in zip(sel, rig.add(fid, pts, noise(rng, len(sel), ps))):
                    ids[CAP_CASES[j]] = int(i)
            else:
                pts["u"] += rng.uniform(-3, 3, len(sel))
                rig.add(fid, pts, noise(rng, len(sel), ps), np.array([ids[CAP_CASES[j]] for j in sel], np.int32),
                        rng.integers(0, 3, len(sel)).astype(np.int32))
    return rig, ids


def cap_sequence(rig, ids):
    """The three adding points in one call, then the three others one by one.  -> the records"""
    out = [rig.observe(CUR, [ids[(f, True)] for f in (0, 7, FAR)], [2, 1, 0])]
    out += [rig.observe(CUR, [ids[(f, False)]], [1]) for f in (0, 7, FAR)]
    return out


def test_flags(octx, world):
    """Oldest observations 0.4 m and 0.6 m from the current frame, and at its pose with px 39.9 and 40.1 pixels
    from pc: nothing, the pose flag, nothing, the pixel flag.  The appended observation field by field."""
    cam, A, sc, imgA = unpack(world)
    rig = ORig(octx, cam)
    F04, F06 = side(sc, A, 0.4), side(sc, A, 0.6)
    for fid, st in ((0, F04), (1, F06), (2, A), (3, A)):
        rig.add_frame(fid, st, imgA)
    us = [60.5, 80.5, 100.5]
    ga, _, _ = rig.seen(0, F04, imgA, lattice(sc, A, us, [40.5]))
    gb, _, _ = rig.seen(1, F06, imgA, lattice(sc, A, us, [56.5]))
    groups = [ga, gb]
    for v, off in ((72.5, 39.9), (86.5, 40.1)):
        pts, pat = fabricate(lattice(sc, A, us, [v]), cam, *rig.pose(A), imgA, 4)
        pts["u"] += off
        groups.append(rig.add(2, pts, pat))
    ids = np.concatenate(groups)[np.random.default_rng(3).permutation(12)]
    levels = (np.arange(12) % 3).astype(np.int32)
    rec, stats = rig.observe(3, ids, levels)
    by_id = {int(r["point_id"]): r for r in rec}
    for g, flags in zip(groups, (0, POSE | ADDED, 0, PIXEL | ADDED)):
        assert all(by_id[int(i)]["flags"] == flags for i in g)
    assert all(abs(by_id[int(i)]["delta_p"] - d) < 1e-6 for g, d in ((ga, 0.4), (gb, 0.6)) for i in g)
    assert all(abs(by_id[int(i)]["pixel_dist"] - d) < 1e-6 for g, d in ((groups[2], 39.9), (groups[3], 40.1)) for i in g)
    assert stats["pose_flagged"] == 3 and stats["pixel_flagged"] == 3 and stats["added"] == 6 and stats["deleted"] == 0
    pts_d, obs_d, pat_d = octx.vmap_dump()
    for i, lv in zip(ids, levels):
        r, p = by_id[int(i)], pts_d[int(i)]
        if not r["flags"] & ADDED:
            assert p["n_obs"] == 1 and r["score"] == 0
            continue
        o, at = obs_d[p["first_obs"] + 1], p["first_obs"] + 1
        u, v = float(r["u"]), float(r["v"])
        assert p["n_obs"] == 2 and o["frame_id"] == 3 and o["level"] == lv and list(o["px"]) == [u, v]
        assert list(o["f"]) == cam2world(cam, u, v)
        assert np.array_equal(pat_d[at], restate_patch(imgA, [u], [v], 4)[0]) and np.ptp(pat_d[at]) > 0
        assert p["value"] == r["score"] == restate_score(imgA, [int(u)], [int(v)])[0] and r["score"] > 0


@pytest.mark.parametrize("ps", [2, 4, 8])
def test_cap_and_eviction(octx, world, ps):
    """12, 48 and 192 floats an observation: the compaction inside a chunk, inside a chunk, across chunks.  The
    furthest at index 0, 7 and 19, with add_flag (20 again, the new observation last) and without (19)."""
    rig, ids = cap_rig(octx, world, ps)
    rig.check_dump()
    held = {c: [(o["frame_id"], o["patch"].copy()) for o in rig.model.points[i]["obs"]] for c, i in ids.items()}
    assert len({p.tobytes() for h in held.values() for _, p in h}) == len(CAP_CASES) * MAX_OBS
    out = cap_sequence(rig, ids)
    rec, stats = out[0]
    assert list(rec["deleted_index"]) == [0, 7, FAR] and all(rec["deleted_frame_id"] == FAR)
    assert all(rec["flags"] == PIXEL | DELETED | ADDED) and all(rec["n_obs"] == MAX_OBS)
    assert (stats["deleted"], stats["added"], stats["deleted_without_add"]) == (3, 3, 0)
    for far_pos, (rec, stats) in zip((0, 7, FAR), out[1:]):
        assert rec["flags"][0] == DELETED and rec["n_obs"][0] == MAX_OBS - 1 and rec["deleted_index"][0] == far_pos
        assert (stats["deleted"], stats["added"], stats["deleted_without_add"]) == (1, 0, 1)
    for (far_pos, add), i in ids.items():
        obs = rig.model.points[i]["obs"]
        kept = [h for k, h in enumerate(held[(far_pos, add)]) if k != far_pos]
        assert len(obs) == len(kept) + add and (not add or obs[-1]["frame_id"] == CUR)
        assert all(o["frame_id"] == f and np.array_equal(o["patch"], p) for o, (f, p) in zip(obs, kept))


def test_skips(octx, world):
    """A point behind the camera, one inside the image but outside the border and one outside the image, each
    at 20 observations: counted, and nothing of them changes."""
    cam, A, sc, imgA = unpack(world)
    rig = ORig(octx, cam, max_points=8, max_frames=22)
    for k in range(MAX_OBS):
        rig.add_frame(k, side(sc, A, 0.05 * (k + 1)), imgA)
    rig.add_frame(CUR, A, imgA)
    Rcw, Pcw = rig.pose(A)
    o = -Rcw.T @ Pcw
    wall = sc._pixels(A, np.array([80.5, 10.5, -30.5]), np.array([60.5, 60.5, 60.5]))[0]
    pts3 = np.vstack([2 * o - wall[0], wall[1:]]).astype(F32)
    pts, _ = fabricate(pts3, cam, Rcw, Pcw, imgA, 4, sample=False)
    rng = np.random.default_rng(5)
    ids = rig.add(0, pts, noise(rng, 3, 4))
    for k in range(1, MAX_OBS):
        rig.add(k, pts, noise(rng, 3, 4), ids, np.zeros(3, np.int32))
    before = [a.tobytes() for a in octx.vmap_dump()]
    rec, stats = rig.observe(CUR, ids)
    assert list(rec["flags"]) == [BEHIND, OUT_OF_FRAME, OUT_OF_FRAME] and all(rec["n_obs"] == MAX_OBS)
    assert all(rec["deleted_index"] == -1) and (stats["behind"], stats["out_of_frame"], stats["deleted"]) == (1, 2, 0)
    assert [a.tobytes() for a in octx.vmap_dump()] == before


def test_errors_write_nothing(built, world):
    import livo_amd
    from livo_amd import synth
    cam, A, sc, imgA = unpack(world)
    with livo_amd.Context(0, t_LI=synth.T_LI) as ctx:
        L, P = ctx._L, livo_amd._ptr
        i32 = lambda *v: np.array(v, np.int32)  # noqa: E731
        rec = np.full(4, 0x5A, np.uint8).repeat(56).view(livo_amd.VOBS_POINT_DTYPE)
        vs = livo_amd.VobsStats()

        def call(fid, ids, levels=None, n=None):
            return L.livo_vio_observe(ctx.h, fid, len(ids) if n is None else n, P(ids), P(levels), P(rec), C.byref(vs))

        assert call(0, i32(0)) == -1  # no map
        rig = ORig(ctx, cam, max_points=8, max_frames=3)
        rig.add_frame(0, A, imgA)
        rig.add_frame(1, side(sc, A, 0.6), imgA)
        rig.seen(0, A, imgA, lattice(sc, A, [60.5, 100.5], [50.5, 70.5]))
        before = [a.tobytes() for a in ctx.vmap_dump()]
        assert call(1, i32(0, 1, 1)) == -1       # an id twice
        assert call(1, i32(0, 4)) == -1          # beyond the map's four points
        assert call(1, i32(-1)) == -1
        assert call(7, i32(0, 1)) == -1          # an unknown frame
        assert call(1, i32(0, 1), i32(0, 9)) == -1 and call(1, i32(0), i32(-1)) == -1
        assert call(1, i32(0), n=-1) == -1
        assert np.all(rec.view(np.uint8) == 0x5A) and [a.tobytes() for a in ctx.vmap_dump()] == before
        assert L.livo_vio_observe(ctx.h, 1, 0, None, None, None, C.byref(vs)) == 0
        assert (vs.n_in, vs.added, vs.n_obs_total) == (0, 0, 4)
        assert [a.tobytes() for a in ctx.vmap_dump()] == before and ctx.vmap_info()["n_obs"] == 4
        rec2, stats = rig.observe(1, i32(3, 0, 2, 1), i32(0, 1, 2, 0))  # ... and the map still works
        assert stats["added"] == 4 and all(rec2["flags"] == POSE | ADDED)


def test_launch_shapes(octx, world):
    """1, one wave short of a block, a block, one wave more, and 257 distinct points; half of them add."""
    cam, A, sc, imgA = unpack(world)
    txt = open(os.path.join(ROOT, "fast-livo-noted_amd", "csrc", "livo_internal.h")).read()
    waves = int(re.search(r"constexpr int kVmBlock = (\d+);", txt).group(1)) // 64
    assert waves >= 2
    rng = np.random.default_rng(7)
    wall = sc._pixels(A, rng.uniform(40, 130, 257), rng.uniform(30, 98, 257))[0].astype(F32)
    F06, F01 = side(sc, A, 0.6), side(sc, A, 0.1)
    for n in (1, waves - 1, waves, waves + 1, 257):
        rig = ORig(octx, cam, max_points=300, max_frames=4)
        rig.add_frame(0, F06, imgA)
        rig.add_frame(1, F01, imgA)
        rig.add_frame(CUR, A, imgA)
        rig.seen(0, F06, imgA, wall[0::2])
        rig.seen(1, F01, imgA, wall[1::2])
        ids = rng.permutation(257)[:n].astype(np.int32)
        rec, stats = rig.observe(CUR, ids, (ids % 3).astype(np.int32))
        added = (rec["flags"] & ADDED) != 0
        assert np.array_equal(added, ids < 129) and stats["added"] == int(added.sum())
        if n == 257:
            assert stats["added"] == 129 and stats["pose_flagged"] == 129 and stats["pixel_flagged"] == 0


def test_host_counts_stay_true(octx, world):
    """After observes that deleted and added, livo_vmap_add sees the device's counts: a point now at 19 takes
    one more, a point at 20 does not; then that point is observed again and evicts again."""
    import livo_amd
    cam, A, sc, imgA = unpack(world)
    rig, ids = cap_rig(octx, world, 4)
    cap_sequence(rig, ids)
    at19, at20 = ids[(7, False)], ids[(7, True)]
    assert len(rig.model.points[at19]["obs"]) == MAX_OBS - 1 and len(rig.model.points[at20]["obs"]) == MAX_OBS
    pts, pat = fabricate(lattice(sc, A, [80.5], [60.5]), cam, *rig.pose(A), imgA, 4)
    P = livo_amd._ptr
    assert octx._L.livo_vmap_add(octx.h, 3, 1, P(np.array([at20], np.int32)), P(pts), None, P(pat), None) == -7
    rig.check_dump()
    rig.add(3, pts, pat, np.array([at19], np.int32), np.zeros(1, np.int32))
    rig.check_dump()
    total = sum(len(p["obs"]) for p in rig.model.points)
    assert octx.vmap_info()["n_obs"] == total == 3 * MAX_OBS + 2 * (MAX_OBS - 1) + MAX_OBS
    rec, stats = rig.observe(CUR, [at19, at20])
    assert list(rec["flags"]) == [DELETED, PIXEL | DELETED | ADDED] and stats["n_obs_total"] == total - 1


def test_determinism(built, world):
    """The same sequence on two contexts: the same records and the same dump, byte for byte."""
    import livo_amd
    from livo_amd import synth
    outs = []
    for _ in range(2):
        with livo_amd.Context(0, t_LI=synth.T_LI) as ctx:
            rig, ids = cap_rig(ctx, world, 4)
            recs = [ctx.vio_observe(CUR, [ids[c] for c in CAP_CASES[:4]], [0, 1, 2, 0])[0].tobytes(),
                    ctx.vio_observe(CUR, [ids[c] for c in CAP_CASES[2:]], None)[0].tobytes()]
            outs.append(recs + [a.tobytes() for a in ctx.vmap_dump()])
    assert outs[0] == outs[1] and len(outs[0][0]) == 4 * 56


def test_closed_loop(octx, world):
    """Frame A selected and stored, some of its points pre-filled to 18 observations from three extra frames;
    then five frames 0.3 m apart, each matched, updated, stored at the updated state and observed with the
    match's ids and levels.  Every stage equals the model frame by frame."""
    cam, A, sc, imgA = unpack(world)
    ps, grid = 4, 16
    rig = ORig(octx, cam, ps, max_points=400, max_frames=12)
    sid = octx.scan_upload(sc.cloud(A, 4000, 1))
    pts, pat, _ = octx.vio_select(A, imgA, rig.vp, grid, sid)
    octx.scan_release(sid)
    rig.add_frame(0, A, imgA, upload=False)
    ids = rig.add(0, pts, pat)
    pick = np.flatnonzero((pts["u"] > 84) & (pts["u"] < 132) & (pts["v"] > 36) & (pts["v"] < 92))[:8]
    assert len(pick) >= 4
    seen = np.stack([pts["x"], pts["y"], pts["z"]], 1)[pick]
    extras = [side(sc, A, -0.2), side(sc, A, -0.1, 0.1), side(sc, A, 0.1, -0.1)]
    imgs = [sc.render(E) for E in extras]
    for k in range(3):
        rig.add_frame(10 + k, extras[k], imgs[k])
    for j in range(MAX_OBS - 3):
        k = j % 3
        p, q = fabricate(seen, cam, *rig.pose(extras[k]), imgs[k], ps)
        rig.add(10 + k, p, q, ids[pick], np.zeros(len(pick), np.int32))
    rig.check_dump()
    recs, chosen = [], set()
    for k in range(1, 6):
        S = side(sc, A, 0.3 * k)
        img = sc.render(S)
        dev, ref = rig.match_equal(S, img, sc.cloud(S, 4000, 10 + k), grid)
        assert ref[4]["n_out"] >= 5
        chosen |= {int(f) for f in ref[0]["frame_id"]}
        restated = dict(dev, pos=ref[1], levels=ref[2], patches=ref[3])
        g, r = octx.vio_update(dev, S), octx.vio_update(restated, S)
        assert g[1] == r[1] and g[2].tobytes() == r[2].tobytes() and g[1]["n_meas"] > 0
        assert all(np.array_equal(g[0][key], r[0][key]) for key in ("pos", "rot", "cov"))
        rig.add_frame(k, g[0], img)
        recs.append(rig.observe(k, ref[0]["point_id"], ref[0]["search_level"])[0])
    flags = np.concatenate(recs)["flags"]
    assert np.any(flags & DELETED) and np.any((flags & POSE) != 0) and np.all(((flags & POSE) == 0) | ((flags & ADDED) != 0))
    assert np.any((flags & (ADDED | BEHIND | OUT_OF_FRAME)) == 0)  # an item in the frame that added nothing
    assert chosen & {1, 2, 3, 4, 5}  # a later match chose an observation that an observe stored
