"""GPU parity of livo_vio_detect (one camera frame in one call) against its definition, the chain of public
calls livo_vio_match, livo_vio_select, livo_vio_update, livo_vmap_add_frame, livo_vio_observe, livo_vmap_add,
and of livo_vmap_release_frames against a count of the references in the dump.

Bars: everything exact, no tolerance.  Two contexts are driven alike, `chain` through the six calls and `one`
through livo_vio_detect; after every frame the state (every block, as bytes), every statistic, first_new_id,
livo_vmap_dump (points, observations, patches, as bytes) and livo_vmap_info are equal.  The six stages are
held to their restatements by their own test files; here the chain is the oracle, and every floor that shows
a case reached what it is for is asserted on the chain alone.  160 x 128 images, patch_size 4, clouds of
4,000 points on a textured wall 6 m in front of frame A.
"""
import ctypes as C

import numpy as np
import pytest
from test_gpu_vmatch import lattice, side
from test_gpu_vobserve import unpack, world  # noqa: F401  (world: a module fixture, shared)
from test_vmatch_abi import MAX_OBS, fabricate, moved
from test_vobserve_abi import ADDED, BEHIND, DELETED, OUT_OF_FRAME

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
PS, GRID = 4, 16


# ------------------------------------------------------------------ rigs ----
def new_ctx():
    import livo_amd
    from livo_amd import synth
    return livo_amd.Context(0, t_LI=synth.T_LI)


def vio_params(cam):
    import livo_amd
    from livo_amd import synth
    vp = livo_amd.vio_params(cam, synth.R_CI, synth.P_CI)
    vp.patch_size = PS
    return vp


def pose(st):
    from livo_amd import synth
    from test_rgb_cloud_abi import restate_pose
    return restate_pose(synth.R_CI, synth.P_CI, st["rot"], st["pos"])


def chain_frame(ctx, vp, fid, st, img, body, grid=GRID, **kw):
    """The definition: the six public calls.  -> state, stats (livo_vio_detect's layout), match dict, observe records"""
    sid = ctx.scan_upload(body)
    try:
        m = ctx.vio_match(st, img, vp, grid, scan_id=sid, **kw)
        pts, pat, sstats = ctx.vio_select(st, img, vp, grid, sid)
    finally:
        ctx.scan_release(sid)
    st1, ustats, _ = ctx.vio_update(dict(m, image=img), st, max_iter=vp.max_iterations, img_point_cov=vp.img_point_cov)
    ctx.vmap_add_frame(fid, st1, vp, img)
    rec, ostats = ctx.vio_observe(fid, m["records"]["point_id"], m["records"]["search_level"])
    first = ctx.vmap_info()["n_points"]
    ctx.vmap_add(fid, pts, pat)
    stats = {"match": m["stats"], "select": sstats, "update": ustats, "observe": ostats, "n_matched": len(rec),
             "n_new": len(pts), "first_new_id": first if len(pts) else -1}
    return st1, stats, m, rec


def one_frame(ctx, vp, fid, st, img, body, grid=GRID, **kw):
    sid = ctx.scan_upload(body)
    try:
        return ctx.vio_detect(fid, st, img, vp, grid, scan_id=sid, **kw)
    finally:
        ctx.scan_release(sid)


def state_bytes(st):
    return [np.ascontiguousarray(st[k], F64).tobytes() for k in ("rot", "pos", "vel", "bias_g", "bias_a", "gravity", "cov")]


def map_bytes(ctx):
    return [a.tobytes() for a in ctx.vmap_dump()], ctx.vmap_info()


def assert_same_map(a, b, but=()):
    da, ia = map_bytes(a)
    db, ib = map_bytes(b)
    assert da == db
    assert {k: v for k, v in ia.items() if k not in but} == {k: v for k, v in ib.items() if k not in but}


class Twin:
    """`chain` and `one` with maps of the same capacities."""

    def __init__(self, cam, max_points=1200, max_frames=32):
        self.chain, self.one, self.vp = new_ctx(), new_ctx(), vio_params(cam)
        self.but = ()  # the fields of livo_vmap_info in which the two are meant to differ
        for c in (self.chain, self.one):
            c.vmap_reset(max_points, max_frames, PS)

    def close(self):
        self.chain.close()
        self.one.close()

    def both(self, fn):
        """A public call made alike on both contexts."""
        out = [fn(c) for c in (self.chain, self.one)]
        return out[0]

    def frame(self, fid, st, img, body, grid=GRID, **kw):
        """One frame on both, compared.  -> the chain's (state, stats, match, records)"""
        want = chain_frame(self.chain, self.vp, fid, st, img, body, grid, **kw)
        got_state, got_stats = one_frame(self.one, self.vp, fid, st, img, body, grid, **kw)
        print(fid, {k: v for k, v in want[1].items() if k.startswith("n_") or k == "first_new_id"}, want[1]["observe"],
              want[1]["update"])
        assert got_stats == want[1]
        assert state_bytes(got_state) == state_bytes(want[0])
        assert_same_map(self.chain, self.one)
        return want


@pytest.fixture()
def twin(built, world):  # noqa: F811
    t = Twin(world["cam"])
    yield t
    t.close()


def first_frame(t, world, n=4000, grid=GRID):  # noqa: F811
    cam, A, sc, imgA = unpack(world)
    return t.frame(0, A, imgA, sc.cloud(A, n, 1), grid)


def prefill(t, world, pick_n, extra_n, own_last=False):  # noqa: F811
    """Frame 0 by the frame call; then `pick_n` of its points get one observation from each of `extra_n` frames
    stored 0.02 m apart to the left of A (the last the furthest from every later frame).  own_last: the last of
    them is a frame of the point's own, 100 + extra_n - 1 + its index.  -> the picked ids"""
    cam, A, sc, imgA = unpack(world)
    first_frame(t, world)
    pts, _, _ = t.chain.vmap_dump()
    obs0 = t.chain.vmap_dump()[1][pts["first_obs"]]
    u, v = obs0["px"][:, 0], obs0["px"][:, 1]
    pick = np.flatnonzero((u > 84) & (u < 132) & (v > 36) & (v < 92))[:pick_n]
    assert len(pick) == pick_n
    seen = pts["pos"][pick].astype(F32)
    groups = [np.arange(pick_n)] * (extra_n - 1) + ([np.array([g]) for g in range(pick_n)] if own_last else [np.arange(pick_n)])
    for j, g in enumerate(groups):
        E = side(sc, A, -0.02 * (j + 1))
        img = sc.render(E)
        p, q = fabricate(seen[g], cam, *pose(E), img, PS)
        t.both(lambda c: c.vmap_add_frame(100 + j, E, t.vp, img))
        t.both(lambda c: c.vmap_add(100 + j, p, q, pick[g].astype(np.int32), np.zeros(len(g), np.int32)))
    assert_same_map(t.chain, t.one, t.but)
    return pick


def loop_frame(t, world, k, **kw):  # noqa: F811
    cam, A, sc, imgA = unpack(world)
    S = side(sc, A, 0.3 * k)
    return t.frame(k, S, sc.render(S), sc.cloud(S, 4000, 10 + k), **kw)


def references(ctx):
    """The restatement of the release: the frame ids that the dump's observations name."""
    return {int(f) for f in ctx.vmap_dump()[1]["frame_id"]}


# ----------------------------------------------------------------- cases ----
def test_first_frame(twin, world):  # noqa: F811
    """An empty map: no survivor, the state unchanged in every byte, the frame stored, points created."""
    cam, A, sc, imgA = unpack(world)
    st1, stats, m, rec = first_frame(twin, world)
    assert stats["n_matched"] == 0 and stats["n_new"] >= 30 and stats["first_new_id"] == 0
    assert state_bytes(st1) == state_bytes(A)
    info = twin.one.vmap_info()
    assert info["n_frames"] == 1 and info["n_points"] == info["n_obs"] == stats["n_new"]
    assert (info["width"], info["height"]) == (160, 128)


def test_closed_loop(twin, world):  # noqa: F811
    """test_gpu_vobserve's closed loop as frames: eight points pre-filled to 20 observations (frame 1, 0.3 m
    away, evicts and adds nothing; from frame 2 on the pose flag adds), then five frames 0.3 m apart.  The
    points that every frame creates compete with the older ones for their cells."""
    prefill(twin, world, 8, MAX_OBS - 1)
    outs = [loop_frame(twin, world, k) for k in range(1, 6)]
    stats = [o[1] for o in outs]
    assert all(s["n_matched"] >= 5 and s["n_new"] > 0 and s["first_new_id"] > 0 for s in stats)
    assert all(sum(s["update"]["updates"]) > 0 and s["update"]["n_meas"] > 0 for s in stats)
    assert sum(s["observe"]["deleted"] for s in stats) >= 1 and sum(s["observe"]["added"] for s in stats) >= 1
    flags = np.concatenate([o[3] for o in outs])["flags"]
    assert np.any(flags & DELETED)
    assert sum(s["observe"]["deleted_without_add"] for s in stats) >= 1 or \
        np.any((flags & (ADDED | BEHIND | OUT_OF_FRAME)) == 0)  # an item in the frame that added nothing
    chosen = set().union(*({int(f) for f in o[2]["records"]["frame_id"]} for o in outs[1:]))
    assert chosen & {1, 2, 3, 4, 5}  # a later match chose an observation that an earlier frame stored
    assert any(state_bytes(o[0]) != state_bytes(side(world["sc"], world["A"], 0.3 * (k + 1))) for k, o in enumerate(outs))


def test_no_survivors_on_a_filled_map(twin, world):  # noqa: F811
    """A frame turned away from the wall: the LiDAR still sees it, the camera has every map point behind it."""
    cam, A, sc, imgA = unpack(world)
    first_frame(twin, world)
    T = moved(A, [0.0, 0.0, 0.0], [0.0, 180.0, 0.0])
    wall = sc._pixels(A, *np.random.default_rng(3).uniform([[20.0], [20.0]], [[140.0], [108.0]], (2, 3000)))[0]
    before = twin.chain.vmap_info()
    st1, stats, m, rec = twin.frame(1, T, imgA, sc.body(T, wall))
    assert stats["n_matched"] == 0 and stats["match"]["map_tested"] > 0 and state_bytes(st1) == state_bytes(T)
    assert twin.one.vmap_info()["n_frames"] == 2
    assert all(v == 0 for k, v in stats["observe"].items() if k != "n_obs_total")
    assert stats["observe"]["n_obs_total"] == before["n_obs"]  # (the chain's: the map's count before the new points)


def test_launch_shapes(built, world):  # noqa: F811
    """More survivors than the update's block of 256 (a grid of 4 pixels: 560 cells inside the border), then
    a map of one point: exactly one survivor."""
    cam, A, sc, imgA = unpack(world)
    t = Twin(cam, max_points=2400, max_frames=4)
    try:
        t.frame(0, A, imgA, sc.cloud(A, 12000, 1), 4)
        B = side(sc, A, 0.02)
        st1, stats, m, rec = t.frame(1, B, sc.render(B), sc.cloud(B, 12000, 2), 4)
        assert stats["n_matched"] > 256 and stats["update"]["n_meas"] == stats["n_matched"] * PS * PS
    finally:
        t.close()
    t = Twin(cam, max_points=200, max_frames=4)
    try:
        p, q = fabricate(lattice(sc, A, [100.5], [60.5]), cam, *pose(A), imgA, PS)
        t.both(lambda c: c.vmap_add_frame(0, A, t.vp, imgA))
        t.both(lambda c: c.vmap_add(0, p, q))
        B = side(sc, A, 0.05)
        st1, stats, m, rec = t.frame(1, B, sc.render(B), sc.cloud(B, 4000, 3))
        assert stats["n_matched"] == 1 and stats["observe"]["n_in"] == 1 and stats["update"]["n_meas"] == PS * PS
    finally:
        t.close()


def raw_detect(ctx, vp, sid, fid, st, img, w=None, h=None, grid=GRID):
    import livo_amd
    s = livo_amd.state_to_c(st)
    d = livo_amd.VdetectParams(grid, 0, 0.0, 100.0)
    vs = livo_amd.VdetectStats()
    h0, w0 = (128, 160) if img is None else img.shape
    rc = ctx._L.livo_vio_detect(ctx.h, sid, fid, C.byref(s), None, C.byref(vp), C.byref(d), livo_amd._ptr(img),
                                w or w0, h or h0, C.byref(vs))
    return rc, livo_amd.state_from_c(s), vs


def test_errors_change_nothing(built, world):  # noqa: F811
    cam, A, sc, imgA = unpack(world)
    t = Twin(cam, max_points=1200, max_frames=2)
    try:
        bare = new_ctx()
        try:
            assert raw_detect(bare, t.vp, -1, 0, A, imgA)[0] == -1  # no map
        finally:
            bare.close()
        first_frame(t, world)
        B = side(sc, A, 0.1)
        imgB, body = sc.render(B), sc.cloud(B, 4000, 2)
        sid = t.one.scan_upload(body)
        before = map_bytes(t.one)
        for fid, img, w in ((0, imgB, None), (1, None, None), (1, imgB, 159), (-1, imgB, None)):
            rc, st, _ = raw_detect(t.one, t.vp, sid, fid, B, img, w)  # a stored id, gray == NULL, a wrong size
            assert rc == -1 and state_bytes(st) == state_bytes(B) and map_bytes(t.one) == before
        assert raw_detect(t.one, t.vp, 77, 1, B, imgB)[0] == -4  # an unknown scan
        assert raw_detect(t.one, t.vp, sid, 1, B, imgB, grid=0)[0] == -1
        t.one.scan_release(sid)
        assert map_bytes(t.one) == before
        t.frame(1, B, imgB, body)
        sid = t.one.scan_upload(body)
        before = map_bytes(t.one)
        rc, st, _ = raw_detect(t.one, t.vp, sid, 2, B, imgB)  # the store holds max_frames frames
        t.one.scan_release(sid)
        assert rc == -7 and state_bytes(st) == state_bytes(B) and map_bytes(t.one) == before
    finally:
        t.close()


def test_max_points_exceeded(built, world):  # noqa: F811
    """Known behind the select: the state, the frames, the points and the observations stay; the dump equals
    the chain context's after livo_vio_match's own capacity error on the same input (the rewarped patches)."""
    import livo_amd
    cam, A, sc, imgA = unpack(world)
    probe = Twin(cam)
    try:
        n0 = first_frame(probe, world)[1]["n_new"]
    finally:
        probe.close()
    t = Twin(cam, max_points=n0 + 3, max_frames=4)
    try:
        first_frame(t, world)
        B = side(sc, A, 0.1)
        imgB, body = sc.render(B), sc.cloud(B, 4000, 2)
        info = t.one.vmap_info()
        sid = t.one.scan_upload(body)
        rc, st, vs = raw_detect(t.one, t.vp, sid, 1, B, imgB)
        t.one.scan_release(sid)
        assert rc == -7 and state_bytes(st) == state_bytes(B) and t.one.vmap_info() == info
        assert vs.n_matched >= 5 and vs.n_new > 3 and vs.first_new_id == n0
        # the chain context: a match whose survivors do not fit the caller's arrays
        sid = t.chain.scan_upload(body)
        s, n = livo_amd.state_to_c(B), C.c_int64()
        one = [np.zeros(1, livo_amd.VMATCH_POINT_DTYPE), np.zeros(3, F64), np.zeros(1, np.int32), np.zeros(3 * PS * PS, F32)]
        rc = t.chain._L.livo_vio_match(t.chain.h, sid, C.byref(s), C.byref(t.vp), GRID, 0, 0.0, 100.0,
                                       livo_amd._ptr(imgB), 160, 128, *(livo_amd._ptr(a) for a in one), 1,
                                       C.byref(n), None)
        t.chain.scan_release(sid)
        assert rc == -7 and n.value == vs.n_matched
        assert_same_map(t.chain, t.one)
        t.both(lambda c: c.vmap_add_frame(1, B, t.vp, imgB))  # ... and the frame id and a slot are still free
        assert_same_map(t.chain, t.one)
    finally:
        t.close()


def test_determinism(built, world):  # noqa: F811
    """The same three frames on two fresh contexts: the same bytes."""
    cam, A, sc, imgA = unpack(world)
    outs = []
    for _ in range(2):
        ctx, vp = new_ctx(), vio_params(cam)
        try:
            ctx.vmap_reset(1200, 4, PS)
            got = []
            for k in range(3):
                S = side(sc, A, 0.3 * k)
                st, stats = one_frame(ctx, vp, k, S, sc.render(S), sc.cloud(S, 4000, 10 + k))
                got += state_bytes(st) + [repr(stats)]
            outs.append(got + map_bytes(ctx)[0])
        finally:
            ctx.close()
    assert outs[0] == outs[1]


def test_release(built, world):  # noqa: F811
    """Six points at 20 observations from 18 frames that only they refer to and one more frame each, the
    furthest, of the point's own: a point that loses its furthest observation leaves that frame without a
    reference.  `one` (max_frames just
    large enough for six frames) releases; its twin (a larger store) never does."""
    import livo_amd
    cam, A, sc, imgA = unpack(world)
    own = 6
    t = Twin(cam, max_points=1200, max_frames=MAX_OBS - 1 + own + 6)
    wide = new_ctx()
    try:
        wide.vmap_reset(1200, 64, PS)
        t.chain, spare = wide, t.chain  # the twin here: the one-call form on a larger store
        spare.close()
        t.frame = lambda fid, st, img, body, grid=GRID: [one_frame(c, t.vp, fid, st, img, body, grid)
                                                         for c in (t.chain, t.one)]
        t.but = ("max_frames",)
        prefill(t, world, own, MAX_OBS - 1, own_last=True)
        for k in range(1, 7):
            a, b = loop_frame(t, world, k)
            assert state_bytes(a[0]) == state_bytes(b[0]) and a[1] == b[1]
            print(k, b[1]["observe"])
        assert_same_map(t.chain, t.one, but=("max_frames",))
        stored = {0} | {100 + j for j in range(MAX_OBS - 2 + own)} | set(range(1, 7))
        idle = sorted(stored - references(t.one))
        print("idle", idle)
        assert len(idle) >= 4 and all(f >= 100 + MAX_OBS - 2 for f in idle)  # (1 shows the release; 4 slots are used below)
        assert t.one.vmap_info()["n_frames"] == len(stored) == t.one.vmap_info()["max_frames"]
        S = side(sc, A, 0.3 * 7)
        img7, body7 = sc.render(S), sc.cloud(S, 4000, 17)
        sid = t.one.scan_upload(body7)
        assert raw_detect(t.one, t.vp, sid, 7, S, img7)[0] == -7  # full
        t.one.scan_release(sid)
        before = map_bytes(t.one)
        L, n = t.one._L, C.c_int64()
        assert L.livo_vmap_release_frames(t.one.h, None, 0, C.byref(n)) == 0 and n.value == len(idle)  # the count
        small = np.full(len(idle), -5, np.int32)
        assert L.livo_vmap_release_frames(t.one.h, livo_amd._ptr(small), len(idle) - 1, C.byref(n)) == -7
        assert n.value == len(idle) and np.all(small == -5) and map_bytes(t.one) == before
        got = t.one.vmap_release_frames()
        assert list(got) == idle
        after = map_bytes(t.one)
        assert after[0] == before[0] and after[1] == dict(before[1], n_frames=before[1]["n_frames"] - len(idle))
        assert len(t.one.vmap_release_frames()) == 0
        # a released id can be stored again; nothing refers to it: it is released again
        t.one.vmap_add_frame(idle[0], A, t.vp, imgA)
        with pytest.raises(livo_amd.LivoError):
            t.one.vmap_add_frame(idle[0], A, t.vp, imgA)
        assert t.one.vmap_info()["n_frames"] == before[1]["n_frames"] - len(idle) + 1
        assert list(t.one.vmap_release_frames()) == [idle[0]] and map_bytes(t.one) == after
        # a frame that only a new point refers to is kept
        p, q = fabricate(lattice(sc, A, [100.5], [60.5]), cam, *pose(A), imgA, PS)
        t.both(lambda c: c.vmap_add_frame(200, A, t.vp, imgA))
        t.both(lambda c: c.vmap_add(200, p, q))
        assert len(t.one.vmap_release_frames()) == 0 and 200 in references(t.one)
        # slot reuse does not show: three more frames beside the twin that never released
        for k in range(7, 10):
            t.one.vmap_release_frames()
            a, b = loop_frame(t, world, k)
            assert state_bytes(a[0]) == state_bytes(b[0]) and a[1] == b[1]
            assert_same_map(t.chain, t.one, but=("max_frames", "n_frames"))
        assert t.one.vmap_info()["n_frames"] < t.chain.vmap_info()["n_frames"] == len(stored) + 4
    finally:
        t.close()
