"""The sensor handlers on the device (livo_frame_ingest_livox / _cloud, livo_frame_info / _dump /
_take) against the restatements of tests/ingest_cases.py.

The frame and its info equal the scalar restatement exactly, floats bit for bit: every operation
of the handlers is a single correctly rounded float or double operation in a fixed order, so
there is no error to allow for.  The take's de-skewed points and downsampled cloud equal
livo_scan_preprocess_imu fed the same slice from the host, bit for bit: the two calls run the
same kernels on the same bytes.
"""
import ctypes as C
import os

import numpy as np
import pytest

import imu_cases as imc
import ingest_cases as ic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def ctx(built):
    import livo_amd
    from livo_amd import synth
    c = livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=4)
    yield c
    c.close()


def _layout(L):
    import livo_amd
    return livo_amd.CloudLayout(L["point_step"], L["off_x"], L["off_y"], L["off_z"], L["off_intensity"], L["off_time"])


def _ingest(ctx, kind, msg, L=None, n_scans=16, filter_num=2, blind=0.01):
    import livo_amd
    p = livo_amd.ingest_params(lidar_type=kind, n_scans=n_scans, point_filter_num=filter_num, blind=blind)
    info = ctx.frame_ingest_livox(msg, p) if kind == ic.AVIA else ctx.frame_ingest_cloud(msg, _layout(L), p)
    assert ctx.frame_info() == info
    return ctx.frame_dump(), info


def _check(got, want, what):
    (gf, gi), (wf, wi) = got, want
    assert gf.shape == wf.shape, (what, gf.shape, wf.shape, gi, wi)
    assert np.array_equal(gf.view(np.uint32), wf.view(np.uint32)), what
    for k, v in wi.items():
        if k == "end_curvature":
            assert F(gi[k]).view(np.uint32) == F(v).view(np.uint32), (what, k)
        else:
            assert gi[k] == v, (what, k, gi[k], v)


@pytest.mark.parametrize("n", ic.SIZES)
def test_avia_sizes_filters_and_densities(ctx, n):
    """Sizes at which the counts cross wave and block edges; against the scalar restatement on one
    filter and density per size in turn, against the vectorised one (which equals it bit for bit,
    tests/test_ingest_reference.py) on the whole grid."""
    grid = [(p, d, r) for p in (1, 2, 3, 7) for d, r in (("none", 0), ("all", 0), ("half", 0), ("half", 300))]
    for k, (p, d, r) in enumerate(grid):
        m = ic.livox_msg(n, d, "random", seed=n + p, run=r)
        got = _ingest(ctx, ic.AVIA, m, filter_num=p)
        _check(got, ic.ingest_vector(ic.AVIA, m, filter_num=p), (n, p, d, r))
        if k % 5 == ic.SIZES.index(n) % 5:
            _check(got, ic.ingest_scalar(ic.AVIA, m, filter_num=p), (n, p, d, r, "scalar"))


@pytest.mark.parametrize("times", ["sorted", "reversed", "random", "ties"])
def test_avia_time_orders(ctx, times):
    """Equal times in runs of 100 points (longer than a wave) keep message order."""
    m = ic.livox_msg(3 * ic.BLOCK + 17, "all", times, seed=3)
    got = _ingest(ctx, ic.AVIA, m, filter_num=1)
    _check(got, ic.ingest_scalar(ic.AVIA, m, filter_num=1), times)
    assert np.all(np.diff(got[0][:, 4]) >= 0) and got[1]["n_kept"] > 3 * ic.BLOCK - 50


def test_avia_quirks_on_the_device(ctx):
    m = np.zeros(8, ic.LIVOX)
    rows = [(9, 9, 9, 0x10, 0, 0), (0.5, 0, 7, 0x10, 16, 5), (0.49, 0.01, 8, 0x10, 0, 4), (30, 0.001, 20, 0xD0, 0, 3),
            (18, 24, 1, 0x20, 0, 2), (18, 25, 2, 0x10, 0, 1), (19, 25, 3, 0x10, 0, 0), (18, 24, 4, 0x10, 17, 9)]
    for k, r in enumerate(rows):
        m[k] = (r[5], r[0], r[1], r[2], 200, r[3], r[4], 0)
    want = ic.ingest_scalar(ic.AVIA, m, n_scans=16, filter_num=1, blind=0.25)
    _check(_ingest(ctx, ic.AVIA, m, n_scans=16, filter_num=1, blind=0.25), want, "quirks")
    assert want[0][:, 2].tolist() == [20, 7]  # sorted by time: point 3 (900 exactly) before point 1 (blind exactly)


@pytest.mark.parametrize("kind,layout", [(ic.OUST64, "ouster"), (ic.VELO16, "velodyne"), (ic.XT32, "hesai"),
                                         (ic.OUST64, "shuffled48"), (ic.VELO16, "shuffled48"),
                                         (ic.XT32, "shuffled48")])
def test_cloud_handlers_layouts_and_times(ctx, kind, layout):
    """The drivers' layouts (Velodyne's 22-byte records put `time` at byte 18) and a point_step of 48
    with shuffled offsets; XT32 stamps before points[0]'s give negative times."""
    L = ic.LAYOUTS[layout]
    k = 0
    for n in (0, 1, 65, ic.BLOCK - 1, ic.BLOCK + 1, 3 * ic.BLOCK + 17):
        for times, p in (("sorted", 1), ("reversed", 2), ("random", 3), ("ties", 1), ("random", 7)):
            d = ic.cloud_msg(kind, n, L, times, seed=n + p, negative=(kind == ic.XT32 and times == "random"))
            got = _ingest(ctx, kind, d, L, filter_num=p, blind=0.5)
            _check(got, ic.ingest_vector(kind, d, L, filter_num=p, blind=0.5), (n, times, p))
            if k % 4 == 0 or n <= 65:
                _check(got, ic.ingest_scalar(kind, d, L, filter_num=p, blind=0.5), (n, times, p, "scalar"))
            if kind == ic.XT32 and times == "random" and n > 65:
                assert (got[0][:, 4] < 0).sum() > 10
            k += 1


def test_blind_equality_and_velodyne_without_times(ctx):
    import livo_amd
    for kind, layout in ((ic.OUST64, "ouster"), (ic.VELO16, "velodyne")):
        L = ic.LAYOUTS[layout]
        d = np.zeros((3, L["point_step"]), np.uint8)
        for i, (x, y, t) in enumerate(((3, 4, 1), (3, 4.01, 2), (3, 3.99, 3))):
            d[i, 0:4], d[i, 4:8] = np.array([x], F).view(np.uint8), np.array([y], F).view(np.uint8)
            d[i, L["off_time"]:L["off_time"] + 4] = np.array([t], np.uint32 if kind == ic.OUST64 else F).view(np.uint8)
        got = _ingest(ctx, kind, d, L, filter_num=1, blind=5.0)
        _check(got, ic.ingest_scalar(kind, d, L, filter_num=1, blind=5.0), kind)
        assert got[1]["n_kept"] == (2 if kind == ic.OUST64 else 1)
    d[2, L["off_time"]:L["off_time"] + 4] = np.array([0.0], F).view(np.uint8)  # the last point's time <= 0
    with pytest.raises(livo_amd.LivoError) as e:
        _ingest(ctx, ic.VELO16, d, L, filter_num=1, blind=5.0)
    assert e.value.code == -1


def _propagate(ctx):
    job, params, carry, state = imc.make_case(20, key="frame")
    st, _, tab = ctx.imu_propagate(job[0], job[1], job[2], params, carry, state)
    return st, tab


@pytest.mark.parametrize("images", [0, 1, 2])
def test_takes_of_a_frame_split_by_images(ctx, images):
    """A LiDAR frame taken in 1, 2 or 3 slices.  Each camera take moves the cursor only; the LiDAR
    take starts where they left it, and its de-skewed points and downsampled cloud equal
    livo_scan_preprocess_imu fed the same slice from the host."""
    m = ic.livox_msg(3 * ic.BLOCK + 17, "all", "random", seed=21)
    m["offset_time"][5:400:9] = 0  # points at time 0: what a camera frame inside the scan consumes
    frame, info = _ingest(ctx, ic.AVIA, m, filter_num=1)
    ref, _ = ic.ingest_scalar(ic.AVIA, m, filter_num=1)
    assert np.array_equal(frame, ref)
    _propagate(ctx)
    cursor = 0
    for k in range(images):  # a camera frame's limit is 0.0 (:222-224)
        want = ic.take_scalar(ref, cursor, 0.0, False)
        if k == 0:
            nt, sid, und, down = ctx.frame_take(0.0, False, make_scan=False)
            assert (sid, und, down) == (None, None, None) and nt >= 44
        else:  # asked for a scan all the same: the second image finds nothing left at time 0
            nt, sid, und, down = ctx.frame_take(0.0, False, leaf_size=0.5)
            assert (nt, sid, len(und), len(down)) == (0, -1, 0, 0)
        assert (nt, ctx.frame_info()["cursor"]) == want, (k, nt, want)
        cursor = want[1]
    lim = ic.take_limit(imc.T0, info["end_curvature"], True)
    want = ic.take_scalar(ref, cursor, lim, True)
    nt, sid, und, down = ctx.frame_take(lim, True, leaf_size=0.5)
    assert (nt, ctx.frame_info()["cursor"]) == want and nt > 0 and want[1] == 0
    _same_as_host(ctx, ref[cursor:cursor + nt], sid, und, down, 0.5)
    w = ctx.frame_to_world(_propagate(ctx)[0], -1)
    assert len(w) == nt  # the frame of the stages that follow is the taken range


def _same_as_host(ctx, part, sid, und, down, leaf):
    if len(part) == 0:
        assert sid == -1 and len(und) == 0 and len(down) == 0
        return
    sid2, und2, down2 = ctx.scan_preprocess_imu(part, leaf_size=leaf)
    ctx.scan_release(sid)
    ctx.scan_release(sid2)
    assert np.array_equal(und.view(np.uint32), und2.view(np.uint32))
    assert np.array_equal(down.view(np.uint32), down2.view(np.uint32))
    assert not np.array_equal(und[:, :3], part[:, :3]) or len(part) < 2


def test_take_edges(ctx):
    m = ic.livox_msg(ic.BLOCK + 1, "all", "ties", seed=2)
    frame, info = _ingest(ctx, ic.AVIA, m, filter_num=1)
    _propagate(ctx)
    # nothing at or before the limit: no scan, an empty frame for the stages
    nt, sid, und, down = ctx.frame_take(-1.0, False)
    assert (nt, sid, len(und), len(down), ctx.frame_info()["cursor"]) == (0, -1, 0, 0, 0)
    assert len(ctx.frame_to_world(_propagate(ctx)[0], -1)) == 0
    # a limit inside a run of equal times takes the whole run
    lim = float(frame[150, 4])
    nt, _, _, _ = ctx.frame_take(lim, False, make_scan=False)
    assert nt == ic.take_scalar(frame, 0, lim, False)[0] and frame[nt - 1, 4] == frame[150, 4] < frame[nt, 4]
    # the limit's round trip through a stamp of 1.7e9 s: the tail may stay behind, and the cursor returns to 0
    lim = ic.take_limit(1.7e9, info["end_curvature"], True)
    want = ic.take_scalar(frame, nt, lim, True)
    got, _, _, _ = ctx.frame_take(lim, True, make_scan=False)
    assert (got, ctx.frame_info()["cursor"]) == want
    # past the end: a take on a consumed frame takes nothing
    ctx.frame_take(1e9, False, make_scan=False)
    assert ctx.frame_take(1e9, False, make_scan=False)[0] == 0 and ctx.frame_info()["cursor"] == len(frame)
    # a new ingest replaces the frame and resets the cursor
    assert _ingest(ctx, ic.AVIA, m[:10], filter_num=1)[1]["cursor"] == 0


def test_refusals_that_need_a_context(built):
    import livo_amd
    from livo_amd import synth
    m = ic.livox_msg(100, "all", "random", seed=1)
    with livo_amd.Context(0, t_LI=synth.T_LI) as c:
        for call in (c.frame_dump, c.frame_info, lambda: c.frame_take(0.0, False, make_scan=False)):
            with pytest.raises(livo_amd.LivoError) as e:
                call()
            assert e.value.code == -1
        c.frame_ingest_livox(m, livo_amd.ingest_params(point_filter_num=1))
        nt = C.c_int64()
        sid = C.c_int32()
        # a scan before any livo_imu_propagate is refused and leaves the cursor; the cursor-only take runs
        assert c._L.livo_frame_take(c.h, 1e9, 0, 0.5, C.byref(sid), None, None, 0, None, C.byref(nt)) == -1
        assert c.frame_info()["cursor"] == 0
        assert c.frame_take(1e9, False, make_scan=False)[0] == 99
        n = C.c_int64()
        out = np.zeros((10, 5), F)
        assert c._L.livo_frame_dump(c.h, out.ctypes.data, 10, C.byref(n)) == -6 and n.value == 99


def test_pinned_source_gives_the_same_frame(ctx):
    import livo_amd
    m = ic.livox_msg(3 * ic.BLOCK + 17, "half", "random", seed=9, run=300)
    pageable = _ingest(ctx, ic.AVIA, m, filter_num=2)
    pinned = livo_amd.page_aligned_copy(m)
    ctx.host_register(pinned)
    try:
        _check(_ingest(ctx, ic.AVIA, pinned, filter_num=2), pageable, "pinned")
    finally:
        ctx.host_unregister(pinned)
    _check(pageable, ic.ingest_scalar(ic.AVIA, m, filter_num=2), "pageable")


def test_loop_ingest_propagate_take_update(ctx):
    """ingest -> imu_propagate -> frame_take -> iekf_update on config1_small's map: the state equals
    the run fed the same frame from a host array, bit for bit (the same kernels on the same bytes)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "config1_small.npz"))
    st0 = {k[6:]: g[k] for k in g.files if k.startswith("state_")}
    rng = np.random.default_rng(11)
    scan = np.asarray(g["scan"], F)[:, :3]
    n = len(scan)
    m = np.zeros(n + 1, ic.LIVOX)
    m["x"][1:], m["y"][1:], m["z"][1:] = scan.T
    m["tag"], m["line"] = 0x10, rng.integers(0, 6, n + 1)
    m["offset_time"] = rng.integers(500_000, 99_000_000, n + 1)
    t = imc.T0 + 0.005 * np.arange(22)
    f_body = st0["rot"].T @ (-st0["gravity"]) + st0["bias_a"]
    acc = f_body + rng.normal(0, 0.02, (22, 3))
    gyr = st0["bias_g"] + np.array([0.01, -0.02, 0.015]) + rng.normal(0, 0.002, (22, 3))
    imu = np.concatenate([t[1:, None], acc[1:], gyr[1:]], 1)
    carry = {"last_imu": np.concatenate([[t[0]], acc[0], gyr[0]]), "acc_s_last": np.zeros(3),
             "angvel_last": gyr[0] - st0["bias_g"], "last_lidar_end_time": t[0]}
    start = dict(st0, vel=np.zeros(3), cov=np.eye(18) * 0.01)
    params = imc.inited_params({**imc.default_params(), "mean_acc": f_body})
    ctx.map_build(g["map"])
    frame, info = _ingest(ctx, ic.AVIA, m, filter_num=1, blind=0.01)
    ref, _ = ic.ingest_vector(ic.AVIA, m, filter_num=1, blind=0.01)
    assert np.array_equal(frame, ref) and info["n_kept"] > n // 2  # (the scan's 2000 points lie within 30 m)
    end = t[0] + float(info["end_curvature"]) / 1000.0
    prior, _, _ = ctx.imu_propagate(imu, t[0], end, params, carry, start)
    lim = ic.take_limit(t[0], info["end_curvature"], True)
    nt, sid, _, down = ctx.frame_take(lim, True, leaf_size=0.2)
    s1, t1 = ctx.iekf_update(sid, prior, prior)
    sid2, _, down2 = ctx.scan_preprocess_imu(ref[:ic.take_scalar(ref, 0, lim, True)[0]], leaf_size=0.2)
    s2, t2 = ctx.iekf_update(sid2, prior, prior)
    ctx.scan_release(sid)
    ctx.scan_release(sid2)
    print("loop taken", nt, "of", len(ref), "down", len(down), "iterations", t1["iterations"])
    assert nt == ic.take_scalar(ref, 0, lim, True)[0] and np.array_equal(down, down2)
    assert t1["iterations"] == t2["iterations"] >= 1 and t1["effct_feat_num"][0] > 100
    for k in ("rot", "pos", "vel", "cov"):
        assert np.array_equal(np.asarray(s1[k]), np.asarray(s2[k])), k
