"""CPU tests of the iVox restatement (oracle/livo_oracle.cpp, section iVox) and of
the device's std::nth_element restatement (fast-livo-noted_amd/csrc/stl_select.h).

Parity status of the iVox backend: the reference ships no tests or fixtures
for it and cannot be built here (glog/PCL/Eigen absent), so the
restatement is pinned against independent numpy restatements of each
documented behaviour:
  * the candidate SET of GetClosestPoint (ivox3d.h:132-204) = the max_num
    smallest in-range points of the nearby grids, nearest first (continuous
    random data, so no ties);
  * AddPoints' LRU grid cache with eviction at capacity (ivox3d.h:256-281)
    against an OrderedDict restatement, point order included;
  * map_incremental's add / no-downsample / skip decision
    (laser_mapping.cpp:329-389) against numpy float32 arithmetic.
The ORDER of the candidates is libstdc++'s std::nth_element's, which the
oracle calls directly; the device restates it (stl_select.h), checked here
element for element against libstdc++ on 300k random arrays and Musser's
median-of-3 killer sequences (the heap-select branch).
"""
import collections
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_nth_element_restatement_matches_libstdcxx(tmp_path):
    exe = tmp_path / "sel_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "fast-livo-noted_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "sel_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe), "300000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 mismatches" in out.stdout


def test_ball_cells_matches_inline_range(tmp_path):
    """livo_internal.h ball_cells (the cell range of a bound ball, host-callable) against a literal
    restatement of the expressions the searches held inline: equal integer ranges and equal rejections."""
    exe = tmp_path / "ball_cells_check"
    # (host code only; the header's HIP vector types come with hipcc, as for the library's own .cpp files)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "fast-livo-noted_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "ball_cells_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe), "5000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 mismatches" in out.stdout


def _round_half_away(x):
    return np.where(x >= 0, np.floor(x + np.float32(0.5)), -np.floor(-x + np.float32(0.5)))


NEAR18 = [(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (1, 1, 0), (-1, 1, 0),
          (1, -1, 0), (-1, -1, 0), (1, 0, 1), (-1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 1), (0, -1, 1),
          (0, 1, -1), (0, -1, -1)]


def _keys(p, res):
    inv = np.float32(1.0 / res)
    return _round_half_away(p.astype(np.float32) * inv).astype(np.int64)


@pytest.mark.parametrize("res", [0.2, 0.5])
def test_ivox_knn_set_matches_numpy(built, res):
    import oracle
    rng = np.random.default_rng(5)
    m = rng.uniform(-3, 3, size=(30_000, 3)).astype(np.float32)
    q = rng.uniform(-3.2, 3.2, size=(2_000, 3)).astype(np.float32)
    iv = oracle.Ivox(resolution=res, nearby_type=18)
    iv.add_points(m)
    idx, d, xyz, cnt = iv.knn(q, 5, 5.0)
    mk = _keys(m, res)
    grid = collections.defaultdict(list)
    for i, k in enumerate(map(tuple, mk)):
        grid[k].append(i)
    qk = _keys(q, res)
    for i in range(q.shape[0]):
        cand = []
        for dl in NEAR18:
            cand += grid.get((qk[i, 0] + dl[0], qk[i, 1] + dl[1], qk[i, 2] + dl[2]), [])
        cand = np.array(cand, np.int64)
        if cand.size:
            dd = m[cand] - q[i]
            dist = dd[:, 0] * dd[:, 0] + (dd[:, 1] * dd[:, 1] + dd[:, 2] * dd[:, 2])
            keep = dist.astype(np.float64) < 25.0
            cand, dist = cand[keep], dist[keep]
        if cand.size == 0:
            assert cnt[i] == -1
            continue
        o = np.argsort(dist, kind="stable")[:5]
        assert cnt[i] == min(5, cand.size)
        assert set(idx[i, :cnt[i]]) == set(cand[o].tolist())
        assert idx[i, 0] == cand[o[0]]  # the final nth_element(begin, begin, end): nearest first
        assert np.array_equal(np.sort(d[i, :cnt[i]]), dist[o])
        assert np.array_equal(xyz[i, :cnt[i]], m[idx[i, :cnt[i]]])


def test_ivox_lru_and_eviction_match_ordereddict(built):
    import oracle
    rng = np.random.default_rng(9)
    pts = rng.uniform(-1, 1, size=(4_000, 3)).astype(np.float32)
    for cap in (1, 7, 50, 10_000):
        iv = oracle.Ivox(resolution=0.3, nearby_type=6, capacity=cap)
        od = collections.OrderedDict()  # key -> [ids]; last = most recently used
        nid = 0
        for lo, hi in ((0, 1000), (1000, 1001), (1001, 4000)):
            iv.add_points(pts[lo:hi])
            for p in pts[lo:hi]:
                k = tuple(_keys(p[None], 0.3)[0])
                if k not in od:
                    od[k] = [nid]
                    if len(od) >= cap:
                        od.popitem(last=False)
                else:
                    od[k].append(nid)
                    od.move_to_end(k)
                nid += 1
        xyz, ids, gof, keys = iv.dump()
        exp_keys = list(reversed(od.keys()))
        assert [tuple(k) for k in keys] == exp_keys
        exp_ids = [i for k in exp_keys for i in od[k]]
        assert ids.tolist() == exp_ids
        assert np.array_equal(xyz, pts[np.array(exp_ids, np.int64)].reshape(-1, 3))
        assert iv.info()["num_grids"] == len(od)


@pytest.mark.parametrize("ext", ["ident", "tilt", "flip"])
def test_map_incremental_matches_numpy(built, ext):
    """ext: the LiDAR-IMU extrinsic (tests/extrinsic_cases.py).  Under tilt and flip the world points are
    oracle.to_world's (held to the 60-digit front-end reference under tilt), so every point the map
    takes is bitwise one of them."""
    import extrinsic_cases as xc
    import oracle
    from livo_amd import synth
    R_LI, t_LI = xc.ext(ext)
    m = synth.make_map(100_000)
    iv = oracle.Ivox()
    iv.add_points(m)
    body, st = xc.scan(4_000, 1, ext)
    cache = oracle.new_cache(body.shape[0])
    st1, stats = iv.iekf_update(body, st, cache, R_LI=R_LI, t_LI=t_LI)
    assert stats["effct_feat_num"][0] >= 0.5 * len(body) and stats["iterations"] >= 2
    n0 = iv.info()["num_points"]
    fs = 0.5
    cat, counts = iv.map_incremental(body, st1, cache, R_LI=R_LI, t_LI=t_LI, filter_size_map=fs)
    # numpy restatement of laser_mapping.cpp:343-380
    pw = oracle.to_world(body, st1, R_LI, t_LI)[:, :3]
    if ext == "ident":
        pI = body.astype(np.float64) + synth.T_LI
        assert np.array_equal(pw, ((st1["rot"] @ pI.T).T + st1["pos"]).astype(np.float32))
    else:
        assert np.abs(pw - xc.world_of(body, st1, R_LI, t_LI)).max() < 4e-6  # (float32 of metres: the same points)
        if ext == "tilt":  # (not symmetric: the transposed matrix puts them metres away)
            assert np.abs(pw - xc.world_of(body, st1, R_LI.T, t_LI)).max() > 0.5
    f = np.float32(fs)
    c = (np.floor(pw / f) + np.float32(0.5)) * f
    near = cache["xyz"].reshape(-1, 5, 3)
    d0 = np.abs(near[:, 0] - c)
    nodown = np.all(d0.astype(np.float64) > 0.5 * fs, axis=1)

    def nrm(v):
        return np.sqrt(v[..., 0] * v[..., 0] + (v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]))
    dist = nrm(pw - c)
    dn = nrm(near - c[:, None, :])
    closer = np.any(dn.astype(np.float64) < dist[:, None].astype(np.float64) + 1e-6, axis=1)
    full = cache["cnt"] >= 5
    has = cache["cnt"] > 0
    exp = np.where(~has, 1, np.where(nodown, 2, np.where(full & closer, 0, 1)))
    assert np.array_equal(cat, exp)
    assert counts["added"] == int(np.sum(exp == 1)) and counts["no_downsample"] == int(np.sum(exp == 2))
    assert iv.info()["num_points"] == n0 + counts["added"] + counts["no_downsample"]
    # insertion order: points_to_add then point_no_need_downsample, each in point order
    xyz, ids, _, _ = iv.dump()
    new = ids >= n0
    order = np.argsort(ids[new])
    exp_pts = np.concatenate([pw[exp == 1], pw[exp == 2]])
    assert np.array_equal(xyz[new][order].view(np.uint32), exp_pts.view(np.uint32))
    assert counts["added"] > 0 and counts["no_downsample"] + int(np.sum(exp == 0)) > 0


def test_map_incremental_flip_equals_pretransformed_identity(built):
    """The upside-down mounting against a second Ivox driven with R_LI = I on the cloud R_LI p_b:
    diag(1, -1, -1) p_b is exact in float32 and R_LI p_b + t_LI takes the same double operations
    either way (the products by 0 add +-0), so the update, the categories, the counts and the whole map
    are equal bit for bit over two scans.  A dropped or half-applied R_LI in the oracle's iVox loop or
    in its map_incremental breaks it."""
    import extrinsic_cases as xc
    import oracle
    from livo_amd import synth
    R_LI, t_LI = xc.EXT["flip"]
    m = synth.make_map(100_000)
    a, b = oracle.Ivox(), oracle.Ivox()
    a.add_points(m)
    b.add_points(m)
    for sid in (1, 2):
        body, st = xc.scan(4_000, sid, "flip")
        pre = np.ascontiguousarray(body * np.array([1.0, -1.0, -1.0], np.float32))
        assert np.array_equal(pre.astype(np.float64), body.astype(np.float64) @ R_LI.T)
        ca, cb = oracle.new_cache(len(body)), oracle.new_cache(len(body))
        sa, ta = a.iekf_update(body, st, ca, R_LI=R_LI, t_LI=t_LI)
        sb, tb = b.iekf_update(pre, st, cb, R_LI=np.eye(3), t_LI=t_LI)
        assert ta["effct_feat_num"] == tb["effct_feat_num"] and ta["effct_feat_num"][0] >= 0.5 * len(body)
        assert np.array_equal(ta["solution"], tb["solution"]) and np.array_equal(sa["cov"], sb["cov"])
        assert all(np.array_equal(ca[k], cb[k]) for k in ca)
        cat_a, cnt_a = a.map_incremental(body, sa, ca, R_LI=R_LI, t_LI=t_LI, filter_size_map=0.5)
        cat_b, cnt_b = b.map_incremental(pre, sb, cb, R_LI=np.eye(3), t_LI=t_LI, filter_size_map=0.5)
        assert np.array_equal(cat_a, cat_b) and cnt_a == cnt_b and cnt_a["added"] > 0
        for x, y in zip(a.dump(), b.dump()):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_ivox_iekf_converges(built):
    import oracle
    from livo_amd import synth
    m = synth.make_map(300_000)
    iv = oracle.Ivox()
    iv.add_points(m)
    body, _, _ = synth.make_scan(5_000, 2)
    st = synth.make_state(2)
    cache = oracle.new_cache(body.shape[0])
    st1, stats = iv.iekf_update(body, st, cache, t_LI=synth.T_LI)
    assert stats["effct_feat_num"][0] > 1000
    assert stats["iterations"] >= 2
    # a second search from the updated state re-finds about the same matches
    h = iv.h_share(body, st1["rot"], st1["pos"], np.eye(3), synth.T_LI, True, cache)
    assert h["effct"] >= 0.9 * stats["effct_feat_num"][-1]


# ---------------------------------------------------------------------------------------------
# The search cascade's rare branches (tests/ivox_cascade_cases.py; GPU side: tests/test_gpu_ivox_cascade.py)
@pytest.fixture(scope="module")
def adv_cli(tmp_path_factory):
    import ivox_cascade_cases as cc
    return cc.build_cli(tmp_path_factory.mktemp("nth_adversary"))


@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("n", [24, 38, 64, 128, 129, 507, 600])
def test_nth_adversary_reaches_depth_limit(adv_cli, n, first):
    """tests/native/nth_adversary.h against libstdc++ itself, where the iVox search selects: a range of n
    elements after `first` others, nth = first + 4.  The sequence is a permutation, the predicate (a
    replay of introselect's rounds) says the depth limit is reached, and stl_select.h's sel_nth_element
    equals std::nth_element element for element on it, which compares the __heap_select branch at the
    nth that iVox uses."""
    import ivox_cascade_cases as cc
    seq, st = cc.adversary(adv_cli, first + n, first, first + 4)
    assert sorted(seq.tolist()) == list(range(first + n))
    assert st["depth_limit"]
    assert st["sel_matches_std"]
    # the predicate is no constant: a sorted range splits evenly, and 16 elements are too few to run out
    assert not cc.check_keys(adv_cli, np.arange(first + n), first, first + 4)["depth_limit"]
    assert not cc.adversary(adv_cli, first + 16, first, first + 4)[1]["depth_limit"]
    # the unmirrored form (pivot to the bottom) gets there for nth near the end, not for nth = first + 4
    assert cc.adversary(adv_cli, first + n, first, first + n - 5, mirrored=False)[1] == {
        "depth_limit": True, "sel_matches_std": True}


CASCADE_ROUTES = {  # scene -> (the kernel that answers under the default kind, raw points > kWRaw: streams)
    "one-grid-128": ("team", False), "one-grid-129": ("wave-all", False),
    "5+123": ("team", False), "5+124": ("wave-all", False),
    "128-in-range-of-168": ("team", False), "129-in-range-of-169": ("wave-all", False),
    "raw-512": ("wave-all", False), "raw-513-one-grid": ("big-wave", True), "raw-513-streams": ("wave-stream", True),
    "stream-5+507": ("wave-stream", True), "stream-5+508": ("big-wave", True),
    "stream-out-of-range": ("wave-stream", True),
    "depth-0-24": ("team", False), "depth-0-64": ("team", False), "depth-0-128": ("team", False),
    "depth-5-24": ("team", False), "depth-5-64": ("team", False), "depth-5-123": ("team", False),
    "depth-0-300": ("big-wave-lane0", False), "depth-5-300": ("big-wave-lane0", False),
    "depth-0-501": ("big-wave-lane0", True), "depth-5-500": ("big-wave-lane0", True),
    "depth-0-600": ("big-wave-lane0", True), "depth-5-600": ("big-wave-lane0", True),
}


def test_cascade_scenes_are_what_they_claim(built, adv_cli):
    """The scenes of tests/test_gpu_ivox_cascade.py, checked with the oracle and numpy alone so the GPU
    comparison cannot pass vacuously: for every query the raw point total, the in-range count per grid
    and the longest list (128 / 129, 512 / 513 raw, 5 + 507 / 5 + 508 staged) are the intended ones, the
    branch they imply under the code's capacities is the intended one, every adversarial segment makes
    the introselect predicate say "limit reached" as staged (distances as keys, at its first), and the
    oracle finds what the counts say."""
    import ivox_cascade_cases as cc
    import oracle
    scenes = cc.capacity_scenes() + [cc.depth_scene(adv_cli, f, n) for f, n in cc.DEPTH_CASES]
    assert {s["name"] for s in scenes} == set(CASCADE_ROUTES)
    for s in scenes:
        ex = s["expect"]
        pk = cc.keys_of(s["points"], s["res"])
        max_grid = int(np.unique(pk, axis=0, return_counts=True)[1].max())
        slice_entries = cc.NEARBY[s["nearby_type"]] * cc.KNN + max_grid + 8
        iv = oracle.Ivox(resolution=s["res"], nearby_type=s["nearby_type"])
        iv.add_points(s["points"])
        _, rd, _, rc = iv.knn(s["queries"], s["max_num"], s["max_range"])
        for qi, q in enumerate(s["queries"]):
            tr = cc.trace(s, q)
            assert (tr["raw"], tr["peak"]) == (ex["raw"], ex["peak"]), (s["name"], qi)
            want, streams = CASCADE_ROUTES[s["name"]]
            assert cc.route(tr, ex["limit"], slice_entries) == want, (s["name"], qi)
            assert (tr["raw"] > cc.WRAW) == streams, (s["name"], qi)
            assert rc[qi] == min(tr["final"], s["max_num"])
            assert rd[qi, 0] == min(d.min() for _, d in tr["segs"] if len(d))
            for t, first, length in s["adv"]:
                assert tr["counts"][t] == length and tr["segs"][t][0] == first
                # the adversarial grid's points are the nearest: its selection is what the query returns
                assert np.array_equal(np.sort(rd[qi]), np.sort(tr["segs"][t][1])[:s["max_num"]])
                if qi in (0, len(s["queries"]) - 1):
                    keys = np.concatenate([np.zeros(first, np.float32), tr["segs"][t][1]])
                    st = cc.check_keys(adv_cli, keys, first, first + 4)
                    assert st["depth_limit"] and st["sel_matches_std"], (s["name"], qi)
        if not s["adv"]:  # the shuffled grids split evenly: no depth limit on the way
            tr = cc.trace(s, s["queries"][0])
            for first, d in tr["segs"]:
                if len(d) > s["max_num"]:
                    keys = np.concatenate([np.zeros(first, np.float32), d])
                    assert not cc.check_keys(adv_cli, keys, first, first + s["max_num"] - 1)["depth_limit"]
    # the LDS edge: the largest slice that fits 64 KB, and one entry more
    g = cc.lds_edge_grid()
    for over in (False, True):
        s = cc.lds_scene(over)
        pk = cc.keys_of(s["points"], s["res"])
        uk, cnt = np.unique(pk, axis=0, return_counts=True)
        assert cnt.max() == s["expect"]["max_grid"] == g + over and tuple(uk[cnt.argmax()]) == (0, 0, 0)
        sl = cc.NEARBY[s["nearby_type"]] * cc.KNN + int(cnt.max()) + 8
        assert sl == s["expect"]["slice"]
        assert (sl * cc.ENTRY_BYTES <= cc.LDS_BYTES) == (not over)
        assert (sl + 1) * cc.ENTRY_BYTES > cc.LDS_BYTES >= (sl - 1) * cc.ENTRY_BYTES
        qk = cc.keys_of(s["queries"], s["res"])
        assert {tuple(k) for k in qk} == set(cc.NEAR26[:7])  # the grid's own cell and every neighbour
        routes, ties = set(), 0
        for q in s["queries"][::8]:
            tr = cc.trace(s, q)
            routes.add(cc.route(tr, False, sl))
            d = np.concatenate([x for _, x in tr["segs"]])
            ties += len(d) - len(np.unique(d))
        assert routes == {"big-global" if over else "big-wave"}
        assert ties > 1000  # exact duplicate distances: the order inside ties is nth_element's
    # keys and range: some coordinates do make exact half products, at both resolutions and signs
    for res in (0.5, 0.2):
        pts, exact = cc.half_product_points(res)
        inv = np.float32(1.0 / float(np.float32(res)))
        prod = (pts[:len(exact), 0] * inv)[exact]
        assert (prod > 0).sum() >= 3 and (prod < 0).sum() >= 3 and np.all(prod - np.floor(prod) == 0.5)
