"""GPU parity of the VIO photometric update:
livo_vio_update against the oracle's ComputeJ / UpdateState restatement.

Bars: iteration / update counts, out_of_frame and the per-level float errors
exact (they steer the reference's control flow: `error <= last_error`, the
error is the float sum of the per-point patch errors in point order, summed
the same way on the device); per-point patch errors bit-exact; state within
1e-9 m / rad of the oracle (HᵀH is summed in a different order); covariance
within 1e-12.

Every case that is there for one branch (clamped reads, the revert, the later
chunks of the error sum) first asserts on the oracle's result that the branch
is taken, so it cannot quietly stop covering it.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 24576  # k_vio_solve stages the patch errors in LDS this many at a time


@pytest.fixture(scope="module")
def vctx(built):
    import livo_amd
    ctx = livo_amd.Context(0)
    yield ctx
    ctx.close()


def _check(g, r):
    gs, gst, gerr = g
    rs, rst, rerr = r
    assert gst["iterations"] == rst["iterations"] and gst["updates"] == rst["updates"]
    assert gst["cov_updated"] == rst["cov_updated"] and gst["n_meas"] == rst["n_meas"]
    assert gst["out_of_frame"] == rst["out_of_frame"]
    assert np.array_equal(np.float32(gst["last_error"]), np.float32(rst["last_error"]))
    assert np.array_equal(gerr.view(np.uint32), rerr.view(np.uint32))
    assert np.abs(gs["pos"] - rs["pos"]).max() < 1e-9
    assert np.abs(gs["rot"] - rs["rot"]).max() < 1e-9
    assert np.abs(gs["cov"] - rs["cov"]).max() < 1e-12


def _reverted(stats):
    """Per level 2, 1, 0: the level ended in the revert branch (an iteration whose error grew)."""
    return [i > u for i, u in zip(stats["iterations"], stats["updates"])]


def _finite(res):
    s, stats, err = res
    return all(np.isfinite(v).all() for v in s.values()) and np.isfinite(err).all() and \
        np.isfinite(stats["last_error"]).all()


def _bytes(res):
    s, stats, err = res
    return b"".join(np.ascontiguousarray(s[k]).tobytes() for k in sorted(s)), \
        {k: (np.float32(v).tobytes() if k == "last_error" else v) for k, v in stats.items()}, err.tobytes()


@pytest.mark.parametrize("n,fid", [(2000, 0), (300, 1), (5000, 2), (1, 3)])
def test_vio_update_parity(vctx, n, fid):
    import oracle
    from livo_amd import synth
    fr, st, truth = synth.make_vio_frame(n, fid)
    g = vctx.vio_update(fr, st)
    r = oracle.vio_update(fr, st)
    _check(g, r)
    if n >= 300:
        assert np.linalg.norm(g[0]["pos"] - truth["pos"]) < 0.2 * np.linalg.norm(st["pos"] - truth["pos"])


def test_vio_prior_and_iterations(vctx):
    import oracle
    from livo_amd import synth
    fr, st, _ = synth.make_vio_frame(1500, 4)
    prior = dict(st)
    prior["pos"] = st["pos"] + np.array([0.01, -0.005, 0.002])
    for it in (0, 1, 2, 10):
        _check(vctx.vio_update(fr, st, prior, max_iter=it), oracle.vio_update(fr, st, prior, max_iter=it))


def test_vio_patch_size_and_cov(vctx):
    import oracle
    from livo_amd import synth
    fr, st, _ = synth.make_vio_frame(800, 5, patch_size=6)
    _check(vctx.vio_update(fr, st, img_point_cov=100.0), oracle.vio_update(fr, st, img_point_cov=100.0))


def test_vio_no_points(vctx):
    from livo_amd import synth
    fr, st, _ = synth.make_vio_frame(10, 6)
    for k in ("pos", "levels", "patches"):
        fr[k] = fr[k][:0]
    s, stats, _ = vctx.vio_update(fr, st)
    assert np.array_equal(s["pos"], st["pos"]) and stats["iterations"] == [0, 0, 0] and stats["cov_updated"] == 0


# ------------------------------------------------ frame edge and revert ----
@pytest.fixture(scope="module")
def frame257(built):
    from livo_amd import synth
    return synth.make_vio_frame(257, 8)


@pytest.fixture(scope="module")
def cropped257(frame257):
    """(frame, state, oracle result) of a 460x332 window of the 257-point frame: points
    near and beyond its border, every level ending in a revert."""
    import oracle
    from livo_amd import synth
    fr, st, _ = frame257
    fr = synth.crop_vio_frame(fr, 90, 90, 550, 422)
    r = oracle.vio_update(fr, st)
    assert r[1]["out_of_frame"] > 0 and all(_reverted(r[1])) and r[1]["cov_updated"] == 1
    return fr, st, r


def test_vio_clamped_border_reverts_every_level(vctx, cropped257):
    fr, st, r = cropped257
    _check(vctx.vio_update(fr, st), r)


def test_vio_update_after_a_reverted_level(vctx):
    """Two levels revert among 600 points and a later level runs clean from the restored state."""
    import oracle
    from livo_amd import synth
    fr, st, _ = synth.make_vio_frame(600, 8)
    fr = synth.crop_vio_frame(fr, 100, 90, 540, 420)
    r = oracle.vio_update(fr, st)
    rev = _reverted(r[1])
    assert sum(rev) >= 2 and r[1]["out_of_frame"] > 0
    assert any(rev[k] and not rev[j] and r[1]["updates"][j] > 0 for k in range(3) for j in range(k + 1, 3))
    _check(vctx.vio_update(fr, st), r)


def test_vio_revert_without_border(vctx):
    """A large initial error and 10 iterations: every level reverts with all points well inside the frame."""
    import oracle
    from livo_amd import synth
    fr, st, _ = synth.make_vio_frame(600, 7, rot_deg=1.0, trans_m=0.1)
    r = oracle.vio_update(fr, st, max_iter=10)
    assert all(_reverted(r[1])) and r[1]["out_of_frame"] == 0
    _check(vctx.vio_update(fr, st, max_iter=10), r)


def test_vio_point_levels_to_eight(vctx, frame257):
    """Point levels 0..8: scale reaches 1024 at pyramid level 2, every tap of the coarse points is clamped."""
    import oracle
    fr, st, _ = frame257
    fr = dict(fr, levels=(np.arange(len(fr["pos"])) % 9).astype(np.int32))
    r = oracle.vio_update(fr, st)
    assert r[1]["out_of_frame"] > 0 and int(fr["levels"].max()) == 8
    _check(vctx.vio_update(fr, st), r)


def test_vio_points_behind_the_camera(vctx, frame257):
    """Every 16th point at negative depth: a finite pixel, the projection Jacobian's sign flipped."""
    import oracle
    from livo_amd import synth
    fr, st, truth = frame257
    fr = synth.mirror_vio_points(fr, truth, 16)
    r = oracle.vio_update(fr, st)
    assert _finite(r)
    g = vctx.vio_update(fr, st)
    assert _finite(g)
    _check(g, r)


def test_vio_undistorted_camera(vctx):
    """d0 = 0: vikit's world2cam without the distortion polynomial (P.distortion == 0)."""
    import oracle
    from livo_amd import synth
    fr, st, _ = synth.make_vio_frame(300, 11)
    fr["cam"] = dict(fr["cam"], d=[0.0] * 5)
    _check(vctx.vio_update(fr, st), oracle.vio_update(fr, st))


@pytest.mark.parametrize("ps", [1, 2, 3, 5, 8])
def test_vio_patch_sizes(vctx, ps):
    """The smallest, the odd (patch_size / 2 rounds down) and the largest patch the ABI accepts."""
    import oracle
    from livo_amd import synth
    fr, st, _ = synth.make_vio_frame(300, 9, patch_size=ps)
    r = oracle.vio_update(fr, st)
    assert r[1]["n_meas"] == len(fr["pos"]) * ps * ps
    _check(vctx.vio_update(fr, st), r)


# ------------------------------------- the chunked error sum, LDS request ----
@pytest.fixture(scope="module")
def base1031(built):
    from livo_amd import synth
    return synth.make_vio_frame(1031, 10)


_tiled_cache = {}


def _tiled(base1031, n):
    """(frame, state, oracle result) of the 1,031-point frame tiled to n points; computed once per n."""
    if n not in _tiled_cache:
        import oracle
        from livo_amd import synth
        fr, st, _ = base1031
        fr = synth.tile_vio_frame(fr, n, seed=n)
        _tiled_cache[n] = (fr, st, oracle.vio_update(fr, st))
    return _tiled_cache[n]


# 16,385: the first size whose dynamic LDS passes 64 KB; 24,576: exactly one chunk;
# 24,577: a second chunk of one element (scalar tail only); 24,609: a second chunk of
# 32 + 1; 49,153: three chunks, the last of one element
@pytest.mark.parametrize("n", [16385, CHUNK, CHUNK + 1, CHUNK + 33, 2 * CHUNK + 1])
def test_vio_error_sum_size_edges(vctx, base1031, n):
    import oracle
    fr, st, r = _tiled(base1031, n)
    assert len(fr["pos"]) == n
    g = vctx.vio_update(fr, st)
    _check(g, r)
    # level 2's error from the unmodified input state: no solve rounding upstream of it
    g1 = vctx.vio_update(fr, st, max_iter=1)
    r1 = oracle.vio_update(fr, st, max_iter=1)
    assert g1[1]["iterations"] == r1[1]["iterations"] == [1, 1, 1]
    assert np.float32(g1[1]["last_error"][0]).tobytes() == np.float32(r1[1]["last_error"][0]).tobytes()
    # without the oracle: level 0's last iteration updated, so its error is the float
    # sum of the returned patch errors in point order over n_meas
    assert r[1]["iterations"][2] == r[1]["updates"][2] and g[1]["iterations"][2] == g[1]["updates"][2]
    n_meas = n * fr["patch_size"] ** 2
    assert g[1]["n_meas"] == n_meas
    fwd = np.float32(np.cumsum(g[2], dtype=np.float32)[-1]) / np.float32(n_meas)
    rev = np.float32(np.cumsum(g[2][::-1], dtype=np.float32)[-1]) / np.float32(n_meas)
    assert fwd.tobytes() != rev.tobytes()  # the order of the sum shows in the result
    assert fwd.tobytes() == np.float32(g[1]["last_error"][2]).tobytes()


def test_vio_context_reuse_is_isolated(vctx, base1031, cropped257):
    """One context, n growing then shrinking: the frame buffer is reused, and nothing of
    an earlier call (partials, patch errors, out_of_frame) reaches a later one."""
    big, st_big, r_big = _tiled(base1031, 2 * CHUNK + 1)
    crop, st_crop, r_crop = cropped257
    empty = dict(crop)
    for k in ("pos", "levels", "patches"):
        empty[k] = crop[k][:0]
    big1 = vctx.vio_update(big, st_big)
    crop1 = vctx.vio_update(crop, st_crop)
    s0, stats0, err0 = vctx.vio_update(empty, st_crop)
    crop2 = vctx.vio_update(crop, st_crop)
    big2 = vctx.vio_update(big, st_big)
    _check(big1, r_big)
    _check(crop1, r_crop)
    assert all(np.array_equal(s0[k], st_crop[k]) for k in s0)
    assert stats0["iterations"] == [0, 0, 0] and stats0["updates"] == [0, 0, 0]
    assert stats0["cov_updated"] == 0 and stats0["out_of_frame"] == 0 and len(err0) == 0
    assert _bytes(crop2) == _bytes(crop1)
    assert _bytes(big2) == _bytes(big1)
