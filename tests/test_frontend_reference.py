"""The CPU oracle's scan front-end (oracle.undistort, oracle.voxel_grid, oracle.to_world) against
the plain numpy restatement oracle/frontend_ref.py, on every edge input of
tests/frontend_cases.py: unsorted times, exact segment boundaries, zero-length segments, the
first point's chain, the small-angle branch of Exp, non-trivial extrinsics, and VoxelGrid's
membership, size and int32 edges.  The same inputs and bars (derived in frontend_cases's
docstring) hold the device front-end in tests/test_gpu_frontend_edges.py; here they pin the
oracle off its trivial points, without a GPU.
"""
import numpy as np
import pytest

import frontend_cases as fc
import frontend_ref as fr


@pytest.mark.parametrize("ext", ["ident", "tilt"])
@pytest.mark.parametrize("case", fc.DESKEW_CASES, ids=fc.case_id)
def test_oracle_undistort(built, case, ext):
    import oracle
    frame = fc.deskew_frame(case, ext)
    R_LI, t_LI = fc.EXTRINSICS[ext]
    got = oracle.undistort(frame.raw, frame.poses, frame.rot_end, frame.pos_end, R_LI=R_LI, t_LI=t_LI)
    ref = fc.deskew_reference(frame, ext, got)
    fc.check_deskew(got, frame, ref)


def test_walk_is_the_suffix_minimum():
    """What the cases are for: on unsorted times the head that moves a point is not its own
    segment.  The literal walk against "suffix minimum of own segments" on a random frame, and
    the share of points whose head differs from their own segment."""
    frame = fc.deskew_frame(("segment", "random", 4097), "ident")
    t = frame.raw[:, 4].astype(np.float64) / 1000.0
    off = frame.poses[:, 0]
    own = np.searchsorted(off[:-1], t, side="left") - 1  # last head with offset < t
    suffix = np.minimum.accumulate(own[::-1])[::-1]
    heads = [[] for _ in t]
    for i, h in fr.walk(frame.raw[:, 4], off):
        heads[i].append(h)
    assert all(heads[i] == [suffix[i]] for i in range(1, len(t)))
    assert heads[0] == list(range(suffix[0], -1, -1))
    assert (suffix != own).mean() > 0.5


def test_reference_rounds_the_first_point_between_moves():
    frame = fc.deskew_frame(("first", 8), "tilt")
    R_LI, t_LI = fc.EXTRINSICS["tilt"]
    cl, last, heads = fr.undistort(frame.raw, frame.poses, frame.rot_end, frame.pos_end, R_LI, t_LI)
    assert heads[0] == list(range(7, -1, -1)) and all(len(h) == 1 for h in heads[1:])
    p = frame.raw[0:1, :3]
    for h in heads[0]:
        P, _ = fr.compensate(p, frame.raw[0:1, 4], frame.poses[h:h + 1], frame.rot_end, frame.pos_end, R_LI, t_LI)
        p = P.astype(np.float32)
    assert np.array_equal(cl[0, :3], p[0]) and np.array_equal(last[0], P[0])


@pytest.mark.parametrize("case", fc.VOXEL_CASES, ids=fc.case_id)
def test_oracle_voxel_grid(built, case):
    import oracle
    raw, leaf = fc.voxel_frame(case)
    fc.check_voxels(oracle.voxel_grid(raw, leaf), raw, leaf, fc.oracle_adds)


def test_voxel_cases_are_what_they_say():
    assert len(fr.voxel_grid(*fc.voxel_frame(("one_voxel", 5000))).count) == 1
    for n in (3, 4, 5, 1025):
        assert len(fr.voxel_grid(*fc.voxel_frame(("one_per_voxel", n))).count) == n
    below = fr.voxel_grid(*fc.voxel_frame(("int32", "below")))
    assert below.filtered and int(below.leaf_index.max()) == 1290 ** 3 - 1 >= 2 ** 30  # 31-bit sort keys
    assert not fr.voxel_grid(*fc.voxel_frame(("int32", "above"))).filtered
    for leaf in (0.5, 0.1, 0.3):  # the lattice separates the float32 rule from floor(x / leaf) in double
        raw, _ = fc.voxel_frame(("lattice", leaf))
        v = fr.voxel_grid(raw, leaf)
        assert len(v.count) > 500
    raw, _ = fc.voxel_frame(("lattice", 0.1))
    f32 = np.floor(raw[:, 0] * (np.float32(1.0) / np.float32(0.1)))
    f64 = np.floor(raw[:, 0].astype(np.float64) / 0.1)
    assert (f32 != f64).any()


def test_oracle_voxel_grid_after_deskew(built):
    import oracle
    frame = fc.deskew_frame(("segment", "random", 4097), "tilt")
    R_LI, t_LI = fc.EXTRINSICS["tilt"]
    und = oracle.undistort(frame.raw, frame.poses, frame.rot_end, frame.pos_end, R_LI=R_LI, t_LI=t_LI)
    fc.check_voxels(oracle.voxel_grid(und, 0.2), und, 0.2, fc.oracle_adds, tags=False)


@pytest.mark.parametrize("n", [0, 1, 257, 30000])
def test_oracle_to_world(built, n):
    import oracle
    from livo_amd import synth
    rng = np.random.default_rng(n + 5)
    pts = fc.cloud(n, rng, np.zeros(n))
    st = synth.make_state(3)
    st["rot"] = fc.rot_axis_angle([3.0, -1.0, 2.0], 110.0)
    R_LI, t_LI = fc.EXTRINSICS["tilt"]
    got = oracle.to_world(pts, st, R_LI=R_LI, t_LI=t_LI)
    assert got.shape == (n, 5)
    ref, bar = fc.to_world_bar(pts, st, "tilt", got)
    assert (np.abs(got[:, :3].astype(np.float64) - ref) <= bar).all()
    assert np.array_equal(got[:, 3], pts[:, 3]) and not got[:, 4].any()
