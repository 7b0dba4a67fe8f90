"""CPU tests of the scan front-end restatement (oracle/livo_oracle.cpp, scan
front-end section).

Parity status: "parity unpinned" against the reference itself (ROS/PCL/Eigen
absent; the reference ships no fixtures).  Pinned against the independent numpy
restatements of the documented behaviour in oracle/frontend_ref.py (on the edge
inputs, with derived bars: tests/test_frontend_reference.py):
  * UndistortPcl's backward walk (IMU_Processing.cpp:340-378), including the
    first point being re-compensated by every remaining IMU segment (the inner
    loop breaks at begin() without stepping) and points at or before the first
    pose untouched;
  * PCL VoxelGrid::applyFilter: leaf indices, voxel order (ascending index),
    point counts exact; centroids to float rounding (the reference sums a
    voxel in std::sort's unstable order; the restatement's centroid is the
    float64 mean).
"""
import numpy as np

import frontend_ref as fr


def _undistort_np(raw, poses, Re, pe, RLI, tLI):
    return fr.undistort(raw, poses, Re, pe, RLI, tLI)[0]


def test_undistort_matches_numpy(built):
    import oracle
    from livo_amd import synth
    raw, poses, Re, pe = synth.make_raw_scan(3_000, 1)
    raw[:40, 4] = 0.0  # points at the first pose's time: never compensated
    got = oracle.undistort(raw, poses, Re, pe, t_LI=synth.T_LI)
    exp = _undistort_np(raw, poses, Re, pe, np.eye(3), synth.T_LI)
    assert np.allclose(got, exp, rtol=0, atol=2e-6)
    assert np.array_equal(got[:40], raw[:40])
    assert np.array_equal(got[:, 3:], raw[:, 3:])


def test_undistort_first_point_recompensated(built):
    """A scan whose first point lies after several IMU poses: the reference moves
    it once per remaining segment (its walk breaks at begin() without stepping)."""
    import oracle
    from livo_amd import synth
    raw, poses, Re, pe = synth.make_raw_scan(50, 2)
    raw[:, 4] = np.linspace(30.0, 99.0, 50, dtype=np.float32)
    got = oracle.undistort(raw, poses, Re, pe, t_LI=synth.T_LI)
    exp = _undistort_np(raw, poses, Re, pe, np.eye(3), synth.T_LI)
    assert np.allclose(got, exp, rtol=0, atol=2e-6)
    # point 1 moved once, with the last pose before its time
    h = poses[int(np.searchsorted(poses[:, 0], raw[1, 4] / 1000.0)) - 1]
    once = fr.compensate(raw[1:2, :3], raw[1:2, 4], h, Re, pe, np.eye(3), synth.T_LI)[0][0]
    assert np.allclose(got[1, :3], once, atol=2e-6)
    # point 0 moved by its segment and every earlier one: not the single move
    h0 = poses[int(np.searchsorted(poses[:, 0], raw[0, 4] / 1000.0)) - 1]
    once0 = fr.compensate(raw[0:1, :3], raw[0:1, 4], h0, Re, pe, np.eye(3), synth.T_LI)[0][0]
    assert np.abs(got[0, :3] - once0).max() > 1e-3


def _voxel_np(raw, leaf):
    v = fr.voxel_grid(raw, leaf)
    assert v.filtered
    return v.centroid.astype(np.float32), v.count


def test_voxel_grid_matches_numpy(built):
    import oracle
    from livo_amd import synth
    raw, _, _, _ = synth.make_raw_scan(6_000, 3)
    for leaf in (0.5, 0.2, 0.05):
        got = oracle.voxel_grid(raw, leaf)
        exp, cnt = _voxel_np(raw, leaf)
        assert got.shape == exp.shape
        assert np.allclose(got, exp, rtol=2e-6, atol=2e-5)
    # leaf too small for 32-bit leaf indices: PCL returns the input unchanged
    big = raw.copy()
    big[0, :3] = [-3000, -3000, -3000]
    big[1, :3] = [3000, 3000, 3000]
    assert np.array_equal(oracle.voxel_grid(big, 0.01), big)
