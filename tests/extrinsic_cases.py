"""Scans under a LiDAR-IMU extrinsic other than the identity, shared by the CPU pins of the oracle
(tests/test_oracle.py, test_ivox_oracle.py, test_ikd_incr_oracle.py) and tests/test_gpu_extrinsic.py.

livo_params.R_LI (the reference's Lidar_rot_to_IMU, read from the config at laser_mapping.cpp:1004)
enters every stage that turns a body point into a world point: p_I = R_LI p_b + t_LI, then
p_w = R p_I + p.  synth's scans are made for R_LI = I; body_for() re-expresses one as a LiDAR
mounted otherwise sees it, so that R_LI p + t_LI lands (to one float32 rounding of p) on the
surfaces the identity scan hit and the map still matches.

    tilt   35 degrees about (1, 2, 3), lever arm of decimetres (frontend_cases.EXTRINSICS): not
           symmetric, so a transposed R_LI shows.
    flip   an upside-down mounting, diag(1, -1, -1): exact entries, so a sign or axis mix-up shows
           with no rounding of the matrix in play.

Bars: those the suite applies to the same quantities with R_LI = I (tests/test_gpu_parity.py); the
oracle and the device run the same operations in the same order in double with contraction off,
so the exact ones carry over.  Floors (oracle_floors) are asserted on the oracle's result alone.
"""
from __future__ import annotations

import numpy as np

import frontend_cases as fc

EXT = {
    "tilt": fc.EXTRINSICS["tilt"],
    "flip": (np.diag([1.0, -1.0, -1.0]), np.array([0.05, -0.12, 0.2])),
}
RAGGED = (0, 1, 63, 64, 257)  # companions of the oracle-checked scan in a batch


def _synth():
    from livo_amd import synth
    return synth


def ident():
    """synth's own extrinsic, under which make_scan's points are expressed."""
    synth = _synth()
    return np.eye(3), synth.T_LI.copy()


def ext(name):
    return ident() if name == "ident" else EXT[name]


def body_for(body, R_LI, t_LI):
    """The scan `body` (synth's extrinsic) as a LiDAR mounted at (R_LI, t_LI) sees it:
    R_LI^T (p_I - t_LI), rounded once to float32."""
    synth = _synth()
    R_LI, t_LI = np.asarray(R_LI, np.float64), np.asarray(t_LI, np.float64)
    p = ((np.asarray(body)[:, :3].astype(np.float64) + synth.T_LI) - t_LI) @ R_LI
    return np.ascontiguousarray(p.astype(np.float32))


def world_of(body, st, R_LI, t_LI):
    """float64 world points R (R_LI p + t_LI) + p: for building queries and clouds."""
    pI = np.asarray(body)[:, :3].astype(np.float64) @ np.asarray(R_LI, np.float64).T + np.asarray(t_LI, np.float64)
    return pI @ np.asarray(st["rot"], np.float64).T + np.asarray(st["pos"], np.float64)


def scan(n, sid, name):
    """(body (n, 3) float32 under extrinsic `name`, initial state)."""
    synth = _synth()
    R, t = ext(name)
    return body_for(synth.make_scan(n, sid)[0], R, t), synth.make_state(sid)


def oracle_floors(stats, n, max_iter=4):
    """The oracle's own result says the case is a real one: the scan lands on the map, and (with
    iterations allowed) an evaluation that reuses the neighbours runs as well as one that searches."""
    assert stats["effct_feat_num"][0] >= 0.9 * n, (stats["effct_feat_num"], n)
    if max_iter >= 1:
        assert stats["iterations"] >= 2, stats["iterations"]
