"""Plain restatement of the scan front-end, and nothing else.

TEST INFRASTRUCTURE ONLY (like oracle.py, solve_ref.py, ikfom_ref.py).  numpy only: no C++, nothing
taken from the oracle library, so the oracle and the device front-end can both be held against it.

undistort    ImuProcess::UndistortPcl's backward propagation (src/IMU_Processing.cpp:340-378):

                 it_pcl = last point
                 for it_kp = last pose .. second pose:            head = it_kp - 1
                     for (; t(it_pcl) > head.offset_time; it_pcl--):
                         move *it_pcl with head
                         if it_pcl == first point: break          (without stepping)

             walk() is that loop, literally, on the times alone: it yields the (point, head) pairs
             in the order the reference makes them.  Every point but the first is met once, so
             its move reads the raw input and is independent of every other; compensate() does
             those moves in one vectorised float64 pass.  The first point is met once per
             remaining head; its moves are chained one by one, each stored as float32 before the
             next reads it, as the reference's PointType does.

voxel_grid   PCL 1.10 VoxelGrid<PointXYZINormal>::applyFilter with downsample_all_data_: bounds,
             the keep-the-input rule (dx dy dz > INT32_MAX), the leaf index in PCL's own float32
             operations, voxels in ascending leaf index.  The centroid is the float64 mean of the
             float32 members (no summation order to copy), with sum |x_i| beside it for the
             float32 summation bound.

to_world     RGBpointBodyToWorld (src/laser_mapping.cpp:647-660): rot (R_LI p + t_LI) + pos in
             float64, not rounded.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

POSE_D = 22  # Pose6D: offset_time, acc[3], gyr[3], vel[3], pos[3], rot[9]
INT32_MAX = 2 ** 31 - 1


def so3_exp_dt(gyr, dt):
    """Exp(ang_vel, dt) (so3_math.h:31-52) for (k, 3) rates and (k,) times -> (k, 3, 3)."""
    gyr = np.asarray(gyr, np.float64).reshape(-1, 3)
    dt = np.asarray(dt, np.float64).reshape(-1)
    nrm = np.sqrt((gyr ** 2).sum(1))
    R = np.broadcast_to(np.eye(3), (len(dt), 3, 3)).copy()
    big = nrm > 0.0000001
    if big.any():
        r = gyr[big] / nrm[big, None]
        K = np.zeros((len(r), 3, 3))
        K[:, 0, 1], K[:, 0, 2] = -r[:, 2], r[:, 1]
        K[:, 1, 0], K[:, 1, 2] = r[:, 2], -r[:, 0]
        K[:, 2, 0], K[:, 2, 1] = -r[:, 1], r[:, 0]
        ang = nrm[big] * dt[big]
        R[big] = np.eye(3) + np.sin(ang)[:, None, None] * K + (1.0 - np.cos(ang))[:, None, None] * (K @ K)
    return R


def _norm(v):
    return np.sqrt((np.asarray(v, np.float64) ** 2).sum(-1))


def compensate(xyz, t_ms, heads, rot_end, pos_end, R_LI, t_LI):
    """One move of each point (IMU_Processing.cpp:359-370), float64 throughout:

        dt = t / 1000 - head.offset_time
        R_i = head.rot Exp(head.gyr, dt)
        T_ei = head.pos + head.vel dt + 0.5 head.acc dt^2 - pos_end
        P = R_LI^T rot_end^T (R_i (R_LI p + t_LI) + T_ei) - R_LI^T t_LI

    xyz (k, 3) float32 or float64, t_ms (k,) float32, heads (k, 22).  Returns (P (k, 3) float64,
    M (k,)): M is the largest magnitude the chain passes through (the norms of p, t_LI,
    R_LI p + t_LI, head.pos, pos_end, the velocity and acceleration terms taken at
    max(|dt|, |t|), T_ei, the rotated sums and P), the scale of its float64 rounding.
    """
    xyz = np.asarray(xyz).astype(np.float64).reshape(-1, 3)
    heads = np.asarray(heads, np.float64).reshape(-1, POSE_D)
    R_LI = np.asarray(R_LI, np.float64).reshape(3, 3)
    t_LI = np.asarray(t_LI, np.float64).reshape(3)
    rot_end = np.asarray(rot_end, np.float64).reshape(3, 3)
    pos_end = np.asarray(pos_end, np.float64).reshape(3)
    t = np.asarray(t_ms, np.float32).reshape(-1).astype(np.float64) / 1000.0
    dt = t - heads[:, 0]
    acc, gyr, vel, pos = heads[:, 1:4], heads[:, 4:7], heads[:, 7:10], heads[:, 10:13]
    Ri = heads[:, 13:22].reshape(-1, 3, 3) @ so3_exp_dt(gyr, dt)
    T = pos + vel * dt[:, None] + 0.5 * acc * (dt * dt)[:, None] - pos_end
    a = xyz @ R_LI.T + t_LI
    b = np.einsum("kij,kj->ki", Ri, a) + T
    c = b @ (R_LI.T @ rot_end.T).T
    P = c - R_LI.T @ t_LI
    span = np.maximum(np.abs(dt), np.abs(t))
    M = np.max(np.stack([_norm(xyz), np.full(len(t), _norm(t_LI)), _norm(a), _norm(pos),
                         np.full(len(t), _norm(pos_end)), _norm(vel) * span, 0.5 * _norm(acc) * span * span,
                         _norm(T), _norm(b), _norm(P)]), axis=0)
    return P, M


def walk(t_ms, offsets):
    """The reference's two nested loops on the times alone.  t_ms: (n,) float32 curvature;
    offsets: (np,) float64 offset_time.  Returns the (point, head) pairs in the order made."""
    t = [float(x) / 1000.0 for x in np.asarray(t_ms, np.float32).reshape(-1)]
    off = [float(x) for x in np.asarray(offsets, np.float64).reshape(-1)]
    pairs = []
    if not t:
        return pairs
    it = len(t) - 1
    for kp in range(len(off) - 1, 0, -1):
        head = kp - 1
        while t[it] > off[head]:
            pairs.append((it, head))
            if it == 0:
                break
            it -= 1
    return pairs


def undistort(raw, poses, rot_end, pos_end, R_LI, t_LI):
    """raw (n, 5) float32 x, y, z, intensity, curvature (ms); poses (np, 22).  Returns

        cloud   (n, 5) float32: every moved point rounded to float32 as it is stored
        last    (n, 3) float64: the unrounded result of each point's last move (the raw
                coordinates for a point that is never moved)
        heads   per point, the list of heads that moved it, in the walk's order
    """
    raw = np.ascontiguousarray(raw, np.float32).reshape(-1, 5)
    poses = np.asarray(poses, np.float64).reshape(-1, POSE_D)
    n = len(raw)
    cloud = raw.copy()
    last = raw[:, :3].astype(np.float64)
    heads = [[] for _ in range(n)]
    pairs = walk(raw[:, 4], poses[:, 0]) if len(poses) else []
    for i, h in pairs:
        heads[i].append(h)
    once = np.array([i for i in range(1, n) if heads[i]], np.int64)
    assert all(len(heads[i]) == 1 for i in once)  # the pointer only steps back
    if len(once):
        hh = np.array([heads[i][0] for i in once], np.int64)
        P, _ = compensate(raw[once, :3], raw[once, 4], poses[hh], rot_end, pos_end, R_LI, t_LI)
        last[once] = P
        cloud[once, :3] = P.astype(np.float32)
    if n:
        for h in heads[0]:  # chained: each move reads the float32 the one before it stored
            P, _ = compensate(cloud[0:1, :3], raw[0:1, 4], poses[h:h + 1], rot_end, pos_end, R_LI, t_LI)
            last[0] = P[0]
            cloud[0, :3] = P[0].astype(np.float32)
    return cloud, last, heads


class Voxels(NamedTuple):
    filtered: bool        # False: dx dy dz > INT32_MAX, PCL returns the input (one "voxel" per point)
    members: list         # per voxel, the input indices of its points, ascending
    count: np.ndarray     # (k,) int64
    centroid: np.ndarray  # (k, 5) float64 mean of the float32 members
    abs_sum: np.ndarray   # (k, 5) float64 sum |x_i| per column
    leaf_index: np.ndarray  # (k,) the 32-bit leaf index of each voxel, ascending


def voxel_grid(raw, leaf):
    """PCL VoxelGrid::applyFilter (pcl/filters/impl/voxel_grid.hpp) of (n, 5) float32 points."""
    raw = np.ascontiguousarray(raw, np.float32).reshape(-1, 5)
    n = len(raw)
    r64 = raw.astype(np.float64)
    if n == 0:
        z = np.zeros((0, 5))
        return Voxels(True, [], np.zeros(0, np.int64), z, z, np.zeros(0, np.uint32))
    one = np.float32(1.0)
    inv = one / np.float32(leaf)  # inverse_leaf_size_ = Array4f::Ones() / leaf_size_
    mn = raw[:, :3].min(0)
    mx = raw[:, :3].max(0)
    d = [int(np.float32(np.float32(mx[k] - mn[k]) * inv)) + 1 for k in range(3)]  # static_cast<int64_t>: truncation
    if d[0] * d[1] * d[2] > INT32_MAX:
        return Voxels(False, [np.array([i]) for i in range(n)], np.ones(n, np.int64), r64, np.abs(r64),
                      np.zeros(n, np.uint32))
    min_b = np.floor(mn * inv).astype(np.int64)
    max_b = np.floor(mx * inv).astype(np.int64)
    div_b = max_b - min_b + 1
    mul = np.array([1, div_b[0], div_b[0] * div_b[1]], np.int64)
    cell = np.floor(raw[:, :3] * inv)                   # float32 product, float32 floor
    assert cell.dtype == np.float32
    ijk = (cell - min_b.astype(np.float32)).astype(np.int64)  # float32 difference, static_cast<int>
    idx = ((ijk * mul).sum(1) & 0xFFFFFFFF).astype(np.uint32)  # int arithmetic, read as unsigned int
    order = np.argsort(idx, kind="stable")
    keys, start, count = np.unique(idx[order], return_index=True, return_counts=True)
    members = np.split(order, start[1:])
    centroid = np.add.reduceat(r64[order], start, axis=0) / count[:, None]
    abs_sum = np.add.reduceat(np.abs(r64[order]), start, axis=0)
    return Voxels(True, members, count.astype(np.int64), centroid, abs_sum, keys)


def to_world(points, state, R_LI, t_LI):
    """rot (R_LI p + t_LI) + pos for (n, >= 3) points, float64, not rounded -> (n, 3)."""
    p = np.asarray(points)[:, :3].astype(np.float64)
    R_LI = np.asarray(R_LI, np.float64).reshape(3, 3)
    rot = np.asarray(state["rot"], np.float64).reshape(3, 3)
    return (p @ R_LI.T + np.asarray(t_LI, np.float64)) @ rot.T + np.asarray(state["pos"], np.float64)


def ulp32(x):
    """The spacing of float32 in the binade of |x|: 2^(e - 24) for |x| in [2^(e-1), 2^e), 2^-149 at least."""
    _, e = np.frexp(np.abs(np.asarray(x, np.float64)))
    return np.ldexp(1.0, np.maximum(e - 24, -149))
