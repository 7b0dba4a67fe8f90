"""Edge inputs of the scan front-end and the bars they are held to, shared by
tests/test_frontend_reference.py (CPU oracle against oracle/frontend_ref.py) and
tests/test_gpu_frontend_edges.py (livo_scan_preprocess against the same reference).

Inputs.  Pose offsets are float64(float32(ms)) / 1000, so a point time (float32 ms, divided by
1000 in double) can equal an offset exactly.  Every pose carries its own jitter in position
(2 cm), velocity, rate and attitude: two adjacent heads move the same point to places
centimetres apart, which is what lets the coordinates show which head moved it.
deskew_reference() asserts that separation (the result under head h - 1 and under head h + 1 differs from the
right one by at least 100 bars in some coordinate) before anything is compared, so a case that
could not tell two heads apart fails on the CPU, from the reference alone.

De-skew bar, point moved once:  |x - ref64| <= ulp32(max(|x|, |ref64|)) / 2 + K 2^-52 M.
The first term is the one float32 rounding of the stored coordinate.  The second covers the
float64 chain on both sides (2^-52 = one 2^-53 rounding each), M being the largest magnitude
in the chain (frontend_ref.compensate).  K counts, in units of 2^-53 M on the result's norm:

    R_LI p + t_LI                  3 x 3 product (3 mul + 2 add a row, <= 3 sqrt(3) < 6) + 1 add     7
    dt = t / 1000 - offset         2 roundings, |err| <= 2^-52 max(|t|, |dt|); into the angle,
                                   the velocity term and twice into the acceleration term
                                   (all taken at max(|t|, |dt|) in M)                               4
    |gyr|, gyr / |gyr|, angle      3 mul, 2 add, sqrt (<= 3 on the norm), 1 div, 1 mul: each K
                                   entry 4, the angle 4 + dt
    sin, cos                       the device library documents 2 ulp for double sin and cos
                                   (4 in these units), plus the angle's 4: s 8, 1 - cos 9
    Exp entries                    s K: 8 + 4 + 1; (c1 K) K: 9 + 2 * 4 + 5; two adds: 37 an entry,
                                   Frobenius norm of the 3 x 3 error <= 3 * 37                    111
    R_i = rot Exp                  3 x 3 product, 5 an entry, Frobenius 15                          15
    R_i a + T_ei                   product 6 + add 1                                                7
    T_ei                           6 roundings a component (mul, add, mul, mul, add, sub),
                                   sqrt(3) * 6 < 11                                                11
    extR_Ri = R_LI^T rot_end^T     5 an entry, Frobenius 15; the product with it 6                 21
    R_LI^T t_LI and the last sub   6 + 1                                                            7
                                                                                            K  =  190

rounded up to K = 192.  At M = 30 m the term is 1.3e-12 m against a half ulp of 1e-6 m: the bar
is "the correctly rounded float32 of the reference", loosened only within 1e-12 m of a tie.
First point, moved m times: m times the bar, ulp32 taken at the largest coordinate the chain
stores (a one-ulp difference after one move passes through the next rotation at unit norm).
Points never moved: bitwise.

VoxelGrid bar, per column of a voxel of n members:
    |x - c64| <= (adds + 1) 2^-24 (sum |x_i|) / n + 2^-150,
adds = ceil(n / 64) + 6 for the device (each lane sums its strided members in turn, then six
xor levels) and n - 1 for the CPU oracle (one running sum), the 1 the division.  2^-150 is the
division's rounding where the quotient is subnormal (half of 2^-149; float32 sums do not
underflow): the lattice holds nextafter(0), whose mean with a zero is no float32.  Integer tag
columns (sums below 2^24, exact in any order) must equal float32(sum) / float32(count) bit for
bit, which also pins the count.  Voxel set and order: exact.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np

import frontend_ref as fr

K_ROUNDINGS = 192
EPS64 = 2.0 ** -52
SIZES = (2, 63, 64, 65, 257, 4097, 70001)


def rot_axis_angle(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt((a * a).sum())
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = math.radians(deg)
    return np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)


# "ident": the extrinsics of every earlier front-end test; "tilt": 35 degrees about a tilted
# axis (orthonormal to double rounding: Rodrigues' formula), a lever arm of decimetres
EXTRINSICS = {
    "ident": (np.eye(3), np.array([0.04165, 0.02326, -0.0284])),
    "tilt": (rot_axis_angle([1.0, 2.0, 3.0], 35.0), np.array([0.31, -0.22, 0.17])),
}
assert np.abs(EXTRINSICS["tilt"][0] @ EXTRINSICS["tilt"][0].T - np.eye(3)).max() < 4e-16


class Frame(NamedTuple):
    raw: np.ndarray       # (n, 5) float32
    poses: np.ndarray     # (np, 22) float64
    rot_end: np.ndarray
    pos_end: np.ndarray


def offsets_s(ms):
    return np.asarray(ms, np.float32).astype(np.float64) / 1000.0


def pose_ms(n_poses=21, first=1.3, step=4.7):
    return (np.float32(first) + np.float32(step) * np.arange(n_poses, dtype=np.float32)).astype(np.float32)


def below(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def above(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def make_poses(ms, rng, rate=0.3, gyr=None, anchor=None):
    """Pose6D rows at offsets ms with per-pose jitter; rot_end 70 degrees or more from identity.
    gyr: one fixed rate for every pose.  anchor: a point a0 of the IMU frame; every pose is then
    placed so that a0 lands within centimetres of the origin of the end frame (the de-skewed
    coordinates are small, and a rotation by 1e-8 rad of a 10 m arm shows in float32)."""
    off = offsets_s(ms)
    m = len(off)
    R0 = rot_axis_angle(rng.normal(size=3), 70.0 + 40.0 * rng.uniform())
    w = rng.normal(size=3)
    w = rate * w / np.sqrt((w * w).sum())
    v = rng.normal(0, 0.05 if anchor is not None else 2.0, size=3)
    acc = rng.normal(0, 0.05 if anchor is not None else 1.0, size=3)
    p0 = rng.normal(0, 5.0, size=3)
    t_end = off[-1] + 0.005
    rot_end = R0 @ rot_axis_angle(w, math.degrees(rate * t_end)) @ rot_axis_angle(rng.normal(size=3), 0.5)
    pos_end = p0 + v * t_end
    poses = np.zeros((m, fr.POSE_D))
    for k in range(m):
        t = off[k]
        Rk = R0 @ rot_axis_angle(w, math.degrees(rate * t)) @ rot_axis_angle(rng.normal(size=3), 0.5)
        poses[k, 0] = t
        poses[k, 1:4] = acc + rng.normal(0, 0.5 if anchor is None else 0.01, size=3)
        poses[k, 4:7] = (w + rng.normal(0, 0.1, size=3)) if gyr is None else gyr
        poses[k, 7:10] = v + rng.normal(0, 0.5 if anchor is None else 0.01, size=3)
        poses[k, 13:22] = Rk.reshape(9)
        if anchor is None:
            poses[k, 10:13] = p0 + v * t + rng.normal(0, 0.02, size=3)
        else:
            poses[k, 10:13] = pos_end - Rk @ anchor + rng.normal(0, 0.01, size=3)
    return poses, rot_end, pos_end


def cloud(n, rng, t_ms):
    d = rng.normal(size=(n, 3))
    d /= np.sqrt((d * d).sum(1))[:, None]
    xyz = d * rng.uniform(2.0, 30.0, size=(n, 1))
    inten = rng.uniform(0, 255, size=(n, 1))
    return np.ascontiguousarray(np.concatenate([xyz, inten, np.asarray(t_ms, np.float64).reshape(n, 1)], 1),
                                np.float32)


def _seed(*key):
    return np.random.default_rng([0x5EED, *[sum(ord(c) * 131 ** i for i, c in enumerate(str(k))) % (2 ** 31) for k in key]])


# ---------------------------------------------------------------- de-skew: segment assignment ----
SEGMENT_KINDS = ("random", "early_last", "late_front", "stop_mid", "runs")


def segment_frame(kind, n):
    rng = _seed("segment", kind, n)
    ms = pose_ms()
    t = np.sort(rng.uniform(1.4, 99.0, size=n)).astype(np.float32)
    if kind == "random":
        t = rng.permutation(t)
    elif kind == "early_last":
        t[-1] = above(ms[0])  # pulls every earlier point down to head 0, dt up to 98 ms
    elif kind == "late_front":
        k = max(1, n // 4)
        t[:k] = rng.uniform(90.0, 99.0, size=k).astype(np.float32)
    elif kind == "stop_mid":
        t = rng.permutation(t)
        t[n // 2] = ms[0] if n % 2 else below(ms[0])  # time <= offset(0): the walk ends here
    elif kind == "runs":
        vals = []
        while len(vals) < n:
            vals += [np.float32(rng.uniform(1.4, 99.0))] * int(rng.integers(2, 201))
        t = np.array(vals[:n], np.float32)  # runs of equal times, the runs themselves unsorted
    poses, Re, pe = make_poses(ms, rng)
    return Frame(cloud(n, rng, t), poses, Re, pe)


# ------------------------------------------------------------------------- de-skew: boundaries ----
BOUNDARY_KINDS = ("exact_sorted", "exact_shuffled", "late", "two_poses", "equal2", "equal3", "all_before",
                  "offsets_below")


def boundary_frame(kind):
    rng = _seed("boundary", kind)
    ms = pose_ms()
    if kind in ("exact_sorted", "exact_shuffled"):
        # every pose k = 0 .. n_poses - 1: just below, exactly at and just above offset(k)
        t = np.array([f(x) for x in ms for f in (below, np.float32, above)], np.float32)
        if kind == "exact_shuffled":
            t = rng.permutation(t)
    elif kind == "late":
        t = rng.uniform(1.4, 130.0, size=200).astype(np.float32)  # a third later than the last pose (95.3 ms)
    elif kind == "two_poses":
        ms = np.array([1.3, 50.0], np.float32)
        t = rng.uniform(1.4, 99.0, size=150).astype(np.float32)
        t[::7] = [[below(50.0), np.float32(50.0), above(50.0)][i % 3] for i in range(len(t[::7]))]
    elif kind in ("equal2", "equal3"):
        reps = 2 if kind == "equal2" else 3
        at = 5 if kind == "equal2" else 9
        ms[at:at + reps] = ms[at]  # zero-length segments
        t = rng.uniform(1.4, 99.0, size=180).astype(np.float32)
        edge = [below(ms[at]), ms[at], above(ms[at]), below(ms[at + reps]), ms[at + reps], above(ms[at + reps])]
        t[::5] = [edge[i % 6] for i in range(len(t[::5]))]
    elif kind == "all_before":
        t = rng.uniform(0.0, 1.29, size=120).astype(np.float32)
        t[3] = ms[0]
    elif kind == "offsets_below":
        ms = pose_ms(21, 0.0, 0.1)
        t = rng.uniform(5.0, 99.0, size=150).astype(np.float32)
    poses, Re, pe = make_poses(ms, rng)
    return Frame(cloud(len(t), rng, t), poses, Re, pe)


# ------------------------------------------------------------------------ de-skew: first point ----
FIRST_MOVES = (1, 2, 8, 20)


def first_frame(m, n=100):
    """The first point lies after m segments; the later points, unsorted, all lie later still."""
    rng = _seed("first", m, n)
    ms = pose_ms()
    t0 = np.float32(ms[m - 1] + np.float32(2.0))
    t = rng.uniform(float(t0), 99.0, size=n).astype(np.float32)
    t[0] = t0
    poses, Re, pe = make_poses(ms, rng)
    return Frame(cloud(n, rng, t), poses, Re, pe)


# -------------------------------------------------------------------- de-skew: rotation branch ----
ROTATION_KINDS = ("gyr_zero", "gyr_0.9e-7", "gyr_1.1e-7", "gyr_3")


def rotation_frame(kind, ext):
    rng = _seed("rotation", kind)
    R_LI, t_LI = EXTRINSICS[ext]
    if kind == "gyr_3":
        ms = np.array([0.5, 250.0], np.float32)
        t = rng.uniform(0.6, 200.0, size=300).astype(np.float32)  # dt up to 0.2 s, angles up to 0.6 rad
        poses, Re, pe = make_poses(ms, rng, rate=3.0)
        return Frame(cloud(len(t), rng, t), poses, Re, pe)
    ms = pose_ms(5, 1.0, 50.0)
    t = rng.uniform(1.1, 240.0, size=300).astype(np.float32)
    u = np.array([2.0, -1.0, 2.0]) / 3.0
    gyr = {"gyr_zero": np.zeros(3), "gyr_0.9e-7": 0.9e-7 * u, "gyr_1.1e-7": 1.1e-7 * u}[kind]
    centre = np.array([9.0, -4.0, 2.5])
    raw = cloud(len(t), rng, t)
    raw[:, :3] = (centre + rng.uniform(-0.05, 0.05, size=(len(t), 3))).astype(np.float32)
    poses, Re, pe = make_poses(ms, rng, gyr=gyr, anchor=R_LI @ centre + t_LI)
    return Frame(raw, poses, Re, pe)


DESKEW_CASES = ([("segment", k, n) for k in SEGMENT_KINDS for n in SIZES] + [("boundary", k) for k in BOUNDARY_KINDS] +
                [("first", m) for m in FIRST_MOVES] + [("first", "single")] + [("rotation", k) for k in ROTATION_KINDS])


def case_id(case):
    return "-".join(str(x) for x in case)


@functools.lru_cache(maxsize=4)
def deskew_frame(case, ext):
    if case[0] == "segment":
        return segment_frame(case[1], case[2])
    if case[0] == "boundary":
        return boundary_frame(case[1])
    if case[0] == "first":
        return first_frame(9, 1) if case[1] == "single" else first_frame(case[1])
    return rotation_frame(case[1], ext)


class DeskewRef(NamedTuple):
    cloud: np.ndarray   # (n, 5) float32, frontend_ref.undistort
    last: np.ndarray    # (n, 3) float64
    heads: list
    bar: np.ndarray     # (n, 3): the bar on |x - last|, 0 for a point never moved
    moves: np.ndarray   # (n,) how often each point is moved


def _chain_scale(frame, heads0, R_LI, t_LI):
    """The first point's chain again: (largest stored coordinate, largest M)."""
    p = frame.raw[0:1, :3].copy()
    peak, M = float(np.abs(p).max()), 0.0
    for h in heads0:
        P, Mi = fr.compensate(p, frame.raw[0:1, 4], frame.poses[h:h + 1], frame.rot_end, frame.pos_end, R_LI, t_LI)
        p = P.astype(np.float32)
        peak, M = max(peak, float(np.abs(P).max())), max(M, float(Mi[0]))
    return peak, M


def deskew_reference(frame, ext, dev=None):
    """frontend_ref.undistort of the frame, the bar of every coordinate, and the assertion that
    the frame separates adjacent heads.  dev: the cloud under test (its coordinates enter
    ulp32(max(|x|, |ref64|)))."""
    R_LI, t_LI = EXTRINSICS[ext]
    raw, poses, Re, pe = frame
    cl, last, heads = fr.undistort(raw, poses, Re, pe, R_LI, t_LI)
    n = len(raw)
    moves = np.array([len(h) for h in heads], np.int64)
    bar = np.zeros((n, 3))
    idx = np.flatnonzero(moves > 0)
    if len(idx) == 0:
        return DeskewRef(cl, last, heads, bar, moves)
    h_last = np.array([heads[i][-1] for i in idx], np.int64)
    h_first = np.array([heads[i][0] for i in idx], np.int64)
    src = raw[idx, :3].copy()
    _, M = fr.compensate(src, raw[idx, 4], poses[h_first], Re, pe, R_LI, t_LI)
    mag = np.abs(last[idx])
    if dev is not None:
        mag = np.maximum(mag, np.abs(np.asarray(dev)[idx, :3].astype(np.float64)))
    bar[idx] = fr.ulp32(mag) / 2 + (K_ROUNDINGS * EPS64 * M)[:, None]
    if moves[0] > 1:
        peak, M0 = _chain_scale(frame, heads[0], R_LI, t_LI)
        if dev is not None:
            peak = max(peak, float(np.abs(np.asarray(dev)[0, :3]).max()))
        bar[0] = moves[0] * (fr.ulp32(peak) / 2 + K_ROUNDINGS * EPS64 * M0)
    # separation: the neighbouring heads would put the point at least 100 bars away.  (For the
    # first point: its first move, from the raw input.)
    right, _ = fr.compensate(src, raw[idx, 4], poses[h_first], Re, pe, R_LI, t_LI)
    one = fr.ulp32(np.abs(right)) / 2 + (K_ROUNDINGS * EPS64 * M)[:, None]
    for step in (-1, 1):
        alt = h_first + step
        ok = (alt >= 0) & (alt <= len(poses) - 2)
        if ok.any():
            other, _ = fr.compensate(src[ok], raw[idx[ok], 4], poses[alt[ok]], Re, pe, R_LI, t_LI)
            ratio = (np.abs(other - right[ok]) / one[ok]).max(1)
            assert ratio.min() >= 100.0, f"heads {step:+d} not separated: {ratio.min():.1f} bars at point " \
                                         f"{idx[ok][int(ratio.argmin())]}"
    return DeskewRef(cl, last, heads, bar, moves)


def check_deskew(got, frame, ref):
    """got against the reference: never-moved points bitwise, every other coordinate under its bar,
    the tag columns untouched.  Returns the largest error as a fraction of its bar."""
    got = np.asarray(got, np.float32)
    assert got.shape == frame.raw.shape
    assert np.array_equal(got[:, 3:].view(np.uint32), frame.raw[:, 3:].view(np.uint32))
    still = ref.moves == 0
    assert np.array_equal(got[still].view(np.uint32), frame.raw[still].view(np.uint32)), "an untouched point moved"
    moved = ~still
    if not moved.any():
        return 0.0
    err = np.abs(got[moved, :3].astype(np.float64) - ref.last[moved])
    frac = err / ref.bar[moved]
    worst = np.unravel_index(int(frac.argmax()), frac.shape)
    i = np.flatnonzero(moved)[worst[0]]
    assert frac.max() <= 1.0, (f"point {i} coordinate {worst[1]}: |{got[i, worst[1]]!r} - {ref.last[i, worst[1]]!r}| = "
                               f"{err[worst]:.3e} > bar {ref.bar[i, worst[1]]:.3e} (heads {ref.heads[i]})")
    return float(frac.max())


# ----------------------------------------------------------------------------------- VoxelGrid ----
def tagged(xyz):
    """(n, 5) float32 with integer tags in the intensity and curvature columns."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    i = np.arange(len(xyz))
    return np.ascontiguousarray(np.concatenate([xyz, (i % 251 + 1)[:, None].astype(np.float32),
                                                (i % 241 + 1)[:, None].astype(np.float32)], 1), np.float32)


VOXEL_CASES = ([("lattice", leaf) for leaf in (0.5, 0.1, 0.3)] + [("one_voxel", n) for n in (1, 63, 64, 65, 129, 5000)] +
               [("one_per_voxel", n) for n in (3, 4, 5, 1025)] + [("int32", "below"), ("int32", "above"),
                                                                  ("negative", 3000)])


@functools.lru_cache(maxsize=None)
def voxel_frame(case):
    """-> (raw (n, 5) float32 with tags, leaf)."""
    rng = _seed("voxel", *case)
    kind, arg = case
    if kind == "lattice":
        leaf = np.float32(arg)
        vals = [np.float32(-0.0), np.float32(0.0)]
        for j in range(-6, 7):
            b = np.float32(j) * leaf  # an exact multiple of the leaf in float32 arithmetic
            vals += [below(b), b, above(b)]
        vals = np.array(vals, np.float32)
        return tagged(vals[rng.integers(0, len(vals), size=(2000, 3))]), float(arg)
    if kind == "one_voxel":
        return tagged(rng.uniform(10.1, 10.4, size=(arg, 3))), 0.5
    if kind == "one_per_voxel":
        i = rng.permutation(arg)
        return tagged(np.stack([i + 0.25, (i * 7) % 5 + 0.25, np.full(arg, 0.25)], 1)), 0.5
    if kind == "int32":
        # leaf 1.0, corners at fractional part 0.25: 1290 x 1290 x 1290 = 2,146,689,000 cells (filtered,
        # leaf indices up to 31 bits) or 1290 x 1290 x 1291 = 2,148,353,100 (the input comes back)
        top = 644.25 if arg == "below" else 645.25
        xyz = rng.uniform(-3.0, 3.0, size=(60, 3))
        xyz[17] = [-644.75, -644.75, -644.75]
        xyz[41] = [644.25, 644.25, top]
        return tagged(xyz), 1.0
    if kind == "negative":
        return tagged(rng.uniform(-1003.0, -997.0, size=(arg, 3))), 0.5
    raise KeyError(case)


def check_voxels(got, raw, leaf, adds, tags=True):
    """got (k, 5) float32 against frontend_ref.voxel_grid(raw, leaf).  adds(n): the float32
    additions behind a voxel of n members.  Returns the largest x, y, z error over its bar."""
    v = fr.voxel_grid(raw, leaf)
    got = np.asarray(got, np.float32)
    assert got.shape == (len(v.count), 5), f"{got.shape[0]} voxels, reference {len(v.count)}"
    if not v.filtered:
        assert np.array_equal(got.view(np.uint32), raw.view(np.uint32)), "dx dy dz > INT32_MAX: input unchanged"
        return 0.0
    cols = 3 if tags else 5
    k = np.array([adds(int(c)) + 1 for c in v.count], np.float64)
    bar = (k * 2.0 ** -24)[:, None] * v.abs_sum[:, :cols] / v.count[:, None] + 2.0 ** -150
    err = np.abs(got[:, :cols].astype(np.float64) - v.centroid[:, :cols])
    # a voxel taken for its neighbour is off by a leaf, not by a rounding: set and order are exact
    assert (err <= bar).all(), f"voxel {int((err / np.maximum(bar, 1e-300)).max(1).argmax())}: error over bar " \
                               f"{(err / np.maximum(bar, 1e-300)).max():.3g}"
    if tags:
        for col in (3, 4):
            s = np.array([raw[m, col].astype(np.float64).sum() for m in v.members])
            assert s.max() < 2 ** 24
            want = s.astype(np.float32) / v.count.astype(np.float32)
            assert np.array_equal(got[:, col].view(np.uint32), want.view(np.uint32)), f"tag column {col}"
    nz = bar > 0
    return float((err[nz] / bar[nz]).max()) if nz.any() else 0.0


def device_adds(n):
    return -(-n // 64) + 6


def oracle_adds(n):
    return max(n - 1, 0)


# ------------------------------------------------------------------------------ resident scans ----
RESIDENT_KINDS = ("wide", "identical", "single")


def to_world_bar(pts, state, ext, dev):
    """-> (ref64 (n, 3), bar (n, 3)) of frontend_ref.to_world: the de-skew bar, M over the chain."""
    R_LI, t_LI = EXTRINSICS[ext]
    p = np.asarray(pts)[:, :3].astype(np.float64)
    ref = fr.to_world(pts, state, R_LI, t_LI)
    M = np.max(np.stack([_n(p), np.full(len(p), _n(t_LI)), _n(p @ R_LI.T + t_LI),
                         np.full(len(p), _n(state["pos"])), _n(ref)]), 0) if len(p) else np.zeros(0)
    mag = np.maximum(np.abs(ref), np.abs(np.asarray(dev)[:, :3].astype(np.float64)))
    return ref, fr.ulp32(mag) / 2 + (K_ROUNDINGS * EPS64 * M)[:, None]


def _n(v):
    return np.sqrt((np.asarray(v, np.float64) ** 2).sum(-1))
