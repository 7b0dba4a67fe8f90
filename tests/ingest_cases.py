"""The sensor handlers, the time sort and UndistortPcl's slice restated twice from the reference
(src/preprocess.cpp:315-349 avia, :424-453 oust64, :578-637 velodyne with point times, :650-680
xt32; src/laser_mapping.cpp:705; src/IMU_Processing.cpp:217-235), and the cases the tests run.

  *_scalar   a Python loop over the message in the reference's statement order, on numpy.float32 /
             float64 scalars (one rounding per operation, as the compiled float code).
  *_vector   the same results from whole-array expressions, a prefix count and a stable argsort.

Both order the frame by the float's order-preserving 32-bit key with ties in message order: one of
the outcomes std::sort may produce, and the one the device documents (-0.0 before +0.0).

A message is either a structured array of LIVOX (livox_ros_driver::CustomPoint, 20 B) or a
(n, point_step) uint8 array with a layout dict (point_step, off_x, off_y, off_z, off_intensity,
off_time).  A frame is (n_kept, 5) float32: x, y, z, intensity, curvature (ms).
"""
import functools
import struct

import numpy as np

F = np.float32
D = np.float64
AVIA, VELO16, OUST64, XT32 = 1, 2, 3, 4
LIVOX = np.dtype([("offset_time", np.uint32), ("x", np.float32), ("y", np.float32), ("z", np.float32),
                  ("reflectivity", np.uint8), ("tag", np.uint8), ("line", np.uint8), ("pad", np.uint8)])
TIME_FMT = {OUST64: "<I", VELO16: "<f", XT32: "<d"}
BLOCK = 256  # the ingest kernels' block size (kIngestBlock)


# ---------------------------------------------------------------- scalar ----
def _info(n, n_pass, frame):
    k = len(frame)
    return {"n_in": n, "n_kept": k, "cursor": 0, "n_rejected": n - n_pass, "n_decimated": n_pass - k,
            "end_curvature": F(frame[-1, 4]) if k else F(0)}


def _rows(rows):
    return np.array(rows, F).reshape(-1, 5)


def avia_scalar(msg, n_scans, filter_num, blind):
    rows, effect_ind = [], 0
    with np.errstate(all="ignore"):
        for i in range(1, len(msg)):
            x, y, z = F(msg["x"][i]), F(msg["y"][i]), F(msg["z"][i])
            rng = D(x * x + y * y)
            if (D(abs(x - F(msg["x"][i - 1]))) < 1e-8 or D(abs(y - F(msg["y"][i - 1]))) < 1e-8
                    or D(abs(z - F(msg["z"][i - 1]))) < 1e-8 or rng < blind or rng > 900
                    or int(msg["line"][i]) > n_scans or (int(msg["tag"][i]) & 0x30) != 0x10):
                continue
            effect_ind += 1
            if effect_ind % filter_num == 0:
                rows.append((x, y, z, np.sqrt(x * x + y * y + z * z), F(msg["offset_time"][i]) / F(1000000)))
    return _rows(rows), effect_ind


def cloud_scalar(kind, data, layout, filter_num, blind):
    rows, n_pass = [], 0
    buf = data.tobytes()
    ps = layout["point_step"]
    n = len(buf) // ps
    with np.errstate(all="ignore"):
        head = struct.unpack_from("<d", buf, layout["off_time"])[0] if kind == XT32 and n else 0.0
        for i in range(n):
            x, y, z = (F(struct.unpack_from("<f", buf, i * ps + layout[k])[0]) for k in ("off_x", "off_y", "off_z"))
            intensity = F(struct.unpack_from("<f", buf, i * ps + layout["off_intensity"])[0])
            t = struct.unpack_from(TIME_FMT[kind], buf, i * ps + layout["off_time"])[0]
            r2 = x * x + y * y + z * z
            if kind == OUST64:
                ok = not (D(r2) < D(blind) * D(blind))
                row = (x, y, z, np.sqrt(r2), F(np.uint32(t)) * F(1.e-6))
            elif kind == VELO16:
                ok = bool(D(r2) > D(blind) * D(blind))
                row = (x, y, z, intensity, F(t) * F(1.e-3))
            else:
                ok = bool(D(r2) > D(blind))
                row = (x, y, z, intensity, F((D(t) - D(head)) * D(F(1000))))
            n_pass += ok
            if i % filter_num == 0 and ok:
                rows.append(row)
    return _rows(rows), n_pass


def _key_scalar(c):
    u = int(np.array(c, F).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def sort_scalar(frame):
    keyed = [(_key_scalar(r[4]), r) for r in frame]
    keyed.sort(key=functools.cmp_to_key(lambda a, b: -1 if a[0] < b[0] else (1 if b[0] < a[0] else 0)))  # stable
    return _rows([r for _, r in keyed])


def ingest_scalar(kind, msg, layout=None, n_scans=16, filter_num=2, blind=0.01):
    """-> (the sorted frame, the info dict)."""
    if kind == AVIA:
        rows, n_pass = avia_scalar(msg, n_scans, filter_num, blind)
        n = len(msg)
    else:
        rows, n_pass = cloud_scalar(kind, msg, layout, filter_num, blind)
        n = msg.size // layout["point_step"]
    frame = sort_scalar(rows)
    return frame, _info(n, n_pass, frame)


def take_scalar(frame, cursor, limit_ms, is_lidar_end):
    """UndistortPcl :217-235 -> (n_taken, the cursor afterwards)."""
    k = cursor
    while k != len(frame) and D(frame[k, 4]) <= limit_ms:
        k += 1
    return k - cursor, (0 if is_lidar_end else k)


# ------------------------------------------------------------ vectorised ----
def _field(data, off, dt):
    return np.ascontiguousarray(data[:, off:off + np.dtype(dt).itemsize]).view(dt).reshape(-1)


def ingest_vector(kind, msg, layout=None, n_scans=16, filter_num=2, blind=0.01):
    with np.errstate(all="ignore"):
        if kind == AVIA:
            n = len(msg)
            x, y, z = msg["x"].astype(F), msg["y"].astype(F), msg["z"].astype(F)
            ok = np.zeros(n, bool)
            if n > 1:
                rng = (x * x + y * y).astype(D)[1:]
                dup = np.zeros(n - 1, bool)
                for a in (x, y, z):
                    dup |= np.abs(a[1:] - a[:-1]).astype(D) < 1e-8
                ok[1:] = ~(dup | (rng < blind) | (rng > 900) | (msg["line"][1:].astype(np.int64) > n_scans)
                           | ((msg["tag"][1:] & 0x30) != 0x10))
            e = np.cumsum(ok)
            keep = ok & (e % filter_num == 0)
            intensity = np.sqrt(x * x + y * y + z * z)
            curv = msg["offset_time"].astype(F) / F(1000000)
        else:
            data = msg.reshape(-1, layout["point_step"])
            n = data.shape[0]
            x, y, z = (_field(data, layout[k], F) for k in ("off_x", "off_y", "off_z"))
            r2 = x * x + y * y + z * z
            t = _field(data, layout["off_time"], {OUST64: np.uint32, VELO16: F, XT32: D}[kind])
            if kind == OUST64:
                ok = ~(r2.astype(D) < D(blind) * D(blind))
                intensity, curv = np.sqrt(r2), t.astype(F) * F(1.e-6)
            elif kind == VELO16:
                ok = r2.astype(D) > D(blind) * D(blind)
                intensity, curv = _field(data, layout["off_intensity"], F), t * F(1.e-3)
            else:
                ok = r2.astype(D) > D(blind)
                intensity = _field(data, layout["off_intensity"], F)
                curv = ((t - (t[0] if n else 0.0)) * D(F(1000))).astype(F)
            keep = ok & (np.arange(n) % filter_num == 0)
        rows = np.stack([x, y, z, intensity, curv], 1).astype(F)[keep]
    u = rows[:, 4].copy().view(np.uint32)
    keys = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000))
    frame = rows[np.argsort(keys, kind="stable")]
    return frame, _info(n, int(ok.sum()), frame)


def take_vector(frame, cursor, limit_ms, is_lidar_end):
    c = frame[cursor:, 4].astype(D)
    cnt = int(np.searchsorted(c, limit_ms, side="right")) if not np.isnan(limit_ms) else 0
    return cnt, (0 if is_lidar_end else cursor + cnt)


def take_limit(lidar_beg_time, end_curvature, is_lidar_end):
    """pcl_offset_time (:219-224): the scalar arithmetic the caller restates."""
    if not is_lidar_end:
        return 0.0
    pcl_end_time = D(lidar_beg_time) + D(end_curvature) / D(1000)
    return float((pcl_end_time - D(lidar_beg_time)) * D(1000))


# ------------------------------------------------------------------ cases ----
def livox_msg(n, density="half", times="random", seed=0, run=0):
    """A synthetic Avia message.  density: 'none' (every point fails the predicate), 'all', or 'half' (about
    half survive, in alternating runs of `run` points when run > 0, else at random).  times: 'sorted',
    'reversed', 'random' or 'ties' (equal offset times in runs of 100 points)."""
    rng = np.random.default_rng(seed)
    m = np.zeros(n, LIVOX)
    ang = rng.uniform(-np.pi, np.pi, n)
    rad = rng.uniform(1.0, 25.0, n)
    m["x"], m["y"], m["z"] = rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-3, 3, n)
    m["reflectivity"] = rng.integers(0, 256, n)
    m["line"] = rng.integers(0, 6, n)
    m["tag"] = 0x10 | rng.integers(0, 16, n).astype(np.uint8) | (rng.integers(0, 4, n).astype(np.uint8) << 6)
    bad = np.zeros(n, bool)
    if density == "none":
        bad[:] = True
    elif density == "half":
        bad = (np.arange(n) // run) % 2 == 1 if run > 0 else rng.random(n) < 0.5
    m["tag"][bad] &= 0xCF  # tag & 0x30 == 0: rejected
    t = np.sort(rng.integers(0, 100_000_000, n)).astype(np.uint32)
    if times == "reversed":
        t = t[::-1].copy()
    elif times == "random":
        t = rng.permutation(t)
    elif times == "ties":
        t = rng.permutation(np.arange(max((n + 99) // 100, 1), dtype=np.uint32) * 777_777)[np.arange(n) // 100]
    m["offset_time"] = t
    return m


LAYOUTS = {
    # the drivers' own layouts, and one of 48 bytes with the fields shuffled
    "ouster": {"point_step": 48, "off_x": 0, "off_y": 4, "off_z": 8, "off_intensity": 16, "off_time": 20},
    "velodyne": {"point_step": 22, "off_x": 0, "off_y": 4, "off_z": 8, "off_intensity": 12, "off_time": 18},
    "hesai": {"point_step": 32, "off_x": 0, "off_y": 4, "off_z": 8, "off_intensity": 12, "off_time": 16},
    "shuffled48": {"point_step": 48, "off_x": 36, "off_y": 4, "off_z": 20, "off_intensity": 44, "off_time": 8},
}


def cloud_msg(kind, n, layout, times="random", seed=0, blind=0.5, negative=False):
    """A synthetic PointCloud2 data block (n, point_step) uint8: random filler bytes around the fields; about a
    tenth of the points inside the blind zone.  negative (XT32): stamps before points[0]'s."""
    rng = np.random.default_rng(seed)
    ps = layout["point_step"]
    data = rng.integers(0, 256, (n, ps)).astype(np.uint8)
    rad = np.where(rng.random(n) < 0.1, rng.uniform(0.0, blind, n), rng.uniform(1.0, 40.0, n))
    v = rng.normal(size=(n, 3))
    xyz = (v / np.linalg.norm(v, axis=1, keepdims=True) * rad[:, None]).astype(F)
    t = np.sort(rng.uniform(0.0, 0.1, n))
    if times == "reversed":
        t = t[::-1].copy()
    elif times == "random":
        t = rng.permutation(t)
    elif times == "ties":
        t = (np.arange(n) // 100 % 7) * 0.01
    if kind == OUST64:
        tb = (t * 1e9).astype(np.uint32)
    elif kind == VELO16:
        tb = t.astype(F)
        if n:
            tb[-1] = max(tb[-1], F(1e-4))  # given_offset_time
    else:
        tb = 1.7e9 + t - (0.05 if negative else 0.0)
        if n and negative:
            tb[0] = 1.7e9
    for k, col in (("off_x", xyz[:, 0]), ("off_y", xyz[:, 1]), ("off_z", xyz[:, 2]),
                   ("off_intensity", rng.uniform(0, 255, n).astype(F)), ("off_time", tb)):
        b = np.ascontiguousarray(col).view(np.uint8).reshape(n, col.dtype.itemsize)
        data[:, layout[k]:layout[k] + b.shape[1]] = b
    return data


SIZES = (0, 1, 2, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 17)
