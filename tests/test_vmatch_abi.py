"""CPU checks of the resident visual map (livo_vmap_*) and livo_vio_match
(LidarSelector::addFromSparseMap, src/lidar_selection.cpp:332-593): the entry points are declared,
exported and bound at ABI version 9, their structures agree between C and ctypes, a null context
comes back as a code, and the per-item arithmetic of the kernels (csrc/vmap_model.h, compiled for
the host by tests/native/vmatch_point_check.cpp) equals, value for value, the restatement below.

The restatement is written from the contract: Python floats are IEEE doubles and
numpy float32 scalars IEEE singles, one rounding per operation, every 3-term sum left to right; no
`@`, no BLAS, no call into the library.  MapModel mirrors the map's entry points and restates the
whole call; tests/test_gpu_vmatch.py compares the device with it byte for byte.  Scene renders the
images the GPU cases use (a textured wall and a foreground board) and gives their clouds.
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
from test_rgb_cloud_abi import restate_pose
from test_vis_select_abi import REC_DTYPE, SMALL, restate_patch, restate_voxel, restate_w2c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "livo.h")
F32, F64 = np.float32, np.float64

MATCH_DTYPE = np.dtype([("point_id", np.int32), ("cell", np.int32), ("obs_index", np.int32), ("frame_id", np.int32),
                        ("search_level", np.int32), ("error", F32), ("ncc", F64), ("u", F64), ("v", F64)])
STAT_FIELDS = ("n_in", "n_voxels", "map_tested", "in_frame", "cell_overflow", "cells_marked", "depth_rejected",
               "view_rejected", "ncc_rejected", "error_rejected", "warp_shared", "warp_nan", "n_out")
MAX_OBS = 20


# ------------------------------------------------------------ restatement ----
def norm3(v):
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def frame_pos(Rcw, Pcw):
    """-Rcw^T Pcw."""
    return [-((Rcw[0][k] * Pcw[0] + Rcw[1][k] * Pcw[1]) + Rcw[2][k] * Pcw[2]) for k in range(3)]


def w2f(R, P, p):
    return [((R[k][0] * p[0] + R[k][1] * p[1]) + R[k][2] * p[2]) + P[k] for k in range(3)]


def w2c(cam, pf):
    """vikit's undistorted world2cam: fx * (x / z) + cx."""
    with np.errstate(all="ignore"):
        u, v = F64(pf[0]) / F64(pf[2]), F64(pf[1]) / F64(pf[2])
    return [float(cam["fx"] * u + cam["cx"]), float(cam["fy"] * v + cam["cy"])]


def cam2world(cam, u, v):
    x, y = (u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"]
    n = math.sqrt((x * x + y * y) + 1.0)
    return [x / n, y / n, 1.0 / n]


def in_frame(cam, border, px):
    return px[0] >= border and px[0] < cam["width"] - border and px[1] >= border and px[1] < cam["height"] - border


def pylist(a):
    return [[float(x) for x in r] for r in np.asarray(a, F64).reshape(3, 3)]


def warp_matrix(cam, Rc, Pc, Rr, Pr, ref_pos, px, f, pos, half):
    """getWarpMatrixAffine at level_ref = pyramid_level = 0: A row-major (a00, a01, a10, a11)."""
    depth_ref = norm3([ref_pos[k] - pos[k] for k in range(3)])
    R = [[(Rc[i][0] * Rr[j][0] + Rc[i][1] * Rr[j][1]) + Rc[i][2] * Rr[j][2] for j in range(3)] for i in range(3)]
    t = [Pc[i] - ((R[i][0] * Pr[0] + R[i][1] * Pr[1]) + R[i][2] * Pr[2]) for i in range(3)]
    x = [[f[k] * depth_ref for k in range(3)], cam2world(cam, px[0] + float(half), px[1]),
         cam2world(cam, px[0], px[1] + float(half))]
    with np.errstate(all="ignore"):
        for m in (1, 2):
            s = float(F64(x[0][2]) / F64(x[m][2]))
            x[m] = [float(F64(x[m][k]) * F64(s)) for k in range(3)]
        p = [w2c(cam, w2f(R, t, x[m])) for m in range(3)]
        h = F64(half)
        return [float((F64(p[1][0]) - F64(p[0][0])) / h), float((F64(p[2][0]) - F64(p[0][0])) / h),
                float((F64(p[1][1]) - F64(p[0][1])) / h), float((F64(p[2][1]) - F64(p[0][1])) / h)]


def det2(A):
    with np.errstate(all="ignore"):
        return float(F64(A[0]) * F64(A[3]) - F64(A[2]) * F64(A[1]))


def search_level(A, max_level=2):
    level, D = 0, det2(A)
    while D > 3.0 and level < max_level:
        level += 1
        D *= 0.25
    return level


def inverse2f(A):
    with np.errstate(all="ignore"):
        inv = F64(1.0) / F64(det2(A))
        return [F32(F64(A[3]) * inv), F32(-F64(A[1]) * inv), F32(-F64(A[2]) * inv), F32(F64(A[0]) * inv)]


def warp_sample(Ai, px_ref, level, ps, e, img, w11_as_product=False):
    """One value of warpAffine, element e = y * ps + x, from the observation's own image."""
    h, w = img.shape
    half, y = ps // 2, e // ps
    x = e - y * ps
    sc = F32(1 << level)
    qx, qy = F32(x - half) * sc, F32(y - half) * sc
    with np.errstate(all="ignore"):
        u = (Ai[0] * qx + Ai[1] * qy) + F32(px_ref[0])
        v = (Ai[2] * qx + Ai[3] * qy) + F32(px_ref[1])
    assert u.dtype == F32 and v.dtype == F32
    if u < 0 or v < 0 or u >= F32(w - 1) or v >= F32(h - 1) or u != u or v != v:
        return F32(0.0)
    xi, yi = int(math.floor(u)), int(math.floor(v))
    sx, sy = u - F32(xi), v - F32(yi)
    one = F32(1.0)
    w00, w01, w10 = (one - sx) * (one - sy), (one - sx) * sy, sx * (one - sy)
    w11 = sx * sy if w11_as_product else ((one - w00) - w01) - w10
    val = ((w00 * F32(img[yi, xi]) + w01 * F32(img[yi + 1, xi])) + w10 * F32(img[yi, xi + 1])) + \
        w11 * F32(img[yi + 1, xi + 1])
    assert val.dtype == F32
    return val


def ncc(ref, cur):
    n = len(ref)
    sum_ref = 0.0
    for v in ref:
        sum_ref += float(v)
    mean_ref = sum_ref / n
    sum_cur = 0.0
    for v in cur:
        sum_cur += float(v)
    mean_cur = sum_cur / n
    num = den1 = den2 = 0.0
    for i in range(n):
        a, b = float(ref[i]) - mean_ref, float(cur[i]) - mean_cur
        num += a * b
        den1 += a * a
        den2 += b * b
    return num / math.sqrt(den1 * den2 + 1e-10)


def patch_error(ref, cur):
    e = F32(0.0)
    for i in range(len(ref)):
        d = F32(ref[i]) - F32(cur[i])
        e = e + d * d
    assert e.dtype == F32
    return e


def close_view(fpos, pos, ref_positions):
    """getCloseViewObs: (index, cosine) of the first observation of the strictly greatest cosine above 0."""
    with np.errstate(all="ignore"):
        o = [F64(fpos[k] - pos[k]) for k in range(3)]
        on = F64(norm3([float(v) for v in o]))
        o = [v / on for v in o]
        best, cosine = 0, 0.0
        for i, rp in enumerate(ref_positions):
            d = [F64(rp[k] - pos[k]) for k in range(3)]
            dn = F64(norm3([float(v) for v in d]))
            d = [v / dn for v in d]
            c = float((o[0] * d[0] + o[1] * d[1]) + o[2] * d[2])
            if c > cosine:
                best, cosine = i, c
    return best, cosine


def floor_keys(world):
    """floor(p / 0.5) per axis of float32 points, as int64 (n, 3)."""
    return np.floor(np.asarray(world, F32).astype(F64) / F64(0.5)).astype(np.int64)


class MapModel:
    """The resident visual map and the whole of livo_vio_match, restated."""

    def __init__(self, cam, ps):
        self.cam, self.ps = cam, ps
        self.points, self.frames = [], {}

    def add_frame(self, fid, Rcw, Pcw, img):
        R, P = pylist(Rcw), [float(x) for x in Pcw]
        self.frames[fid] = {"R": R, "P": P, "pos": frame_pos(R, P), "img": np.ascontiguousarray(img, np.uint8)}

    def add(self, fid, pts, patches, point_ids=None, levels=None):
        assert fid in self.frames
        ids = []
        for i, r in enumerate(pts):
            u, v = float(r["u"]), float(r["v"])
            ob = {"frame_id": fid, "level": 0 if point_ids is None or levels is None else int(levels[i]),
                  "px": [u, v], "f": cam2world(self.cam, u, v), "patch": np.array(patches[i], F32).reshape(-1)}
            if point_ids is None:
                self.points.append({"pos": [float(r["x"]), float(r["y"]), float(r["z"])], "value": F32(r["score"]),
                                    "voxel": tuple(int(k) for k in r["voxel"]), "obs": [ob]})
                ids.append(len(self.points) - 1)
            else:
                assert len(self.points[point_ids[i]]["obs"]) < MAX_OBS
                self.points[point_ids[i]]["obs"].append(ob)
                ids.append(int(point_ids[i]))
        return np.asarray(ids, np.int32)

    def dump(self):
        pst3 = 3 * self.ps * self.ps
        n_obs = sum(len(p["obs"]) for p in self.points)
        pts = np.zeros(len(self.points), [("pos", F64, (3,)), ("value", F32), ("n_obs", np.int32),
                                          ("voxel", np.int64, (3,)), ("first_obs", np.int64)])
        obs = np.zeros(n_obs, [("frame_id", np.int32), ("level", np.int32), ("px", F64, (2,)), ("f", F64, (3,))])
        pat = np.zeros((n_obs, pst3), F32)
        at = 0
        for i, p in enumerate(self.points):
            pts[i] = (p["pos"], p["value"], len(p["obs"]), p["voxel"], at)
            for o in p["obs"]:
                obs[at] = (o["frame_id"], o["level"], o["px"], o["f"])
                pat[at] = o["patch"]
                at += 1
        return pts, obs, pat

    def match(self, world, Rcw, Pcw, img, grid, ncc_en=False, ncc_thre=0.0, outlier=100.0, store=True, quirk=True):
        """-> records (MATCH_DTYPE), pos (n, 3), levels (n), patches (n, 3 ps^2), stats, info."""
        cam, ps = self.cam, self.ps
        h, w = img.shape
        assert (w, h) == (cam["width"], cam["height"]) and ps % 2 == 0
        half, pst, border = ps // 2, ps * ps, (ps // 2 + 1) * 8
        gnh = h // grid
        length = (w // grid) * gnh
        world = np.ascontiguousarray(world, F32).reshape(-1, 3)
        stats = dict.fromkeys(STAT_FIELDS, 0)
        stats["n_in"] = len(world)
        empty = (np.zeros(0, MATCH_DTYPE), np.zeros((0, 3), F64), np.zeros(0, np.int32), np.zeros((0, 3 * pst), F32))
        if not self.points:
            return empty + (stats, {})
        R, P = pylist(Rcw), [float(x) for x in Pcw]
        fpos = frame_pos(R, P)
        # the cloud pass: the voxel set, the depth image (the last cloud index on a pixel wins)
        vset = set(map(tuple, floor_keys(world).tolist()))
        stats["n_voxels"] = len(vset)
        depth = np.zeros(w * h, F32)
        if len(world):
            x, y, z = (world[:, k].astype(F64) for k in range(3))
            pf = [((R[k][0] * x + R[k][1] * y) + R[k][2] * z) + P[k] for k in range(3)]
            with np.errstate(all="ignore"):
                px = F64(cam["fx"]) * pf[0] / pf[2] + F64(cam["cx"])
                py = F64(cam["fy"]) * pf[1] / pf[2] + F64(cam["cy"])
                hit = (pf[2] > 0) & (px >= border) & (px < w - border) & (py >= border) & (py < h - border)
            idx = np.flatnonzero(hit)
            pix = py[idx].astype(np.int64) * w + px[idx].astype(np.int64)
            last = np.full(w * h, -1, np.int64)
            np.maximum.at(last, pix, idx)
            depth = np.where(last >= 0, pf[2].astype(F32)[np.maximum(last, 0)], F32(0.0))
        # the map pass: every cell's nearest point, the greatest id among equals
        marked, cell_pt, cell_dist = set(), {}, {}
        for i, pt in enumerate(self.points):
            if pt["voxel"] not in vset:
                continue
            stats["map_tested"] += 1
            pf = w2f(R, P, pt["pos"])
            if pf[2] < 0:
                continue
            pc = w2c(cam, pf)
            if not in_frame(cam, border, pc):
                continue
            stats["in_frame"] += 1
            index = int(pc[0] / float(grid)) * gnh + int(pc[1] / float(grid))
            if index >= length:
                stats["cell_overflow"] += 1
                continue
            marked.add(index)
            dist = F32(norm3([fpos[k] - pt["pos"][k] for k in range(3)]))
            if dist <= F32(10000.0) and dist <= cell_dist.get(index, F32(10000.0)):
                cell_dist[index], cell_pt[index] = dist, i
        stats["cells_marked"] = len(marked)
        recs, poss, levs, pats, warp_of = [], [], [], [], {}
        info = {"levels_at_warp": [], "zero_samples": 0, "own_levels": []}
        for c in sorted(cell_pt):
            i = cell_pt[c]
            pt = self.points[i]
            pf = w2f(R, P, pt["pos"])
            pc = w2c(cam, pf)
            u0, v0 = int(pc[0]), int(pc[1])
            if any(depth[(v + v0) * w + u + u0] != 0 and abs(pf[2] - float(depth[(v + v0) * w + u + u0])) > 1.5
                   for u in range(-half, half + 1) for v in range(-half, half + 1) if (u, v) != (0, 0)):
                stats["depth_rejected"] += 1
                continue
            k, cosine = close_view(fpos, pt["pos"], [self.frames[o["frame_id"]]["pos"] for o in pt["obs"]])
            if cosine < 0.5:
                stats["view_rejected"] += 1
                continue
            ob = pt["obs"][k]
            fr = self.frames[ob["frame_id"]]
            A = warp_matrix(cam, R, P, fr["R"], fr["P"], fr["pos"], ob["px"], ob["f"], pt["pos"], half)
            own = (search_level(A), A)
            info["own_levels"].append(own[0])
            if quirk and ob["frame_id"] in warp_of:  # Warp_map: keyed by the reference frame id
                level, A = warp_of[ob["frame_id"]]
                stats["warp_shared"] += 1
            else:
                level, A = own
                warp_of[ob["frame_id"]] = own
            info["levels_at_warp"].append(level)
            Ai = inverse2f(A)
            if Ai[0] != Ai[0]:
                stats["warp_nan"] += 1
                ref = ob["patch"][:pst].copy()
            else:
                ref = np.array([warp_sample(Ai, ob["px"], level, ps, e, fr["img"]) for e in range(pst)], F32)
                info["zero_samples"] += int(np.sum(ref == 0))
                if store:
                    ob["patch"][:pst] = ref
            cur = restate_patch(img, [pc[0]], [pc[1]], ps)[0, :pst]
            val = 0.0
            if ncc_en:
                val = ncc(ref, cur)
                if val < ncc_thre:
                    stats["ncc_rejected"] += 1
                    continue
            err = patch_error(ref, cur)
            if float(err) > outlier * float(pst):
                stats["error_rejected"] += 1
                continue
            recs.append((i, c, k, ob["frame_id"], level, err, val, pc[0], pc[1]))
            poss.append(pt["pos"])
            levs.append(level)
            pats.append(np.concatenate([ref, ob["patch"][pst:]]))
        stats["n_out"] = len(recs)
        if not recs:
            return empty + (stats, info)
        return (np.array(recs, MATCH_DTYPE), np.array(poss, F64), np.array(levs, np.int32), np.array(pats, F32),
                stats, info)


# ------------------------------------------------------------------ scene ----
def small_cam(w=160, h=128):
    return dict(SMALL, width=w, height=h, cy=h / 2 - 0.4)


class Scene:
    """A textured wall 6 m in front of the pose `base`, and a board 2 m in front of its left half.  render()
    gives the gray image of a state, cloud() points on the surfaces as a body-frame cloud of a state."""

    def __init__(self, base, cam, seed=11, board=True, wall_z=6.0):
        from livo_amd import synth
        self.cam, self.synth = cam, synth
        Rcw, Pcw = restate_pose(synth.R_CI, synth.P_CI, base["rot"], base["pos"])
        self.Rwc, self.o = Rcw.T, -Rcw.T @ Pcw  # camera axes and centre of the base pose, in the world
        rng = np.random.default_rng(seed)
        self.tex = [synth._texture(640, 512, rng).astype(F64), 255.0 - synth._texture(640, 512, rng).astype(F64)]
        self.planes = [(wall_z - 2.0, (-50.0, -0.3)), (wall_z, (-1e9, 1e9))] if board else [(wall_z, (-1e9, 1e9))]

    def _hit(self, o, d):
        """Rays (world origin o, directions d (n, 3)) -> world hit points and the surface hit (0 board, 1 wall)."""
        oc, dc = (o - self.o) @ self.Rwc, d @ self.Rwc  # in the base camera's axes: the planes are z = const
        best = np.full(len(d), np.inf)
        which = np.full(len(d), len(self.planes) - 1)
        for k, (z, (x0, x1)) in enumerate(self.planes):
            t = (z - oc[2]) / dc[:, 2]
            x = oc[0] + t * dc[:, 0]
            ok = (t > 0) & (x >= x0) & (x < x1) & (t < best)
            best, which = np.where(ok, t, best), np.where(ok, k, which)
        return o + best[:, None] * d, which

    def _pixels(self, state, u, v):
        Rcw, Pcw = restate_pose(self.synth.R_CI, self.synth.P_CI, state["rot"], state["pos"])
        d = np.stack([(u - self.cam["cx"]) / self.cam["fx"], (v - self.cam["cy"]) / self.cam["fy"], np.ones_like(u)], 1)
        return self._hit(-Rcw.T @ Pcw, d @ Rcw)

    def render(self, state):
        w, h = self.cam["width"], self.cam["height"]
        vv, uu = np.mgrid[0:h, 0:w].astype(F64)
        hit, which = self._pixels(state, uu.ravel(), vv.ravel())
        q = (hit - self.o) @ self.Rwc
        a, b = q[:, 0] * 40.0 + 320.0, q[:, 1] * 40.0 + 256.0
        a0, b0 = np.floor(a), np.floor(b)
        sa, sb = a - a0, b - b0
        ia, ib = a0.astype(np.int64), b0.astype(np.int64)
        out = np.zeros(len(a))
        for k in range(len(self.tex)):
            T = self.tex[k]
            g = lambda di, dj: T[(ib + dj) % 512, (ia + di) % 640]  # noqa: E731
            val = (1 - sa) * (1 - sb) * g(0, 0) + sa * (1 - sb) * g(1, 0) + (1 - sa) * sb * g(0, 1) + sa * sb * g(1, 1)
            out = np.where(which == (k if len(self.planes) == 2 else 1 - k), val, out)
        return np.clip(np.rint(out), 0, 255).astype(np.uint8).reshape(h, w)

    def cloud(self, state, n, seed, margin=0.1, R_LI=None, t_LI=None):
        """n body-frame points (float32) of `state` on the surfaces seen through random pixels of its image."""
        rng = np.random.default_rng(seed)
        w, h = self.cam["width"], self.cam["height"]
        hit, _ = self._pixels(state, rng.uniform(-margin * w, (1 + margin) * w, n),
                              rng.uniform(-margin * h, (1 + margin) * h, n))
        return self.body(state, hit, R_LI, t_LI)

    def body(self, state, world, R_LI=None, t_LI=None):
        """World points in the LiDAR frame of `state`: R_LI^T (R^T (p_w - p) - t_LI); by default synth's
        extrinsic (R_LI = I, t_LI = synth.T_LI)."""
        imu = (np.asarray(world) - state["pos"]) @ state["rot"] - (self.synth.T_LI if t_LI is None else np.asarray(t_LI))
        if R_LI is not None:
            imu = imu @ np.asarray(R_LI, F64)
        return np.ascontiguousarray(imu, F32)


def moved(state, dpos, drot_deg=(0.0, 0.0, 0.0)):
    """`state` moved by dpos (world, m) and rotated by drot_deg (a rotation vector, degrees)."""
    from livo_amd import synth
    out = dict(state)
    out["pos"] = np.asarray(state["pos"], F64) + np.asarray(dpos, F64)
    out["rot"] = np.asarray(state["rot"], F64) @ synth.so3_exp(np.deg2rad(np.asarray(drot_deg, F64)))
    return out


def fabricate(world, cam, Rcw, Pcw, img, ps, sample=True):
    """livo_vis_point records and patches of float32 world points seen in a frame, as livo_vio_select would
    write them (the score is the point's index; sample=False: zero patches, for pixels outside the border)."""
    world = np.ascontiguousarray(world, F32).reshape(-1, 3)
    _, px, py = restate_w2c(world, cam, Rcw, Pcw)
    rec = np.zeros(len(world), REC_DTYPE)
    rec["x"], rec["y"], rec["z"] = world[:, 0], world[:, 1], world[:, 2]
    rec["score"] = np.arange(len(world)) + 1
    rec["u"], rec["v"] = px, py
    rec["src_index"], rec["cell"] = np.arange(len(world)), -1
    for k in range(3):
        rec["voxel"][:, k] = restate_voxel(world[:, k])
    pat = restate_patch(img, px, py, ps) if sample else np.zeros((len(world), 3 * ps * ps), F32)
    return rec, pat


# ----------------------------------------------------------- native cases ----
def hx(*vals):
    return " ".join(float(v).hex() for a in vals for v in np.asarray(a, F64).reshape(-1))


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    d = tmp_path_factory.mktemp("vmatch_native")
    exe = d / "vmatch_point_check"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "fast-livo-noted_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "vmatch_point_check.cpp"), "-o", str(exe)])

    def run(lines):
        path = d / "cases.txt"
        path.write_text("\n".join(lines) + "\n")
        out = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
        rows = [ln.split() for ln in out.stdout.split("\n") if ln]
        assert len(rows) == len(lines)
        return [[t if re.fullmatch(r"-?\d+", t) else float.fromhex(t) if "x" in t or "n" in t else t
                 for t in r[1:]] for r in rows]

    run.dir = d
    return run


def same(a, b):
    a, b = np.asarray(a, F64).reshape(-1), np.asarray(b, F64).reshape(-1)
    return a.shape == b.shape and a.tobytes() == b.tobytes() or \
        (a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]))


EYE = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


def test_warp_matrix_levels_and_nan_inverse(native):
    """A for a pure translation toward the wall that halves the depth, and halves it again: determinants
    about 4 and 16, levels 1 and 2; general poses; the NaN inverse of a point at its frame's centre."""
    cam = small_cam()
    rng = np.random.default_rng(5)
    cases = []
    for ref_z in (-6.0, -18.0):  # the current camera at the origin, a wall point at z = 6: depths 12 and 24
        cases.append((EYE, [0.0, 0.0, 0.0], EYE, [0.0, 0.0, -ref_z], [70.3, 60.9], [0.4, -0.2, 6.0]))
    from livo_amd import synth
    for _ in range(40):
        Rc, Rr = (synth.so3_exp(rng.normal(0, 0.05, 3)) for _ in range(2))
        cases.append((Rc, rng.normal(0, 0.2, 3), Rr, rng.normal(0, 0.5, 3), rng.uniform(24, 100, 2),
                      np.append(rng.normal(0, 1.5, 2), rng.uniform(3, 9))))
    cases.append((EYE, [0.0, 0.0, 0.0], EYE, [0.0, 0.0, 0.0], [70.0, 60.0], [0.0, 0.0, 0.0]))  # depth_ref = 0
    lines = ["A " + hx(cam["fx"], cam["fy"], cam["cx"], cam["cy"], Rc, Pc, Rr, Pr, px, pos) + " 2"
             for Rc, Pc, Rr, Pr, px, pos in cases]
    got = native(lines)
    dets, levels = [], []
    for (Rc, Pc, Rr, Pr, px, pos), g in zip(cases, got):
        Rc, Rr, Pc, Pr = pylist(Rc), pylist(Rr), [float(v) for v in Pc], [float(v) for v in Pr]
        px, pos = [float(v) for v in px], [float(v) for v in pos]
        rp = frame_pos(Rr, Pr)
        f = cam2world(cam, px[0], px[1])
        A = warp_matrix(cam, Rc, Pc, Rr, Pr, rp, px, f, pos, 2)
        want = f + A + [det2(A), str(search_level(A))] + [float(v) for v in inverse2f(A)] + rp
        assert [str(x) if isinstance(x, str) else None for x in g][8] == want[8]
        assert same([x for k, x in enumerate(g) if k != 8], [x for k, x in enumerate(want) if k != 8]), (g, want)
        dets.append(det2(A))
        levels.append(search_level(A))
    assert 3.5 < dets[0] < 4.5 and levels[0] == 1 and 14.0 < dets[1] < 18.0 and levels[1] == 2
    assert np.isnan(got[-1][9]) and np.isnan(float(inverse2f([float("nan")] * 4)[0]))
    assert set(levels[2:-1]) >= {0}


def test_search_level_boundary(native):
    up = float(np.nextafter(F64(3.0), F64(4.0)))
    As = [[3.0, 0.0, 0.0, 1.0], [up, 0.0, 0.0, 1.0], [12.0, 0.0, 0.0, 1.0], [4.0 * up, 0.0, 0.0, 1.0],
          [100.0, 0.0, 0.0, 1.0], [-5.0, 0.0, 0.0, 1.0], [0.0, 2.0, 2.0, 0.0]]
    got = [int(r[0]) for r in native(["L " + hx(A) for A in As])]
    assert got == [search_level(A) for A in As] == [0, 1, 1, 2, 2, 0, 0]


def test_warped_samples_bounds_and_weights(native):
    """A sample on each side of each of the four image bounds, fractional positions (w11 = 1 - w00 - w01 - w10,
    which differs from sx * sy on some of them), every level, a NaN position."""
    from livo_amd import synth
    w, h = 160, 128
    img = synth._texture(w, h, np.random.default_rng(3))
    path = native.dir / "img.bin"
    path.write_bytes(img.tobytes())
    eye = [1.0, 0.0, 0.0, 1.0]
    below = lambda x: float(np.nextafter(F32(x), F32(-1e9)))  # noqa: E731
    cases = []  # (Ai, px_ref, level, ps, e); e = 10: x = y = 0 offset for ps = 4 (x - half = 0)
    for px in ([0.0, 50.0], [below(0.0), 50.0], [50.0, 0.0], [50.0, below(0.0)], [below(w - 1), 50.0],
               [float(w - 1), 50.0], [50.0, below(h - 1)], [50.0, float(h - 1)], [float("nan"), 50.0]):
        cases.append((eye, px, 0, 4, 10))
    rng = np.random.default_rng(9)
    for _ in range(300):
        Ai = [float(F32(v)) for v in (rng.normal(1, 0.2), rng.normal(0, 0.2), rng.normal(0, 0.2), rng.normal(1, 0.2))]
        ps = int(rng.choice([4, 8]))
        cases.append((Ai, rng.uniform(-4, [w + 4, h + 4]), int(rng.integers(0, 3)), ps, int(rng.integers(0, ps * ps))))
    got = native([f"I {w} {h} {path}"] + ["S " + hx(Ai, px) + f" {lv} {ps} {e}" for Ai, px, lv, ps, e in cases])[1:]
    want = [warp_sample([F32(a) for a in Ai], px, lv, ps, e, img) for Ai, px, lv, ps, e in cases]
    assert same([g[0] for g in got], [float(v) for v in want])
    edge = [float(v) for v in want[:9]]
    assert [v == 0 for v in edge] == [False, True, False, True, False, True, False, True, True]
    other = [warp_sample([F32(a) for a in Ai], px, lv, ps, e, img, w11_as_product=True) for Ai, px, lv, ps, e in cases]
    assert sum(float(a) != float(b) for a, b in zip(want, other)) >= 10
    assert sum(float(v) == 0 for v in want[9:]) >= 5 and sum(float(v) > 0 for v in want[9:]) >= 200


def test_ncc_and_error(native):
    """NCC in double and the float error in index order; a constant patch, where the 1e-10 term decides."""
    rng = np.random.default_rng(2)
    cases = [(np.full(16, 97.0, F32), rng.uniform(0, 255, 16).astype(F32)), (np.full(16, 97.0, F32), np.full(16, 97.0, F32)),
             (np.zeros(64, F32), np.zeros(64, F32))]
    for n in (16, 64, 16, 64, 4):
        a = rng.uniform(0, 255, n).astype(F32)
        cases.append((a, (a + rng.normal(0, 6, n)).astype(F32)))
    got = native([f"N {hx(len(a))} " + hx(a) + " " + hx(b) for a, b in cases])
    for (a, b), g in zip(cases, got):
        assert same(g, [ncc(a, b), float(patch_error(a, b))])
    assert got[0][0] == 0.0 and got[1][0] == 0.0 and got[3][0] > 0.9


def test_cloud_point_order_and_keys(native):
    """fx * x / z + cx against world2cam's fx * (x / z) + cx on points where they differ in the last bit; the
    depth pixel; the keys of x = -1.0: AddPoint's -3, floor's -2."""
    from livo_amd import synth
    cam = small_cam()
    st = synth.make_state(3)
    Rcw, Pcw = restate_pose(synth.R_CI, synth.P_CI, st["rot"], st["pos"])
    R, P = pylist(Rcw), [float(v) for v in Pcw]
    rng = np.random.default_rng(4)
    sc = Scene(st, cam, board=False)
    world = (sc.body(st, sc._pixels(st, rng.uniform(0, 160, 400), rng.uniform(0, 128, 400))[0]).astype(F64) +
             synth.T_LI) @ st["rot"].T + st["pos"]
    world = np.concatenate([world.astype(F32), -world[:20].astype(F32)])
    got = native(["C " + hx(cam["fx"], cam["fy"], cam["cx"], cam["cy"], 160, 128, 24, Rcw, Pcw, p) for p in world])
    differ = hits = 0
    for p, g in zip(world, got):
        pw = [float(v) for v in p]
        pf = w2f(R, P, pw)
        keys = [int(math.floor(v / 0.5)) for v in pw]
        a = cam["fx"] * pf[0] / pf[2] + cam["cx"]
        b = cam["fy"] * pf[1] / pf[2] + cam["cy"]
        hit = pf[2] > 0 and in_frame(cam, 24, [a, b])
        assert [int(x) for x in g[:4]] == keys + [int(hit)]
        if hit:
            assert int(g[4]) == int(b) * 160 + int(a) and same(g[5], float(F32(pf[2])))
        assert same(g[6:], [a, w2c(cam, pf)[0]])
        differ += a != w2c(cam, pf)[0]
        hits += hit
    assert differ >= 5 and 100 < hits < len(world)
    keys = native(["K " + hx(v) for v in (-1.0, -0.3, 0.0, 0.49, -0.5, 2.75)])
    assert [[int(a), int(b)] for a, b in keys] == [[-3, -2], [-1, -1], [0, 0], [0, 0], [-2, -1], [5, 5]]
    assert [int(v) for v in restate_voxel(np.asarray([-1.0, -0.5], F32))] == [-3, -2]
    assert floor_keys([[-1.0, -0.5, 2.75]]).tolist() == [[-2, -1, 5]]


def test_map_point_and_view_choice(native):
    """A map point's fate, cell, distance and bid; getCloseViewObs: the first of equal cosines, a view from
    beyond 60 degrees."""
    from livo_amd import synth
    cam = small_cam()
    st = synth.make_state(2)
    Rcw, Pcw = restate_pose(synth.R_CI, synth.P_CI, st["rot"], st["pos"])
    R, P = pylist(Rcw), [float(v) for v in Pcw]
    fpos = frame_pos(R, P)
    rng = np.random.default_rng(8)
    sc = Scene(st, cam, board=False)
    pts = sc._pixels(st, rng.uniform(-20, 180, 300), rng.uniform(-20, 150, 300))[0]
    pts = np.concatenate([pts, 2 * np.asarray(fpos) - pts[:30]])  # behind the camera
    got = native(["M " + hx(cam["fx"], cam["fy"], cam["cx"], cam["cy"], 160, 128, 4, 20, Rcw, Pcw, p) for p in pts])
    fates = []
    for p, g in zip(pts, got):
        pos = [float(v) for v in p]
        pf = w2f(R, P, pos)
        pc = w2c(cam, pf)
        fate = 0 if pf[2] < 0 or not in_frame(cam, 24, pc) else 1
        fates.append(fate)
        assert int(g[0]) == fate
        if fate:
            dist = F32(norm3([fpos[k] - pos[k] for k in range(3)]))
            assert int(g[1]) == int(pc[0] / 20.0) * 6 + int(pc[1] / 20.0)
            assert same(g[2:6], [float(dist), pc[0], pc[1], pf[2]])
            assert int(g[6]) == (int(dist.view(np.uint32)) << 32) | (0xFFFFFFFF - 7)
    assert 50 < sum(fates) < 250
    pos = [0.0, 0.0, 6.0]
    views = [([0.0, 0.0, 0.0], [[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [1.0, 0.0, 0.0]]),   # equal cosines: the first
             ([0.0, 0.0, 0.0], [[11.0, 0.0, 6.0], [0.0, 12.0, 5.0]]),                    # beyond 60 degrees
             ([0.0, 0.0, 0.0], [[0.0, 0.0, 12.0]]),                                      # behind: cosine stays 0
             ([0.3, 0.1, 0.0], [list(rng.normal(0, 1.0, 3)) for _ in range(20)])]
    got = native(["V " + hx(f, pos) + f" {hx(len(r))} " + hx(r) for f, r in views])
    for (f, r), g in zip(views, got):
        best, cosine = close_view(f, pos, r)
        assert int(g[0]) == best and same(g[1], cosine)
    assert int(got[0][0]) == 0 and got[1][1] < 0.5 and got[2] == ["0", 0.0]


# -------------------------------------------------------------------- ABI ----
NEW = ("livo_vmap_reset", "livo_vmap_add_frame", "livo_vmap_add", "livo_vmap_info", "livo_vmap_dump", "livo_vio_match")


def test_header_library_and_binding_carry_the_entry_points(built):
    import livo_amd
    txt = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", livo_amd.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(rf"^int {name}\(", txt, flags=re.M) and name in livo_amd.SIGNATURES
        assert re.search(rf"\bT {name}\b", out)
    assert livo_amd.load().livo_abi_version() == int(re.search(r"#define LIVO_ABI_VERSION (\d+)", txt).group(1)) == 9
    for m in ("vmap_reset", "vmap_add_frame", "vmap_add", "vmap_info", "vmap_dump", "vio_match"):
        assert hasattr(livo_amd.Context, m)


def test_struct_layouts_match_c(tmp_path):
    import livo_amd
    fields = {"livo_vmatch_point": list(MATCH_DTYPE.names), "livo_vmap_point": list(livo_amd.VMAP_POINT_DTYPE.names),
              "livo_vmap_obs": list(livo_amd.VMAP_OBS_DTYPE.names)}
    src = tmp_path / "vm.c"
    body = "".join(f'printf("%zu ", sizeof({s}));' + "".join(f'printf("%zu ", offsetof({s}, {f}));' for f in fs)
                   for s, fs in fields.items())
    src.write_text('#include "livo.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){' + body +
                   'printf("%zu %zu\\n", sizeof(livo_vmatch_stats), sizeof(livo_vmap_counts));return 0;}\n')
    exe = tmp_path / "vm"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for dt in (livo_amd.VMATCH_POINT_DTYPE, livo_amd.VMAP_POINT_DTYPE, livo_amd.VMAP_OBS_DTYPE):
        want += [dt.itemsize] + [dt.fields[f][1] for f in dt.names]
    want += [C.sizeof(livo_amd.VmatchStats), C.sizeof(livo_amd.VmapCounts)]
    assert got == want and livo_amd.VMATCH_POINT_DTYPE == MATCH_DTYPE
    assert livo_amd.VMATCH_POINT_DTYPE.itemsize == 48 and livo_amd.VMAP_POINT_DTYPE.itemsize == 64
    assert tuple(f for f, _ in livo_amd.VmatchStats._fields_) == STAT_FIELDS


def test_null_context_returns_invalid(built):
    import livo_amd
    L = livo_amd.load()
    st, vp, n = livo_amd.State(), livo_amd.vio_params(small_cam(), np.eye(3), np.zeros(3)), C.c_int64(-7)
    assert L.livo_vmap_reset(None, 10, 2, 4) == -1
    assert L.livo_vmap_add_frame(None, 0, C.byref(st), C.byref(vp), None, 160, 128) == -1
    assert L.livo_vmap_add(None, 0, 0, None, None, None, None, None) == -1
    assert L.livo_vmap_info(None, None) == -1
    assert L.livo_vmap_dump(None, None, 0, None, None, 0, C.byref(n), C.byref(n)) == -1
    assert L.livo_vio_match(None, -1, C.byref(st), C.byref(vp), 20, 0, 0.0, 100.0, None, 160, 128, None, None, None,
                            None, 0, C.byref(n), None) == -1
    assert n.value == -7


# ------------------------------------------------- the cases, restated only ----
def closed_loop_inputs():
    """Frame A (make_state(1)) and frame B a few cm and tenths of a degree away, on the wall with the board."""
    from livo_amd import synth
    cam = small_cam()
    A = synth.make_state(1)
    B = moved(A, [0.03, -0.02, 0.015], [0.2, -0.15, 0.1])
    sc = Scene(A, cam)
    return cam, sc, A, B


def test_scene_renders_consistent_views():
    """The wall's texture moves with the pose: frame B's image differs from frame A's, and a wall point's
    neighbourhood looks alike in both (what lets the closed loop keep points)."""
    cam, sc, A, B = closed_loop_inputs()
    ia, ib = sc.render(A), sc.render(B)
    assert ia.shape == (128, 160) and ia.std() > 10 and np.mean(ia != ib) > 0.3
    assert np.mean(np.abs(ia.astype(int) - ib.astype(int))) < 12
