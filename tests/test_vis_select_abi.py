"""CPU checks of livo_vio_select (LidarSelector::addSparseMap, src/lidar_selection.cpp:140-193,
with getpatch :117-138 and AddPoint's voxel key :195-208): the entry point is declared, exported
and bound, its structures agree between C and ctypes, invalid arguments come back as codes, and
the per-point arithmetic of the kernels (cam_model.h, compiled for the host by
tests/native/vis_point_check.cpp) equals, bit for bit, the numpy restatement below.

The restatement follows the reference's operation order: Frame::w2f row sums left to right,
vikit's pinhole world2cam with no p_cam.z test, isInFrame(pc.cast<int>(), border) taken in
double, vikit's shiTomasiScore (integer sums, then float, one rounding per operation, the final
0.5 * in double), the strict `cur_value > map_value[index]` in cloud order, getpatch's mixed
float / double weights, and AddPoint's truncating key.  Every sum is spelled elementwise on
float32 / float64 arrays (IEEE operations, one rounding each): no `@`, no BLAS, no call into the
library.  tests/test_gpu_vis_select.py applies it to the device's world points.

The frame cases (frame_case) are built so that the restatement alone shows what they are for;
case_worth checks it here on the CPU, on restated world points, and the GPU test again on the
device's.  Every unique point is in the cloud twice, at two cloud indices, so every winner is
decided by the tie rule; a sixth of the points lie behind the camera on the ray of an in-frame
pixel; a rectangle of the image around one cell is flat, which leaves that cell empty.  Which
frame can show what:
  160 x 128, patch 4 (border 24), grid 20 / 40: 48 / 12 cells, 29 / 11 of them reachable and
      not flat; no index aliases or overflows (the frame test ends before the last row of cells);
  160 x 152, grid 40: 3 rows of cells, rows [120, 128) of the frame give row 3, which aliases
      into the next column, and column 3 with row 3 gives index 12 = length: the overflow;
  640 x 512 (synth.PINHOLE, distorted), patch 8 (border 40), grid 40: 192 cells, 153 reachable.
"""
import ctypes as C
import functools
import os
import re
import struct
import subprocess

import numpy as np
import pytest
from test_rgb_cloud_abi import restate_pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "livo.h")
F32, F64 = np.float32, np.float64

REC_DTYPE = np.dtype([("x", F32), ("y", F32), ("z", F32), ("score", F32), ("u", F64), ("v", F64),
                      ("src_index", np.int32), ("cell", np.int32), ("voxel", np.int64, (3,))])


# ------------------------------------------------------------ restatement ----
def restate_world(body, rot, pos, R_LI, t_LI):
    """pointBodyToWorld (laser_mapping.cpp:662-671): double math, float storage."""
    b = np.ascontiguousarray(body, F32).reshape(-1, 3).astype(F64)
    R, RL = np.asarray(rot, F64).reshape(3, 3), np.asarray(R_LI, F64).reshape(3, 3)
    p, tL = np.asarray(pos, F64).reshape(3), np.asarray(t_LI, F64).reshape(3)
    imu = [((RL[k, 0] * b[:, 0] + RL[k, 1] * b[:, 1]) + RL[k, 2] * b[:, 2]) + tL[k] for k in range(3)]
    return np.stack([(((R[k, 0] * imu[0] + R[k, 1] * imu[1]) + R[k, 2] * imu[2]) + p[k]).astype(F32)
                     for k in range(3)], axis=1)


def restate_w2c(xyz, cam, Rcw, Pcw):
    """new_frame_->w2c(pt) of float world points: (p_cam.z, u, v), all float64; no z test."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    fx, fy, cx, cy = (F64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    d = [F64(v) for v in list(cam["d"]) + [0.0] * (5 - len(cam["d"]))]
    with np.errstate(all="ignore"):
        x, y, z = (xyz[:, k].astype(F64) for k in range(3))  # V3D pt(p.x, p.y, p.z)
        pf = [((Rcw[k, 0] * x + Rcw[k, 1] * y) + Rcw[k, 2] * z) + Pcw[k] for k in range(3)]
        u = pf[0] / pf[2]  # project2d
        v = pf[1] / pf[2]
        if not abs(d[0]) > 0.0000001:  # vikit: distortion_ = |d0| > 1e-7
            px = fx * u + cx
            py = fy * v + cy
        else:
            r2 = u * u + v * v
            r4 = r2 * r2
            r6 = r4 * r2
            a1 = 2 * u * v
            a2 = r2 + 2 * u * u
            a3 = r2 + 2 * v * v
            cdist = 1 + d[0] * r2 + d[1] * r4 + d[4] * r6
            xd = u * cdist + d[2] * a1 + d[3] * a2
            yd = v * cdist + d[2] * a3 + d[3] * a1
            px = xd * fx + cx
            py = yd * fy + cy
    return pf[2], px, py


def restate_sums(img, u, v):
    """shiTomasiScore's three sums over rows [v-4, v+4), columns [u-4, u+4), as integers, and the
    `return 0.0` mask.  (The reference adds them as floats: integers below 2^24, exact in any order.)"""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    u, v = np.asarray(u, np.int64).reshape(-1), np.asarray(v, np.int64).reshape(-1)
    zero = (u - 4 < 1) | (u + 4 >= w - 1) | (v - 4 < 1) | (v + 4 >= h - 1)
    uc, vc = np.where(zero, 5, u), np.where(zero, 5, v)  # (any pixel with its box inside: not used)
    im = img.astype(np.int64)
    sxx, syy, sxy = (np.zeros(len(u), np.int64) for _ in range(3))
    for y in range(-4, 4):
        for x in range(-4, 4):
            dx = im[vc + y, uc + x + 1] - im[vc + y, uc + x - 1]
            dy = im[vc + y + 1, uc + x] - im[vc + y - 1, uc + x]
            sxx += dx * dx
            syy += dy * dy
            sxy += dx * dy
    assert max(sxx.max(initial=0), syy.max(initial=0), np.abs(sxy).max(initial=0)) < 2 ** 24
    return sxx, syy, sxy, zero


def restate_eigen(sxx, syy, sxy):
    """The smaller eigenvalue from the sums, in float32: one rounding per operation."""
    with np.errstate(all="ignore"):
        dXX = sxx.astype(F32) / F32(128.0)  # 2 * box_area: exact
        dYY = syy.astype(F32) / F32(128.0)
        dXY = sxy.astype(F32) / F32(128.0)
        s = dXX + dYY
        t = s * s - F32(4.0) * (dXX * dYY - dXY * dXY)
        r = np.sqrt(t)  # NaN for a negative t
        assert s.dtype == F32 and t.dtype == F32 and r.dtype == F32
        return (F64(0.5) * (s - r).astype(F64)).astype(F32), t


def restate_score(img, u, v):
    sxx, syy, sxy, zero = restate_sums(img, u, v)
    score, _ = restate_eigen(sxx, syy, sxy)
    return np.where(zero, F32(0.0), score)


def restate_patch(img, px, py, ps):
    """getpatch at levels 0, 1, 2 -> (n, 3 * ps^2) float32, patch_size_total * level + x * ps + y."""
    img = np.ascontiguousarray(img, np.uint8)
    px, py = np.asarray(px, F64).reshape(-1), np.asarray(py, F64).reshape(-1)
    imf = img.astype(F32)
    half, pst = ps // 2, ps * ps
    out = np.zeros((len(px), 3 * pst), F32)
    u_ref, v_ref = px.astype(F32), py.astype(F32)
    for level in range(3):
        scale = 1 << level
        u_f = np.floor((px / F64(scale)).astype(F32)) * F32(scale)  # floorf(pc[0]/scale)*scale
        v_f = np.floor((py / F64(scale)).astype(F32)) * F32(scale)
        ui, vi = u_f.astype(np.int64), v_f.astype(np.int64)         # const int u_ref_i = ...
        su = (u_ref - ui.astype(F32)) / F32(scale)
        sv = (v_ref - vi.astype(F32)) / F32(scale)
        assert su.dtype == F32 and sv.dtype == F32
        su64, sv64 = su.astype(F64), sv.astype(F64)
        w_tl = ((F64(1.0) - su64) * (F64(1.0) - sv64)).astype(F32)
        w_tr = (su64 * (F64(1.0) - sv64)).astype(F32)
        w_bl = ((F64(1.0) - su64) * sv64).astype(F32)
        w_br = su * sv
        for x in range(ps):
            r = vi - half * scale + x * scale
            for y in range(ps):
                c = ui - half * scale + y * scale
                val = ((w_tl * imf[r, c] + w_tr * imf[r, c + scale]) + w_bl * imf[r + scale, c]) + \
                    w_br * imf[r + scale, c + scale]
                assert val.dtype == F32
                out[:, pst * level + x * ps + y] = val
    return out


def restate_voxel(w):
    """One coordinate of AddPoint's VOXEL_KEY: float quotient, -1.0 below zero, truncation."""
    w = np.asarray(w, F32)
    loc = (w.astype(F64) / F64(0.5)).astype(F32)
    loc = np.where(loc < 0, (loc.astype(F64) - F64(1.0)).astype(F32), loc)
    return loc.astype(np.int64)


def restate_winners(ok, index, score, length):
    """addSparseMap's first loop over the accepted points, in cloud order: `cur_value > map_value[index]`,
    map_value starting at 0 (false for a NaN).  n_max: points of the winning score in the cell."""
    map_value = np.zeros(length, F32)
    winner = np.full(length, -1, np.int64)
    n_max = np.zeros(length, np.int64)
    for i in np.flatnonzero(ok):
        c = index[i]
        if score[i] > map_value[c]:
            map_value[c] = score[i]
            winner[c] = i
            n_max[c] = 1
        elif score[i] == map_value[c] and winner[c] >= 0:
            n_max[c] += 1
    return winner, map_value, n_max


def restate_select(xyz, cam, Rcw, Pcw, img, ps, grid):
    """addSparseMap on float world points.  Returns (records: REC_DTYPE, ascending cell; patches (n, 3 ps^2);
    stats; info: tie_cells = winners with two or more points of the maximal score, behind_winners)."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    h, w = img.shape
    assert cam["width"] == w and cam["height"] == h
    b = (ps // 2 + 1) * 8
    gnh = h // grid
    length = (w // grid) * gnh
    z, px, py = restate_w2c(xyz, cam, Rcw, Pcw)
    with np.errstate(all="ignore"):
        inframe = (px >= b) & (px < w - b) & (py >= b) & (py < h - b)  # (false for a NaN)
        behind = inframe & ~(z > 0)
        pxs, pys = np.where(inframe, px, 0.0), np.where(inframe, py, 0.0)
        index = (pxs / F64(grid)).astype(np.int64) * gnh + (pys / F64(grid)).astype(np.int64)
    overflow = inframe & (index >= length)
    ok = inframe & ~overflow
    score = restate_score(img, pxs.astype(np.int64), pys.astype(np.int64))
    winner, map_value, n_max = restate_winners(ok, index, score, length)
    cells = np.flatnonzero(winner >= 0)
    win = winner[cells]
    rec = np.zeros(len(cells), REC_DTYPE)
    rec["x"], rec["y"], rec["z"] = xyz[win, 0], xyz[win, 1], xyz[win, 2]
    rec["score"] = map_value[cells]
    rec["u"], rec["v"] = px[win], py[win]
    rec["src_index"], rec["cell"] = win, cells
    for k in range(3):
        rec["voxel"][:, k] = restate_voxel(xyz[win, k])
    patches = restate_patch(img, px[win], py[win], ps)
    stats = {"n_in": len(xyz), "in_frame": int(inframe.sum()), "behind_in_frame": int(behind.sum()),
             "cell_overflow": int(overflow.sum()), "n_out": len(cells), "n_cells": int(length)}
    info = {"tie_cells": int(np.sum(n_max[cells] >= 2)), "behind_winners": int(np.sum(behind[win])),
            "nan_scores": int(np.sum(np.isnan(score[ok]))), "zero_scores": int(np.sum(score[ok] == 0))}
    return rec, patches, stats, info


# ------------------------------------------------------------------ cases ----
SMALL = {"fx": 120.0 * 1.03, "fy": 120.0 * 0.99, "cx": 78.7, "cy": 0.0, "d": [0.0] * 5}
FRAMES = {  # name -> (width, height, patch_size, grid_size, distorted, the cell made flat as (column, row))
    "160x128-g20": (160, 128, 4, 20, False, (2, 2)),
    "160x128-g40": (160, 128, 4, 40, False, (1, 1)),
    "160x152-g20": (160, 152, 4, 20, False, (2, 2)),
    "160x152-g40": (160, 152, 4, 40, False, (1, 1)),
    "640x512-g40": (640, 512, 8, 40, True, (5, 5)),
}
SIZES = (0, 1, 63, 257, 3000)
BIG_N = 20_000
CASE_SEED = {"160x128-g20": 1, "160x128-g40": 1, "160x152-g20": 1, "160x152-g40": 6, "640x512-g40": 1}


@functools.lru_cache(maxsize=None)
def frame_image(name):
    """The frame's synth._texture image with the rectangle around one cell made flat, its camera and
    the extrinsics."""
    from livo_amd import synth
    w, h, ps, grid, distorted, (fc, fr) = FRAMES[name]
    img = synth._texture(w, h, np.random.default_rng(1000 + w + h)).copy()
    # the score's window at (u, v) spans columns u - 5 .. u + 4 and rows v - 5 .. v + 4
    img[fr * grid - 6:(fr + 1) * grid + 6, fc * grid - 6:(fc + 1) * grid + 6] = 117
    cam = dict(synth.PINHOLE) if distorted else dict(SMALL, width=w, height=h, cy=h / 2 - 0.4)
    assert cam["width"] == w and cam["height"] == h
    return img, cam, synth.R_CI, synth.P_CI


def frame_case(name, n, R_LI=None, t_LI=None):
    """(state, body points (n, 3) float32) of the frame: ceil(n / 2) unique points, the rest copies of them at
    other cloud indices; the unique points are back-projected from pixels spread over the frame and a margin
    around it, a sixth of them mirrored through the camera centre (behind it, on the same ray).  R_LI, t_LI:
    the LiDAR-IMU extrinsic the body points are expressed under (default: synth's, R_LI = I)."""
    from livo_amd import synth
    img, cam, Rci, Pci = frame_image(name)
    seed = CASE_SEED[name]
    rng = np.random.default_rng(7919 * seed + n)
    st = synth.make_state(seed)
    m = (n + 1) // 2
    w, h = cam["width"], cam["height"]
    u, v = rng.uniform(-0.15 * w, 1.15 * w, m), rng.uniform(-0.15 * h, 1.15 * h, m)
    z = rng.uniform(2.0, 12.0, m)
    z[rng.random(m) < 1.0 / 6.0] *= -1.0
    pf = np.stack([(u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z], axis=1)
    Rcw, Pcw = restate_pose(Rci, Pci, st["rot"], st["pos"])
    world = (pf - Pcw) @ Rcw                                  # p_w = Rcw^T (pf - Pcw)
    body = (world - st["pos"]) @ st["rot"] - (synth.T_LI if t_LI is None else np.asarray(t_LI, F64))
    if R_LI is not None:
        body = body @ np.asarray(R_LI, F64)                   # p_b = R_LI^T (p_I - t_LI)
    src = np.concatenate([np.arange(m), rng.permutation(m)[:n - m]])
    return st, np.ascontiguousarray(body[src][rng.permutation(n)], F32)


def case_worth(name, n, stats, info):
    """What a case must show, in the restatement alone; `n` points of frame `name`."""
    if n < 3000:
        return
    assert info["tie_cells"] >= 10
    assert info["behind_winners"] >= 1 and stats["behind_in_frame"] >= 1
    assert stats["n_out"] < stats["n_cells"] and 2 * stats["n_out"] > stats["n_cells"]
    if name == "160x152-g40":
        assert stats["cell_overflow"] >= 1
    else:
        assert stats["cell_overflow"] == 0
    assert stats["in_frame"] < stats["n_in"]


def restate_case(name, world, st):
    img, cam, Rci, Pci = frame_image(name)
    Rcw, Pcw = restate_pose(Rci, Pci, st["rot"], st["pos"])
    return restate_select(world, cam, Rcw, Pcw, img, FRAMES[name][2], FRAMES[name][3])


def negative_discriminant_sums():
    """Sums for which the discriminant rounds below zero.  From an 8-bit image there are none: sxx + syy <
    2^24, so s = dXX + dYY is exact; s * s >= 4 dXX dYY and rounding is monotonic, so fl(s * s) >= 4 fl(dXX *
    dYY) >= 4 fl(fl(dXX * dYY) - fl(dXY * dXY)), and t >= 0 (test_discriminant_never_rounds_negative).  Beyond
    that range s is rounded and t can fall below zero: the first such pair, searched deterministically."""
    rng = np.random.default_rng(0)
    for _ in range(100000):
        sxx = np.asarray([rng.integers(2 ** 24, 2 ** 26)], np.int64)
        syy = sxx + rng.integers(1, 64)
        sxy = np.zeros(1, np.int64)
        _, t = restate_eigen(sxx, syy, sxy)
        if t[0] < 0:
            return sxx, syy, sxy
    raise AssertionError("no sums found")


# ------------------------------------------------------------------ tests ----
def test_header_library_and_binding_carry_the_entry_point(built):
    import livo_amd
    txt = open(HEADER).read()
    assert re.search(r"^int livo_vio_select\(", txt, flags=re.M)
    assert "livo_vio_select" in livo_amd.SIGNATURES
    out = subprocess.run(["nm", "-D", "--defined-only", livo_amd.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT livo_vio_select\b", out)
    L = livo_amd.load()
    assert L.livo_abi_version() == int(re.search(r"#define LIVO_ABI_VERSION (\d+)", txt).group(1)) >= 8
    assert hasattr(livo_amd.Context, "vio_select")


def test_vis_struct_layouts_match_c(tmp_path):
    import livo_amd
    fields = ["x", "y", "z", "score", "u", "v", "src_index", "cell", "voxel"]
    src = tmp_path / "vis.c"
    src.write_text('#include "livo.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu",'
                   ' sizeof(livo_vis_point), sizeof(livo_vis_stats), offsetof(livo_vis_stats, n_cells));\n' +
                   "".join(f'printf(" %zu", offsetof(livo_vis_point, {f}));\n' for f in fields) +
                   'printf("\\n");return 0;}\n')
    exe = tmp_path / "vis"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == 64
    assert got == [C.sizeof(livo_amd.VisPoint), C.sizeof(livo_amd.VisStats), livo_amd.VisStats.n_cells.offset] + \
        [getattr(livo_amd.VisPoint, f).offset for f in fields]
    dt = livo_amd.VIS_POINT_DTYPE
    assert dt.itemsize == 64 and [dt.fields[f][1] for f in fields] == got[3:]
    assert dt == REC_DTYPE


def test_invalid_arguments_return_invalid(built):
    import livo_amd
    L = livo_amd.load()
    st = livo_amd.State()
    img, cam, Rci, Pci = frame_image("160x128-g40")
    n = C.c_int64(-7)
    fake = C.c_void_p(8)  # never dereferenced: the invalid argument is found first

    def call(ctx, s, pp, nn, grid=40, w=160, h=128):
        return L.livo_vio_select(ctx, -1, s, pp, grid, livo_amd._ptr(img), w, h, None, None, 0, nn, None)

    def params(ps=4, **kw):
        p = livo_amd.vio_params(dict(cam, **kw), Rci, Pci)
        p.patch_size = ps
        return p

    p = params()
    assert call(None, C.byref(st), C.byref(p), C.byref(n)) == -1
    assert call(fake, None, C.byref(p), C.byref(n)) == -1
    assert call(fake, C.byref(st), None, C.byref(n)) == -1
    assert call(fake, C.byref(st), C.byref(p), None) == -1
    assert call(fake, C.byref(st), C.byref(p), C.byref(n), grid=0) == -1
    assert call(fake, C.byref(st), C.byref(p), C.byref(n), grid=-40) == -1
    for ps in (0, 9, -1):
        assert call(fake, C.byref(st), C.byref(params(ps)), C.byref(n)) == -1
    assert call(fake, C.byref(st), C.byref(p), C.byref(n), h=127) == -1  # not cam.height
    # too small for one cell inside the border: 160 - 2 * 24 = 112 < 113; 128 - 48 = 80 < 81
    assert call(fake, C.byref(st), C.byref(p), C.byref(n), grid=113) == -1
    assert call(fake, C.byref(st), C.byref(p), C.byref(n), grid=81) == -1
    small = params(width=60, height=60)
    assert call(fake, C.byref(st), C.byref(small), C.byref(n), grid=20, w=60, h=60) == -1  # 60 - 48 < 20
    assert n.value == -7


@pytest.fixture(scope="module")
def vis_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("vis_native") / "vis_point_check"
    # (host code only, the flags of the library's own .cpp files: no FMA contraction)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "fast-livo-noted_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "vis_point_check.cpp"), "-o", str(exe)])
    return str(exe)


def run_native(exe, path, img, ps, uv, pc, keys):
    img = np.ascontiguousarray(img, np.uint8)
    uv = np.ascontiguousarray(uv, np.int32).reshape(-1, 2)
    pc = np.ascontiguousarray(pc, F64).reshape(-1, 2)
    keys = np.ascontiguousarray(keys, F32).reshape(-1)
    with open(path, "wb") as f:
        f.write(struct.pack("=6i", img.shape[1], img.shape[0], ps, len(uv), len(pc), len(keys)))
        for a in (img, uv, pc, keys):
            f.write(a.tobytes())
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = [ln.split() for ln in out.stdout.split("\n") if ln]
    s = np.array([int(t[1]) for t in lines if t[0] == "s"], np.uint32)
    p = np.array([[int(x) for x in t[1:]] for t in lines if t[0] == "p"], np.uint32).reshape(len(pc), 3 * ps * ps)
    k = np.array([int(t[1]) for t in lines if t[0] == "k"], np.int64)
    return s, p, k


KEY_CASES = [-1.0, -0.3, -0.5, 0.0, 0.49, -0.0, 0.5, 0.25, -0.25, 1e-30, -1e-30, 123.456, -123.456, 16777.217,
             -99999.75, 3.0e6, -3.0e6, 0.99999994, -0.49999997]


@pytest.mark.parametrize("name", ["160x128-g40", "160x152-g20", "640x512-g40"])
def test_per_point_functions_match_restatement(name, vis_check, tmp_path):
    img, cam, _, _ = frame_image(name)
    w, h, ps = FRAMES[name][0], FRAMES[name][1], FRAMES[name][2]
    rng = np.random.default_rng(w + ps)
    # scores: every alignment of the window's first byte, the flat rectangle, and the `return 0.0` rim
    uv = np.stack([rng.integers(0, w, 3000), rng.integers(0, h, 3000)], axis=1)
    rim = [(4, 40), (5, 40), (w - 6, 40), (w - 5, 40), (40, 4), (40, 5), (40, h - 6), (40, h - 5), (0, 0),
           (w - 1, h - 1), (-3, 40), (40, -3), (w + 2, 40), (40, h + 2)]
    uv = np.concatenate([uv, np.asarray(rim)])
    b = (ps // 2 + 1) * 8
    pc = np.stack([rng.uniform(b, w - b, 1500), rng.uniform(b, h - b, 1500)], axis=1)
    below = float(np.nextafter(F64(w - b), F64(0.0)))
    pc = np.concatenate([pc, [[b, b], [below, float(np.nextafter(F64(h - b), F64(0.0)))], [b + 0.5, b + 3.75],
                              [below, b], [float(np.nextafter(F32(64.0), F32(0.0))), 64.0]]])
    keys = np.concatenate([np.asarray(KEY_CASES, F32), rng.normal(0, 30, 500).astype(F32)])
    s, p, k = run_native(vis_check, tmp_path / "cases.bin", img, ps, uv, pc, keys)
    want = restate_score(img, uv[:, 0], uv[:, 1])
    assert np.array_equal(s, want.view(np.uint32))
    assert np.array_equal(p, restate_patch(img, pc[:, 0], pc[:, 1], ps).view(np.uint32))
    assert np.array_equal(k, restate_voxel(keys))
    # the cases are worth something: positive, zero (rim and flat) and distinct scores, every byte alignment
    assert np.sum(want > 0) > 1000 and np.sum(want[:3000] == 0) >= 1 and np.all(want[3000:][[0, 3, 4, 7]] == 0)
    assert np.all(want[3000:][[1, 2, 5, 6]] > 0)
    assert len(set(((uv[:3000, 1] - 5) * w + uv[:3000, 0] - 5) % 4)) == 4


def test_discriminant_never_rounds_negative():
    """The issue's NaN case cannot come from an 8-bit image (negative_discriminant_sums has the argument):
    over random and nearly equal sums of the image's range, t >= 0 and the score is finite and >= 0."""
    rng = np.random.default_rng(3)
    top = 64 * 255 * 255
    sxx = rng.integers(0, top + 1, 400000)
    syy = np.clip(sxx + rng.integers(-300, 301, sxx.size), 0, top)
    syy[::4] = rng.integers(0, top + 1, sxx[::4].size)
    bound = np.floor(np.sqrt(sxx.astype(F64) * syy.astype(F64))).astype(np.int64)  # Cauchy-Schwarz
    sxy = rng.integers(-1, 2, sxx.size) * (bound * rng.random(sxx.size) ** 8).astype(np.int64)
    sxy[1::4] = 0
    score, t = restate_eigen(sxx, syy, sxy)
    assert np.all(t >= 0) and np.all(np.isfinite(score))
    # ... while the formula itself does give NaN once s is no longer exact, and a NaN never wins a cell
    score, t = restate_eigen(*negative_discriminant_sums())
    assert t[0] < 0 and np.isnan(score[0])
    nan = score[0]
    winner, value, _ = restate_winners(np.ones(4, bool), np.asarray([0, 0, 0, 1]), np.asarray([nan, 2.0, nan, nan], F32), 2)
    assert list(winner) == [1, -1] and value[0] == 2.0 and value[1] == 0.0


def test_constructed_cases_mean_what_they_say():
    """Restatement only: flat and pure-edge regions score exactly 0 and are never selected, a discriminant
    cannot round negative here (test_discriminant_never_rounds_negative), u - 4 < 1 returns 0, and the voxel
    keys."""
    cam = {"width": 64, "height": 64, "fx": 32.0, "fy": 32.0, "cx": 32.0, "cy": 32.0, "d": [0.0] * 5}
    Rcw, Pcw = np.eye(3), np.zeros(3)
    at = lambda u, v: [((u - 32.0) / 32.0, (v - 32.0) / 32.0, 1.0)]  # noqa: E731  (fx a power of two: exact)
    # flat
    flat = np.full((64, 64), 90, np.uint8)
    assert restate_score(flat, [30], [30])[0] == 0 and restate_score(flat, [30], [30]).dtype == F32
    rec, _, stats, _ = restate_select(at(30.0, 30.0), cam, Rcw, Pcw, flat, 4, 16)
    assert len(rec) == 0 and stats["in_frame"] == 1 and stats["n_out"] == 0
    # a pure edge: one gradient direction only
    edge = np.tile(np.where(np.arange(64) < 30, 40, 200).astype(np.uint8), (64, 1))
    sxx, syy, sxy, _ = restate_sums(edge, [30], [30])
    assert sxx[0] > 0 and syy[0] == 0 and sxy[0] == 0
    assert restate_score(edge, [30], [30])[0] == 0
    assert len(restate_select(at(30.0, 30.0), cam, Rcw, Pcw, edge, 4, 16)[0]) == 0
    # a corner does score, and is selected
    corner = np.zeros((64, 64), np.uint8)
    corner[30:, 30:] = 200
    assert restate_score(corner, [30], [30])[0] > 0
    rec, pat, stats, _ = restate_select(at(30.0, 30.0) * 2, cam, Rcw, Pcw, corner, 4, 16)
    assert len(rec) == 1 and rec["src_index"][0] == 0 and rec["cell"][0] == 1 * 4 + 1 and rec["u"][0] == 30.0
    assert list(pat[0, :16]) == [0] * 10 + [200, 200] + [0, 0] + [200, 200]  # rows 28..31, columns 28..31
    # u - 4 < 1 (and its three siblings) return 0 on an image that scores everywhere else
    from livo_amd import synth
    tex = synth._texture(64, 64, np.random.default_rng(5))
    assert restate_score(tex, [4], [30])[0] == 0 and restate_score(tex, [5], [30])[0] > 0
    assert restate_score(tex, [59], [30])[0] == 0 and restate_score(tex, [58], [30])[0] > 0
    assert restate_score(tex, [30], [4])[0] == 0 and restate_score(tex, [30], [59])[0] == 0
    # AddPoint's key: -1.0 m gives -3 (floor: -2), -0.3 gives -1, -0.5 gives -2, 0.0 and 0.49 give 0
    assert list(restate_voxel([-1.0, -0.3, -0.5, 0.0, 0.49])) == [-3, -1, -2, 0, 0]
    # the lowest cloud index wins among equal scores; a later, strictly better point replaces it
    pts = at(30.25, 30.5) + at(30.75, 30.25) + at(30.5, 30.5)
    rec, _, _, info = restate_select(pts, cam, Rcw, Pcw, corner, 4, 16)
    assert len(rec) == 1 and rec["src_index"][0] == 0 and info["tie_cells"] == 1 and rec["u"][0] == 30.25
    # a point behind the camera on the ray of an in-frame pixel is accepted and counted
    x, y, z = at(30.0, 30.0)[0]
    rec, _, stats, info = restate_select([(-x, -y, -z)], cam, Rcw, Pcw, corner, 4, 16)
    assert len(rec) == 1 and stats["behind_in_frame"] == 1 and info["behind_winners"] == 1


@pytest.mark.parametrize("name", list(FRAMES))
def test_frame_cases_prove_their_worth(name):
    """The GPU test's inputs show ties, behind-camera winners, the overflow, empty and occupied cells in the
    restatement alone (on restated world points; the GPU test repeats this on the device's)."""
    from livo_amd import synth
    n = BIG_N if name == "640x512-g40" else 3000
    st, body = frame_case(name, n)
    world = restate_world(body, st["rot"], st["pos"], np.eye(3), synth.T_LI)
    rec, pat, stats, info = restate_case(name, world, st)
    case_worth(name, n, stats, info)
    assert np.all(np.diff(rec["cell"]) > 0) and pat.shape == (len(rec), 3 * FRAMES[name][2] ** 2)
    if name == "160x152-g40":  # rows [120, 128) alias into the next column: a winner of cell 3 with u < 40
        alias = rec[(rec["v"] >= 120) & (rec["cell"] == (rec["u"] // 40).astype(np.int64) * 3 + 3)]
        assert len(alias) >= 1
