"""CPU checks of livo_cloud_colorize (LaserMapping::publish_frame_world_rgb,
src/laser_mapping.cpp:1351-1381): the entry point is declared, exported and bound, its
structures agree between C and ctypes, NULL arguments come back as codes, and the per-point
arithmetic of the kernel (cam_model.h, compiled for the host by tests/native/rgb_point_check.cpp)
equals, value for value, the numpy restatement below.

The restatement follows the reference's operation order: Frame::w2f row sums left to right,
vikit's pinhole world2cam, isInFrame(pc.cast<int>(), 0) taken in double, and
LidarSelector::getpixel (src/lidar_selection.cpp:1004-1022) with its mixed float / double
weights and the image as a flat byte array.  Every sum is spelled elementwise on float32 /
float64 arrays (IEEE operations, one rounding each): no `@`, no BLAS.
tests/test_gpu_rgb_cloud.py applies it to the device's world points.
"""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "livo.h")

KEPT, BEHIND, OUT_OF_FRAME = 0, 1, 2
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------ restatement ----
def restate_pose(Rci, Pci, rot, pos):
    """Rcw = Rci * Rwi^T, Pcw = -Rci * Rwi^T * Pwi + Pci (lidar_selection.cpp:900-901)."""
    Rci = np.asarray(Rci, F64).reshape(3, 3)
    rot = np.asarray(rot, F64).reshape(3, 3)
    Pci = np.asarray(Pci, F64).reshape(3)
    pos = np.asarray(pos, F64).reshape(3)
    Rcw = np.zeros((3, 3), F64)
    Pcw = np.zeros(3, F64)
    for i in range(3):
        for j in range(3):  # Rwi^T[k][j] = rot[j][k]
            Rcw[i, j] = (Rci[i, 0] * rot[j, 0] + Rci[i, 1] * rot[j, 1]) + Rci[i, 2] * rot[j, 2]
    for k in range(3):
        Pcw[k] = -((Rcw[k, 0] * pos[0] + Rcw[k, 1] * pos[1]) + Rcw[k, 2] * pos[2]) + Pci[k]
    return Rcw, Pcw


def restate_colorize(xyz, cam, Rcw, Pcw, img):
    """Per world point (float32 x, y, z): fate (KEPT / BEHIND / OUT_OF_FRAME), rgb (n, 3) uint8 as
    r, g, b, and the edge flag (a tap outside the image buffer, read as 0)."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[0], img.shape[1]
    assert img.shape == (h, w, 3) and cam["width"] == w and cam["height"] == h
    fx, fy, cx, cy = (F64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    d = [F64(v) for v in list(cam["d"]) + [0.0] * (5 - len(cam["d"]))]
    with np.errstate(all="ignore"):
        x, y, z = (xyz[:, k].astype(F64) for k in range(3))  # V3D p_w(p.x, p.y, p.z)
        pf = [((Rcw[k, 0] * x + Rcw[k, 1] * y) + Rcw[k, 2] * z) + Pcw[k] for k in range(3)]
        front = pf[2] > 0  # (false for a NaN)
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
        inframe = (px > -1.0) & (px < F64(w)) & (py > -1.0) & (py < F64(h))
        kept = front & inframe
        fate = np.where(front, np.where(inframe, KEPT, OUT_OF_FRAME), BEHIND).astype(np.int32)
        # getpixel, on the kept points (the others get pixel 0, 0: their colour is not used)
        u_ref = np.where(kept, px, 0.0).astype(F32)
        v_ref = np.where(kept, py, 0.0).astype(F32)
        u_i = np.floor(u_ref)  # floorf, then int: exact in float32 again
        v_i = np.floor(v_ref)
        su = u_ref - u_i
        sv = v_ref - v_i
        assert su.dtype == F32 and sv.dtype == F32
        su64, sv64 = su.astype(F64), sv.astype(F64)
        w_tl = ((F64(1.0) - su64) * (F64(1.0) - sv64)).astype(F32)
        w_tr = (su64 * (F64(1.0) - sv64)).astype(F32)
        w_bl = ((F64(1.0) - su64) * sv64).astype(F32)
        w_br = su * sv
        assert w_br.dtype == F32
        flat = img.reshape(-1)
        nbytes = flat.size
        row = 3 * w
        o = (v_i.astype(np.int64) * w + u_i.astype(np.int64)) * 3
        edge = np.zeros(len(xyz), bool)

        def tap(off):
            nonlocal edge
            inside = (off >= 0) & (off < nbytes)
            edge = edge | ~inside
            return np.where(inside, flat[np.clip(off, 0, nbytes - 1)], 0).astype(F32)

        ch = []
        for c in range(3):  # B, G, R
            val = ((w_tl * tap(o + c) + w_tr * tap(o + c + 3)) + w_bl * tap(o + row + c)) + w_br * tap(o + row + c + 3)
            assert val.dtype == F32
            ch.append((val.astype(np.int32) & 255).astype(np.uint8))  # pointRGB.r = pixel[2]: truncation
        rgb = np.stack([ch[2], ch[1], ch[0]], axis=1)
        rgb[~kept] = 0
        edge = edge & kept
    return fate, rgb, edge


def restate_stats(fate, edge):
    return {"n_in": int(len(fate)), "n_out": int(np.sum(fate == KEPT)), "behind": int(np.sum(fate == BEHIND)),
            "out_of_frame": int(np.sum(fate == OUT_OF_FRAME)), "edge_reads": int(np.sum(edge))}


# ------------------------------------------------------------------ cases ----
W, H = 64, 48
CAM_PLAIN = {"width": W, "height": H, "fx": 32.0, "fy": 32.0, "cx": 32.0, "cy": 24.0, "d": [0.0] * 5}
CAM_DIST = {"width": W, "height": H, "fx": 41.3, "fy": 40.7, "cx": 31.2, "cy": 23.6,
            "d": [-0.0944205499243979, 0.0946727677776504, -0.00807970960613932, 8.07461209775283e-05, 0.0]}


def random_image(w=W, h=H, seed=11):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def edge_points():
    """World points for CAM_PLAIN under the identity pose (camera = world, fx = fy = 32, a power of two:
    x = (u - 32) / 32 at z = 1 lands on pixel u exactly).  (u, v, z) per case."""
    nan, inf = float("nan"), float("inf")
    just_below_1 = float(np.nextafter(F32(1.0), F32(0.0)))  # u = 64 - 2^-19 in double: rounds up to 64.0f
    uvz = [
        (5.0, 7.0, 1.0), (0.0, 0.0, 1.0), (12.0, 30.0, 2.0),        # exact integer pixels
        (63.0, 10.0, 1.0),                                          # last column: right taps from the next row
        (63.0, 47.0, 1.0),                                          # last pixel: three taps outside
        (-0.5, 10.0, 1.0),                                          # left taps: previous row's last pixel
        (-0.5, 0.0, 1.0),                                           # ... outside the buffer in row 0
        (W - 0.5, 10.0, 1.0), (W - 0.5, 46.5, 1.0),                 # right taps: next row's first pixel
        (10.0, H - 0.5, 1.0), (10.25, H - 1.0, 1.0), (W - 0.5, H - 0.5, 1.0),  # last row: lower taps outside
        (0.5, -0.5, 1.0), (20.75, -0.25, 4.0),                      # v in (-1, 0): upper taps outside
        (-1.0, 10.0, 1.0), (float(W), 10.0, 1.0), (10.0, -1.0, 1.0), (10.0, float(H), 1.0),  # just out of frame
        (10.0, 10.0, 0.0), (32.0, 24.0, 0.0),                       # z = 0
        (10.0, 10.0, -1.0), (32.0, 24.0, -3.0),                     # z < 0
    ]
    pts = [((u - 32.0) / 32.0 * z, (v - 24.0) / 32.0 * z, z) for u, v, z in uvz]
    pts += [
        (0.0, 0.0, 1e-12),                  # z = 1e-12 on the axis: the principal point
        (1e-3, 0.0, 1e-12),                 # ... off it: far out of frame
        (nan, 0.0, 1.0), (0.0, 0.0, nan), (nan, nan, nan),
        (inf, 0.0, 1.0), (0.0, 0.0, inf), (-inf, 0.0, 1.0),
        (just_below_1, 0.0, 1.0),           # (float)u = 64: column `width`, the next row's first pixel
        (0.0, 0.75 * just_below_1, 1.0),    # (float)v = 48: row `height`, every tap outside
    ]
    return np.asarray(pts, F32)


def random_points(n, seed, Rcw, Pcw, cam):
    """World points whose camera-frame image covers the frame and a margin around it, a tenth behind."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.3, 12.0, n)
    z[rng.random(n) < 0.1] *= -1.0
    u = rng.uniform(-0.4 * cam["width"], 1.4 * cam["width"], n)
    v = rng.uniform(-0.4 * cam["height"], 1.4 * cam["height"], n)
    pf = np.stack([(u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z], axis=1)
    q = pf - Pcw  # p_w = Rcw^T (pf - Pcw)
    return np.stack([q[:, 0] * Rcw[0, k] + q[:, 1] * Rcw[1, k] + q[:, 2] * Rcw[2, k] for k in range(3)], axis=1).astype(F32)


def random_pose(seed):
    from livo_amd import synth
    rng = np.random.default_rng(seed)
    rot = synth.so3_exp(rng.normal(0, 0.7, 3))
    pos = rng.normal(0, 2.0, 3)
    Rci = synth.R_CI @ synth.so3_exp(rng.normal(0, 0.05, 3))
    Pci = synth.P_CI + rng.normal(0, 0.01, 3)
    return Rci, Pci, rot, pos


IDENTITY_POSE = (np.eye(3), np.zeros(3), np.eye(3), np.zeros(3))


def cases():
    """(name, cam, (Rci, Pci, rot, pos), image, world points)."""
    img = random_image()
    out = [("edges", CAM_PLAIN, IDENTITY_POSE, img, edge_points())]
    for name, cam, seed in (("plain", CAM_PLAIN, 3), ("distorted", CAM_DIST, 4)):
        pose = random_pose(seed)
        Rcw, Pcw = restate_pose(*pose)
        pts = np.concatenate([random_points(2000, seed, Rcw, Pcw, cam), edge_points()])
        out.append((name, cam, pose, img, pts))
    return out


# ------------------------------------------------------------------ tests ----
def test_header_library_and_binding_carry_the_entry_point(built):
    import livo_amd
    txt = open(HEADER).read()
    assert re.search(r"^int livo_cloud_colorize\(", txt, flags=re.M)
    assert "livo_cloud_colorize" in livo_amd.SIGNATURES
    out = subprocess.run(["nm", "-D", "--defined-only", livo_amd.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT livo_cloud_colorize\b", out)
    L = livo_amd.load()
    assert L.livo_abi_version() == int(re.search(r"#define LIVO_ABI_VERSION (\d+)", txt).group(1))
    assert hasattr(livo_amd.Context, "colorize")


def test_rgb_struct_layouts_match_c(tmp_path):
    import livo_amd
    src = tmp_path / "rgb.c"
    src.write_text('#include "livo.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu '
                   '%zu %zu\\n", sizeof(livo_rgb_point), sizeof(livo_rgb_stats), offsetof(livo_rgb_point, r), '
                   'offsetof(livo_rgb_point, a), offsetof(livo_rgb_stats, edge_reads));return 0;}\n')
    exe = tmp_path / "rgb"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == 16
    assert got == [C.sizeof(livo_amd.RgbPoint), C.sizeof(livo_amd.RgbStats), livo_amd.RgbPoint.r.offset,
                   livo_amd.RgbPoint.a.offset, livo_amd.RgbStats.edge_reads.offset]
    dt = livo_amd.RGB_POINT_DTYPE
    assert dt.itemsize == 16 and dt.fields["r"][1] == livo_amd.RgbPoint.r.offset and dt.fields["a"][1] == 15


def test_null_arguments_return_invalid(built):
    import livo_amd
    L = livo_amd.load()
    st = livo_amd.State()
    p = livo_amd.vio_params(CAM_PLAIN, np.eye(3), np.zeros(3))
    n = C.c_int64(-7)
    img = random_image()
    fake = C.c_void_p(8)  # never dereferenced: the NULL argument is found first
    args = lambda ctx, s, pp, nn: L.livo_cloud_colorize(ctx, -1, s, pp, livo_amd._ptr(img), W, H, None, None, 0, nn,  # noqa: E731
                                                        None)
    assert args(None, C.byref(st), C.byref(p), C.byref(n)) == -1
    assert args(fake, None, C.byref(p), C.byref(n)) == -1
    assert args(fake, C.byref(st), None, C.byref(n)) == -1
    assert args(fake, C.byref(st), C.byref(p), None) == -1
    assert n.value == -7


@pytest.fixture(scope="module")
def rgb_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rgb_native") / "rgb_point_check"
    # (host code only, the flags of the library's own .cpp files: no FMA contraction)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "fast-livo-noted_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "rgb_point_check.cpp"), "-o", str(exe)])
    return str(exe)


def run_native(exe, path, cam, pose, img, pts):
    Rci, Pci, rot, pos = (np.asarray(a, F64).reshape(-1) for a in pose)
    d = list(cam["d"]) + [0.0] * (5 - len(cam["d"]))
    with open(path, "wb") as f:
        f.write(struct.pack("=3i", cam["width"], cam["height"], len(pts)))
        f.write(np.asarray([cam["fx"], cam["fy"], cam["cx"], cam["cy"]] + d, F64).tobytes())
        for a in (Rci, Pci, rot, pos):
            f.write(a.tobytes())
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())
        f.write(np.ascontiguousarray(pts, F32).tobytes())
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = out.stdout.split("\n")
    head = lines[0].split()
    assert head[0] == "pose"
    pose_native = np.array([float.fromhex(t) for t in head[1:]], F64)
    rows = np.array([[int(t) for t in ln.split()] for ln in lines[1:] if ln], np.int64).reshape(-1, 6)
    return pose_native, rows


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_per_point_function_matches_restatement(case, rgb_check, tmp_path):
    name, cam, pose, img, pts = case
    pose_native, rows = run_native(rgb_check, tmp_path / "cases.bin", cam, pose, img, pts)
    Rcw, Pcw = restate_pose(*pose)
    assert np.array_equal(pose_native.view(np.uint64), np.concatenate([Rcw.reshape(9), Pcw]).view(np.uint64))
    fate, rgb, edge = restate_colorize(pts, cam, Rcw, Pcw, img)
    assert rows.shape[0] == len(pts)
    kept = fate == KEPT
    mismatches = int(np.sum(rows[:, 0] != fate)) + int(np.sum(rows[:, 5] != edge)) + \
        int(np.sum(rows[kept, 1:4] != rgb[kept])) + int(np.sum(rows[kept, 4] != 255))
    assert mismatches == 0
    # the cases are worth something: every fate occurs, and the edge reads too
    assert kept.sum() > 10 and np.sum(fate == BEHIND) >= 5 and np.sum(fate == OUT_OF_FRAME) >= 5 and edge.sum() >= 5
    if name != "edges":
        assert 0.2 < kept.mean() < 0.8


def test_edge_cases_mean_what_they_say():
    """The constructed points hit the cases they are named for (restatement only): the flat-offset
    wraps give the neighbouring row's pixel, last-row and row -1 points are kept with 0 taps."""
    img = random_image()
    Rcw, Pcw = restate_pose(*IDENTITY_POSE)
    pts = edge_points()
    fate, rgb, edge = restate_colorize(pts, CAM_PLAIN, Rcw, Pcw, img)
    bgr = lambda r, c: img[r, c].astype(F32)  # noqa: E731
    trunc = lambda v: (v.astype(np.int32) & 255)[::-1]  # noqa: E731  (B, G, R) floats -> r, g, b
    assert list(fate[:3]) == [KEPT] * 3 and not edge[:3].any()
    assert np.array_equal(rgb[0], img[7, 5][::-1]) and np.array_equal(rgb[1], img[0, 0][::-1])
    assert fate[3] == KEPT and not edge[3] and np.array_equal(rgb[3], img[10, 63][::-1])  # (su = 0: weight 0 on the wrap)
    assert fate[4] == KEPT and edge[4] and np.array_equal(rgb[4], img[47, 63][::-1])
    # u = -0.5, v = 10: half of row 9's last pixel, half of row 10's first
    assert fate[5] == KEPT and not edge[5]
    assert np.array_equal(rgb[5], trunc(F32(0.5) * bgr(9, 63) + F32(0.5) * bgr(10, 0)))
    assert fate[6] == KEPT and edge[6] and np.array_equal(rgb[6], trunc(F32(0.5) * bgr(0, 0)))
    # u = 63.5, v = 10: half of (10, 63), half of the next row's first pixel
    assert fate[7] == KEPT and not edge[7]
    assert np.array_equal(rgb[7], trunc(F32(0.5) * bgr(10, 63) + F32(0.5) * bgr(11, 0)))
    assert list(fate[9:14]) == [KEPT] * 5 and edge[9:14].all()
    assert np.array_equal(rgb[9], trunc(F32(0.5) * bgr(47, 10)))  # v = 47.5: the lower taps read 0
    assert np.array_equal(rgb[12], trunc(F32(0.25) * bgr(0, 0) + F32(0.25) * bgr(0, 1)))  # u = 0.5, v = -0.5
    assert list(fate[14:18]) == [OUT_OF_FRAME] * 4
    assert list(fate[18:22]) == [BEHIND] * 4
    n0 = 22
    assert fate[n0] == KEPT and np.array_equal(rgb[n0], img[24, 32][::-1])  # z = 1e-12 on the axis
    assert fate[n0 + 1] == OUT_OF_FRAME
    # a NaN coordinate reaches p_cam.z through 0 * NaN: `p_cam.z > 0` is false
    assert list(fate[n0 + 2:n0 + 5]) == [BEHIND] * 3
    # +-inf in x: 0 * inf = NaN in p_cam.z; inf in z: p_cam.z = inf > 0, the pixel is NaN
    assert fate[n0 + 5] == BEHIND and fate[n0 + 6] == OUT_OF_FRAME and fate[n0 + 7] == BEHIND
    assert fate[n0 + 8] == KEPT and not edge[n0 + 8] and np.array_equal(rgb[n0 + 8], img[25, 0][::-1])
    assert fate[n0 + 9] == KEPT and edge[n0 + 9] and np.array_equal(rgb[n0 + 9], [0, 0, 0])
