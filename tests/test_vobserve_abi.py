"""CPU checks of livo_vio_observe (LidarSelector::addObservation, src/lidar_selection.cpp:905-962, with
Point::getFurthestViewObs, src/point.cpp:211-239): the entry point is declared, exported and bound, still at
ABI version 9, its two structures agree between C and numpy / ctypes, a null context comes back as a code,
and the per-item arithmetic of the kernel (csrc/vmap_model.h, compiled for the host by
tests/native/vobserve_point_check.cpp) equals, value for value, the restatement below.

The restatement is written from the contract with test_vmatch_abi's scalar helpers:
Python floats are IEEE doubles, one rounding per operation, 3-term sums left to right.  ObserveModel adds
the whole call to MapModel; tests/test_gpu_vobserve.py compares the device with it byte for byte.  Lists
are in the map's order: index 0 is the oldest observation held (the reference's obs_.back()).
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
from test_vis_select_abi import restate_patch, restate_score
from test_vmatch_abi import (EYE, MAX_OBS, MapModel, cam2world, hx, in_frame, norm3, pylist, same, small_cam,
                             w2c, w2f)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "livo.h")
F32, F64 = np.float32, np.float64

OBS_DTYPE = np.dtype([("point_id", np.int32), ("flags", np.int32), ("n_obs", np.int32), ("deleted_index", np.int32),
                      ("deleted_frame_id", np.int32), ("score", F32), ("u", F64), ("v", F64), ("delta_p", F64),
                      ("pixel_dist", F64)])
OBS_STAT_FIELDS = ("n_in", "behind", "out_of_frame", "pose_flagged", "pixel_flagged", "added", "deleted",
                   "deleted_without_add", "n_obs_total")
BEHIND, OUT_OF_FRAME, POSE, PIXEL, DELETED, ADDED = 1, 2, 4, 8, 16, 32


# ------------------------------------------------------------ restatement ----
def observe_project(cam, border, R, P, pos):
    """-> (fate, pc): 1 behind (pt_cam.z <= 0; a NaN passes), 2 outside the border, 0 with the pixel."""
    pf = w2f(R, P, pos)
    if pf[2] <= 0:
        return 1, [0.0, 0.0]
    pc = w2c(cam, pf)
    if not in_frame(cam, border, pc):
        return 2, [0.0, 0.0]
    return 0, pc


def delta_p(Rr, Pr, cur_pos):
    """|ref.Pcw + ref.Rcw cur.pos|: the row sums left to right, then the sum (w2f's order)."""
    return norm3(w2f(Rr, Pr, cur_pos))


def pixel_dist(pc, px):
    dx, dy = pc[0] - px[0], pc[1] - px[1]
    return math.sqrt(dx * dx + dy * dy)


def view_dist(ref_pos, cur_pos):
    return norm3([ref_pos[k] - cur_pos[k] for k in range(3)])


def furthest(dist):
    """getFurthestViewObs in the map's order: from the highest index down, strictly above a maximum that
    starts at 0; the newest if none is."""
    best, maxdist = len(dist) - 1, 0.0
    for k in range(len(dist) - 1, -1, -1):
        if dist[k] > maxdist:
            best, maxdist = k, dist[k]
    return best


class ObserveModel(MapModel):
    """MapModel with livo_vio_observe restated."""

    def observe(self, fid, ids, levels=None):
        """-> records (OBS_DTYPE), stats; self.points is edited as the device edits the map."""
        cam, ps = self.cam, self.ps
        cur = self.frames[fid]
        border = (ps // 2 + 1) * 8
        ids = [int(i) for i in ids]
        assert len(set(ids)) == len(ids)
        recs = np.zeros(len(ids), OBS_DTYPE)
        stats = dict.fromkeys(OBS_STAT_FIELDS, 0)
        stats["n_in"] = len(ids)
        for i, pid in enumerate(ids):
            pt = self.points[pid]
            obs = pt["obs"]
            fate, pc = observe_project(cam, border, cur["R"], cur["P"], pt["pos"])
            flags, deleted, frame, score, dp, pd = 0, -1, -1, F32(0.0), 0.0, 0.0
            if fate:
                flags = BEHIND if fate == 1 else OUT_OF_FRAME
                stats["behind" if fate == 1 else "out_of_frame"] += 1
            else:
                ref = self.frames[obs[0]["frame_id"]]
                dp = delta_p(ref["R"], ref["P"], cur["pos"])
                pd = pixel_dist(pc, obs[0]["px"])
                if dp > 0.5:
                    flags |= POSE
                    stats["pose_flagged"] += 1
                if pd > 40.0:
                    flags |= PIXEL
                    stats["pixel_flagged"] += 1
                add = bool(flags & (POSE | PIXEL))
                if len(obs) >= MAX_OBS:
                    deleted = furthest([view_dist(self.frames[o["frame_id"]]["pos"], cur["pos"]) for o in obs])
                    frame = obs[deleted]["frame_id"]
                    del obs[deleted]
                    flags |= DELETED
                    stats["deleted"] += 1
                    stats["deleted_without_add"] += not add
                if add:
                    score = F32(restate_score(cur["img"], [int(pc[0])], [int(pc[1])])[0])
                    pt["value"] = score
                    obs.append({"frame_id": fid, "level": 0 if levels is None else int(levels[i]), "px": list(pc),
                                "f": cam2world(cam, pc[0], pc[1]),
                                "patch": restate_patch(cur["img"], [pc[0]], [pc[1]], ps)[0].copy()})
                    flags |= ADDED
                    stats["added"] += 1
            recs[i] = (pid, flags, len(obs), deleted, frame, score, pc[0], pc[1], dp, pd)
        stats["n_obs_total"] = sum(len(p["obs"]) for p in self.points)
        return recs, stats


# ----------------------------------------------------------- native cases ----
@pytest.fixture(scope="module")
def native(tmp_path_factory):
    d = tmp_path_factory.mktemp("vobserve_native")
    exe = d / "vobserve_point_check"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "fast-livo-noted_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "vobserve_point_check.cpp"), "-o", str(exe)])

    def run(lines):
        path = d / "cases.txt"
        path.write_text("\n".join(lines) + "\n")
        out = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
        rows = [ln.split() for ln in out.stdout.split("\n") if ln]
        assert len(rows) == len(lines)
        return [[int(t) if re.fullmatch(r"-?\d+", t) else float.fromhex(t) for t in r[1:]] for r in rows]

    return run


def up(x, n=1):
    for _ in range(n):
        x = float(np.nextafter(F64(x), F64(np.inf)))
    return x


def down(x, n=1):
    for _ in range(n):
        x = float(np.nextafter(F64(x), F64(-np.inf)))
    return x


def test_delta_p_at_half_a_metre(native):
    """delta_p exactly 0.5 and one step on either side (a pure translation: sqrt(x * x) is x here); general
    poses, where the row sums' order shows."""
    from livo_amd import synth
    cases = [(EYE, [0.0, 0.0, 0.0], [x, 0.0, 0.0]) for x in (0.5, up(0.5), down(0.5))]
    cases += [(EYE, [0.3, 0.0, 0.4], [0.0, 0.0, 0.0]), (EYE, [0.0, -0.5, 0.0], [0.0, 0.0, 0.0])]
    rng = np.random.default_rng(21)
    for _ in range(60):
        cases.append((synth.so3_exp(rng.normal(0, 0.4, 3)), rng.normal(0, 0.4, 3), rng.normal(0, 0.4, 3)))
    got = native(["D " + hx(R, P, c) for R, P, c in cases])
    want = [delta_p(pylist(R), [float(v) for v in P], [float(v) for v in c]) for R, P, c in cases]
    assert same([g[0] for g in got], want) and [g[1] for g in got] == [int(w > 0.5) for w in want]
    assert want[:3] == [0.5, up(0.5), down(0.5)] and [g[1] for g in got[:3]] == [0, 1, 0]
    assert 10 < sum(g[1] for g in got) < 55


def test_pixel_dist_at_forty(native):
    """d = (24, 32) is 40 exactly; pc.x one step up and down; general offsets."""
    px = [50.0, 40.0]
    cases = [([x, 72.0], px) for x in (74.0, up(74.0), down(74.0))]
    rng = np.random.default_rng(22)
    cases += [(list(rng.uniform(24, 136, 2)), list(rng.uniform(0, 160, 2))) for _ in range(60)]
    got = native(["X " + hx(pc, q) for pc, q in cases])
    want = [pixel_dist(pc, q) for pc, q in cases]
    assert same([g[0] for g in got], want) and [g[1] for g in got] == [int(w > 40.0) for w in want]
    assert want[0] == 40.0 and want[1] > 40.0 > want[2] and [g[1] for g in got[:3]] == [0, 1, 0]
    assert 10 < sum(g[1] for g in got) < 55


def test_furthest_view_choice(native):
    """Equal maxima (the highest index), all zero and all NaN (index n - 1), a NaN among finite distances,
    the maximum at either end of a full list."""
    nan = float("nan")
    c = [0.1, -0.2, 0.3]
    at = lambda d: [c[0] + d, c[1], c[2]]  # noqa: E731  (a frame d metres along x: the distance is |d| or near it)
    rng = np.random.default_rng(23)
    full = [list(rng.normal(0, 1.0, 3)) for _ in range(MAX_OBS)]
    far = [c[0] + 50.0, c[1], c[2]]
    cases = [
        [at(1.0), at(2.0), at(-2.0), at(0.5)],                       # two equal maxima: index 2
        [at(2.0), at(1.0), at(-2.0), at(2.0), at(0.5)],              # three: index 3
        [list(c)] * 5,                                               # all zero: index 4
        [[nan, 0.0, 0.0]] * 4,                                       # all NaN: index 3
        [at(1.0), [nan, 0.0, 0.0], at(3.0), [0.0, nan, 0.0], at(2.0)],  # a NaN among finite ones: index 2
        [far] + full[1:],                                            # the maximum at index 0
        full[:-1] + [far],                                           # ... and at index 19
        [at(0.25)],
    ]
    got = native(["F " + hx(c) + f" {hx(len(r))} " + hx(r) for r in cases])
    picks = []
    for r, g in zip(cases, got):
        dist = [view_dist([float(v) for v in p], c) for p in r]
        assert g[0] == furthest(dist) and same(g[1:], dist)
        picks.append(g[0])
    assert picks == [2, 3, 4, 3, 2, 0, MAX_OBS - 1, 0]
    d0, d1 = got[0][1:], got[1][1:]
    assert d0[1] == d0[2] == max(d0) and d1[0] == d1[2] == d1[3] == max(d1)  # the ties are ties in the distances


def test_projection_skips(native):
    """pt_cam.z of 0, -0.0, the least positive double and NaN; pc on each side of each of the four borders."""
    cam = small_cam()
    border = 24
    head = hx(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["width"], cam["height"], border)
    O = [0.0, 0.0, 0.0]
    cases = [[0.0, 0.0, z] for z in (0.0, -0.0, up(0.0), float("nan"), -1.0, 1.0)]
    # the x (y) at depth 1 whose pixel is the first at or above a bound, and its neighbour below
    for axis, f, c0, bounds in ((0, cam["fx"], cam["cx"], (border, cam["width"] - border)),
                                (1, cam["fy"], cam["cy"], (border, cam["height"] - border))):
        for b in bounds:
            x = (b - c0) / f
            while f * x + c0 >= b:
                x = down(x)
            while f * x + c0 < b:
                x = up(x)
            for v in (x, down(x)):
                p = [0.05, 0.02, 1.0]
                p[axis] = v
                cases.append(p)
    got = native(["P " + head + " " + hx(EYE, O, p) for p in cases])
    want = [observe_project(cam, border, EYE, O, p) for p in cases]
    for g, (fate, pc) in zip(got, want):
        assert g[0] == fate and same(g[1:], pc)
    # z = 5e-324 passes the z test (its pixel is (cx, cy)); a NaN passes it too and fails the frame test
    assert [w[0] for w in want[:6]] == [1, 1, 0, 2, 1, 0]
    assert [w[0] for w in want[6:]] == [0, 2, 2, 0, 0, 2, 2, 0]


# -------------------------------------------------------------------- ABI ----
def test_header_library_and_binding_carry_the_entry_point(built):
    import livo_amd
    txt = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", livo_amd.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"^int livo_vio_observe\(", txt, flags=re.M) and "livo_vio_observe" in livo_amd.SIGNATURES
    assert re.search(r"\bT livo_vio_observe\b", out)
    assert livo_amd.load().livo_abi_version() == int(re.search(r"#define LIVO_ABI_VERSION (\d+)", txt).group(1)) == 9
    assert hasattr(livo_amd.Context, "vio_observe")
    for name, bit in (("BEHIND", BEHIND), ("OUT_OF_FRAME", OUT_OF_FRAME), ("POSE", POSE), ("PIXEL", PIXEL),
                      ("DELETED", DELETED), ("ADDED", ADDED)):
        assert int(re.search(rf"#define LIVO_VOBS_{name}\s+(\d+)", txt).group(1)) == bit == getattr(livo_amd, "VOBS_" + name)


def test_struct_layouts_match_c(tmp_path):
    import livo_amd
    fields = {"livo_vobs_point": list(OBS_DTYPE.names), "livo_vobs_stats": list(OBS_STAT_FIELDS)}
    src = tmp_path / "vo.c"
    body = "".join(f'printf("%zu ", sizeof({s}));' + "".join(f'printf("%zu ", offsetof({s}, {f}));' for f in fs)
                   for s, fs in fields.items())
    src.write_text('#include "livo.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){' + body +
                   'printf("%zu\\n", _Alignof(livo_vobs_point));return 0;}\n')
    exe = tmp_path / "vo"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    dt = livo_amd.VOBS_POINT_DTYPE
    want = [dt.itemsize] + [dt.fields[f][1] for f in dt.names]
    want += [C.sizeof(livo_amd.VobsStats)] + [getattr(livo_amd.VobsStats, f).offset for f in OBS_STAT_FIELDS] + [8]
    assert got == want and dt == OBS_DTYPE and dt.itemsize == 56
    assert tuple(f for f, _ in livo_amd.VobsStats._fields_) == OBS_STAT_FIELDS


def test_null_context_returns_invalid(built):
    import livo_amd
    L = livo_amd.load()
    ids = np.zeros(1, np.int32)
    assert L.livo_vio_observe(None, 0, 0, None, None, None, None) == -1
    assert L.livo_vio_observe(None, 0, 1, livo_amd._ptr(ids), None, None, None) == -1


# ------------------------------------------------- the model, on its own ----
def test_model_evicts_and_appends_in_list_order():
    """ObserveModel on a hand-made map: a point at 20 observations loses the furthest one and keeps the order
    of the rest; without add_flag it drops to 19."""
    cam = small_cam()
    img = np.random.default_rng(1).integers(0, 255, (128, 160), dtype=np.uint8)
    m = ObserveModel(cam, 4)
    for k in range(MAX_OBS):
        m.add_frame(k, np.eye(3), [-0.01 * (k + 1) if k != 7 else -0.3, 0.0, 0.0], img)
    m.add_frame(50, np.eye(3), [0.0, 0.0, 0.0], img)
    pts = np.zeros(2, [("x", F32), ("y", F32), ("z", F32), ("score", F32), ("u", F64), ("v", F64), ("voxel", np.int64, (3,))])
    pts["z"], pts["u"], pts["v"] = 5.0, [78.0, 140.0], 63.0  # pc = (cx, cy): 0.9 and 61.3 pixels from the stored px
    m.add(0, pts, np.zeros((2, 48), F32))
    for k in range(1, MAX_OBS):
        m.add(k, pts, np.full((2, 48), float(k), F32), [0, 1], [0, 0])
    rec, stats = m.observe(50, [1, 0], [2, 1])
    assert list(rec["flags"]) == [PIXEL | DELETED | ADDED, DELETED] and list(rec["n_obs"]) == [20, 19]
    assert list(rec["deleted_index"]) == [7, 7] and list(rec["deleted_frame_id"]) == [7, 7]
    assert [o["frame_id"] for o in m.points[1]["obs"]] == [k for k in range(MAX_OBS) if k != 7] + [50]
    assert [o["frame_id"] for o in m.points[0]["obs"]] == [k for k in range(MAX_OBS) if k != 7]
    assert m.points[1]["obs"][-1]["level"] == 2 and m.points[1]["obs"][7]["patch"][0] == 8.0
    assert stats == {"n_in": 2, "behind": 0, "out_of_frame": 0, "pose_flagged": 0, "pixel_flagged": 1, "added": 1,
                     "deleted": 2, "deleted_without_add": 1, "n_obs_total": 39}
