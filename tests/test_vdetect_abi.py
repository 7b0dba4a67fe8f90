"""CPU checks of livo_vio_detect and livo_vmap_release_frames: both are declared, exported and bound with as
many arguments as the header gives them, still at ABI version 9; livo_vdetect_params and livo_vdetect_stats
agree between C and ctypes, field by field; null arguments come back as a code; and the arithmetic that the
two small kernels of the frame share with the host path (csrc/vmap_model.h: vm_make_frame, vm_make_point,
vm_make_obs, compiled for the host by tests/native/vdetect_point_check.cpp) equals, bit for bit, the
restatements of tests/test_vmatch_abi.py (frame_pos, cam2world), tests/test_rgb_cloud_abi.py (restate_pose)
and tests/test_vis_select_abi.py (restate_voxel).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from test_rgb_cloud_abi import restate_pose
from test_vis_select_abi import restate_voxel
from test_vmatch_abi import cam2world, frame_pos, hx, pylist, same, small_cam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "livo.h")
F32, F64 = np.float32, np.float64
NEW = ("livo_vio_detect", "livo_vmap_release_frames")
PARAM_FIELDS = ("grid_size", "ncc_en", "ncc_thre", "outlier_threshold")
STAT_FIELDS = ("match", "select", "update", "observe", "n_matched", "n_new", "first_new_id", "pad_")


# -------------------------------------------------------------------- ABI ----
def header_arity(txt, name):
    """The number of parameters of `name`'s declaration in the header."""
    m = re.search(rf"^int {name}\((.*?)\);", txt, flags=re.M | re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_library_and_binding_carry_the_entry_points(built):
    import livo_amd
    txt = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", livo_amd.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW:
        assert name in livo_amd.SIGNATURES and re.search(rf"\bT {name}\b", out)
        res, args = livo_amd.SIGNATURES[name]
        assert res is C.c_int and len(args) == header_arity(txt, name)
    assert header_arity(txt, "livo_vio_detect") == 11 and header_arity(txt, "livo_vmap_release_frames") == 4
    assert livo_amd.load().livo_abi_version() == int(re.search(r"#define LIVO_ABI_VERSION (\d+)", txt).group(1)) == 9
    assert hasattr(livo_amd.Context, "vio_detect") and hasattr(livo_amd.Context, "vmap_release_frames")
    sig = livo_amd.SIGNATURES["livo_vio_detect"][1]
    assert sig[6] == C.POINTER(livo_amd.VdetectParams) and sig[10] == C.POINTER(livo_amd.VdetectStats)


def test_struct_layouts_match_c(tmp_path):
    import livo_amd
    fields = {"livo_vdetect_params": PARAM_FIELDS, "livo_vdetect_stats": STAT_FIELDS}
    body = "".join(f'printf("%zu ", sizeof({s}));' + "".join(f'printf("%zu ", offsetof({s}, {f}));' for f in fs)
                   for s, fs in fields.items())
    src = tmp_path / "vd.c"
    src.write_text('#include "livo.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){' + body +
                   'printf("%zu\\n", _Alignof(livo_vdetect_stats));return 0;}\n')
    exe = tmp_path / "vd"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for cls, fs in ((livo_amd.VdetectParams, PARAM_FIELDS), (livo_amd.VdetectStats, STAT_FIELDS)):
        assert tuple(f for f, _ in cls._fields_) == fs
        want += [C.sizeof(cls)] + [getattr(cls, f).offset for f in fs]
    assert got == want + [8]
    S = livo_amd.VdetectStats
    assert C.sizeof(livo_amd.VdetectParams) == 24
    assert C.sizeof(S) == sum(C.sizeof(t) for t in (livo_amd.VmatchStats, livo_amd.VisStats, livo_amd.VioStats,
                                                    livo_amd.VobsStats)) + 24


def test_null_arguments_return_invalid(built):
    import livo_amd
    L = livo_amd.load()
    n = C.c_int64(7)
    assert L.livo_vio_detect(None, -1, 0, None, None, None, None, None, 160, 128, None) == -1
    assert L.livo_vmap_release_frames(None, None, 0, C.byref(n)) == -1 and n.value == 7


# ----------------------------------------------------------- native cases ----
@pytest.fixture(scope="module")
def native(tmp_path_factory):
    d = tmp_path_factory.mktemp("vdetect_native")
    exe = d / "vdetect_point_check"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "fast-livo-noted_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "vdetect_point_check.cpp"), "-o", str(exe)])

    def run(lines):
        path = d / "cases.txt"
        path.write_text("\n".join(lines) + "\n")
        out = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
        rows = [ln.split() for ln in out.stdout.split("\n") if ln]
        assert len(rows) == len(lines)
        return [[int(t) if re.fullmatch(r"-?\d+", t) else float.fromhex(t) for t in r[1:]] for r in rows]

    return run


def test_frame_of_a_state(native):
    """vm_make_frame(frame_cam(p, state)): Rcw = Rci Rwi^T, Pcw = -Rcw Pwi + Pci and the position -Rcw^T Pcw,
    for synth's extrinsic at its states and for general rotations, where the order of the sums shows."""
    from livo_amd import synth
    cam = small_cam()
    head = hx(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["width"], cam["height"])
    rng = np.random.default_rng(41)
    cases = [(synth.R_CI, synth.P_CI, synth.make_state(k)["rot"], synth.make_state(k)["pos"]) for k in range(4)]
    for _ in range(40):
        cases.append((synth.so3_exp(rng.normal(0, 0.8, 3)), rng.normal(0, 0.3, 3), synth.so3_exp(rng.normal(0, 0.8, 3)),
                      rng.normal(0, 20.0, 3)))
    got = native([f"F {hx(7 + i)} {head} " + hx(*c) for i, c in enumerate(cases)])
    moved = 0
    for i, (g, c) in enumerate(zip(got, cases)):
        Rcw, Pcw = restate_pose(*c)
        pos = frame_pos(pylist(Rcw), [float(x) for x in Pcw])
        assert g[0] == 7 + i and same(g[1:10], Rcw) and same(g[10:13], Pcw) and same(g[13:16], pos)
        moved += not same(pos, -Rcw.T @ Pcw)  # the matrix product sums in another order: some last bits differ
    assert moved > 0


def test_fresh_point_and_its_observation(native):
    """vm_make_point / vm_make_obs on a selected record: the float position widened, value = score, the voxel
    key of a negative coordinate (-1.0 m is key -3, not floor's -2), one observation at level 0 with
    f = cam2world(u, v)."""
    cam = small_cam()
    head = hx(cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    rng = np.random.default_rng(42)
    xyz = [[-1.0, 0.3, 5.0], [-0.3, -0.5, 0.0], [1.3, -123.456, 6.0]] + [list(rng.normal(0, 8.0, 3)) for _ in range(40)]
    uv = [[78.7, 63.6], [24.0, 103.99]] + [list(rng.uniform(24, 136, 2)) for _ in range(41)]
    score = [0.0, 1.5] + list(rng.uniform(0, 4000, 41))
    got = native([f"N {head} {hx(100 + i, i % 5)} " + hx(p, s, q) for i, (p, s, q) in enumerate(zip(xyz, score, uv))])
    for i, (g, p, s, q) in enumerate(zip(got, xyz, score, uv)):
        p32 = np.asarray(p, F32)
        assert same(g[0:3], p32.astype(F64)) and g[3] == float(F32(s)) and g[4] == 1
        assert g[5:8] == [int(k) for k in restate_voxel(p32)]
        assert g[8:11] == [100 + i, 0, i % 5] and same(g[11:13], q) and same(g[13:16], cam2world(cam, q[0], q[1]))
    assert got[0][5:8] == [-3, 0, 10] and got[1][5:8] == [-1, -2, 0]
    assert any(k < 0 and k != int(np.floor(float(F32(v)) / 0.5)) for g, p in zip(got, xyz) for k, v in zip(g[5:8], p))
