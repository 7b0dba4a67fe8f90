"""CPU checks of the sensor-handler entry points (livo_ingest_params_default, livo_frame_ingest_livox /
_cloud, livo_frame_info / _dump / _take): declared, exported and bound; the structs agree between C
and ctypes; refused arguments come back as codes before the context is read; without a device the
calls answer LIVO_E_HIP; the ABI version is still 9.  The refusals that need a live context (no
ingest yet, no propagation yet) and what the calls compute are in tests/test_gpu_ingest.py.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ingest_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "livo.h")
NEW = ("livo_ingest_params_default", "livo_frame_ingest_livox", "livo_frame_ingest_cloud", "livo_frame_info",
       "livo_frame_dump", "livo_frame_take")
INVALID, HIP, RANGE = -1, -2, -6


def test_header_library_and_binding_carry_the_entry_points(built):
    import livo_amd
    txt = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", livo_amd.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(rf"^int {name}\(", txt, flags=re.M) and name in livo_amd.SIGNATURES, name
        assert re.search(rf"\bT {name}\b", out), name
    assert livo_amd.load().livo_abi_version() == int(re.search(r"#define LIVO_ABI_VERSION (\d+)", txt).group(1)) == 9
    for m in ("frame_ingest_livox", "frame_ingest_cloud", "frame_take", "frame_dump", "frame_info"):
        assert hasattr(livo_amd.Context, m)
    assert "given_offset_time" in txt  # the header names the Velodyne branch that is not built
    facade = open(os.path.join(ROOT, "fast-livo-noted_amd", "host", "laser_mapping_gpu.hpp")).read()
    for word in ("livox_pcl_cbk", "standard_pcl_cbk", "livo_frame_take", "lidar_beg_time", "lidar_end_time"):
        assert word in facade, word


def test_struct_layouts_match_c(tmp_path):
    import livo_amd
    structs = {"livo_livox_point": livo_amd.LivoxPoint, "livo_cloud_layout": livo_amd.CloudLayout,
               "livo_ingest_params": livo_amd.IngestParams, "livo_ingest_info": livo_amd.IngestInfo}
    body = ""
    for cname, cls in structs.items():
        body += f'printf("%zu ", sizeof({cname}));'
        body += "".join(f'printf("%zu ", offsetof({cname}, {f}));' for f, _ in cls._fields_)
    src = tmp_path / "ingest.c"
    src.write_text('#include "livo.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){' + body +
                   'printf("%d %d %d %d", LIVO_LIDAR_AVIA, LIVO_LIDAR_VELO16, LIVO_LIDAR_OUST64, LIVO_LIDAR_XT32);'
                   "return 0;}\n")
    exe = tmp_path / "ingest"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for cls in structs.values():
        want += [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    want += [livo_amd.LIDAR_AVIA, livo_amd.LIDAR_VELO16, livo_amd.LIDAR_OUST64, livo_amd.LIDAR_XT32]
    assert got == want
    assert [C.sizeof(c) for c in structs.values()] == [20, 24, 24, 48]
    assert livo_amd.LIVOX_POINT_DTYPE == ic.LIVOX and ic.LIVOX.itemsize == 20


def test_params_default(built):
    import livo_amd
    assert livo_amd.load().livo_ingest_params_default(None) == INVALID
    p = livo_amd.ingest_params()
    assert (p.lidar_type, p.n_scans, p.point_filter_num, p.reserved, p.blind) == (1, 16, 2, 0, 0.01)


def _layout(L):
    import livo_amd
    return livo_amd.CloudLayout(L["point_step"], L["off_x"], L["off_y"], L["off_z"], L["off_intensity"], L["off_time"])


def test_refused_arguments(built):
    import livo_amd
    L = livo_amd.load()
    fake = C.c_void_p(8)  # never dereferenced: the refused argument is found first
    info = livo_amd.IngestInfo()
    m = ic.livox_msg(10, "all")
    P = livo_amd.ingest_params
    ok = P()
    livox = lambda ctx, p, pts, n: L.livo_frame_ingest_livox(ctx, C.byref(p) if p else None, pts, n, C.byref(info))
    assert livox(None, ok, m.ctypes.data, 10) == INVALID
    assert livox(fake, None, m.ctypes.data, 10) == INVALID
    assert livox(fake, ok, None, 10) == INVALID
    assert livox(fake, ok, m.ctypes.data, -1) == INVALID
    assert livox(fake, P(point_filter_num=0), m.ctypes.data, 10) == INVALID
    assert livox(fake, P(n_scans=-1), m.ctypes.data, 10) == INVALID
    for t in (0, 5, -1, 2, 3, 4):  # unknown, or a PointCloud2 type
        assert livox(fake, P(lidar_type=t), m.ctypes.data, 10) == INVALID, t
    assert livox(fake, ok, m.ctypes.data, 2**31 - 256) == RANGE

    lay = ic.LAYOUTS["hesai"]
    d = ic.cloud_msg(ic.XT32, 10, lay)
    cloud = lambda ctx, p, data, n, l: L.livo_frame_ingest_cloud(ctx, C.byref(p) if p else None, data, n,
                                                                 C.byref(l) if l else None, C.byref(info))
    xt = P(lidar_type=4)
    assert cloud(None, xt, d.ctypes.data, 10, _layout(lay)) == INVALID
    assert cloud(fake, None, d.ctypes.data, 10, _layout(lay)) == INVALID
    assert cloud(fake, xt, None, 10, _layout(lay)) == INVALID
    assert cloud(fake, xt, d.ctypes.data, 10, None) == INVALID
    assert cloud(fake, xt, d.ctypes.data, -1, _layout(lay)) == INVALID
    assert cloud(fake, P(lidar_type=4, point_filter_num=0), d.ctypes.data, 10, _layout(lay)) == INVALID
    assert cloud(fake, P(lidar_type=4, n_scans=-2), d.ctypes.data, 10, _layout(lay)) == INVALID
    for t in (1, 0, 5):  # AVIA is the other call's; unknown types
        assert cloud(fake, P(lidar_type=t), d.ctypes.data, 10, _layout(lay)) == INVALID, t
    assert cloud(fake, xt, d.ctypes.data, 2**31 - 256, _layout(lay)) == RANGE
    # offsets that do not fit in point_step: a float needs 4 bytes, XT32's timestamp 8
    for key, bad in (("off_x", 29), ("off_y", -1), ("off_z", 32), ("off_intensity", 30), ("off_time", 25),
                     ("point_step", 0), ("point_step", 23), ("point_step", 241)):
        assert cloud(fake, xt, d.ctypes.data, 10, _layout({**lay, key: bad})) == INVALID, (key, bad)
    # VELO16's float time fits where XT32's double does not; its last point's time must be > 0
    vl = ic.LAYOUTS["velodyne"]
    v = ic.cloud_msg(ic.VELO16, 10, vl)
    for t in (0.0, -1.0, float("nan")):
        v[9, 18:22] = np.array([t], np.float32).view(np.uint8)
        assert cloud(fake, P(lidar_type=2), v.ctypes.data, 10, _layout(vl)) == INVALID, t

    nt, n, sid = C.c_int64(-5), C.c_int64(-5), C.c_int32(-5)
    assert L.livo_frame_info(None, C.byref(info)) == INVALID and L.livo_frame_info(fake, None) == INVALID
    assert L.livo_frame_dump(None, None, 0, C.byref(n)) == INVALID and L.livo_frame_dump(fake, None, 0, None) == INVALID
    take = lambda ctx, leaf, s, t: L.livo_frame_take(ctx, 0.0, 1, leaf, s, None, None, 0, None, t)
    assert take(None, 0.5, C.byref(sid), C.byref(nt)) == INVALID
    assert take(fake, 0.5, C.byref(sid), None) == INVALID
    assert take(fake, float("nan"), C.byref(sid), C.byref(nt)) == INVALID
    assert (nt.value, n.value, sid.value) == (-5, -5, -5)


def test_without_a_device_every_call_fails_loudly(built):
    import livo_amd
    L = livo_amd.load()
    h = C.c_void_p()
    if L.livo_ctx_create(0, None, C.byref(h)) == 0:  # a device is present: the GPU tests hold the calls
        L.livo_ctx_destroy(h)
        pytest.skip("GPU present")
    fake = C.c_void_p(8)  # no context can exist without a device; the calls answer before they read it
    info = livo_amd.IngestInfo()
    m = ic.livox_msg(10, "all")
    assert L.livo_frame_ingest_livox(fake, C.byref(livo_amd.ingest_params()), m.ctypes.data, 10, C.byref(info)) == HIP
    lay = ic.LAYOUTS["ouster"]
    d = ic.cloud_msg(ic.OUST64, 10, lay)
    assert L.livo_frame_ingest_cloud(fake, C.byref(livo_amd.ingest_params(lidar_type=3)), d.ctypes.data, 10,
                                     C.byref(_layout(lay)), C.byref(info)) == HIP
    n, sid = C.c_int64(), C.c_int32()
    assert L.livo_frame_info(fake, C.byref(info)) == HIP
    assert L.livo_frame_dump(fake, None, 0, C.byref(n)) == HIP
    assert L.livo_frame_take(fake, 0.0, 1, 0.5, C.byref(sid), None, None, 0, None, C.byref(n)) == HIP
    assert L.livo_frame_take(fake, 0.0, 0, 0.5, None, None, None, 0, None, C.byref(n)) == HIP
