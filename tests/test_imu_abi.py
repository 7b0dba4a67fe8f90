"""CPU checks of the IMU entry points (livo_imu_params_default / _inited, livo_imu_init,
livo_imu_propagate, livo_imu_propagate_batch, livo_scan_preprocess_imu): declared, exported and
bound; the four new structs agree between C and ctypes; refused arguments come back as codes;
without a device the compute calls answer LIVO_E_HIP while livo_imu_init, host code, succeeds;
the ABI version is still 9.  tests/test_gpu_imu.py holds what the calls compute.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "livo.h")
NEW = ("livo_imu_params_default", "livo_imu_params_inited", "livo_imu_init", "livo_imu_propagate",
       "livo_imu_propagate_batch", "livo_scan_preprocess_imu")


def test_header_library_and_binding_carry_the_entry_points(built):
    import livo_amd
    txt = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", livo_amd.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(rf"^int {name}\(", txt, flags=re.M) and name in livo_amd.SIGNATURES, name
        assert re.search(rf"\bT {name}\b", out), name
    assert livo_amd.load().livo_abi_version() == int(re.search(r"#define LIVO_ABI_VERSION (\d+)", txt).group(1)) == 9
    for m in ("imu_propagate", "imu_propagate_batch", "scan_preprocess_imu"):
        assert hasattr(livo_amd.Context, m)
    assert callable(livo_amd.imu_init)
    facade = open(os.path.join(ROOT, "fast-livo-noted_amd", "host", "laser_mapping_gpu.hpp")).read()
    for word in ("imu_params", "imu_carry", "Process2", "livo_imu_propagate", "livo_scan_preprocess_imu"):
        assert word in facade, word


def test_struct_layouts_match_c(tmp_path):
    import livo_amd
    structs = {"livo_imu_sample": livo_amd.ImuSample, "livo_imu_params": livo_amd.ImuParams,
               "livo_imu_carry": livo_amd.ImuCarry, "livo_imu_job": livo_amd.ImuJob}
    body = ""
    for cname, cls in structs.items():
        body += f'printf("%zu ", sizeof({cname}));'
        body += "".join(f'printf("%zu ", offsetof({cname}, {f}));' for f, _ in cls._fields_)
    src = tmp_path / "imu.c"
    src.write_text('#include "livo.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){' + body +
                   'printf("%d %d %d", LIVO_IMU_INIT_COLLECTING, LIVO_IMU_INIT_RESET, LIVO_IMU_INIT_DONE);'
                   "return 0;}\n")
    exe = tmp_path / "imu"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for cls in structs.values():
        want += [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    want += [livo_amd.IMU_INIT_COLLECTING, livo_amd.IMU_INIT_RESET, livo_amd.IMU_INIT_DONE]
    assert got == want
    assert [C.sizeof(c) for c in structs.values()] == [56, 120, 112, 32]


def _args():
    import livo_amd
    import imu_cases as ic
    job, params, carry, state = ic.make_case(3)
    imu = np.ascontiguousarray(job[0])
    j = livo_amd.ImuJob(imu.ctypes.data, 3, job[1], job[2])
    return (imu, j, livo_amd.imu_params_to_c(params), livo_amd.imu_carry_to_c(carry), livo_amd.state_to_c(state))


def test_params_default_and_inited(built):
    import livo_amd
    L = livo_amd.load()
    assert L.livo_imu_params_default(None) == -1 and L.livo_imu_params_inited(None) == -1
    p = livo_amd.imu_params_from_c(livo_amd.imu_params_to_c(None))
    for k in ("cov_acc", "cov_gyr", "cov_bias_gyr", "cov_bias_acc"):
        assert np.array_equal(p[k], np.full(3, 0.1))
    assert np.array_equal(p["mean_acc"], [0.0, 0.0, -1.0])
    q = livo_amd.imu_params_inited({"mean_acc": [0.1, 0.2, 9.8]})
    assert np.array_equal(q["cov_acc"], np.full(3, 0.01)) and np.array_equal(q["cov_gyr"], np.full(3, 0.01))
    assert np.array_equal(q["cov_bias_gyr"], np.full(3, 1e-4)) and np.array_equal(q["cov_bias_acc"], np.full(3, 1e-4))
    assert np.array_equal(q["mean_acc"], [0.1, 0.2, 9.8])


def test_null_and_negative_arguments_return_invalid(built):
    import livo_amd
    L = livo_amd.load()
    imu, j, p, cy, st = _args()
    n = C.c_int32(-5)
    fake = C.c_void_p(8)  # never dereferenced: the refused argument is found first
    R = (C.byref(j), C.byref(p), C.byref(cy), C.byref(st))
    assert L.livo_imu_propagate(None, *R, None, 0, C.byref(n)) == -1
    for k in range(4):
        a = list(R)
        a[k] = None
        assert L.livo_imu_propagate(fake, *a, None, 0, C.byref(n)) == -1, k
    assert L.livo_imu_propagate(fake, *R, None, -1, C.byref(n)) == -1
    bad = livo_amd.ImuJob(imu.ctypes.data, -1, j.pcl_beg_time, j.pcl_end_time)
    assert L.livo_imu_propagate(fake, C.byref(bad), *R[1:], None, 0, C.byref(n)) == -1
    bad = livo_amd.ImuJob(None, 2, j.pcl_beg_time, j.pcl_end_time)
    assert L.livo_imu_propagate(fake, C.byref(bad), *R[1:], None, 0, C.byref(n)) == -1
    B = (C.byref(j), C.byref(p), C.byref(cy), C.byref(st))
    assert L.livo_imu_propagate_batch(None, 1, *B, None, 0, None) == -1
    assert L.livo_imu_propagate_batch(fake, -1, *B, None, 0, None) == -1
    for k in range(4):
        a = list(B)
        a[k] = None
        assert L.livo_imu_propagate_batch(fake, 1, *a, None, 0, None) == -1, k
    # a table that would not fit is refused before anything runs: 3 samples need 4 rows
    rows = np.zeros((3, 22))
    assert L.livo_imu_propagate_batch(fake, 1, *B, rows.ctypes.data, 3, None) == -6
    assert n.value == -5
    sid, nd = C.c_int32(), C.c_int64()
    raw = np.zeros((2, 5), np.float32)
    assert L.livo_scan_preprocess_imu(None, raw.ctypes.data, 2, 0.5, C.byref(sid), None, None, 0, C.byref(nd)) == -1
    assert L.livo_scan_preprocess_imu(fake, raw.ctypes.data, -1, 0.5, C.byref(sid), None, None, 0, C.byref(nd)) == -1
    assert L.livo_scan_preprocess_imu(fake, None, 2, 0.5, C.byref(sid), None, None, 0, C.byref(nd)) == -1
    assert L.livo_scan_preprocess_imu(fake, raw.ctypes.data, 2, 0.5, None, None, None, 0, C.byref(nd)) == -1
    assert L.livo_scan_preprocess_imu(fake, raw.ctypes.data, 2, float("nan"), C.byref(sid), None, None, 0,
                                      C.byref(nd)) == -1
    it, status = C.c_int32(1), C.c_int32()
    mg = np.zeros(3)
    assert L.livo_imu_init(None, None, 3, C.byref(p), C.byref(it), mg.ctypes.data, C.byref(st), C.byref(status)) == -1
    assert L.livo_imu_init(None, imu.ctypes.data, -1, C.byref(p), C.byref(it), mg.ctypes.data, C.byref(st),
                           C.byref(status)) == -1
    assert L.livo_imu_init(None, imu.ctypes.data, 3, None, C.byref(it), mg.ctypes.data, C.byref(st),
                           C.byref(status)) == -1
    assert L.livo_imu_init(None, imu.ctypes.data, 3, C.byref(p), C.byref(it), mg.ctypes.data, C.byref(st), None) == -1


def test_without_a_device_compute_fails_loudly_and_init_runs(built):
    import livo_amd
    L = livo_amd.load()
    imu, j, p, cy, st = _args()
    it, status = C.c_int32(1), C.c_int32(-1)
    mg = np.zeros(3)
    # host code: runs with or without a device, and without a context
    assert L.livo_imu_init(None, imu.ctypes.data, 3, C.byref(p), C.byref(it), mg.ctypes.data, C.byref(st),
                           C.byref(status)) == 0
    assert (status.value, it.value) in ((0, 4), (1, 1))  # three samples: collecting, or moving and reset
    h = C.c_void_p()
    if L.livo_ctx_create(0, None, C.byref(h)) == 0:  # a device is present: the GPU tests hold the calls
        L.livo_ctx_destroy(h)
        pytest.skip("GPU present")
    fake = C.c_void_p(8)  # no context can exist without a device; the calls answer before they read it
    n = C.c_int32()
    assert L.livo_imu_propagate(fake, C.byref(j), C.byref(p), C.byref(cy), C.byref(st), None, 0, C.byref(n)) == -2
    assert L.livo_imu_propagate_batch(fake, 1, C.byref(j), C.byref(p), C.byref(cy), C.byref(st), None, 0, None) == -2
    sid, nd = C.c_int32(), C.c_int64()
    raw = np.zeros((2, 5), np.float32)
    assert L.livo_scan_preprocess_imu(fake, raw.ctypes.data, 2, 0.5, C.byref(sid), None, None, 0, C.byref(nd)) == -2
