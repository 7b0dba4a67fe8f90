"""CPU checks of the LiDAR-to-camera hand-off (livo_cloud_publish, livo_cloud_info_get, LIVO_CLOUD_WORLD and
LIVO_CLOUD_WORLD_DOWN): the entry points are declared, exported and bound, the two ids and livo_cloud_info agree
between C and ctypes, the arguments refused before any device work come back as codes, and the ABI version is
still 9.  tests/test_gpu_world_cloud.py holds what the calls compute.
"""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "livo.h")
NEW = ("livo_cloud_publish", "livo_cloud_info_get")


def test_header_library_and_binding_carry_the_entry_points(built):
    import livo_amd
    txt = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", livo_amd.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(rf"^int {name}\(", txt, flags=re.M) and name in livo_amd.SIGNATURES
        assert re.search(rf"\bT {name}\b", out)
    assert livo_amd.load().livo_abi_version() == int(re.search(r"#define LIVO_ABI_VERSION (\d+)", txt).group(1)) == 9
    for m in ("cloud_publish", "cloud_info"):
        assert hasattr(livo_amd.Context, m)
    sig = livo_amd.SIGNATURES["livo_cloud_publish"]
    assert sig[0] is C.c_int and sig[1][1] is C.c_int32 and sig[1][3] is C.c_float
    assert sig[1][4] is C.POINTER(livo_amd.CloudInfo) is livo_amd.SIGNATURES["livo_cloud_info_get"][1][1]


def test_constants_and_struct_layout_match_c(tmp_path):
    import livo_amd
    fields = [f for f, _ in livo_amd.CloudInfo._fields_]
    assert fields == ["n", "n_down", "down_filtered", "pad_", "device_bytes"]
    src = tmp_path / "wc.c"
    src.write_text('#include "livo.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){'
                   'printf("%d %d %zu ", LIVO_CLOUD_WORLD, LIVO_CLOUD_WORLD_DOWN, sizeof(livo_cloud_info));' +
                   "".join(f'printf("%zu ", offsetof(livo_cloud_info, {f}));' for f in fields) + "return 0;}\n")
    exe = tmp_path / "wc"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:3] == [livo_amd.CLOUD_WORLD, livo_amd.CLOUD_WORLD_DOWN, C.sizeof(livo_amd.CloudInfo)]
    assert got[:3] == [0x40000000, 0x40000001, 32]
    assert got[3:] == [getattr(livo_amd.CloudInfo, f).offset for f in fields]
    # the ids fit the frame stages' int32_t scan_id
    assert C.c_int32(livo_amd.CLOUD_WORLD_DOWN).value == livo_amd.CLOUD_WORLD_DOWN


def test_null_and_invalid_arguments_return_invalid(built):
    import livo_amd
    L = livo_amd.load()
    st = livo_amd.State()
    info = livo_amd.CloudInfo(n=-7)
    fake = C.c_void_p(8)  # never dereferenced: the refused argument is found first
    assert L.livo_cloud_publish(None, -1, C.byref(st), 0.2, C.byref(info)) == -1
    assert L.livo_cloud_publish(fake, -1, None, 0.2, C.byref(info)) == -1
    for leaf in (float("nan"), float("inf"), float("-inf")):
        assert L.livo_cloud_publish(fake, -1, C.byref(st), leaf, C.byref(info)) == -1
    for sid in (livo_amd.CLOUD_WORLD, livo_amd.CLOUD_WORLD_DOWN):  # a published cloud is no source
        assert L.livo_cloud_publish(fake, sid, C.byref(st), 0.2, C.byref(info)) == -1
    assert L.livo_cloud_info_get(None, C.byref(info)) == -1
    assert L.livo_cloud_info_get(fake, None) == -1
    assert info.n == -7
