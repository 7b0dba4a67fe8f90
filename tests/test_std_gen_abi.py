"""livo_std_gen_* on the host: the defaults, the struct sizes against ctypes, and every refusal that is found
before the device is touched."""
import ctypes as C
import math

import numpy as np
import pytest

import std_gen_cases as G

E_INVALID, E_RANGE = -1, -6


@pytest.fixture(scope="module")
def lib():
    import livo_amd
    return livo_amd, livo_amd.load()


def test_defaults_are_read_parameters(lib):
    livo_amd, _ = lib
    p = livo_amd.std_gen_params()
    for k, v in G.DEFAULTS.items():
        assert getattr(p, k) == v, k
    assert livo_amd.std_gen_params(voxel_size=1.0).voxel_size == 1.0


def test_struct_sizes(lib):
    livo_amd, _ = lib
    assert C.sizeof(livo_amd.StdGenParams) == 11 * 8 + 4 * 4
    assert C.sizeof(livo_amd.StdGenStats) == 9 * 8
    assert C.sizeof(livo_amd.StdCorner) == 32 == livo_amd.STD_CORNER_DTYPE.itemsize == G.CORNER.itemsize
    assert livo_amd.STD_GEN_MAX_IMAGE == 80 and livo_amd.STD_GEN_MAX_NEAR == 64


BAD = [
    (dict(voxel_size=2.5), E_RANGE),                        # 2.5 * sqrt(17) >= 10
    (dict(voxel_size=10.0 / math.sqrt(17.0)), E_RANGE),
    (dict(proj_image_resolution=0.2), E_RANGE),             # an image side of 87 > 80
    (dict(descriptor_max_len=2100.0), E_RANGE),             # the packed side key
    (dict(descriptor_max_len=2000.0, std_side_resolution=0.001), E_RANGE),
    (dict(descriptor_near_num=2), E_INVALID),
    (dict(descriptor_near_num=65), E_INVALID),
    (dict(maximum_corner_num=0), E_INVALID),
    (dict(voxel_init_num=-1), E_INVALID),
    (dict(voxel_size=0.0), E_INVALID),
    (dict(proj_image_resolution=0.0), E_INVALID),
    (dict(std_side_resolution=0.0), E_INVALID),
] + [(dict([(k, v)]), E_INVALID)
     for k in ("voxel_size", "plane_detection_thre", "plane_merge_normal_thre", "proj_image_resolution", "proj_dis_min",
               "proj_dis_max", "corner_thre", "non_max_suppression_radius", "descriptor_min_len", "descriptor_max_len",
               "std_side_resolution")
     for v in (-1.0, math.nan, math.inf)]


@pytest.mark.parametrize("kw,code", BAD, ids=[f"{list(k)[0]}={list(k.values())[0]}" for k, _ in BAD])
def test_parameter_refusals_come_before_the_context(lib, kw, code):
    livo_amd, L = lib
    p = livo_amd.std_gen_params(**kw)
    fake = C.c_void_p(1)  # never read: the parameters are refused first
    assert L.livo_std_generate(fake, C.byref(p), None) == code


def test_null_and_host_point_refusals(lib):
    livo_amd, L = lib
    p = livo_amd.std_gen_params()
    assert L.livo_std_gen_params_default(None) == E_INVALID
    assert L.livo_std_generate(None, C.byref(p), None) == E_INVALID
    assert L.livo_std_generate(C.c_void_p(1), None, None) == E_INVALID
    assert L.livo_std_key_add(None, 0) == E_INVALID
    assert L.livo_std_key_clear(None) == E_INVALID
    assert L.livo_std_key_count(None, None) == E_INVALID
    fake = C.c_void_p(1)
    pts = np.zeros((4, 3), np.float32)
    ptr = pts.ctypes.data_as(C.c_void_p)
    assert L.livo_std_key_add_host(fake, ptr, -1, 12) == E_INVALID
    assert L.livo_std_key_add_host(fake, None, 4, 12) == E_INVALID
    assert L.livo_std_key_add_host(fake, ptr, 4, 8) == E_INVALID     # a stride below three floats
    for bad in (np.nan, np.inf, -np.inf):
        pts[2, 1] = bad
        assert L.livo_std_key_add_host(fake, ptr, 4, 12) == E_INVALID  # a non-finite point
