"""CPU checks of the loop search's C ABI (livo_std_*): the structures agree between C (a probe compiled
against include/livo.h) and the ctypes mirrors, the entry points are exported and bound, and the
refusals that need no device come back as codes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
E_INVALID, E_RANGE = -1, -6

STRUCTS = {
    "livo_std_params": ("StdParams", ["skip_near_num", "candidate_num", "rough_dis_threshold", "vertex_diff_threshold",
                                      "icp_threshold", "normal_threshold", "dis_threshold"]),
    "livo_std_desc": ("StdDesc", ["side_length", "vertex_A", "vertex_B", "vertex_C", "center", "vertex_attached",
                                  "frame_id", "pad"]),
    "livo_std_plane": ("StdPlane", ["xyz", "normal"]),
    "livo_std_pair": ("StdPair", ["src", "frame", "db_index"]),
    "livo_std_result": ("StdResult", ["frame", "n_candidates", "n_pairs", "candidate", "score", "rot", "t"]),
    "livo_std_candidate": ("StdCandidate", ["frame", "votes", "use_size", "max_vote", "max_vote_index", "score", "rot",
                                            "t"]),
    "livo_std_info": ("StdInfo", ["frames", "descs", "planes", "cells", "max_descs", "max_frames", "max_planes",
                                  "staged_descs", "staged_planes"]),
}
PROBE = "#include <stddef.h>\n#include <stdio.h>\n#include \"livo.h\"\nint main(void) {\n" + "".join(
    f'    printf("{t} %zu\\n", sizeof({t}));\n' + "".join(
        f'    printf("{t}.{f} %zu\\n", offsetof({t}, {f}));\n' for f in fs) for t, (_, fs) in STRUCTS.items()) + \
    '    printf("max %d %d\\n", LIVO_STD_MAX_FRAMES, LIVO_STD_MAX_CANDIDATES);\n    return 0;\n}\n'
FUNCS = {"livo_std_params_default": 1, "livo_std_reset": 5, "livo_std_stage": 5, "livo_std_search": 5,
         "livo_std_commit": 2, "livo_std_candidates": 4, "livo_std_matches": 5, "livo_std_info_get": 2,
         "livo_std_dump": 8}


def test_structs_match_the_ctypes_mirrors(built, tmp_path):
    import livo_amd
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-I" + INC, str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    seen = 0
    for ln in lines:
        key, val = ln.rsplit(" ", 1)
        if key.startswith("max"):
            assert ln == f"max {livo_amd.STD_MAX_FRAMES} {livo_amd.STD_MAX_CANDIDATES}" == "max 20000 64"
            continue
        t, _, f = key.partition(".")
        mirror = getattr(livo_amd, STRUCTS[t][0])
        want = C.sizeof(mirror) if not f else getattr(mirror, f).offset
        assert int(val) == want, (key, val, want)
        seen += 1
    assert seen == sum(1 + len(fs) for _, fs in STRUCTS.values())
    assert C.sizeof(livo_amd.StdDesc) == 152 == livo_amd.STD_DESC_DTYPE.itemsize
    assert C.sizeof(livo_amd.StdPlane) == 24 == livo_amd.STD_PLANE_DTYPE.itemsize
    assert C.sizeof(livo_amd.StdPair) == livo_amd.STD_PAIR_DTYPE.itemsize
    assert C.sizeof(livo_amd.StdCandidate) == livo_amd.STD_CANDIDATE_DTYPE.itemsize
    import std_cases
    assert std_cases.DESC == livo_amd.STD_DESC_DTYPE and std_cases.PLANE == livo_amd.STD_PLANE_DTYPE


def test_symbols_are_exported_and_bound(built):
    import livo_amd
    L = livo_amd.load()
    header = open(os.path.join(INC, "livo.h")).read()
    for name, nargs in FUNCS.items():
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == nargs and name in header
    for m in ("std_reset", "std_stage", "std_search", "std_commit", "std_candidates", "std_matches", "std_info",
              "std_dump"):
        assert callable(getattr(livo_amd.Context, m))
    assert livo_amd.load().livo_abi_version() == 9  # additive: the version stays


def test_defaults_are_read_parameters(built):
    import livo_amd
    import std_cases
    p = livo_amd.std_params()
    assert {f: getattr(p, f) for f, _ in p._fields_} == std_cases.DEFAULTS
    assert livo_amd.load().livo_std_params_default(None) == E_INVALID


FAKE = C.c_void_p(0x1000)  # never dereferenced: the refusal is found first


def test_null_arguments_are_refused(built):
    import livo_amd
    L = livo_amd.load()
    p = livo_amd.std_params()
    r, n, f, info = livo_amd.StdResult(), C.c_int64(), C.c_int32(), livo_amd.StdInfo()
    d, pl = livo_amd.StdDesc(), livo_amd.StdPlane()
    assert L.livo_std_reset(None, C.byref(p), 8, 8, 8) == E_INVALID
    assert L.livo_std_reset(FAKE, None, 8, 8, 8) == E_INVALID
    assert L.livo_std_stage(None, C.byref(d), 1, C.byref(pl), 1) == E_INVALID
    assert L.livo_std_stage(FAKE, None, 1, C.byref(pl), 1) == E_INVALID
    assert L.livo_std_stage(FAKE, C.byref(d), 1, None, 1) == E_INVALID
    assert L.livo_std_search(None, C.byref(r), None, 0, C.byref(n)) == E_INVALID
    assert L.livo_std_search(FAKE, None, None, 0, C.byref(n)) == E_INVALID
    assert L.livo_std_commit(None, C.byref(f)) == E_INVALID
    assert L.livo_std_candidates(None, None, 0, C.byref(n)) == E_INVALID
    assert L.livo_std_candidates(FAKE, None, 0, None) == E_INVALID
    assert L.livo_std_matches(None, 0, None, 0, C.byref(n)) == E_INVALID
    assert L.livo_std_matches(FAKE, 0, None, 0, None) == E_INVALID
    assert L.livo_std_info_get(None, C.byref(info)) == E_INVALID
    assert L.livo_std_info_get(FAKE, None) == E_INVALID
    assert L.livo_std_dump(None, None, 0, C.byref(n), -1, None, 0, None) == E_INVALID


@pytest.mark.parametrize("field,value", [("rough_dis_threshold", float("nan")), ("vertex_diff_threshold", float("inf")),
                                         ("icp_threshold", float("nan")), ("normal_threshold", -1.0),
                                         ("dis_threshold", float("-inf")), ("skip_near_num", -1), ("candidate_num", -1),
                                         ("candidate_num", 65)])
def test_bad_parameters_are_refused_before_the_context_is_read(built, field, value):
    import livo_amd
    p = livo_amd.std_params(**{field: value})
    assert livo_amd.load().livo_std_reset(FAKE, C.byref(p), 8, 8, 8) == E_INVALID


def test_bad_sizes_are_refused_before_the_context_is_read(built):
    import livo_amd
    L = livo_amd.load()
    p = livo_amd.std_params()
    assert L.livo_std_reset(FAKE, C.byref(p), 0, 8, 8) == E_INVALID
    assert L.livo_std_reset(FAKE, C.byref(p), 8, 0, 8) == E_INVALID
    assert L.livo_std_reset(FAKE, C.byref(p), 8, 8, 0) == E_INVALID
    assert L.livo_std_reset(FAKE, C.byref(p), 8, 20001, 8) == E_RANGE  # MAX_FRAME_N: the reference's vote array
    assert L.livo_std_reset(FAKE, C.byref(p), 1 << 31, 8, 8) == E_RANGE
    d = np.zeros(2, livo_amd.STD_DESC_DTYPE)
    pl = np.zeros(1, livo_amd.STD_PLANE_DTYPE)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.livo_std_stage(FAKE, ptr(d), -1, ptr(pl), 1) == E_INVALID
    assert L.livo_std_stage(FAKE, ptr(d), 2, ptr(pl), -1) == E_INVALID
    d["vertex_B"][1, 2] = np.nan
    assert L.livo_std_stage(FAKE, ptr(d), 2, ptr(pl), 1) == E_INVALID
    d["vertex_B"][1, 2] = 0.0
    d["side_length"][0, 1] = 2.0 ** 20
    assert L.livo_std_stage(FAKE, ptr(d), 2, ptr(pl), 1) == E_RANGE
    d["side_length"][0, 1] = 0.0
    pl["normal"][0, 0] = np.inf
    assert L.livo_std_stage(FAKE, ptr(d), 2, ptr(pl), 1) == E_INVALID
    assert L.livo_std_search(FAKE, C.byref(livo_amd.StdResult()), None, -1, None) == E_INVALID
