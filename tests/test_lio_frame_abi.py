"""CPU checks of livo_lio_frame: the entry point is declared, exported and bound, its structures
agree between C (a probe compiled against include/livo.h) and the ctypes mirrors, and the refusals
that need no device come back as codes."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
E_INVALID = -1  # LIVO_E_INVALID

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "livo.h"
#define S(t) printf(#t " %zu\n", sizeof(t))
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void) {
    S(livo_lio_params); O(livo_lio_params, filter_size_surf); O(livo_lio_params, match_leaf);
    O(livo_lio_params, filter_size_map_min); O(livo_lio_params, ekf_inited); O(livo_lio_params, first_scan);
    O(livo_lio_params, dense_map_en); O(livo_lio_params, prev_scan_id);
    S(livo_lio_stats); O(livo_lio_stats, stage); O(livo_lio_stats, scan_id); O(livo_lio_stats, n_taken);
    O(livo_lio_stats, n_down); O(livo_lio_stats, map_built); O(livo_lio_stats, iter);
    O(livo_lio_stats, map_counts); O(livo_lio_stats, cloud);
    printf("enum %d %d %d\n", LIVO_LIO_EMPTY, LIVO_LIO_FIRST_SCAN, LIVO_LIO_UPDATED);
    return 0;
}
"""


def test_structs_match_the_ctypes_mirrors(built, tmp_path):
    import livo_amd
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-I" + INC, str(src), "-o", str(exe)], check=True)
    out = dict(ln.rsplit(" ", 1) for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                           check=True).stdout.splitlines() if not ln.startswith("enum"))
    mirrors = {"livo_lio_params": livo_amd.LioParams, "livo_lio_stats": livo_amd.LioStats}
    seen = 0
    for key, val in out.items():
        t, _, f = key.partition(".")
        want = C.sizeof(mirrors[t]) if not f else getattr(mirrors[t], f).offset
        assert int(val) == want, (key, val, want)
        seen += 1
    assert seen == 8 + 9
    assert (livo_amd.LIO_EMPTY, livo_amd.LIO_FIRST_SCAN, livo_amd.LIO_UPDATED) == (0, 1, 2)
    assert len(livo_amd.LioParams._fields_) == 7 and len(livo_amd.LioStats._fields_) == 9


def test_symbol_is_exported_and_bound(built):
    import livo_amd
    L = livo_amd.load()
    assert L.livo_lio_frame.restype is C.c_int and len(L.livo_lio_frame.argtypes) == 9
    assert "livo_lio_frame" in open(os.path.join(INC, "livo.h")).read()


def _args():
    import livo_amd
    job = livo_amd.ImuJob(None, 0, 0.0, 0.0)
    q = livo_amd.imu_params_to_c(None)
    cy = livo_amd.imu_carry_to_c(livo_amd.new_imu_carry())
    lp = livo_amd.LioParams(0.5, 0.2, 0.5, 1, 0, 1, -1)
    return [job, q, cy, lp, livo_amd.State(), livo_amd.State(), livo_amd.LioStats()]


@pytest.mark.parametrize("null", ["ctx", "job", "imu", "carry", "p", "state", "state_propagat"])
def test_null_arguments_are_refused(built, null):
    import livo_amd
    L = livo_amd.load()
    job, q, cy, lp, s, sp, ls = _args()
    fake = C.c_void_p(0x1000)  # never dereferenced: a NULL argument is found first
    a = {"ctx": fake, "job": C.byref(job), "imu": C.byref(q), "carry": C.byref(cy), "p": C.byref(lp),
         "state": C.byref(s), "state_propagat": C.byref(sp)}
    a[null] = None
    rc = L.livo_lio_frame(a["ctx"], a["job"], a["imu"], a["carry"], 1.0, a["p"], a["state"], a["state_propagat"],
                          C.byref(ls))
    assert rc == E_INVALID


@pytest.mark.parametrize("field,value", [("filter_size_surf", float("nan")), ("match_leaf", float("inf")),
                                         ("filter_size_map_min", 0.0), ("filter_size_map_min", float("nan")),
                                         ("n_imu", -1), ("n_imu", 3)])
def test_bad_arguments_are_refused_before_the_device(built, field, value):
    """(n_imu = 3 with no samples: the job's own refusal.)  The context is never read."""
    import livo_amd
    L = livo_amd.load()
    job, q, cy, lp, s, sp, ls = _args()
    if field == "n_imu":
        job.n_imu = value
    else:
        setattr(lp, field, value)
    rc = L.livo_lio_frame(C.c_void_p(0x1000), C.byref(job), C.byref(q), C.byref(cy), 1.0, C.byref(lp), C.byref(s),
                          C.byref(sp), None)
    assert rc == E_INVALID
