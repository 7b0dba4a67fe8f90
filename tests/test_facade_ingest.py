"""The C++ facade's resident-frame flow (livox_pcl_cbk -> Process2 -> iterate -> map_incremental,
host/facade_demo.cpp mode `ingest`) against the host-array flow it replaces (mode `ingest_host`: a
C++ restatement of avia_handler, std::stable_sort and the slice in the caller's code, then the
Process2 that uploads a host array).  Both feed the same kernels the same bytes, so every printed
value is equal.  The synthetic Avia frame is split by one image 30 ms into it.
"""
import os
import subprocess

import pytest

from test_facade import DEMO, _inputs


def test_usage_names_the_ingest_modes(built):
    r = subprocess.run([DEMO], capture_output=True, text=True)
    assert r.returncode == 2 and "ingest" in r.stderr and "ingest_host" in r.stderr


@pytest.mark.gpu
def test_facade_ingest_matches_the_host_array_flow(built, tmp_path):
    _, body, _, files = _inputs(tmp_path, n_map=300_000)
    out = {}
    for mode in ("ingest", "ingest_host"):
        r = subprocess.run([DEMO, *files, "4", mode], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (mode, r.stderr)
        out[mode] = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    a, b = out["ingest"], out["ingest_host"]
    assert set(a) == {"take", "iekf", "incr"}
    cam, lidar = (int(x) for x in a["take"])
    # the image inside the scan consumes the points at time 0, a twentieth of the message; the LiDAR frame the rest
    assert cam >= len(body) // 20 and lidar > len(body) // 2 and cam + lidar <= len(body)
    assert int(a["iekf"][0]) >= 1
    assert a == b
