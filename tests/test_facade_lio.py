"""The C++ facade's one-call LiDAR frame (LaserMappingGpu::RunLidarFrame, host/facade_demo.cpp mode
`lio`) against the separate methods it replaces (mode `lio_chain`: Process2, iterate,
map_incremental, publish_cloud) over three consecutive frames on the iVox backend.  Both feed the
same kernels the same bytes, so every printed value, the hex bytes of state and state_propagat
included, is equal.
"""
import subprocess

import pytest

from test_facade import DEMO, _inputs


def test_usage_names_the_lio_modes(built):
    r = subprocess.run([DEMO], capture_output=True, text=True)
    assert r.returncode == 2 and "lio" in r.stderr and "lio_chain" in r.stderr


@pytest.mark.gpu
def test_facade_lio_matches_the_chain(built, tmp_path):
    _, body, _, files = _inputs(tmp_path)
    out = {}
    for mode in ("lio", "lio_chain"):
        r = subprocess.run([DEMO, *files, "4", mode], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (mode, r.stderr)
        out[mode] = {" ".join(ln.split()[:2]): ln.split()[2:] for ln in r.stdout.splitlines()}
    a, b = out["lio"], out["lio_chain"]
    assert set(a) == {f"{w} {k}" for w in ("frame", "state", "prop") for k in range(3)}
    for k in range(3):
        taken, down, iters, added, _, cn, cd = (int(x) for x in a[f"frame {k}"])
        assert taken > len(body) // 2 and 0 < down <= taken and iters >= 1 and cn == taken and 0 < cd <= cn
        assert len(a[f"state {k}"][0]) == 2 * 348 * 8 and a[f"state {k}"] != a[f"prop {k}"]
    assert a == b
