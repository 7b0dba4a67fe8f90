"""The C++ facade's loop closure (LaserMappingGpu::StdStage / SearchLoop / AddSTDescs,
host/facade_demo.cpp mode `loop`) against the Python binding on the same sequence: twelve key frames,
the last a revisit of place 2.  Both feed the same kernels the same bytes, so every printed value,
the hex bytes of score, rot and t included, is equal."""
import struct
import subprocess

import numpy as np
import pytest

import std_cases as S
from test_facade import DEMO

SKIP_NEAR, CANDIDATES, N_SEQ = 5, 3, 12


def _sequence():
    rng = np.random.default_rng(7)
    places = [S.make_place(rng, 24, 20) for _ in range(N_SEQ - 1)]
    R, t = S.random_rigid(rng)
    frames = [(S.place_descs(tr, f), pl) for f, (tr, pl) in enumerate(places)]
    q_tris, q_planes = S.revisit(rng, places[2][0], places[2][1], R, t, N_SEQ - 1)
    frames.append((S.place_descs(q_tris, N_SEQ - 1), q_planes))
    return frames


def test_usage_names_the_loop_mode(built):
    r = subprocess.run([DEMO], capture_output=True, text=True)
    assert r.returncode == 2 and "loop" in r.stderr.split("lio_chain", 1)[1]


@pytest.mark.gpu
def test_facade_loop_matches_the_binding(built, gpu_ctx, tmp_path):
    import livo_amd
    frames = _sequence()
    path = tmp_path / "seq.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", len(frames), SKIP_NEAR, CANDIDATES, 0))
        for d, p in frames:
            f.write(struct.pack("<2i", len(d), len(p)))
            f.write(np.ascontiguousarray(d).tobytes())
            f.write(np.ascontiguousarray(p).tobytes())
    r = subprocess.run([DEMO, str(path), "-", "-", "0", "loop"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = []
    gpu_ctx.std_reset(livo_amd.std_params(skip_near_num=SKIP_NEAR, candidate_num=CANDIDATES), 1 << 16, len(frames),
                      1 << 16)
    for k, (d, p) in enumerate(frames):
        gpu_ctx.std_stage(d, p)
        res = gpu_ctx.std_search()
        assert gpu_ctx.std_commit() == k
        v = np.concatenate([[res["score"]], res["rot"].ravel(), res["t"]]).astype(np.float64)
        want.append(f"loop {k} {res['frame']} {res['n_candidates']} {len(res['pairs'])} {v.tobytes().hex()}")
        want.append(" ".join([f"pairs {k}"] + [f"{a}:{b}:{c}" for a, b, c in res["pairs"].tolist()]))
    assert r.stdout.splitlines() == want
    assert want[-2].split()[2] == "2" and int(want[-2].split()[4]) >= 4  # the revisit closes the loop on frame 2
    assert all(w.split()[2] == "-1" for w in want[:-2:2])
