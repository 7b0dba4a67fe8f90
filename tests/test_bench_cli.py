"""bench.py's command line: a plain run is the headline alone, --full adds the rest,
--dump-outputs writes what the last timed step returned.

  * CPU: the options and their defaults; dump_outputs on hand-made ctypes arrays
    (names, shapes, float64, entries beyond a scan's last evaluation zeroed);
  * GPU: one small plain run with --dump-outputs: the result line carries the
    headline fields and none of the --full ones, and the dumped arrays equal, bit
    for bit, a synchronous update of the same batch of scans in this process.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STATE_SHAPES = {"rot": (3, 3), "pos": (3,), "vel": (3,), "bias_g": (3,), "bias_a": (3,), "gravity": (3,),
                "cov": (18, 18)}
STATS_SHAPES = {"iterations": (), "knn_passes": (), "converged": (), "rematch_num": (), "effct_feat_num": (16,),
                "solution": (16, 18), "res_mean": (16,)}
FULL_ONLY = ("roofline", "device_ms_per_step", "sync_value", "fixed8_value", "value_with_upload", "cpu_baseline",
             "drop_in", "config5", "ikfom", "ivox", "ikd_incremental", "vio")


def test_options(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_arrays(tmp_path):
    import bench
    import livo_amd
    n = 3
    states = (livo_amd.State * n)()
    stats = (livo_amd.IterStats * n)()
    for b in range(n):
        states[b].rot[:] = [float(b * 10 + i) for i in range(9)]
        states[b].pos[:] = [b + 0.25, b + 0.5, b + 0.75]
        states[b].cov[:] = [float(b * 1000 + i) for i in range(324)]
        stats[b].iterations = b + 1
        stats[b].knn_passes = 2
        for e in range(16):  # entries beyond `iterations` hold junk that must not be written
            stats[b].effct_feat_num[e] = 100 + e
            stats[b].res_mean[e] = 0.5 + e
            stats[b].solution[e][:] = [float(e * 18 + i) for i in range(18)]
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), states, stats, n)
    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(got) == set(STATE_SHAPES) | set(STATS_SHAPES)
    for k, v in got.items():
        assert v.dtype == np.float64 and v.shape == (n,) + {**STATE_SHAPES, **STATS_SHAPES}[k], k
    assert np.array_equal(got["rot"][2], np.arange(20.0, 29.0).reshape(3, 3))
    assert np.array_equal(got["pos"][1], [1.25, 1.5, 1.75])
    assert np.array_equal(got["cov"][1].ravel(), np.arange(1000.0, 1324.0))
    assert np.array_equal(got["iterations"], [1.0, 2.0, 3.0])
    for b in range(n):
        assert np.array_equal(got["effct_feat_num"][b, :b + 1], 100.0 + np.arange(b + 1))
        assert np.array_equal(got["solution"][b, b], np.arange(b * 18.0, b * 18.0 + 18))
        assert not got["effct_feat_num"][b, b + 1:].any() and not got["solution"][b, b + 1:].any()
        assert not got["res_mean"][b, b + 1:].any()


@pytest.mark.gpu
def test_plain_run_dumps_last_step(built, tmp_path):
    import livo_amd
    from livo_amd import synth
    batch, steps, n_scan, n_map = 4, 3, 5_000, 100_000
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--batch", str(batch), "--scan-points", str(n_scan), "--map-points",
                        str(n_map), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(line) == 1, r.stdout[-2000:]
    j = json.loads(line[0])
    assert j["steps"] == steps and j["total_scans"] == steps * batch
    assert j["value"] > 0 and j["unit"] == "scan updates/s" and j["higher_is_better"] is True
    assert j["ms_per_step"] == pytest.approx(1e3 * batch / j["value"], rel=5e-3)
    assert not [k for k in FULL_ONLY if k in j]
    # the last timed step is pool batch steps - 1: seeds (steps - 1) * batch + s on rank 0
    seeds = [(steps - 1) * batch + s for s in range(batch)]
    with livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=4) as ctx:
        ctx.map_build(synth.make_map(n_map))
        sids = [ctx.scan_upload(synth.make_scan(n_scan, s)[0]) for s in seeds]
        states, stats = ctx.iekf_update_batch(sids, [synth.make_state(s) for s in seeds])
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == set(STATE_SHAPES) | set(STATS_SHAPES)
    for b in range(batch):
        for k in STATE_SHAPES:
            assert np.array_equal(got[k][b], states[b][k]), (b, k)
        ne = stats[b]["iterations"]
        assert got["iterations"][b] == ne and got["knn_passes"][b] == stats[b]["knn_passes"]
        assert np.array_equal(got["solution"][b, :ne], stats[b]["solution"]), b
        assert np.array_equal(got["effct_feat_num"][b, :ne], stats[b]["effct_feat_num"]), b
        assert np.array_equal(got["res_mean"][b, :ne], stats[b]["res_mean"]), b
        assert not got["solution"][b, ne:].any()
