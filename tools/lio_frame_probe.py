"""Host time per LiDAR frame, results on the host: livo_lio_frame (one call) against the chain it
replaces (livo_imu_propagate, livo_frame_take, inherit / release, livo_iekf_update,
livo_map_incremental, livo_cloud_publish), on the config-2 room at odometry sizes: a 1M-point map
updated after every 100k-point scan.  Every frame is a distinct synthetic Avia message made from
scan j (every point survives the handler), ingested outside the timed region; the timed region
runs from the first call of the frame to the last result on the host.  After one warm frame, the
median of `frames` frames; the whole run is repeated `repeats` times on fresh contexts and the
medians' spread is given.

Rows: chain (ikd-Tree), single call on ikd-Tree and iVox with ekf_inited 1 and 0.  With LIVO_LIB
set to another build of the library (the parent commit's) only the chain row runs, labelled
`chain-parent`: run the tool twice and put the outputs side by side.

usage: python tools/lio_frame_probe.py [frames] [repeats]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-livo-noted_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_MAP, N_SCAN, LEAF, FS_MAP, MATCH = 1_000_000, 100_000, 0.5, 0.5, 0.2
T0 = 1.7e9


def frames_of(n, synth, ic, imc):
    out = []
    for j in range(n):
        body, _, _ = synth.make_scan(N_SCAN, j)
        rng = np.random.default_rng(100 + j)
        m = np.zeros(len(body) + 1, ic.LIVOX)
        m["x"][1:], m["y"][1:], m["z"][1:] = np.asarray(body, np.float32).T
        m["tag"], m["line"] = 0x10, rng.integers(0, 6, len(m))
        m["offset_time"] = np.sort(rng.integers(500_000, 99_000_000, len(m)))  # a driver's message: nearly in order
        st = dict(synth.make_state(j), vel=np.zeros(3))
        t = T0 + 0.11 * j + 0.005 * np.arange(22)
        f_body = st["rot"].T @ (-st["gravity"]) + st["bias_a"]
        imu = np.concatenate([t[:, None], np.tile(f_body, (22, 1)), np.tile(st["bias_g"], (22, 1))], 1)
        carry = {"last_imu": imu[0].copy(), "acc_s_last": np.zeros(3), "angvel_last": np.zeros(3),
                 "last_lidar_end_time": t[0]}
        out.append({"msg": m, "state": st, "imu": imu[1:], "t0": t[0], "carry": carry,
                    "params": imc.inited_params({**imc.default_params(), "mean_acc": f_body})})
    return out


def run(livo_amd, synth, ic, world, frames, ivox, single, ekf):
    c = livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=4)
    try:
        if ivox:
            c.set_backend(livo_amd.BACKEND_IVOX)
            c.ivox_init(resolution=0.5, nearby_type=18, capacity=5_000_000)
            c.ivox_add_points(world)
        else:
            c.map_build(world)
        p = livo_amd.ingest_params(lidar_type=ic.AVIA, n_scans=16, point_filter_num=1, blind=0.01)
        prev, ts = -1, []
        for fr in frames:
            info = c.frame_ingest_livox(fr["msg"], p)
            end = fr["t0"] + float(info["end_curvature"]) / 1000.0
            lim = ic.take_limit(fr["t0"], info["end_curvature"], True)
            t = time.perf_counter()
            if single:
                _, _, _, S = c.lio_frame(fr["imu"], fr["t0"], end, fr["params"], fr["carry"], fr["state"], lim,
                                         filter_size_surf=LEAF, filter_size_map_min=FS_MAP, match_leaf=MATCH,
                                         ekf_inited=ekf, prev_scan_id=prev)
                sid = S["scan_id"]
            else:
                st, _, _ = c.imu_propagate(fr["imu"], fr["t0"], end, fr["params"], fr["carry"], fr["state"],
                                           want_poses=False)
                nt = livo_amd.C.c_int64()
                nd, sidc = livo_amd.C.c_int64(), livo_amd.C.c_int32()
                rc = c._L.livo_frame_take(c.h, lim, 1, LEAF, livo_amd.C.byref(sidc), None, None, 0,
                                          livo_amd.C.byref(nd), livo_amd.C.byref(nt))
                assert rc == 0
                sid = sidc.value
                c.scans[sid] = int(nd.value)
                if prev >= 0:
                    if ivox:
                        c.scan_inherit_neighbors(sid, prev)
                    c.scan_release(prev)
                if ekf:
                    st, _ = c.iekf_update(sid, st, st)
                s = livo_amd.state_to_c(st)
                counts = np.zeros(2, np.int64)
                assert c._L.livo_map_incremental(c.h, sid, s, FS_MAP, int(ekf), None, counts.ctypes.data) == 0
                c.cloud_publish(st, -1, MATCH)
            ts.append((time.perf_counter() - t) * 1e3)
            prev = sid
        return statistics.median(ts[1:])
    finally:
        c.close()


def main():
    import imu_cases as imc
    import ingest_cases as ic
    import livo_amd
    from livo_amd import synth
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    parent = bool(os.environ.get("LIVO_LIB"))
    world = synth.make_map(N_MAP)
    frames = frames_of(n + 1, synth, ic, imc)
    rows = [("chain-parent ikd ekf=1", False, False, True)] if parent else [
        ("chain ikd ekf=1", False, False, True), ("single ikd ekf=1", False, True, True),
        ("single ikd ekf=0", False, True, False), ("single ivox ekf=1", True, True, True),
        ("single ivox ekf=0", True, True, False)]
    res = {"frames": n, "repeats": repeats, "map_points": N_MAP, "scan_points": N_SCAN}
    for name, ivox, single, ekf in rows:
        med = [run(livo_amd, synth, ic, world, frames, ivox, single, ekf) for _ in range(repeats)]
        res[name] = {"median_of_medians": round(statistics.median(med), 4), "min": round(min(med), 4),
                     "max": round(max(med), 4)}
        print(f"{name:24s} ms/frame: median of {repeats} medians {res[name]['median_of_medians']:.4f}  "
              f"spread {res[name]['min']:.4f} .. {res[name]['max']:.4f}", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
