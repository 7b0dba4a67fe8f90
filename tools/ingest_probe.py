"""Host time per call of the sensor handlers on the device against the host path they replace, on a
synthetic Avia message (every point survives the predicate): after one warm call, the median of 20 calls of
  - device: livo_frame_ingest_livox (upload of the 20-byte records, handler, time sort) +
    livo_frame_take (slice, de-skew, VoxelGrid, resident scan), the scan released;
  - host:   avia_handler + std::sort in plain single-thread C++ (tools/ingest_probe_helper.cpp), then
    livo_scan_preprocess_imu from the host array, the scan released.
24,000 points (an Avia frame) and 240,000, point_filter_num 1 and 2.  One process; every timed call
returns only when its results are resident and its counts are on the host.

usage: python tools/ingest_probe.py [calls]      (OUT_DIR: where the helper is built, default out/)
"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-livo-noted_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def helper():
    out = os.environ.get("OUT_DIR", os.path.join(ROOT, "out"))
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "ingest_probe_helper.so")
    src = os.path.join(ROOT, "tools", "ingest_probe_helper.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                               src, "-o", so])
    H = C.CDLL(so)
    H.avia_sort_host.restype = C.c_int64
    H.avia_sort_host.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_void_p]
    return H


def main():
    import imu_cases as imc
    import ingest_cases as ic
    import livo_amd
    from livo_amd import synth
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    H = helper()
    res = {"calls": calls}

    def timed(name, fn):
        fn()
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        res[name] = {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}
        print(f"{name:28s} median {res[name]['median']:.4f} ms  min {res[name]['min']:.4f}  max {res[name]['max']:.4f}",
              flush=True)

    with livo_amd.Context(0, t_LI=synth.T_LI) as ctx:
        L = ctx._L
        job, params, carry, state = imc.make_case(20, key="frame")
        ctx.imu_propagate(job[0], job[1], job[2], params, carry, state, want_poses=False)
        for n in (24_000, 240_000):
            m = ic.livox_msg(n, "all", "random", seed=n)
            raw = np.zeros((n, 5), np.float32)
            for p in (1, 2):
                q = livo_amd.ingest_params(point_filter_num=p)
                info = livo_amd.IngestInfo()
                sid, nd, nt = C.c_int32(), C.c_int64(), C.c_int64()
                kept = {}

                def device():
                    rc = L.livo_frame_ingest_livox(ctx.h, C.byref(q), m.ctypes.data, n, C.byref(info))
                    lim = ic.take_limit(0.0, info.end_curvature, True)
                    rc = rc or L.livo_frame_take(ctx.h, lim, 1, 0.5, C.byref(sid), None, None, 0, C.byref(nd),
                                                 C.byref(nt))
                    rc = rc or L.livo_scan_release(ctx.h, sid.value)
                    if rc:
                        raise livo_amd.LivoError("device path", rc)
                    kept["device"] = (nt.value, nd.value)

                def host():
                    k = H.avia_sort_host(m.ctypes.data, n, q.n_scans, p, q.blind, raw.ctypes.data)
                    rc = L.livo_scan_preprocess_imu(ctx.h, raw.ctypes.data, k, 0.5, C.byref(sid), None, None, 0,
                                                    C.byref(nd))
                    rc = rc or L.livo_scan_release(ctx.h, sid.value)
                    if rc:
                        raise livo_amd.LivoError("host path", rc)
                    kept["host"] = (k, nd.value)

                def host_cpu_part():
                    H.avia_sort_host(m.ctypes.data, n, q.n_scans, p, q.blind, raw.ctypes.data)

                timed(f"device_n{n}_p{p}_ms", device)
                timed(f"host_n{n}_p{p}_ms", host)
                timed(f"host_cpu_part_n{n}_p{p}_ms", host_cpu_part)
                assert kept["device"] == kept["host"], kept
                res[f"n{n}_p{p}"] = {"kept": kept["host"][0], "down": kept["host"][1],
                                     "device_upload_bytes": n * 20, "host_upload_bytes": kept["host"][0] * 20}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
