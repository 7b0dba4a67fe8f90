"""Host time per call of the IMU forward propagation (livo_imu_propagate, livo_imu_propagate_batch)
on jobs of 20 samples, a LiDAR frame's worth at 200 Hz: after one warm call, the median of 20 calls of
  - one job (livo_imu_propagate: the table stays resident, the state comes back),
  - a batch of 8 jobs and a batch of 64 jobs in one launch each (states, carries and tables back),
  - the float64 numpy restatement (tests/imu_cases.py, dense F @ P @ F.T + Q) of the same jobs, one thread.
One process; every timed call returns only when its results are on the host.

usage: python tools/imu_propagate_probe.py [samples] [calls]
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("MKL_NUM_THREADS", "1")

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-livo-noted_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import imu_cases as ic
    import livo_amd
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    cases = [ic.make_case(m, key=f"probe{k}") for k in range(64)]
    params = cases[0][1]
    res = {"samples": m, "calls": calls}

    def timed(name, fn):
        fn()
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        res[name] = {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}
        print(f"{name:24s} median {res[name]['median']:.4f} ms  min {res[name]['min']:.4f}  max {res[name]['max']:.4f}",
              flush=True)

    with livo_amd.Context(0) as ctx:
        L = ctx._L
        q = livo_amd.imu_params_to_c(params)
        for n in (1, 8, 64):
            imus = [np.ascontiguousarray(c[0][0]) for c in cases[:n]]
            jobs = (livo_amd.ImuJob * n)(*[livo_amd.ImuJob(a.ctypes.data, m, c[0][1], c[0][2])
                                           for a, c in zip(imus, cases)])
            carries0 = [livo_amd.imu_carry_to_c(c[2]) for c in cases[:n]]
            states0 = [livo_amd.state_to_c(c[3]) for c in cases[:n]]
            carries = (livo_amd.ImuCarry * n)()
            states = (livo_amd.State * n)()
            poses = np.zeros((n, m + 1, 22))
            cnt = np.zeros(n, np.int32)

            def run():
                for k in range(n):  # (the calls update in place: every call starts from the same inputs)
                    C.memmove(C.byref(carries[k]), C.byref(carries0[k]), C.sizeof(livo_amd.ImuCarry))
                    C.memmove(C.byref(states[k]), C.byref(states0[k]), C.sizeof(livo_amd.State))
                if n == 1:
                    rc = L.livo_imu_propagate(ctx.h, C.byref(jobs[0]), C.byref(q), C.byref(carries[0]),
                                              C.byref(states[0]), None, 0, None)
                else:
                    rc = L.livo_imu_propagate_batch(ctx.h, n, C.cast(jobs, C.c_void_p), C.byref(q),
                                                    C.cast(carries, C.c_void_p), C.cast(states, C.c_void_p),
                                                    livo_amd._ptr(poses), m + 1, livo_amd._ptr(cnt))
                if rc:
                    raise livo_amd.LivoError("livo_imu_propagate", rc)

            timed(f"device_{n}_jobs_ms", run)
    for n in (1, 8, 64):
        timed(f"numpy64_{n}_jobs_ms", lambda: [ic.propagate(c[0], params, c[2], c[3]) for c in cases[:n]])
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
