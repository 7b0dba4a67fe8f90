"""Host time per livo_std_search and per livo_std_commit on databases of 1,000 and 10,000 key frames
of 1,000 descriptors each (1e6 and 1e7 stored descriptors).  Every context is built once, frame by
frame as a session would, and measured when it reaches each size: after one warm call, the median of
20 calls; the medians of five fresh contexts are reported with their spread.  The searched frame is a
noisy copy of key frame 100 (a revisit: candidates, verification and the plane check all run), so
every search finds a loop; each timed call returns only when its result is on the host.

Side lengths are 5 x sorted uniform 2-30 m sides, as the STD front-end produces at its 0.2 m side
resolution; 200 plane points a frame.

usage: python tools/std_search_probe.py [frames ...]     (default: 1000 10000)
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-livo-noted_amd"))

N_DESC, N_PLANES, CALLS, CONTEXTS = 1000, 200, 20, 5


def make_frame(rng, livo_amd, frame):
    d = np.zeros(N_DESC, livo_amd.STD_DESC_DTYPE)
    d["side_length"] = 5.0 * np.sort(rng.uniform(2.0, 30.0, (N_DESC, 3)), axis=1)
    for k in ("vertex_A", "vertex_B", "vertex_C"):
        d[k] = rng.uniform(-50.0, 50.0, (N_DESC, 3))
    d["center"] = (d["vertex_A"] + d["vertex_B"] + d["vertex_C"]) / 3.0
    d["vertex_attached"] = rng.integers(8, 40, (N_DESC, 3))
    d["frame_id"] = frame
    p = np.zeros(N_PLANES, livo_amd.STD_PLANE_DTYPE)
    p["xyz"] = rng.uniform(-50.0, 50.0, (N_PLANES, 3))
    n = rng.normal(size=(N_PLANES, 3))
    p["normal"] = n / np.linalg.norm(n, axis=1, keepdims=True)
    return d, p


def revisit_of(rng, d, p, frame):
    q = d.copy()
    for k in ("vertex_A", "vertex_B", "vertex_C"):
        q[k] += rng.uniform(-0.01, 0.01, (N_DESC, 3))
    q["center"] = (q["vertex_A"] + q["vertex_B"] + q["vertex_C"]) / 3.0
    q["side_length"] += rng.uniform(-0.05, 0.05, (N_DESC, 3))
    q["frame_id"] = frame
    return q, p.copy()


def timed(fn, calls=CALLS):
    fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def one_context(livo_amd, sizes, seed):
    rng = np.random.default_rng(seed)
    out = {}
    top = max(sizes) + CALLS + 2
    with livo_amd.Context(0) as ctx:
        L, h = ctx._L, ctx.h
        ctx.std_reset(livo_amd.std_params(), top * N_DESC, top, top * N_PLANES)
        kept = None
        res, n = livo_amd.StdResult(), C.c_int64()
        pairs = np.zeros(N_DESC * 27, livo_amd.STD_PAIR_DTYPE)
        frame = 0
        for size in sorted(sizes):
            while frame < size:
                d, p = make_frame(rng, livo_amd, frame)
                if frame == 100:
                    kept = (d, p)
                ctx.std_stage(d, p)
                ctx.std_commit()
                frame += 1
            q, qp = revisit_of(rng, kept[0], kept[1], frame)
            ctx.std_stage(q, qp)

            def search():
                rc = L.livo_std_search(h, C.byref(res), pairs.ctypes.data_as(C.c_void_p), len(pairs), C.byref(n))
                assert rc == 0 and res.frame == 100, (rc, res.frame)

            t_search = timed(search)
            fresh = [make_frame(rng, livo_amd, frame + k) for k in range(CALLS + 1)]
            it = iter(fresh)

            def commit():  # the staged frame is new on every call; the time is the commit's alone
                d, p = next(it)
                ctx.std_stage(d, p)
                t0 = time.perf_counter()
                assert L.livo_std_commit(h, None) == 0 and L.livo_sync(h) == 0
                return (time.perf_counter() - t0) * 1e3

            commit()
            t_commit = statistics.median(commit() for _ in range(CALLS))
            frame += CALLS + 1
            out[size] = dict(search_ms=t_search, commit_ms=t_commit, candidates=res.n_candidates, pairs=int(n.value))
    return out


def main():
    import livo_amd
    sizes = [int(a) for a in sys.argv[1:]] or [1000, 10000]
    runs = []
    for k in range(CONTEXTS):
        runs.append(one_context(livo_amd, sizes, 100 + k))
        print(f"context {k}: " + json.dumps(runs[-1]), file=sys.stderr, flush=True)
    for size in sizes:
        row = {"frames": size, "descriptors": size * N_DESC}
        for key in ("search_ms", "commit_ms"):
            v = sorted(r[size][key] for r in runs)
            row[key] = {"median": round(statistics.median(v), 4), "min": round(v[0], 4), "max": round(v[-1], 4)}
        row["candidates"] = runs[0][size]["candidates"]
        row["pairs"] = runs[0][size]["pairs"]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
