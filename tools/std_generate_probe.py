"""Host time per livo_std_generate and per livo_std_key_add on key clouds of about 50,000 and 500,000 points
of the synthetic room of tests/std_gen_cases.py (the same surfaces at a higher density).  After one warm call,
the median of 20 calls; the medians of five fresh contexts are reported with their spread.  Every timed
generate starts from a key cloud appended device to device from the published world cloud and returns when its
counts are on the host; every timed key_add ends with a livo_sync.

usage: python tools/std_generate_probe.py [points ...]     (default: 50000 500000)
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

CALLS, CONTEXTS = 20, 5


def one_context(livo_amd, synth, G, sizes, seed):
    out = {}
    with livo_amd.Context(0) as ctx:
        L, h = ctx._L, ctx.h
        ctx.std_reset(livo_amd.std_params(), 1 << 16, 64, 1 << 16)
        prm = livo_amd.std_gen_params()
        state = synth.make_state(0)
        state["rot"], state["pos"] = np.eye(3), np.zeros(3)
        for size in sizes:
            pts = G.room(np.random.default_rng(seed), density=50.0 * size / 9726.0).astype(np.float32)
            sid = ctx.scan_upload(pts)
            ctx.cloud_publish(state, sid, match_leaf=0.0)
            ctx.scan_release(sid)
            add_ms, gen_ms, stats = [], [], None
            for k in range(CALLS + 1):
                ctx.std_key_clear()
                assert L.livo_sync(h) == 0
                t0 = time.perf_counter()
                ctx.std_key_add(livo_amd.CLOUD_WORLD)
                assert L.livo_sync(h) == 0
                t1 = time.perf_counter()
                stats = ctx.std_generate(prm)
                t2 = time.perf_counter()
                if k:  # (the first call is the warm one)
                    add_ms.append((t1 - t0) * 1e3)
                    gen_ms.append((t2 - t1) * 1e3)
            out[size] = dict(key_add_ms=statistics.median(add_ms), generate_ms=statistics.median(gen_ms), stats=stats)
    return out


def main():
    import livo_amd
    from livo_amd import synth

    import std_gen_cases as G
    sizes = [int(a) for a in sys.argv[1:]] or [50000, 500000]
    runs = []
    for k in range(CONTEXTS):
        runs.append(one_context(livo_amd, synth, G, sizes, 100 + k))
        print(f"context {k}: " + json.dumps(runs[-1]), file=sys.stderr, flush=True)
    for size in sizes:
        row = {"points": runs[0][size]["stats"]["points"]}
        for key in ("key_add_ms", "generate_ms"):
            v = sorted(r[size][key] for r in runs)
            row[key] = {"median": round(statistics.median(v), 4), "min": round(v[0], 4), "max": round(v[-1], 4)}
        row["stats"] = runs[0][size]["stats"]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
