"""Host time per call of livo_vio_match (LidarSelector::addFromSparseMap on the device) at the
reference's frame size: 200k full-resolution points, a 1280 x 1024 gray image, patch_size 8,
grid_size 40, an undistorted camera (livo_vio_match takes no other).  The map is what one
livo_vio_select of the same frame gives, stored with the retained image; the match runs at a
state a few cm and tenths of a degree away.  After one warm call, the median of 20 calls each of
  - livo_vio_match with the image upload,
  - livo_vio_match with gray = NULL (the resident image reused),
  - the sizing call (out = NULL: everything but the scatter and the map's patch store),
  - livo_vio_select with its resident image on the same frame (the yardstick).
One process; every timed call returns only when its results are on the host.

usage: python tools/vmatch_probe.py [points] [calls]
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


def main():
    import livo_amd
    from livo_amd import synth
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    w, h, grid, ps = 1280, 1024, 40, 8
    gray = synth._texture(w, h, np.random.default_rng(5))
    cam = dict(synth.PINHOLE, width=w, height=h, fx=960.0, fy=960.0, cx=640.0, cy=512.0, d=[0.0] * 5)
    Rci = synth.R_CI @ synth.so3_exp(np.array([0.0, 0.0, -np.radians(30.0)]))  # about half of the frame in view
    vp = livo_amd.vio_params(cam, Rci, synth.P_CI)
    vp.patch_size = ps
    raw, _, _, _ = synth.make_raw_scan(n, 4)
    s0 = synth.make_state(4)
    s1 = dict(s0, pos=s0["pos"] + np.array([0.03, -0.02, 0.015]),
              rot=s0["rot"] @ synth.so3_exp(np.radians([0.2, -0.15, 0.1])))
    st0, st1 = livo_amd.state_to_c(s0), livo_amd.state_to_c(s1)
    with livo_amd.Context(0, t_LI=synth.T_LI) as ctx:
        sid, _, _ = ctx.scan_preprocess(raw, leaf_size=0.5)
        L = ctx._L
        cells = (w // grid) * (h // grid)
        pts, pat, sel_stats = ctx.vio_select(s0, gray, vp, grid)
        ctx.vmap_reset(max(len(pts), 1), 2, ps)
        ctx.vmap_add_frame(0, s0, vp, None)
        ctx.vmap_add(0, pts, pat)
        rec = np.zeros(cells, livo_amd.VMATCH_POINT_DTYPE)
        pos = np.zeros((cells, 3), np.float64)
        lev = np.zeros(cells, np.int32)
        out_pat = np.zeros((cells, 3 * ps * ps), np.float32)
        sel = np.zeros(cells, livo_amd.VIS_POINT_DTYPE)
        cnt = C.c_int64()
        ms, vs = livo_amd.VmatchStats(), livo_amd.VisStats()
        P = livo_amd._ptr

        def match(image, sizing=False):
            bufs = (None, None, None, None, 0) if sizing else (P(rec), P(pos), P(lev), P(out_pat), cells)
            rc = L.livo_vio_match(ctx.h, -1, C.byref(st1), C.byref(vp), grid, 0, 0.0, 100.0, P(image), w, h, *bufs,
                                  C.byref(cnt), C.byref(ms))
            if rc:
                raise livo_amd.LivoError("livo_vio_match", rc)

        def select(image):
            rc = L.livo_vio_select(ctx.h, -1, C.byref(st0), C.byref(vp), grid, P(image), w, h, P(sel), P(out_pat), cells,
                                   C.byref(cnt), C.byref(vs))
            if rc:
                raise livo_amd.LivoError("livo_vio_select", rc)

        res = {"points": n, "image": [w, h], "grid_size": grid, "patch_size": ps, "calls": calls,
               "map_points": int(len(pts)), "select_stats": sel_stats}
        for name, warm, fn in (("match_upload_ms", lambda: match(gray), lambda: match(gray)),
                               ("match_resident_ms", lambda: match(gray), lambda: match(None)),
                               ("match_sizing_ms", lambda: match(gray), lambda: match(None, True)),
                               ("select_resident_ms", lambda: select(gray), lambda: select(None))):
            warm()  # buffers allocated, image resident
            ctx.sync()
            ts = []
            for _ in range(calls):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            res[name] = {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4),
                         "max": round(max(ts), 4)}
            print(f"{name:22s} median {res[name]['median']:.3f} ms  min {res[name]['min']:.3f}  "
                  f"max {res[name]['max']:.3f}", flush=True)
            if name == "match_resident_ms":
                res["stats"] = {f: int(getattr(ms, f)) for f, _ in livo_amd.VmatchStats._fields_}
        ctx.scan_release(sid)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
