"""Host time per call of livo_vio_select (LidarSelector::addSparseMap on the device) at the
reference's frame size: 200k full-resolution points, a 1280 x 1024 gray image, patch_size 8,
grid_size 40.  After one warm call, the median of 20 calls each of
  - the call with the image upload,
  - the call with gray = NULL (the resident image reused),
  - the sizing call (out = NULL: the score pass and the counters only), resident image,
  - livo_cloud_colorize with its resident image on the same frame (the yardstick: the same cloud
    traffic, one bilinear sample a point).
One process; every timed call returns only when its results are on the host.

usage: python tools/vis_select_probe.py [points] [calls]
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
    w, h, grid = 1280, 1024, 40
    gray = synth._texture(w, h, np.random.default_rng(5))
    bgr = np.ascontiguousarray(np.repeat(gray[:, :, None], 3, axis=2))
    cam = dict(synth.PINHOLE, width=w, height=h, fx=960.0, fy=960.0, cx=640.0, cy=512.0)
    Rci = synth.R_CI @ synth.so3_exp(np.array([0.0, 0.0, -np.radians(30.0)]))  # about half of the frame in view
    vp = livo_amd.vio_params(cam, Rci, synth.P_CI)
    vp.patch_size = 8
    raw, _, _, _ = synth.make_raw_scan(n, 4)
    st = livo_amd.state_to_c(synth.make_state(4))
    with livo_amd.Context(0, t_LI=synth.T_LI) as ctx:
        sid, _, _ = ctx.scan_preprocess(raw, leaf_size=0.5)
        L = ctx._L
        cells = (w // grid) * (h // grid)
        out = np.zeros(cells, livo_amd.VIS_POINT_DTYPE)
        pat = np.zeros((cells, 3 * 64), np.float32)
        rgb = np.zeros(n, livo_amd.RGB_POINT_DTYPE)
        cnt = C.c_int64()
        vs = livo_amd.VisStats()

        def select(image, sizing=False):
            rc = L.livo_vio_select(ctx.h, -1, C.byref(st), C.byref(vp), grid, livo_amd._ptr(image), w, h,
                                   None if sizing else livo_amd._ptr(out), None if sizing else livo_amd._ptr(pat),
                                   0 if sizing else cells, C.byref(cnt), C.byref(vs))
            if rc:
                raise livo_amd.LivoError("livo_vio_select", rc)

        def colorize(image):
            rc = L.livo_cloud_colorize(ctx.h, -1, C.byref(st), C.byref(vp), livo_amd._ptr(image), w, h,
                                       livo_amd._ptr(rgb), None, n, C.byref(cnt), None)
            if rc:
                raise livo_amd.LivoError("livo_cloud_colorize", rc)

        res = {"points": n, "image": [w, h], "grid_size": grid, "patch_size": 8, "calls": calls}
        for name, warm, fn in (("select_upload_ms", lambda: select(gray), lambda: select(gray)),
                               ("select_resident_ms", lambda: select(gray), lambda: select(None)),
                               ("select_sizing_ms", lambda: select(gray), lambda: select(None, True)),
                               ("colorize_resident_ms", lambda: colorize(bgr), lambda: colorize(None))):
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
            if name == "select_resident_ms":
                res["stats"] = {f: int(getattr(vs, f)) for f, _ in livo_amd.VisStats._fields_}
        ctx.scan_release(sid)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
