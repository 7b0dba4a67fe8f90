"""Host time per call of livo_cloud_colorize (publish_frame_world_rgb on the device) at the
reference's frame size: 200k full-resolution points, a 1280 x 1024 BGR image.  After one warm
call, the median of 20 calls each of
  - the call with the image upload,
  - the call with image = NULL (the resident image reused),
  - livo_frame_to_world alone on the same frame (the yardstick: transform + copy back).
One process; every timed call returns only when its results are on the host.

usage: python tools/rgb_cloud_probe.py [points] [calls]
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
    w, h = 1280, 1024
    img = np.random.default_rng(5).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    cam = dict(synth.PINHOLE, width=w, height=h, fx=960.0, fy=960.0, cx=640.0, cy=512.0)
    Rci = synth.R_CI @ synth.so3_exp(np.array([0.0, 0.0, -np.radians(30.0)]))  # about half of the frame in view
    vp = livo_amd.vio_params(cam, Rci, synth.P_CI)
    raw, _, _, _ = synth.make_raw_scan(n, 4)
    st = livo_amd.state_to_c(synth.make_state(4))
    with livo_amd.Context(0, t_LI=synth.T_LI) as ctx:
        sid, _, _ = ctx.scan_preprocess(raw, leaf_size=0.5)
        L = ctx._L
        out = np.zeros(n, livo_amd.RGB_POINT_DTYPE)
        idx = np.zeros(n, np.int32)
        world = np.zeros((n, 5), np.float32)
        cnt = C.c_int64()
        rs = livo_amd.RgbStats()

        def colorize(image):
            rc = L.livo_cloud_colorize(ctx.h, -1, C.byref(st), C.byref(vp), livo_amd._ptr(image), w, h,
                                       livo_amd._ptr(out), livo_amd._ptr(idx), n, C.byref(cnt), C.byref(rs))
            if rc:
                raise livo_amd.LivoError("livo_cloud_colorize", rc)

        def to_world(_):
            rc = L.livo_frame_to_world(ctx.h, -1, C.byref(st), livo_amd._ptr(world), n, C.byref(cnt))
            if rc:
                raise livo_amd.LivoError("livo_frame_to_world", rc)

        res = {"points": n, "image": [w, h], "calls": calls}
        for name, fn, arg in (("colorize_upload_ms", colorize, img), ("colorize_resident_ms", colorize, None),
                              ("frame_to_world_ms", to_world, None)):
            fn(img if fn is colorize else None)  # warm: buffers allocated, image resident
            ctx.sync()
            ts = []
            for _ in range(calls):
                t0 = time.perf_counter()
                fn(arg)
                ts.append((time.perf_counter() - t0) * 1e3)
            res[name] = {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4),
                         "max": round(max(ts), 4)}
            print(f"{name:22s} median {res[name]['median']:.3f} ms  min {res[name]['min']:.3f}  "
                  f"max {res[name]['max']:.3f}", flush=True)
        res["kept"] = int(rs.n_out)
        res["stats"] = {f: int(getattr(rs, f)) for f, _ in livo_amd.RgbStats._fields_}
        ctx.scan_release(sid)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
