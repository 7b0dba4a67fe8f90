"""Host time per call of livo_vio_observe (LidarSelector::addObservation on the device) beside
livo_vio_match, on tools/vmatch_probe.py's frame: 200k full-resolution points, a 1280 x 1024
gray image, patch_size 8, grid_size 40, an undistorted camera.  The map is what one
livo_vio_select of the frame gives, stored with the retained image; one livo_vio_match at a
state a few cm and tenths of a degree away gives the survivors.  After one warm call, the median
of 20 calls each of
  - livo_vio_match with the resident image (the yardstick, in the same process),
  - livo_vio_observe of the survivors from a frame stored at the match's state: 3 cm from the
    points' only observation, so nothing is added and the map stays as it is,
  - livo_vio_observe of the survivors from a frame stored 0.6 m to the side: every point in that
    frame adds, so the lists grow by one a call up to 20, and the last two calls evict: the
    first the points' one observation from another pose, the second, with nothing left that is
    0.5 m away, without adding.
One process; every timed call returns only when its records are on the host.  A record, not a bar.

usage: python tools/vobserve_probe.py [points] [calls]
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
    Rcw = Rci @ s0["rot"].T
    s2 = dict(s1, pos=s1["pos"] + 0.6 * Rcw[0])  # 0.6 m along the camera's x axis
    st1 = livo_amd.state_to_c(s1)
    with livo_amd.Context(0, t_LI=synth.T_LI) as ctx:
        sid, _, _ = ctx.scan_preprocess(raw, leaf_size=0.5)
        L = ctx._L
        cells = (w // grid) * (h // grid)
        pts, pat, _ = ctx.vio_select(s0, gray, vp, grid)
        ctx.vmap_reset(max(len(pts), 1), 3, ps)
        ctx.vmap_add_frame(0, s0, vp, None)
        ctx.vmap_add(0, pts, pat)
        m = ctx.vio_match(s1, gray, vp, grid)
        ids = np.ascontiguousarray(m["records"]["point_id"])
        lev = np.ascontiguousarray(m["records"]["search_level"])
        ctx.vmap_add_frame(1, s1, vp, gray)
        ctx.vmap_add_frame(2, s2, vp, gray)
        rec = np.zeros(cells, livo_amd.VMATCH_POINT_DTYPE)
        pos = np.zeros((cells, 3), np.float64)
        out_lev = np.zeros(cells, np.int32)
        out_pat = np.zeros((cells, 3 * ps * ps), np.float32)
        obs = np.zeros(len(ids), livo_amd.VOBS_POINT_DTYPE)
        cnt = C.c_int64()
        ms, os_ = livo_amd.VmatchStats(), livo_amd.VobsStats()
        P = livo_amd._ptr

        def match():
            rc = L.livo_vio_match(ctx.h, -1, C.byref(st1), C.byref(vp), grid, 0, 0.0, 100.0, None, w, h, P(rec), P(pos),
                                  P(out_lev), P(out_pat), cells, C.byref(cnt), C.byref(ms))
            if rc:
                raise livo_amd.LivoError("livo_vio_match", rc)

        def observe(fid):
            rc = L.livo_vio_observe(ctx.h, fid, len(ids), P(ids), P(lev), P(obs), C.byref(os_))
            if rc:
                raise livo_amd.LivoError("livo_vio_observe", rc)

        res = {"points": n, "image": [w, h], "grid_size": grid, "patch_size": ps, "calls": calls,
               "map_points": int(len(pts)), "survivors": int(len(ids))}
        for name, fn in (("match_resident_ms", match), ("observe_keep_ms", lambda: observe(1)),
                         ("observe_add_ms", lambda: observe(2))):
            fn()  # buffers allocated
            ctx.sync()
            if name != "match_resident_ms":
                res[name[:-3] + "_first_stats"] = {f: int(getattr(os_, f)) for f, _ in livo_amd.VobsStats._fields_}
            ts = []
            for _ in range(calls):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            res[name] = {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4),
                         "max": round(max(ts), 4)}
            print(f"{name:22s} median {res[name]['median']:.3f} ms  min {res[name]['min']:.3f}  "
                  f"max {res[name]['max']:.3f}", flush=True)
            if name != "match_resident_ms":
                res[name[:-3] + "_last_stats"] = {f: int(getattr(os_, f)) for f, _ in livo_amd.VobsStats._fields_}
        for name in ("observe_keep_ms", "observe_add_ms"):
            res[name[:-3] + "_over_match"] = round(res[name]["median"] / res["match_resident_ms"]["median"], 3)
        ctx.scan_release(sid)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
