"""Host time per camera frame of livo_vio_detect beside the chain of six public calls that defines it
(livo_vio_match, livo_vio_select, livo_vio_update, livo_vmap_add_frame, livo_vio_observe, livo_vmap_add), on
tools/vmatch_probe.py's and tools/vobserve_probe.py's frame: 200k full-resolution points, a 1280 x 1024 gray
image, patch_size 8, grid_size 40, an undistorted camera.  Twin contexts in one process hold the same map:
what one livo_vio_select of the frame gives, stored with its image as frame 0.  Then the same frames on
both, one warm frame and `calls` timed ones, each a few cm and tenths of a degree from the last: the chain
with every array sized for the grid's cells (one call a stage, no sizing calls), then the one call.  Per
frame the two are checked to agree (state bytes, the counts); the medians, the chain's spread (max - min)
and the bytes copied each way per frame (from the stages' counts) are written to profiles/vdetect_probe.json
(OUT_DIR names another folder; the record DESIGN.md §8.6 quotes is kept as profiles/r28_vdetect_probe.json).
A record, not a bar.

usage: python tools/vdetect_probe.py [points] [calls]
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
SLOT_BYTES, OBS_BYTES, POINT_BYTES, FRAME_BYTES = 11904, 56, 56, 128  # VioSlot, VmObs, VmPoint, VmFrame


def main():
    import livo_amd
    from livo_amd import synth
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    w, h, grid, ps = 1280, 1024, 40, 8
    pst3 = 3 * ps * ps
    gray = synth._texture(w, h, np.random.default_rng(5))
    cam = dict(synth.PINHOLE, width=w, height=h, fx=960.0, fy=960.0, cx=640.0, cy=512.0, d=[0.0] * 5)
    Rci = synth.R_CI @ synth.so3_exp(np.array([0.0, 0.0, -np.radians(30.0)]))  # about half of the frame in view
    vp = livo_amd.vio_params(cam, Rci, synth.P_CI)
    vp.patch_size = ps
    raw, _, _, _ = synth.make_raw_scan(n, 4)
    s0 = synth.make_state(4)
    cells = (w // grid) * (h // grid)
    P = livo_amd._ptr
    rng = np.random.default_rng(9)
    states = [dict(s0, pos=s0["pos"] + rng.normal(0, 0.02, 3), rot=s0["rot"] @ synth.so3_exp(np.radians(rng.normal(0, 0.15, 3))))
              for _ in range(calls + 1)]
    ctxs = [livo_amd.Context(0, t_LI=synth.T_LI) for _ in range(2)]
    try:
        for ctx in ctxs:
            ctx.scan_preprocess(raw, leaf_size=0.5)
            pts, pat, _ = ctx.vio_select(s0, gray, vp, grid)
            ctx.vmap_reset(len(pts) + (calls + 2) * cells, calls + 3, ps)
            ctx.vmap_add_frame(0, s0, vp, None)
            ctx.vmap_add(0, pts, pat)
        a, b = ctxs
        L = a._L
        rec = np.zeros(cells, livo_amd.VMATCH_POINT_DTYPE)
        pos = np.zeros((cells, 3), np.float64)
        lev = np.zeros(cells, np.int32)
        mpat = np.zeros((cells, pst3), np.float32)
        sel = np.zeros(cells, livo_amd.VIS_POINT_DTYPE)
        spat = np.zeros((cells, pst3), np.float32)
        obs = np.zeros(cells, livo_amd.VOBS_POINT_DTYPE)
        nm, ns = C.c_int64(), C.c_int64()
        ms, ss, us, os_ = livo_amd.VmatchStats(), livo_amd.VisStats(), livo_amd.VioStats(), livo_amd.VobsStats()
        d = livo_amd.VdetectParams(grid, 0, 0.0, 100.0)
        ds = livo_amd.VdetectStats()

        def ok(name, rc):
            if rc:
                raise livo_amd.LivoError(name, rc)

        def chain(fid, st):
            s = livo_amd.state_to_c(st)
            ok("match", L.livo_vio_match(a.h, -1, C.byref(s), C.byref(vp), grid, 0, 0.0, 100.0, P(gray), w, h, P(rec), P(pos),
                                         P(lev), P(mpat), cells, C.byref(nm), C.byref(ms)))
            ok("select", L.livo_vio_select(a.h, -1, C.byref(s), C.byref(vp), grid, P(gray), w, h, P(sel), P(spat), cells,
                                           C.byref(ns), C.byref(ss)))
            k = nm.value
            ids = np.ascontiguousarray(rec["point_id"][:k])
            ok("update", L.livo_vio_update(a.h, C.byref(vp), P(gray), w, h, P(pos), P(lev), P(mpat), k, C.byref(s), None, None,
                                           C.byref(us)))
            ok("add_frame", L.livo_vmap_add_frame(a.h, fid, C.byref(s), C.byref(vp), P(gray), w, h))
            ok("observe", L.livo_vio_observe(a.h, fid, k, P(ids), P(lev), P(obs), C.byref(os_)))
            ok("add", L.livo_vmap_add(a.h, fid, ns.value, None, P(sel), None, P(spat), None))
            return bytes(s)

        def one(fid, st):
            s = livo_amd.state_to_c(st)
            ok("detect", L.livo_vio_detect(b.h, -1, fid, C.byref(s), None, C.byref(vp), C.byref(d), P(gray), w, h, C.byref(ds)))
            return bytes(s)

        tc, to, matched, new = [], [], [], []
        for k, st in enumerate(states):
            t0 = time.perf_counter()
            sa = chain(k + 1, st)
            t1 = time.perf_counter()
            sb = one(k + 1, st)
            t2 = time.perf_counter()
            assert sa == sb and (ds.n_matched, ds.n_new) == (nm.value, ns.value), "the two forms disagree"
            if k > 0:  # (frame 1 allocates)
                tc.append((t1 - t0) * 1e3)
                to.append((t2 - t1) * 1e3)
                matched.append(nm.value)
                new.append(ns.value)
        assert [x.tobytes() for x in a.vmap_dump()] == [x.tobytes() for x in b.vmap_dump()], "the maps differ"
        m, q, img = statistics.median(matched), statistics.median(new), w * h
        res = {"points": n, "image": [w, h], "grid_size": grid, "patch_size": ps, "frames": calls,
               "survivors_median": m, "new_points_median": q,
               "chain_ms": {"median": round(statistics.median(tc), 4), "min": round(min(tc), 4), "max": round(max(tc), 4)},
               "detect_ms": {"median": round(statistics.median(to), 4), "min": round(min(to), 4), "max": round(max(to), 4)},
               # per frame, at the median counts: four images, the update's arrays and slot, the ids and levels,
               # the staged observations, patches, places and points / every stage's results and counters
               "chain_bytes_to_device": int(4 * img + m * (24 + 4 + 4 * pst3) + SLOT_BYTES + 8 * m + FRAME_BYTES
                                            + q * (OBS_BYTES + 4 * pst3 + 12 + POINT_BYTES)),
               "chain_bytes_to_host": int(96 + m * (48 + 24 + 4 + 4 * pst3) + 32 + q * (64 + 4 * pst3) + SLOT_BYTES + 56 + 56 * m),
               "detect_bytes_to_device": int(img + SLOT_BYTES),
               "detect_bytes_to_host": int(96 + 32 + SLOT_BYTES + 56 + 56 * m + FRAME_BYTES)}
        res["chain_spread_ms"] = round(res["chain_ms"]["max"] - res["chain_ms"]["min"], 4)
        res["detect_over_chain"] = round(res["detect_ms"]["median"] / res["chain_ms"]["median"], 3)
    finally:
        for ctx in ctxs:
            ctx.close()
    out = os.path.join(ROOT, os.environ.get("OUT_DIR", "profiles"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "vdetect_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
