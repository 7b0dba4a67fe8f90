"""The camera-frame stages interleaved on one context: livo_vio_select, livo_cloud_colorize,
livo_vio_update, livo_scan_preprocess and livo_frame_to_world share the context's grow-only device
buffers (the scratch, the selection's table and records, the VIO frame, the front end's arrays, the
rocPRIM scratch) and its two retained images.  Every other test drives one stage on a context of its
own; here one context runs them in an order in which each buffer is reallocated while another stage
holds something it must not lose, then once more on smaller inputs, so that a stale tail of a buffer
that did not shrink would be read if a count were wrong.

Bar: every output is byte-equal to the same call on a fresh context that has done nothing else (for a
call with image = None: the fresh context's call with the image).  The BGR and the gray image stay
apart: an upload of one never serves the other stage's image = None.
"""
import ctypes as C

import numpy as np
import pytest
from test_rgb_cloud_abi import CAM_DIST, random_image
from test_vis_select_abi import FRAMES, frame_case, frame_image

pytestmark = pytest.mark.gpu


def _ctx():
    import livo_amd
    from livo_amd import synth
    return livo_amd.Context(0, t_LI=synth.T_LI)


def _vis(name):
    import livo_amd
    img, cam, Rci, Pci = frame_image(name)
    vp = livo_amd.vio_params(cam, Rci, Pci)
    vp.patch_size = FRAMES[name][2]
    return img, vp, FRAMES[name][3]


def _sel(res):
    pts, pat, stats = res
    return pts.tobytes(), pat.tobytes(), stats


def _col(res):
    pts, idx, stats = res
    return pts.tobytes(), idx.tobytes(), stats


def _vio(res):
    s, stats, err = res
    return b"".join(np.ascontiguousarray(s[k]).tobytes() for k in sorted(s)), \
        {k: (np.float32(v).tobytes() if k == "last_error" else v) for k, v in stats.items()}, err.tobytes()


def _pre(res):
    _, und, down = res
    return und.tobytes(), down.tobytes()


def _fresh(call, body=None, raw=None):
    """`call(ctx, sid)` on a context that has only uploaded `body` or preprocessed `raw` (sid: that scan)."""
    with _ctx() as ctx:
        sid = -1
        if body is not None:
            sid = ctx.scan_upload(body)
        if raw is not None:
            sid = ctx.scan_preprocess(*raw, leaf_size=0.5)[0]
        return call(ctx, sid)


def test_interleaved_stages_equal_fresh_contexts(built):
    import livo_amd
    from livo_amd import synth
    st_s, body_s = frame_case("160x128-g20", 65)
    st_l, body_l = frame_case("160x152-g40", 3000)
    img_a, vp_a, grid_a = _vis("160x128-g20")
    img_b, vp_b, grid_b = _vis("160x152-g40")
    img_c, vp_c, grid_c = _vis("160x152-g20")  # more cells than either: the selection's buffer grows
    bgr = random_image()  # 64 x 48
    vp_rgb = livo_amd.vio_params(CAM_DIST, synth.R_CI, synth.P_CI)
    fr300, st300, _ = synth.make_vio_frame(300, 1)
    fr100, st100, _ = synth.make_vio_frame(100, 3)
    raw1500, raw700 = synth.make_raw_scan(1500, 3), synth.make_raw_scan(700, 2)
    st_p, st_q = synth.make_state(3), synth.make_state(2)

    # what fresh contexts give
    want_sel_a = _fresh(lambda c, s: _sel(c.vio_select(st_s, img_a, vp_a, grid_a, s)), body=body_s)
    want_col_l = _fresh(lambda c, s: _col(c.colorize(st_l, bgr, vp_rgb, s)), body=body_l)
    want_sel_b = _fresh(lambda c, s: _sel(c.vio_select(st_l, img_b, vp_b, grid_b, s)), body=body_l)
    want_sel_c = _fresh(lambda c, s: _sel(c.vio_select(st_l, img_c, vp_c, grid_c, s)), body=body_l)
    want_vio300 = _fresh(lambda c, s: _vio(c.vio_update(fr300, st300)))
    want_vio100 = _fresh(lambda c, s: _vio(c.vio_update(fr100, st100)))
    want_col_s = _fresh(lambda c, s: _col(c.colorize(st_s, bgr, vp_rgb, s)), body=body_s)
    want_world_s = _fresh(lambda c, s: c.frame_to_world(st_s, s).tobytes(), body=body_s)
    want_frame = {}
    for key, raw, st in (("p", raw1500, st_p), ("q", raw700, st_q)):
        with _ctx() as ctx:
            res = ctx.scan_preprocess(*raw, leaf_size=0.5)
            want_frame[key] = {"pre": _pre(res), "world": ctx.frame_to_world(st, -1).tobytes(),
                               "down": ctx.frame_to_world(st, res[0]).tobytes(),
                               "col": _col(ctx.colorize(st, bgr, vp_rgb, -1))}
        want_frame[key]["sel"] = _fresh(lambda c, s: _sel(c.vio_select(st, img_a, vp_a, grid_a, -1)), raw=raw)
    # the cases are worth running: some points kept and some dropped, some cells selected
    assert 0 < want_col_l[2]["n_out"] < 3000 and 0 < want_col_s[2]["n_out"] < 65
    assert want_sel_a[2]["n_out"] > 0 and want_sel_b[2]["n_out"] > 0 and want_sel_c[2]["n_out"] > want_sel_b[2]["n_out"]
    assert 0 < want_frame["p"]["col"][2]["n_out"] < 1500 and len(want_frame["q"]["world"]) == 700 * 20

    with _ctx() as ctx:
        sid_s, sid_l = ctx.scan_upload(body_s), ctx.scan_upload(body_l)                      # 1
        assert _sel(ctx.vio_select(st_s, img_a, vp_a, grid_a, sid_s)) == want_sel_a          # 2
        assert _col(ctx.colorize(st_l, bgr, vp_rgb, sid_l)) == want_col_l                    # 3: the scratch grows
        assert _sel(ctx.vio_select(st_s, None, vp_a, grid_a, sid_s)) == want_sel_a           # 4: its image is there
        assert _sel(ctx.vio_select(st_l, img_b, vp_b, grid_b, sid_l)) == want_sel_b          # 5: a larger image
        assert _sel(ctx.vio_select(st_l, img_c, vp_c, grid_c, sid_l)) == want_sel_c          # ... and more cells
        assert _col(ctx.colorize(st_l, None, vp_rgb, sid_l)) == want_col_l
        assert _vio(ctx.vio_update(fr300, st300)) == want_vio300                             # 6
        pre = ctx.scan_preprocess(*raw1500, leaf_size=0.5)                                   # 7
        assert _pre(pre) == want_frame["p"]["pre"]
        assert _col(ctx.colorize(st_l, None, vp_rgb, sid_l)) == want_col_l                   # 8
        assert _sel(ctx.vio_select(st_l, None, vp_c, grid_c, sid_l)) == want_sel_c
        assert ctx.frame_to_world(st_p, -1).tobytes() == want_frame["p"]["world"]            # 9: the new frame
        assert _col(ctx.colorize(st_p, None, vp_rgb, -1)) == want_frame["p"]["col"]
        assert ctx.frame_to_world(st_p, pre[0]).tobytes() == want_frame["p"]["down"]
        assert _sel(ctx.vio_select(st_p, img_a, vp_a, grid_a, -1)) == want_frame["p"]["sel"]
        pre2 = ctx.scan_preprocess(*raw700, leaf_size=0.5)                                   # 10: a smaller frame
        assert _pre(pre2) == want_frame["q"]["pre"]
        # 11: every stage once more, on inputs smaller than its buffers
        assert ctx.frame_to_world(st_q, -1).tobytes() == want_frame["q"]["world"]
        assert ctx.frame_to_world(st_q, pre2[0]).tobytes() == want_frame["q"]["down"]
        assert _col(ctx.colorize(st_q, None, vp_rgb, -1)) == want_frame["q"]["col"]
        assert _sel(ctx.vio_select(st_q, None, vp_a, grid_a, -1)) == want_frame["q"]["sel"]
        assert _vio(ctx.vio_update(fr100, st100)) == want_vio100
        assert _sel(ctx.vio_select(st_s, img_a, vp_a, grid_a, sid_s)) == want_sel_a
        assert _col(ctx.colorize(st_s, bgr, vp_rgb, sid_s)) == want_col_s
        assert ctx.frame_to_world(st_s, sid_s).tobytes() == want_world_s
        assert _sel(ctx.vio_select(st_l, img_b, vp_b, grid_b, sid_l)) == want_sel_b
        assert _col(ctx.colorize(st_l, None, vp_rgb, sid_l)) == want_col_l
        # the frame of step 7 is gone, the downsampled scan it left is not
        assert ctx.frame_to_world(st_p, pre[0]).tobytes() == want_frame["p"]["down"]


def _select_rc(ctx, st, vp, grid, img, sid):
    import livo_amd
    n, s = C.c_int64(-7), livo_amd.state_to_c(st)
    return ctx._L.livo_vio_select(ctx.h, sid, C.byref(s), C.byref(vp), grid, livo_amd._ptr(img), vp.cam.width,
                                  vp.cam.height, None, None, 0, C.byref(n), None)


def _colorize_rc(ctx, st, vp, img, sid):
    import livo_amd
    n, s = C.c_int64(-7), livo_amd.state_to_c(st)
    return ctx._L.livo_cloud_colorize(ctx.h, sid, C.byref(s), C.byref(vp), livo_amd._ptr(img), vp.cam.width,
                                      vp.cam.height, None, None, 0, C.byref(n), None)


def test_the_two_images_stay_apart(built):
    """A BGR and a gray image of the same 160 x 128: each stage's image = None sees only its own upload."""
    st, body = frame_case("160x128-g20", 65)
    gray, vp, grid = _vis("160x128-g20")
    bgr = random_image(160, 128)
    with _ctx() as ctx:
        sid = ctx.scan_upload(body)
        assert _colorize_rc(ctx, st, vp, bgr, sid) == 0
        assert _select_rc(ctx, st, vp, grid, None, sid) == -1  # LIVO_E_INVALID: no gray image yet
        assert _colorize_rc(ctx, st, vp, None, sid) == 0
    with _ctx() as ctx:
        sid = ctx.scan_upload(body)
        assert _select_rc(ctx, st, vp, grid, gray, sid) == 0
        assert _colorize_rc(ctx, st, vp, None, sid) == -1  # LIVO_E_INVALID: no BGR image yet
        assert _select_rc(ctx, st, vp, grid, None, sid) == 0
        # each upload leaves the other's image as it was
        assert _colorize_rc(ctx, st, vp, bgr, sid) == 0
        assert _select_rc(ctx, st, vp, grid, None, sid) == 0
        want = _fresh(lambda c, s: _sel(c.vio_select(st, gray, vp, grid, s)), body=body)
        assert _sel(ctx.vio_select(st, None, vp, grid, sid)) == want
