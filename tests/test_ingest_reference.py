"""The two restatements of the sensor handlers, the time sort and the slice (tests/ingest_cases.py)
agree bit for bit on every case the GPU tests run, and each quirk of the reference's handlers is
checked on a message worked out by hand.  CPU only; tests/test_gpu_ingest.py holds the device.
"""
import numpy as np
import pytest

import ingest_cases as ic

F = np.float32


def _same(a, b):
    fa, ia = a
    fb, ib = b
    assert fa.shape == fb.shape and np.array_equal(fa.view(np.uint32), fb.view(np.uint32))
    assert {k: (v if k != "end_curvature" else F(v).view(np.uint32)) for k, v in ia.items()} == \
           {k: (v if k != "end_curvature" else F(v).view(np.uint32)) for k, v in ib.items()}


@pytest.mark.parametrize("n", ic.SIZES)
def test_restatements_agree_on_avia(n):
    for p in (1, 2, 3, 7):
        for density, run in (("none", 0), ("all", 0), ("half", 0), ("half", 300)):
            m = ic.livox_msg(n, density, "random", seed=n + p, run=run)
            _same(ic.ingest_scalar(ic.AVIA, m, filter_num=p), ic.ingest_vector(ic.AVIA, m, filter_num=p))


@pytest.mark.parametrize("kind,layout", [(ic.OUST64, "ouster"), (ic.VELO16, "velodyne"), (ic.XT32, "hesai"),
                                         (ic.OUST64, "shuffled48"), (ic.VELO16, "shuffled48"),
                                         (ic.XT32, "shuffled48")])
def test_restatements_agree_on_clouds(kind, layout):
    L = ic.LAYOUTS[layout]
    for n in (0, 1, 65, ic.BLOCK + 1, 3 * ic.BLOCK + 17):
        for times in ("sorted", "reversed", "random", "ties"):
            d = ic.cloud_msg(kind, n, L, times, seed=n, negative=(kind == ic.XT32 and times == "random"))
            for p in (1, 3):
                a = ic.ingest_scalar(kind, d, L, filter_num=p, blind=0.5)
                _same(a, ic.ingest_vector(kind, d, L, filter_num=p, blind=0.5))
                if n > 100 and p == 1:
                    assert 0 < a[1]["n_rejected"] < n


def test_restated_slices_agree():
    m = ic.livox_msg(3 * ic.BLOCK + 17, "all", "ties", seed=5)
    frame, info = ic.ingest_scalar(ic.AVIA, m, filter_num=1)
    for cursor in (0, 1, 100, len(frame)):
        for lim in (-1.0, 0.0, float(frame[150, 4]), float(frame[-1, 4]), 1e9):
            for end in (False, True):
                assert ic.take_scalar(frame, cursor, lim, end) == ic.take_vector(frame, cursor, lim, end)


def _avia(rows):
    """rows: (x, y, z, tag, line, offset_time)"""
    m = np.zeros(len(rows), ic.LIVOX)
    for k, r in enumerate(rows):
        m[k] = (r[5], r[0], r[1], r[2], 200, r[3], r[4], 0)
    return m


def _both(kind, msg, layout=None, **kw):
    a = ic.ingest_scalar(kind, msg, layout, **kw)
    _same(a, ic.ingest_vector(kind, msg, layout, **kw))
    return a


def test_avia_point_zero_is_never_emitted():
    m = _avia([(5, 1, 1, 0x10, 0, 10), (6, 2, 2, 0x10, 0, 20), (7, 3, 3, 0x10, 0, 30)])
    frame, info = _both(ic.AVIA, m, filter_num=1)
    assert frame[:, 0].tolist() == [6, 7] and info["n_rejected"] == 1 and info["n_kept"] == 2
    frame, info = _both(ic.AVIA, m[:1], filter_num=1)
    assert len(frame) == 0 and info == {"n_in": 1, "n_kept": 0, "cursor": 0, "n_rejected": 1, "n_decimated": 0,
                                        "end_curvature": 0}
    # intensity is the range, not the reflectivity; curvature is offset_time / 1e6 in float
    frame, _ = _both(ic.AVIA, _avia([(0, 0, 0, 0x10, 0, 0), (3, 4, 12, 0x10, 0, 2_500_000)]), filter_num=1)
    assert frame.tolist() == [[3, 4, 12, 13, 2.5]]


def test_avia_line_tag_and_filter_count():
    # line == n_scans passes, n_scans + 1 does not
    m = _avia([(1, 1, 1, 0x10, 0, 0), (5, 2, 2, 0x10, 16, 1), (6, 3, 3, 0x10, 17, 2), (7, 4, 4, 0x10, 15, 3)])
    frame, _ = _both(ic.AVIA, m, n_scans=16, filter_num=1)
    assert frame[:, 0].tolist() == [5, 7]
    # tag & 0x30 must be 0x10, whatever the other bits are
    tags = [0x00, 0x10, 0x20, 0x30, 0xCF, 0xDF, 0xEF, 0xFF, 0x1F, 0x91]
    m = _avia([(1, 1, 1, 0x10, 0, 0)] + [(5 + k, 2 + k, 2 + k, t, 0, k) for k, t in enumerate(tags)])
    frame, info = _both(ic.AVIA, m, filter_num=1)
    assert frame[:, 0].tolist() == [5 + k for k, t in enumerate(tags) if t & 0x30 == 0x10] == [6, 10, 13, 14]
    # the 1-in-p count runs over the survivors, not over the message index
    m = _avia([(1, 1, 1, 0x10, 0, 0)] + [(5 + k, 2 + k, 2 + k, 0x10 if k % 3 else 0x00, 0, k) for k in range(12)])
    frame, info = _both(ic.AVIA, m, filter_num=3)
    surv = [5 + k for k in range(12) if k % 3]
    assert frame[:, 0].tolist() == surv[2::3] and info["n_decimated"] == len(surv) - len(surv[2::3])


def test_avia_duplicates_are_measured_against_the_previous_message_point():
    # point 2 is rejected by its tag; points 3, 4, 5 repeat its x, y, z in turn and fall with it,
    # point 6 differs from point 5 in all three
    m = _avia([(1, 1, 1, 0x10, 0, 0), (5, 5, 5, 0x10, 0, 1), (6, 6, 6, 0x00, 0, 2), (6, 7, 7, 0x10, 0, 3),
               (8, 7, 8, 0x10, 0, 4), (9, 9, 8, 0x10, 0, 5), (10, 10, 10, 0x10, 0, 6)])
    frame, _ = _both(ic.AVIA, m, filter_num=1)
    assert frame[:, 0].tolist() == [5, 10]
    # a difference of one float step at 1.0 (1.2e-7) is no duplicate; an exact repeat is
    x1 = float(np.nextafter(F(1), F(2)))
    m = _avia([(2, 2, 2, 0x10, 0, 0), (1, 1, 1, 0x10, 0, 1), (x1, 1.5, 1.5, 0x10, 0, 2), (x1, 3, 3, 0x10, 0, 3)])
    frame, _ = _both(ic.AVIA, m, filter_num=1)
    assert frame[:, 4].tolist() == [F(1) / F(1000000), F(2) / F(1000000)]


def test_avia_range_limits_as_written():
    # range = x^2 + y^2 (no z) against blind unsquared: exactly blind is kept; exactly 900 is kept
    m = _avia([(9, 9, 9, 0x10, 0, 0), (0.5, 0, 7, 0x10, 0, 1), (0.49, 0.01, 8, 0x10, 0, 2), (30, 0.001, 20, 0x10, 0, 3),
               (18, 24, 1, 0x10, 0, 4), (18, 24.001, 2, 0x10, 0, 5)])
    frame, _ = _both(ic.AVIA, m, filter_num=1, blind=0.25)
    # (30^2 + 0.001^2 rounds to 900 in float and stays; 18^2 + 24.001^2 = 900.048 goes)
    assert frame[:, 2].tolist() == [7, 20, 1]
    assert float(F(30) * F(30) + F(0.001) * F(0.001)) == 900 and F(0.49) * F(0.49) + F(0.01) * F(0.01) < 0.25


def _cloud(kind, layout, rows):
    """rows: (x, y, z, intensity, time)"""
    L = ic.LAYOUTS[layout]
    d = np.zeros((len(rows), L["point_step"]), np.uint8)
    for i, r in enumerate(rows):
        for k, v in zip(("off_x", "off_y", "off_z", "off_intensity"), r[:4]):
            d[i, L[k]:L[k] + 4] = np.array([v], F).view(np.uint8)
        t = np.array([r[4]], {ic.OUST64: np.uint32, ic.VELO16: F, ic.XT32: np.float64}[kind]).view(np.uint8)
        d[i, L["off_time"]:L["off_time"] + t.size] = t
    return d, L


def test_blind_edges_of_the_cloud_handlers():
    # r^2 == blind^2 exactly (3, 4, 0 against 5): kept by OUST64, dropped by VELO16
    rows = [(3, 4, 0, 9, 1), (3, 4, 0.01, 9, 2), (3, 3.99, 0, 9, 3)]
    d, L = _cloud(ic.OUST64, "ouster", rows)
    frame, _ = _both(ic.OUST64, d, L, filter_num=1, blind=5.0)
    assert frame[:, 4].tolist() == [F(1) * F(1e-6), F(2) * F(1e-6)] and frame[0, 3] == 5  # intensity = range
    d, L = _cloud(ic.VELO16, "velodyne", rows)
    frame, _ = _both(ic.VELO16, d, L, filter_num=1, blind=5.0)
    assert frame[:, 4].tolist() == [F(2) * F(1e-3)] and frame[0, 3] == 9  # intensity = the message's
    # XT32 compares r^2 with blind unsquared: r = 2 (r^2 = 4) against blind 4 and 3.9
    d, L = _cloud(ic.XT32, "hesai", [(2, 0, 0, 9, 100.0), (0, 2.1, 0, 8, 100.25), (0, 0, 1.9, 7, 99.5)])
    frame, info = _both(ic.XT32, d, L, filter_num=1, blind=4.0)
    assert frame.tolist() == [[0, F(2.1), 0, 8, 250]] and info["n_rejected"] == 2
    frame, _ = _both(ic.XT32, d, L, filter_num=1, blind=3.6)
    assert frame[:, 4].tolist() == [-500, 0, 250]  # times before points[0]'s are negative and sort first
    # the message index, not the survivor count, is filtered: i % 2 == 0 of points 0..2
    frame, info = _both(ic.XT32, d, L, filter_num=2, blind=3.6)
    assert frame[:, 4].tolist() == [-500, 0] and info["n_decimated"] == 1 and info["n_rejected"] == 0


def test_empty_frames():
    for kind, layout in ((ic.OUST64, "ouster"), (ic.VELO16, "velodyne"), (ic.XT32, "hesai")):
        L = ic.LAYOUTS[layout]
        frame, info = _both(kind, np.zeros((0, L["point_step"]), np.uint8), L)
        assert frame.shape == (0, 5) and info["n_kept"] == 0 and info["end_curvature"] == 0
    frame, info = _both(ic.AVIA, np.zeros(0, ic.LIVOX))
    assert frame.shape == (0, 5) and info["end_curvature"] == 0 and info["n_in"] == 0
    assert ic.take_scalar(frame, 0, 1e9, True) == ic.take_vector(frame, 0, 1e9, True) == (0, 0)


def test_sort_keeps_ties_in_message_order_and_signed_zeros_apart():
    d, L = _cloud(ic.XT32, "hesai", [(9, 0, 0, 0, 50.0), (8, 0, 0, 1, 50.0), (7, 0, 0, 2, 49.0), (6, 0, 0, 3, 50.0),
                                     (5, 0, 0, 4, 49.0)])
    frame, info = _both(ic.XT32, d, L, filter_num=1, blind=1.0)
    assert frame[:, 3].tolist() == [2, 4, 0, 1, 3] and info["end_curvature"] == 0
    rows = np.array([[0, 0, 0, 0, 0.0], [1, 0, 0, 0, -0.0], [2, 0, 0, 0, 0.0], [3, 0, 0, 0, -0.0]], F)
    assert ic.sort_scalar(rows)[:, 0].tolist() == [1, 3, 0, 2]


def test_take_limit_loses_the_tail_at_a_real_stamp_and_keeps_it_at_zero():
    # three points share the last time; the round trip through lidar_beg_time = 1.7e9 s moves the
    # limit by up to 2.4e-4 ms (one step of a double at 1.7e9 s)
    m = _avia([(1, 1, 1, 0x10, 0, 0)] + [(5 + k, 2 + k, 2 + k, 0x10, 0, t) for k, t in
                                       enumerate((10_000_000, 50_000_000, 99_999_000, 99_999_000, 99_999_000))])
    frame, info = _both(ic.AVIA, m, filter_num=1)
    end = info["end_curvature"]
    assert end == F(99_999_000) / F(1000000) and len(frame) == 5
    lim0, lim = ic.take_limit(0.0, end, True), ic.take_limit(1.7e9, end, True)
    assert lim0 == float(end) and lim < float(end) and float(end) - lim < 2.4e-4
    assert ic.take_scalar(frame, 0, lim0, True) == ic.take_vector(frame, 0, lim0, True) == (5, 0)
    assert ic.take_scalar(frame, 0, lim, True) == ic.take_vector(frame, 0, lim, True) == (2, 0)


def test_camera_take_consumes_the_points_at_or_before_time_zero():
    d, L = _cloud(ic.XT32, "hesai", [(9, 0, 0, 0, 50.0), (8, 0, 0, 1, 49.99), (7, 0, 0, 2, 50.0), (6, 0, 0, 3, 50.01),
                                     (5, 0, 0, 4, 50.02)])
    frame, info = _both(ic.XT32, d, L, filter_num=1, blind=1.0)
    assert (frame[:, 4] <= 0).sum() == 3
    lim = ic.take_limit(1.7e9, info["end_curvature"], False)
    assert lim == 0.0
    assert ic.take_scalar(frame, 0, lim, False) == ic.take_vector(frame, 0, lim, False) == (3, 3)  # the image's take
    lim = ic.take_limit(1.7e9, info["end_curvature"], True)
    n, cur = ic.take_scalar(frame, 3, lim, True)
    assert (n, cur) == ic.take_vector(frame, 3, lim, True) and cur == 0 and n in (1, 2)
