"""Scenes that steer an iVox query down a chosen branch of the search cascade
(fast-livo-noted_amd/csrc/ivox_kernels.hip), shared by the GPU comparison
(tests/test_gpu_ivox_cascade.py) and its CPU companion (tests/test_ivox_oracle.py), which checks with
numpy alone that every scene is what it claims to be.

Geometry.  Resolution 1.0, so cell 0 spans [-0.5, 0.5) under Pos2Grid's half-away rounding, and queries
on the x axis at x = -j 2^-12 (j < 64, all in cell 0; left_edge_queries where the neighbour's points
must be the nearest).  A "rank" r is placed at x = (1 + r) 2^-12 in cell
0, or at x = -0.5 - (1 + r) 2^-12 in the neighbour cell (-1, 0, 0), with y = z = 0: every squared
distance is an integer multiple of 2^-24 below 2^24 of them, hence exact in float32 and strictly
increasing in r for every such query.  A grid keeps insertion order, so a grid filled in the order of
an adversarial rank sequence (tests/native/nth_adversary.h) stages that sequence.

The constants restate the code's (kIvTeamCap, kIvCap, kWRaw, the 64 KB of dynamic LDS at 12 bytes an
entry, and the nearby count of each NearbyType from livo_ivox_init).
"""
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = np.float32(2.0 ** -12)
TEAM_CAP = 128      # kIvTeamCap
THREAD_CAP = 128    # kIvCap
WRAW = 512          # kWRaw
LDS_BYTES = 65536   # launch_ivox_knn: slice * kBigEntryBytes <= 65536 -> k_ivox_knn_big_wave
ENTRY_BYTES = 12    # kBigEntryBytes
NEARBY = {0: 1, 6: 7, 18: 19, 26: 27}  # livo_ivox_init
KNN = 5
MAX_KEY = (1 << 20) - 64  # kIvMaxKey

NEAR26 = [(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (1, 1, 0), (-1, 1, 0),
          (1, -1, 0), (-1, -1, 0), (1, 0, 1), (-1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 1), (0, -1, 1),
          (0, 1, -1), (0, -1, -1), (1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, 1), (-1, 1, -1),
          (1, -1, -1), (-1, -1, -1)]


# ----------------------------------------------------------- the adversary's command line ----
def build_cli(out_dir) -> str:
    """tests/native/nth_adversary_cli.cpp compiled with g++ into out_dir (as sel_check is)."""
    exe = os.path.join(str(out_dir), "nth_adversary_cli")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "fast-livo-noted_amd", "csrc"),
                               os.path.join(ROOT, "tests", "native", "nth_adversary_cli.cpp"), "-o", exe])
    return exe


def _status(line):
    f = dict(kv.split("=") for kv in line.split())
    return {"depth_limit": f["depth_limit"] == "1", "sel_matches_std": f["sel_matches_std"] == "1"}


@functools.lru_cache(maxsize=None)
def _gen(cli, n, first, nth, mirrored):
    out = subprocess.run([cli, "gen", str(n), str(first), str(nth), str(int(mirrored))], capture_output=True,
                         text=True, check=True).stdout.splitlines()
    return tuple(int(t) for t in out[0].split()), _status(out[1])


def adversary(cli, n, first, nth, mirrored=True):
    """(ranks, status): a permutation of 0..n-1 on which std::nth_element(a + first, a + nth, a + n)
    runs out of introselect depth, and the CLI's own verdict on it."""
    seq, st = _gen(cli, n, first, nth, bool(mirrored))
    return np.array(seq, np.int64), dict(st)


def check_keys(cli, keys, first, nth):
    """The predicate on float32 keys: does nth_element(keys + first, keys + nth, end) reach the limit."""
    args = [repr(float(np.float32(k))) for k in keys]
    out = subprocess.run([cli, "check", str(first), str(nth)] + args, capture_output=True, text=True, check=True)
    return _status(out.stdout.splitlines()[0])


# ----------------------------------------------------------------------------- geometry ----
def centre(ranks):
    r = np.asarray(ranks, np.int64)
    p = np.zeros((len(r), 3), np.float32)
    p[:, 0] = (1 + r).astype(np.float32) * S
    return p


def left(ranks):
    r = np.asarray(ranks, np.int64)
    p = np.zeros((len(r), 3), np.float32)
    p[:, 0] = np.float32(-0.5) - (1 + r).astype(np.float32) * S
    return p


def axis_queries(n=64):
    q = np.zeros((n, 3), np.float32)
    q[:, 0] = -np.arange(n, dtype=np.float32) * S
    return q


def left_edge_queries(n=64):
    """Queries of cell 0 next to its (-1, 0, 0) neighbour, at x = -0.5 + (64 - j) 2^-12: the neighbour's
    points are the nearest ones (rank r at (65 + r - j) 2^-12, exact and increasing in r), so what the
    selection on that grid's segment leaves is what the query returns, in that order."""
    q = np.zeros((n, 3), np.float32)
    q[:, 0] = np.float32(-0.5) + (64 - np.arange(n, dtype=np.float32)) * S
    return q


def extras():
    """Ordinary points in three other nearby cells, so the final selections have work:
    7 in (1, 0, 0) (its own cut to 5), 3 in (0, 1, 0), 2 in (0, 0, -1)."""
    a = np.array([[0.75 + k / 64.0, 0.0, 0.0] for k in (3, 0, 6, 1, 5, 2, 4)], np.float32)
    b = np.array([[0.0, 0.75 + k / 32.0, 0.0] for k in (1, 0, 2)], np.float32)
    c = np.array([[0.0, 0.0, -0.875 - k / 16.0] for k in (0, 1)], np.float32)
    return np.concatenate([a, b, c])


def _scene(name, points, queries=None, res=1.0, nearby_type=18, max_num=KNN, max_range=5.0, adv=(), **expect):
    return {"name": name, "points": np.ascontiguousarray(points, np.float32),
            "queries": axis_queries() if queries is None else np.ascontiguousarray(queries, np.float32),
            "res": res, "nearby_type": nearby_type, "max_num": max_num, "max_range": max_range,
            "adv": tuple(adv), "expect": expect}


# ------------------------------------------------------------------------------- scenes ----
# (first, length): 24..128 stay in the team (and, up to a list of 128, in the per-thread kind); 300 is
# loaded all at once by the wave search (raw <= 512), 500 / 501 stream (raw > 512, list <= 512), 600
# outgrows the wave search: all of those reach k_ivox_knn_big_wave, which runs out of depth as well
DEPTH_CASES = [(0, 24), (0, 64), (0, 128), (5, 24), (5, 64), (5, 123), (0, 300), (5, 300), (0, 501), (5, 500),
               (0, 600), (5, 600)]


def depth_scene(cli, first, length):
    """One adversarial grid of `length` points selected at nth = first + 4.  first = 0: the centre grid.
    first = 5: the (-1, 0, 0) neighbour of a centre grid of 7 ordinary points (cut to 5 survivors), so
    the staged segment starts at 5.  adv: (nearby grid ordinal, first, length)."""
    seq, st = adversary(cli, first + length, first, first + 4)
    assert st["depth_limit"] and st["sel_matches_std"]
    ranks = seq[first:]
    if first == 0:
        pts = [centre(ranks)]
        raw = length
    else:
        # (the centre's points lie beyond the neighbour's from the queries at the cell's left edge:
        # its survivors fill the segment's first 5 places and then lose the final cut)
        pts = [centre(1500 + np.array([3, 0, 6, 2, 5, 1, 4])), left(ranks)]
        raw = 7 + length
    pts.append(extras())
    return _scene(f"depth-{first}-{length}", np.concatenate(pts),
                  queries=axis_queries() if first == 0 else left_edge_queries(),
                  adv=[(0 if first == 0 else 1, first, length)], raw=raw + 12, peak=first + length, limit=True)


def capacity_scenes():
    """List lengths at the team's and the per-thread kind's capacity (128 / 129), counted in in-range
    points only, and the wave search's staging limits (512 / 513 raw, 512 / 513 staged)."""
    rng = np.random.default_rng(17)

    def perm(n):
        return rng.permutation(n)
    far = lambda n: np.stack([np.float32(0.3) + np.arange(n, dtype=np.float32) * S, np.zeros(n, np.float32),
                              np.zeros(n, np.float32)], 1)  # cell 0, beyond max_range 0.25 of every query
    right_out = lambda n: np.stack([np.float32(0.8) + np.arange(n, dtype=np.float32) / np.float32(64),
                                    np.zeros(n, np.float32), np.zeros(n, np.float32)], 1)  # cell (1, 0, 0), > 0.75 away
    five = centre([3, 0, 4, 1, 2])

    def mixed(n_in, n_far, at):  # n_far out-of-range points inserted after the first `at` in-range ones
        c = centre(perm(n_in))
        return np.concatenate([c[:at], far(n_far), c[at:]])
    sc = [
        _scene("one-grid-128", centre(perm(128)), raw=128, peak=128, limit=False),
        _scene("one-grid-129", centre(perm(129)), raw=129, peak=129, limit=False),
        _scene("5+123", np.concatenate([five, left(perm(123))]), raw=128, peak=128, limit=False),
        _scene("5+124", np.concatenate([five, left(perm(124))]), raw=129, peak=129, limit=False),
        # only in-range points count: 40 more of the same grid lie beyond max_range
        _scene("128-in-range-of-168", mixed(128, 40, 60), max_range=0.25, raw=168, peak=128, limit=False),
        _scene("129-in-range-of-169", mixed(129, 40, 60), max_range=0.25, raw=169, peak=129, limit=False),
        # the wave search: every raw point at once up to 512, streaming past that
        _scene("raw-512", centre(perm(512)), raw=512, peak=512, limit=False),
        _scene("raw-513-one-grid", centre(perm(513)), raw=513, peak=513, limit=False),
        _scene("raw-513-streams", np.concatenate([centre(perm(7)), left(perm(506))]), raw=513, peak=511, limit=False),
        _scene("stream-5+507", np.concatenate([five, left(perm(507)), right_out(10)]), max_range=0.75, raw=522,
               peak=512, limit=False),
        _scene("stream-5+508", np.concatenate([five, left(perm(508)), right_out(10)]), max_range=0.75, raw=523,
               peak=513, limit=False),
        _scene("stream-out-of-range", mixed(300, 300, 100), max_range=0.25, raw=600, peak=300, limit=False),
    ]
    return sc


LDS_NEARBY_TYPE = 6


def lds_edge_grid():
    """The largest grid whose big-pass slice (nearby x 5 + grid + 8 entries, ivox_ensure_big) still fits
    64 KB of dynamic LDS at 12 bytes an entry."""
    slice_max = LDS_BYTES // ENTRY_BYTES
    return slice_max - NEARBY[LDS_NEARBY_TYPE] * KNN - 8


def lds_scene(over):
    """One grid of lds_edge_grid() (+ 1 when over) points on a 2^-8 lattice of cell 0 in shuffled order
    (coordinates k 2^-8, |k| <= 384 with the queries': squares exact, many exact ties: (i, j) / (j, i),
    mirrored pairs), a few points in the x and y neighbours; queries on the same lattice in cell 0 and
    in its six neighbours."""
    g = lds_edge_grid() + (1 if over else 0)
    rng = np.random.default_rng(23)
    ij = np.stack(np.meshgrid(np.arange(-37, 37), np.arange(-37, 37), indexing="ij"), -1).reshape(-1, 2)
    assert len(ij) >= g
    ij = ij[rng.permutation(len(ij))[:g]]
    pts = np.zeros((g, 3), np.float32)
    pts[:, :2] = ij.astype(np.float32) / np.float32(256)
    nb = np.array([[1.0, 0.0, 0.0], [0.75, 0.25, 0.0], [0.0, -1.0, 0.0], [-0.75, 0.0, 0.0], [0.0, 0.0, 0.75],
                   [0.0, 0.0, 0.75]], np.float32)
    q = np.zeros((160, 3), np.float32)
    q[:, :2] = rng.integers(-120, 121, size=(160, 2)).astype(np.float32) / np.float32(256)
    cell = np.array(NEAR26[:7], np.float32)[rng.integers(0, 7, size=160)]
    q += cell  # (cell 0 and each of its six neighbours)
    q[:16] = 0.0
    q[:16, 0] = np.arange(16, dtype=np.float32) / np.float32(256)  # on lattice points: distance 0 and ties
    return _scene("lds-over" if over else "lds-edge", np.concatenate([pts, nb]), queries=q,
                  nearby_type=LDS_NEARBY_TYPE, max_grid=g, slice=NEARBY[LDS_NEARBY_TYPE] * KNN + g + 8)


# ------------------------------------------------------- numpy restatement of the bookkeeping ----
def round_half_away(x):
    x = np.asarray(x, np.float32)
    return np.where(x >= 0, np.floor(x + np.float32(0.5)), -np.floor(-x + np.float32(0.5)))


def keys_of(p, res):
    inv = np.float32(1.0 / float(np.float32(res)))
    return round_half_away(np.asarray(p, np.float32) * inv).astype(np.int64)


def dist2(p, q):
    d = np.asarray(p, np.float32) - np.asarray(q, np.float32)
    return d[..., 0] * d[..., 0] + (d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])


def trace(scene, q):
    """What GetClosestPoint stages for query q: raw = points of all nearby grids, counts = in-range points
    per nearby grid (in the reference's grid order), peak = the longest the list gets (survivors so far +
    the current grid's in-range points), segs = per grid (first, in-range keys in insertion order)."""
    pts, res, K = scene["points"], scene["res"], scene["max_num"]
    pk = keys_of(pts, res)
    qk = keys_of(q[None], res)[0]
    r2 = float(scene["max_range"]) * float(scene["max_range"])
    raw, n, peak, counts, segs = 0, 0, 0, [], []
    for dl in NEAR26[:NEARBY[scene["nearby_type"]]]:
        sel = np.flatnonzero(np.all(pk == qk + np.array(dl), axis=1))
        raw += len(sel)
        d = dist2(pts[sel], q)
        keep = d.astype(np.float64) < r2
        m = int(keep.sum())
        counts.append(m)
        segs.append((n, d[keep]))
        peak = max(peak, n + m)
        n += min(m, K)
    return {"raw": raw, "counts": counts, "peak": peak, "segs": segs, "final": n}


def route(tr, limit, slice_entries):
    """The kernel that answers a query under the default kind, from its trace: 'team'; 'wave-all' /
    'wave-stream' (k_ivox_knn_wave_list); 'big-wave' / 'big-wave-lane0' (its depth-limit fallback) /
    'big-global' (k_ivox_knn_big)."""
    if tr["peak"] <= TEAM_CAP:
        return "team"  # (the team heap-selects its own depth-limit cases)
    if tr["raw"] <= WRAW:
        if not limit:
            return "wave-all"
    elif tr["peak"] <= WRAW and not limit:
        return "wave-stream"
    if slice_entries * ENTRY_BYTES > LDS_BYTES:
        return "big-global"
    return "big-wave-lane0" if limit else "big-wave"


def by_grid_dev(xyz, ids, keys):
    g = {}
    for p, i, k in zip(xyz, ids, map(tuple, keys)):
        g.setdefault(tuple(int(v) for v in k), []).append((int(i), tuple(p.tolist())))
    return g


def by_grid_oracle(iv):
    xyz, ids, gof, keys = iv.dump()
    g = {}
    for p, i, go in zip(xyz, ids, gof):
        g.setdefault(tuple(int(v) for v in keys[go]), []).append((int(i), tuple(p.tolist())))
    return g


# ------------------------------------------------------------------------ keys and range ----
def half_product_points(res):
    """Coordinates whose float32 product with inv_resolution is exactly k + 0.5 (both signs of k), the
    floats one ulp either side, and -0.0; returned with the mask of the exact half products."""
    inv = np.float32(1.0 / float(np.float32(res)))
    vals, exact = [], []
    for k in range(-6, 6):
        v0 = np.float32((k + 0.5) / float(inv))
        for v in (v0, np.nextafter(v0, np.float32(np.inf)), np.nextafter(v0, np.float32(-np.inf))):
            vals.append(v)
            exact.append(float(np.float32(v * inv)) == k + 0.5)
    vals.append(np.float32(-0.0))
    exact.append(False)
    v = np.array(vals, np.float32)
    pts = np.concatenate([np.stack([v, np.zeros_like(v), np.zeros_like(v)], 1),
                          np.stack([np.zeros_like(v), v, v[::-1]], 1)])
    return pts, np.array(exact)
