"""High-precision reference of the per-point plane pass, and the neighbourhoods that exercise it.

TEST INFRASTRUCTURE ONLY (like oracle.py).  The pass is esti_plane (common_lib.h:670-702: a 5x3
column-pivoting Householder QR solve of A x = -1 in float), the residual pd2 and the gates of
h_share_model (laser_mapping.cpp:514-552): sqdis[4] > 5, s > 0.9, |pd2| <= 2.

lstsq()  the least-squares solution of A x = -1 in mpmath at DPS digits (normal equations on the
         chosen columns: the basic solution of a rank-deficient fit is the one on its pivot columns),
         the singular values of A and the residual vector, the unit normal and d = 1 / |x|.
gates()  pd2, s, the largest fit residual and the decisions, evaluated in mpmath from the float
         plane, world point and body point, each with its distance to its threshold in float ulps.
sheets() the case families.  A sheet is one small map (clusters of five points, at least SEP m
         apart, so that a query inside a cluster has exactly that cluster as its five nearest) and
         its queries; world point = body point (identity rotation, zero position, t_LI = 0) except
         on the sheet of the body point at the origin, which carries its own state.  Origin-bound
         families (a plane through the origin region, the rank-0 cluster at the origin, the tau = 0
         cluster around it) cannot share a map, hence several sheets; each sheet leaves the box
         ROOM_BOX free for a crop of the synthetic room (the tests that solve add it).
sweeps() four sweeps of 65 cases, one quantity stepped by nextafter through its threshold.

Measured on the committed cases (tests/test_plane_reference.py prints them): the largest ratio
error / (FLT_EPSILON (kappa + kappa^2 rho)) of the oracle's x = n / d is MEASURED_RATIO, so the bar
is C_BAR = 4 * ratio rounded up to a power of two.
"""
from __future__ import annotations

import mpmath as mp
import numpy as np

DPS = 60
FLT_EPS = float(np.finfo(np.float32).eps)
SEP = 8.0            # least distance between two clusters of a sheet (centre to centre, less their radii)
DIAM = 0.6           # largest cluster diameter (the tau = 0 and sweep clusters say their own)
N_SHEETS = 65        # sheet s also holds step s of the edge_thr sweep
ROOM_CROP = (np.array([15.0, -8.0]), np.array([30.0, 8.0]))               # x, y range of the room crop
ROOM_BOX = (np.array([15.0, -8.0, -1.7]), np.array([30.0, 8.0, 2.5]))     # no cluster within SEP of it
MAX_SQD, MIN_S, MAX_RES, PLANE_THR = 5.0, 0.9, 2.0, 0.1
DECIDED_ULPS = 16    # a gate quantity further than this from its threshold is decided
RANK_MARGIN = 8.0    # a rank test within this factor of its threshold is not held against the reference
FULL_RANK_RATIO = 1e-5
VOID_BOUND = 0.25      # kappa * FLT_EPSILON from which the first-order error bound says nothing
MEASURED_RATIO = 2.34   # largest error / (FLT_EPSILON (kappa + kappa^2 rho)) over the committed cases
C_BAR = 16.0            # 4 * MEASURED_RATIO rounded up to a power of two

IDENTITY = {"rot": np.eye(3), "pos": np.zeros(3), "vel": np.zeros(3), "bias_g": np.zeros(3),
            "bias_a": np.zeros(3), "gravity": np.array([0.0, 0.0, -9.81]), "cov": np.eye(18) * 1e-3}


def _mpf(v):
    return mp.mpf(float(v))  # exact: every float32 / float64 is an mpf


def ulp32(v) -> float:
    return float(np.spacing(np.float32(abs(float(v)))))


# ------------------------------------------------------------------ reference ---
def lstsq(pts5x3, cols=(0, 1, 2)) -> dict:
    """min |A x + 1| over the columns `cols` of A (the others of x are zero).  x is None when those
    columns are dependent (smallest singular value below 1e-30 of the largest)."""
    with mp.workdps(DPS):
        P = np.asarray(pts5x3, np.float32).reshape(5, 3)
        cols = tuple(cols)
        A = mp.matrix([[_mpf(P[i, c]) for c in cols] for i in range(5)]) if cols else None
        x = [mp.mpf(0)] * 3
        sv = []
        solved = True
        if cols:
            sv = sorted((abs(s) for s in mp.svd_r(A, compute_uv=False)), reverse=True)
            solved = sv[-1] > sv[0] * mp.mpf(10) ** -30
            if solved:
                sol = mp.lu_solve(A.T * A, A.T * mp.matrix([-1] * 5))
                for k, c in enumerate(cols):
                    x[c] = sol[k]
        r = [sum(_mpf(P[i, c]) * x[c] for c in range(3)) + 1 for i in range(5)]
        nx = mp.sqrt(sum(v * v for v in x))
        out = {"x": np.array([float(v) for v in x]) if solved else None,
               "sv": np.array([float(s) for s in sv]),
               "r": np.array([float(v) for v in r]),
               "rnorm": float(mp.sqrt(sum(v * v for v in r))), "xnorm": float(nx)}
        if solved and nx > 0:
            out["normal"] = np.array([float(v / nx) for v in x])
            out["d"] = float(1 / nx)
            out["max_res"] = float(max(abs(v) for v in r) / nx)  # largest |n.p + d|
        return out


def error_bar(ref: dict) -> float:
    """FLT_EPSILON (kappa + kappa^2 rho) of a solved lstsq(): the first-order perturbation bound of a
    least-squares solution under relative perturbations of A of size FLT_EPSILON."""
    kappa = ref["sv"][0] / ref["sv"][-1]
    rho = ref["rnorm"] / (ref["sv"][0] * ref["xnorm"])
    return FLT_EPS * (kappa + kappa * kappa * rho)


def gates(pabcd, world, body, sqd4=None, pts=None) -> dict:
    """The gates from a float plane.  *_ulps: signed distance of the quantity to its threshold in
    units of the float ulp of the largest term the float evaluation rounds (the sum n.w + d is
    rounded at the size of its largest term, not of its result); positive = above the threshold."""
    with mp.workdps(DPS):
        pa = [_mpf(v) for v in np.asarray(pabcd, np.float32)]
        w = [_mpf(v) for v in np.asarray(world, np.float32)]
        b = [_mpf(v) for v in np.asarray(body, np.float32)]
        out = {}
        finite = all(mp.isfinite(v) for v in pa)
        out["finite"] = finite
        if sqd4 is not None:
            out["sqd"] = float(sqd4)
            out["sqd_ulps"] = (float(sqd4) - MAX_SQD) / ulp32(MAX_SQD)
            out["ok_sqd"] = not (float(sqd4) > MAX_SQD)
        if not finite:  # NaN > 0.9 is false, fabs(NaN) > thr is false: the fit passes, the point does not
            out.update(pd2=float("nan"), s=float("nan"), ok_fit=True, ok_s=False, ok_res=False,
                       fit_ulps=-np.inf, s_ulps=-np.inf, res_ulps=np.inf)
            return out
        terms = [pa[0] * w[0], pa[1] * w[1], pa[2] * w[2], pa[3]]
        pd2 = sum(terms)
        big = max([abs(t) for t in terms] + [abs(terms[0] + terms[1]), abs(pd2)])
        u_pd = ulp32(max(big, mp.mpf(MAX_RES) / 2))
        bn = mp.sqrt(sum(v * v for v in b))
        out["pd2"] = float(pd2)
        out["res_ulps"] = float((abs(pd2) - MAX_RES) / u_pd)
        out["ok_res"] = bool(abs(pd2) <= MAX_RES)
        if bn == 0:  # x / 0: -inf, or NaN for pd2 = 0; neither is > 0.9
            out.update(s=float("-inf"), ok_s=False, s_ulps=-np.inf)
        else:
            k = mp.mpf(0.9) / mp.sqrt(bn)  # (the double 0.9 of the reference's source)
            s = 1 - k * abs(pd2)
            out["s"] = float(s)
            out["s_ulps"] = float((s - mp.mpf(0.9)) / (ulp32(MIN_S) + k * u_pd))
            out["ok_s"] = bool(s > mp.mpf(0.9))
        if pts is not None:
            P = np.asarray(pts, np.float32).reshape(5, 3)
            worst, worst_u = mp.mpf(0), -np.inf
            for i in range(5):
                t = [pa[0] * _mpf(P[i, 0]), pa[1] * _mpf(P[i, 1]), pa[2] * _mpf(P[i, 2]), pa[3]]
                r = abs(sum(t))
                u = ulp32(max([abs(v) for v in t] + [abs(t[0] + t[1]), mp.mpf(PLANE_THR)]))
                worst = max(worst, r)
                worst_u = max(worst_u, float((r - mp.mpf(float(np.float32(PLANE_THR)))) / u))
            out["fit_res"] = float(worst)
            out["fit_ulps"] = worst_u
            out["ok_fit"] = worst_u <= 0
        return out


def decision(g: dict) -> bool:
    """point_selected_surf && res_last <= 2 of a gates() result (with sqd4 and pts given)."""
    return bool(g.get("ok_sqd", True) and g["ok_fit"] and g["ok_s"] and g["ok_res"])


def decided(g: dict) -> bool:
    """No gate quantity that the decision depends on is within DECIDED_ULPS of its threshold (the
    gates in the order of the pass; one that rejects clearly decides)."""
    stages = ([("sqd_ulps", "ok_sqd")] if "sqd_ulps" in g else []) + [("fit_ulps", "ok_fit"), ("s_ulps", "ok_s"),
                                                                     ("res_ulps", "ok_res")]
    for u, ok in stages:
        if abs(g[u]) <= DECIDED_ULPS:
            return False
        if not g[ok]:
            return True
    return True


# ------------------------------------------------------------------- clusters ---
def _frame(rng):
    """A random orthonormal frame: columns u, v (in plane), n (normal)."""
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def _patch(rng, centre, frame, noise, spread=0.2):
    uv = rng.uniform(-spread, spread, size=(5, 2))
    h = rng.normal(scale=noise, size=5)
    return centre + uv[:, :1] * frame[:, 0] + uv[:, 1:] * frame[:, 1] + h[:, None] * frame[:, 2]


def _dyadic(rng, lo, hi, bits=6, size=None):
    return rng.integers(int(lo * 2 ** bits), int(hi * 2 ** bits) + 1, size=size) / 2.0 ** bits


class _Sheet:
    def __init__(self, index):
        self.index = index
        self.centres, self.radii = [], []
        self.pts, self.queries, self.family, self.start = [], [], [], []

    def free(self, c, rad):
        lo, hi = ROOM_BOX
        if np.all(c + rad + SEP > lo) and np.all(c - rad - SEP < hi):
            return False
        if not self.centres:
            return True
        d = np.linalg.norm(np.asarray(self.centres) - c, axis=1) - np.asarray(self.radii) - rad
        return bool(np.all(d >= SEP))

    def add(self, family, pts, queries):
        pts = np.asarray(pts, np.float64).astype(np.float32)
        c = pts.astype(np.float64).mean(axis=0)
        rad = float(np.linalg.norm(pts - c, axis=1).max())
        queries = np.atleast_2d(np.asarray(queries, np.float64)).astype(np.float32)
        rad = max(rad, float(np.linalg.norm(queries - c, axis=1).max()))
        if not (family.startswith("tau_zero") or family.startswith("edge_")):
            assert max(np.linalg.norm(pts - p, axis=1).max() for p in pts) <= DIAM, family
        if not self.free(c, rad):
            return False
        self.centres.append(c)
        self.radii.append(rad)
        start = 5 * len(self.centres) - 5
        self.pts.append(pts)
        for q in queries:
            self.queries.append(q)
            self.family.append(family)
            self.start.append(start)
        return True

    def place(self, rng, family, make, r_lo, r_hi, tries=400):
        """make(centre) -> (pts, queries) at a free centre with r_lo <= |centre| <= r_hi."""
        for _ in range(tries):
            v = rng.normal(size=3)
            c = v / np.linalg.norm(v) * rng.uniform(r_lo, r_hi)
            pts, q = make(c)
            if self.add(family, pts, q):
                return
        raise AssertionError(f"sheet {self.index}: no room for a {family} cluster")

    def done(self, state=None):
        return {"index": self.index, "map": np.concatenate(self.pts).astype(np.float32),
                "query": np.asarray(self.queries, np.float32), "family": np.asarray(self.family),
                "start": np.asarray(self.start, np.int64), "state": state if state is not None else IDENTITY}


def _query(rng, pts, frame=None, height=0.02, spread=0.12):
    """A query near the cluster's centroid: in-plane offset, a small height along the normal."""
    c = np.asarray(pts, np.float64).mean(axis=0)
    if frame is None:
        frame = _frame(rng)
    o = rng.uniform(-spread, spread, size=2)
    return c + o[0] * frame[:, 0] + o[1] * frame[:, 1] + rng.uniform(-height, height) * frame[:, 2]


def _origin_zone(sh, rng, s):
    """The clusters bound to the origin region, one kind per sheet (they exclude one another)."""
    kind = s % 9
    if kind == 8:  # every coordinate near 4e-20: all squares are denormal and every tail is at most FLT_MIN,
        # so each step takes tau = 0 with a tail that is not small beside its head (Eigen drops it)
        sh.add("tau_zero_denorm", rng.uniform(-1.0, 1.0, size=(5, 3)) * 4e-20, rng.uniform(-0.3, 0.3, size=(4, 3)))
    elif kind == 0:  # rank 0: five points at the origin, NaN normal
        sh.add("coincident_origin", np.zeros((5, 3)), rng.uniform(-0.3, 0.3, size=(4, 3)))
    elif kind <= 4:  # tau = 0 at step 0: the pivot column's only non-zero is its first row
        ax = (kind - 1) % 3
        tiny = kind == 4  # ... or a tail whose squares underflow below FLT_MIN
        others = [a for a in range(3) if a != ax]
        pts = np.zeros((5, 3))
        pts[0, ax] = 2.0
        pts[1:, others[0]] = rng.uniform(-0.45, 0.45, size=4)
        pts[1:, others[1]] = rng.uniform(-0.45, 0.45, size=4)
        if tiny:
            pts[1:, ax] = rng.uniform(0.5, 3.0, size=4) * 1e-20 * rng.choice([-1, 1], size=4)
        q = np.zeros((4, 3))
        q[:, ax] = rng.uniform(1.5, 1.7, size=4)
        q[:, others] = rng.uniform(-0.05, 0.05, size=(4, 2))
        assert sh.add("tau_zero_tiny" if tiny else "tau_zero", pts, q)
    else:  # a plane 1 mm, 1 cm or 5 cm from the origin, the cluster 1-5 m away along it
        dist = (0.001, 0.01, 0.05)[kind - 5]
        fr = _frame(rng)
        c = rng.uniform(1.0, 5.0) * fr[:, 0] + dist * fr[:, 2]
        pts = _patch(rng, c, fr, 0.005)
        assert sh.add("near_origin_plane", pts, [_query(rng, pts, fr) for _ in range(4)])


def _free_families(sh, rng, s):
    def room(c):
        fr = _frame(rng)
        pts = _patch(rng, c, fr, 0.005)
        return pts, _query(rng, pts, fr)

    def rough(c):
        fr = _frame(rng)
        pts = _patch(rng, c, fr, 0.08)
        return pts, _query(rng, pts, fr)

    def collinear(jitter):
        def make(c):
            p0 = np.round(c * 64) / 64
            v = _dyadic(rng, -1, 1, bits=4, size=3)
            v[rng.integers(3)] = 1.0  # never the zero direction
            t = rng.choice(np.arange(-5, 6), size=5, replace=False) / 32.0
            pts = p0 + t[:, None] * v  # exact in float32: dyadic, below 2^24 in units of 2^-9
            assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
            if jitter:
                pts = pts + rng.normal(scale=jitter, size=(5, 3))
            return pts, pts.mean(axis=0) + rng.uniform(-0.1, 0.1, size=3)
        return make

    def coincident(split):
        def make(c):
            a = (c + rng.uniform(-0.1, 0.1, size=3)).astype(np.float32)
            b = (c + rng.uniform(-0.2, 0.2, size=3)).astype(np.float32)
            pts = np.array([a] * split + [b] * (5 - split))
            return pts, c + rng.uniform(-0.2, 0.2, size=3)
        return make

    def axis(kind):
        def make(c):
            fr = np.eye(3)[:, rng.permutation(3)]
            if kind == "zero_col":  # a cluster in a coordinate plane: one column of A is zero
                z = int(np.argmax(np.abs(fr[:, 2])))
                c = c.copy()
                c[z] = 0.0
                pts = _patch(rng, c, fr, 0.0)
                pts[:, z] = 0.0
            elif kind == "two_zero_cols":  # a cluster on a coordinate axis: two zero columns
                a = int(rng.integers(3))
                pts = np.zeros((5, 3))
                pts[:, a] = np.sign(c[a] + 1e-9) * np.linalg.norm(c) + rng.uniform(-0.25, 0.25, size=5)
            else:  # the exact axis-aligned plane (z = c after the permutation)
                z = int(np.argmax(np.abs(fr[:, 2])))
                pts = _patch(rng, c, fr, 0.0)
                pts[:, z] = np.float32(c[z])
            return pts, _query(rng, pts, fr)
        return make

    def norm_ties(kind):
        def make(c):
            a, b = int(rng.integers(3)), 0
            a, b = [(0, 1), (0, 2), (1, 2)][a]
            o = 3 - a - b
            m = np.linalg.norm(c)
            if kind == "identical":  # columns a and b are the same bit for bit; the other one is the largest
                pts = np.zeros((5, 3))
                pts[:, a] = pts[:, b] = np.float32(0.35 * m) + rng.uniform(-0.15, 0.15, size=5).astype(np.float32)
                pts[:, o] = 0.8 * m * np.sign(c[o] + 1e-9) + rng.uniform(-0.15, 0.15, size=5)
                return pts, pts.mean(axis=0) + rng.uniform(-0.05, 0.05, size=3)
            # mirror pairs under the swap of axes a and b, and one point on the mirror plane; the
            # tied columns are the largest, and the query sits beside the pairs so that the mirror
            # point is the fifth neighbour (the norms' Packet4f sums then commute)
            base = np.float32(0.65 * m)
            e = rng.uniform(-0.12, 0.12, size=(2, 2)).astype(np.float32)
            h = 0.3 * m * np.sign(c[o] + 1e-9)
            pts = np.zeros((5, 3), np.float32)
            for k in range(2):
                pts[2 * k, [a, b]] = base + e[k]
                pts[2 * k + 1, [a, b]] = (base + e[k])[::-1]
                pts[2 * k:2 * k + 2, o] = np.float32(h + rng.uniform(-0.1, 0.1))
            g = np.float32(base + 0.2)
            pts[4, [a, b]] = g
            pts[4, o] = np.float32(h)
            q = pts[:4].astype(np.float64).mean(axis=0) + rng.uniform(-0.01, 0.01, size=3)
            q[[a, b]] -= 0.05
            return pts, q
        return make

    def downdate(c):
        # columns a and b nearly parallel: both close to a multiple of the ones vector
        m = np.linalg.norm(c)
        c2 = np.array([m, m * rng.uniform(0.9, 1.0), rng.uniform(0.5, 1.5)]) / np.sqrt(2)
        c2 = c2[rng.permutation(3)] * rng.choice([-1, 1], size=3)
        fr = _frame(rng)
        pts = _patch(rng, c2, fr, 0.005)
        return pts, _query(rng, pts, fr)

    def far(r):
        return lambda c: room(c / np.linalg.norm(c) * r)

    # (counts: the fits that cannot be held against the reference, because their rank test falls on
    # rounding noise or their pivot columns depend to 1e-5, stay under 5 % of all cases: most fits
    # at 5000 m, a third of the exactly rank-deficient ones, every step of edge_res)
    for r, n in ((200.0, 6), (1000.0, 5), (5000.0, 1 - s % 2)):
        for _ in range(n):
            sh.place(rng, "far", far(r), r, r)
    for _ in range(9):
        sh.place(rng, "room", room, 13.5, 20.0, tries=3000)
    for _ in range(12):
        sh.place(rng, "rough", rough, 22.0, 60.0)
    for _ in range(2):
        sh.place(rng, "collinear", collinear(0.0), 22.0, 80.0)
    if s % 4 == 1:
        sh.place(rng, "collinear_jitter", collinear(1e-6), 22.0, 80.0)
    for split in (5, 3 + s % 2):
        sh.place(rng, "coincident", coincident(split), 22.0, 80.0)
    for kind in ("zero_col", "zero_col", "two_zero_cols", "plane", "plane"):
        sh.place(rng, "axis", axis(kind), 22.0, 80.0)
    for kind in ("mirror", "mirror", "identical", "identical"):
        sh.place(rng, "norm_ties", norm_ties(kind), 22.0, 80.0)
    for _ in range(5):
        sh.place(rng, "downdate", downdate, 25.0, 80.0)


# ------------------------------------------------------------------ sweeps ---
SWEEP_LEN = 65
THR_CENTRE = np.array([-14.0, 3.0, 9.0])  # the edge_thr cluster of every sheet


def _step(v: np.float32, n: int) -> np.float32:
    """v moved by n float32 steps (nextafter, n times)."""
    assert v > 0  # positive floats are ordered as their integers
    return np.array(int(np.array(v, np.float32).view(np.int32)) + n, np.int32).view(np.float32)[()]


def _bisect(lo: np.float32, hi: np.float32, pred) -> np.float32:
    """The first float (in nextafter order from lo to hi) at which pred is true; pred(lo) false, pred(hi) true."""
    assert not pred(lo) and pred(hi)
    to_i = lambda v: int(np.array(v, np.float32).view(np.int32))  # positive floats: ordered as ints
    a, b = to_i(lo), to_i(hi)
    while b - a > 1:
        m = (a + b) // 2
        if pred(np.array(m, np.int32).view(np.float32)[()]):
            b = m
        else:
            a = m
    return np.array(b, np.int32).view(np.float32)[()]


def _thr_cluster(lift: np.float32) -> np.ndarray:
    c = THR_CENTRE
    pts = np.array([[c[0] - 0.2, c[1] - 0.15, c[2]], [c[0] + 0.2, c[1] - 0.2, c[2]],
                    [c[0] + 0.15, c[1] + 0.2, c[2]], [c[0] - 0.2, c[1] + 0.2, c[2]],
                    [c[0] + 0.02, c[1] - 0.01, 0.0]], np.float32)
    pts[4, 2] = lift
    return pts


_THR_Z0 = None


def thr_lift(step: int) -> np.float32:
    """The lifted neighbour's z at step 0..64 of edge_thr: step 32 is the first lift at which the
    oracle's esti_plane fails the 0.1 test (located by bisection on the oracle)."""
    global _THR_Z0
    import oracle
    if _THR_Z0 is None:
        z = np.float32(THR_CENTRE[2])
        _THR_Z0 = _bisect(z + np.float32(0.05), z + np.float32(0.3),
                          lambda v: not oracle.esti_plane(_thr_cluster(v))[0])
    return _step(_THR_Z0, step - SWEEP_LEN // 2)


def _sweep_sheet():
    """edge_sqdis, edge_s and edge_res: one cluster each on an exact plane z = 1, 65 queries each,
    the middle one the first past the threshold in the reference (gates() of the oracle's plane)."""
    import oracle
    sh = _Sheet(N_SHEETS)
    out = {}
    # edge_sqdis: four neighbours near the query, the fifth sqrt(5) m away along x
    pts = np.array([[-20.1, 0.1, 1.0], [-19.9, 0.1, 1.0], [-20.0, -0.1, 1.0], [-20.05, 0.0, 1.0],
                    [-17.75, 0.0, 1.0]], np.float32)

    def sq(x):
        return float(np.float32(np.float32(pts[4, 0] - x) ** 2))  # dy = dz = 0: calc_dist is dx * dx
    x0 = _bisect(np.float32(19.9), np.float32(20.1), lambda v: sq(-v) > MAX_SQD)
    qs = np.array([[-_step(x0, k - 32), 0.0, 1.0] for k in range(SWEEP_LEN)], np.float32)
    assert sh.add("edge_sqdis", pts, qs)
    out["edge_sqdis"] = ("sqd_ulps", pts)
    # ... and one query whose fifth neighbour is at 1 + 4 + 0 = 5.0 exactly (kept: the gate is sqdis > 5)
    pts = np.array([[-20.125, 20.0, 1.0], [-19.875, 20.125, 1.0], [-20.0, 19.875, 1.0], [-20.0625, 20.0625, 1.0],
                    [-19.0, 22.0, 1.0]], np.float32)
    assert sh.add("edge_sqdis_exact", pts, [[-20.0, 20.0, 1.0]])
    # edge_s: body range 6 m, the height stepped through |pd2| = sqrt(|body|) / 9
    pts = np.array([[-0.2, -6.1, 1.0], [0.2, -6.2, 1.0], [0.15, -5.8, 1.0], [-0.2, -5.85, 1.0],
                    [0.0, -6.0, 1.0]], np.float32)
    pa = oracle.esti_plane(pts)[1]

    def ref(q, key):
        return gates(pa_cur[0], q, q)[key]
    pa_cur = [pa]
    q0 = np.array([0.01, -6.01, 0.0], np.float32)

    def with_z(z):
        q = q0.copy()
        q[2] = z
        return q
    z0 = _bisect(np.float32(1.05), np.float32(1.6), lambda v: not ref(with_z(v), "ok_s"))
    assert sh.add("edge_s", pts, np.array([with_z(_step(z0, k - 32)) for k in range(SWEEP_LEN)]))
    out["edge_s"] = ("s_ulps", pts)
    # edge_res: body range 400 m (s passes up to |pd2| = 2.2), the height stepped through |pd2| = 2
    pts = np.array([[-400.2, 0.1, 1.0], [-399.8, 0.2, 1.0], [-399.85, -0.2, 1.0], [-400.2, -0.15, 1.0],
                    [-400.0, 0.0, 1.0]], np.float32)
    pa_cur[0] = oracle.esti_plane(pts)[1]
    q0 = np.array([-400.01, 0.01, 0.0], np.float32)
    z0 = _bisect(np.float32(2.5), np.float32(3.5), lambda v: not ref(with_z(v), "ok_res"))
    assert sh.add("edge_res", pts, np.array([with_z(_step(z0, k - 32)) for k in range(SWEEP_LEN)]))
    out["edge_res"] = ("res_ulps", pts)
    return sh.done(), out


def _origin_body_sheet():
    """One body point exactly at the origin (sqrt(bn) = 0) whose world point lands inside a good
    cluster; a second body point beside it."""
    rng = np.random.default_rng(0xB0D7)
    sh = _Sheet(N_SHEETS + 1)
    c = np.array([3.0, -2.0, 1.5])
    fr = _frame(rng)
    pts = _patch(rng, c, fr, 0.005)
    st = dict(IDENTITY)
    ang = 0.3
    st["rot"] = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
    st["pos"] = pts.mean(axis=0) + 0.01 * fr[:, 2] + 0.03 * fr[:, 0]
    body = np.array([[0.0, 0.0, 0.0], [0.05, -0.04, 0.002]], np.float32)
    world = (body.astype(np.float64) @ st["rot"].T + st["pos"]).astype(np.float32)
    assert sh.add("origin_body", pts, world)
    out = sh.done(st)
    out["body"] = body
    return out


# ------------------------------------------------------------------- public ---
_CACHE = {}


def _check(sheet):
    """A query's five nearest map points are its cluster, in the order of its exact distances."""
    import oracle
    q = sheet["query"]
    idx, d = oracle.knn_brute(sheet["map"], q, 5)
    want = sheet["start"][:, None] + np.arange(5)
    assert np.array_equal(np.sort(idx, axis=1), want), sheet["index"]
    p = sheet["map"][want].astype(np.float64)
    exact = ((p - q[:, None, :].astype(np.float64)) ** 2).sum(axis=2)
    order = np.argsort(exact, axis=1, kind="stable")
    distinct = np.all(np.diff(np.sort(d, axis=1), axis=1) > 0, axis=1)  # float ties: PointType_CMP's order
    assert np.array_equal(idx[distinct], np.take_along_axis(want, order, axis=1)[distinct]), sheet["index"]
    sheet["nn_idx"], sheet["nn_d"] = idx, d
    sheet["body"] = sheet.get("body", q)
    return sheet


def sheets():
    """The N_SHEETS family sheets, then the sweep sheet, then the origin-body sheet."""
    if "sheets" not in _CACHE:
        out = []
        for s in range(N_SHEETS):
            rng = np.random.default_rng(0x91A7E000 + s)
            sh = _Sheet(s)
            _origin_zone(sh, rng, s)
            pts = _thr_cluster(thr_lift(s))
            assert sh.add("edge_thr", pts, pts[:4].astype(np.float64).mean(axis=0) + [0.01, 0.02, 0.004])
            _free_families(sh, rng, s)
            out.append(_check(sh.done()))
        sw, info = _sweep_sheet()
        out.append(_check(sw))
        assert sw["nn_d"][sw["family"] == "edge_sqdis_exact", 4] == MAX_SQD
        out.append(_check(_origin_body_sheet()))
        _CACHE["sheets"], _CACHE["sweep_info"] = out, info
    return _CACHE["sheets"]


def neighbourhoods(sheet) -> np.ndarray:
    """(n, 5, 3): each query's cluster in its neighbour order (the rows esti_plane sees)."""
    return sheet["map"][sheet["nn_idx"]]


def sweeps() -> dict:
    """name -> list of 65 (sheet index, query index) in step order."""
    sh = sheets()
    out = {}
    sw = sh[N_SHEETS]
    for name in ("edge_sqdis", "edge_s", "edge_res"):
        out[name] = [(N_SHEETS, int(i)) for i in np.flatnonzero(sw["family"] == name)]
    out["edge_thr"] = [(s, int(np.flatnonzero(sh[s]["family"] == "edge_thr")[0])) for s in range(SWEEP_LEN)]
    assert all(len(v) == SWEEP_LEN for v in out.values())
    return out


def room_crop(n_map: int = 200_000):
    """The synthetic room inside ROOM_CROP at the density of the n_map-point map, and 2,000 world
    points on the same surfaces (another sample of the room, a metre inside the crop), which are body
    points under the identity state with t_LI = 0."""
    if "room" not in _CACHE:
        from livo_amd import synth
        lo, hi = ROOM_CROP
        m = synth.make_map(n_map)
        m = np.ascontiguousarray(m[np.all((m[:, :2] >= lo) & (m[:, :2] <= hi), axis=1)])
        w = synth.make_map(n_map // 2, seed=synth.SEED_MAP + 61)
        w = w[np.all((w[:, :2] >= lo + 1.0) & (w[:, :2] <= hi - 1.0), axis=1)]
        w = np.ascontiguousarray(w[::max(len(w) // 2000, 1)][:2000], np.float32)
        assert len(w) == 2000 and 5_000 <= len(m) <= 20_000, (len(w), len(m))
        _CACHE["room"] = (m, w)
    return _CACHE["room"]
