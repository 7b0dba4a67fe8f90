"""The loop search's specification and fixtures (include/STD/STDesc.cpp of the reference).

  * a scalar restatement of AddSTDescs (:355-374), candidate_selector (:960-1099), candidate_verify
    (:1102-1192), triangle_solver (:1194-1219), plane_geometric_verify (:1221-1280) and SearchLoop
    (:299-353), written line by line, in IEEE doubles in the reference's order of operations;
  * an independent all-pairs cross-check of the selector, from the definitions of the cells;
  * a generator of places (sets of triangles), revisits under a known rigid transform, and the
    deliberate edge cases; every threshold comparison the restatement makes on a generated case is
    recorded with its relative margin, which `Case.expected()` asserts to be >= MARGIN.

Nothing here touches the device.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

DESC = np.dtype([("side_length", np.float64, (3,)), ("vertex_A", np.float64, (3,)), ("vertex_B", np.float64, (3,)),
                 ("vertex_C", np.float64, (3,)), ("center", np.float64, (3,)), ("vertex_attached", np.float64, (3,)),
                 ("frame_id", np.uint32), ("pad", np.uint32)])
PLANE = np.dtype([("xyz", np.float32, (3,)), ("normal", np.float32, (3,))])

DEFAULTS = dict(skip_near_num=50, candidate_num=50, rough_dis_threshold=0.01, vertex_diff_threshold=0.5,
                icp_threshold=0.5, normal_threshold=0.2, dis_threshold=0.5)  # read_parameters :83-93
MAX_FRAME_N = 20000
MARGIN = 1e-6     # least relative margin of a threshold comparison on a generated case
SV_GAP = 0.01     # least relative gap of a sampled covariance's two non-zero singular values

# Largest deviation of the float64 restatement (numpy's SVD) from a 60-digit mpmath evaluation of
# triangle_solver on every sampled pair of every case below (measure_solver_deviation, checked by
# tests/test_std_reference.py): rot 1.63e-13, t 1.22e-12 (the mismatched pairs of the edge
# cases, whose second singular value is small, set both; t also carries |center| ~ 1e2).  The device's
# Jacobi sweep is backward-stable like LAPACK's bidiagonalisation but rounds differently: it gets
# 8 x these.
ROT_DEV = 1.63e-13
T_DEV = 1.22e-12
ROT_TOL = 8 * ROT_DEV
T_TOL = 8 * T_DEV

_margins: list | None = None  # the recorder: (kind, relative margin)


def _lt(a: float, b: float, kind: str) -> bool:
    if _margins is not None:
        _margins.append((kind, abs(a - b) / max(abs(b), 1e-300)))
    return a < b


def _norm(v) -> float:
    return math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def _f3(a):
    return (float(a[0]), float(a[1]), float(a[2]))


def _mulv(R, v, t=None):
    out = [R[r][0] * v[0] + R[r][1] * v[1] + R[r][2] * v[2] for r in range(3)]
    if t is not None:
        out = [out[r] + t[r] for r in range(3)]
    return tuple(out)


class Db:
    """data_base_ and plane_cloud_vec_."""

    def __init__(self):
        self.cells: dict = {}   # STDesc_LOC -> descriptors in insertion order (indices into .descs)
        self.descs: list = []
        self.planes: list = []

    def add(self, descs: np.ndarray, planes: np.ndarray):  # AddSTDescs :355-374
        for d in descs:
            s = _f3(d["side_length"])
            pos = (int(s[0] + 0.5), int(s[1] + 0.5), int(s[2] + 0.5))
            self.cells.setdefault(pos, []).append(len(self.descs))
            self.descs.append(d)
        self.planes.append(planes)


def selector(db: Db, src: np.ndarray, prm: dict):
    """candidate_selector -> [(frame, [(i, db index), ...]), ...] in candidate order."""
    matches = []  # (i, db index) in the order of useful_match_index
    for i, s in enumerate(src):
        side, att = _f3(s["side_length"]), _f3(s["vertex_attached"])
        dis_threshold = _norm(side) * prm["rough_dis_threshold"]
        for x in (-1, 0, 1):
            for y in (-1, 0, 1):
                for z in (-1, 0, 1):
                    pos = (int(side[0] + x), int(side[1] + y), int(side[2] + z))  # (int): toward zero
                    centre = (pos[0] + 0.5, pos[1] + 0.5, pos[2] + 0.5)
                    if not _lt(_norm(_sub(side, centre)), 1.5, "centre"):
                        continue
                    for j in db.cells.get(pos, ()):
                        d = db.descs[j]
                        gap = (int(s["frame_id"]) - int(d["frame_id"])) & 0xFFFFFFFF  # unsigned int
                        if not gap > prm["skip_near_num"]:
                            continue
                        if not _lt(_norm(_sub(side, _f3(d["side_length"]))), dis_threshold, "side"):
                            continue
                        datt = _f3(d["vertex_attached"])
                        diff = 2.0 * _norm(_sub(att, datt)) / _norm(_add(att, datt))
                        if _lt(diff, prm["vertex_diff_threshold"], "attached"):
                            matches.append((i, j))
    match_array = [0] * MAX_FRAME_N
    for _, j in matches:
        match_array[int(db.descs[j]["frame_id"])] += 1
    out = []
    for _ in range(prm["candidate_num"]):  # :1066-1098
        max_vote, max_vote_index = 1, -1
        for f in range(len(db.planes)):  # (the entries beyond the stored frames are zero)
            if match_array[f] > max_vote:
                max_vote, max_vote_index = match_array[f], f
        if max_vote_index >= 0 and max_vote >= 5:
            match_array[max_vote_index] = 0
            out.append((max_vote_index, [m for m in matches if int(db.descs[m[1]]["frame_id"]) == max_vote_index]))
    return out


def selector_cross(db: Db, src: np.ndarray, prm: dict):
    """The same match lists from the definitions: every (source, stored) pair is tested, the stored
    descriptor's cell is derived from its own side lengths, and the pair is listed once per visit of
    that cell by the source.  -> {frame: [(i, db index), ...]} in (i, visit, insertion) order."""
    per_frame: dict = {}
    for i, s in enumerate(src):
        side = np.asarray(s["side_length"], np.float64)
        visits = []
        for inc in np.ndindex(3, 3, 3):
            cell = np.trunc(side + (np.asarray(inc) - 1.0)).astype(np.int64)
            if np.sqrt(((side - (cell + 0.5)) ** 2).sum()) < 1.5:
                visits.append(tuple(cell))
        thr = np.sqrt((side ** 2).sum()) * prm["rough_dis_threshold"]
        for v in visits:
            for j, d in enumerate(db.descs):
                dside = np.asarray(d["side_length"], np.float64)
                if tuple(np.trunc(dside + 0.5).astype(np.int64)) != v:
                    continue
                if not (int(s["frame_id"]) - int(d["frame_id"])) % 2 ** 32 > prm["skip_near_num"]:
                    continue
                a, b = np.asarray(s["vertex_attached"]), np.asarray(d["vertex_attached"])
                if np.linalg.norm(side - dside) < thr and \
                        2.0 * np.linalg.norm(a - b) / np.linalg.norm(a + b) < prm["vertex_diff_threshold"]:
                    per_frame.setdefault(int(d["frame_id"]), []).append((i, j))
    return per_frame


def triangle_solver(s, d):
    """-> rot (3x3 nested tuples), t, and the covariance's singular values."""
    src = np.stack([s["vertex_A"] - s["center"], s["vertex_B"] - s["center"], s["vertex_C"] - s["center"]], axis=1)
    ref = np.stack([d["vertex_A"] - d["center"], d["vertex_B"] - d["center"], d["vertex_C"] - d["center"]], axis=1)
    U, S, Vt = np.linalg.svd(src @ ref.T)
    V = Vt.T
    rot = V @ U.T
    if np.linalg.det(rot) < 0:
        rot = V @ np.diag([1.0, 1.0, -1.0]) @ U.T
    t = -rot @ s["center"] + d["center"]
    if _margins is not None:
        _margins.append(("sv_gap", (S[0] - S[1]) / S[0] / SV_GAP * MARGIN))  # (scaled: >= MARGIN means >= SV_GAP)
    return tuple(map(tuple, rot.tolist())), tuple(t.tolist()), S


def _agrees(R, t, s, d) -> bool:
    ok = True
    for k in ("vertex_A", "vertex_B", "vertex_C"):
        # (all three distances are computed before the test, :1139-1143)
        ok = _lt(_norm(_sub(_mulv(R, _f3(s[k]), t), _f3(d[k]))), 3.0, "vote") and ok
    return ok


def plane_geometric_verify(source: np.ndarray, target: np.ndarray, R, t, prm: dict) -> float:
    useful = 0
    txyz = target["xyz"].astype(np.float32)
    for p in source:
        pi = _mulv(R, _f3(p["xyz"]), t)
        ni = _mulv(R, _f3(p["normal"]))
        q = np.array(pi, np.float64).astype(np.float32)
        dx, dy, dz = (q[0] - txyz[:, 0]), (q[1] - txyz[:, 1]), (q[2] - txyz[:, 2])
        d2 = (dx * dx + dy * dy) + dz * dz  # float32, L2_Simple's order
        order = np.argsort(d2, kind="stable")
        if _margins is not None:
            for a in range(min(3, len(order) - 1)):  # the three nearest are ordered, the 4th lies apart
                lo, hi = float(d2[order[a]]), float(d2[order[a + 1]])
                _margins.append(("neighbour", (hi - lo) / max(hi, 1e-300)))
        for j in order[:3]:  # only the neighbours that exist (the reference reads stale indices)
            tp = target[j]
            tpi, tni = _f3(tp["xyz"]), _f3(tp["normal"])
            inc, add = _norm(_sub(ni, tni)), _norm(_add(ni, tni))
            dd = _sub(pi, tpi)
            ptp = abs(tni[0] * dd[0] + tni[1] * dd[1] + tni[2] * dd[2])
            a = _lt(inc, prm["normal_threshold"], "normal")
            b = a or _lt(add, prm["normal_threshold"], "normal")
            if b and _lt(ptp, prm["dis_threshold"], "plane"):
                useful += 1
                break
    return useful / len(source) if len(source) else float("nan")


def candidate_verify(db: Db, src, src_planes, frame: int, mlist: list, prm: dict) -> dict:
    skip_len = len(mlist) // 50 + 1
    use_size = len(mlist) // skip_len
    solved, vote_list = [], []
    for i in range(use_size):
        si, dj = mlist[i * skip_len]
        R, t, S = triangle_solver(src[si], db.descs[dj])
        solved.append((R, t))
        vote_list.append(sum(1 for a, b in mlist if _agrees(R, t, src[a], db.descs[b])))
    max_vote_index, max_vote = 0, 0
    for i, v in enumerate(vote_list):
        if max_vote < v:
            max_vote_index, max_vote = i, v
    out = dict(frame=frame, votes=len(mlist), use_size=use_size, max_vote=max_vote, max_vote_index=max_vote_index,
               score=-1.0, rot=np.eye(3), t=np.zeros(3), success=[], matches=mlist,
               samples=[mlist[i * skip_len] for i in range(use_size)])
    if max_vote >= 4:
        R, t = solved[max_vote_index]
        out["success"] = [(a, b) for a, b in mlist if _agrees(R, t, src[a], db.descs[b])]
        out["score"] = plane_geometric_verify(src_planes, db.planes[frame], R, t, prm)
        out["rot"], out["t"] = np.array(R), np.array(t)
    return out


def search_loop(db: Db, src, src_planes, prm: dict) -> dict:
    res = dict(frame=-1, score=0.0, rot=np.eye(3), t=np.zeros(3), pairs=[], candidates=[])
    if len(src) == 0:
        return res
    best_score, best = 0.0, None
    for frame, mlist in selector(db, src, prm):
        c = candidate_verify(db, src, src_planes, frame, mlist, prm)
        res["candidates"].append(c)
        if c["score"] > best_score:
            best_score, best = c["score"], c
    if best_score > prm["icp_threshold"]:
        res.update(frame=best["frame"], score=best_score, rot=best["rot"], t=best["t"], pairs=best["success"])
    return res


# ---------------------------------------------------------------------------------------------
# Generator
# ---------------------------------------------------------------------------------------------
def _label(p0, p1, p2):
    """build_stdesc's vertex order: |AB| <= |AC| <= |BC|."""
    pts = [np.asarray(p0), np.asarray(p1), np.asarray(p2)]
    best = None
    for a in range(3):
        for b in range(3):
            if b == a:
                continue
            c = 3 - a - b
            ab, ac, bc = (np.linalg.norm(pts[a] - pts[b]), np.linalg.norm(pts[a] - pts[c]),
                          np.linalg.norm(pts[b] - pts[c]))
            if ab <= ac <= bc:
                best = (pts[a], pts[b], pts[c], (ab, ac, bc))
    return best


def make_desc(A, B, C, attached, frame: int, side=None) -> np.ndarray:
    d = np.zeros((), DESC)
    d["vertex_A"], d["vertex_B"], d["vertex_C"] = A, B, C
    d["center"] = (np.asarray(A) + np.asarray(B) + np.asarray(C)) / 3.0
    sides = (np.linalg.norm(A - B), np.linalg.norm(A - C), np.linalg.norm(B - C))
    d["side_length"] = 5.0 * np.asarray(sides) if side is None else side  # 1 / std_side_resolution (0.2)
    d["vertex_attached"] = attached
    d["frame_id"] = frame
    return d


def make_place(rng, n_tri: int = 40, n_planes: int = 30):
    """Triangles with sides in 2-30 m that differ by 0.5 m or more (the order survives the noise)."""
    tris = []
    while len(tris) < n_tri:
        p0 = rng.uniform(-40.0, 40.0, 3)
        p1 = p0 + rng.uniform(-15.0, 15.0, 3)
        p2 = p0 + rng.uniform(-15.0, 15.0, 3)
        A, B, C, s = _label(p0, p1, p2)
        if s[0] >= 2.0 and s[2] <= 30.0 and s[1] - s[0] >= 0.5 and s[2] - s[1] >= 0.5:
            tris.append((A, B, C, rng.integers(8, 40, 3).astype(np.float64)))
    planes = np.zeros(n_planes, PLANE)
    planes["xyz"] = rng.uniform(-40.0, 40.0, (n_planes, 3))
    nrm = rng.normal(size=(n_planes, 3))
    planes["normal"] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    return tris, planes


def place_descs(tris, frame: int) -> np.ndarray:
    return np.array([make_desc(A, B, C, att, frame) for A, B, C, att in tris], DESC)


def random_rigid(rng):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(0.3, 2.5)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)
    return R, rng.uniform(-20.0, 20.0, 3)


def revisit(rng, tris, planes, R, t, frame: int, noise: float = 0.01):
    """The place seen again from a frame in which p_place = R p + t, about 1 cm of vertex noise."""
    out = []
    for A, B, C, att in tris:
        v = [R.T @ (p - t) + rng.uniform(-noise, noise, 3) for p in (A, B, C)]
        a2, b2, c2, _ = _label(*v)
        assert np.allclose(a2, v[0]) and np.allclose(b2, v[1])  # the vertex order survived the noise
        out.append((v[0], v[1], v[2], att + rng.integers(-1, 2, 3)))
    pl = np.zeros(len(planes), PLANE)
    pl["xyz"] = (planes["xyz"].astype(np.float64) - t) @ R + rng.uniform(-noise, noise, (len(planes), 3))
    nrm = planes["normal"].astype(np.float64) @ R + rng.normal(scale=0.01, size=(len(planes), 3))
    pl["normal"] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    return out, pl


@dataclass
class Case:
    name: str
    frames: list            # [(descs, planes)] committed in order
    query: np.ndarray
    query_planes: np.ndarray
    prm: dict
    generated: bool = True  # False: a deliberate edge case of exactly representable numbers, margins exempt
    truth: tuple | None = None
    _exp: dict | None = field(default=None, repr=False)
    margins: list = field(default_factory=list, repr=False)

    def db(self) -> Db:
        db = Db()
        for d, p in self.frames:
            db.add(d, p)
        return db

    def expected(self) -> dict:
        """The restatement's result, computed once; a generated case's margins are asserted here."""
        global _margins
        if self._exp is None:
            _margins = []
            try:
                self._exp = search_loop(self.db(), self.query, self.query_planes, self.prm)
            finally:
                self.margins, _margins = _margins, None
            worst = min(self.margins, key=lambda m: m[1], default=("none", 1.0))
            # the singular-value gap bounds the solver's conditioning everywhere, edge cases included
            sv = min((m[1] for m in self.margins if m[0] == "sv_gap"), default=1.0)
            assert sv >= MARGIN, (self.name, "singular-value gap", sv / MARGIN * SV_GAP)
            if self.generated:
                assert worst[1] >= MARGIN, (self.name, worst)
        return self._exp


def _prm(**kw):
    return {**DEFAULTS, "skip_near_num": 5, "candidate_num": 3, **kw}


N_FRAMES, N_TRI = 64, 40
_cache: dict = {}


def _world(seed: int = 20240611):
    """64 places of 40 triangles, and place 10 seen again under a known transform."""
    if "world" not in _cache:
        rng = np.random.default_rng(seed)
        places = [make_place(rng, N_TRI) for _ in range(N_FRAMES)]
        R, t = random_rigid(rng)
        q_tris, q_planes = revisit(rng, places[10][0], places[10][1], R, t, N_FRAMES)
        other = make_place(rng, N_TRI)
        _cache["world"] = dict(places=places, R=R, t=t, q_tris=q_tris, q_planes=q_planes, other=other, rng=rng)
    return _cache["world"]


def _frames(w):
    return [(place_descs(tr, f), pl) for f, (tr, pl) in enumerate(w["places"])]


def _tri_desc(tri, frame, side, att=(20.0, 20.0, 20.0)):
    return make_desc(tri[0], tri[1], tri[2], np.asarray(att, np.float64), frame, np.asarray(side, np.float64))


def _edge(name, groups, queries, q_frame, prm, q_planes=None, tgt_planes=None, n_frames=None):
    """A hand-made case on place 10's geometry: groups = {frame: [(triangle, side)]} stored,
    queries = [(triangle, side)] of the revisit.  The selector reads the sides, the attached counts
    and the frames, all exactly representable; the verification reads the vertices."""
    w = _world()
    tris, planes = w["places"][10]
    n_frames = n_frames if n_frames is not None else max(groups) + 1
    frames = []
    for f in range(n_frames):
        ds = [_tri_desc(tris[k], f, side) for k, side in groups.get(f, [])]
        pl = planes if tgt_planes is None else tgt_planes
        frames.append((np.array(ds, DESC) if ds else np.zeros(0, DESC), pl))
    q = [_tri_desc(w["q_tris"][k], q_frame, side) for k, side in queries]
    return Case(name, frames, np.array(q, DESC) if q else np.zeros(0, DESC),
                w["q_planes"] if q_planes is None else q_planes, prm, generated=False, truth=(w["R"], w["t"]))


SA, SB = (40.25, 60.25, 80.25), (50.25, 70.25, 90.25)


def _own_cells(ks, base=100.25):
    """(triangle k, a side of its own cell): query k then matches stored k only."""
    return [(k, (base + 4.0 * n, base + 40.0 + 4.0 * n, base + 80.0 + 4.0 * n)) for n, k in enumerate(ks)]


def cases() -> dict:
    if "cases" in _cache:
        return _cache["cases"]
    w = _world()
    tris, planes = w["places"][10]
    qp = w["q_planes"]
    C = {}

    def add(c):
        C[c.name] = c

    add(Case("revisit", _frames(w), place_descs(w["q_tris"], N_FRAMES), qp, _prm(), truth=(w["R"], w["t"])))
    add(Case("no_revisit", _frames(w), place_descs(w["other"][0], N_FRAMES), w["other"][1], _prm()))
    # cells of 65 and 130 entries (across the wave width): frames 0-12 hold 5 each of cell A and get 10
    # votes from two sources, frames 13-38 hold 5 each of cell B and get 5: ties, and more than 3 candidates
    g = {f: [(k, SA) for k in range(5)] for f in range(13)}
    g.update({f: [(k, SB) for k in range(5)] for f in range(13, 39)})
    add(_edge("runs_65_130", g, [(0, SA), (1, SA), (2, SB)], 60, _prm()))
    # match lists of 49, 50, 51, 99 and 100 pairs: the skip_len edges
    g = {f: [(j % 7, SA) for j in range(n)] for f, n in enumerate((49, 50, 51, 99, 100))}
    add(_edge("skip_len", g, [(0, SA)], 60, _prm(candidate_num=5)))
    add(_edge("votes_4_5", {0: [(k, SA) for k in range(4)], 1: [(k, SA) for k in range(5)]}, [(0, SA)], 60, _prm()))
    # frame gap: 5 is refused, 6 accepted (skip_near_num 5); a stored id above the source's wraps and passes
    g = {f: [(k, SA) for k in range(5)] for f in (14, 15)}
    add(_edge("gap_5_6", g, [(0, SA)], 20, _prm()))
    add(_edge("gap_wraps", {10: [(k, SA) for k in range(5)]}, [(0, SA)], 3, _prm()))
    # .49 commits to cell 40 and .51 to 41; the search truncates and visits both
    g = {0: [(k, (40.49, 60.25, 80.25)) for k in range(5)], 1: [(k, (40.51, 60.25, 80.25)) for k in range(5)]}
    add(_edge("frac_49_51", g, [(0, (40.49, 60.25, 80.25))], 60, _prm()))
    # (int)(0.25 - 1) == (int)(0.25) == 0: cell 0 is visited twice and its 3 entries give 6 votes (floor: 3)
    add(_edge("trunc_twice", {0: [(k, (0.25, 60.25, 80.25)) for k in range(3)]}, [(0, (0.25, 60.25, 80.25))], 60,
              _prm(rough_dis_threshold=0.02)))
    # side 31.0, increment +1: centre 32.5 at distance exactly 1.5, skipped; 31.0078125 visits it
    g = {0: [(k, (31.625, 60.25, 80.25)) for k in range(5)]}
    add(_edge("centre_exact", g, [(0, (31.0, 60.5, 80.5))], 60, _prm()))
    add(_edge("centre_inside", g, [(0, (31.0078125, 60.5, 80.5))], 60, _prm()))
    # five pairs in cells of their own: 3 (4) of the same triangle, the others mismatched
    own = _own_cells(range(5))
    add(_edge("max_vote_3", {0: [(k if n < 3 else k + 20, s) for n, (k, s) in enumerate(own)]}, own, 60, _prm()))
    add(_edge("max_vote_4", {0: [(k if n < 4 else k + 20, s) for n, (k, s) in enumerate(own)]}, own, 60, _prm()))
    good = {0: own}
    flipped = qp.copy()
    flipped["normal"] = -flipped["normal"]
    add(_edge("normal_flipped", good, own, 60, _prm(), q_planes=flipped))
    # 4 source planes of which 2 (3) find their target: the others carry a normal turned a quarter
    for n_ok in (2, 3):
        four = qp[:4].copy()
        for k in range(n_ok, 4):
            nx, ny, nz = (float(v) for v in four["normal"][k])
            perp = np.cross([nx, ny, nz], [1.0, 0.0, 0.0] if abs(nx) < 0.9 else [0.0, 1.0, 0.0])
            four["normal"][k] = perp / np.linalg.norm(perp)
        add(_edge(f"score_{n_ok}_of_4", good, own, 60, _prm(), q_planes=four))
    add(_edge("target_2_planes", good, own, 60, _prm(), tgt_planes=planes[:2].copy()))
    add(_edge("empty_source_cloud", good, own, 60, _prm(), q_planes=np.zeros(0, PLANE)))
    add(_edge("empty_descs", good, [], 60, _prm()))
    _cache["cases"] = C
    return C


def measure_solver_deviation():
    """Largest |rot| and |t| deviation of triangle_solver (float64, numpy) from the same formula at 60
    digits (mpmath), over every sampled pair of every case."""
    import mpmath as mp

    mp.mp.dps = 60
    dev_r = dev_t = 0.0
    for c in cases().values():
        db = c.db()
        for cand in c.expected()["candidates"]:
            for si, dj in cand["samples"]:
                s, d = c.query[si], db.descs[dj]
                R, t, _ = triangle_solver(s, d)
                M = lambda v: mp.matrix([mp.mpf(float(x)) for x in v])  # noqa: E731
                sc, rc = M(s["center"]), M(d["center"])
                src = mp.matrix(3, 3)
                ref = mp.matrix(3, 3)
                for col, k in enumerate(("vertex_A", "vertex_B", "vertex_C")):
                    a, b = M(s[k]) - sc, M(d[k]) - rc
                    for r in range(3):
                        src[r, col], ref[r, col] = a[r], b[r]
                U, S, Vh = mp.svd_r(src * ref.T)
                V = Vh.T
                rot = V * U.T
                if mp.det(rot) < 0:
                    rot = V * mp.diag([1, 1, -1]) * U.T
                tt = -(rot * sc) + rc
                dev_r = max(dev_r, max(abs(float(rot[r, q] - mp.mpf(R[r][q]))) for r in range(3) for q in range(3)))
                dev_t = max(dev_t, max(abs(float(tt[r] - mp.mpf(t[r]))) for r in range(3)))
    return dev_r, dev_t
