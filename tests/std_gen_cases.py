"""GenerateSTDescs' specification and fixtures (include/STD/STDesc.cpp of the reference).

  * a scalar restatement of init_voxel_map (:376-422), init_plane (:1367-1409), getPlane (:492-507),
    build_connection (:424-490), corner_extractor (:509-617), extract_corner (:619-781),
    non_maxi_suppression (:783-822) and build_stdesc (:824-958), written line by line, IEEE doubles
    and floats where the reference uses them, sums in the reference's order;
  * the four places where the reference is implementation-defined, pinned as DESIGN.md 8.17 pins
    them: the visiting order is an argument of every function that walks the voxel map (default:
    first appearance), the normal's sign, the ties at the maximum_corner_num cut, the neighbours
    build_stdesc finds (ordered by (distance, index), only those that exist);
  * the eigen-solve is the cyclic Jacobi iteration the device runs (Eigen::EigenSolver cannot be
    restated line by line; both give the symmetric matrix's eigenpairs);
  * the per-voxel greedy formulation of corner_extractor's membership next to the sequential walk;
  * generators of the edge cases and of a small room sampled twice; every threshold comparison on
    a generated case is recorded with its relative margin, which `Case.expected()` asserts.

Nothing here touches the device.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

import std_cases as S

CORNER = np.dtype([("xyz", np.float32, (3,)), ("attached", np.float32), ("normal", np.float32, (3,)),
                   ("pad", np.float32)])
DEFAULTS = dict(voxel_size=2.0, voxel_init_num=10, plane_detection_thre=0.01, plane_merge_normal_thre=0.1,
                proj_image_resolution=0.5, proj_dis_min=0.0, proj_dis_max=2.0, corner_thre=10.0, maximum_corner_num=100,
                non_max_suppression_radius=2.0, descriptor_near_num=10, descriptor_min_len=2.0, descriptor_max_len=50.0,
                std_side_resolution=0.2)  # read_parameters :57-81
MARGIN = 1e-6       # least relative margin of a threshold comparison on a generated case
CELL_MARGIN = 1e-6  # least distance of a projected point from a cell edge, in cells
SWEEPS = 10         # kStdGenSweeps

# Largest deviation of this float64 restatement from its own evaluation in 60-digit arithmetic over every
# voxel, job and triangle of the cases below (measure_deviation, checked by tests/test_std_gen_reference.py).
# The device runs the same operations in the same order and gets 8 x these.
DEV = dict(center=5.4e-14, normal=6.7e-14, corner=3.8e-14, side=3.4e-14, vertex=3.8e-14)
TOL = {k: 8 * v for k, v in DEV.items()}

_margins: list | None = None  # the recorder: (kind, relative margin)


def _rec(kind, a, b):
    if _margins is not None:
        _margins.append((kind, abs(a - b) / max(abs(a), abs(b), 1e-300)))


def _lt(a, b, kind):
    _rec(kind, a, b)
    return a < b


def _gt(a, b, kind):
    _rec(kind, a, b)
    return a > b


def f32(x) -> float:
    return float(np.float32(x))


class Num:
    """The arithmetic a function runs in: IEEE doubles here, 60-digit mpmath in measure_deviation."""
    sqrt = staticmethod(math.sqrt)
    f = staticmethod(float)           # a constant or an input
    f32 = staticmethod(f32)           # the reference's casts to float (the identity in exact arithmetic)


def norm3(v, N=Num):
    return N.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def same_normal(a, b, thre, kind=None):
    d = norm3((a[0] - b[0], a[1] - b[1], a[2] - b[2]))
    s = norm3((a[0] + b[0], a[1] + b[1], a[2] + b[2]))
    if kind:
        return _lt(d, thre, kind) | _lt(s, thre, kind)
    return d < thre or s < thre


# ---------------------------------------------------------------------------------------------
# init_voxel_map, init_plane
# ---------------------------------------------------------------------------------------------
def voxel_key(p, voxel_size: float):
    out = []
    for j in range(3):
        loc = float(p[j]) / voxel_size
        if loc < 0:
            loc -= 1.0
        out.append(int(loc))  # (int64_t): truncation
    return tuple(out)


@dataclass
class Voxel:
    key: tuple
    idx: list = field(default_factory=list)  # input indices of its points, in input order
    is_plane: bool = False
    center: tuple = (0.0, 0.0, 0.0)
    normal: tuple = (0.0, 0.0, 0.0)
    min_eig: float = math.nan
    connect: list = field(default_factory=lambda: [False] * 6)
    checked: list = field(default_factory=lambda: [False] * 6)
    tree: list = field(default_factory=lambda: [None] * 6)
    is_project: bool = False
    proj_normals: list = field(default_factory=list)


def jacobi(a, N=Num):
    """The eigenpairs of the symmetric 3 x 3 `a`: SWEEPS cyclic sweeps -> (diagonal, eigenvector columns)."""
    a = [list(r) for r in a]
    one = N.f(1.0)
    v = [[one if r == c else N.f(0.0) for c in range(3)] for r in range(3)]
    for _ in range(SWEEPS):
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = a[p][q]
            if apq == 0:
                continue
            theta = (a[q][q] - a[p][p]) / (2 * apq)
            t = one / (abs(theta) + N.sqrt(theta * theta + one))
            if theta < 0:
                t = -t
            c = one / N.sqrt(t * t + one)
            s = t * c
            a[p][p] = a[p][p] - t * apq
            a[q][q] = a[q][q] + t * apq
            a[p][q] = a[q][p] = N.f(0.0)
            arp, arq = a[r][p], a[r][q]
            a[r][p] = a[p][r] = c * arp - s * arq
            a[r][q] = a[q][r] = s * arp + c * arq
            for k in range(3):
                vp, vq = v[k][p], v[k][q]
                v[k][p] = c * vp - s * vq
                v[k][q] = s * vp + c * vq
    return [a[0][0], a[1][1], a[2][2]], v


def pin_sign(n):
    """Pin 2: the component of largest magnitude positive, the first of equal ones."""
    big = n[0]
    if abs(n[1]) > abs(big):
        big = n[1]
    if abs(n[2]) > abs(big):
        big = n[2]
    return tuple(-x for x in n) if big < 0 else tuple(n)


def plane_fit(points, N=Num):
    """init_plane's centre, least eigenvalue and pinned normal of a point list."""
    cov = [[N.f(0.0)] * 3 for _ in range(3)]
    cen = [N.f(0.0)] * 3
    for p in points:
        p = [N.f(float(x)) for x in p]
        for r in range(3):
            for c in range(3):
                cov[r][c] = cov[r][c] + p[r] * p[c]
            cen[r] = cen[r] + p[r]
    cnt = N.f(float(len(points)))
    cen = [x / cnt for x in cen]
    cov = [[cov[r][c] / cnt - cen[r] * cen[c] for c in range(3)] for r in range(3)]
    ev, vec = jacobi(cov, N)
    m = 0
    if ev[1] < ev[m]:
        m = 1
    if ev[2] < ev[m]:
        m = 2
    return tuple(cen), ev[m], pin_sign((vec[0][m], vec[1][m], vec[2][m])), sorted(ev)


def init_voxel_map(pts: np.ndarray, prm: dict) -> dict:
    """-> {key: Voxel} in order of first appearance (a dict keeps insertion order: pin 1's default)."""
    vox: dict = {}
    for i in range(len(pts)):
        k = voxel_key(pts[i], prm["voxel_size"])
        if k not in vox:
            vox[k] = Voxel(k)
        vox[k].idx.append(i)
    for v in vox.values():
        if len(v.idx) > prm["voxel_init_num"]:
            cen, ev, nrm, evs = plane_fit([pts[i] for i in v.idx])
            v.min_eig = ev
            if _lt(ev, prm["plane_detection_thre"], "eigenvalue"):
                v.is_plane, v.center, v.normal = True, cen, nrm
                mags = sorted(abs(x) for x in nrm)
                _rec("normal sign", mags[2], mags[1])
    return vox


def get_plane(vox: dict, order) -> np.ndarray:
    out = [(vox[k].center, vox[k].normal) for k in order if vox[k].is_plane]
    pl = np.zeros(len(out), S.PLANE)
    for i, (c, n) in enumerate(out):
        pl["xyz"][i], pl["normal"][i] = c, n
    return pl


# ---------------------------------------------------------------------------------------------
# build_connection
# ---------------------------------------------------------------------------------------------
DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1))


def _nb(k, d):
    return (k[0] + d[0], k[1] + d[1], k[2] + d[2])


def build_connection(vox: dict, order, prm: dict):
    for k in order:
        cur = vox[k]
        if not cur.is_plane:
            continue
        for i in range(6):
            near = vox.get(_nb(k, DIRS[i]))
            if near is None:
                cur.checked[i] = True
                cur.connect[i] = False
            elif not cur.checked[i]:
                cur.checked[i] = True
                j = i - 3 if i >= 3 else i + 3
                near.checked[j] = True
                if near.is_plane:
                    if same_normal(cur.normal, near.normal, prm["plane_merge_normal_thre"], "merge"):
                        cur.connect[i] = near.connect[j] = True
                        cur.tree[i], near.tree[j] = near, cur
                    else:
                        cur.connect[i] = near.connect[j] = False
                else:
                    cur.connect[i] = False
                    near.connect[j] = True
                    near.tree[j] = cur


def connection_state(vox: dict):
    return {k: (tuple(v.connect), tuple(v.checked), tuple(t.key if t is not None else None for t in v.tree))
            for k, v in vox.items()}


# ---------------------------------------------------------------------------------------------
# corner_extractor
# ---------------------------------------------------------------------------------------------
ROUND = tuple((x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1))


def job_list(vox: dict, order):
    """The static set of jobs (V, i) in visiting order, then i (:527-552)."""
    jobs = []
    for k in order:
        cur = vox[k]
        if cur.is_plane:
            continue
        for i in range(6):
            if not cur.connect[i]:
                continue
            c = cur.tree[i]
            if not any(c.checked[j] and c.connect[j] for j in range(6)):
                continue
            if len(cur.idx) > 10:
                jobs.append((k, i, c.key))
    return jobs


def members_sequential(vox: dict, order):
    """corner_extractor's walk as written: -> per job the 27 slots' voxel keys (None: no member)."""
    for v in vox.values():
        v.is_project, v.proj_normals = False, []
    out = []
    for k, i, ck in job_list(vox, order):
        normal = vox[ck].normal
        slots = []
        for inc in ROUND:
            w = vox.get(_nb(k, inc))
            take = None
            if w is not None and not w.is_plane:
                skip = False
                if w.is_project:
                    for n in w.proj_normals:
                        if same_normal(normal, n, 0.5, "repeated projection"):
                            skip = True
                if not skip:
                    take = w.key
                    w.is_project = True
                    w.proj_normals.append(normal)
            slots.append(take)
        out.append(slots)
    return out


def members_greedy(vox: dict, order):
    """The same membership, one independent greedy walk per voxel W over its candidate jobs in job order."""
    jobs = job_list(vox, order)
    by_voxel: dict = {}
    for j, (k, _, _) in enumerate(jobs):
        by_voxel.setdefault(k, []).append(j)
    out = [[None] * 27 for _ in jobs]
    for wk, w in vox.items():
        if w.is_plane:
            continue
        cand = []
        for slot, inc in enumerate(ROUND):
            for j in by_voxel.get((wk[0] - inc[0], wk[1] - inc[1], wk[2] - inc[2]), ()):
                cand.append((j, slot))
        taken = []
        for j, slot in sorted(cand):
            normal = vox[jobs[j][2]].normal
            if any(same_normal(normal, n, 0.5) for n in taken):
                continue
            taken.append(normal)
            out[j][slot] = wk
    return out


def plane_frame(normal, center, N=Num):
    A, B, C = normal
    D = -((A * center[0] + B * center[1]) + C * center[2])
    x = [N.f(1.0), N.f(1.0), N.f(0.0)]
    if C != 0:
        x[2] = -(A + B) / C
        branch = 0
    elif B != 0:
        x[1] = -A / B
        branch = 1
    else:
        x[0], x[1] = N.f(0.0), N.f(1.0)
        branch = 2
    xn = norm3(x, N)
    if xn > 0:
        x = [c / xn for c in x]
    y = [B * x[2] - C * x[1], C * x[0] - A * x[2], A * x[1] - B * x[0]]
    yn = norm3(y, N)
    if yn > 0:
        y = [c / yn for c in y]
    dx = -((x[0] * center[0] + x[1] * center[1]) + x[2] * center[2])
    dy = -((y[0] * center[0] + y[1] * center[1]) + y[2] * center[2])
    return dict(A=A, B=B, C=C, D=D, x=x, y=y, dx=dx, dy=dy, center=center, branch=branch)


def project(f, p, N=Num):
    """-> (distance to the plane, project_x, project_y) of :656-676."""
    x, y, z = (N.f(float(c)) for c in p)
    A, B, C, D = f["A"], f["B"], f["C"], f["D"]
    dis = abs(((x * A + y * B) + z * C) + D)
    q = (A * A + B * B) + C * C
    c0 = (-A * ((B * y + C * z) + D) + x * (B * B + C * C)) / q
    c1 = (-B * ((A * x + C * z) + D) + y * (A * A + C * C)) / q
    c2 = (-C * ((A * x + B * y) + D) + z * (A * A + B * B)) / q
    xa, ya = f["x"], f["y"]
    px = ((c0 * ya[0] + c1 * ya[1]) + c2 * ya[2]) + f["dy"]
    py = ((c0 * xa[0] + c1 * xa[1]) + c2 * xa[2]) + f["dx"]
    return dis, px, py


def extract_corner(center, normal, points, prm: dict, info: dict | None = None):
    """-> the corners [(x, y, z, attached, nx, ny, nz)] of one job, floats as PointXYZINormal holds them."""
    res = prm["proj_image_resolution"]
    f = plane_frame(normal, center)
    p2 = []
    for p in points:
        dis, px, py = project(f, p)
        if dis > 0 or prm["proj_dis_min"] > 0:
            _rec("plane distance", dis, prm["proj_dis_min"])
        _rec("plane distance", dis, prm["proj_dis_max"])
        if dis < prm["proj_dis_min"] or dis > prm["proj_dis_max"]:
            continue
        p2.append((px, py))
    if info is not None:
        info.update(projected=len(p2), branch=f["branch"], cells={}, segments=0)
    if len(p2) <= 5:
        return []
    min_x = min(10.0, min(p[0] for p in p2))
    max_x = max(-10.0, max(p[0] for p in p2))
    min_y = min(10.0, min(p[1] for p in p2))
    max_y = max(-10.0, max(p[1] for p in p2))
    seglen = 5 * res
    nxs, nys = int((max_x - min_x) / seglen + 1), int((max_y - min_y) / seglen + 1)
    cnt: dict = {}
    sx: dict = {}
    sy: dict = {}
    for px, py in p2:
        qx, qy = (px - min_x) / res, (py - min_y) / res
        xi, yi = int(qx), int(qy)
        if _margins is not None:
            for q, lo in ((qx, px == min_x), (qy, py == min_y)):
                if not lo:  # (the box's own minimum sits on its edge exactly)
                    _margins.append(("cell edge", min(q - math.floor(q), math.floor(q) + 1 - q) / CELL_MARGIN * MARGIN))
        c = (xi, yi)
        sx[c] = sx.get(c, 0.0) + px
        sy[c] = sy.get(c, 0.0) + py
        cnt[c] = cnt.get(c, 0) + 1
    out = []
    for xs in range(nxs):
        for ys in range(nys):
            best, bc = 0, None
            for xi in range(xs * 5, xs * 5 + 5):
                for yi in range(ys * 5, ys * 5 + 5):
                    if cnt.get((xi, yi), 0) > best:
                        best, bc = cnt[(xi, yi)], (xi, yi)
            if bc is not None and best >= prm["corner_thre"]:
                px, py = sx[bc] / best, sy[bc] / best
                xyz = [f32((py * f["x"][k] + px * f["y"][k]) + center[k]) for k in range(3)]
                out.append((xyz[0], xyz[1], xyz[2], float(best), f32(normal[0]), f32(normal[1]), f32(normal[2])))
    if info is not None:
        info.update(cells=cnt, segments=nxs * nys)
    return out


def d2f(a, b) -> float:
    """The float squared distance of two corners, x then y then z."""
    F = np.float32
    dx, dy, dz = F(a[0]) - F(b[0]), F(a[1]) - F(b[1]), F(a[2]) - F(b[2])
    return float((dx * dx + dy * dy) + dz * dz)


def non_maxi_suppression(corners, prm: dict):
    r2 = f32(prm["non_max_suppression_radius"] * prm["non_max_suppression_radius"])
    keep = []
    for i, a in enumerate(corners):
        add = True
        for j, b in enumerate(corners):
            if j != i and _lt(d2f(a, b), r2, "radius") and a[3] <= b[3]:
                add = False
        if add:
            keep.append(i)
    return keep


def corner_cut(corners, prm: dict):
    """Pin 3: the first maximum_corner_num by (attached count descending, index ascending)."""
    if prm["maximum_corner_num"] > len(corners):
        return list(corners)
    order = sorted(range(len(corners)), key=lambda i: (-corners[i][3], i))
    return [corners[i] for i in order[:prm["maximum_corner_num"]]]


def triangle(p1, p2, p3, prm: dict, N=Num):
    """One (i, m, n) of build_stdesc -> None (a length gate) or (key, sides, vertex indices 0..2)."""
    def side(u, v):
        d = [N.f(float(np.float32(u[k]) - np.float32(v[k]))) for k in range(3)]
        return N.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    a, b, c = side(p1, p2), side(p1, p3), side(p3, p2)
    hi, lo = prm["descriptor_max_len"], prm["descriptor_min_len"]
    if N is Num:
        for s in (a, b, c):
            _rec("side gate", s, hi)
            _rec("side gate", s, lo)
    if a > hi or b > hi or c > hi or a < lo or b < lo or c < lo:
        return None
    l1, l2, l3 = [1, 2, 0], [1, 0, 3], [0, 2, 3]
    swaps = []
    if N is Num:
        _rec("side order", a, b)
    if a > b:
        a, b, l1, l2 = b, a, l2, l1
    swaps.append(l1 == [1, 0, 3])
    if N is Num:
        _rec("side order", b, c)
    if b > c:
        b, c, l2, l3 = c, b, l3, l2
        swaps.append(True)
    else:
        swaps.append(False)
    if N is Num:
        _rec("side order", a, c)
    if a > c:
        a, c, l1, l3 = c, a, l3, l1
        swaps.append(True)
    else:
        swaps.append(False)
    key = tuple(int(f32(s * 1000)) for s in (a, b, c)) if N is Num else None
    va = 0 if l1[0] == l2[0] else (1 if l1[1] == l2[1] else 2)
    vb = 0 if l1[0] == l3[0] else (1 if l1[1] == l3[1] else 2)
    vc = 0 if l2[0] == l3[0] else (1 if l2[1] == l3[1] else 2)
    return key, (a, b, c), (va, vb, vc), tuple(swaps)


def knn(corners, i, k):
    """Pin 4: the k (or fewer) nearest of corner i by (float squared distance, index)."""
    d = sorted((d2f(corners[i], corners[j]), j) for j in range(len(corners)))
    if _margins is not None:
        for t in range(min(k, len(d) - 1)):
            if d[t + 1][0] != d[t][0]:  # (equal distances are ordered by index: no comparison of values)
                _margins.append(("knn order", (d[t + 1][0] - d[t][0]) / max(d[t + 1][0], 1e-300)))
    return [j for _, j in d[:k]]


def build_stdesc(corners, prm: dict, frame_id: int, info: dict | None = None):
    scale = 1.0 / prm["std_side_resolution"]
    near = prm["descriptor_near_num"]
    seen = set()
    out = []
    tried = 0
    swaps_seen = set()
    for i in range(len(corners)):
        nb = knn(corners, i, near)
        for m in range(1, min(near, len(nb)) - 1):
            for n in range(m + 1, min(near, len(nb))):
                tried += 1
                p = (corners[i], corners[nb[m]], corners[nb[n]])
                t = triangle(p[0], p[1], p[2], prm)
                if t is None:
                    continue
                key, sides, vs, swaps = t
                swaps_seen.add(swaps)
                if key in seen:
                    continue
                seen.add(key)
                A, B, C = (tuple(float(np.float32(p[v][k])) for k in range(3)) for v in vs)
                out.append((tuple(scale * s for s in sides), A, B, C, tuple(((A[k] + B[k]) + C[k]) / 3 for k in range(3)),
                            tuple(p[v][3] for v in vs), frame_id))
    if info is not None:
        info.update(tried=tried, swaps=swaps_seen)
    d = np.zeros(len(out), S.DESC)
    for i, (sl, A, B, C, cen, att, fid) in enumerate(out):
        d["side_length"][i], d["vertex_A"][i], d["vertex_B"][i], d["vertex_C"][i] = sl, A, B, C
        d["center"][i], d["vertex_attached"][i], d["frame_id"][i] = cen, att, fid
    return d


def generate(pts: np.ndarray, prm: dict, order=None, frame_id: int = 0) -> dict:
    """GenerateSTDescs of `pts` (n x 3 float32).  order: the voxel visiting order (keys); None: first appearance."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    vox = init_voxel_map(pts, prm)
    order = list(vox) if order is None else list(order)
    planes = get_plane(vox, order)
    build_connection(vox, order, prm)
    jobs = job_list(vox, order)
    slots = members_sequential(vox, order)
    rank = {k: r for r, k in enumerate(order)}
    raw, job_info = [], []
    for (k, i, ck), sl in zip(jobs, slots):
        points = [pts[p] for w in sl if w is not None for p in vox[w].idx]
        info: dict = {}
        raw += extract_corner(vox[ck].center, vox[ck].normal, points, prm, info)
        info.update(v=rank[k], c=rank[ck], dir=i, members=[0 if w is None else rank[w] + 1 for w in sl])
        job_info.append(info)
    keep = non_maxi_suppression(raw, prm)
    sup = [raw[i] for i in keep]
    fin = corner_cut(sup, prm)
    tinfo: dict = {}
    descs = build_stdesc(fin, prm, frame_id, tinfo)
    corners = np.zeros(len(fin), CORNER)
    for i, c in enumerate(fin):
        corners["xyz"][i], corners["attached"][i], corners["normal"][i] = c[0:3], c[3], c[4:7]
    stats = dict(points=len(pts), voxels=len(vox), plane_voxels=len(planes), jobs=len(jobs), corners_raw=len(raw),
                 corners_suppressed=len(sup), corners=len(fin), triangles_tried=tinfo["tried"], descs=len(descs))
    voxels = np.array([(vox[k].idx[0], len(vox[k].idx), int(vox[k].is_plane)) for k in order], np.int32).reshape(-1, 3)
    return dict(stats=stats, vox=vox, order=order, voxels=voxels, planes=planes, jobs=job_info, raw=raw, keep=keep,
                corners=corners, descs=descs, swaps=tinfo["swaps"])


# ---------------------------------------------------------------------------------------------
# Generators
# ---------------------------------------------------------------------------------------------
def _origin(key, vs=2.0):
    return np.array(key, np.float64) * vs


def wall(rng, key, normal, n, offset=0.5, noise=0.0, vs=2.0):
    """n points of the voxel `key` on the plane of `normal` through the point offset (in edges) along it
    from the voxel's low corner region, kept inside the voxel."""
    nrm = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    o = _origin(key, vs)
    out = []
    while len(out) < n:
        p = o + rng.uniform(0.05, 0.95, 3) * vs
        p = p - nrm * (np.dot(p - (o + 0.5 * vs), nrm) - (offset - 0.5) * vs) + nrm * rng.normal(0, noise) * (noise > 0)
        if np.all(p > o + 0.02 * vs) and np.all(p < o + 0.98 * vs):
            out.append(p)
    return np.array(out, np.float32)


def blob(rng, key, n, vs=2.0, lo=0.1, hi=0.9):
    return (_origin(key, vs) + rng.uniform(lo, hi, (n, 3)) * vs).astype(np.float32)


def surface(rng, origin, u, v, density, noise=0.005):
    """Points of the parallelogram origin + s u + t v at `density` per square metre."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    n = int(np.linalg.norm(np.cross(u, v)) * density)
    nrm = np.cross(u, v) / np.linalg.norm(np.cross(u, v))
    st = rng.uniform(0, 1, (n, 2))
    return np.asarray(origin) + st[:, :1] * u + st[:, 1:] * v + rng.normal(0, noise, (n, 1)) * nrm


def room(rng, density=50.0):
    """A room corner, walls off the voxel faces, with two boxes: -> n x 3 float64."""
    parts = [surface(rng, (0.3, 0.4, 0.2), (9, 0, 0), (0, 9, 0), density),       # floor
             surface(rng, (0.3, 0.4, 0.2), (0, 9, 0), (0, 0, 4.5), density),     # wall x = 0.3
             surface(rng, (0.3, 0.4, 0.2), (9, 0, 0), (0, 0, 4.5), density)]     # wall y = 0.4
    for (bx, by, sx, sy, sz) in ((3.1, 2.7, 1.6, 2.1, 1.3), (5.6, 6.3, 2.3, 1.2, 2.4)):
        o = np.array((bx, by, 0.2))
        parts += [surface(rng, o + (0, 0, sz), (sx, 0, 0), (0, sy, 0), density),
                  surface(rng, o, (sx, 0, 0), (0, 0, sz), density), surface(rng, o + (0, sy, 0), (sx, 0, 0), (0, 0, sz), density),
                  surface(rng, o, (0, sy, 0), (0, 0, sz), density), surface(rng, o + (sx, 0, 0), (0, sy, 0), (0, 0, sz), density)]
    pts = np.concatenate(parts)
    return pts[rng.permutation(len(pts))]


# ---------------------------------------------------------------------------------------------
# Corner modules: a job whose projection image is laid out cell by cell
# ---------------------------------------------------------------------------------------------
MODULE_PRM = dict(plane_detection_thre=0.001)  # a cluster spread 0.15 round a cell's centre is no plane at 0.001


def module(axis: int, clusters, origin=(0, 0, 0), anchor_h=(0.7, 0.9, 1.1)):
    """A non-plane voxel V = origin with the plane voxels C, C2 behind it and points laid out in the image of the
    job (V, C).  axis 0: C's points lie at exactly x = 2 (normal 1 0 0: extract_corner's last branch, image axes
    px = z, py = y); axis 1: at exactly y = 2 (normal 0 1 0: the `B != 0` branch, px = -z, py = x).  A cluster
    (i, j, k, du, dw, h0, h1) is k points on a circle of radius 0.15 round the centre of cell (i, j), moved by (du, dw), at distances h0..h1 from the plane; three anchor points in cell (0, 0) hold the image's minimum.  The
    layout spans the voxels round V; V itself holds the cells 4..7 x 4..7."""
    o = np.array(origin, np.float64) * 2.0
    g = np.random.default_rng(11 + axis)
    walls = []
    for key in (((1, 0, 0), (1, 1, 0)) if axis == 0 else ((0, 1, 0), (1, 1, 0))):
        w = blob(g, key, 60).astype(np.float64)
        w[:, axis] = 2.0
        walls.append(w + o)

    def at(u, w, h):
        return o + ((2.0 - h, -1.9 + w, -1.9 + u) if axis == 0 else (-1.9 + w, 2.0 - h, 3.9 - u))
    pts = [at(0.0, 0.0, anchor_h[0]), at(0.1, 0.05, anchor_h[1]), at(0.05, 0.1, anchor_h[2])]
    for (i, j, k, du, dw, h0, h1) in clusters:
        for t in range(k):
            a = 2 * math.pi * t / k
            pts.append(at((i + 0.5) * 0.5 + du + 0.15 * math.cos(a), (j + 0.5) * 0.5 + dw + 0.15 * math.sin(a),
                          h0 + (h1 - h0) * t / k))
    return np.concatenate(walls + [np.array(pts)]).astype(np.float32)


def _cl(i, j, k, du=0.0, dw=0.0, h0=0.5, h1=1.5):
    return (i, j, k, du, dw, h0, h1)


# the cells case: segment (0,0) two cells of 10 (the first in x-then-y order wins), (0,1) a cell of 9 (no corner),
# (1,0) and (2,1) no points, (1,1) a cell of 11 in V with ten more behind proj_dis_max in the voxel at -x (-y) of V,
# (2,0) a cell of exactly 10
CELLS = [_cl(1, 2, 10), _cl(2, 1, 10), _cl(2, 6, 9), _cl(6, 6, 11), _cl(6, 6, 10, h0=2.5, h1=3.5), _cl(10, 2, 10)]
# the suppression case: row j = 1 two corners of 12, 1.5 apart (both die); row j = 6 a 15 and a 12, 2.02 apart (both
# live); row j = 10 a 15 and a 12, 1.5 apart (the 12 dies)
# (the small offsets keep the corners off a regular grid, whose equal distances would leave no margin)
NMS = [_cl(3, 1, 12, 0.013, -0.007), _cl(6, 1, 12, -0.021, 0.012), _cl(1, 6, 15, -0.01, 0.004), _cl(5, 6, 12, 0.01, -0.009),
       _cl(3, 10, 15, 0.017, 0.006), _cl(6, 10, 12, -0.004, -0.011)]
ONE = [_cl(5, 6, 13)]


@dataclass
class Case:
    name: str
    pts: np.ndarray
    prm: dict
    frame_id: int = 0
    _exp: dict | None = None

    def expected(self) -> dict:
        """The restatement's result under the pinned order; asserts the margins."""
        global _margins
        if self._exp is None:
            _margins = []
            try:
                self._exp = generate(self.pts, self.prm, frame_id=self.frame_id)
                self._exp["margins"] = _margins
            finally:
                _margins = None
            worst: dict = {}
            for kind, m in self._exp["margins"]:
                worst[kind] = min(worst.get(kind, math.inf), m)
            bad = {k: m for k, m in worst.items() if m < MARGIN}
            assert not bad, (self.name, bad)
            self._exp["worst_margins"] = worst
        return self._exp


def _prm(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def _cat(*parts):
    return np.concatenate([np.asarray(p, np.float32).reshape(-1, 3) for p in parts])


CHAIN_NORMALS = tuple((math.cos(math.radians(a)), math.sin(math.radians(a)), 0.0) for a in (25.0, 0.0, 50.0))


def _arm(rng, v, step, normal, n_plane=40):
    """A non-plane voxel v and, along `step`, two plane voxels of one normal behind it."""
    c1 = tuple(v[k] + step[k] for k in range(3))
    c2 = tuple(v[k] + 2 * step[k] for k in range(3))
    return [blob(rng, v, 30), wall(rng, c1, normal, n_plane), wall(rng, c2, normal, n_plane)]


_cases: dict | None = None


def cases() -> dict:
    global _cases
    if _cases is not None:
        return _cases
    c: dict = {}
    rng = np.random.default_rng(20241021)

    def add(name, pts, **kw):
        c[name] = Case(name, _cat(pts), _prm(**kw))

    # voxel keys: negatives, an exact negative multiple of the size, -0.0, and voxels of 10 against 11 points
    keys = [np.array([[-2.0, 0.5, 0.5], [-0.0, -0.0, 0.5], [-0.5, -3.9, -4.0], [1.9999999, -1e-7, 7.0]], np.float32),
            wall(rng, (4, 0, 0), (0, 0, 1), 10), wall(rng, (6, 0, 0), (0, 0, 1), 11)]
    add("keys", _cat(*keys))
    # planes: the least eigenvalue on either side of 0.01 (a slab of uniform thickness t has variance t^2 / 12)
    thin = wall(rng, (0, 0, 0), (0, 0, 1), 400)
    thin[:, 2] += rng.uniform(-0.5, 0.5, 400).astype(np.float32) * np.float32(0.30)   # variance ~0.0075
    thick = wall(rng, (3, 0, 0), (0, 0, 1), 400)
    thick[:, 2] += rng.uniform(-0.5, 0.5, 400).astype(np.float32) * np.float32(0.40)  # variance ~0.0133
    # a normal whose largest component is negative as given, and walls at exactly x = 0 and y = 0 behind a
    # non-plane voxel: extract_corner's `B != 0` branch (normal 0 1 0) and its last one (normal 1 0 0)
    down = wall(rng, (6, 0, 0), (0.2, -0.1, -1.0), 60)

    def exact(key, axis):
        w = blob(rng, key, 60)
        w[:, axis] = np.float32(key[axis] * 2.0)
        return w
    arms = [blob(rng, (0, 3, 0), 60, lo=0.3, hi=0.7), exact((0, 4, 0), 0), exact((0, 5, 0), 0),
            blob(rng, (3, 0, 3), 60, lo=0.3, hi=0.7), exact((4, 0, 3), 1), exact((5, 0, 3), 1)]
    add("planes", _cat(thin, thick, down, *arms))
    # connections: normals just under and just over 0.1 apart, a missing and a non-plane neighbour, a plane voxel
    # with no connected plane (so no job through it)
    def tilt(d):  # a unit normal at chord distance d from (0, 0, 1)
        a = 2 * math.asin(d / 2)
        return (math.sin(a), 0.0, math.cos(a))
    conn = [wall(rng, (0, 0, 0), (0, 0, 1), 40), wall(rng, (1, 0, 0), tilt(0.095), 40),       # merge
            wall(rng, (0, 1, 0), tilt(0.105), 40),                                            # no merge
            blob(rng, (0, 0, 1), 30),                                                         # non-plane neighbour: a job
            blob(rng, (5, 0, 1), 30), wall(rng, (5, 0, 0), (0, 0, 1), 40)]                    # a plane alone: no job
    add("connect", _cat(*conn))
    # jobs: V with 10 against 11 points
    add("v_10_11", _cat(*_arm(rng, (0, 0, 0), (1, 0, 0), (0, 0, 1))[1:], blob(rng, (0, 0, 0), 10),
                        *_arm(rng, (0, 4, 0), (1, 0, 0), (0, 0, 1))[1:], blob(rng, (0, 4, 0), 11)))
    # a W between two arms with normals closer than 0.5 (taken once) and further apart (taken twice)
    for name, ang in (("w_once", 20.0), ("w_twice", 40.0)):
        n2 = (math.cos(math.radians(ang)), math.sin(math.radians(ang)), 0.0)
        add(name, _cat(blob(rng, (0, 0, 0), 60, lo=0.3, hi=0.7), *_arm(rng, (-1, 0, 0), (-1, 0, 0), (1, 0, 0)),
                       *_arm(rng, (0, -1, 0), (0, -1, 0), n2)))
    # the chain: W = (0,0,0) is reached from three arms whose normals are 25, 0 and 50 degrees in visiting order; the
    # middle one is close to both others, the others are not close to each other
    add("chain", _cat(blob(rng, (0, 0, 0), 60, lo=0.3, hi=0.7), *_arm(rng, (-1, 0, 0), (-1, 0, 0), CHAIN_NORMALS[0]),
                      *_arm(rng, (0, -1, 0), (0, -1, 0), CHAIN_NORMALS[1]), *_arm(rng, (0, 0, -1), (0, 0, -1), CHAIN_NORMALS[2])))
    add("empty", np.zeros((0, 3), np.float32))
    add("no_plane", _cat(blob(rng, (0, 0, 0), 50), blob(rng, (1, 0, 0), 50)))
    # the room, sampled twice: the second time with range noise, turned a quarter about z and moved (the voxel grid
    # maps onto itself, the projection images' axes and bins do not)
    r0 = room(np.random.default_rng(7))
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    r1 = (r0 + np.random.default_rng(9).normal(0, 0.001, r0.shape)) @ R.T + np.array([2.0, -4.0, 0.0])
    add("room", r0)
    add("room_again", r1)
    c["room_again"].frame_id = 1
    # the cut and the neighbour count on the room's corners: fewer corners than descriptor_near_num, ties at the cut
    for k in (2, 3, 9):
        add(f"room_cut_{k}", r0, maximum_corner_num=k)
    add("room_short_sides", r0, descriptor_min_len=4.0, descriptor_max_len=7.0)
    add("room_fine", r0, proj_image_resolution=0.25, corner_thre=4.0, non_max_suppression_radius=1.0)
    # corners, cell by cell, through both of the axis construction's lower branches
    for axis in (0, 1):
        add(f"cells_{axis}", module(axis, CELLS), **MODULE_PRM)
        add(f"nms_{axis}", module(axis, NMS), **MODULE_PRM)
    # 5 against 6 projected points: eight more points of V lie beyond a proj_dis_max of 1
    for k in (5, 6):
        add(f"projected_{k}", module(0, [_cl(6, 6, k, h0=0.3, h1=0.7), _cl(5, 5, 4, h0=1.4, h1=1.6), _cl(7, 5, 4, h0=1.4, h1=1.6)],
                                     anchor_h=(1.3, 1.5, 1.7)),
            proj_dis_max=1.0, corner_thre=3.0, **MODULE_PRM)
    # 99, 100 and 101 surviving corners, counts of 15, 12 and 13: ties at the cut of 100
    for n in (99, 100, 101):
        ys = np.cumsum([0] + [8 + m % 3 for m in range(40)])  # uneven gaps: no two modules equally far from a third
        mods = [module(0, NMS, (0, int(ys[m]), 0)) for m in range(33)] + \
               [module(0, ONE, (0, int(ys[33 + m]), 0)) for m in range(n - 99)]
        add(f"cut_{n}", _cat(*mods), **MODULE_PRM)
    _cases = c
    return c


LOOP_PRM = dict(S.DEFAULTS, skip_near_num=0)


def room_loop() -> dict:
    """The room's two key frames through the loop search's restatement: frame 0 committed, frame 1 searched."""
    cs = cases()
    a, b = cs["room"].expected(), cs["room_again"].expected()
    db = S.Db()
    db.add(a["descs"], a["planes"])
    return S.search_loop(db, b["descs"], b["planes"], LOOP_PRM)


def measure_deviation(names=None) -> dict:
    """The float64 restatement against 60-digit mpmath on every plane voxel, corner and triangle of the cases."""
    import mpmath as mp
    mp.mp.dps = 60

    class M:
        sqrt = staticmethod(mp.sqrt)
        f = staticmethod(mp.mpf)
        f32 = staticmethod(lambda x: x)

    dev = dict(center=0.0, normal=0.0, corner=0.0, side=0.0, vertex=0.0)
    for name, case in cases().items():
        if names is not None and name not in names:
            continue
        e = case.expected()
        pts = case.pts
        for v in e["vox"].values():
            if not v.is_plane:
                continue
            cen, _, nrm, _ = plane_fit([pts[i] for i in v.idx], M)
            dev["center"] = max(dev["center"], max(abs(float(cen[k] - v.center[k])) for k in range(3)))
            dev["normal"] = max(dev["normal"], max(abs(float(nrm[k] - v.normal[k])) for k in range(3)))
        # a corner: the cell mean and the reprojection, from the exact plane of the restatement's voxel
        order, vox = e["order"], e["vox"]
        for info in e["jobs"]:
            if not info.get("cells"):
                continue
            ck = order[info["c"]]
            cv = vox[ck]
            f = plane_frame(tuple(mp.mpf(x) for x in cv.normal), tuple(mp.mpf(x) for x in cv.center), M)
            f64 = plane_frame(cv.normal, cv.center)
            points = [pts[p] for w in info["members"] if w for p in vox[order[w - 1]].idx]
            sums: dict = {}
            proj = []
            for p in points:
                dis, px, py = project(f64, p)
                if dis < case.prm["proj_dis_min"] or dis > case.prm["proj_dis_max"]:
                    continue
                proj.append((px, py, project(f, p, M)))
            min_x, min_y = min(10.0, min(q[0] for q in proj)), min(10.0, min(q[1] for q in proj))
            res = case.prm["proj_image_resolution"]
            for px, py, (_, ex, ey) in proj:
                cidx = (int((px - min_x) / res), int((py - min_y) / res))
                s = sums.setdefault(cidx, [0.0, 0.0, mp.mpf(0), mp.mpf(0), 0])
                s[0] += px
                s[1] += py
                s[2] += ex
                s[3] += ey
                s[4] += 1
            for s in sums.values():
                if s[4] < case.prm["corner_thre"]:
                    continue
                for k in range(3):
                    got = (s[1] / s[4] * f64["x"][k] + s[0] / s[4] * f64["y"][k]) + cv.center[k]
                    want = (s[3] / s[4] * f["x"][k] + s[2] / s[4] * f["y"][k]) + f["center"][k]
                    dev["corner"] = max(dev["corner"], abs(float(got - want)))
        for d in e["descs"]:
            A, B, C = (tuple(mp.mpf(float(x)) for x in d[k]) for k in ("vertex_A", "vertex_B", "vertex_C"))
            def fd(u, w):  # the float difference is the specified arithmetic
                return [mp.mpf(float(np.float32(float(u[k])) - np.float32(float(w[k])))) for k in range(3)]
            exact = [mp.sqrt(sum(x * x for x in fd(u, w))) for u, w in ((A, B), (A, C), (B, C))]
            scale = mp.mpf(1) / mp.mpf(case.prm["std_side_resolution"])
            for k in range(3):
                dev["side"] = max(dev["side"], abs(float(scale * exact[k] - mp.mpf(float(d["side_length"][k])))))
                cen = (A[k] + B[k] + C[k]) / 3
                dev["vertex"] = max(dev["vertex"], abs(float(cen - mp.mpf(float(d["center"][k])))))
    return dev
