"""Shared cases and a grid-free reference for KD_TREE::Delete_Point_Boxes
(ikd_Tree.cpp:501-521 -> Delete_by_range, :626-688) and the incremental map's
life cycle around it.

The reference (class Brute) keeps the map as two arrays, the float32 points by
id and an alive mask, and uses no grid, cell or tree:

* a deletion is the mask  vertex_min <= p  and  p < vertex_max  on the three
  axes, in float32, over the alive points, united over the boxes; its count is
  the size of that union.  A NaN vertex compares false, so it hits nothing;
  0.0 <= -0.0 is true.  These are Delete_by_range's own comparisons on a point
  (:645-647: range_min <= p && range_max > p); its subtree pruning (:637-644)
  only skips or takes whole subtrees the same comparisons decide;
* the 5 nearest alive points of a query by (d, x, id), with
  d = (dx*dx + dy*dy) + dz*dz in float32, unfused, in that order; with fewer
  than 5 alive points the missing neighbours are index -1 at distance +inf
  (what oracle.DynMap.knn returns and test_knn_edge_maps pins for the device);
* Add_Points is not restated here: it stays with oracle.DynMap (pinned in
  tests/test_ikd_incr_oracle.py), and the reference takes over the points and
  ids the oracle's call left (Ref.add).

A case is {"map": (M, 3) float32, "steps": [...]}; a step is
("delete", boxes) or ("add", points, downsample_size, downsample) or
("iekf", body, state), where boxes / points may be a function of the Ref (the
step depends on the map the earlier steps left).  tests/test_ikd_delete_reference.py
runs every case on the CPU (oracle.DynMap against Brute),
tests/test_gpu_ikd_delete.py on the device (against Brute).
"""
import functools

import numpy as np

f32 = np.float32
INF = f32(np.inf)
K = 5


def up(v, n=1):
    v = np.asarray(v, f32)
    for _ in range(n):
        v = np.nextafter(v, INF)
    return v


def down(v, n=1):
    v = np.asarray(v, f32)
    for _ in range(n):
        v = np.nextafter(v, -INF)
    return v


class Brute:
    """The map as points by id and an alive mask; nothing else."""

    def __init__(self, xyz):
        self.P = np.ascontiguousarray(xyz, f32).reshape(-1, 3).copy()
        self.alive = np.ones(len(self.P), bool)

    @property
    def n_ids(self):
        return len(self.P)

    def hit_mask(self, boxes):
        """Alive points inside any box [vertex_min, vertex_max), float32 comparisons."""
        b = np.ascontiguousarray(boxes, f32).reshape(-1, 6)
        hit = np.zeros(len(self.P), bool)
        with np.errstate(invalid="ignore"):
            for lo, hi in zip(b[:, :3], b[:, 3:]):
                hit |= np.all((lo <= self.P) & (self.P < hi), axis=1)
        return hit & self.alive

    def delete_boxes(self, boxes) -> int:
        hit = self.hit_mask(boxes)
        self.alive &= ~hit
        return int(hit.sum())

    def dump(self):
        ids = np.nonzero(self.alive)[0].astype(np.int32)
        return self.P[ids], ids

    def dead(self):
        """Coordinates of every id deleted so far."""
        return self.P[~self.alive]

    def knn(self, q, k=K):
        q = np.ascontiguousarray(q, f32).reshape(-1, 3)
        P, ids = self.dump()
        out_i = np.full((len(q), k), -1, np.int32)
        out_d = np.full((len(q), k), INF, f32)
        if len(ids) == 0:
            return out_i, out_d
        kk = min(k, len(ids))
        for s in range(0, len(q), 256):
            c = q[s:s + 256]
            dx = P[None, :, 0] - c[:, None, 0]
            dy = P[None, :, 1] - c[:, None, 1]
            dz = P[None, :, 2] - c[:, None, 2]
            d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == f32
            kth = np.partition(d, kk - 1, axis=1)[:, kk - 1]
            for r in range(len(c)):
                cand = np.nonzero(d[r] <= kth[r])[0]
                o = cand[np.lexsort((ids[cand], P[cand, 0], d[r, cand]))[:kk]]
                out_i[s + r, :kk] = ids[o]
                out_d[s + r, :kk] = d[r, o]
        return out_i, out_d


class Ref:
    """The brute-force reference with the oracle beside it (Add_Points, IEKF)."""

    def __init__(self, xyz):
        import oracle
        self.b = Brute(xyz)
        self.dm = oracle.DynMap(xyz)
        self.base_ids = self.b.n_ids

    def delete(self, boxes):
        """(brute-force count, oracle's count)."""
        return self.b.delete_boxes(boxes), self.dm.delete_boxes(boxes)

    def add(self, W, ds, downsample=True):
        """oracle.DynMap.add_points; the reference takes the ids and points it left."""
        n0 = self.b.n_ids
        st = self.dm.add_points(W, ds, downsample=downsample)
        self.adopt(n0, st["added"])
        return st

    def adopt(self, n0, added):
        xyz, ids = self.dm.dump()
        new = ids >= n0
        assert np.array_equal(ids[new], np.arange(n0, n0 + added))  # the next ids, none reused
        self.b.P = np.concatenate([self.b.P, xyz[new]])
        self.b.alive = np.zeros(n0 + added, bool)
        self.b.alive[ids] = True


def queries(ref, seed, n_live=250, n_rand=250):
    """Every deleted point's coordinates (distance-0 candidates that must not
    come back), surviving points, random points about the map."""
    rng = np.random.default_rng(seed)
    P, _ = ref.b.dump()
    allp = ref.b.P
    lo, hi = (allp.min(0) - 1, allp.max(0) + 1) if len(allp) else (-np.ones(3), np.ones(3))
    live = P[rng.choice(len(P), min(n_live, len(P)), replace=False)] if len(P) else P
    return np.concatenate([ref.b.dead(), live, rng.uniform(lo, hi, (n_rand, 3))]).astype(f32)


def resolve(x, ref):
    return x(ref) if callable(x) else x


def point_boxes(p):
    """One box per point holding exactly that coordinate triple: [p, nextafter(p))."""
    p = np.asarray(p, f32).reshape(-1, 3)
    return np.concatenate([p, up(p)], axis=1)


EVERYTHING = np.array([[-np.inf] * 3 + [np.inf] * 3], f32)


# ------------------------------------------------------------------ faces ----
BOX_A = np.array([-2.5, 0.0, 0.5, 1.5, 3.0, 2.25], f32)    # x: - to +; y: a min face at 0.0; z: + to +
BOX_B = np.array([-3.0, -2.0, -3.5, 0.0, -0.5, -1.0], f32)  # x: a max face at 0.0; y, z: - to -


def face_points(box, rng, per=3):
    """For each axis: points on vertex_min and on vertex_max and one float32 step
    to each side of both (at a 0.0 face also -0.0), the other two coordinates
    inside the box; and the corners."""
    lo, hi = box[:3], box[3:]
    out = []
    for a in range(3):
        for v in (lo[a], hi[a]):
            vals = [down(v), v, up(v)] + ([f32(-0.0)] if v == 0 else [])
            for x in vals:
                for _ in range(per):
                    p = rng.uniform(lo + f32(0.1), hi - f32(0.1)).astype(f32)
                    p[a] = x
                    out.append(p)
    out += [lo.copy(), hi.copy(), down(hi), down(lo), up(lo),
            np.array([lo[0], down(hi[1]), lo[2]], f32), np.array([hi[0], lo[1], lo[2]], f32)]
    return np.array(out, f32)


@functools.lru_cache(None)
def case_faces():
    rng = np.random.default_rng(101)
    m = np.concatenate([rng.uniform(-4, 4, (1500, 3)).astype(f32), face_points(BOX_A, rng), face_points(BOX_B, rng)])
    m = m[rng.permutation(len(m))]
    p7 = m[7]
    odd = np.array([np.concatenate([p7, p7]),                      # min == max: empty
                    [1.0, 1.0, 1.0, 1.0, 3.0, 3.0],                 # min == max on one axis
                    [3.0, 3.0, 3.0, -3.0, -3.0, -3.0],              # inverted
                    [-3.0, -3.0, 3.0, 3.0, 3.0, -3.0],              # inverted on one axis
                    [np.nan, -9, -9, 9, 9, 9], [-9, -9, -9, 9, 9, np.nan], [np.nan] * 6,
                    [1e4, 1e4, 1e4, 1e4 + 10, 1e4 + 10, 1e4 + 10],  # far outside the map
                    [-3e38, 5.0, -3e38, 3e38, 3e38, 3e38],          # huge, beside the map
                    [1e30, 1e30, 1e30, 2e30, 2e30, 2e30]], f32)
    W = rng.uniform(-4, 4, (600, 3)).astype(f32)
    steps = [("delete", np.zeros((0, 6), f32)),  # the first incremental call on the built map
             ("delete", BOX_A[None]), ("delete", BOX_B[None]), ("delete", odd),
             ("delete", np.zeros((0, 6), f32)),
             ("delete", np.stack([BOX_A, BOX_B])),  # again: nothing left in them
             ("delete", EVERYTHING),
             ("add", W, 0.5, True)]
    return {"map": m, "steps": steps}


# ------------------------------------------------ overlap, repeats, shapes ----
def _far_boxes(rng, n):
    c = rng.uniform(100, 200, (n, 3))
    return np.concatenate([c, c + 1.0], axis=1).astype(f32)


@functools.lru_cache(None)
def case_overlap():
    rng = np.random.default_rng(102)
    m = rng.uniform(-5, 5, (2000, 3)).astype(f32)
    m[:3] = [[0.5, 0.5, 0.5], [0.25, 0.75, 0.5], [0.9, 0.1, 0.2]]  # inside all three boxes below
    three = np.array([[-1, -1, -1, 1, 1, 1], [0, 0, 0, 2, 2, 2], [-0.5, 0, -2, 1.5, 1, 3], [0, 0, 0, 2, 2, 2]], f32)

    def hit(ref, k):  # a small box about the k-th alive point
        P, _ = ref.b.dump()
        return np.concatenate([P[k] - f32(0.3), P[k] + f32(0.3)]).astype(f32)

    def first(ref):
        return np.concatenate([hit(ref, 11)[None], _far_boxes(np.random.default_rng(1), 299)])

    def last(ref):
        return np.concatenate([_far_boxes(np.random.default_rng(2), 299), hit(ref, 600)[None]])

    def both(ref):
        h = hit(ref, 1200)[None]
        return np.concatenate([h, _far_boxes(np.random.default_rng(3), 298), h])

    steps = [("delete", three), ("delete", three), ("delete", first), ("delete", first), ("delete", last),
             ("delete", both)]
    return {"map": m, "steps": steps}


@functools.lru_cache(None)
def case_n_ids(n):
    """n ids (the deletion's launch covers ids in blocks of 256): the first and the last id deleted, again,
    then three points added without downsampling and the newest deleted."""
    rng = np.random.default_rng(200 + n)
    m = rng.uniform(-1, 1, (n, 3)).astype(f32)
    W = rng.uniform(-1, 1, (3, 3)).astype(f32)
    ends = point_boxes(m[[0, n - 1]])
    steps = [("delete", ends), ("delete", ends), ("add", W, 0.5, False), ("delete", point_boxes(W[2])),
             ("delete", np.concatenate([ends, point_boxes(W[2])]))]
    return {"map": m, "steps": steps}


# --------------------------------------------------- session-added points ----
@functools.lru_cache(None)
def case_session_added():
    rng = np.random.default_rng(103)
    m = rng.uniform(-4, 4, (3000, 3)).astype(f32)
    A = rng.uniform(-4, 4, (800, 3)).astype(f32)
    B = rng.uniform(-4, 4, (500, 3)).astype(f32)

    def some(ref, added, n, seed):
        _, ids = ref.b.dump()
        ids = ids[ids >= ref.base_ids] if added else ids[ids < ref.base_ids]
        pick = np.random.default_rng(seed).choice(ids, n, replace=False)
        return point_boxes(ref.b.P[pick])

    region = np.array([[0, 0, 0, 2, 2, 2], [-2, -1, -1.5, -0.5, 0, 0]], f32)  # whole 0.5 m boxes of Add_Points
    again = np.concatenate([rng.uniform([0, 0, 0], [2, 2, 2], (300, 3)),
                            rng.uniform([-2, -1, -1.5], [-0.5, 0, 0], (150, 3)),
                            rng.uniform(-4, 4, (150, 3))]).astype(f32)
    steps = [("add", A, 0.5, True), ("add", B, 0.5, False),
             ("delete", lambda r: some(r, False, 40, 1)),   # base ids only
             ("delete", lambda r: some(r, True, 40, 2)),    # ids added in this session only
             ("delete", region),                            # both
             ("add", again, 0.5, True),                     # into boxes whose stored point was just deleted
             ("delete", lambda r: np.concatenate([some(r, True, 30, 3), some(r, False, 30, 4)])),
             ("add", again[::-1].copy(), 0.5, True)]
    return {"map": m, "steps": steps}


# ------------------------------------------ emptied cells, an emptied map ----
def _clusters(rng):
    """5 x 4 x 3 clusters 3 m apart, each inside a 0.5 m cube: a box about one removes whole cells of any
    grid with cells under 2.5 m, and the clusters at the least and the greatest corner hold the first and
    the last point of a (z, y, x) cell-key order."""
    g = np.stack(np.meshgrid(np.arange(5), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3) * 3.0
    pts = np.concatenate([c + rng.uniform(-0.25, 0.25, (int(rng.integers(40, 80)), 3)) for c in g])
    return pts[rng.permutation(len(pts))].astype(f32), g


def _iekf_scan(rng, lo, hi, n=400):
    """A scan of points about the map's extent, the state's pose the identity."""
    from livo_amd import synth
    st = synth.make_state(0)
    st["rot"], st["pos"] = np.eye(3), np.zeros(3)
    return rng.uniform(lo, hi, (n, 3)).astype(f32), st


@functools.lru_cache(None)
def case_cells_and_empty():
    rng = np.random.default_rng(104)
    m, g = _clusters(rng)

    def about(c):
        c = np.asarray(c, f32)
        return np.concatenate([c - f32(1.0), c + f32(1.0)])[None]

    body, st = _iekf_scan(rng, [-1, -1, -1], [13, 10, 7])
    W1 = np.concatenate([g[5] + rng.uniform(-0.25, 0.25, (200, 3)), rng.uniform(-1, 13, (300, 3))]).astype(f32)
    W2 = rng.uniform(0, 6, (200, 3)).astype(f32)
    steps = [("delete", about(g.min(0))), ("delete", about(g.max(0))), ("delete", about(g[31])),
             ("iekf", body, st),
             ("delete", np.array([[-1e3] * 3 + [1e3] * 3], f32)),  # everything
             ("iekf", body, st),
             ("delete", about(g[3])),                              # on the emptied map
             ("add", W1, 0.5, True), ("iekf", body, st), ("add", W2, 0.5, False),
             ("delete", EVERYTHING), ("add", W2, 0.5, False), ("add", W1, 0.3, True)]
    return {"map": m, "steps": steps}


# ----------------------------------------------- delete, then the fused add ----
@functools.lru_cache(None)
def case_fused():
    """test_add_points_wrapped_box_key_clash_fused's map and batches (0.05 m boxes) with a deletion before
    every add."""
    rng = np.random.default_rng(105)
    m = rng.uniform(0, 2, (400, 3)).astype(f32)
    steps = [("add", rng.uniform(0, 2, (200, 3)).astype(f32), 0.05, True)]
    for _ in range(5):
        c = rng.uniform(0.2, 1.5, 3)
        steps.append(("delete", np.concatenate([c, c + 0.4]).astype(f32)[None]))
        steps.append(("add", rng.uniform(0, 2, (200, 3)).astype(f32), 0.05, True))
    return {"map": m, "steps": steps}


# -------------------------------------------------- the runs under deletion ----
RUNS_BASE = 4000


def _x_slab(ref, frac):
    """A slab across the map holding about frac of the base's points among those still alive, from the low-x side."""
    P, ids = ref.b.dump()
    x = np.sort(P[ids < ref.base_ids, 0])
    cut = x[min(int(frac * ref.base_ids), len(x) - 1)]
    return np.array([[-1e3, -1e3, -1e3, cut, 1e3, 1e3]], f32)


def _added_since_base(ref):
    P, ids = ref.b.dump()
    return point_boxes(P[ids >= ref.base_ids])


@functools.lru_cache(None)
def case_runs():
    rng = np.random.default_rng(106)
    m = rng.uniform([-6, -6, -1.5], [6, 6, 1.5], (RUNS_BASE, 3)).astype(f32)
    W1 = rng.uniform([-6, -6, -1.5], [6, 6, 1.5], (300, 3)).astype(f32)
    W2 = rng.uniform([-6, -6, -1.5], [6, 6, 1.5], (300, 3)).astype(f32)
    steps = [("delete", lambda r: _x_slab(r, 0.05)), ("add", W1, 0.3, True), ("delete", _added_since_base),
             ("add", W2, 0.3, True), ("delete", lambda r: _x_slab(r, 0.30))]
    return {"map": m, "steps": steps}


# ------------------------------------------------------ a sliding local map ----
SLIDE_HALF = 8.0


@functools.lru_cache(None)
def case_sliding():
    """A local map cube about the sensor (the synthetic room within 8 m of the origin), six scans: before each,
    one or two slabs on the sides the sensor faces away from leave the map (lasermap_fov_segment's
    cub_needrm boxes), each 0.6 m further in than the last on that side."""
    from livo_amd import synth
    m = synth.make_map(60_000)
    m = m[np.all(np.abs(m[:, :2]) < SLIDE_HALF, axis=1)]
    edge = {}
    scans = []
    for k in range(6):
        body, _, _ = synth.make_scan(2000, 100 + k)
        st = synth.make_state(100 + k)
        h = st["rot"][:, 0]
        order = np.argsort(-np.abs(h[:2]))
        boxes = []
        for a in order[:1 + k % 2]:
            side = -1.0 if h[a] > 0 else 1.0  # behind the sensor on this axis
            e0 = edge.get((a, side), (SLIDE_HALF + 40.0) * side)
            e1 = (min(abs(e0), SLIDE_HALF) - 0.6) * side
            edge[(a, side)] = e1
            b = np.array([-1e3, -1e3, -1e3, 1e3, 1e3, 1e3], f32)
            b[a], b[a + 3] = min(e0, e1), max(e0, e1)
            boxes.append(b)
        scans.append((np.array(boxes, f32), body, st))
    return {"map": m, "scans": scans, "filter_size_map": 0.3}


STEP_CASES = {
    "faces": case_faces,
    "overlap": case_overlap,
    "n_ids_1": lambda: case_n_ids(1),
    "n_ids_255": lambda: case_n_ids(255),
    "n_ids_256": lambda: case_n_ids(256),
    "n_ids_257": lambda: case_n_ids(257),
    "session_added": case_session_added,
    "cells_and_empty": case_cells_and_empty,
    "fused": case_fused,
    "runs": case_runs,
}
