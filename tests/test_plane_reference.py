"""The CPU oracle's plane fit and gates against the mpmath reference (oracle/plane_ref.py).

The oracle's esti_plane is Eigen's float column-pivoting QR restated; everything on the device is
held against it bit for bit, and until now it was itself pinned only on well-conditioned patches
(tests/test_oracle.py).  Here:
  * coverage: over the case families every branch of the QR is taken by at least 20 cases (tau = 0,
    a rank-2 and a rank-1 basic solution, a recomputed column norm, c[i] == 0 in back substitution,
    bit-equal column norms, the NaN normal, a body point at the origin), and all six column
    permutations occur.  nonzero takes 1, 2 and 3; 0 cannot be reached in float arithmetic: the
    step-0 test is mxn^2 < (mxn eps)^2 (also 0 < 0 for a zero matrix, NaN < NaN, inf < inf), so the
    rank-0 cluster at the origin runs with nonzero = 3 and divides by zero pivots (the NaN normal);
  * the trace entry point returns the bits of orc_esti_plane on every case;
  * accuracy: full-rank fits against lstsq() at C_BAR * FLT_EPSILON (kappa + kappa^2 rho); rank-
    deficient fits against the basic solution on the trace's pivot columns at the same bar with the
    sub-matrix's kappa and rho.  Fits the trace calls full rank at sigma_min <= 1e-5 sigma_max (most
    at 5000 m, the 400 m sweep) are held to the same bar, reported apart.  Fits whose rank test lies
    within RANK_MARGIN of its threshold (exactly dependent columns: the test then falls on rounding
    noise), the clusters whose squares lie below FLT_MIN (Eigen drops their tails) and any with
    kappa FLT_EPSILON >= VOID_BOUND are left to the GPU-against-oracle tests: at most 5 % of the cases;
  * decisions: oracle.h_share's sel equals the reference's gates wherever they are decided
    (DECIDED_ULPS), and each sweep flips once, within 2 steps of the reference's flip.
"""
import collections

import numpy as np
import pytest

MIN_CASES = 20


@pytest.fixture(scope="module")
def cases(built):
    import oracle
    import plane_ref as pr
    rows = []
    for sh in pr.sheets():
        tree = oracle.Tree(sh["map"])
        st = sh["state"]
        hs = tree.h_share(sh["body"], st["rot"], st["pos"], np.eye(3), np.zeros(3), True)
        # the tree's neighbours are the brute-force ones; among points at one float distance and one x
        # (duplicates) PointType_CMP leaves the order to the traversal, so the rows are the tree's
        idx = hs["cache"]["idx"]
        assert np.array_equal(np.sort(idx, axis=1), np.sort(sh["nn_idx"], axis=1))
        assert np.array_equal(hs["cache"]["d"], sh["nn_d"])
        distinct = np.all(np.diff(sh["nn_d"], axis=1) > 0, axis=1)
        assert np.array_equal(idx[distinct], sh["nn_idx"][distinct])
        nb = sh["map"][idx]
        world = oracle.to_world(sh["body"], st)[:, :3]
        for i in range(len(nb)):
            ok, pa, tr = oracle.esti_plane_trace(nb[i])
            rows.append({"sheet": sh["index"], "i": i, "family": str(sh["family"][i]), "pts": nb[i], "ok": ok,
                         "pabcd": pa, "trace": tr, "sel": int(hs["sel"][i]), "normvec": hs["normvec"][i],
                         "world": world[i], "body": sh["body"][i], "sqd4": float(sh["nn_d"][i, 4])})
    return rows


def _rank_margin(tr):
    """The closest any rank test of the fit came to its threshold, as a factor (>= 1)."""
    last = min(tr["nonzero"], 2)  # the tests run at steps 0 .. nonzero (the failing one included)
    worst = np.inf
    for k in range(last + 1):
        a, b = float(tr["big_sq"][k]), float(tr["rank_thr"][k])
        if a == b:
            return 1.0
        if a > 0 and b > 0:
            worst = min(worst, max(a / b, b / a))
    return worst


def test_trace_is_the_same_function(cases):
    import oracle
    for c in cases:
        ok, pa = oracle.esti_plane(c["pts"])
        assert ok == c["ok"], (c["family"], c["sheet"], c["i"])
        assert np.array_equal(pa.view(np.uint32), c["pabcd"].view(np.uint32)), (c["family"], c["sheet"], c["i"])


def _branches(rows):
    n = collections.Counter()
    for c in rows:
        tr = c["trace"]
        n[f"nonzero={tr['nonzero']}"] += 1
        n[f"perm={tr['perm']}"] += 1
        n["tau_zero"] += bool(tr["tau_zero"].any())
        n["tau_zero_step0"] += bool(tr["tau_zero"][0])
        n["norm_recomputed"] += bool(tr["recomputed"].any())
        n["back_skipped"] += bool(tr["back_skipped"][:max(tr["nonzero"], 0)].any())
        n["tie_step0"] += bool(tr["tie"][0])
        n["tie_step1"] += bool(tr["tie"][1])
        n["nan_normal"] += bool(np.isnan(c["pabcd"]).any())
        n["fit_rejected"] += not c["ok"]
        if "body" in c:
            n["body_at_origin"] += not np.any(c["body"])
    return n


def test_coverage(cases):
    n = _branches(cases)
    print("branches over the case families:", dict(sorted(n.items())))
    for key in ("nonzero=1", "nonzero=2", "nonzero=3", "tau_zero", "tau_zero_step0", "norm_recomputed",
                "back_skipped", "tie_step0", "tie_step1", "nan_normal", "fit_rejected"):
        assert n[key] >= MIN_CASES, (key, n[key])
    assert n["nonzero=0"] == 0  # unreachable, see the module docstring
    assert n["body_at_origin"] == 1
    perms = [k for k in n if k.startswith("perm=")]
    assert len(perms) == 6, perms
    fam = collections.Counter(c["family"] for c in cases)
    rough = [c for c in cases if c["family"] == "rough"]
    share = sum(not c["ok"] for c in rough) / len(rough)
    print("families:", dict(fam), "rough rejected by the 0.1 test:", round(share, 3))
    assert 0.15 <= share <= 0.45, share  # "about 30 %"


def test_room_scan_branches(built, map100k, tree100k):
    """The evidence for the gap (no assertion): the branches one synthetic room scan reaches."""
    import oracle
    from livo_amd import synth
    body = synth.make_scan(10_000, 1)[0]
    st = synth.make_state(1)
    hs = tree100k.h_share(body, st["rot"], st["pos"], np.eye(3), synth.T_LI, True)
    rows = []
    for idx in hs["cache"]["idx"]:
        ok, pa, tr = oracle.esti_plane_trace(map100k[idx])
        rows.append({"ok": ok, "pabcd": pa, "trace": tr})
    print("branches of make_scan(10_000, 1) on map100k:", dict(sorted(_branches(rows).items())))


def test_accuracy(cases):
    import plane_ref as pr
    worst = collections.defaultdict(float)
    excluded = collections.Counter()
    fails = []
    for c in cases:
        tr = c["trace"]
        fam = c["family"]
        if np.isnan(c["pabcd"]).any():
            # the rank-0 fit: every pivot is zero, there is no solution to compare; NaN-ness is the check
            assert not np.any(c["pts"]), (fam, c["sheet"], c["i"])
            continue
        if _rank_margin(tr) < pr.RANK_MARGIN:
            excluded["rank test near its threshold"] += 1
            continue
        if np.abs(c["pts"]).max() < 1e-18:
            # squares below FLT_MIN: makeHouseholder drops a tail as large as its head (tau = 0), the
            # fit is Eigen's answer, not a least-squares one; held GPU against oracle only
            assert tr["tau_zero"].all() and fam == "tau_zero_denorm"
            excluded["squares below FLT_MIN"] += 1
            continue
        nz = tr["nonzero"]
        cols = tr["perm"][:nz]
        ref = pr.lstsq(c["pts"], cols)
        if ref["x"] is None or pr.FLT_EPS * ref["sv"][0] >= pr.VOID_BOUND * ref["sv"][-1]:
            excluded["kappa FLT_EPSILON too large for a first-order bound"] += 1
            continue
        ill = nz == 3 and ref["sv"][-1] <= pr.FULL_RANK_RATIO * ref["sv"][0]
        x = c["pabcd"][:3].astype(np.float64) / np.float64(c["pabcd"][3])
        err = np.linalg.norm(x - ref["x"]) / np.linalg.norm(ref["x"])
        ratio = err / pr.error_bar(ref)
        key = (fam + " (kappa > 1e5)" if ill else fam) if nz == 3 else f"{fam} (rank {nz})"
        worst[key] = max(worst[key], ratio)
        if ratio > pr.C_BAR:
            fails.append((key, c["sheet"], c["i"], ratio))
    share = sum(excluded.values()) / len(cases)
    top = max(worst.values())
    print("largest error / (FLT_EPSILON (kappa + kappa^2 rho)) by family:",
          {k: round(v, 3) for k, v in sorted(worst.items())})
    print(f"largest ratio {top:.3f}; C_BAR {pr.C_BAR}; excluded {dict(excluded)} = {share:.2%} of {len(cases)}")
    assert share <= 0.05, share
    assert not fails, fails[:10]
    # the bar stands at four times the measured ratio, rounded up to a power of two
    assert pr.C_BAR == 2.0 ** np.ceil(np.log2(4 * pr.MEASURED_RATIO))
    assert top <= pr.MEASURED_RATIO * 1.001, (top, pr.MEASURED_RATIO)


def _ref_gates(c):
    import plane_ref as pr
    return pr.gates(c["pabcd"], c["world"], c["body"], sqd4=c["sqd4"], pts=c["pts"])


def test_decisions(cases):
    import plane_ref as pr
    undecided = 0
    for c in cases:
        g = _ref_gates(c)
        if not pr.decided(g):
            undecided += 1
            continue
        want = pr.decision(g)
        assert c["sel"] == int(want), (c["family"], c["sheet"], c["i"], g)
        if g["ok_sqd"]:
            assert c["ok"] == g["ok_fit"], (c["family"], c["sheet"], c["i"], g)
    print("undecided cases (inside 16 ulps of a threshold):", undecided, "of", len(cases))
    assert undecided <= 4 * 65  # the sweeps and little else


@pytest.mark.parametrize("name", ["edge_sqdis", "edge_s", "edge_res", "edge_thr"])
def test_sweep_flips_once(cases, name):
    import plane_ref as pr
    by = {(c["sheet"], c["i"]): c for c in cases}
    steps = [by[k] for k in pr.sweeps()[name]]
    sel = np.array([c["sel"] for c in steps])
    if name == "edge_thr":
        # the stepped quantity is the fit's largest residual: the reference is the exact fit
        ref = np.array([pr.lstsq(c["pts"])["max_res"] <= float(np.float32(pr.PLANE_THR)) for c in steps], int)
    else:
        ref = np.array([pr.decision(_ref_gates(c)) for c in steps], int)
    print(name, "oracle", "".join(map(str, sel)), "reference", "".join(map(str, ref)))
    assert ref[0] == 1 and ref[-1] == 0 and np.count_nonzero(np.diff(ref)) == 1, ref
    assert sel[0] == 1 and sel[-1] == 0 and np.count_nonzero(np.diff(sel)) == 1, sel
    assert abs(int(np.argmin(sel)) - int(np.argmin(ref))) <= 2
