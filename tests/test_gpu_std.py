"""The loop search on the device (livo_std_*) against the scalar restatement of the reference's
SearchLoop / AddSTDescs (tests/std_cases.py): candidates, votes, match lists, sample votes, success
pairs and scores exactly, rot / t within 8 x the restatement's own measured deviation from a 60-digit
evaluation (std_cases.ROT_TOL, T_TOL).  Databases of at most 64 frames x 40 descriptors."""
import numpy as np
import pytest

import std_cases as S

pytestmark = pytest.mark.gpu
E_INVALID, E_RANGE, E_CAPACITY = -1, -6, -7
NAMES = list(S.cases())
_runs: dict = {}


def _prm(livo_amd, prm):
    return livo_amd.std_params(**prm)


def _load(ctx, case):
    import livo_amd
    nd = sum(len(d) for d, _ in case.frames) + 1
    npl = sum(len(p) for _, p in case.frames) + 1
    ctx.std_reset(_prm(livo_amd, case.prm), nd, len(case.frames), npl)
    for f, (d, p) in enumerate(case.frames):
        ctx.std_stage(d, p)
        assert ctx.std_commit() == f
    ctx.std_stage(case.query, case.query_planes)


def _run(ctx, name):
    """One search of the case on the device, with every stage's record; computed once."""
    if name not in _runs:
        case = S.cases()[name]
        _load(ctx, case)
        res = ctx.std_search()
        cands = ctx.std_candidates()
        _runs[name] = dict(res=res, cands=cands, matches=[ctx.std_matches(k) for k in range(len(cands))],
                           info=ctx.std_info())
    return _runs[name]


def _same_score(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


@pytest.mark.parametrize("name", NAMES)
def test_search_equals_the_restatement(gpu_ctx, name):
    case = S.cases()[name]
    exp = case.expected()
    db = case.db()
    got = _run(gpu_ctx, name)
    res, cands = got["res"], got["cands"]
    assert res["n_candidates"] == len(exp["candidates"]) == len(cands)
    for k, (c, e) in enumerate(zip(cands, exp["candidates"])):
        for f in ("frame", "votes", "use_size", "max_vote", "max_vote_index"):
            assert int(c[f]) == e[f], (name, k, f, int(c[f]), e[f])
        m = got["matches"][k]
        assert list(zip(m["src"].tolist(), m["db_index"].tolist())) == e["matches"], (name, k)
        assert (m["frame"] == e["frame"]).all()
        assert _same_score(float(c["score"]), e["score"]), (name, k, float(c["score"]), e["score"])
        dr = np.abs(c["rot"].reshape(3, 3) - e["rot"]).max()
        dt = np.abs(c["t"] - e["t"]).max()
        print(f"{name} candidate {k}: |rot| dev {dr:.3e} (tol {S.ROT_TOL:.3e})  |t| dev {dt:.3e} (tol {S.T_TOL:.3e})")
        assert dr <= S.ROT_TOL and dt <= S.T_TOL, (name, k, dr, dt)
    assert res["frame"] == exp["frame"] and res["score"] == exp["score"]
    pairs = res["pairs"]
    assert list(zip(pairs["src"].tolist(), pairs["db_index"].tolist())) == exp["pairs"]
    assert res["n_pairs"] == len(exp["pairs"])
    if exp["frame"] < 0:
        assert np.array_equal(res["rot"], np.eye(3)) and np.array_equal(res["t"], np.zeros(3)) and res["candidate"] == -1
    else:
        assert (pairs["frame"] == exp["frame"]).all()
        assert np.abs(res["rot"] - exp["rot"]).max() <= S.ROT_TOL and np.abs(res["t"] - exp["t"]).max() <= S.T_TOL
        assert int(cands[res["candidate"]]["frame"]) == exp["frame"]
    info = got["info"]
    assert info["frames"] == len(case.frames) and info["descs"] == len(db.descs)
    assert info["cells"] == len(db.cells) and info["planes"] == sum(len(p) for p in db.planes)
    assert info["staged_descs"] == len(case.query) and info["staged_planes"] == len(case.query_planes)


def test_two_searches_give_the_same_bytes(gpu_ctx):
    case = S.cases()["skip_len"]
    _load(gpu_ctx, case)
    out = []
    for _ in range(2):
        r = gpu_ctx.std_search()
        c = gpu_ctx.std_candidates()
        out.append((r["frame"], r["score"], r["rot"].tobytes(), r["t"].tobytes(), r["pairs"].tobytes(), c.tobytes(),
                    b"".join(gpu_ctx.std_matches(k).tobytes() for k in range(len(c)))))
    assert out[0] == out[1] and out[0][0] == 4


def test_dump_is_what_was_committed_in_insertion_order(gpu_ctx):
    case = S.cases()["revisit"]
    _load(gpu_ctx, case)
    descs, planes = gpu_ctx.std_dump(frame=10)
    want = np.concatenate([d for d, _ in case.frames])
    assert descs.tobytes() == want.tobytes()
    assert planes.tobytes() == np.ascontiguousarray(case.frames[10][1]).tobytes()
    assert gpu_ctx.std_dump(frame=63)[1].tobytes() == np.ascontiguousarray(case.frames[63][1]).tobytes()
    with pytest.raises(Exception) as e:
        gpu_ctx.std_commit()  # the staged query would be frame 64 of a database made for 64
    assert e.value.code == E_CAPACITY
    assert gpu_ctx.std_info()["frames"] == 64


def test_refusals_come_back_as_codes(gpu_ctx):
    import ctypes as C

    import livo_amd
    L, h = gpu_ctx._L, gpu_ctx.h
    case = S.cases()["votes_4_5"]
    d0, p0 = case.frames[0]
    gpu_ctx.std_reset(_prm(livo_amd, case.prm), 6, 4, 40)
    r, n = livo_amd.StdResult(), C.c_int64()
    assert L.livo_std_search(h, C.byref(r), None, 0, C.byref(n)) == E_INVALID   # nothing staged
    assert L.livo_std_commit(h, None) == E_INVALID
    assert L.livo_std_candidates(h, None, 0, C.byref(n)) == E_INVALID           # no search yet
    wrong = d0.copy()
    wrong["frame_id"][-1] = 1
    gpu_ctx.std_stage(wrong, p0)
    assert L.livo_std_commit(h, None) == E_INVALID                               # a frame_id that is not the index
    gpu_ctx.std_stage(d0, p0)
    assert gpu_ctx.std_commit() == 0
    d1, p1 = case.frames[1]
    gpu_ctx.std_stage(d1, p1)                                                    # 4 + 5 descriptors > 6
    assert L.livo_std_commit(h, None) == E_CAPACITY
    gpu_ctx.std_stage(d1[:2], np.concatenate([p1, p1]))                          # 30 + 60 planes > 40
    assert L.livo_std_commit(h, None) == E_CAPACITY
    info = gpu_ctx.std_info()
    assert (info["frames"], info["descs"], info["planes"]) == (1, 4, len(p0))
    gpu_ctx.std_stage(d1[:2], p1[:3])
    assert gpu_ctx.std_commit() == 1
    assert L.livo_std_matches(h, 0, None, 0, C.byref(n)) == E_INVALID            # a commit drops the last search
    res = gpu_ctx.std_search()                                                   # (the frame stays staged)
    assert res["frame"] == -1 and res["n_candidates"] == 0
    assert L.livo_std_matches(h, 0, None, 0, C.byref(n)) == E_INVALID            # no such candidate
    dd = np.zeros(16, livo_amd.STD_DESC_DTYPE)
    assert L.livo_std_dump(h, dd.ctypes.data_as(C.c_void_p), 3, C.byref(n), -1, None, 0, None) == E_RANGE
    assert L.livo_std_dump(h, None, 0, C.byref(n), 2, None, 0, None) == E_INVALID            # frame 2 is not stored
    p = livo_amd.std_params()
    assert L.livo_std_reset(h, C.byref(p), 8, 20001, 8) == E_RANGE
