"""The batch host path: lane staging, the stored plan and both models on one lane.

Nine scans of 0 .. 2000 points against a 20k-point map.  Batches of 1, 3, 8, 9
and 5 scans on one context, each synchronous and through submit / wait: 9
crosses the staging floor of 8 scans (the lane's area is reallocated), 5 then
reuses the larger area, and 1, 3 and 5 are fewer than, or no multiple of, the
four stream groups.  Then two batches in flight (9 and 3 scans, the later ticket
collected first), and the same with IKFoM batches alternating with LaserMapping
batches on the same lanes (a lane keeps one staging area per model).  Every
batched update equals the scan's single synchronous update bit for bit, on the
fused path (default), the separate passes (LIVO_FUSED=0, synchronous
LaserMapping batches only) and with the slots copied back after the batch
(LIVO_SLOT_WB=0).  The 2000-point scan is also held to the oracle, at
test_gpu_parity's bar for a full update.
"""
import copy

import numpy as np
import pytest

from test_gpu_parity import _iekf_compare

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 257, 500, 1000, 1500, 2000)
BATCHES = (1, 3, 8, 9, 5)
LM_KEYS = ("rot", "pos", "vel", "bias_g", "bias_a", "gravity", "cov")


@pytest.fixture(scope="module")
def data(built):
    import oracle
    from livo_amd import synth
    m = synth.make_map(20_000)
    scans = [synth.make_scan(max(n, 1), 700 + i)[0][:n] for i, n in enumerate(SIZES)]
    return {"map": m, "tree": oracle.Tree(m), "scans": scans,
            "lm": [synth.make_state(700 + i) for i in range(len(SIZES))],
            "ik": [synth.make_ikfom_state(700 + i) for i in range(len(SIZES))]}


def _bits(x):
    return np.asarray(x).tobytes()  # (bitwise: the empty scan's statistics hold NaN)


def _same_lm(got, ref):
    for k in LM_KEYS:
        assert _bits(got[0][k]) == _bits(ref[0][k]), k
    assert got[1]["iterations"] == ref[1]["iterations"]
    assert got[1]["effct_feat_num"] == ref[1]["effct_feat_num"]
    assert _bits(got[1]["solution"]) == _bits(ref[1]["solution"])


def _same_ik(got, ref):
    for k in ref[0]:
        assert _bits(got[0][k]) == _bits(ref[0][k]), k
    assert got[1]["iterations"] == ref[1]["iterations"]
    assert got[1]["effct_feat_num"] == ref[1]["effct_feat_num"]
    assert _bits(got[1]["dx"]) == _bits(ref[1]["dx"])


@pytest.mark.parametrize("mode", ["default", "unfused", "slot_copy"])
def test_batches_equal_single_updates(data, mode, monkeypatch):
    import livo_amd
    from livo_amd import synth
    if mode == "unfused":
        monkeypatch.setenv("LIVO_FUSED", "0")
    if mode == "slot_copy":
        monkeypatch.setenv("LIVO_SLOT_WB", "0")
    submit_lm = mode != "unfused"  # the separate LaserMapping passes run as synchronous batches only
    scans, n = data["scans"], len(SIZES)
    with livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=4) as ctx:
        ctx.map_build(data["map"])
        # scans 0..8, and the first three once more under ids of their own (the second batch in flight)
        sids = [ctx.scan_upload(b) for b in scans] + [ctx.scan_upload(b) for b in scans[:3]]
        src = list(range(n)) + [0, 1, 2]
        ref_lm = [ctx.iekf_update(sids[i], copy.deepcopy(data["lm"][i])) for i in range(n)]
        ref_ik = [ctx.ikfom_update(sids[i], copy.deepcopy(data["ik"][i])) for i in range(n)]
        assert ref_lm[n - 1][1]["effct_feat_num"][0] > 0 and ref_ik[n - 1][1]["effct_feat_num"][0] > 0

        def pick(k):  # 5: the last five, the 2000-point scan among them
            return list(range(n - 5, n)) if k == 5 else list(range(k))

        def check_lm(out, sel):
            for got, i in zip(zip(*out), sel):
                _same_lm(got, ref_lm[src[i]])

        def check_ik(out, sel):
            for got, i in zip(zip(*out), sel):
                _same_ik(got, ref_ik[src[i]])

        def lm_args(sel):
            return [sids[i] for i in sel], [data["lm"][src[i]] for i in sel]

        def ik_args(sel):
            return [sids[i] for i in sel], [data["ik"][src[i]] for i in sel]

        # LaserMapping batches alone
        for k in BATCHES:
            sel = pick(k)
            check_lm(ctx.iekf_update_batch(*lm_args(sel)), sel)
            if submit_lm:
                t = ctx.iekf_update_batch_submit(*lm_args(sel))
                check_lm(ctx.iekf_update_batch_wait(t, k), sel)
        nine, three = list(range(9)), [9, 10, 11]
        if submit_lm:
            ta = ctx.iekf_update_batch_submit(*lm_args(nine))
            tb = ctx.iekf_update_batch_submit(*lm_args(three))
            check_lm(ctx.iekf_update_batch_wait(tb, 3), three)  # the later ticket first
            check_lm(ctx.iekf_update_batch_wait(ta, 9), nine)
        # IKFoM batches, a LaserMapping batch of another size on the same lane between them
        for k, k_lm in zip(BATCHES, (3, 9, 1, 5, 8)):
            sel = pick(k)
            check_ik(ctx.ikfom_update_batch(*ik_args(sel)), sel)
            check_lm(ctx.iekf_update_batch(*lm_args(pick(k_lm))), pick(k_lm))
            t = ctx.ikfom_update_batch_submit(*ik_args(sel))
            check_ik(ctx.ikfom_update_batch_wait(t, k), sel)
            if submit_lm:
                t = ctx.iekf_update_batch_submit(*lm_args(pick(k_lm)))
                check_lm(ctx.iekf_update_batch_wait(t, k_lm), pick(k_lm))
        ta = ctx.ikfom_update_batch_submit(*ik_args(nine))
        if submit_lm:  # one batch of each model in flight
            tb = ctx.iekf_update_batch_submit(*lm_args(three))
            check_lm(ctx.iekf_update_batch_wait(tb, 3), three)
        else:
            tb = ctx.ikfom_update_batch_submit(*ik_args(three))
            check_ik(ctx.ikfom_update_batch_wait(tb, 3), three)
        check_ik(ctx.ikfom_update_batch_wait(ta, 9), nine)
        # the 2000-point scan against the oracle (and its single update once more, after the batches)
        stg = _iekf_compare(ctx, data["tree"], scans[n - 1], data["lm"][n - 1], 4, synth.T_LI)
        assert stg["iterations"] == ref_lm[n - 1][1]["iterations"]
        assert _bits(stg["solution"]) == _bits(ref_lm[n - 1][1]["solution"])
