"""Inline staging of submitted fused batches: a stream group of at
most four scans carries its jobs, poses and control blocks in its launches'
arguments, and each scan's first solve fills the device slot from the slot's
host-mapped staging copy; no copy kernel runs ahead of the group's chain.

One script of batches runs on a context of its own per (max_iterations, staging)
against a 20k-point map: scans of 0, 1, 255, 256, 257 and 513 points (below, at
and above one and two 256-point blocks), a scan a kilometre from the map (no
effective point), and copies of them under ids of their own.  Batches of 1, 3
(ragged groups), 8 and 17 scans (17: groups of 4, 4, 4 and 5, the last beyond
the inline array, staged by the copy kernel beside three inline groups), then
two batches in flight on both lanes three times over, then every scan's
neighbour records (the records launch that runs without a solve).  Every
submitted batch equals the synchronous call of the same context bit for bit,
and the whole script -- states, covariances, every statistic, neighbour indices
and distances -- equals the same script with LIVO_STAGE_COPY=1, bit for bit.
max_iterations 0 stops every scan at its first solve (the staging copy is that
solve's input and the target of its write-back), 1 and 2 keep the first
search's records (the dead-record rule needs 2 and more), 4 is the default.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 255, 256, 257, 513)
LM_KEYS = ("rot", "pos", "vel", "bias_g", "bias_a", "gravity", "cov")
N_SCANS = 20  # 17 in the largest batch, 3 more for the second batch in flight


@pytest.fixture(scope="module")
def data(built):
    from livo_amd import synth
    base = [synth.make_scan(max(n, 1), 900 + i)[0][:n] for i, n in enumerate(SIZES)]
    far = (synth.make_scan(300, 906)[0] + np.float32(1000.0)).astype(np.float32)
    kinds = base + [far]  # index 6: no effective point
    src = [k % len(kinds) for k in range(N_SCANS)]
    return {"map": synth.make_map(20_000), "scans": [kinds[s] for s in src], "src": src,
            "states": [synth.make_state(900 + s) for s in src], "runs": {}}


def _bits(x):
    return np.asarray(x).tobytes()  # (bitwise: an empty scan's statistics hold NaN)


def _flat(states, stats):
    out = []
    for st, ss in zip(states, stats):
        out.append(tuple(_bits(st[k]) for k in LM_KEYS) + tuple(_bits(ss[k]) for k in sorted(ss)))
    return out


def _script(data, max_iter, stage_copy):
    """Every output of the script, in order; submit / wait held to the synchronous call on the way."""
    key = (max_iter, stage_copy)
    if key in data["runs"]:
        return data["runs"][key]
    import livo_amd
    from livo_amd import synth
    mp = pytest.MonkeyPatch()
    if stage_copy:
        mp.setenv("LIVO_STAGE_COPY", "1")
    else:
        mp.delenv("LIVO_STAGE_COPY", raising=False)
    out = []
    try:
        with livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=max_iter) as ctx:
            ctx.map_build(data["map"])
            sids = [ctx.scan_upload(s) for s in data["scans"]]

            def args(sel):
                return [sids[i] for i in sel], [data["states"][i] for i in sel]

            def both(sel):
                ref = _flat(*ctx.iekf_update_batch(*args(sel)))
                t = ctx.iekf_update_batch_submit(*args(sel))
                got = _flat(*ctx.iekf_update_batch_wait(t, len(sel)))
                assert got == ref, (max_iter, stage_copy, sel)
                return got

            for i in range(len(SIZES) + 1):  # batches of 1: every size, and the far scan
                out.append(both([i]))
            out.append(both([5, 3, 0]))  # 3 scans in 3 groups
            out.append(both([0, 1, 2, 3, 4, 5]))  # 6 in 4 groups: 1, 2, 1, 2
            out.append(both(list(range(8))))
            out.append(both(list(range(17))))  # groups of 4, 4, 4, 5: the last by copy kernel
            sync_a = _flat(*ctx.iekf_update_batch(*args(list(range(8)))))
            sync_b = _flat(*ctx.iekf_update_batch(*args([17, 18, 19])))
            for rep in range(3):  # two in flight, both lanes, three times over
                ta = ctx.iekf_update_batch_submit(*args(list(range(8))))
                tb = ctx.iekf_update_batch_submit(*args([17, 18, 19]))
                first, second = (tb, ta) if rep % 2 else (ta, tb)
                res = {}
                for t in (first, second):
                    res[t] = _flat(*ctx.iekf_update_batch_wait(t, 8 if t == ta else 3))
                assert res[ta] == sync_a and res[tb] == sync_b, (max_iter, stage_copy, rep)
                out.append(res[ta] + res[tb])
            # the records after submitted batches (rebuilt on demand where the last search skipped them)
            t = ctx.iekf_update_batch_submit(*args(list(range(17))))
            out.append(_flat(*ctx.iekf_update_batch_wait(t, 17)))
            nn = []
            for i in range(17):
                if len(data["scans"][i]):
                    idx, d = ctx.scan_neighbors(sids[i])
                    nn.append((_bits(idx), _bits(d)))
            out.append(nn)
            # what the script exercised: a scan with effective points, and one with none
            st513 = ctx.iekf_update_batch(*args([5]))[1][0]
            stfar = ctx.iekf_update_batch(*args([6]))[1][0]
            assert st513["effct_feat_num"][0] > 100 and stfar["effct_feat_num"][0] == 0
            assert st513["iterations"] == (max_iter + 1 if max_iter < 2 else st513["iterations"])
    finally:
        mp.undo()
    data["runs"][key] = out
    return out


@pytest.mark.parametrize("max_iter", [0, 1, 2, 4])
def test_inline_staging_equals_copy_staging(data, max_iter):
    inline = _script(data, max_iter, False)
    copied = _script(data, max_iter, True)
    assert len(inline) == len(copied)
    for step, (a, b) in enumerate(zip(inline, copied)):
        assert a == b, (max_iter, step)
