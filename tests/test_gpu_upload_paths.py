"""The three scan-upload entry points where they share state (livo_capi.cpp,
UploadDev): the pinned ring wrapping and the scratch growing with uploads in
flight, the single and the batched asynchronous upload interleaved on one
stream and scratch, strided input, and batches of empty scans.

Every scan is checked against livo_scan_upload of the same points in the same
context: one IEKF update from the same state and the neighbour records it
leaves, bit for bit.  Small map (30k points), two iterations: the checks are
about how a scan is stored, which the first search and solve already expose.
"""
import numpy as np
import pytest

from test_gpu_bench_mode import _same_update

pytestmark = pytest.mark.gpu

PIN_RING = 16  # kPinRing (livo_capi.cpp)
SEG_MAX = 16   # kFeSegMax (livo_internal.h): scans per pass of the batched upload


@pytest.fixture(scope="module")
def world(built):
    """The map, a pool of scan points (one synthetic scan; the tests' scans are random subsets of it) and the
    state every update starts from (that scan's)."""
    from livo_amd import synth
    return synth.cached_map(30_000), synth.make_scan(20_000, 900)[0][:, :3].copy(), synth.make_state(900)


def _context():
    import livo_amd
    from livo_amd import synth
    return livo_amd.Context(0, t_LI=synth.T_LI, max_iterations=2)


def _scans(pool, sizes, seed):
    """One (n, 3) float32 array per size: n distinct points of the pool (page-aligned, so each can be page-locked)."""
    import livo_amd
    rng = np.random.default_rng(seed)
    return [livo_amd.page_aligned_copy(pool[rng.choice(len(pool), n, replace=False)]) if n > 0
            else np.zeros((0, 3), np.float32) for n in sizes]


def _update(ctx, sid, state):
    out = ctx.iekf_update(sid, state)
    return out, ctx.scan_neighbors(sid)


def _reference(ctx, pts, state):
    sid = ctx.scan_upload(pts)
    ref = _update(ctx, sid, state)
    ctx.scan_release(sid)
    # (the comparison is about something: the update found planes for some of the scan's points)
    assert len(pts) < 64 or (ref[0][1]["iterations"] >= 1 and ref[0][1]["effct_feat_num"][0] > 0)
    return ref


def _same(ctx, sid, state, ref):
    (out, (idx, d)), (ref_out, (ref_idx, ref_d)) = _update(ctx, sid, state), ref
    _same_update(out, ref_out)
    assert np.array_equal(idx, ref_idx) and np.array_equal(d.view(np.uint32), ref_d.view(np.uint32))


def test_ring_wrap_and_scratch_growth_in_flight(world):
    """2 * kPinRing + 1 livo_scan_upload_async calls back to back, 64 to ~4000 points, a larger size every
    third call: every pinned slot is taken again (the last one a third time) and grown, and the build
    scratch grows eleven times, each time with earlier uploads still queued on the upload stream."""
    m, pool, state = world
    sizes = [64 + 394 * (k // 3) for k in range(2 * PIN_RING + 1)]
    assert sizes[-1] == 4004 and len(set(sizes)) == 11
    scans = _scans(pool, sizes, 1)
    with _context() as ctx:
        ctx.map_build(m)
        ref = [_reference(ctx, x, state) for x in scans]
        ids = [ctx.scan_upload_async(x) for x in scans]  # (no wait in between)
        assert len(set(ids)) == len(ids)
        for sid, r in zip(ids, ref):
            _same(ctx, sid, state, r)


@pytest.mark.parametrize("pinned", [False, True])
def test_single_and_batch_uploads_interleaved(world, pinned):
    """livo_scan_upload_async (one scan) alternating with livo_scan_upload_batch_async of 17 scans (two passes;
    an empty scan, one of 1 point, one of 257) on the shared upload stream and scratch, from pageable arrays
    (pinned ring) and from page-locked ones (read in place).  Three rounds with nothing released, every
    non-empty scan checked; then all released and one more round, built in the spare pool's buffers."""
    m, pool, state = world
    single_n = 1500
    sizes = [900, 1, 2000, 0, 257, 3100, 5, 1234] + [300 + 170 * s for s in range(9)]
    assert len(sizes) == SEG_MAX + 1
    scans = _scans(pool, [single_n] + sizes, 2)
    with _context() as ctx:
        ctx.map_build(m)
        ref = [_reference(ctx, x, state) if len(x) else None for x in scans]
        if pinned:
            for x in scans:
                if x.nbytes:
                    ctx.host_register(x)

        def one_round():
            return [ctx.scan_upload_async(scans[0])] + ctx.scan_upload_batch_async(scans[1:])

        rounds = [one_round() for _ in range(3)]
        ids = [sid for r in rounds for sid in r]
        assert len(set(ids)) == len(ids)
        for r in rounds:
            for sid, rf in zip(r, ref):
                if rf is not None:
                    _same(ctx, sid, state, rf)
        for sid in ids:
            ctx.scan_release(sid)
        again = one_round()
        assert len(set(again)) == len(again)
        for sid, rf in zip(again, ref):
            if rf is not None:
                _same(ctx, sid, state, rf)
        ctx.sync()
        if pinned:
            for x in scans:
                if x.nbytes:
                    ctx.host_unregister(x)


def test_strided_input(world):
    """(N, 5) float32 arrays (a 20-byte stride; the two extra columns hold values that must not be read as
    coordinates) through livo_scan_upload, livo_scan_upload_async and livo_scan_upload_batch_async: each
    stores what livo_scan_upload stores of the packed (N, 3) copy.  Sizes around one block of 256."""
    m, pool, state = world
    sizes = [1, 255, 256, 257, 3000]
    packed = _scans(pool, sizes, 3)
    wide = [np.ascontiguousarray(np.concatenate([x, np.full((len(x), 2), 1e6, np.float32)], axis=1)) for x in packed]
    assert all(w.strides == (20, 4) for w in wide)
    with _context() as ctx:
        ctx.map_build(m)
        ref = [_reference(ctx, x, state) for x in packed]
        ids = {"sync": [ctx.scan_upload(w) for w in wide], "async": [ctx.scan_upload_async(w) for w in wide],
               "batch": ctx.scan_upload_batch_async(wide)}
        for name, got in ids.items():
            assert len(got) == len(sizes), name
            for sid, r in zip(got, ref):
                _same(ctx, sid, state, r)


def test_batches_of_empty_scans(world):
    """A batch of empty scans only, and a batch whose first pass (16 scans) is all empty and whose second is
    not: every scan gets an id of its own and can be released, and the two non-empty scans are stored as
    livo_scan_upload stores them."""
    m, pool, state = world
    live = _scans(pool, [700, 257], 4)
    empty = np.zeros((0, 3), np.float32)
    with _context() as ctx:
        ctx.map_build(m)
        ref = [_reference(ctx, x, state) for x in live]
        a = ctx.scan_upload_batch_async([empty] * 3)
        b = ctx.scan_upload_batch_async([empty] * SEG_MAX + live)
        assert len(a) == 3 and len(b) == SEG_MAX + 2
        assert len(set(a + b)) == len(a) + len(b)
        for sid, r in zip(b[SEG_MAX:], ref):
            _same(ctx, sid, state, r)
        for sid in a + b:
            ctx.scan_release(sid)
        assert not ctx.scans
