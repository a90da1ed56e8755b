"""GPU: the keyframe callback to its two publishes — ``mrgfe_keyframe_callback_records`` / ``_records_device`` (csrc/filters.hip cloud_pair_records_kernel
directly behind the partition).  The expectation is the existing call on a twin store: its packed ``kept`` / ``removed`` turned into records here with
numpy; every comparison is bit for bit.  Destinations are sentinel-filled with room for 64 records more than the input has points."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = {"x": 0, "y": 4, "z": 8, "intensity": 12}
SIZES = [255, 256, 257, 4097]
CENTRES = [0, 1, 3]
RADIUS = 3.0
SENTINEL = 0xA5
SLACK = 64


def cloud_of(n, seed=0):
    rng = np.random.default_rng(1000 + 7 * n + seed)
    c = rng.normal(0, 4, (n, 4)).astype(np.float32)
    c[:, 3] = rng.uniform(0, 1, n).astype(np.float32)
    c.view(np.uint32)[n // 2, 1] = 0x7FC12345  # a NaN with a payload: kept, bits as they are
    c[n // 3, 0] = np.inf
    return c


def centres_of(k):
    return np.random.default_rng(50 + k).normal(0, 3, (k, 3)).astype(np.float32)


def pack(cloud, step):
    """16: the points; 32: x, y, z, 1.0f, intensity, 0, 0, 0 (the pcl::PointXYZI in memory)"""
    c = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 4).view(np.uint32)
    if step == 16:
        return c.copy().view(np.uint8).reshape(-1)
    r = np.zeros((len(c), 8), dtype=np.uint32)
    r[:, :3] = c[:, :3]
    r[:, 3] = np.float32(1.0).view(np.uint32)
    r[:, 4] = c[:, 3]
    return r.view(np.uint8).reshape(-1)


def message(cloud):
    c = np.ascontiguousarray(cloud, dtype=np.float32)
    return {"data": c.tobytes(), "width": len(c), "height": 1, "point_step": 16, "fields": FIELDS, "row_step": 0}


def sentinel_buffer(ctx, n, step, pinned):
    from mrg_slam_amd._lib import lib

    buf = np.full((n + SLACK) * step, SENTINEL, dtype=np.uint8)
    if pinned:
        assert lib().mrgfe_pin_host_buffer(ctx._h, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 0
    return buf


def release(ctx, buf, pinned):
    from mrg_slam_amd._lib import lib

    if pinned:
        assert lib().mrgfe_unpin_host_buffer(ctx._h, buf.ctypes.data_as(C.c_void_p)) == 0


@pytest.fixture(scope="module")
def ctx():
    from mrg_slam_amd import Context

    return Context()


@pytest.fixture(scope="module")
def twins(ctx):
    """the existing call, once per (size, centres): packed kept / removed, the stored records, the store's byte count"""
    from mrg_slam_amd import MapCloudStore

    out = {}
    for n in SIZES:
        for k in CENTRES:
            store = MapCloudStore(ctx)
            kept, removed = store.keyframe_callback(7, message(cloud_of(n)), centres_of(k), RADIUS)
            out[n, k] = (kept.copy(), removed.copy(), store.read([7])[0].copy(), store.bytes())
    return out


@pytest.mark.parametrize("k", CENTRES)
@pytest.mark.parametrize("n", SIZES)
def test_records_equal_the_packed_outputs_of_the_twin(ctx, twins, n, k):
    import torch

    from mrg_slam_amd import MapCloudStore

    cloud, centres = cloud_of(n), centres_of(k)
    kept, removed, stored, nbytes = twins[n, k]
    assert len(kept) + len(removed) == n and (k == 0) == (len(removed) == 0)
    if k:
        assert 0 < len(removed) < n, (n, k, len(removed))
    dev = torch.from_numpy(cloud).to("cuda:0")
    for step, form, pinned in ((32, "bytes", False), (32, "bytes", True), (16, "bytes", False), (32, "device", False), (16, "device", True)):
        what = (n, k, step, form, pinned)
        store = MapCloudStore(ctx)
        kb, rb = sentinel_buffer(ctx, n, step, pinned), sentinel_buffer(ctx, n, step, pinned)
        try:
            if form == "bytes":
                gk, gr = store.keyframe_callback(9, message(cloud), centres, RADIUS, records=step, kept_out=kb, removed_out=rb)
            else:
                gk, gr = store.keyframe_callback_device(9, dev.data_ptr(), n, centres, RADIUS, want_removed=True, records=step, kept_out=kb, removed_out=rb)
            assert np.array_equal(gk, pack(kept, step)), what
            assert np.array_equal(gr, pack(removed, step)), what
            assert (kb[len(gk):] == SENTINEL).all() and (rb[len(gr):] == SENTINEL).all(), what
            es, e2 = ctx.egress_stats(), ctx.second_egress_stats()
            assert es["direct"] == pinned and es["bytes"] == len(gk) and es["launches"] == 1 and es["waits"] == 1, (what, es)
            assert e2["bytes"] == len(gr) and e2["waits"] == 0 and e2["launches"] == (1 if len(gr) else 0) and (not len(gr) or e2["direct"] == pinned), (what, e2)
            assert np.array_equal(store.read([9])[0], stored) and store.bytes() == nbytes and store.has(9) == len(kept), what
        finally:
            release(ctx, kb, pinned)
            release(ctx, rb, pinned)


@pytest.mark.parametrize("k", [0, 3])
def test_either_sink_may_be_missing(ctx, twins, k):
    from mrg_slam_amd import MapCloudStore

    n = 4097
    cloud, centres = cloud_of(n), centres_of(k)
    kept, removed, stored, nbytes = twins[n, k]
    for want_kept, want_removed in ((True, False), (False, True), (False, False)):
        store = MapCloudStore(ctx)
        gk, gr = store.keyframe_callback(3, message(cloud), centres, RADIUS, want_kept=want_kept, want_removed=want_removed, records=32)
        assert (gk is None) == (not want_kept) and (gr is None) == (not want_removed)
        if want_kept:
            assert np.array_equal(gk, pack(kept, 32))
        if want_removed:
            assert np.array_equal(gr, pack(removed, 32))
        assert np.array_equal(store.read([3])[0], stored) and store.bytes() == nbytes


def raw_call(store, key, cloud, centres, step, kept, kept_cap, removed, removed_cap):
    from mrg_slam_amd import _lib
    from mrg_slam_amd.map_cloud import keyframe_params

    p = keyframe_params(message(cloud), store._ctx)
    buf = np.frombuffer(message(cloud)["data"], dtype=np.uint8)
    fp = C.POINTER(C.c_float)
    nk, nr = C.c_size_t(77), C.c_size_t(77)
    rc = _lib.lib().mrgfe_keyframe_callback_records(store._h, key, C.byref(p), buf.ctypes.data_as(C.c_void_p), buf.nbytes, centres.ctypes.data_as(fp), len(centres),
                                                    float(np.float32(RADIUS * RADIUS)), step, kept.ctypes.data_as(C.c_void_p) if kept is not None else None, kept_cap, C.byref(nk),
                                                    removed.ctypes.data_as(C.c_void_p) if removed is not None else None, removed_cap, C.byref(nr))
    return rc, nk.value, nr.value


def test_refusals_leave_the_store_and_the_buffers_alone(ctx):
    from mrg_slam_amd import MapCloudStore, _lib

    n = 300
    cloud, centres = cloud_of(n), centres_of(3)
    store = MapCloudStore(ctx)
    kb, rb = np.full(n * 32, SENTINEL, dtype=np.uint8), np.full(n * 32, SENTINEL, dtype=np.uint8)
    cases = {"kept capacity short": (32, kb, n * 32 - 1, rb, rb.nbytes), "removed capacity short": (32, kb, kb.nbytes, rb, n * 32 - 1), "point_step 24": (24, kb, kb.nbytes, rb, rb.nbytes)}
    for what, (step, k, kc, r, rc_) in cases.items():
        rc, nk, nr = raw_call(store, 5, cloud, centres, step, k, kc, r, rc_)
        assert rc == _lib.ERR_INVALID and (nk, nr) == (0, 0), (what, rc)
        assert store.has(5) is None and store.bytes() == 0 and (kb == SENTINEL).all() and (rb == SENTINEL).all(), what
    rc, nk, nr = raw_call(store, 5, cloud, centres, 32, kb, kb.nbytes, rb, rb.nbytes)
    assert rc == 0 and nk + nr == n and store.has(5) == nk
    # a duplicate key: MRGFE_ERR_STATE, nothing written
    before = store.bytes()
    kb[:], rb[:] = SENTINEL, SENTINEL
    rc, nk, nr = raw_call(store, 5, cloud, centres, 32, kb, kb.nbytes, rb, rb.nbytes)
    assert rc == _lib.ERR_STATE and (nk, nr) == (0, 0) and store.bytes() == before and (kb == SENTINEL).all() and (rb == SENTINEL).all()
