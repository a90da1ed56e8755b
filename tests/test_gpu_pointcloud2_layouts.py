"""GPU: byte-aligned PointCloud2 layouts (``mrgfe_ctx_set_byte_layouts``) — records whose field offsets or steps are not multiples of 4, as the
Velodyne driver publishes them (22 bytes a point) — through every call that reads the bytes of a message: ``mrgfe_ingest_pointcloud2`` against the host
mirror ``io.xyzi_from_pointcloud2``, and ``mrgfe_scan_callback[_device]``, ``mrgfe_keyframe_callback``, ``mrgfe_map_store_add_keyframes`` and
``mrgfe_odom_frame`` against the same call on the message repacked to the packed 16-byte layout.  Every comparison is of bytes: the clouds carry a NaN
with a payload, a signalling NaN, +-inf and denormals, and the filler fields of the records are random."""
import ctypes as C

import numpy as np
import pytest

from conftest import small_cloud

pytestmark = pytest.mark.gpu

U8, U16, F32, F64 = 2, 4, 7, 8  # sensor_msgs/PointField datatypes
XYZI = [("x", 0, F32, 1), ("y", 4, F32, 1), ("z", 8, F32, 1), ("intensity", 12, F32, 1)]
# name -> (field list, point_step, numpy record)
LAYOUTS = {
    "V22": (XYZI + [("ring", 16, U16, 1), ("time", 18, F32, 1)], 22,
            {"names": ["x", "y", "z", "intensity", "ring", "time"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u2", "<f4"], "offsets": [0, 4, 8, 12, 16, 18], "itemsize": 22}),
    "H26": (XYZI + [("ring", 16, U16, 1), ("timestamp", 18, F64, 1)], 26,
            {"names": ["x", "y", "z", "intensity", "ring", "timestamp"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u2", "<f8"], "offsets": [0, 4, 8, 12, 16, 18], "itemsize": 26}),
    "L19": ([("tag", 0, U8, 1), ("x", 1, F32, 1), ("y", 5, F32, 1), ("z", 9, F32, 1), ("intensity", 13, F32, 1), ("line", 17, U16, 1)], 19,  # odd: all four residues occur
            {"names": ["tag", "x", "y", "z", "intensity", "line"], "formats": ["u1", "<f4", "<f4", "<f4", "<f4", "<u2"], "offsets": [0, 1, 5, 9, 13, 17], "itemsize": 19}),
    "N13": (XYZI[:3] + [("tag", 12, U8, 1)], 13,  # no intensity
            {"names": ["x", "y", "z", "tag"], "formats": ["<f4", "<f4", "<f4", "u1"], "offsets": [0, 4, 8, 12], "itemsize": 13}),
}
NAMES = ["V22", "H26", "L19", "N13", "V22x2"]  # V22x2: organised, height 2, row_step = width * 22 + 3
COUNTS = [1, 255, 256, 257, 2049]  # the edges of a workgroup and of the 2048-point tile
N_PIPE = 3001
SPECIAL = np.array([0x7FC12345, 0x7F812345, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x80000000], dtype=np.uint32)  # NaNs with payloads, +-inf, denormals, -0
ANG_V = np.array([0.3, -0.2, 0.9], dtype=np.float32)
PERIOD = 0.1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b, what=""):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(bits(a), bits(b)), what


def cloud_of(n, seed=0, coords=True):
    """``small_cloud`` with the special bit patterns written in: into the intensity, and (``coords``) into x, y and z as well."""
    c = small_cloud(max(n, 8), seed=40 + seed)[:n].copy()
    u = c.view(np.uint32)
    for k, s in enumerate(SPECIAL):
        if k < n:
            u[(k * 37) % n, 3] = s
        if coords and n > 16:
            u[(5 + k * 53) % n, k % 3] = s
    return c


def message(cloud, name, seed=0):
    """The cloud as a PointCloud2 of one of the layouts: (message with ``fields`` as the driver's list, ``{name: offset}`` dict of its FLOAT32 fields)."""
    organised = name == "V22x2"
    fields, step, rec = LAYOUTS["V22" if organised else name]
    n = len(cloud)
    h = 2 if organised else 1
    assert n % h == 0
    w = n // h
    row_step = w * step + (3 if organised else 0)
    raw_bytes = (h - 1) * row_step + w * step
    rng = np.random.default_rng(77 + 13 * n + seed)
    data = rng.integers(0, 256, raw_bytes, dtype=np.uint8)  # every byte the message does not describe, and every filler field, is random
    for r in range(h):
        rows = data[r * row_step: r * row_step + w * step].view(np.dtype(rec))
        part = cloud[r * w: (r + 1) * w]
        for k, f in enumerate(("x", "y", "z", "intensity")):
            if f in rows.dtype.names:
                rows[f] = part[:, k]  # (float32 to float32: the bits as they are)
    offs = {f[0]: f[1] for f in fields if f[0] in ("x", "y", "z", "intensity")}
    return {"data": data.tobytes(), "width": w, "height": h, "point_step": step, "row_step": row_step if organised else 0, "fields": list(fields)}, offs


def host_mirror(msg, offs):
    """``io.xyzi_from_pointcloud2``, row by row for an organised message (the mirror takes contiguous records)."""
    from mrg_slam_amd import io

    w, h, step = msg["width"], msg["height"], msg["point_step"]
    rs = msg["row_step"] or w * step
    return np.concatenate([io.xyzi_from_pointcloud2(msg["data"][r * rs: r * rs + w * step], w, 1, step, offs) for r in range(h)])


def repacked(cloud):
    c = np.ascontiguousarray(cloud, dtype=np.float32)
    return {"data": c.tobytes(), "width": len(c), "height": 1, "point_step": 16, "row_step": 0, "fields": {"x": 0, "y": 4, "z": 8, "intensity": 12}}


def with_dict(msg, offs):
    """The same message with ``fields`` as a ``{name: offset}`` dict: the wrappers switch nothing for it."""
    return dict(msg, fields=dict(offs))


def n_points(name, n):
    return 2 * n if name == "V22x2" else n


@pytest.fixture(scope="module")
def ctx_on():
    from mrg_slam_amd import Context

    c = Context()
    c.set_byte_layouts(True)
    return c


@pytest.fixture(scope="module")
def pipe():
    """One message per layout for the pipeline calls (about 3000 points), with the cloud it stands for."""
    out = {}
    for k, name in enumerate(NAMES):
        n = N_PIPE + (1 if name == "V22x2" else 0)
        msg, offs = message(cloud_of(n, seed=k), name, seed=k)
        out[name] = (msg, offs, host_mirror(msg, offs))
    return out


def test_some_payload_ends_at_every_residue():
    ends = set()
    for name in NAMES:
        for n in COUNTS:
            m = n_points(name, n)
            msg, _ = message(np.zeros((m, 4), np.float32), name)
            ends.add(len(msg["data"]) % 4)
    assert ends == {0, 1, 2, 3}


@pytest.mark.parametrize("name", NAMES)
def test_ingest_equals_the_host_mirror(name, ctx_on):
    import torch

    from mrg_slam_amd import io

    for n in COUNTS:
        m = n_points(name, n)
        cloud = cloud_of(m, seed=n)
        msg, offs = message(cloud, name, seed=n)
        want = host_mirror(msg, offs)
        if "intensity" not in offs:
            cloud[:, 3] = 0.0
        same(want, cloud, (name, n, "the mirror"))
        got = io.ingest_pointcloud2(msg["data"], msg["width"], msg["height"], msg["point_step"], msg["fields"], msg["row_step"], ctx=ctx_on)
        same(got, want, (name, n, "host output"))
        d = torch.full((m, 4), -1.0, dtype=torch.float32, device="cuda:0")
        assert io.ingest_pointcloud2(msg["data"], msg["width"], msg["height"], msg["point_step"], with_dict(msg, offs)["fields"], msg["row_step"], ctx=ctx_on, dev_ptr=d.data_ptr()) is None
        same(d.cpu().numpy(), want, (name, n, "device output"))


@pytest.mark.parametrize("name", NAMES)
def test_scan_callback_equals_the_repacked_message(name, ctx_on, pipe):
    import torch

    from mrg_slam_amd import scan_callback, scan_callback_to_device, synth

    msg, _, cloud = pipe[name]
    T = synth.make_pose([0.3, -0.1, 0.45], synth.rot_xyz(0.01, -0.02, 1.2)).astype(np.float32)
    ref = repacked(cloud)
    for ang_v, Tm in ((ANG_V, T), (None, None)):
        out = []
        for m in (msg, ref):
            host = scan_callback(m["data"], m["width"], m["height"], m["point_step"], m["fields"], m["row_step"], ang_v, PERIOD, Tm, None, ctx=ctx_on)
            n = m["width"] * m["height"]
            buf = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
            k = scan_callback_to_device(m["data"], m["width"], m["height"], m["point_step"], m["fields"], buf.data_ptr(), n, m["row_step"], ang_v, PERIOD, Tm, None, ctx=ctx_on)
            out.append((host, buf[:k].cpu().numpy()))
        print(f"scan_callback {name}: {len(cloud)} -> {len(out[0][0])} points")
        assert 100 < len(out[1][0]) < len(cloud)  # the default filters did something
        same(out[0][0], out[1][0], (name, "host"))
        same(out[0][1], out[1][1], (name, "device"))
        same(out[0][0], out[0][1], (name, "host against device"))


@pytest.mark.parametrize("name", NAMES)
def test_keyframe_callback_equals_the_repacked_message(name, ctx_on, pipe):
    from mrg_slam_amd import MapCloudStore

    msg, _, cloud = pipe[name]
    ref = repacked(cloud)
    centres = cloud[[100, 1500], :3] + np.float32(0.25)
    store = MapCloudStore(ctx_on)
    for key, ctr in ((1, None), (3, centres)):
        before = store.bytes()
        kept, removed = store.keyframe_callback(key, msg, ctr, 2.0)
        assert store.bytes() - before == 16 * store.has(key)
        kept_r, removed_r = store.keyframe_callback(key + 1, ref, ctr, 2.0)
        if ctr is None:
            assert store.has(key) == store.has(key + 1) == len(cloud) and len(removed) == len(removed_r) == 0
        else:
            assert store.has(key) == len(kept) == len(kept_r) and len(removed) == len(removed_r) and len(kept) + len(removed) == len(cloud)
            assert len(removed) > 10 and len(kept) > 1000
        same(kept, kept_r, (name, "kept"))
        same(removed, removed_r, (name, "removed"))
        # what the store holds, read back through map generation without a voxel filter or distance cut (identity pose)
        same(store.generate([key], [np.eye(4)], None, 0.0, distance_far_thresh=0.0), store.generate([key + 1], [np.eye(4)], None, 0.0, distance_far_thresh=0.0), (name, "stored"))


def test_add_keyframes_takes_three_layouts_in_one_call(ctx_on):
    from mrg_slam_amd import MapCloudStore

    clouds = [cloud_of(2049, 1, coords=False), cloud_of(1, 2, coords=False), cloud_of(257, 3, coords=False)]  # (the identity pose is a multiplication: finite coordinates)
    v22, _ = message(clouds[0], "V22", 1)
    l19, _ = message(clouds[2], "L19", 3)
    store = MapCloudStore(ctx_on)
    added = store.add_keyframes([(11, v22), (12, repacked(clouds[1])), (13, l19)])
    assert list(added) == [1, 1, 1] and store.bytes() == 16 * (2049 + 1 + 257)
    eye = [np.eye(4)] * 3
    got = store.generate([11, 12, 13], eye, None, 0.0, distance_far_thresh=0.0)
    same(got, np.concatenate(clouds), "the three clouds")
    for key, c in zip((11, 12, 13), clouds):
        same(store.generate([key], eye[:1], None, -1.0, distance_far_thresh=0.0), c, key)
    # a strict-only call on the same store still launches the strict gather
    assert list(store.add_keyframes([(21, repacked(clouds[2])), (11, v22)])) == [1, 0]
    same(store.generate([21], eye[:1], None, 0.0, distance_far_thresh=0.0), clouds[2])


def test_odom_frame_equals_the_repacked_frames(ctx_on):
    from mrg_slam_amd import Context, HipOdometry, SmallGicpHip, synth

    a = cloud_of(N_PIPE, 5, coords=False)
    move = synth.make_pose([0.4, -0.1, 0.02], synth.rot_xyz(0.002, -0.003, 0.02)).astype(np.float32)
    b = a.copy()
    b[:, :3] = a[:, :3] @ move[:3, :3].T + move[:3, 3]
    records = []
    for ctx, as_v22 in ((ctx_on, True), (Context(), False)):
        odo = HipOdometry(SmallGicpHip(transformation_epsilon=0.01, ctx=ctx))
        rows = []
        for k, c in enumerate((a, b)):
            msg = message(c, "V22", k)[0] if as_v22 else repacked(c)
            r = odo.frame(msg, 100.0 + 0.1 * k, None, want_status=True, want_aligned=True)
            rows.append((r.outcome, bytes(r.raw), None if r.aligned is None else r.aligned.copy()))
        records.append(rows)
        odo.close()
    assert [r[0] for r in records[0]] == ["first_frame", "accepted"]
    for (o1, raw1, al1), (o2, raw2, al2) in zip(*records):
        assert o1 == o2 and raw1 == raw2
        assert (al1 is None) == (al2 is None)
        if al1 is not None:
            same(al1, al2, "aligned")


def test_a_strict_layout_gives_the_same_bytes_with_the_switch_on_and_off(ctx_on):
    from mrg_slam_amd import Context, MapCloudStore, io, scan_callback

    cloud = cloud_of(N_PIPE, 9)
    rec = np.random.default_rng(3).integers(0, 256, (len(cloud), 24), dtype=np.uint8)  # 24-byte records: a leading stamp word, a trailing tag word
    rec[:, 4:20] = cloud.view(np.uint8).reshape(len(cloud), 16)
    msg = {"data": rec.tobytes(), "width": len(cloud), "height": 1, "point_step": 24, "row_step": 0, "fields": {"x": 4, "y": 8, "z": 12, "intensity": 16}}
    outs = []
    for ctx in (ctx_on, Context()):
        store = MapCloudStore(ctx)
        kept, removed = store.keyframe_callback(1, msg, cloud[[7, 2000], :3], 2.0)
        store.add_keyframes([(2, msg)])
        outs.append((io.ingest_pointcloud2(msg["data"], msg["width"], 1, 24, msg["fields"], ctx=ctx),
                     scan_callback(msg["data"], msg["width"], 1, 24, msg["fields"], 0, ANG_V, PERIOD, None, None, ctx=ctx), kept, removed,
                     store.generate([2], [np.eye(4)], None, 0.0, distance_far_thresh=0.0)))
    same(outs[0][0], cloud)
    for g, w in zip(*outs):
        same(g, w)


def test_the_switch(pipe):
    """Off by default; the refusal is MRGFE_ERR_INVALID and names the entry point; on, off again; a registration and a store made on the context follow it."""
    import torch

    from mrg_slam_amd import Context, HipOdometry, IcpHip, MapCloudStore, MrgfeError, _lib, io, scan_callback, scan_callback_to_device

    ctx = Context()
    store = MapCloudStore(ctx)
    odo = HipOdometry(IcpHip(ctx=ctx))
    dev = torch.empty((N_PIPE + 1, 4), dtype=torch.float32, device="cuda:0")
    key = [100]

    def calls(m):
        key[0] += 2
        args = (m["data"], m["width"], m["height"], m["point_step"], m["fields"])
        return [("mrgfe_ingest_pointcloud2", lambda: io.ingest_pointcloud2(*args, m["row_step"], ctx=ctx)),
                ("mrgfe_scan_callback", lambda: scan_callback(*args, m["row_step"], ctx=ctx)),
                ("mrgfe_scan_callback_device", lambda: scan_callback_to_device(*args, dev.data_ptr(), len(dev), m["row_step"], ctx=ctx)),
                ("mrgfe_keyframe_callback", lambda k=key[0]: store.keyframe_callback(k, m)),
                ("mrgfe_map_store_add_keyframes", lambda k=key[0] + 1: store.add_keyframes([(k, m)])),
                ("mrgfe_odom_frame", lambda: odo.frame(m, 1.0))]

    def refused(m, what):
        state = store.bytes()
        for fn, call in calls(m):
            try:
                call()
            except MrgfeError as ex:
                assert ex.status == _lib.ERR_INVALID and _lib.last_error().startswith(fn + ":"), (what, fn, str(ex))
            else:
                raise AssertionError(f"{what}: {fn} took the layout")
        assert store.bytes() == state

    def accepted(m):
        for _, call in calls(m):
            call()
        odo.reset()

    msgs = {name: with_dict(pipe[name][0], pipe[name][1]) for name in NAMES}  # dicts: the wrappers switch nothing themselves
    for name, m in msgs.items():
        refused(m, f"{name} on a fresh context")
    ctx.set_byte_layouts(True)
    for m in msgs.values():
        accepted(m)
    ctx.set_byte_layouts(False)
    for name, m in msgs.items():
        refused(m, f"{name} after the switch went off")
    # the driver's field list switches the context on by itself, through any wrapper
    lst = pipe["V22"][0]
    got = io.ingest_pointcloud2(lst["data"], lst["width"], lst["height"], lst["point_step"], lst["fields"], lst["row_step"], ctx=ctx)
    same(got, pipe["V22"][2])
    accepted(msgs["L19"])
    odo.close()
