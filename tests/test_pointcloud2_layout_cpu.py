"""CPU: ``mrgfe_pointcloud2_layout`` — the layout arguments of the calls that read PointCloud2 bytes, found in the message's field list by the
matching rule of ``pcl::fromROSMsg`` (the first field with the name, datatype FLOAT32 and count 1), held against a table of field lists."""
import ctypes as C

import pytest

I8, U8, I16, U16, I32, U32, F32, F64 = 1, 2, 3, 4, 5, 6, 7, 8  # sensor_msgs/PointField datatypes

XYZI = [("x", 0, F32, 1), ("y", 4, F32, 1), ("z", 8, F32, 1), ("intensity", 12, F32, 1)]
V22 = XYZI + [("ring", 16, U16, 1), ("time", 18, F32, 1)]
H26 = XYZI + [("ring", 16, U16, 1), ("timestamp", 18, F64, 1)]

# (name, fields, point_step, (off_x, off_y, off_z, off_intensity), needs_byte_layouts)
TABLE = [
    ("velodyne 22", V22, 22, (0, 4, 8, 12), 1),
    ("26 bytes, FLOAT64 stamp", H26, 26, (0, 4, 8, 12), 1),
    ("intensity UINT8", XYZI[:3] + [("intensity", 12, U8, 1)], 16, (0, 4, 8, -1), 0),
    ("intensity UINT16", XYZI[:3] + [("intensity", 12, U16, 1), ("ring", 14, U16, 1)], 16, (0, 4, 8, -1), 0),
    ("intensity count 2", XYZI[:3] + [("intensity", 12, F32, 2)], 20, (0, 4, 8, -1), 0),
    ("no intensity", XYZI[:3] + [("tag", 12, U8, 1)], 13, (0, 4, 8, -1), 1),
    ("leading byte", [("tag", 0, U8, 1), ("x", 1, F32, 1), ("y", 5, F32, 1), ("z", 9, F32, 1), ("intensity", 13, F32, 1)], 19, (1, 5, 9, 13), 1),
    ("duplicate name: the first match wins", XYZI + [("x", 16, F32, 1), ("intensity", 20, F32, 1)], 24, (0, 4, 8, 12), 0),
    ("duplicate name: a non-matching first is passed over", [("intensity", 12, U8, 1)] + XYZI[:3] + [("intensity", 16, F32, 1)], 20, (0, 4, 8, 16), 0),
    ("strict: packed 16", XYZI, 16, (0, 4, 8, 12), 0),
    ("strict: pcl 32", XYZI[:3] + [("intensity", 16, F32, 1)], 32, (0, 4, 8, 16), 0),
    ("strict offsets in an odd step", XYZI, 18, (0, 4, 8, 12), 1),
]


def call(fields, width, height, point_step, row_step=0, bigendian=0):
    from mrg_slam_amd import _lib

    arr = (_lib.PointField * max(len(fields), 1))()
    for a, (name, off, dt, cnt) in zip(arr, fields):
        a.name, a.offset, a.datatype, a.count = name.encode(), off, dt, cnt
    lay, needs = _lib.KeyframeParams(), C.c_int(-1)
    st = _lib.lib().mrgfe_pointcloud2_layout(arr, len(fields), width, height, point_step, row_step, bigendian, C.byref(lay), C.byref(needs))
    return st, lay, needs.value, _lib.last_error()


@pytest.mark.parametrize("name,fields,step,offs,needs", TABLE, ids=[t[0] for t in TABLE])
def test_the_table_of_field_lists(name, fields, step, offs, needs):
    st, lay, got_needs, err = call(fields, 100, 1, step)
    assert st == 0, err
    assert (lay.off_x, lay.off_y, lay.off_z, lay.off_intensity) == offs
    assert (lay.width, lay.height, lay.point_step, lay.row_step) == (100, 1, step, 0)  # copied as they are (row_step 0: the entry point fills it in)
    assert got_needs == needs


def test_the_struct_mirror_and_the_size_function():
    from mrg_slam_amd import _lib

    assert _lib.lib().mrgfe_pointcloud2_field_size() == C.sizeof(_lib.PointField) == 24
    # the first eight members of mrgfe_scan_params are a mrgfe_keyframe_params (include/mrgfe.h): a layout is copied over the head of one
    head = [(n, t) for n, t in _lib.ScanParams._fields_[:8]]
    assert head == list(_lib.KeyframeParams._fields_)
    assert all(getattr(_lib.ScanParams, n).offset == getattr(_lib.KeyframeParams, n).offset for n, _ in head)


@pytest.mark.parametrize("axis", ["x", "y", "z"])
def test_a_coordinate_without_a_match_is_an_error_that_names_it(axis):
    from mrg_slam_amd import _lib

    for bad in (F64, U32, I32):  # FLOAT64, or an integer of the same size: PCL maps neither
        fields = [(n, o, bad if n == axis else t, c) for n, o, t, c in V22]
        st, _, needs, err = call(fields, 10, 1, 22)
        assert st == _lib.ERR_INVALID and err.startswith("mrgfe_pointcloud2_layout:") and f"'{axis}'" in err and needs == 0
    st, _, _, err = call([f for f in V22 if f[0] != axis], 10, 1, 22)  # no such field at all
    assert st == _lib.ERR_INVALID and f"'{axis}'" in err
    st, _, _, err = call([(n, o, t, 3 if n == axis else c) for n, o, t, c in V22], 10, 1, 22)  # count 3
    assert st == _lib.ERR_INVALID and f"'{axis}'" in err


def test_refusals():
    from mrg_slam_amd import _lib

    st, _, _, err = call(V22, 10, 1, 22, bigendian=1)
    assert st == _lib.ERR_INVALID and "big-endian" in err
    st, lay, _, _ = call(V22, 10, 2, 15, row_step=100)  # fields outside the record, rows shorter than their points: the entry point's to refuse
    assert st == 0 and (lay.point_step, lay.row_step, lay.off_intensity) == (15, 100, 12)
    L = _lib.lib()
    assert L.mrgfe_pointcloud2_layout(None, 3, 1, 1, 16, 0, 0, C.byref(_lib.KeyframeParams()), None) == _lib.ERR_INVALID
    assert L.mrgfe_pointcloud2_layout(None, 0, 1, 1, 16, 0, 0, None, None) == _lib.ERR_INVALID
    assert L.mrgfe_ctx_set_byte_layouts(None, 1) == _lib.ERR_INVALID and _lib.last_error().startswith("mrgfe_ctx_set_byte_layouts:")


def test_row_step_and_organised_clouds():
    st, lay, needs, err = call(V22, 50, 2, 22, row_step=50 * 22 + 3)
    assert st == 0 and lay.row_step == 1103 and needs == 1, err
    st, lay, needs, err = call(XYZI, 50, 2, 16, row_step=50 * 16 + 3)  # a strict record in a row that is not a multiple of 4
    assert st == 0 and needs == 1, err
    st, lay, needs, err = call(XYZI, 50, 2, 16, row_step=50 * 16 + 48)
    assert st == 0 and needs == 0, err
    st, lay, needs, err = call(XYZI, 3, 1, 16)
    assert st == 0 and needs == 0
    from mrg_slam_amd import _lib  # needs_byte_layouts may also be NULL:

    arr = (_lib.PointField * 4)()
    for a, (name, off, dt, cnt) in zip(arr, XYZI):
        a.name, a.offset, a.datatype, a.count = name.encode(), off, dt, cnt
    assert _lib.lib().mrgfe_pointcloud2_layout(arr, 4, 3, 1, 16, 0, 0, C.byref(lay), None) == 0


def test_layout_from_fields_takes_both_forms():
    """``io.layout_from_fields``: a ``{name: offset}`` dict is taken as FLOAT32 fields; a list carries datatype and count; both go through the C helper."""
    from mrg_slam_amd import MrgfeError, _lib, io

    class Ctx:  # stands for a Context: records the switch
        on = None

        def set_byte_layouts(self, on=True):
            self.on = on

    lay, needs = io.layout_from_fields({"x": 0, "y": 4, "z": 8, "intensity": 12}, 7, 1, 22)
    assert (lay.off_x, lay.off_y, lay.off_z, lay.off_intensity, lay.point_step, lay.width, needs) == (0, 4, 8, 12, 22, 7, True)
    lay, needs = io.layout_from_fields({"x": 4, "y": 8, "z": 12}, 7, 1, 20)
    assert (lay.off_x, lay.off_intensity, needs) == (4, -1, False)
    for none in (None, -1):  # the two ways the wrappers' callers have said "no intensity field"
        lay, needs = io.layout_from_fields({"x": 0, "y": 4, "z": 8, "intensity": none}, 7, 1, 12)
        assert (lay.off_z, lay.off_intensity, needs) == (8, -1, False)
    c = Ctx()
    lay, needs = io.layout_from_fields(V22, 7, 1, 22, ctx=c)
    assert needs and c.on is True and lay.off_intensity == 12
    c = Ctx()
    io.layout_from_fields(XYZI, 7, 1, 16, ctx=c)  # a strict layout switches nothing
    assert c.on is None
    c = Ctx()
    io.layout_from_fields({"x": 0, "y": 4, "z": 8}, 7, 1, 22, ctx=c)  # a dict is the caller's claim: it switches nothing either
    assert c.on is None

    class Field:  # an object with the attributes of sensor_msgs/PointField
        def __init__(self, name, offset, datatype, count):
            self.name, self.offset, self.datatype, self.count = name, offset, datatype, count

    lay, needs = io.layout_from_fields([Field(*f) for f in XYZI[:3] + [("intensity", 12, U8, 1)]], 7, 1, 13)
    assert (lay.off_intensity, needs) == (-1, True)
    with pytest.raises(MrgfeError) as e:
        io.layout_from_fields([("x", 0, F64, 1), ("y", 8, F32, 1), ("z", 12, F32, 1)], 7, 1, 16)
    assert e.value.status == _lib.ERR_INVALID and "'x'" in str(e.value)
    with pytest.raises(MrgfeError):
        io.layout_from_fields(XYZI, 7, 1, 16, is_bigendian=True)
