"""CPU: the call surface of the NDT reference-order switch — ``mrgfe_ctx_set_ndt_reference_order`` is declared in include/mrgfe.h beside the other context
switches, bound by the ctypes table and by ``Context.set_ndt_reference_order``, and refuses a NULL context without touching a device.  What the switch does is
held on the GPU (tests/test_gpu_pclndt_reforder.py)."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mrgfe_ctx_set_ndt_reference_order"


def test_null_context_is_refused_with_the_functions_name():
    from mrg_slam_amd import _lib

    for on in (0, 1):
        assert _lib.lib().mrgfe_ctx_set_ndt_reference_order(None, on) == _lib.ERR_INVALID
        assert _lib.last_error().startswith(NAME + ":")


def test_the_binding_exists_and_matches_the_header():
    from mrg_slam_amd import _lib

    pub = open(os.path.join(ROOT, "include", "mrgfe.h")).read()
    assert re.search(r"int\s+mrgfe_ctx_set_ndt_reference_order\(mrgfe_ctx\* ctx, int on\);", pub)
    assert "mrgfe_node_create makes its own" in pub[pub.index("NDT sums in the reference's own order"): pub.index(NAME + "(")]  # nodes are not offered the mode: said there
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and args == [C.c_void_p, C.c_int]
    fn = getattr(_lib.lib(), NAME)
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_int]
    sig = inspect.signature(_lib.Context.set_ndt_reference_order)
    assert list(sig.parameters) == ["self", "on"] and sig.parameters["on"].default is True
    assert NAME in _lib.Context.set_ndt_reference_order.__doc__


def test_the_method_passes_the_contexts_handle_and_the_flag(monkeypatch):
    """Context.set_ndt_reference_order(on) is one call of the entry point with the context's handle and 0 / 1 (no device needed: the library is replaced)."""
    from mrg_slam_amd import _lib

    calls = []

    class FakeLib:
        def mrgfe_ctx_set_ndt_reference_order(self, h, on):
            calls.append((h, on))
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: FakeLib())
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._h = None  # (nothing to destroy)
    handle = object()
    ctx.__dict__["_h"] = handle
    ctx.set_ndt_reference_order()
    ctx.set_ndt_reference_order(False)
    ctx.set_ndt_reference_order(2)
    ctx.__dict__["_h"] = None
    assert calls == [(handle, 1), (handle, 0), (handle, 1)]
