"""diag_lib.diag_library() on a stand-in library (no GPU, no shared object): what it swaps in, that it
puts everything back also after a body that raises, that it refuses to nest, and that nat.call inside it
reaches the swapped-in library."""
import pytest

import diag_lib
from lidar_ai_recommendation_software_amd import _native as nat


class StandIn:
    """Records the calls it gets; every entry point returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("lidar_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return b"" if name == "lidar_last_error" else 0
        return fn


@pytest.fixture
def originals():
    """A recognisable product library and handle table in place of whatever the process has loaded."""
    saved_lib, had, saved_handles = nat._lib, hasattr(nat._tls, "handles"), getattr(nat._tls, "handles", None)
    lib, handles = object(), nat._ThreadHandles()
    nat._lib, nat._tls.handles = lib, handles
    try:
        yield lib, handles
    finally:
        handles.clear()
        nat._lib = saved_lib
        if had:
            nat._tls.handles = saved_handles
        else:
            del nat._tls.handles


def test_body_that_raises_restores_library_and_handles(originals):
    lib, handles = originals
    handles[(0, 0)] = "product handle"
    stand_in = StandIn()
    with pytest.raises(ZeroDivisionError):
        with diag_library_of(stand_in) as ctx:
            assert nat._lib is stand_in and nat.load_library() is stand_in
            assert nat._tls.handles is not handles and len(nat._tls.handles) == 0
            nat._tls.handles[(0, 0)] = "diag handle"  # what nat.handle(0) would have created
            assert ctx.lib is stand_in
            1 / 0
    assert nat._lib is lib
    assert nat._tls.handles is handles and handles == {(0, 0): "product handle"}
    # the handle created inside was destroyed on the stand-in, the product's was not touched
    assert [c for c in stand_in.calls if c[0] == "lidar_destroy"] == [("lidar_destroy", ("diag handle",))]
    with diag_library_of(StandIn()):  # and the context can be entered again
        pass
    assert nat._lib is lib and nat._tls.handles is handles


def test_no_handle_table_before_means_none_after():
    saved_lib, had, saved_handles = nat._lib, hasattr(nat._tls, "handles"), getattr(nat._tls, "handles", None)
    if had:
        del nat._tls.handles
    try:
        with diag_library_of(StandIn()):
            assert hasattr(nat._tls, "handles")
        assert not hasattr(nat._tls, "handles") and nat._lib is saved_lib
    finally:
        if had:
            nat._tls.handles = saved_handles


def test_nesting_is_refused(originals):
    lib, handles = originals
    outer = StandIn()
    with diag_library_of(outer):
        inner_handles = nat._tls.handles
        with pytest.raises(RuntimeError, match="nest"):
            with diag_library_of(StandIn()):
                pass
        assert nat._lib is outer and nat._tls.handles is inner_handles  # the outer context is intact
    assert nat._lib is lib and nat._tls.handles is handles


def test_call_reaches_the_stand_in(originals):
    stand_in = StandIn()
    with diag_library_of(stand_in):
        nat.call("lidar_reserve", "h", 4096)
        nat._tls.handles[(0, 0)] = "diag handle"
    assert ("lidar_reserve", ("h", 4096)) in stand_in.calls
    with pytest.raises(AttributeError):  # the recognisable product object has no entry points: not reached
        nat.call("lidar_reserve", "h", 4096)


def test_clean_handles_restores_the_table(originals):
    stand_in = StandIn()
    with diag_library_of(stand_in) as ctx:
        mine = nat._tls.handles
        with pytest.raises(KeyError):
            with ctx.clean_handles():
                assert nat._tls.handles is not mine
                nat._tls.handles[(0, 0)] = "clean handle"
                raise KeyError("x")
        assert nat._tls.handles is mine
    assert ("lidar_destroy", ("clean handle",)) in stand_in.calls


def diag_library_of(lib):
    return diag_lib.diag_library(lib=lib)
