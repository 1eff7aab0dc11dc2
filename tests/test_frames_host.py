"""Host-side checks of the frame-issue module (``_frames.py``) and of what the two colour operators share: the capacity
rule, the capacity state, the arity of the backward results, and that ``rasterizer`` hands out ``_frames``' own objects.
No GPU and no built library."""
import inspect
import types

import pytest

from mvs_gaussian_splatting_amd import _frames, rasterizer


@pytest.mark.parametrize("R", [0, 1, 699050, 699051, 2 ** 20, 10_000_000])
def test_capacity_rule(R):
    """1.5 x in steps of 2^20 instances; 699051 is the first count whose 1.5 x crosses a step."""
    assert _frames.capacity_for(R) == (int(R * 1.5) + (1 << 20)) >> 20 << 20
    assert _frames.capacity_for(699050) == 1 << 20 and _frames.capacity_for(699051) == 2 << 20


def test_capacity_state_observe():
    st = _frames._CapacityState()
    st.observe(0, 0, 7)                                     # an empty frame: counts recorded, no capacity learned
    assert (st.capacity, st.last_counts, st.depth_span) == (0, (0, 0), 7)
    st.observe(3_000_000, 50_000, 5)
    big = _frames.capacity_for(3_000_000)
    assert (st.capacity, st.last_counts, st.depth_span) == (big, (3_000_000, 50_000), 7)
    st.observe(1000, 10, 1 << 24)                           # a smaller frame never lowers the capacity
    assert (st.capacity, st.last_counts, st.depth_span) == (big, (1000, 10), 1 << 24)
    st.observe(0, 0)
    assert (st.capacity, st.last_counts, st.depth_span) == (big, (0, 0), 1 << 24)
    st.observe(3_000_001 + (1 << 20), 1)
    assert st.capacity == _frames.capacity_for(3_000_001 + (1 << 20)) > big


@pytest.mark.parametrize("fn,n", [(rasterizer._RasterizeGaussians, 11), (rasterizer._RasterizeGaussiansFused, 12)])
def test_colour_backward_arity_without_a_gradient(fn, n):
    """One result per forward input: without the three camera slots when the frame had no camera inputs."""
    n_forward = len(inspect.signature(fn.forward).parameters) - 1           # minus ctx
    assert n_forward == n + 3
    for cam_shapes, want in ((None, n), (((4, 4), (4, 4), (3,)), n + 3)):
        out = fn.backward(types.SimpleNamespace(cam_shapes=cam_shapes), None, None)
        assert out == (None,) * want


def test_aux_maps_backward_arity_without_a_gradient():
    fn = rasterizer._AuxMaps
    assert fn.backward(types.SimpleNamespace(), None) == (None,) * 10
    assert len(inspect.signature(fn.forward).parameters) - 1 == 10


def test_rasterizer_binds_the_frame_modules_objects():
    for name in ("_states", "_round_ws", "_grown_key", "_counts_pinned_thread", "synchronize_counts", "_ptr"):
        assert getattr(rasterizer, name) is getattr(_frames, name), name
    assert (_frames._SYNC_OFF, _frames._SYNC_DEFERRED) == (rasterizer.SYNC_OFF, rasterizer.SYNC_DEFERRED)
