"""Frame issue: how ``rasterizer.py``'s operators get a frame onto the GPU and what they keep of it for the backward.
Nothing here depends on what the operator's inputs are: a frame arrives as a filled ``GsrParams``.

Host synchronisation.  Upstream reads ``num_rendered`` back in every forward to size its sort buffers: the GPU drains
while the host round-trips, sizes the binning workspace and issues the second half of the frame.  Here only the first
frame of a (device, P, W, H) combination does that (``gsr_forward_preprocess`` + ``gsr_forward_render``).  Later frames
are ENQUEUED WHOLE by ``gsr_forward`` with a caller-side capacity (``capacity_for``: 1.5 x the largest instance count
seen); the host then waits for the event behind the scan kernel only (a third of the way into the frame: the GPU keeps
the rest of the frame queued and never idles), compares the real count with the capacity and, if the frame did not fit,
re-issues it on the two-call path with a workspace of the right size BEFORE the operator returns.  The operator
therefore never raises and never hands out an incomplete image, whatever the camera sequence (``train.py:81-107`` draws
a random camera per iteration, ``render.py:32-35`` saves every image at once) -- it is bit-identical to the per-frame
read-back.  The modes (``rasterizer.set_sync_free``) arrive in ``_run_forward`` as an argument.
"""
from __future__ import annotations

import collections
import ctypes as C
import threading
from typing import NamedTuple, Optional

import torch

from . import _lib

_SYNC_OFF, _SYNC_DEFERRED = 0, 2        # rasterizer.SYNC_OFF / SYNC_DEFERRED (SYNC_VERIFIED = 1 is everything else)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _round_ws(nbytes: int) -> int:
    """Workspace sizes that depend on the per-view instance count are rounded up to 32 MiB steps, so that the caching
    allocator reuses one block from frame to frame instead of growing a new size class per view."""
    step = 1 << 25
    return max(step, (int(nbytes) + step - 1) // step * step)


def capacity_for(R: int) -> int:
    """The instance capacity a frame is issued with after one of ``R`` instances was seen: 1.5 x, in steps of 2^20."""
    return (int(R * 1.5) + (1 << 20)) >> 20 << 20


# ---- instance capacity of the frames issued without a count read-back ------------------------------------------------
class _CapacityState:
    """Per (device, P, W, H, binning mode): the instance capacity later frames are issued with, the widest depth-key span
    seen (frames are issued without the depth sort's fourth pass while it stays clearly below 2^24), and the workspaces
    forward-only frames share (nothing reads them after the frame: a fresh allocation per frame is pure host time)."""
    __slots__ = ("capacity", "last_counts", "depth_span", "fo_ws", "reissued")

    def __init__(self):
        self.capacity = 0
        self.last_counts = (0, 0)
        self.depth_span = 0     # largest (max depth key - min depth key) of the frames seen
        self.fo_ws = {}         # stream handle -> (capacity, geom, img, binning) of the forward-only frames on that stream
        self.reissued = 0       # frames that did not fit their capacity and were issued again (verified mode)

    def observe(self, R: int, V: int, span: int = 0) -> None:
        self.last_counts = (R, V)
        if span > self.depth_span:
            self.depth_span = span
        want = capacity_for(R)
        if R > 0 and want > self.capacity:
            self.capacity = want


class _Pending:
    """One DEFERRED frame whose instance count has not been compared with its capacity yet."""
    __slots__ = ("event", "slot", "capacity", "state", "done", "counts", "error", "dev_index")

    def __init__(self, event, slot, capacity, state, dev_index):
        self.event, self.slot, self.capacity, self.state, self.dev_index = event, slot, capacity, state, dev_index
        self.done, self.counts, self.error = False, None, None


_MAX_STATES = 16
_states: "collections.OrderedDict[tuple, _CapacityState]" = collections.OrderedDict()
_pending: "collections.deque[_Pending]" = collections.deque()
_free_slots: list = []
_parked_slots: list = []    # (slot, device index) of frames whose enqueue failed half-way: a kernel may still write them
_free_events: dict = {}     # device index -> HIP events created while that device was current
_defer_lock = threading.RLock()
_fo_owner = [None]          # the one state that keeps forward-only workspaces alive (~1 GB at 6 M Gaussians)


def _state_for(key) -> _CapacityState:
    with _defer_lock:
        st = _states.get(key)
        if st is None:
            st = _states[key] = _CapacityState()
            while len(_states) > _MAX_STATES:
                _states.popitem(last=False)
        else:
            _states.move_to_end(key)
        return st


def _keep_forward_only_ws(st: _CapacityState, stream: int, entry: tuple) -> None:
    """Forward-only frames of one stream reuse one set of workspaces; only the most recently used state holds any (a
    second resolution or a densified model takes the memory over instead of adding to it)."""
    with _defer_lock:
        owner = _fo_owner[0]
        if owner is not None and owner is not st:
            owner.fo_ws.clear()
        _fo_owner[0] = st
        if len(st.fo_ws) > 4:
            st.fo_ws.clear()
        st.fo_ws[stream] = entry


_RING = 64                  # deferred frames that may be in flight unchecked; the host waits for the oldest beyond that
_ring_store: list = []      # the one pinned allocation behind the slots (pin_memory() costs ~1 ms: never per frame)


def _pinned_slot() -> torch.Tensor:
    """A 64-byte slice of one pinned block for the counts of a deferred frame.  When all slots are out, the oldest
    pending frame is checked (blocking) to get its slot back."""
    while True:
        with _defer_lock:
            if not _ring_store:
                block = torch.zeros(_RING, 16, dtype=torch.int32).pin_memory()
                _ring_store.append(block)
                _free_slots.extend(block[i] for i in range(_RING))
            if _free_slots:
                return _free_slots.pop()
            oldest = _pending[0] if _pending else None
            parked = list(_parked_slots)
        if oldest is not None:
            _verify(oldest, block=True)
            continue
        if not parked:
            raise _lib.GsrError("pinned count slots exhausted with nothing pending")
        for slot, dev_index in parked:      # frames whose enqueue failed: safe again once their device has drained
            torch.cuda.synchronize(dev_index)
        with _defer_lock:
            for item in parked:
                if item in _parked_slots:
                    _parked_slots.remove(item)
                    _free_slots.append(item[0])


def _new_event(dev_index: int) -> int:
    """A HIP event of device ``dev_index`` (the current device): events are pooled per device -- recording an event
    on a stream of another device is an invalid-handle error."""
    with _defer_lock:
        pool = _free_events.get(dev_index)
        if pool:
            return pool.pop()
    ev = C.c_void_p()
    _lib.check(_lib.load().gsr_event_create(C.byref(ev)), "gsr_event_create")
    return ev.value


def _release_event(event: int, dev_index: int) -> None:
    with _defer_lock:
        _free_events.setdefault(dev_index, []).append(event)


def _verify(pend: _Pending, block: bool) -> bool:
    """Compare a deferred frame's real instance count with the capacity it ran with (waits for the scan kernel of that
    frame when ``block``).  Raises GsrError for an overflowed frame -- every time it is asked about."""
    with _defer_lock:
        if not pend.done:
            lib = _lib.load()
            if block:
                _lib.check(lib.gsr_event_wait(pend.event), "gsr_event_wait")
            else:
                done = C.c_int32(0)
                _lib.check(lib.gsr_event_query(pend.event, C.byref(done)), "gsr_event_query")
                if not done.value:
                    return False
            R, V = int(pend.slot[0]) & 0xffffffff, int(pend.slot[1]) & 0xffffffff
            pend.done, pend.counts = True, (R, V)
            pend.state.observe(R, V)
            _free_slots.append(pend.slot)
            _release_event(pend.event, pend.dev_index)
            pend.slot = pend.event = None
            try:
                _pending.remove(pend)
            except ValueError:
                pass
            if R > pend.capacity:
                pend.error = (f"frame issued in the DEFERRED sync-free mode overflowed its binning capacity: {R} instances "
                              f"> capacity {pend.capacity}; its image and gradients are incomplete and must be discarded "
                              "(later frames get a larger capacity; the default mode, set_sync_free(True), re-issues "
                              "such a frame by itself)")
        if pend.error:
            raise _lib.GsrError(pend.error)
        return True


def _drain_pending(block: bool = False) -> None:
    """Check every earlier deferred frame whose count has arrived (all of them when ``block``)."""
    while True:
        with _defer_lock:
            pend = _pending[0] if _pending else None
        if pend is None or not _verify(pend, block):
            return


def synchronize_counts() -> None:
    """Deferred mode only (a no-op otherwise: verified frames are checked before the operator returns).  Blocks until
    every frame issued so far has had its instance count checked; raises GsrError if one overflowed."""
    _drain_pending(block=True)


def _grown_key(P: int) -> tuple:
    """Capacity-state key of the frames that render a P-Gaussian model with virtual rows appended (grow.py): P + G changes
    from frame to frame, and all of them share one state instead of one (evicting) state per row count."""
    return ("grown", int(P))


def _counts_of(dev, P: int, W: int, H: int, grown: bool, binning_mode: int) -> tuple:
    """(last_counts, reissued) of that shape's state, as ``rasterizer.last_counts`` / ``reissued_frames`` hand them out."""
    key = (torch.device(dev).index or 0, _grown_key(P) if grown else int(P), int(W), int(H), binning_mode)
    with _defer_lock:
        st = _states.get(key)
        return (st.last_counts, st.reissued) if st is not None else ((0, 0), 0)


_thread_local = threading.local()


def _counts_pinned_thread():
    """Per-thread pinned host words the scan kernel mirrors (num_rendered, num_visible, depth range) into, and a ctypes
    view of them.  A frame of the two-call or the verified path has read them before the operator returns, so one buffer
    per thread serves every frame (forward and backward arrive on different threads)."""
    t = getattr(_thread_local, "pinned", None)
    if t is None:
        t = torch.zeros(16, dtype=torch.int32).pin_memory()
        _thread_local.pinned = t
        _thread_local.words = (C.c_uint32 * 16).from_address(t.data_ptr())
    return t, _thread_local.words


def _thread_event(dev_index: int) -> int:
    """The counts event of the verified path: one per (thread, device), reused by every frame (it is waited for before
    the next frame can record it again)."""
    evs = getattr(_thread_local, "events", None)
    if evs is None:
        evs = _thread_local.events = {}
    ev = evs.get(dev_index)
    if ev is None:
        ev = evs[dev_index] = _new_event(dev_index)
    return ev


class _Frame(NamedTuple):
    """What a forward leaves behind for its backward."""
    geom: torch.Tensor
    binning: torch.Tensor
    img: torch.Tensor
    radii: torch.Tensor
    layout_R: int          # (num_rendered, num_visible) the workspaces are laid out for: the real counts after the
    layout_V: int          #  two-call forward, (capacity, P) after gsr_forward
    pending: Optional[_Pending]     # deferred mode: the check that has not happened yet
    counts: Optional[tuple]         # the real (num_rendered, num_visible) when known


_DEPTH_SORT_BITS = 24                                   # csrc/gsr_common.h: the depth sort's three regular 8-bit passes
_DEPTH_SPAN_TRUSTED = int(0.9 * (1 << _DEPTH_SORT_BITS))


def _depth_span(words, V: int) -> int:
    """max - min depth key of a frame from its pinned counts (0 for a frame without visible Gaussians)."""
    mn, mx = int(words[2]), int(words[3])
    return mx - mn if V > 0 and mx >= mn else 0


def _run_forward(lib, dev, params, P: int, W: int, H: int, sync_mode: int, state_key=None):
    """Native forward on torch's current stream.  Returns (color, _Frame).  ``sync_mode``: rasterizer.SYNC_*.
    ``state_key``: the capacity state's key in place of P (grown frames, ``_grown_key``); such frames do not keep
    forward-only workspaces (their size varies)."""
    stream = _stream(dev)
    dev_index = dev.index or 0
    radii = torch.empty(P, dtype=torch.int32, device=dev)      # written for every Gaussian by the kernel
    color = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    mode = params.binning_mode
    st = _state_for((dev_index, P if state_key is None else state_key, W, H, mode))
    if _pending:
        _drain_pending()
    sync_free = sync_mode != _SYNC_OFF and st.capacity > 0 and mode != _lib.BINNING_KEYS64 and P > 0
    keep_fo = params.forward_only and state_key is None
    cached = st.fo_ws.get(stream) if (sync_free and keep_fo) else None
    if cached is not None and cached[0] == st.capacity:
        # forward-only frames of one stream run one after the other and nothing outlives them: same workspaces every frame
        _, geom, img, binning = cached
    else:
        geom = torch.empty(lib.gsr_geom_bytes(P), dtype=torch.uint8, device=dev)
        img = torch.empty(lib.gsr_image_bytes(W, H), dtype=torch.uint8, device=dev)
        binning = None
    if sync_free:
        cap = st.capacity
        nbytes = lib.gsr_binning_bytes(cap, P, W, H, mode)
        if binning is None:
            binning = torch.empty(_round_ws(nbytes), dtype=torch.uint8, device=dev)
            if keep_fo:
                _keep_forward_only_ws(st, stream, (cap, geom, img, binning))

        def enqueue_whole(event):
            _lib.check(lib.gsr_forward(C.byref(params), geom.data_ptr(), binning.data_ptr(), nbytes, cap, img.data_ptr(),
                                       radii.data_ptr(), color.data_ptr(), event, stream), "gsr_forward")

        if sync_mode == _SYNC_DEFERRED:
            slot, event = _pinned_slot(), _new_event(dev_index)
            params.counts_pinned = slot.data_ptr()
            pend = _Pending(event, slot, cap, st, dev_index)
            slot[0] = 0             # a frame whose enqueue fails half-way must not be read as an overflow later
            try:
                enqueue_whole(event)
            except _lib.GsrError:
                with _defer_lock:   # the scan kernel may already be queued and will write the slot: park it until the
                    _parked_slots.append((slot, dev_index))     # device has drained; the event was never recorded
                _release_event(event, dev_index)
                raise
            with _defer_lock:
                _pending.append(pend)
            return color, _Frame(geom, binning, img, radii, cap, P, pend, None)
        # verified mode: the whole frame is queued, the host waits for its scan kernel only.  Two things are taken on trust
        # from the frames before and checked against the counts: the instance capacity, and -- while every frame seen
        # stayed below 0.9 x 2^24 depth-key steps -- that the depth sort needs no fourth pass (GsrParams.depth_span_lt24:
        # three launches that find nothing to do, 14 us of a 6 M-Gaussian frame and 9 us of a 100 k one).
        pinned, words = _counts_pinned_thread()
        params.counts_pinned = pinned.data_ptr()
        narrow = st.depth_span < _DEPTH_SPAN_TRUSTED
        params.depth_span_lt24 = 1 if narrow else 0
        event = _thread_event(dev_index)
        enqueue_whole(event)
        _lib.check(lib.gsr_event_wait(event), "gsr_event_wait")
        params.depth_span_lt24 = 0
        R, V = int(words[0]), int(words[1])
        span = _depth_span(words, V)
        with _defer_lock:        # forward calls of several threads may share this (device, P, W, H) state
            st.observe(R, V, span)
        if R <= cap and not (narrow and span >> _DEPTH_SORT_BITS):
            return color, _Frame(geom, binning, img, radii, cap, P, None, (R, V))
        # The frame did not fit (its kernels dropped the instances past the capacity: no out-of-bounds access), or spans
        # more depth than it was sorted for (lists in the wrong order), and is still running.  Issue it again behind
        # itself, on the two-call path, into the same outputs -- nothing of the wrong frame has left the operator.
        with _defer_lock:
            st.reissued += 1
            if params.forward_only:
                st.fo_ws.pop(stream, None)
    pinned, _words = _counts_pinned_thread()
    params.counts_pinned = pinned.data_ptr()
    num_rendered, num_visible = C.c_uint32(0), C.c_uint32(0)
    _lib.check(lib.gsr_forward_preprocess(C.byref(params), geom.data_ptr(), _ptr(radii), stream,
                                          C.byref(num_rendered), C.byref(num_visible)), "gsr_forward_preprocess")
    R, V = int(num_rendered.value), int(num_visible.value)
    with _defer_lock:
        st.observe(R, V, _depth_span(_words, V))
    nbytes = lib.gsr_binning_bytes(R, V, W, H, mode)
    binning = torch.empty(_round_ws(nbytes), dtype=torch.uint8, device=dev)
    _lib.check(lib.gsr_forward_render(C.byref(params), geom.data_ptr(), binning.data_ptr(), nbytes, img.data_ptr(),
                                      R, V, color.data_ptr(), stream), "gsr_forward_render")
    return color, _Frame(geom, binning, img, radii, R, V, None, (R, V))


def _run_backward(lib, dev, params, frame: _Frame, grad_out_color: torch.Tensor, grads: "_lib.GsrGrads") -> None:
    if frame.pending is not None:
        _verify(frame.pending, block=True)      # deferred mode: the scan kernel of this frame's forward finished long ago
    P = int(params.P)
    nbytes = lib.gsr_backward_bytes(P, frame.layout_R)
    bwd_ws = torch.empty(_round_ws(nbytes), dtype=torch.uint8, device=dev)
    _lib.check(lib.gsr_backward(C.byref(params), _ptr(frame.radii), frame.geom.data_ptr(), frame.binning.data_ptr(),
                                frame.img.data_ptr(), frame.layout_R, frame.layout_V, grad_out_color.data_ptr(),
                                bwd_ws.data_ptr(), nbytes, C.byref(grads), _stream(dev)), "gsr_backward")
