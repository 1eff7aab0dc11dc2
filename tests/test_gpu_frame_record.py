"""What a colour frame leaves behind (``ctx.layout`` / ``frame_pending`` / ``counts`` / ``binning_mode`` and the four saved
workspaces, read back by ``rasterizer._frame_of``) is the same record for both colour operators, for the autograd node
and the ``_KeepFrame`` stand-in, in every sync-free mode, on the two-call frame and on the capacity frame."""
import pytest
import torch

from conftest import small_scene

pytestmark = pytest.mark.gpu
P, W, H, DEG = 64, 40, 24, 3        # 3 x 2 tiles, partial on both edges


def _same_tensor(a, b) -> bool:
    """The same memory seen the same way (autograd hands saved tensors out as fresh objects)."""
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.dtype == b.dtype and a.stride() == b.stride()


def _render_variants(dev, keep_nodes):
    """Both operators x (autograd, no_grad + aux_maps) x three sync modes x two frames.
    -> ({(operator, entry, mode, frame): (colour, radii, record)}, {(operator, mode, frame): means3D.grad}).
    ``keep_nodes``: the list the patched ``_KeepFrame`` appends its instances to."""
    from gpu_util import product_settings
    from mvs_gaussian_splatting_amd import GaussianRasterizer, rasterizer as rz
    model, cam, bg, _ = small_scene(P=P, sh_degree=DEG, width=W, height=H)
    model.to(dev); cam.to(dev)
    st = product_settings(cam, bg, DEG, dev)
    means2D = torch.zeros(P, 3, device=dev)
    xyz = model._xyz.detach().clone().requires_grad_(True)

    def call(operator, aux_maps):
        r = GaussianRasterizer(st, aux_maps=aux_maps)
        if operator == "fused":
            return r.forward_fused(xyz, means2D, model._features_dc.detach(), model._features_rest.detach(),
                                   model._opacity.detach(), model._scaling.detach(), model._rotation.detach())
        with torch.no_grad():
            feats, opac, scal, rot = model.get_features, model.get_opacity, model.get_scaling, model.get_rotation
        return r.forward(means3D=xyz, means2D=means2D, opacities=opac, shs=feats, scales=scal, rotations=rot)

    def record(node):
        frame, mode = rz._frame_of(node)
        saved = node.saved_tensors
        assert all(_same_tensor(a, b) for a, b in zip((frame.radii, frame.geom, frame.binning, frame.img), saved[-4:]))
        assert (frame.layout_R, frame.layout_V) == node.layout and frame.pending is node.frame_pending
        assert frame.counts == node.counts and mode == node.binning_mode
        return node.layout, node.counts, mode, node.frame_pending is not None

    out, grads = {}, {}
    prev = rz.sync_free_mode()
    try:
        for mode in (rz.SYNC_OFF, rz.SYNC_VERIFIED, rz.SYNC_DEFERRED):
            rz.set_sync_free(mode)
            for operator in ("getter", "fused"):
                for entry in ("autograd", "no_grad"):
                    rz.synchronize_counts()
                    rz._states.clear()
                    for frame in (0, 1):                # 0: two calls, learns the capacity; 1: issued with it
                        if entry == "autograd":
                            color, radii = call(operator, False)
                            node = color.grad_fn
                            rec = record(node)
                            xyz.grad = None
                            color.backward(torch.ones_like(color))
                            grads[operator, mode, frame] = xyz.grad.clone()
                            color = color.detach()
                        else:
                            del keep_nodes[:]
                            with torch.no_grad():
                                color, radii, _maps = call(operator, True)
                            (node,) = keep_nodes
                            assert all(a is b for a, b in zip(rz._frame_of(node)[0][:4],
                                                              [node.saved_tensors[i] for i in (-3, -2, -1, -4)]))
                            rec = record(node)
                        rz.synchronize_counts()
                        out[operator, entry, mode, frame] = (color.clone(), radii.clone(), rec)
    finally:
        try:
            rz.synchronize_counts()
        finally:
            rz.set_sync_free(prev)
            rz._states.clear()
    return out, grads


@pytest.fixture()
def keep_nodes(monkeypatch):
    from mvs_gaussian_splatting_amd import rasterizer as rz
    nodes = []

    class Recording(rz._KeepFrame):
        def __init__(self):
            nodes.append(self)

    monkeypatch.setattr(rz, "_KeepFrame", Recording)
    return nodes


def test_frame_record_of_both_operators_and_every_entry(gpu_device, keep_nodes):
    """means3D.grad (backward with ones) is asserted bit-equal between the two operators too: on this scene it is, at
    the commit before the operators shared one body as well."""
    from mvs_gaussian_splatting_amd import _frames, rasterizer as rz
    out, grads = _render_variants(gpu_device, keep_nodes)
    assert len(out) == 24 and len(grads) == 12
    color0, radii0, _ = out["getter", "autograd", rz.SYNC_OFF, 0]
    R0, V0 = out["getter", "autograd", rz.SYNC_OFF, 0][2][1]
    assert R0 >= V0 == int((radii0 > 0).sum()) >= 1 and float(color0.max()) > 0.0      # the frame is not an empty one
    worst = {k: (float((c - color0).abs().max()), int((r != radii0).sum())) for k, (c, r, _) in out.items()}
    print("[frame record] max |colour - first variant|, radii that differ:",
          {k: v for k, v in worst.items() if v != (0.0, 0)} or "all variants bit-equal")
    for (operator, entry, mode, frame), (color, radii, (layout, counts, bmode, pending)) in out.items():
        key = (operator, entry, mode, frame)
        # the record: frame 0 is laid out for its own counts; frame 1 for (capacity, P) unless every frame takes two calls
        R, V = out[operator, entry, mode, 0][2][1]
        if frame == 0 or mode == rz.SYNC_OFF:
            assert layout == counts == (R, V) and not pending, key
        else:
            assert layout == (_frames.capacity_for(R), P), key
            assert pending == (mode == rz.SYNC_DEFERRED) and counts == (None if pending else (R, V)), key
        # ... and is the same for both operators
        assert out["getter", entry, mode, frame][2] == out["fused", entry, mode, frame][2], key
        assert torch.equal(color, color0) and torch.equal(radii, radii0), (key, worst[key])
    g0 = grads["getter", rz.SYNC_OFF, 0]
    scale = float(g0.abs().max())
    assert scale > 0.0
    rel = {k: float((g - g0).abs().max()) / scale for k, g in grads.items()}
    print("[frame record] means3D.grad, max-norm relative to the getter-fed two-call frame:",
          {k: v for k, v in rel.items() if v} or "all bit-equal")
    for key, g in grads.items():
        assert torch.equal(g, g0), (key, rel[key])
