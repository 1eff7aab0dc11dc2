"""A restatement of the fork's grow / learned-split branch (gaussian_renderer/__init__.py:91-253) in plain torch, written
from its contract (mvs_gaussian_splatting_amd/grow.py), in any dtype and on any device: the extended operator inputs of
a frame, differentiable w.r.t. the model's raw tensors, the learned tensors and means2D.

    ext, selected = restate(model, which, flags, threshold, percent_dense_extent, means2D, noise)

``model``: dict of raw tensors (xyz, f_dc, f_rest, opacity, scaling, rotation, dirs_prob, conti_dirs, grow_dist,
split_distance, split_scale, dirs, xyz_gradient_accum, denom).  ``which``: "grow" / "split".  ``flags``: dict of
grow_dir, continous_dir, grow_distance, learn_split_distance, learn_split_scale.  Returns the activated tensors the
operator receives (means3D, means2D, shs, opacities, scales, rotations; P + G rows) and the bool [P] selection.
"""
import numpy as np
import torch

RECORDED = ("means3D", "means2D", "shs", "opacities", "scales", "rotations")
LEARNED = ("dirs_prob", "conti_dirs", "grow_dist", "split_distance", "split_scale")
RAW = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def cotangent(seed, shapes):
    """The fixture's linear cotangent: one standard-normal CPU tensor per recorded tensor, drawn in RECORDED order."""
    gen = torch.Generator().manual_seed(int(seed))
    return {k: torch.randn(tuple(shapes[k]), generator=gen) for k in RECORDED}


def rotation_matrix(q):
    q = q / torch.sqrt((q * q).sum(dim=1, keepdim=True))
    w, x, y, z = q.unbind(1)
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=1).reshape(-1, 3, 3)


def selection(model, which, threshold, pde):
    g = model["xyz_gradient_accum"].reshape(-1) / model["denom"].reshape(-1)
    g = torch.where(torch.isnan(g), torch.zeros_like(g), g)
    sel = g.abs() >= threshold
    big = torch.exp(model["scaling"].detach()).max(dim=1).values > pde
    if which == "split":
        sel = sel & big
    return sel, big


def _max_lowest(s):
    """max over dim 1 whose gradient goes to the lowest index among ties."""
    m = s.detach().max(dim=1, keepdim=True).values
    first = torch.argmax((s.detach() == m).to(torch.int8), dim=1)
    return s.gather(1, first[:, None])


def restate(model, which, flags, threshold, pde, means2D, noise=None):
    sel, _ = selection(model, which, threshold, pde)
    idx = torch.nonzero(sel).reshape(-1)
    xyz = model["xyz"]
    shs = torch.cat((model["f_dc"], model["f_rest"]), dim=1)
    opac = torch.sigmoid(model["opacity"])
    scales = torch.exp(model["scaling"])
    rots = torch.nn.functional.normalize(model["rotation"], dim=-1)
    if which == "grow":
        if flags["grow_dir"]:
            logits = model["dirs_prob"][idx]
            y = torch.softmax(logits, dim=-1)
            a = torch.argmax((logits.detach() == logits.detach().max(dim=1, keepdim=True).values).to(torch.int8), dim=1)
            hard = torch.zeros_like(y).scatter_(1, a[:, None], 1.0)
            dirs = (hard - y.detach() + y) @ model["dirs"].to(y.dtype)
        else:
            dirs = torch.nn.functional.normalize(model["conti_dirs"][idx], dim=-1)
        d = 2 * torch.sigmoid(model["grow_dist"][idx]) if flags["grow_distance"] else 1.0
        new_xyz = xyz[idx] + dirs * _max_lowest(scales[idx]) * d
        out_xyz = torch.cat((xyz, new_xyz))
        out_scales = torch.cat((scales, scales[idx]))
    else:
        st = scales[idx]
        if flags["learn_split_distance"]:
            s = st * (2.2 * torch.sigmoid(model["split_distance"][idx]))
        else:
            s = (st * noise.to(st.dtype)).detach()          # torch.normal: no gradient to its std
        R = rotation_matrix(model["rotation"][idx])
        off = (R @ s[:, :, None])[:, :, 0]
        if flags["learn_split_scale"]:
            k = (0.6 * torch.sigmoid(model["split_scale"][idx]) + 0.5) * 2
        else:
            k = torch.full((idx.numel(), 1), 1.6, dtype=st.dtype, device=st.device)
        moved = xyz.index_add(0, idx, off)
        out_xyz = torch.cat((moved, xyz[idx] - off))
        divided = scales.index_put((idx,), st / k)
        out_scales = torch.cat((divided, st / k))
    ext = {"means3D": out_xyz, "means2D": torch.cat((means2D, means2D[idx])), "shs": torch.cat((shs, shs[idx])),
           "opacities": torch.cat((opac, opac[idx])), "scales": out_scales, "rotations": torch.cat((rots, rots[idx]))}
    return ext, sel


def case_model(z, dtype=torch.float64, device="cpu"):
    """Leaf tensors (requires_grad) of the fixture's model in ``dtype``."""
    m = {}
    for k in RAW + LEARNED:
        m[k] = torch.from_numpy(np.asarray(z[f"model/{k}"])).to(dtype).to(device).requires_grad_(True)
    m["dirs"] = torch.from_numpy(np.asarray(z["dirs"])).to(dtype).to(device)
    m["xyz_gradient_accum"] = torch.from_numpy(np.asarray(z["xyz_gradient_accum"])).to(device)
    m["denom"] = torch.from_numpy(np.asarray(z["denom"])).to(device)
    return m


def case_config(z, name):
    learn_d, learn_s = (bool(v) for v in z[f"{name}/flags"])
    flags = {"grow_dir": bool(z[f"{name}/arg/grow_dir"]), "continous_dir": bool(z[f"{name}/arg/continous_dir"]),
             "grow_distance": bool(z[f"{name}/arg/grow_distance"]), "learn_split_distance": learn_d,
             "learn_split_scale": learn_s}
    which = "grow" if flags["grow_dir"] or flags["continous_dir"] else "split"
    pde = float(np.float32(float(z["percent_dense"]) * float(z[f"{name}/extent"])))
    return which, flags, float(z["threshold"]), pde
