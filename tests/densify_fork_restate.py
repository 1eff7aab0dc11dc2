"""A float32 torch restatement of the fork's ``densify_and_prune`` (``scene/gaussian_model.py:751-773``) in the
reference's own op sequence -- boolean-mask gathers, ``cat`` and ``repeat`` -- over plain dicts of tensors, on any
device.  It is the CPU check of tests/golden/densify_fork.npz (``test_densify_fork_host.py``), the larger-size check of
the HIP path (``test_gpu_densify_fork.py``) and the torch baseline of ``tools/bench_densify_fork.py``.

``params``: group name -> tensor (``xyz, f_dc, f_rest, opacity, scaling, rotation`` and the learned groups of the
flags), ``moments``: group name -> (exp_avg, exp_avg_sq).  ``noise`` / ``dir_noise``: the standard-normal draws of the
split's ``torch.normal`` and of the continuous re-init's ``torch.randn``, in the reference's order.
"""
import torch

FLAG_NAMES = ("grow_dir", "continous_dir", "grow_distance", "learn_split_distance", "learn_split_scale",
              "symmetric_split", "split_notreinit", "prob_notreinit")


def build_rotation(r):
    """utils/general_utils.py:78-99."""
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), device=r.device)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - w * z)
    R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y)
    R[:, 2, 1] = 2 * (y * z + w * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def split_draw_rows(flags, n_split_rows):
    """Rows of ``noise`` the split consumes over ``n_split_rows`` split rows (:523-537 / :694-708)."""
    if flags["learn_split_distance"]:
        return 0
    return n_split_rows if flags["symmetric_split"] else 2 * n_split_rows


class _State:
    def __init__(self, params, moments):
        self.p = {k: t.clone() for k, t in params.items()}          # the grow re-init writes in place (:645-655)
        self.m = dict(moments) if moments is not None else None

    def cat(self, d):                                           # cat_tensors_to_optimizer :445-466
        for k, t in d.items():
            self.p[k] = torch.cat((self.p[k], t), dim=0)
            if self.m is not None:
                a, b = self.m[k]
                self.m[k] = (torch.cat((a, torch.zeros_like(t)), dim=0), torch.cat((b, torch.zeros_like(t)), dim=0))

    def keep(self, mask):                                       # _prune_optimizer :401-417
        for k in self.p:
            self.p[k] = self.p[k][mask]
            if self.m is not None:
                self.m[k] = (self.m[k][0][mask], self.m[k][1][mask])


def _split(st, flags, sel, noise):
    """densify_and_split :509-580 / densify_and_growsplit :679-749 after the selection, N = 2."""
    p = st.p
    n = int(sel.sum())
    stds1 = torch.exp(p["scaling"])[sel]
    if flags["learn_split_distance"]:
        samples = stds1 * (2.2 * torch.sigmoid(p["split_distance"]))[sel]
        samples = torch.cat((samples, -samples), dim=0)
        stds = stds1
    elif flags["symmetric_split"]:
        stds = stds1
        samples = torch.zeros((n, 3), device=stds.device) + stds * noise[:n]
        samples = torch.cat((samples, -samples), dim=0)
    else:
        stds = stds1.repeat(2, 1)
        samples = torch.zeros((2 * n, 3), device=stds.device) + stds * noise[:2 * n]
    rots = build_rotation(p["rotation"][sel]).repeat(2, 1, 1)
    new = {"xyz": torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + p["xyz"][sel].repeat(2, 1)}
    if flags["learn_split_scale"]:
        k = (0.6 * torch.sigmoid(p["split_scale"]) + 0.5)[sel].repeat(2, 3)
        new["scaling"] = torch.log(stds1.repeat(2, 1) / (k * 2))
    else:
        new["scaling"] = torch.log(stds1.repeat(2, 1) / (0.8 * 2))
    for k in ("rotation", "opacity", "dirs_prob", "conti_dirs", "grow_dist"):
        if k in p:
            new[k] = p[k][sel].repeat(2, 1)
    for k in ("f_dc", "f_rest"):
        new[k] = p[k][sel].repeat(2, 1, 1)
    for k in ("split_distance", "split_scale"):
        if k in p:
            new[k] = p[k][sel].repeat(2, 1)
            if not flags["split_notreinit"]:
                new[k] = torch.zeros_like(new[k])
    st.cat(new)
    st.keep(~torch.cat((sel, torch.zeros(2 * n, dtype=torch.bool, device=sel.device))))


def densify_and_prune(params, moments, accum, denom, flags, percent_dense, max_grad, min_opacity, extent,
                      max_screen_size, iteration, opacity_reset_interval, dirs=None, noise=None, dir_noise=None):
    """Returns (params, moments, info); info: {"branch", "selected", "split_rows"}."""
    st = _State(params, moments)
    grads = accum / denom
    grads[grads.isnan()] = 0.0
    pde = percent_dense * extent
    P = grads.shape[0]
    grow = (flags["grow_dir"] or flags["continous_dir"]) and iteration > opacity_reset_interval
    if grow:
        p = st.p
        sel = torch.norm(grads, dim=-1) >= max_grad                                       # :614
        if flags["grow_dir"]:                                                              # :617-621, :360-366
            logits = p["dirs_prob"][sel]
            y = logits.softmax(-1)
            index = y.max(-1, keepdim=True)[1]
            one_hot = torch.zeros_like(logits).scatter_(-1, index, 1.0) - y.detach() + y
            gdir = torch.einsum("b n, n d -> b d", one_hot, dirs)
        else:
            gdir = torch.nn.functional.normalize(p["conti_dirs"][sel], p=2.0, dim=-1)
        d = 2 * torch.sigmoid(p["grow_dist"])[sel] if flags["grow_distance"] else 1
        shift = torch.max(torch.exp(p["scaling"])[sel], dim=1, keepdim=True).values
        new = {"xyz": p["xyz"][sel] + (gdir * shift * d)}
        G = int(sel.sum())
        if not flags["prob_notreinit"]:                                                    # :645-655
            if flags["grow_dir"]:
                p["dirs_prob"][sel] = torch.ones((G, dirs.shape[0]), device=dirs.device) / dirs.shape[0]
            elif flags["continous_dir"]:
                p["conti_dirs"][sel] = torch.nn.functional.normalize(dir_noise[:G], p=2.0, dim=-1)
            if flags["grow_distance"]:
                p["grow_dist"][sel] = torch.zeros((G, 1), device=sel.device)
        for k in p:
            if k != "xyz":
                new[k] = p[k][sel]
        st.cat(new)
        n_all = st.p["xyz"].shape[0]                                                       # :687-693
        padded = torch.zeros(n_all, device=sel.device)
        padded[:P] = grads.squeeze()
        split = padded >= max_grad
        split[P:] = True
        split = split & (torch.max(torch.exp(st.p["scaling"]), dim=1).values > pde)
    else:
        p = st.p
        sel = torch.norm(grads, dim=-1) >= max_grad                                       # :590-592
        clone = sel & (torch.max(torch.exp(p["scaling"]), dim=1).values <= pde)
        st.cat({k: t[clone] for k, t in p.items()})
        n_all = st.p["xyz"].shape[0]                                                       # :518-523
        padded = torch.zeros(n_all, device=sel.device)
        padded[:P] = grads.squeeze()
        split = (padded >= max_grad) & (torch.max(torch.exp(st.p["scaling"]), dim=1).values > pde)
    n_split_rows = int(split.sum())
    _split(st, flags, split, noise)
    prune = (torch.sigmoid(st.p["opacity"]) < min_opacity).squeeze(1)                      # :758-764
    if max_screen_size:
        n = st.p["xyz"].shape[0]
        prune = prune | (torch.zeros(n, device=prune.device) > max_screen_size) | \
            (torch.exp(st.p["scaling"]).max(dim=1).values > 0.1 * extent)
    st.keep(~prune)
    return st.p, st.m, {"branch": "grow" if grow else "clone_split", "selected": int(sel.sum()),
                        "split_rows": n_split_rows}
