"""The frame the trainer issues, restated: the colour image and the four maps of ONE oracle frame, each under the loss its own
test uses, and the gradients of the coefficient-weighted sum of the five.

A training frame with the 2DGS regularisers carries up to five autograd nodes over one rasterised frame (rasterizer.py:
the colour node, ``_AuxMaps``, ``_FeatureMaps``, ``_DistortionMap``, ``_MedianDepth``).  The map nodes own no state: they read
the colour node's workspaces by reference and return gradients of their own, which autograd sums.  Every node alone has a
float64 restatement (depth_restate, features_restate, distortion_restate, median_restate), and all four take
``(pre, point_list, ranges, n_contrib, settings)``: one ``oracle.rasterize_ref(..., want_aux=True, want_margin=True)`` per
dtype feeds the five terms.

Terms (each with the weights of its own test, zero on that term's own threshold-fragile pixels, taken from the float64 pass
and reused for float32):

    colour      grad_util.weighted_sum(colour, linear_weights)           zero where margin <= grad_util.MARGIN
    aux         depth_restate.maps_loss(maps, map_weights)               as tests/test_gpu_depth.py
    features    grad_util.weighted_sum(feat, feature_weights)            as tests/test_gpu_features.py; feat = the 5 user rows
                                                                         feature_rows(P, 5) and the three view-space normal
                                                                         rows, concatenated as renderer.render does
    distortion  distortion_restate.dist_loss(dist, dist_weights)         mapping "ndc"; as tests/test_gpu_distortion.py
    median      median_restate.median_loss(median, median_weights)       zero also where the fragility is below FRAGILE

Coefficients.  The terms differ by orders of magnitude, and a plain sum would hide a wrong small term under the max-norm of
the colour term: every term gets ``c_t = 1 / max|d term_t / d xyz|``, from the float64 pass alone, so that each contributes a
position gradient of max-norm one to the sum.

Shared by tests/test_joint_frame_host.py (which asserts, on the CPU, that the bars of the GPU test are reachable in float32)
and tests/test_gpu_joint_frame.py.  Computed once per scene and shared, never modified.
"""
import functools

import torch

from conftest import make_settings
from depth_restate import map_weights, maps_from_lists, maps_loss
from distortion_restate import dist_loss, dist_weights, distortion_from_lists
from features_restate import feature_maps_from_lists, feature_rows, feature_weights
from grad_util import ESCAPE_CAP, MARGIN, TOL, linear_weights, oracle_operator_inputs, weighted_sum
from median_restate import FRAGILE, SCENES, median_from_lists, median_loss, median_weights, scene
from oracle import rasterize_ref

TERMS = ("colour", "aux", "features", "distortion", "median")
N_USER = 5                                  # user feature rows in front of the three normal rows
MAX_LEFT_OUT = {"colour": 0.05, "aux": 0.05, "features": 0.05, "distortion": 0.05, "median": 0.02}
MAPPING = "ndc"

assert set(SCENES) == {"small", "big"}


def geometry_names(use_cov=False):
    return ("xyz", "opacity", "means2D") + (("cov3D",) if use_cov else ("scaling", "rotation"))


def leaf_names(use_cov=False):
    """Every tensor the joint frame differentiates: the geometry, the SH rows (``sh`` of the operator, held as the two raw
    tensors it is concatenated from) and the user feature rows ``F``."""
    return geometry_names(use_cov) + ("f_dc", "f_rest", "F")


def normal_rows(model, kw, xyz, settings, dtype):
    """The three rows ``renderer.render(return_normals=True)`` appends: ``features.gaussian_normals`` of the activated
    scales and rotations.  With ``cov3D_precomp`` the operator has no scales or rotations: the rows are the model's, held
    constant."""
    from mvs_gaussian_splatting_amd.features import gaussian_normals
    if "scales" in kw:
        scales, rotations = kw["scales"], kw["rotations"]
    else:
        scales = torch.exp(model._scaling.detach().to(dtype).to(xyz.device))
        rotations = torch.nn.functional.normalize(model._rotation.detach().to(dtype).to(xyz.device))
    return gaussian_normals(scales, rotations, xyz, settings.viewmatrix.to(dtype), settings.campos.to(dtype))


def term_losses(color, aux_maps, feat, dist, median, weights):
    """The five losses of a frame, from its colour image and its maps (oracle or HIP), un-weighted: {term: 0-dim tensor}."""
    return {"colour": weighted_sum(color, weights["colour"]), "aux": maps_loss(aux_maps, weights["aux"]),
            "features": weighted_sum(feat, weights["features"]), "distortion": dist_loss(dist, weights["distortion"]),
            "median": median_loss(median, weights["median"])}


def joint_loss(losses, coef):
    return sum(coef[t] * losses[t] for t in TERMS)


def bar_of(g64, g32):
    """(bar, float32 restatement's error) of grad_util.compare_grads for one tensor, max-norm relative."""
    scale = float(g64.abs().max())
    e32 = float((g32.double() - g64).abs().max()) / scale if scale > 0.0 else 0.0
    return max(TOL, 2.0 * e32), e32


def joint_reference(name, use_cov=False):
    """The float64 and float32 joint reference of a scene (below), computed once per (scene, use_cov) and shared."""
    return _joint_reference(name, bool(use_cov))      # (one cache entry however the default is spelt)


@functools.lru_cache(maxsize=None)
def _joint_reference(name, use_cov):
    """-> dict:
      "names"                 leaf_names(use_cov)
      "coef"                  {term: c_t}
      "weights"               {term: float64 loss weights}
      "left_out"              {term: share of the covered pixels with zero weight}
      "covered", "radii", "aux", "F" (float32 [P,5]), "settings"
      "maps"                  the float64 maps: colour [3,H,W], aux [3,H,W], features [8,H,W], distortion [1,H,W],
                              median [1,H,W], median_id [H,W]
      torch.float64 / torch.float32 -> {"terms": {term: {name: un-weighted gradient, None where the term does not depend on
                              the tensor}}, "joint": {name: sum_t c_t gradient}}
    The caps (every term's left-out share, and grad_util.compare_grads' ESCAPE_CAP on the float32 joint sum against the
    float64 one, per tensor) are asserted here, on the oracle alone."""
    model, cam, bg = scene(name)
    st = make_settings(cam, bg, 3)
    H, W = SCENES[name]["height"], SCENES[name]["width"]
    P = int(model._xyz.shape[0])
    names = leaf_names(use_cov)
    F32 = feature_rows(P, N_USER)
    out = {"names": names, "F": F32, "settings": st}
    for dt in (torch.float64, torch.float32):
        leaves, xyz, m2, op, kw = oracle_operator_inputs(model, dt, use_cov=use_cov)
        leaves["F"] = F32.to(dt).clone().requires_grad_(True)       # (a copy: .to(float32) would hand back the shared rows)
        color, radii, aux = rasterize_ref(xyz, m2, op, st, want_aux=True, want_margin=True, **kw)
        lists = (aux["pre"], aux["point_list"], aux["ranges"], aux["n_contrib"], st)
        rows = torch.cat((leaves["F"], normal_rows(model, kw, xyz, st, dt)), dim=1)
        maps = maps_from_lists(*lists)
        feat = feature_maps_from_lists(*lists, rows)
        dist = distortion_from_lists(*lists, MAPPING)
        median, median_id, _, frag = median_from_lists(*lists)
        if dt == torch.float64:
            covered = aux["n_contrib"] > 0
            robust = aux["margin"] > MARGIN
            keep = robust & (frag >= FRAGILE)
            out["weights"] = {"colour": linear_weights((3, H, W)) * robust[None], "aux": map_weights(H, W) * robust[None],
                              "features": feature_weights(N_USER + 3, H, W) * robust[None],
                              "distortion": dist_weights(H, W) * robust[None], "median": median_weights(H, W) * keep[None]}
            n_cov = max(1, int(covered.sum()))
            out["left_out"] = {t: float((covered & ~(keep if t == "median" else robust)).sum()) / n_cov for t in TERMS}
            out.update(covered=covered, robust=robust, keep=keep, radii=radii.clone(), aux=aux)
            out["maps"] = {"colour": color.detach(), "aux": maps.detach(), "features": feat.detach(),
                           "distortion": dist.detach(), "median": median.detach(), "median_id": median_id}
        losses = term_losses(color, maps, feat, dist, median, out["weights"])
        terms = {}
        for t in TERMS:
            got = torch.autograd.grad(losses[t], [leaves[k] for k in names], retain_graph=True, allow_unused=True)
            terms[t] = {k: (None if g is None else g.detach().clone()) for k, g in zip(names, got)}
        out[dt] = {"terms": terms}
    g64 = out[torch.float64]["terms"]
    out["coef"] = {t: 1.0 / float(g64[t]["xyz"].abs().max()) for t in TERMS}
    for dt in (torch.float64, torch.float32):
        terms = out[dt]["terms"]
        out[dt]["joint"] = {k: sum(out["coef"][t] * terms[t][k] for t in TERMS if terms[t][k] is not None) for k in names}
    print(f"[joint] scene {name}{', cov3D_precomp' if use_cov else ''}: {int(out['covered'].sum())} covered pixels; left out "
          + ", ".join(f"{t} {out['left_out'][t]:.4f}" for t in TERMS) + "; coefficients "
          + ", ".join(f"{t} {out['coef'][t]:.4e}" for t in TERMS))
    for t in TERMS:
        assert out["left_out"][t] <= MAX_LEFT_OUT[t], \
            f"scene {name}: the oracle alone leaves out {out['left_out'][t]:.4f} of the covered pixels of the {t} term"
    for k in names:
        bar, e32 = bar_of(out[torch.float64]["joint"][k], out[torch.float32]["joint"][k])
        assert bar <= ESCAPE_CAP, (f"scene {name}: the joint gradient of {k} is too ill-conditioned to test (the float32 "
                                   f"restatement itself is {e32:.2e} off float64)")
    return out


def present(grads):
    """A per-term gradient dict without the tensors the term does not depend on (for grad_util.compare_grads)."""
    return {k: g for k, g in grads.items() if g is not None}
