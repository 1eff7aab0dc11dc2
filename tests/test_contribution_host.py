"""CPU-side checks of the contribution statistics: the library and the binding agree on the ABI that carries them, the
restatement the GPU tests compare against (tests/contribution_restate.py) is itself checked against the alpha map of
tests/depth_restate.py, and the host side -- ContributionStats, prune_points_, prune_by_contribution -- on a CPU model
with a stepped torch.optim.Adam."""
import ctypes as C
import os
import re
import types

import pytest
import torch
from torch import nn

from conftest import ROOT, make_settings, small_scene
from contribution_restate import members_near, stats_from_lists
from depth_restate import maps_ref
from grad_util import MARGIN, oracle_operator_inputs

from mvs_gaussian_splatting_amd.densify import GROUP_ATTR


def test_library_exports_the_entry_point_and_the_three_abi_versions_agree():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "gsr_contribution_accumulate"), "gsr_contribution_accumulate is not exported"
    assert "gsr_contribution_accumulate" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    assert "gsr_contribution_accumulate" in header
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 24
    # GsrAuxFrame is reused unchanged: six 32-bit words, then four pointers
    assert C.sizeof(_lib.GsrAuxFrame) == 24 + 4 * C.sizeof(C.c_void_p) and _lib.GsrAuxFrame.geom_ws.offset == 24
    # argument checks run before any HIP call; a frame without Gaussians or instances is a success that launches nothing
    assert lib.gsr_contribution_accumulate(None, None, None, None) == -1
    frame = _lib.GsrAuxFrame()
    frame.P, frame.width, frame.height, frame.binning_mode = 0, 72, 40, _lib.BINNING_TWO_LEVEL_CULLED
    frame.img_ws = 256                      # never dereferenced: nothing is launched
    assert lib.gsr_contribution_accumulate(C.byref(frame), None, None, None) == 0
    frame.P, frame.num_rendered = 10, 0
    assert lib.gsr_contribution_accumulate(C.byref(frame), None, None, None) == 0


def test_restated_sums_add_up_to_the_restated_alpha_map():
    """In float64 the weights scatter-added per Gaussian and the weights summed per pixel are the same numbers:
    sum_g sum[g] == sum over pixels of the alpha map to 1e-12 relative; under a mask the same with the masked map.  The
    counts add up to the composited (pixel, entry) pairs, and a Gaussian never composited has sum = count = max = 0."""
    model, cam, bg, _ = small_scene(P=400, width=72, height=40)
    st = make_settings(cam, bg, 3)
    _, xyz, m2, op, kw = oracle_operator_inputs(model, torch.float64)
    with torch.no_grad():
        maps, _, radii, aux = maps_ref(xyz, m2, op, st, **kw)
        lists = (aux["pre"], aux["point_list"], aux["ranges"], aux["n_contrib"], st)
        total, count, largest = stats_from_lists(*lists)
        robust = aux["margin"] > MARGIN
        total_m, count_m, largest_m = stats_from_lists(*lists, mask=robust)
    assert total.dtype == torch.float64 and count.dtype == torch.int64 and tuple(total.shape) == (400,)
    whole = float(maps[2].sum())
    err = abs(float(total.sum()) - whole) / whole
    err_m = abs(float(total_m.sum()) - float(maps[2][robust].sum())) / whole
    print(f"[contribution restate] sum of the alpha map {whole:.6f}; relative difference of the per-Gaussian sums "
          f"{err:.2e}, under the robust mask {err_m:.2e}")
    assert whole > 100.0 and err <= 1e-12 and err_m <= 1e-12
    assert int(count.sum()) > int((aux["n_contrib"] > 0).sum()), "pixels composite more than one entry"
    assert bool((count_m <= count).all()) and bool((total_m <= total).all()) and bool((largest_m <= largest).all())
    never = count == 0
    assert bool(never[radii == 0].all()) and float(total[never].abs().max()) == 0.0 and float(largest[never].max()) == 0.0
    assert bool(((largest > 0) == (count > 0)).all()) and float(largest.max()) <= 0.99
    assert bool((total <= count.double() * largest + 1e-12).all()), "a sum is at most count x max"
    # the Gaussians near a fragile pixel are exactly those whose masked count can differ
    near = members_near(aux["point_list"], aux["ranges"], aux["pre"]["grid"], ~robust, 400)
    assert bool((count_m == count)[~near].all())


def test_stats_merge_score_and_the_reinterpreted_max():
    from mvs_gaussian_splatting_amd import ContributionStats

    def bits(x):
        return int(torch.tensor(x, dtype=torch.float32).view(torch.int32))

    a, b = ContributionStats(4), ContributionStats(4)
    assert a.raw.dtype == torch.int64 and tuple(a.raw.shape) == (4, 3) and a.views == 0 and int(a.raw.abs().sum()) == 0
    a.raw[0] = torch.tensor([3 << 29, 2, bits(0.75)])               # sum 1.5 over 2 pixels
    a.raw[1] = torch.tensor([1 << 30, 4, bits(0.25)])
    a.raw[3] = torch.tensor([(1 << 62) + 1, 1 << 40, bits(0.99)])   # far beyond 32 bits
    b.raw[0] = torch.tensor([1 << 28, 1, bits(0.25)])
    b.raw[1] = torch.tensor([1 << 29, 1, bits(0.5)])
    a.views, b.views = 2, 3
    assert torch.equal(a.weight_sum(), torch.tensor([1.5, 1.0, 0.0, 2.0 ** 32 + 2.0 ** -30], dtype=torch.float64))
    assert torch.equal(a.pixel_count(), torch.tensor([2, 4, 0, 1 << 40]))
    assert a.max_weight().dtype == torch.float32
    assert torch.equal(a.max_weight(), torch.tensor([0.75, 0.25, 0.0, 0.99], dtype=torch.float32))
    assert torch.equal(a.score("sum"), a.weight_sum()) and torch.equal(a.score("max"), a.max_weight())
    assert torch.equal(a.score("count"), a.pixel_count())
    assert torch.equal(a.score("mean")[:3], torch.tensor([0.75, 0.25, 0.0], dtype=torch.float64))
    with pytest.raises(ValueError):
        a.score("median")
    assert a.merge(b) is a and a.views == 5
    assert torch.equal(a.raw[0], torch.tensor([(3 << 29) + (1 << 28), 3, bits(0.75)]))      # add, add, max
    assert torch.equal(a.raw[1], torch.tensor([(1 << 30) + (1 << 29), 5, bits(0.5)]))
    assert torch.equal(a.raw[2], torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        a.merge(ContributionStats(5))
    a.reset()
    assert a.views == 0 and int(a.raw.abs().sum()) == 0


class _Model:
    pass


def _model(P, seed):
    """A duck-typed model on the CPU with the six parameter groups, a learned per-Gaussian tensor of the fork, the
    densification statistics, exposures and a torch.optim.Adam that has stepped once."""
    g = torch.Generator().manual_seed(seed)
    m = _Model()
    shapes = {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, 15, 3), "opacity": (P, 1), "scaling": (P, 3), "rotation": (P, 4)}
    for k, a in GROUP_ATTR.items():
        setattr(m, a, nn.Parameter(torch.randn(*shapes[k], generator=g)))
    m._split_scale = nn.Parameter(torch.randn(P, 1, generator=g))
    m.xyz_gradient_accum = torch.rand(P, 1, generator=g)
    m.denom = torch.rand(P, 1, generator=g)
    m.max_radii2D = torch.rand(P, generator=g)
    m._exposure = nn.Parameter(torch.randn(5, 3, 4, generator=g))
    groups = [{"params": [getattr(m, a)], "lr": 1e-2 * (i + 1), "name": k} for i, (k, a) in enumerate(GROUP_ATTR.items())]
    groups.append({"params": [m._split_scale], "lr": 1e-3, "name": "split_scale"})
    m.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for group in m.optimizer.param_groups:
        p = group["params"][0]
        p.grad = torch.randn(p.shape, generator=g)
    m.optimizer.step()
    return m


_ROWS = tuple(GROUP_ATTR.values()) + ("_split_scale",)


def _snapshot(m):
    snap = {a: getattr(m, a).detach().clone() for a in _ROWS + ("xyz_gradient_accum", "denom", "max_radii2D", "_exposure")}
    for group in m.optimizer.param_groups:
        state = m.optimizer.state[group["params"][0]]
        snap["m:" + group["name"]] = state["exp_avg"].clone()
        snap["v:" + group["name"]] = state["exp_avg_sq"].clone()
    return snap


def _assert_rows(m, snap, keep):
    """Every per-Gaussian tensor and moment of ``m`` is rows ``keep`` of the snapshot, bit for bit and in order."""
    n = int(keep.sum())
    for a in _ROWS:
        t = getattr(m, a)
        assert isinstance(t, nn.Parameter) and t.requires_grad and t.is_contiguous() and t.shape[0] == n
        assert torch.equal(t.detach(), snap[a][keep]), a
        assert any(t is group["params"][0] for group in m.optimizer.param_groups), f"the optimizer does not own {a}"
    for a in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert torch.equal(getattr(m, a), snap[a][keep]), a
    assert torch.equal(m._exposure.detach(), snap["_exposure"]), "exposures have no row per Gaussian"
    assert len(m.optimizer.state) == len(m.optimizer.param_groups)
    for group in m.optimizer.param_groups:
        state = m.optimizer.state[group["params"][0]]
        assert torch.equal(state["exp_avg"], snap["m:" + group["name"]][keep]), group["name"]
        assert torch.equal(state["exp_avg_sq"], snap["v:" + group["name"]][keep]), group["name"]
        assert float(state["step"]) == 1.0


def test_prune_points_keeps_rows_moments_and_order():
    from mvs_gaussian_splatting_amd import prune_points_
    P = 131
    m = _model(P, 3)
    snap = _snapshot(m)
    keep = torch.rand(P, generator=torch.Generator().manual_seed(4)) < 0.6
    assert prune_points_(m, keep) == int(keep.sum()) < P
    _assert_rows(m, snap, keep)
    for group in m.optimizer.param_groups:       # the pruned model trains on
        p = group["params"][0]
        p.grad = torch.ones_like(p)
    m.optimizer.step()
    assert not torch.equal(m._xyz.detach(), snap["_xyz"][keep])
    for bad in (torch.ones(P, dtype=torch.bool), torch.ones(int(keep.sum()), dtype=torch.uint8), [True] * int(keep.sum())):
        with pytest.raises(ValueError):
            prune_points_(m, bad)
    assert prune_points_(m, torch.ones(int(keep.sum()), dtype=torch.bool)) == int(keep.sum())      # keeping all is a no-op
    assert torch.equal(m.denom, snap["denom"][keep])


def _stats(scores_fx, counts=None):
    from mvs_gaussian_splatting_amd import ContributionStats
    s = ContributionStats(len(scores_fx))
    s.raw[:, 0] = torch.tensor(scores_fx, dtype=torch.int64)
    s.raw[:, 1] = torch.tensor(counts if counts is not None else [1 if v else 0 for v in scores_fx], dtype=torch.int64)
    s.raw[:, 2] = torch.tensor([0.5 if v else 0.0 for v in scores_fx]).view(torch.int32).to(torch.int64)
    return s


def test_prune_by_contribution_ranks_breaks_ties_by_index_and_wants_one_criterion():
    from mvs_gaussian_splatting_amd import prune_by_contribution
    # scores in units of 2^-30; three-way tie at 7 (rows 1, 4, 6), two never composited (rows 2, 8)
    fx = [5, 7, 0, 9, 7, 3, 7, 1, 0, 2]
    m = _model(10, 7)
    snap = _snapshot(m)
    out = prune_by_contribution(m, _stats(fx), keep_ratio=0.35)       # ceil(3.5) = 4 rows: 9, then 7, 7 by lower index ... and a third 7
    keep = torch.tensor([False, True, False, True, True, False, True, False, False, False])
    assert out == {"points": 4, "pruned": 6}
    _assert_rows(m, snap, keep)
    m = _model(10, 7)
    out = prune_by_contribution(m, _stats(fx), keep_ratio=0.3)        # 3 rows: of the tie the two lowest indices stay
    assert out == {"points": 3, "pruned": 7}
    _assert_rows(m, snap, torch.tensor([False, True, False, True, True, False, False, False, False, False]))
    m = _model(10, 7)
    assert prune_by_contribution(m, _stats(fx), kind="count", min_score=1) == {"points": 8, "pruned": 2}
    _assert_rows(m, snap, torch.tensor(fx) > 0)
    m = _model(10, 7)
    assert prune_by_contribution(m, _stats(fx), kind="sum", min_score=7 / 2.0 ** 30) == {"points": 4, "pruned": 6}
    _assert_rows(m, snap, keep)
    m = _model(10, 7)                                                   # mean = sum / max(count, 1)
    assert prune_by_contribution(m, _stats(fx, counts=[5, 1, 0, 9, 7, 1, 1, 1, 0, 1]), kind="mean",
                                 keep_ratio=0.2) == {"points": 2, "pruned": 8}
    _assert_rows(m, snap, torch.tensor([False, True, False, False, False, False, True, False, False, False]))
    m = _model(10, 7)
    assert prune_by_contribution(m, _stats(fx), keep_ratio=1.0) == {"points": 10, "pruned": 0}
    assert prune_by_contribution(m, _stats(fx), keep_ratio=0.0) == {"points": 0, "pruned": 10}
    m = _model(10, 7)
    for kw in ({}, {"keep_ratio": 0.5, "min_score": 0.1}):
        with pytest.raises(ValueError, match="exactly one"):
            prune_by_contribution(m, _stats(fx), **kw)
    with pytest.raises(ValueError):
        prune_by_contribution(m, _stats(fx), keep_ratio=1.5)
    with pytest.raises(ValueError):
        prune_by_contribution(m, _stats(fx[:9]), keep_ratio=0.5)
    with pytest.raises(ValueError):
        prune_by_contribution(m, _stats(fx), kind="median", keep_ratio=0.5)
    assert m._xyz.shape[0] == 10, "a refused call changes nothing"


def test_requests_are_refused_before_anything_runs_without_a_gpu():
    """Wrong row count, wrong mask, a grown-branch frame: ValueError; CPU tensors: GsrError (there is no CPU path)."""
    from mvs_gaussian_splatting_amd import ContributionStats, GaussianRasterizer, _lib, render
    from mvs_gaussian_splatting_amd.rasterizer import GaussianRasterizationSettings, rasterize_gaussians_fused
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    model, cam, bg, _ = small_scene(P=12, sh_degree=0, width=48, height=32, focal=12.0, scale=1.0)
    st = make_settings(cam, bg, 0, cls=GaussianRasterizationSettings)
    kw = dict(means3D=model.get_xyz, means2D=None, opacities=model.get_opacity, shs=model.get_features,
              scales=model.get_scaling, rotations=model.get_rotation)
    with pytest.raises(ValueError, match="rows"):
        GaussianRasterizer(st, contribution=ContributionStats(11))(**kw)
    for mask in (torch.ones(32, 47, dtype=torch.uint8), torch.ones(32, 48, dtype=torch.bool), torch.ones(48, 32, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="contribution_mask"):
            GaussianRasterizer(st, contribution=ContributionStats(12), contribution_mask=mask)(**kw)
    with pytest.raises(ValueError, match="raw"):
        GaussianRasterizer(st, contribution=types.SimpleNamespace(raw=torch.zeros(12, 3), views=0))(**kw)
    with pytest.raises(_lib.GsrError):
        GaussianRasterizer(st, contribution=ContributionStats(12))(**kw)
    stats = ContributionStats(12)
    with pytest.raises(ValueError, match="grown"):
        rasterize_gaussians_fused(model._xyz, None, model._features_dc, model._features_rest, model._opacity,
                                  model._scaling, model._rotation, st, _state_key=("grown", 12), contribution=stats)
    split = types.SimpleNamespace(learn_split_distance=True, learn_split_scale=False)
    opt = types.SimpleNamespace(densify_from_iter=500, densification_interval=100, densify_until_iter=15000,
                                opacity_reset_interval=3000)
    with pytest.raises(ValueError, match="grow / learned-split"):
        render(cam, model, PipelineParams(), bg, iteration=1, opt=opt, modelcg=split, contribution=stats)
    assert stats.views == 0 and int(stats.raw.abs().sum()) == 0
    # the plain constructor and call signature are what they were
    assert GaussianRasterizer(st).contribution is None and GaussianRasterizer(st).aux_maps is False
