"""PGSR's unbiased plane depth without a GPU: the float64 restatement of both kernels against finite
differences and against the analytic ray-plane depth, the decision rules, every refusal of the wrappers and of the four C
entry points, the ABI, the trainer's switch, and the census of the inputs tests/test_gpu_planes.py runs on."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from conftest import ROOT
import planes_restate as R

F64 = torch.float64


def _central(f, x, eps):
    g = torch.zeros_like(x)
    flat, gf = x.view(-1), g.view(-1)
    for i in range(flat.numel()):
        old = float(flat[i])
        flat[i] = old + eps
        hi = float(f(x))
        flat[i] = old - eps
        lo = float(f(x))
        flat[i] = old
        gf[i] = (hi - lo) / (2 * eps)
    return g


def test_restated_float64_gradients_agree_with_central_finite_differences():
    vm, cp = R.row_camera()
    s, q, m = R.make_rows(40)
    keep = ~R.planes(s, q, m, vm, cp)["facing0"]         # at a facing of exactly 0 a difference quotient crosses the sign
    keep[6] = False                                      # and the all-zero quaternion sits on the clamp's kink
    s, q, m = s[keep], q[keep].to(F64), m[keep].to(F64)
    up = torch.randn(s.shape[0], 4, dtype=F64, generator=torch.Generator().manual_seed(3))
    loss = lambda qq, mm: (R.planes(s, qq, mm, vm, cp)["planes"] * up).sum()      # noqa: E731
    qg, mg = q.clone().requires_grad_(True), m.clone().requires_grad_(True)
    loss(qg, mg).backward()
    scale_q = q.norm(dim=1, keepdim=True)                # a step relative to the quaternion's length
    fd_q = torch.stack([_central(lambda x: loss(torch.cat([q[:i], x[None], q[i + 1:]]), m), q[i].clone(),
                                 1e-6 * float(scale_q[i])) for i in range(q.shape[0])])
    fd_m = _central(lambda x: loss(q, x), m.clone(), 1e-6)
    assert R.rel_err(qg.grad, fd_q) < 1e-6 and R.rel_err(mg.grad, fd_m) < 1e-6
    assert float(qg.grad.abs().max()) > 0 and float(mg.grad.abs().max()) > 0

    N, D, A = (t.to(F64) for t in R.make_maps(7, 7))
    ok = R.plane_depth(N, D, A, *R.TANFOV)["valid"]
    N = torch.where(torch.isnan(N), torch.zeros_like(N), N)
    upz = torch.randn(7, 7, dtype=F64, generator=torch.Generator().manual_seed(4))
    lz = lambda n, d: (R.plane_depth(n, d, A, *R.TANFOV)["z"] * upz).sum()        # noqa: E731
    Ng, Dg = N.clone().requires_grad_(True), D.clone().requires_grad_(True)
    out = R.plane_depth(Ng, Dg, A, *R.TANFOV)
    (out["z"] * upz).sum().backward()
    fd_N, fd_D = _central(lambda x: lz(x, D), N.clone(), 1e-6), _central(lambda x: lz(N, x), D.clone(), 1e-6)
    assert R.rel_err(Ng.grad[:, ok], fd_N[:, ok]) < 1e-6 and R.rel_err(Dg.grad[ok], fd_D[ok]) < 1e-6
    # the closed-form unit gradients the kernel writes are autograd's
    assert R.rel_err(out["dz_dN"] * upz, Ng.grad) < 1e-14 and R.rel_err(out["dz_dD"] * upz, Dg.grad) < 1e-14
    assert not bool(Ng.grad[:, ~ok].any()) and not bool(Dg.grad[~ok].any())


def test_a_plane_tilted_50_degrees_is_exact_where_the_expected_depth_is_biased():
    W, H, tanx, tany = 48, 36, 0.5, 0.375
    tilt = math.radians(50.0)
    n = torch.tensor([math.sin(tilt), 0.0, -math.cos(tilt)], dtype=F64)          # view space, facing the camera
    d0 = 4.0 * math.cos(tilt)                                                    # the plane passes through (0, 0, 4)
    g = torch.Generator().manual_seed(2)
    ab = (torch.rand(900, 2, dtype=F64, generator=g) - 0.5) * torch.tensor([6.0, 4.0], dtype=F64)
    e1, e2 = torch.tensor([math.cos(tilt), 0.0, math.sin(tilt)], dtype=F64), torch.tensor([0.0, 1.0, 0.0], dtype=F64)
    centres = torch.tensor([0.0, 0.0, 4.0], dtype=F64) + ab[:, :1] * e1 + ab[:, 1:] * e2
    assert float((centres @ n + d0).abs().max()) < 1e-14                         # coplanar: n . x = -d0
    vm, campos = torch.eye(4), torch.zeros(3)
    quat = torch.tensor([math.cos(tilt / 2), 0.0, -math.sin(tilt / 2), 0.0]).repeat(900, 1)   # z axis -> (-sin, 0, cos)
    rows = R.planes(torch.tensor([[1.0, 1.0, 0.01]]).repeat(900, 1), quat.to(F64), centres, vm, campos)["planes"]
    assert R.rel_err(rows[:, :3], n.repeat(900, 1)) < 1e-7 and R.rel_err(rows[:, 3], torch.full((900,), d0, dtype=F64)) < 1e-7
    rows = torch.cat([n.repeat(900, 1), torch.full((900, 1), d0, dtype=F64)], dim=1)          # the exact rows
    rx, ry = R.rays(H, W, tanx, tany, F64)
    fx, fy, cx, cy = R.focal(H, W, tanx, tany)
    u, v = centres[:, 0] / centres[:, 2] * fx + cx, centres[:, 1] / centres[:, 2] * fy + cy
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    w = 0.2 * torch.exp(-((xs[..., None] - u) ** 2 + (ys[..., None] - v) ** 2) / (2 * 2.5 ** 2))     # [H,W,P]
    alpha = w.sum(-1)
    w = w / alpha.max() * 0.95
    alpha = w.sum(-1)
    normal, distance, depth = (w @ rows[:, :3]).permute(2, 0, 1), w @ rows[:, 3], w @ centres[:, 2]
    out = R.plane_depth(normal, distance, alpha, tanx, tany, alpha_min=0.3)
    covered = out["valid"]
    truth = d0 / -(n[0] * rx + n[1] * ry + n[2])
    err_plane = float(((out["z"] - truth).abs() / truth)[covered].max())
    err_expected = float(((depth / alpha - truth).abs() / truth)[covered].max())
    print(f"[planes host] {int(covered.sum())} covered pixels: plane depth off by {err_plane:.2e}, depth / alpha by "
          f"{err_expected:.2e} (relative, max)")
    assert int(covered.sum()) > 200 and bool((alpha[covered] >= 0.3).all())
    assert err_plane < 1e-13, "the plane depth is the ray-plane intersection to float64 rounding"
    assert err_expected > 100 * err_plane and err_expected > 1e-6, "the expected depth is measurably off"


def test_decision_rules_distance_sign_and_quaternion_scale():
    vm, cp = R.row_camera()
    s = torch.tensor([[0.2, 0.2, 0.5], [0.5, 0.2, 0.2], [0.3, 0.3, 0.3], [0.4, 0.1, 0.1000001], [0.3, 0.2, 0.1]])
    q = torch.tensor([[0.3, -0.5, 0.2, 0.7]]).repeat(5, 1)
    q[4] = torch.tensor([math.cos(0.4), 0.0, 0.0, math.sin(0.4)]) * 3.0
    m = torch.randn(5, 3, generator=torch.Generator().manual_seed(1))
    m[4] = torch.stack([cp[0] + 1.75, cp[1] - 0.5, cp[2]])                       # campos - mean is orthogonal to n = z
    out = R.planes(s, q, m, vm, cp)
    assert out["axis"].tolist() == [0, 1, 0, 1, 2], "an exact tie picks the smallest index"
    assert out["tie"].tolist() == [True, True, True, False, False] and not bool(out["fragile"][:3].any())
    assert bool(out["facing0"][4]) and float(out["sign"][4]) == 1.0 and float(out["planes"][4, 3]) == 0.0
    assert not bool(out["fragile"][4]), "exactly 0 is a rule, not a fragile row"
    assert bool(out["fragile"][3]), "scales a millionth apart without being equal are fragile"
    s, q, m = R.make_rows(4099)
    out = R.planes(s, q, m, vm, cp)
    assert float(out["planes"][:, 3].min()) >= 0.0, "d >= 0 by construction"
    # unit normals, as far as the float32 viewmatrix is orthonormal
    assert R.rel_err(out["planes"][:, :3].norm(dim=1), torch.ones(4099, dtype=F64)) < 1e-6
    for k in (7.5, 1e-3, -2.0):                          # -q is the same rotation
        again = R.planes(s, q.to(F64) * k, m, vm, cp)
        assert torch.equal(again["axis"], out["axis"]) and R.rel_err(again["planes"], out["planes"]) < 1e-14
    # float32 restatement: the same decisions off the fragile rows
    f32 = R.planes(s, q, m, vm, cp, torch.float32)
    ok = ~out["fragile"]
    assert torch.equal(f32["axis"][ok], out["axis"][ok])


def test_census_of_the_gpu_test_inputs():
    vm, cp = R.row_camera()
    lines = []
    for P in R.ROW_SIZES:
        out = R.planes(*R.make_rows(P), vm, cp)
        fragile, ties, zeros = int(out["fragile"].sum()), int(out["tie"].sum()), int(out["facing0"].sum())
        lines.append(f"P={P}: {fragile} fragile, {ties} exact ties, {zeros} facing 0")
        assert fragile <= 0.02 * P, lines[-1]
        assert not bool((out["fragile"] & out["tie"] & out["facing0"]).any())
        if P >= 63:
            assert ties >= 3 * (P // 16) - 3 and zeros >= 2 * (P // 16) - 2, "every kind of row is present"
    for W, H in R.MAP_SHAPES:
        out = R.plane_depth(*R.make_maps(W, H), *R.TANFOV)
        covered, fragile = int(out["valid"].sum()), int((out["fragile"] & out["valid"]).sum())
        total_fragile = int(out["fragile"].sum())
        lines.append(f"{W}x{H}: {covered} valid of {W * H}, {total_fragile} fragile")
        assert total_fragile <= 0.02 * max(covered, 1), lines[-1]
        assert covered >= 1 and fragile <= total_fragile
        if W * H >= 16:
            assert covered < W * H - 3, "the invalid kinds are present"
            assert not bool(torch.isnan(out["z"]).any()) and not bool(torch.isnan(out["dz_dN"]).any())
            assert not bool(out["z"][~out["valid"]].any()) and not bool(out["dz_dN"][:, ~out["valid"]].any())
    print("[planes host] census: " + "; ".join(lines))


def test_every_python_refusal_comes_before_a_gpu_is_asked_for():
    from mvs_gaussian_splatting_amd import _lib, gaussian_planes, plane_depth
    vm, cp = R.row_camera()
    s, q, m = R.make_rows(8)
    good = dict(scales=s, rotations=q, means3D=m, viewmatrix=vm, campos=cp)
    for kw in ({"scales": s[:7]}, {"scales": s[:, :2]}, {"rotations": q[:, :3]}, {"means3D": m[:5]}, {"means3D": m.view(-1)},
               {"viewmatrix": vm[:3]}, {"campos": torch.zeros(4)}, {"scales": s.to("meta")}, {"means3D": m.to("meta")},
               {"viewmatrix": vm.clone().requires_grad_(True)}, {"campos": cp.clone().requires_grad_(True)}):
        with pytest.raises(ValueError):
            gaussian_planes(**{**good, **kw})
    for kw in ({"scales": s.numpy()}, {"rotations": q.double()}, {"means3D": None}, {"viewmatrix": vm.double()},
               {"campos": [0.0, 0.0, 0.0]}):
        with pytest.raises(TypeError):
            gaussian_planes(**{**good, **kw})
    with pytest.raises(_lib.GsrError):
        gaussian_planes(**good)
    with pytest.raises(_lib.GsrError):
        gaussian_planes(s, q.clone().requires_grad_(True), m, vm, cp)

    N, D, A = R.make_maps(7, 5)
    good = dict(normal=N, distance=D[None], alpha=A[None], tanfovx=0.6, tanfovy=0.4)
    for kw in ({"normal": N[:2]}, {"normal": N[None]}, {"distance": D.t().contiguous()}, {"distance": D[None, None]},
               {"alpha": A[:, :3]}, {"alpha": A.to("meta")}, {"normal": N.to("meta")}, {"tanfovx": 0.0}, {"tanfovy": -1.0},
               {"tanfovx": math.inf}, {"tanfovy": math.nan}, {"alpha_min": 0.0}, {"alpha_min": 1.5}, {"alpha_min": math.nan},
               {"min_cos": -0.1}, {"min_cos": 1.0}, {"min_cos": math.nan}, {"distance": torch.zeros(0, 4)}):
        with pytest.raises(ValueError):
            plane_depth(**{**good, **kw})
    for kw in ({"normal": N.numpy()}, {"normal": N.double()}, {"distance": D.half()}, {"alpha": None}, {"distance": None}):
        with pytest.raises(TypeError):
            plane_depth(**{**good, **kw})
    with pytest.raises(_lib.GsrError):
        plane_depth(**good)
    with pytest.raises(_lib.GsrError):
        plane_depth(N.clone().requires_grad_(True), D, A, 0.6, 0.4, alpha_min=0.3, min_cos=0.0)


@pytest.fixture(scope="module")
def host_math(tmp_path_factory):
    """``csrc/planes_math.h`` -- the arithmetic both kernels run -- built by the host compiler from
    ``tests/planes_host_check.cpp`` with the kernels' ``-ffp-contract=off`` and loaded through ctypes."""
    import shutil
    import subprocess
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or \
        os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = str(tmp_path_factory.mktemp("planes_host") / "libplanes_host_check.so")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                    "-I" + os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc"),
                    os.path.join(ROOT, "tests", "planes_host_check.cpp"), "-o", out], check=True)
    return C.CDLL(out)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def test_the_kernels_arithmetic_built_for_the_host_meets_the_gpu_tests_bar(host_math):
    """What tests/test_gpu_planes.py asks of the kernels, asked of the same header on the CPU: decisions, the validity
    mask, exact zeros, and every value and gradient within twice the float32 restatement's error of the float64 one."""
    vm, cp = R.row_camera()
    for P in R.ROW_SIZES:
        s, q, m = R.make_rows(P)
        up = torch.randn(P, 4, generator=torch.Generator().manual_seed(17))
        refs = []
        for dtype in (F64, torch.float32):
            qg, mg = q.clone().to(dtype).requires_grad_(True), m.clone().to(dtype).requires_grad_(True)
            out = R.planes(s, qg, mg, vm, cp, dtype)
            out["planes"].backward(up.to(dtype))
            refs.append(dict(out, planes=out["planes"].detach(), d_rot=qg.grad, d_mean=mg.grad))
        r64, r32 = refs
        got = {"planes": torch.full((P, 4), math.nan), "d_rot": torch.full((P, 4), math.nan), "d_mean": torch.full((P, 3), math.nan)}
        host_math.planes_fwd(_ptr(s), _ptr(q), _ptr(m), P, _ptr(vm), _ptr(cp), _ptr(got["planes"]))
        host_math.planes_bwd(_ptr(s), _ptr(q), _ptr(m), P, _ptr(vm), _ptr(cp), _ptr(up), _ptr(got["d_rot"]), _ptr(got["d_mean"]))
        firm = ~r64["fragile"]
        off = (got["planes"].double()[:, :3] - r64["planes"][:, :3]).abs().max(dim=1).values
        assert float(off[firm].max()) < 1e-5, "axis or sign differs from the float64 restatement on a firm row"
        assert float(got["planes"][:, 3].min()) >= 0.0 and all(bool(torch.isfinite(t).all()) for t in got.values())
        if P > 6:
            assert not bool(got["d_rot"][6].any()), "the all-zero quaternion has no gradient"
        same = firm & ~r32["fragile"] & (r32["axis"] == r64["axis"]) & (r32["sign"].double() == r64["sign"])
        for key in got:
            err, own = R.rel_err(got[key][same], r64[key][same]), R.rel_err(r32[key][same], r64[key][same])
            assert err <= 2 * own, f"P={P} {key}: {err:.3e} above twice the float32 restatement's {own:.3e}"
    for W, H in R.MAP_SHAPES:
        N, D, A = R.make_maps(W, H)
        fx, fy, _, _ = R.focal(H, W, *R.TANFOV)
        got = {"z": torch.full((H, W), math.nan), "dz_dD": torch.full((H, W), math.nan), "dz_dN": torch.full((3, H, W), math.nan)}
        host_math.plane_depth(_ptr(N), _ptr(D), _ptr(A), H, W, C.c_float(fx), C.c_float(fy), C.c_float(0.5),
                              C.c_float(0.05), _ptr(got["z"]), _ptr(got["dz_dD"]), _ptr(got["dz_dN"]))
        r64, r32 = R.plane_depth(N, D, A, *R.TANFOV), R.plane_depth(N, D, A, *R.TANFOV, dtype=torch.float32)
        firm, valid = ~r64["fragile"], got["dz_dD"] != 0
        assert torch.equal(valid[firm], r64["valid"][firm]), "the validity mask differs off the fragile pixels"
        mask = firm & r64["valid"] & r32["valid"]
        for key, t in got.items():
            assert not bool(torch.isnan(t).any()) and not bool(t[..., ~valid].any())
            err, own = R.rel_err(t[..., mask], r64[key][..., mask]), R.rel_err(r32[key][..., mask], r64[key][..., mask])
            assert err <= 2 * own, f"{W}x{H} {key}: {err:.3e} above twice the float32 restatement's {own:.3e}"


def test_the_host_copy_of_a_camera_is_taken_once_per_tensor_version():
    from mvs_gaussian_splatting_amd.features import _host_camera
    vm, cp = R.row_camera()
    first = _host_camera(vm, cp)
    assert list(first[0]) == vm.reshape(-1).tolist() and list(first[1]) == cp.tolist()
    again = _host_camera(vm, cp)
    assert again[0] is first[0] and again[1] is first[1], "the same tensors are not read back again"
    vm[3, 0] += 1.0                                      # an in-place write: the copy is stale
    fresh = _host_camera(vm, cp)
    assert fresh[0] is not first[0] and list(fresh[0]) == vm.reshape(-1).tolist() and fresh[1] is first[1]
    assert _host_camera(vm.clone(), cp)[0] is not fresh[0], "another tensor is another camera"


ENTRY_POINTS = ("gsr_gaussian_planes_fwd", "gsr_gaussian_planes_bwd", "gsr_plane_depth_fwd", "gsr_plane_depth_bwd")


def test_library_exports_the_entry_points_and_the_three_abi_versions_agree():
    from mvs_gaussian_splatting_amd import _lib
    import mvs_gaussian_splatting_amd as pkg
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and name in header
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 37
    for name in ("gaussian_planes", "plane_depth"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    assert pkg.plane_depth is pkg.surface.plane_depth and pkg.gaussian_planes is pkg.features.gaussian_planes


def test_raw_abi_refuses_bad_arguments_before_any_hip_call():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 256)()
    ptr = C.addressof(buf)
    ptr += (-ptr) % 16
    cam = (C.c_float * 16)(*([1.0] * 16))
    cam_ptr = C.addressof(cam)
    inf, nan = math.inf, math.nan
    alive = []

    def bad_cam(i, v):
        alive.append((C.c_float * 16)(*[v if j == i else 1.0 for j in range(16)]))
        return C.addressof(alive[-1])

    good = dict(scales=ptr, rot=ptr, means=ptr, P=4, vm=cam_ptr, cp=cam_ptr, planes=ptr)
    fwd = lambda **kw: lib.gsr_gaussian_planes_fwd(*{**good, **kw}.values(), None)      # noqa: E731
    goodb = dict(scales=ptr, rot=ptr, means=ptr, P=4, vm=cam_ptr, cp=cam_ptr, g=ptr, drot=ptr, dmean=ptr)
    bwd = lambda **kw: lib.gsr_gaussian_planes_bwd(*{**goodb, **kw}.values(), None)     # noqa: E731
    for call, own in ((fwd, ("planes",)), (bwd, ("g", "drot", "dmean"))):
        for kw in [{k: None} for k in ("scales", "rot", "means", "vm", "cp") + own] + \
                  [{"P": -1}, {"vm": None, "P": 0}, {"cp": None, "P": 0}, {"vm": bad_cam(5, nan)}, {"vm": bad_cam(0, inf)},
                   {"cp": bad_cam(2, nan)}, {"cp": bad_cam(1, -inf), "P": 0}]:
            assert call(**kw) == -1, kw
            assert lib.gsr_last_error()
        for kw in ({"scales": ptr + 2}, {"means": ptr + 1}, {"rot": ptr + 4}, {"rot": ptr + 8}):
            assert call(**kw) == -3, kw
        # P = 0 is a successful no-op: no pointer is read, no HIP call is made
        assert call(P=0, scales=None, rot=None, means=None, **{k: None for k in own}) == 0
        # a finite entry outside viewmatrix[:3,:3] is not read
        assert call(P=0, vm=bad_cam(3, nan)) == 0 and call(P=0, vm=bad_cam(12, inf)) == 0
    for kw in ({"planes": ptr + 4}, {"planes": ptr + 8}):
        assert fwd(**kw) == -3, kw
    for kw in ({"g": ptr + 4}, {"drot": ptr + 8}, {"dmean": ptr + 2}):
        assert bwd(**kw) == -3, kw

    good = dict(normal=ptr, dist=ptr, alpha=ptr, H=4, W=4, tx=0.5, ty=0.5, amin=0.5, mcos=0.05, z=ptr, ud=ptr, un=ptr)
    pfwd = lambda **kw: lib.gsr_plane_depth_fwd(*{**good, **kw}.values(), None)         # noqa: E731
    bad = [{"normal": None}, {"dist": None}, {"alpha": None}, {"z": None}, {"ud": None}, {"un": None}, {"H": 0}, {"W": 0},
           {"H": -3}, {"H": 2 ** 14 + 1, "W": 2 ** 14}, {"amin": 0.0}, {"amin": 1.5}, {"amin": nan}, {"mcos": -0.01},
           {"mcos": 1.0}, {"mcos": nan}, {"mcos": inf}]
    bad += [{k: v} for k in ("tx", "ty") for v in (0.0, -1.0, inf, nan)]
    for kw in bad:
        assert pfwd(**kw) == -1, kw
        assert lib.gsr_last_error()
    for k in ("normal", "dist", "alpha", "z", "ud", "un"):
        assert pfwd(**{k: ptr + 2}) == -3, k
    good = dict(g=ptr, ud=ptr, un=ptr, H=4, W=4, gd=ptr, gn=ptr)
    pbwd = lambda **kw: lib.gsr_plane_depth_bwd(*{**good, **kw}.values(), None)         # noqa: E731
    for kw in [{k: None} for k in ("g", "ud", "un", "gd", "gn")] + [{"H": 0}, {"W": -1}, {"H": 2 ** 28, "W": 2}]:
        assert pbwd(**kw) == -1, kw
    for k in ("g", "ud", "un", "gd", "gn"):
        assert pbwd(**{k: ptr + 1}) == -3, k


class _Cam:
    FoVx = FoVy = 1.0
    image_width, image_height = 8, 8
    original_image = torch.zeros(3, 8, 8)


def test_optimization_params_gain_the_field_and_the_trainer_switches_off_and_refuses(monkeypatch):
    from mvs_gaussian_splatting_amd import trainer
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, training_iteration
    assert OptimizationParams().unbiased_depth is False

    class Plain:
        def update_learning_rate(self, iteration):
            pass

    class Dataset:
        grow_dir = True

    class Stop(Exception):
        pass

    calls = []

    def render(camera, model, pipe, bg, **kw):
        calls.append(kw)
        raise Stop
    monkeypatch.setattr(trainer, "render", render)

    def kwargs(opt, iteration=10, **kw):
        with pytest.raises(Stop):
            training_iteration(Plain(), _Cam, opt, None, torch.zeros(3), iteration, cameras_extent=1.0, **kw)
        return calls[-1]

    terms = ({"lambda_normal": 0.05, "normal_from_iter": 5}, {"lambda_multi_view_geo": 0.05, "multi_view_from_iter": 5},
             {"lambda_multi_view_ncc": 0.15, "multi_view_from_iter": 5})
    for term in terms:
        off = kwargs(OptimizationParams(**term), source_camera=_Cam)
        on = kwargs(OptimizationParams(unbiased_depth=True, **term), source_camera=_Cam)
        assert "return_plane_depth" not in off and on.get("return_plane_depth") is True
        assert {k: v for k, v in on.items() if k != "return_plane_depth" and k != "opt"} == \
            {k: v for k, v in off.items() if k != "opt"}, "the other arguments are the term's own"
        assert list(kwargs(OptimizationParams(unbiased_depth=False, **term), source_camera=_Cam)) == list(off)
        # before the term's first iteration the switch does nothing
        assert "return_plane_depth" not in kwargs(OptimizationParams(unbiased_depth=True, **term), iteration=4,
                                                  source_camera=_Cam)
        # the refusals are the terms' own, before anything is rendered
        n = len(calls)
        with pytest.raises(ValueError, match="pose_optimizer"):
            training_iteration(Plain(), _Cam, OptimizationParams(unbiased_depth=True, **term), None, torch.zeros(3), 10,
                               cameras_extent=1.0, source_camera=_Cam, pose_optimizer=object())
        with pytest.raises(ValueError, match="grow / learned-split"):
            training_iteration(Plain(), _Cam, OptimizationParams(unbiased_depth=True, **term), None, torch.zeros(3), 10,
                               cameras_extent=1.0, source_camera=_Cam, dataset=Dataset())
        assert len(calls) == n
    on = kwargs(OptimizationParams(unbiased_depth=True, depth_ratio=0.5, **terms[0]))
    assert on.get("return_plane_depth") is True and on.get("return_median_depth") is True
    # no geometry term: today's call, whatever the switch says
    today = kwargs(OptimizationParams())
    alone = kwargs(OptimizationParams(unbiased_depth=True, lambda_dist=100.0, dist_from_iter=0), pose_optimizer=None)
    assert "return_plane_depth" not in alone and "return_depth" not in today
    assert list(kwargs(OptimizationParams(unbiased_depth=True))) == list(today)


def test_render_and_fuse_views_pass_the_switch_on_and_leave_today_s_calls_alone():
    from mvs_gaussian_splatting_amd import renderer, tsdf
    seen = []

    class Halt(Exception):
        pass

    def fake(camera, model, pipe, bg, **kw):
        seen.append(kw)
        raise Halt
    for kw, expect in (({}, {"return_depth": True}), ({"depth_ratio": 0.5}, {"return_depth": True, "return_median_depth": True}),
                       ({"unbiased_depth": True}, {"return_plane_depth": True}),
                       ({"unbiased_depth": True, "depth_ratio": 1.0}, {"return_plane_depth": True, "return_median_depth": True})):
        with pytest.raises(Halt):
            tsdf.fuse_views(["cam"], "model", "pipe", "bg", object(), renderer=fake, **kw)
        assert seen[-1] == expect

    class Model:
        pass
    # refused on a grow frame exactly as return_normals is
    import mvs_gaussian_splatting_amd.grow as grow
    real = grow.branch
    grow.branch = lambda *a, **k: grow.GROW
    try:
        for flag in ("return_plane_depth", "return_normals"):
            with pytest.raises(ValueError, match="grow / learned-split"):
                renderer.render(_Cam, Model(), None, torch.zeros(3), **{flag: True})
    finally:
        grow.branch = real
