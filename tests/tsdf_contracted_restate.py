"""numpy restatement of TSDF fusion in contracted space (csrc/tsdf.hip, ABI v33; ``tsdf.ContractedTSDFVolume``; DESIGN.md
§7.20), written from the definitions: the contraction, its inverse, the integration of a view into a contracted volume
and the uncontraction of a mesh.  ``dtype=np.float64`` is the truth; ``dtype=np.float32`` runs the stated operations
rounded one by one and gives the GPU tests their bar (twice its own error against float64).

Everything from the world point ``p`` onward, and the extraction, is tests/tsdf_restate.py: ``integrate`` there is
whole-array arithmetic on ``origin + voxel_size * index``, so it is handed a volume whose "origin" is the array of the
uncontracted points (with a voxel size of 0) and whose truncation is the per-point array ``sdf_trunc * g``; the points
the ``q_max`` test skips are put back afterwards.  Also the inputs the host and GPU tests share.
"""
import math

import numpy as np

import tsdf_restate as R


# ---- the contraction ---------------------------------------------------------------------------------------------------
def contract(x):
    """float64: x for |x| <= 1, (2 - 1 / |x|) x / |x| otherwise.  x [...,3]."""
    x = np.asarray(x, np.float64)
    m = np.linalg.norm(x, axis=-1, keepdims=True)
    far = m > 1
    safe = np.where(far, m, 1.0)
    return np.where(far, (2.0 - 1.0 / safe) * (x / safe), x)


def scale_and_growth(m2, dtype=np.float64):
    """s and g of the inverse at |q|^2 = m2 (m2 < 4), each operation rounded to ``dtype``."""
    f = dtype
    m = np.sqrt(np.asarray(m2, f))
    far = m > f(1.0)
    with np.errstate(all="ignore"):
        s = np.where(far, f(1.0) / ((f(2.0) - m) * m), f(1.0)).astype(f)
        g = np.where(far, f(1.0) / (f(2.0) - m), f(1.0)).astype(f)
    return s, g


def squared_norm(q, dtype=np.float64):
    q = np.asarray(q, dtype)
    return (q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]


def uncontract(q, center, radius, dtype=np.float64):
    """Rows q [...,3] with |q| < 2 -> center + radius * (q * s), per axis q s, times radius, plus center."""
    f = dtype
    q = np.asarray(q, f)
    s, _ = scale_and_growth(squared_norm(q, f), f)
    return np.stack([f(center[a]) + f(radius) * (q[..., a] * s) for a in range(3)], axis=-1)


def grid_points(dims, origin, voxel_size, dtype=np.float64):
    """q [nz,ny,nx,3] = origin + voxel_size * (i, j, k): multiply, then add, per axis."""
    f = dtype
    nx, ny, nz = dims
    kk, jj, ii = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([f(origin[a]) + f(voxel_size) * idx.astype(f) for a, idx in enumerate((ii, jj, kk))], axis=-1)


# ---- integration -------------------------------------------------------------------------------------------------------
def integrate(vol, view, dtype=np.float64):
    """One view into the contracted volume ``vol`` (tsdf_restate's dict and ``center``, ``radius``, ``q_max``), in place.
    -> (updated, fragile) as tsdf_restate.integrate; a point within MARGIN of ``|q| = q_max`` is fragile as well."""
    f = dtype
    nz, ny, nx = vol["tsdf"].shape
    q = grid_points((nx, ny, nz), vol["origin"], vol["voxel_size"], f)
    m2 = squared_norm(q, f)
    inside = m2 < f(vol["q_max"]) * f(vol["q_max"])
    m2_safe = np.where(inside, m2, f(0.0))                                 # skipped points: anything finite
    s, g = scale_and_growth(m2_safe, f)
    p = [f(vol["center"][a]) + f(vol["radius"]) * (q[..., a] * s) for a in range(3)]
    names = ("tsdf", "weight") + (("color",) if vol.get("color") is not None else ())
    before = {n: vol[n].copy() for n in names}
    world = dict(vol, origin=tuple(p), voxel_size=0.0, sdf_trunc=f(vol["sdf_trunc"]) * g)
    live, fragile = R.integrate(world, view, dtype)
    for n in names:                                                        # the q_max test comes first: nothing written
        vol[n][~inside] = before[n][~inside]
    # within MARGIN of the bound, but not on it: equality is decided exactly where the grid is dyadic, and it skips
    m = np.sqrt(squared_norm(grid_points((nx, ny, nz), vol["origin"], vol["voxel_size"])))
    near_bound = (np.abs(m - vol["q_max"]) < R.MARGIN) & (m != vol["q_max"])
    return live & inside, (fragile & inside) | near_bound


def run_views(vol, views, dtype=np.float64, **override):
    """``views`` in order into ``vol`` -> (updated by any view, fragile in any view); float32: matrices and focal lengths
    rounded as the device holds them."""
    touched = np.zeros(vol["tsdf"].shape, bool)
    fragile = np.zeros(vol["tsdf"].shape, bool)
    for view in views:
        v = dict(view, **override)
        if vol.get("color") is None:
            v["color"] = None
        if dtype == np.float32:
            v["viewmatrix"] = v["viewmatrix"].astype(np.float32)
            v["fx"], v["fy"] = np.float32(v["fx"]), np.float32(v["fy"])
        up, fr = integrate(vol, v, dtype)
        touched |= up
        fragile |= fr
    return touched, fragile


def extract(vol, min_weight=1e-6, dtype=np.float64, contracted=False):
    """tsdf_restate.extract on the grid, then the vertices through the inverse contraction."""
    vertices, faces, colors = R.extract(vol, min_weight, dtype)
    if not contracted and len(vertices):
        vertices = uncontract(vertices, vol["center"], vol["radius"], dtype)
    return vertices, faces, colors


# ---- the shared integration case ------------------------------------------------------------------------------------------
# 70 x 9 x 6, past one 64-wide x-chunk with a ragged tail.  Dyadic origin and voxel: q = 0 is point (34, 4, 2), |q| = 1
# exactly at (50, 4, 2) and (18, 4, 2), |q| = 2 exactly at (66, 4, 2) and (2, 4, 2); the box corners have |q| > 2.
CASE_DIMS, CASE_VOXEL, CASE_ORIGIN = (70, 9, 6), 0.0625, (-2.125, -0.25, -0.125)
CASE_CENTER, CASE_RADIUS, CASE_Q_MAX = (0.375, -0.25, 0.5), 1.5, 1.875
CASE_TRUNC = 0.5                                          # world units: about 5 voxels of the unit ball (5 * 1.5 * 0.0625)
CASE_W, CASE_H = 48, 40
CASE_WEIGHTS, CASE_MAX_WEIGHT = (0.5, 2.25), 2.5          # both views: 2.75, clamped


def case_volume(with_color, dtype=np.float64):
    vol = R.empty_volume(CASE_DIMS, CASE_ORIGIN, CASE_VOXEL, CASE_TRUNC, with_color, dtype)
    vol.update(center=CASE_CENTER, radius=CASE_RADIUS, q_max=CASE_Q_MAX)
    return vol


def integration_case():
    """Two free-pose 48 x 40 views of the contracted slab (world: a thin plate through the centre that reaches 12 units
    out along x):
      0  an overview from the side at distance 9: the far ends of the plate leave the image left and right;
      1  a camera inside the unit ball that looks along the plate: what lies behind it has z <= 0.2.
    Depth: a sphere of radius 0.5 round the centre and a plane through it almost along the plate, ray-cast in float64,
    so that much of the plate lies inside the truncation band; then exact zeros; max_depth below the largest value.
    -> (cameras, views) as tsdf_restate.integrate takes them, without max_weight."""
    from mvs_gaussian_splatting_amd.synthetic import SyntheticCamera
    rng = np.random.default_rng(33)
    c = np.array(CASE_CENTER)
    level = np.eye(3)
    along = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])      # looks along world x
    poses = [(R._rotation((1.0, 0.5, 3.0), 9.0) @ level, c + np.array([0.3, 0.0, 0.0]), 9.0, 26.0, 30.0),
             (R._rotation((0.1, 1.0, 0.05), 14.0) @ along, c + np.array([-1.0, 0.05, 0.45]), 0.0, 30.0, 34.0)]
    normals = [(0.03, 0.12, 1.0), (0.03, 0.12, 1.0)]
    cameras, views = [], []
    for v, (Rc2w, aim, dist, fx0, fy0) in enumerate(poses):
        pos = aim - dist * Rc2w[:, 2]
        cam = SyntheticCamera(CASE_W, CASE_H, fx0, fy0, R=Rc2w, T=-Rc2w.T @ pos)
        M = cam.world_view_transform.numpy().astype(np.float64)
        fx = float(np.float32(CASE_W / (2.0 * math.tan(cam.FoVx * 0.5))))          # rounded as the binding rounds them
        fy = float(np.float32(CASE_H / (2.0 * math.tan(cam.FoVy * 0.5))))
        depth = R._raycast_surface(M, CASE_W, CASE_H, fx, fy, c, 0.5, normals[v]).astype(np.float32)
        depth[(np.arange(CASE_H)[:, None] * 3 + np.arange(CASE_W)[None, :] * 5 + v) % 13 == 1] = 0.0
        max_depth = float(np.float32(np.quantile(depth[depth > 0], (0.9, 0.97)[v])))
        views.append({"viewmatrix": M, "W": CASE_W, "H": CASE_H, "fx": fx, "fy": fy, "depth": depth,
                      "color": rng.random((3, CASE_H, CASE_W)).astype(np.float32), "weight": CASE_WEIGHTS[v],
                      "max_depth": max_depth})
        cameras.append(cam)
    return cameras, views


def run_case(views, with_color, max_weight=None, dtype=np.float64):
    """-> (volume, updated by any view, fragile in any view)."""
    vol = case_volume(with_color, dtype)
    return (vol,) + run_views(vol, views, dtype, max_weight=max_weight)


# ---- the unit ball: a contracted volume that must equal the plain one bit for bit -------------------------------------------
BALL_DIMS, BALL_VOXEL, BALL_ORIGIN, BALL_TRUNC = (70, 9, 6), 0.0234375, (-0.8125, -0.09375, -0.0625), 0.09375


def ball_case():
    """70 x 9 x 6 points that all have |q| <= 0.83, two views of a sphere of radius 0.3 and a plane through 0 -> (cameras,
    views)."""
    from mvs_gaussian_splatting_amd.synthetic import SyntheticCamera
    rng = np.random.default_rng(34)
    poses = [(R._rotation((1.0, 0.5, 3.0), 12.0) @ np.eye(3), 3.0, 50.0), (R._rotation((0.3, 1.0, 0.4), 140.0) @ np.eye(3), 2.5, 45.0)]
    cameras, views = [], []
    for v, (Rc2w, dist, f0) in enumerate(poses):
        cam = SyntheticCamera(CASE_W, CASE_H, f0, f0, R=Rc2w, T=-Rc2w.T @ (-dist * Rc2w[:, 2]))
        M = cam.world_view_transform.numpy().astype(np.float64)
        fx = float(np.float32(CASE_W / (2.0 * math.tan(cam.FoVx * 0.5))))
        fy = float(np.float32(CASE_H / (2.0 * math.tan(cam.FoVy * 0.5))))
        depth = R._raycast_surface(M, CASE_W, CASE_H, fx, fy, np.zeros(3), 0.3, (0.03, 0.12, 1.0)).astype(np.float32)
        views.append({"viewmatrix": M, "W": CASE_W, "H": CASE_H, "fx": fx, "fy": fy, "depth": depth,
                      "color": rng.random((3, CASE_H, CASE_W)).astype(np.float32), "weight": CASE_WEIGHTS[v],
                      "max_depth": None})
        cameras.append(cam)
    return cameras, views


# ---- a sphere beyond the unit ball, filled analytically ----------------------------------------------------------------------
SHELL_RES, SHELL_R, SHELL_Q_MAX = 33, 1.9, 1.9
SHELL_CENTER, SHELL_RADIUS = (0.375, -0.25, 0.5), 1.5
SHELL_SPHERE = 3.0 * SHELL_RADIUS                         # |x| = 3: |q| = 2 - 1/3


def shell_sphere_field(with_color=False):
    """33^3 samples of [-1.9, 1.9]^3: the clamped analytic signed distance of the sphere of radius 3 * radius about the
    centre, evaluated at the uncontracted grid points with the truncation 5 world voxels * g; weight 1 where
    |q| < q_max, 0 (and tsdf 1) elsewhere.  float32 fields, as the device holds them."""
    n = SHELL_RES
    voxel = 2.0 * SHELL_R / (n - 1)
    origin = (-SHELL_R,) * 3
    q = grid_points((n, n, n), origin, voxel)
    m2 = squared_norm(q)
    inside = m2 < SHELL_Q_MAX ** 2
    s, g = scale_and_growth(np.where(inside, m2, 0.0))
    dist = SHELL_RADIUS * np.sqrt(m2) * s                                  # |p - center|
    trunc = 5.0 * SHELL_RADIUS * voxel
    tsdf = np.where(inside, np.clip((dist - SHELL_SPHERE) / (trunc * g), -1.0, 1.0), 1.0).astype(np.float32)
    assert not np.any(tsdf == 0)
    color = (0.5 + 0.25 * q).astype(np.float32) if with_color else None
    return {"tsdf": tsdf, "weight": inside.astype(np.float32), "color": color, "origin": origin, "voxel_size": voxel,
            "sdf_trunc": trunc, "center": SHELL_CENTER, "radius": SHELL_RADIUS, "q_max": SHELL_Q_MAX}
