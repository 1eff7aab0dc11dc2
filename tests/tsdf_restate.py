"""numpy restatement of the TSDF fusion and of the marching-tetrahedra extraction (csrc/tsdf.hip), written
from the definitions, not from the kernel: the integration is whole-array arithmetic, the extraction walks cubes and
tetrahedra in Python, keys every vertex by (owning grid point, direction) in a dictionary and orients by permutation
parity computed on the spot -- no case table, no masks, no scans.  ``dtype=np.float64`` is the truth the GPU tests compare
against; ``dtype=np.float32`` runs the same operations rounded to float32 one by one and gives the tests their bar (twice
its own error against float64).  Also the inputs the host and GPU tests share.
"""
import itertools
import math

import numpy as np

MARGIN = 1e-4          # fragility margin: pixels for u + 0.5 / v + 0.5, relative to sdf_trunc for sdf and max_depth, absolute for z
DIRECTIONS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)]


# ---- integration -----------------------------------------------------------------------------------------------------
def integrate(vol, view, dtype=np.float64):
    """One view into ``vol`` (dict: tsdf, weight [nz,ny,nx], color [nz,ny,nx,3] or None, origin, voxel_size, sdf_trunc),
    in place.  ``view``: viewmatrix [4,4] (row-vector convention), W, H, fx, fy, depth [H,W], color [3,H,W] or None,
    weight, max_depth or None, max_weight or None.  Returns (updated, fragile), bool [nz,ny,nx]: the points this view
    wrote, and the points one of whose float64 comparisons is within MARGIN of flipping."""
    f = dtype
    nz, ny, nx = vol["tsdf"].shape
    M = np.asarray(view["viewmatrix"], dtype=f)
    vs, trunc = f(vol["voxel_size"]), f(vol["sdf_trunc"])
    o = [f(v) for v in vol["origin"]]
    W, H = view["W"], view["H"]
    kk, jj, ii = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    px_w = o[0] + vs * ii.astype(f)
    py_w = o[1] + vs * jj.astype(f)
    pz_w = o[2] + vs * kk.astype(f)
    col = lambda c: ((px_w * M[0, c] + py_w * M[1, c]) + pz_w * M[2, c]) + M[3, c]      # noqa: E731
    x, y, z = col(0), col(1), col(2)
    fragile = np.abs(z.astype(np.float64) - 0.2) < MARGIN
    live = z > f(0.2)
    with np.errstate(all="ignore"):
        u = (f(view["fx"]) * x) / z + f((W - 1) / 2.0)
        v = (f(view["fy"]) * y) / z + f((H - 1) / 2.0)
        su, sv = u + f(0.5), v + f(0.5)
        fragile |= live & ((np.abs(su - np.rint(su)) < MARGIN) | (np.abs(sv - np.rint(sv)) < MARGIN))
        fx_, fy_ = np.floor(su), np.floor(sv)
        live &= (fx_ >= 0) & (fx_ < W) & (fy_ >= 0) & (fy_ < H)
    pxi = np.where(live, fx_, 0).astype(np.int64)
    pyi = np.where(live, fy_, 0).astype(np.int64)
    d = np.asarray(view["depth"], dtype=f)[pyi, pxi]
    live &= d > 0
    if view.get("max_depth") is not None:
        fragile |= live & (np.abs(d - f(view["max_depth"])) < MARGIN * trunc)
        live &= ~(d > f(view["max_depth"]))
    sdf = d - z
    fragile |= live & (np.abs(sdf + trunc) < MARGIN * trunc)
    live &= ~(sdf < -trunc)
    t = np.minimum(f(1.0), sdf / trunc)
    w = f(view["weight"])
    w_old = vol["weight"]
    w_sum = w_old + w
    with np.errstate(all="ignore"):
        vol["tsdf"][...] = np.where(live, (vol["tsdf"] * w_old + t * w) / w_sum, vol["tsdf"])
        if vol.get("color") is not None:
            pix = np.asarray(view["color"], dtype=f)[:, pyi, pxi]                             # [3,nz,ny,nx]
            for ch in range(3):
                c = vol["color"][..., ch]
                vol["color"][..., ch] = np.where(live, (c * w_old + pix[ch] * w) / w_sum, c)
    cap = f(np.inf) if view.get("max_weight") is None else f(view["max_weight"])
    vol["weight"][...] = np.where(live, np.minimum(w_sum, cap), w_old)
    return live, fragile


def empty_volume(dims, origin, voxel_size, sdf_trunc, with_color, dtype=np.float64):
    nx, ny, nz = dims
    return {"tsdf": np.ones((nz, ny, nx), dtype), "weight": np.zeros((nz, ny, nx), dtype),
            "color": np.zeros((nz, ny, nx, 3), dtype) if with_color else None,
            "origin": tuple(origin), "voxel_size": voxel_size, "sdf_trunc": sdf_trunc}


# ---- extraction ------------------------------------------------------------------------------------------------------
def _even(perm):
    return sum(1 for a in range(len(perm)) for b in range(a + 1, len(perm)) if perm[a] > perm[b]) % 2 == 0


def kuhn_tetrahedra():
    """The six tetrahedra of the unit cube around its diagonal, one per order of the axes (lexicographic), each as four
    corner offsets with the middle two swapped where needed to make det [v1 - v0, v2 - v0, v3 - v0] positive."""
    tets = []
    for axes in itertools.permutations(range(3)):
        path = [np.zeros(3, dtype=np.int64)]
        for a in axes:
            step = path[-1].copy()
            step[a] += 1
            path.append(step)
        if np.linalg.det(np.array([path[n] - path[0] for n in (1, 2, 3)], dtype=np.float64)) < 0:
            path[1], path[2] = path[2], path[1]
        tets.append([tuple(int(c) for c in p) for p in path])
    return tets


def _tet_triangles(inside):
    """Triangles of a positively oriented tetrahedron, as triples of (local, local) edges, for the rule of DESIGN.md
    §7.14.  ``inside``: four bools."""
    ins = [n for n in range(4) if inside[n]]
    outs = [n for n in range(4) if not inside[n]]
    if len(ins) in (0, 4):
        return []
    if len(ins) == 2:
        P, Q = ins
        R, S = outs
        if not _even((P, Q, R, S)):
            R, S = S, R
        return [((P, R), (P, S), (Q, S)), ((P, R), (Q, S), (Q, R))]
    A = ins[0] if len(ins) == 1 else outs[0]
    B, C, D = [n for n in range(4) if n != A]
    if not _even((A, B, C, D)):
        C, D = D, C
    return [((A, B), (A, C), (A, D))] if len(ins) == 1 else [((A, B), (A, D), (A, C))]


def extract(vol, min_weight=1e-6, dtype=np.float64):
    """-> (vertices [V,3], faces int64 [F,3], colors [V,3] or None) in the order of ``TSDFVolume.extract_mesh``."""
    f = dtype
    tsdf, weight, color = vol["tsdf"], vol["weight"], vol.get("color")
    nz, ny, nx = tsdf.shape
    ok = weight >= min_weight
    inside = tsdf < 0
    sl = lambda a, d: a[d[2]:nz - 1 + d[2], d[1]:ny - 1 + d[1], d[0]:nx - 1 + d[0]]         # noqa: E731
    corners = list(itertools.product((0, 1), repeat=3))
    processed = np.logical_and.reduce([sl(ok, c) for c in corners])
    n_in = np.sum([sl(inside, c).astype(np.int64) for c in corners], axis=0)
    tets = kuhn_tetrahedra()
    lin = lambda i, j, k: (k * ny + j) * nx + i                                            # noqa: E731
    tri_keys = []
    for k, j, i in zip(*np.nonzero(processed & (n_in > 0) & (n_in < 8))):                  # C order = cube linear index
        for tet in tets:
            pts = [(i + c[0], j + c[1], k + c[2]) for c in tet]
            for tri in _tet_triangles([bool(inside[p[2], p[1], p[0]]) for p in pts]):
                keys = []
                for a, b in tri:
                    lo, hi = sorted((pts[a], pts[b]), key=lambda p: lin(*p))
                    keys.append((lin(*lo), DIRECTIONS.index(tuple(int(h - l) for l, h in zip(lo, hi))), lo, hi))
                tri_keys.append(keys)
    order = sorted({(key[0], key[1]): key for tri in tri_keys for key in tri}.items())
    index = {kd: n for n, (kd, _) in enumerate(order)}
    faces = np.array([[index[(key[0], key[1])] for key in tri] for tri in tri_keys], dtype=np.int64).reshape(-1, 3)
    vertices = np.zeros((len(order), 3), dtype=f)
    colors = None if color is None else np.zeros((len(order), 3), dtype=f)
    o, vs = [f(v) for v in vol["origin"]], f(vol["voxel_size"])
    for n, (_, (_, _, lo, hi)) in enumerate(order):
        ta, tb = f(tsdf[lo[2], lo[1], lo[0]]), f(tsdf[hi[2], hi[1], hi[0]])
        s = ta / (ta - tb)
        for a in range(3):
            pa, pb = o[a] + vs * f(lo[a]), o[a] + vs * f(hi[a])
            vertices[n, a] = pa + (pb - pa) * s
        if colors is not None:
            ca, cb = color[lo[2], lo[1], lo[0]].astype(f), color[hi[2], hi[1], hi[0]].astype(f)
            colors[n] = ca + (cb - ca) * s
    return vertices, faces, colors


# ---- mesh properties (independent of any oracle) --------------------------------------------------------------------------
def directed_edge_counts(faces):
    counts = {}
    for a, b, c in np.asarray(faces).tolist():
        for e in ((a, b), (b, c), (c, a)):
            counts[e] = counts.get(e, 0) + 1
    return counts


def assert_closed_oriented_sphere(vertices, faces):
    """Every undirected edge lies in exactly two faces, once in each direction; V - E + F = 2; positive signed volume."""
    counts = directed_edge_counts(faces)
    assert counts and all(n == 1 for n in counts.values()), "a directed edge is used twice: inconsistent orientation"
    assert all((b, a) in counts for a, b in counts), "an edge has no opposite: the mesh is open"
    V, E, F = len(vertices), len(counts) // 2, len(faces)
    assert len(np.unique(np.asarray(faces))) == V, "an emitted vertex is not referenced"
    assert V - E + F == 2, f"Euler characteristic {V - E + F}"
    assert signed_volume(vertices, faces) > 0


def signed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    return float(np.einsum("ni,ni->n", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


# ---- shared inputs ---------------------------------------------------------------------------------------------------
SPHERE_DIMS, SPHERE_R, SPHERE_TRUNC = (24, 20, 22), 8.0, 3.0
SPHERE_C = (11.5 + math.sqrt(2) / 10, 9.5 - math.sqrt(3) / 10, 10.5 + math.pi / 20)       # off-centre by irrational fractions


def sphere_field(with_color=True):
    """The analytic sphere clamp((|p - c| - r) / trunc, -1, 1), weight 1, voxel 1, origin 0, as float32 fields (what the
    device holds) and a smooth colour field."""
    nx, ny, nz = SPHERE_DIMS
    kk, jj, ii = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    dist = np.sqrt((ii - SPHERE_C[0]) ** 2 + (jj - SPHERE_C[1]) ** 2 + (kk - SPHERE_C[2]) ** 2)
    tsdf = np.clip((dist - SPHERE_R) / SPHERE_TRUNC, -1.0, 1.0).astype(np.float32)
    assert not np.any(tsdf == 0)
    color = np.stack((ii / nx, jj / ny, 0.5 + 0.5 * np.sin(kk * 0.7)), axis=-1).astype(np.float32) if with_color else None
    return {"tsdf": tsdf, "weight": np.ones_like(tsdf), "color": color, "origin": (0.0, 0.0, 0.0), "voxel_size": 1.0,
            "sdf_trunc": SPHERE_TRUNC}


PLANE_DIMS = (17, 9, 21)


def plane_field():
    """A tilted plane through a 17 x 9 x 21 grid; weight 0 on an irregular region, so processed and unprocessed cubes
    alternate; one sample exactly 0 (it counts as outside)."""
    nx, ny, nz = PLANE_DIMS
    kk, jj, ii = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    tsdf = np.clip((0.31 * (ii - 8.2) + 0.83 * (jj - 4.1) - 0.17 * (kk - 10.3)) / 2.0, -1.0, 1.0).astype(np.float32)
    weight = np.ones_like(tsdf)
    weight[((ii * 7 + jj * 3 + kk * 5) % 11 == 0) | ((ii > 11) & (kk % 4 == 1))] = 0.0
    on = np.argmin(np.where(weight > 0, np.abs(tsdf), 9.0))
    tsdf.reshape(-1)[on] = 0.0
    return {"tsdf": tsdf, "weight": weight, "color": None, "origin": (-1.25, 0.5, 2.0), "voxel_size": 0.125,
            "sdf_trunc": 0.25}


CASE_DIMS, CASE_VOXEL, CASE_TRUNC, CASE_MAX_DEPTH = (19, 13, 11), 0.25, 0.75, 6.6
CASE_W, CASE_H, CASE_F = 37, 29, 30.0
# float32 values: what the device receives, so the float64 truth starts from the same inputs
CASE_ORIGIN = tuple(float(np.float32(v)) for v in (-2.25 + math.sqrt(2) / 50, -1.5 + math.sqrt(3) / 70, 4.75 + math.pi / 100))


def _raycast(M, W, H, fx, fy):
    """float64 depth (view-space z) of a sphere and a tilted plane, per pixel; 0 where the ray hits neither."""
    A, b = M[:3, :3], M[3, :3]
    c_v = np.array([0.1, -0.05, 6.07]) @ A + b
    n_w = np.array([0.1, 1.0, 0.05]) / np.linalg.norm([0.1, 1.0, 0.05])
    n_v, p0_v = n_w @ A, np.array([0.0, 0.9, 6.0]) @ A + b
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack(((xs - (W - 1) / 2.0) / fx, (ys - (H - 1) / 2.0) / fy, np.ones_like(xs)), axis=-1)
    qa, qb, qc = (d * d).sum(-1), -2.0 * (d @ c_v), c_v @ c_v - 0.9 ** 2
    disc = qb * qb - 4 * qa * qc
    with np.errstate(all="ignore"):
        s_sphere = np.where(disc > 0, (-qb - np.sqrt(np.abs(disc))) / (2 * qa), np.inf)
        s_plane = (n_v @ p0_v) / (d @ n_v)
    s_sphere = np.where(s_sphere > 0, s_sphere, np.inf)
    s_plane = np.where(s_plane > 0, s_plane, np.inf)
    s = np.minimum(s_sphere, s_plane)
    return np.where(np.isfinite(s), s, 0.0)


def integration_case():
    """The inputs of the integration tests: three orbit cameras at 37 x 29 around a 19 x 13 x 11 volume; per view the
    float32 depth map (ray-cast in float64; some pixels invalid) and a colour image.  -> (cameras, views): ``views`` are
    the dicts ``integrate`` takes, without weight / max_weight."""
    from mvs_gaussian_splatting_amd.synthetic import orbit_camera
    rng = np.random.default_rng(11)
    cameras, views = [], []
    for n in range(3):
        cam = orbit_camera(n, 3, CASE_W, CASE_H, CASE_F, CASE_F)
        M = cam.world_view_transform.double().numpy()
        fx = float(np.float32(CASE_W / (2.0 * math.tan(cam.FoVx * 0.5))))          # rounded as the binding rounds them
        fy = float(np.float32(CASE_H / (2.0 * math.tan(cam.FoVy * 0.5))))
        depth = _raycast(M, CASE_W, CASE_H, fx, fy).astype(np.float32)
        depth[(np.arange(CASE_H)[:, None] * 5 + np.arange(CASE_W)[None, :] * 3) % 17 == 0] = 0.0       # invalid pixels
        depth[3:6, 20:26] = 0.0
        color = rng.random((3, CASE_H, CASE_W)).astype(np.float32)
        cameras.append(cam)
        views.append({"viewmatrix": cam.world_view_transform.numpy().astype(np.float64), "W": CASE_W, "H": CASE_H,
                      "fx": fx, "fy": fy, "depth": depth, "color": color, "max_depth": CASE_MAX_DEPTH})
    return cameras, views


def run_case(views, with_color, max_weight=None, dtype=np.float64):
    """The three views in order into a fresh volume -> (volume, updated by any view, fragile in any view)."""
    vol = empty_volume(CASE_DIMS, CASE_ORIGIN, CASE_VOXEL, CASE_TRUNC, with_color, dtype)
    touched = np.zeros(vol["tsdf"].shape, bool)
    fragile = np.zeros(vol["tsdf"].shape, bool)
    for view in views:
        v = dict(view, weight=1.0, max_weight=max_weight)
        if not with_color:
            v["color"] = None
        if dtype == np.float32:
            v["viewmatrix"] = v["viewmatrix"].astype(np.float32)
            v["fx"], v["fy"] = np.float32(v["fx"]), np.float32(v["fy"])
        up, fr = integrate(vol, v, dtype)
        touched |= up
        fragile |= fr
    return vol, touched, fragile
