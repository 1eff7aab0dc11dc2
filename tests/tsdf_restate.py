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


# ---- integration past one x-chunk: ragged tails, the frustum tests, unequal weights, a pre-loaded state -----------------
WIDE_DIMS = ((65, 5, 3), (130, 3, 3), (128, 2, 3))       # one live lane in chunk 2; three chunks and a row tail; two full chunks
WIDE_LENGTH = 2.75                                       # x extent of every volume, so the poses below serve all three
WIDE_WEIGHTS = (0.5, 2.25, 1.0)                          # dyadic: every weight sum is exact in float32
WIDE_MAX_WEIGHT = 3.0
WIDE_SIZES = ((23, 45), (31, 27), (13, 11))              # (W, H) per view: odd, no multiple of 16
CLASSES = ("near", "behind", "off_left", "off_right", "off_top", "off_bottom", "zero", "negative", "nan", "far",
           "behind_surface", "t_one", "t_below_one")


def _rotation(axis, degrees):
    """Rodrigues' rotation matrix about ``axis``."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    t = math.radians(degrees)
    return np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)


def _raycast_surface(M, W, H, fx, fy, centre, radius, normal=None):
    """float64 depth (view-space z) per pixel of the nearest of a sphere round ``centre`` (either root: the camera may sit
    inside it) and, with ``normal``, the plane through ``centre``; 0 where the ray meets neither."""
    A, b = M[:3, :3], M[3, :3]
    c_v = np.asarray(centre) @ A + b
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack(((xs - (W - 1) / 2.0) / fx, (ys - (H - 1) / 2.0) / fy, np.ones_like(xs)), axis=-1)
    qa, qb, qc = (d * d).sum(-1), -2.0 * (d @ c_v), c_v @ c_v - radius ** 2
    disc = qb * qb - 4 * qa * qc
    with np.errstate(all="ignore"):
        root = np.sqrt(np.abs(disc))
        hits = [np.where(disc > 0, (-qb - root) / (2 * qa), np.inf), np.where(disc > 0, (-qb + root) / (2 * qa), np.inf)]
        if normal is not None:
            n_v = (np.asarray(normal) / np.linalg.norm(normal)) @ A
            hits.append((n_v @ c_v) / (d @ n_v))
    s = np.minimum.reduce([np.where(h > 0, h, np.inf) for h in hits])
    return np.where(np.isfinite(s), s, 0.0)


def wide_case(n):
    """Volume ``WIDE_DIMS[n]`` (x extent 2.75, centred near the world origin) under three free-pose views, every rotation
    about an axis that is no coordinate axis:
      0  an overview from the side, the long axis upright in a 23 x 45 image and a little longer than it (points leave
         through the top and the bottom alone); max_depth cuts the far quarter of the surface;
      1  a camera inside the volume that looks obliquely along it: half the grid is behind it, a slab has 0 < z <= 0.2;
         no max_depth, a few +inf pixels;
      2  a close camera with a 13 x 11 image, the long axis level: most points leave through the left and the right;
         max_depth lies beyond every pixel.
    Depth: a sphere and a plane through the volume's centre, ray-cast in float64, then exact 0, negative and NaN pixels.
    Views 0 and 1 see a plane tilted against all of them; view 2 sees one almost square to its axis, so that the whole
    slab of the volume lies inside the truncation band there and the pixel a bounds test relaxed by one would read -- the
    far end of the neighbouring row -- would update.  View 0 carries ``guard``, float32 [2,W]: the rows to be laid
    directly above and below its map in memory (valid depth, at max_depth), which is what a relaxed top or bottom test
    would read.  Volume 1 has sdf_trunc 0.3 > 0.2, so a point at 0.2 < z <= 0.3 over a 0 pixel has sdf >= -sdf_trunc and
    only the ``d > 0`` test skips it; a negative depth here is always below -sdf_trunc as well.
    -> dict(dims, origin, voxel_size, sdf_trunc, cameras, views, preload); ``views`` as ``integrate`` takes them, without
    max_weight; ``preload``: float32 fields (random tsdf in [-1, 1], weights in {0, 0.5, 4}, colours)."""
    from mvs_gaussian_splatting_amd.synthetic import SyntheticCamera
    nx, ny, nz = dims = WIDE_DIMS[n]
    rng = np.random.default_rng(40 + n)
    vs = float(np.float32(WIDE_LENGTH / (nx - 1) * (1.0 + math.sqrt(2) / 300)))
    trunc = float(np.float32(0.3 if n == 1 else 3.0 * 0.043))
    ext = np.array([nx - 1, ny - 1, nz - 1]) * vs
    origin = tuple(float(np.float32(v)) for v in -ext / 2 + np.array([math.sqrt(2) / 50, -math.sqrt(3) / 70, math.pi / 100]))
    centre = np.array(origin) + ext / 2
    L = ext[0]
    # camera axes in the world (columns: right, down, forward), then a tilt about a generic axis
    up_x = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])       # image y runs along world x
    level = np.eye(3)
    along = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])      # looks along world x
    # (camera axes in the world, tilted about a generic axis; the point the optical axis passes through; distance; fx, fy)
    poses = [(_rotation((3.0, 0.6, 0.5), 20.0 + 3 * n) @ up_x, centre + np.array([-0.04 * L, 0.0, 0.0]), 1.1 * L, 57.0, 55.0),
             (_rotation((0.3, 1.0, 0.4), 33.0 - 3 * n) @ along, centre + np.array([-0.3 * L, 0.3 * vs, -0.4 * vs]), 0.0, 21.0, 19.0),
             (_rotation((1.0, 0.5, 3.0), 27.0 + 3 * n) @ level, centre + np.array([-0.1 * L, 0.0, 0.0]), 0.5 * L, 20.0, 22.0)]
    normals = [(0.25, 0.1, 1.0), (0.25, 0.1, 1.0), poses[2][0][:, 2] + np.array([0.02, 0.05, -0.03])]
    cut = lambda d, q: float(np.float32(np.quantile(d[d > 0], q)))           # noqa: E731  (NaN > 0 is false)
    cameras, views = [], []
    for v, ((Rc2w, aim, dist, fx0, fy0), (W, H)) in enumerate(zip(poses, WIDE_SIZES)):
        pos = aim - dist * Rc2w[:, 2]
        cam = SyntheticCamera(W, H, fx0, fy0, R=Rc2w, T=-Rc2w.T @ pos)
        M = cam.world_view_transform.numpy().astype(np.float64)
        fx = float(np.float32(W / (2.0 * math.tan(cam.FoVx * 0.5))))               # rounded as the binding rounds them
        fy = float(np.float32(H / (2.0 * math.tan(cam.FoVy * 0.5))))
        depth = _raycast_surface(M, W, H, fx, fy, centre, 0.06 * L, normals[v]).astype(np.float32)
        code = (np.arange(H)[:, None] * 3 + np.arange(W)[None, :] * 5 + v) % 13
        depth[code == 1] = 0.0
        depth[code == 4] = -depth[code == 4] - np.float32(0.5)
        depth[code == 7] = np.nan
        if v == 1:
            depth[code == 10] = np.inf
        views.append({"viewmatrix": M, "W": W, "H": H, "fx": fx, "fy": fy, "depth": depth,
                      "color": rng.random((3, H, W)).astype(np.float32), "weight": WIDE_WEIGHTS[v],
                      "max_depth": None if v == 1 else cut(depth[:, W // 2], 0.75) if v == 0 else cut(depth, 1.0) + 0.0625})
        if v == 0:
            views[0]["guard"] = np.full((2, W), views[0]["max_depth"], np.float32)
        cameras.append(cam)
    preload = {"tsdf": rng.uniform(-1.0, 1.0, (nz, ny, nx)).astype(np.float32),
               "weight": rng.choice(np.array([0.0, 0.5, 4.0], np.float32), (nz, ny, nx)),
               "color": rng.random((nz, ny, nx, 3)).astype(np.float32)}
    return {"dims": dims, "origin": origin, "voxel_size": vs, "sdf_trunc": trunc, "cameras": cameras, "views": views,
            "preload": preload}


def wide_volume(case, with_color, preload, dtype=np.float64):
    vol = empty_volume(case["dims"], case["origin"], case["voxel_size"], case["sdf_trunc"], with_color, dtype)
    if preload:
        for name in ("tsdf", "weight") + (("color",) if with_color else ()):
            vol[name] = case["preload"][name].astype(dtype)
    return vol


def run_views(vol, views, dtype=np.float64, **override):
    """``views`` in order into ``vol`` (in place), each with ``override`` on top and, for float32, its view matrix and
    focal lengths rounded as the device holds them -> (updated by any view, fragile in any view, [updated per view])."""
    touched = np.zeros(vol["tsdf"].shape, bool)
    fragile = np.zeros(vol["tsdf"].shape, bool)
    per_view = []
    for view in views:
        v = dict(view, **override)
        if vol.get("color") is None:
            v["color"] = None
        if dtype == np.float32:
            v["viewmatrix"] = v["viewmatrix"].astype(np.float32)
            v["fx"], v["fy"] = np.float32(v["fx"]), np.float32(v["fy"])
        up, fr = integrate(vol, v, dtype)
        per_view.append(up)
        touched |= up
        fragile |= fr
    return touched, fragile, per_view


def run_wide(case, with_color, max_weight=None, preload=False, dtype=np.float64):
    """The case's views in order -> (volume, updated by any view, fragile in any view, [updated per view])."""
    vol = wide_volume(case, with_color, preload, dtype)
    return (vol,) + run_views(vol, case["views"], dtype, max_weight=max_weight)


def view_classes(vol, view):
    """Which test of the integration stops each grid point, in float64 and in the kernel's order -> dict of bool
    [nz,ny,nx]: CLASSES, ``only_<side>`` (off that side with the other coordinate inside the image), ``inf_update`` and
    ``updated``.  The four sides are counted one by one: a point off two sides is in both.  Also the points a slightly
    wrong kernel would update: ``relaxed_<side>``, one pixel outside that side alone, where the pixel at ``py * W + px``
    of the flat map (for view["guard"], of the map with its guard rows) is a valid depth that passes every later test; a
    read outside that memory counts as no update.  ``zero_visible``: over a 0 pixel with ``-z >= -sdf_trunc``."""
    nz, ny, nx = vol["tsdf"].shape
    M, vs, trunc, o = np.asarray(view["viewmatrix"], np.float64), vol["voxel_size"], vol["sdf_trunc"], vol["origin"]
    W, H = view["W"], view["H"]
    kk, jj, ii = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = np.stack((o[0] + vs * ii, o[1] + vs * jj, o[2] + vs * kk), axis=-1)
    x, y, z = (p @ M[:3, c] + M[3, c] for c in range(3))
    out = {"near": (z > 0) & (z <= 0.2), "behind": z < 0}
    front = z > 0.2
    with np.errstate(all="ignore"):
        px, py = np.floor(view["fx"] * x / z + (W - 1) / 2.0 + 0.5), np.floor(view["fy"] * y / z + (H - 1) / 2.0 + 0.5)
    in_x, in_y = (px >= 0) & (px < W), (py >= 0) & (py < H)
    out.update(off_left=front & (px < 0), off_right=front & (px >= W), off_top=front & (py < 0), off_bottom=front & (py >= H))
    out.update(only_left=out["off_left"] & in_y, only_right=out["off_right"] & in_y, only_top=out["off_top"] & in_x,
               only_bottom=out["off_bottom"] & in_x)
    seen = front & in_x & in_y
    d = np.asarray(view["depth"], np.float64)[np.where(seen, py, 0).astype(np.int64), np.where(seen, px, 0).astype(np.int64)]
    out.update(zero=seen & (d == 0), negative=seen & (d < 0), nan=seen & np.isnan(d))
    valid = seen & (d > 0)
    out["far"] = valid & (d > np.inf if view.get("max_depth") is None else d > view["max_depth"])
    sdf = d - z
    out["behind_surface"] = valid & ~out["far"] & (sdf < -trunc)
    out["updated"] = valid & ~out["far"] & ~out["behind_surface"]
    out.update(t_one=out["updated"] & (sdf / trunc >= 1), t_below_one=out["updated"] & (sdf / trunc < 1),
               inf_update=out["updated"] & np.isinf(d), zero_visible=out["zero"] & ~(-z < -trunc))
    guard = view.get("guard", np.full((2, W), np.nan))
    flat = np.concatenate((guard[0], np.asarray(view["depth"]).reshape(-1), guard[1])).astype(np.float64)
    for side, off in (("left", front & (px == -1) & in_y), ("right", front & (px == W) & in_y),
                      ("top", front & (py == -1) & in_x), ("bottom", front & (py == H) & in_x)):
        at = np.where(off, (py + 1) * W + px, 0).astype(np.int64)
        d = np.where((at >= 0) & (at < flat.size), flat[np.clip(at, 0, flat.size - 1)], np.nan)
        limit = np.inf if view.get("max_depth") is None else view["max_depth"]
        out["relaxed_" + side] = off & (d > 0) & ~(d > limit) & ~(d - z < -trunc)
    return out


# ---- extraction past one x-chunk: random signs, holes, signed zeros, a sphere across the chunk seam ----------------------
RANDOM_DIMS = ((65, 3, 7), (70, 6, 5), (130, 5, 3))


def random_field(n):
    """``tsdf ~ U(-1, 1)`` float32 on ``RANDOM_DIMS[n]``: every cube is mixed, several sheets meet in one cube.  About 3 %
    of the weights are 0, the rest in {1, 2, 3}; four samples each are exactly 0.0 and -0.0 (both outside); random
    colours; origin off zero and a voxel size that is no power of two."""
    nx, ny, nz = RANDOM_DIMS[n]
    rng = np.random.default_rng(70 + n)
    tsdf = rng.uniform(-1.0, 1.0, (nz, ny, nx)).astype(np.float32)
    weight = rng.choice(np.array([1.0, 2.0, 3.0], np.float32), (nz, ny, nx))
    weight[rng.random((nz, ny, nx)) < 0.03] = 0.0
    # signed zeros on weighted interior points, away from the holes' cubes where possible
    at = rng.choice(np.flatnonzero((weight > 0).reshape(-1)), 8, replace=False)
    tsdf.reshape(-1)[at[:4]] = 0.0
    tsdf.reshape(-1)[at[4:]] = -0.0
    return {"tsdf": tsdf, "weight": weight, "color": rng.random((nz, ny, nx, 3)).astype(np.float32),
            "origin": (0.37, -1.21, 2.05), "voxel_size": float(np.float32(0.137)), "sdf_trunc": 0.5}


SEAM_DIMS, SEAM_R = (96, 20, 22), 8.0
SEAM_C = (63.5 + math.sqrt(2) / 10, 9.5 - math.sqrt(3) / 10, 10.5 + math.pi / 20)


def seam_sphere_field():
    """``sphere_field``'s sphere in a 96 x 20 x 22 grid, centred near x = 64: the surface crosses i = 63 | 64, the border
    between the first two 64-point x-chunks of the kernels' launch."""
    nx, ny, nz = SEAM_DIMS
    kk, jj, ii = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    dist = np.sqrt((ii - SEAM_C[0]) ** 2 + (jj - SEAM_C[1]) ** 2 + (kk - SEAM_C[2]) ** 2)
    tsdf = np.clip((dist - SEAM_R) / SPHERE_TRUNC, -1.0, 1.0).astype(np.float32)
    assert not np.any(tsdf == 0)
    color = np.stack((ii / nx, jj / ny, 0.5 + 0.5 * np.sin(kk * 0.7)), axis=-1).astype(np.float32)
    return {"tsdf": tsdf, "weight": np.ones_like(tsdf), "color": color, "origin": (0.0, 0.0, 0.0), "voxel_size": 1.0,
            "sdf_trunc": SPHERE_TRUNC}


def mesh_census(vol, min_weight=1e-6):
    """What a field makes the extraction do, walking cubes and edges as ``extract`` does.  -> dict: ``patterns`` (set of the
    8-bit inside masks, corner c = x + 2y + 4z, of processed mixed cubes), ``tet_cases`` (set of (tetrahedron, 4-bit inside
    mask of its corners in ``kuhn_tetrahedra`` order) that emit), ``polarities`` (set of (direction, owner inside) of the
    emitted edges), ``keys`` (emitted (owner, direction), sorted), ``ends`` (int [V,2,3]: the (i, j, k) of both ends),
    ``orphans`` (crossed edges none of whose cubes is processed), ``shared`` (crossed edges held by a processed and an
    unprocessed cube)."""
    tsdf, weight = vol["tsdf"], vol["weight"]
    nz, ny, nx = tsdf.shape
    ok, inside = weight >= min_weight, tsdf < 0
    processed = np.zeros((nz, ny, nx), bool)                               # by base point; False where there is no cube
    sl = lambda a, d: a[d[2]:nz - 1 + d[2], d[1]:ny - 1 + d[1], d[0]:nx - 1 + d[0]]         # noqa: E731
    corners = [(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]
    processed[:nz - 1, :ny - 1, :nx - 1] = np.logical_and.reduce([sl(ok, c) for c in corners])
    bits = np.zeros((nz, ny, nx), np.int64)
    for c, off in enumerate(corners):
        bits[:nz - 1, :ny - 1, :nx - 1] |= sl(inside, off).astype(np.int64) << c
    mixed = processed & (bits != 0) & (bits != 255)
    patterns = set(np.unique(bits[mixed]).tolist())
    tet_cases = set()
    for t, tet in enumerate(kuhn_tetrahedra()):
        m = np.zeros_like(bits)
        for n, (x, y, z) in enumerate(tet):
            m |= ((bits >> (x + 2 * y + 4 * z)) & 1) << n
        tet_cases |= {(t, int(v)) for v in np.unique(m[mixed]) if v not in (0, 15)}
    found, polarities, orphans, shared = [], set(), 0, 0
    for d, (dx, dy, dz) in enumerate(DIRECTIONS):
        crossed = inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]
        for k, j, i in zip(*np.nonzero(crossed)):
            holders = [processed[k - oz, j - oy, i - ox] for ox, oy, oz in corners
                       if not (ox & dx or oy & dy or oz & dz) and i - ox >= 0 and j - oy >= 0 and k - oz >= 0
                       and i - ox + 1 < nx and j - oy + 1 < ny and k - oz + 1 < nz]
            if not any(holders):
                orphans += 1
                continue
            shared += not all(holders)
            found.append(((k * ny + j) * nx + i, d, i, j, k, i + dx, j + dy, k + dz))
            polarities.add((d, bool(inside[k, j, i])))
    found = np.array(sorted(found), np.int64).reshape(-1, 8)
    return {"patterns": patterns, "tet_cases": tet_cases, "polarities": polarities,
            "keys": found[:, :2], "ends": found[:, 2:].reshape(-1, 2, 3),
            "orphans": orphans, "shared": shared}


# ---- fusion and extraction together, across the chunk seam -----------------------------------------------------------------
FUSE_DIMS, FUSE_VOXEL, FUSE_TRUNC, FUSE_R = (80, 24, 23), 0.1, 0.3, 0.8
FUSE_ORIGIN = tuple(float(np.float32(v)) for v in (-6.2 + math.sqrt(2) / 100, -1.15 - math.sqrt(3) / 100, -1.1 + math.pi / 300))
FUSE_C = (0.13, 0.02, -0.01)                             # x index 63.2: the sphere spans i = 55 .. 71
FUSE_W, FUSE_H, FUSE_F = 81, 75, 90.0


def fusion_case():
    """Six cameras round an analytic sphere of radius 0.8 inside an 80 x 24 x 23 volume of 0.1 voxels, one along each
    signed axis and each tilted about a generic axis; float32 depth ray-cast in float64, 0 off the sphere.
    -> (cameras, views); weight 1, no limits, no colour."""
    from mvs_gaussian_splatting_amd.synthetic import SyntheticCamera
    bases = [np.eye(3), np.diag([-1.0, 1.0, -1.0]),                                                       # +z, -z
             np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]),                              # +x
             np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]),                              # -x
             np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]]),                              # +y
             np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])]                              # -y
    cameras, views = [], []
    for n, base in enumerate(bases):
        Rc2w = _rotation((1.0 + n, 2.0, 3.0 - n), 7.0 + 4 * n) @ base
        cam = SyntheticCamera(FUSE_W, FUSE_H, FUSE_F, FUSE_F, R=Rc2w, T=-Rc2w.T @ (np.array(FUSE_C) - 3.0 * Rc2w[:, 2]))
        M = cam.world_view_transform.numpy().astype(np.float64)
        fx = float(np.float32(FUSE_W / (2.0 * math.tan(cam.FoVx * 0.5))))
        fy = float(np.float32(FUSE_H / (2.0 * math.tan(cam.FoVy * 0.5))))
        depth = _raycast_surface(M, FUSE_W, FUSE_H, fx, fy, FUSE_C, FUSE_R).astype(np.float32)
        cameras.append(cam)
        views.append({"viewmatrix": M, "W": FUSE_W, "H": FUSE_H, "fx": fx, "fy": fy, "depth": depth, "color": None,
                      "weight": 1.0, "max_depth": None, "max_weight": None})
    return cameras, views


def run_fusion(views, dtype=np.float64):
    """``fusion_case``'s views into a fresh volume -> (volume, fragile in any view)."""
    vol = empty_volume(FUSE_DIMS, FUSE_ORIGIN, FUSE_VOXEL, FUSE_TRUNC, False, dtype)
    return vol, run_views(vol, views, dtype)[1]
