"""A numpy restatement of the mesh rasterizer of csrc/mesh_raster.hip (``mesh.rasterize_mesh``, ``mesh.face_view_counts``;
DESIGN.md §7.29), the inputs the tests run it on, and which pixels of a general scene no float32 implementation can be
held to.

The rule per face and view (csrc/mesh_raster_math.h), in the same operation order:

1. corners to view space in float32: ``xv = ((x M[0] + y M[4]) + z M[8]) + M[12]`` and likewise ``yv``, ``zv``;
2. ``zv > near`` for all three: as it is; for none: dropped; else Sutherland-Hodgman against ``z = near`` over the edges
   (0,1), (1,2), (2,0): emit the first corner if inside, then the intersection ``a + t (b - a)``,
   ``t = (near - za) / (zb - za)`` with ``a`` the inside end, ``z = near`` exactly; pieces (o0,o1,o2), (o0,o2,o3);
3. ``u = (fx xv) / zv + cx``, ``cx = (W - 1) / 2``; ``X = rint(u * 256)``; a piece with ``|rint| > 2^29`` or a value that
   is not finite is dropped and counted;
4. integers: ``edge(a, b, P) = (Xb - Xa)(Py - Ya) - (Yb - Ya)(Px - Xa)``; ``A = edge(p0, p1, p2)``; 0 drops; negative
   swaps p1 and p2 (with ``cull_backfaces`` a positive one is dropped); a centre ``(256 ix, 256 iy)`` is covered when
   every ``E_k > 0`` or ``E_k = 0`` on an edge with ``dy < 0`` or ``dy = 0 and dx > 0``;
5. ``lambda_k = float64(E_k) / float64(A)``; ``1/z = (l0 / z0 + l1 / z1) + l2 / z2`` in float64; ``z`` = its reciprocal
   rounded to float32, clamped to the piece's ``[min z_k, max z_k]``;
6. per pixel the smallest ``float_bits(z) << 32 | face`` wins; depth 0 and id -1 where nothing landed.

``dtype=np.float64`` evaluates steps 1-3 in float64 on the same float32 inputs.  A piece is FRAGILE when that changes its
clipping or snaps one of its corners to a different integer; a pixel is fragile when a fragile piece covers its centre in
either evaluation.  Everywhere else the float32 steps decide what float64 decides, and a float32 implementation must
give the restatement's bits.
"""
import types

import numpy as np

from mesh_cull_restate import camera, focal, look_at  # noqa: F401  (the tests take the cameras from here)

NEAR = 0.25
COORD_MAX = 2.0 ** 29
LANE_PIXELS, DRAIN_WAVES = 16, 256          # include/gsr.h: GSR_RASTER_LANE_PIXELS, GSR_RASTER_DRAIN_WAVES


# ---- steps 1 to 3 ------------------------------------------------------------------------------------------------------
def view_space(vertices, cam, t=np.float32):
    M = cam.world_view_transform.numpy().astype(np.float32).reshape(-1).astype(t)
    x, y, z = (np.asarray(vertices)[:, a].astype(np.float32).astype(t) for a in range(3))
    with np.errstate(all="ignore"):
        xv = ((x * M[0] + y * M[4]) + z * M[8]) + M[12]
        yv = ((x * M[1] + y * M[5]) + z * M[9]) + M[13]
        zv = ((x * M[2] + y * M[6]) + z * M[10]) + M[14]
    return np.stack((xv, yv, zv), axis=1)


def clip(v, near):
    """v: [3,3] view-space corners of dtype t -> the 0, 3 or 4 clipped corners, as a list of (x, y, z)."""
    t = v.dtype.type
    near = t(near)
    inside = [bool(v[k, 2] > near) for k in range(3)]
    if all(inside):
        return [tuple(v[k]) for k in range(3)]
    if not any(inside):
        return []
    out = []
    with np.errstate(all="ignore"):
        for i in range(3):
            j = (i + 1) % 3
            if inside[i]:
                out.append(tuple(v[i]))
            if inside[i] != inside[j]:
                a, b = (v[i], v[j]) if inside[i] else (v[j], v[i])
                s = (near - a[2]) / (b[2] - a[2])
                out.append((a[0] + s * (b[0] - a[0]), a[1] + s * (b[1] - a[1]), near))
    return out


def snap(corner, cam, t):
    """One corner to sub-pixel integers -> (X, Y) or None when it is out of range."""
    H, W, fx, fy = focal(cam)
    fx, fy = t(fx), t(fy)
    cx, cy = (t(W) - t(1)) * t(0.5), (t(H) - t(1)) * t(0.5)
    with np.errstate(all="ignore"):
        u = (fx * corner[0]) / corner[2] + cx
        v = (fy * corner[1]) / corner[2] + cy
        rx, ry = np.rint(u * t(256)), np.rint(v * t(256))
    if not (abs(rx) <= COORD_MAX and abs(ry) <= COORD_MAX):           # a NaN fails
        return None
    return int(rx), int(ry)


def pieces_of(vertices, faces, cam, near=NEAR, dtype=np.float32):
    """Steps 1-3 -> per face a list of pieces ``(X [3], Y [3], z float32 [3])`` or ``None`` for a dropped one."""
    vs = view_space(vertices, cam, dtype)
    out = []
    for f in np.asarray(faces, dtype=np.int64):
        poly = clip(vs[f], np.float32(near))
        tris = [] if len(poly) < 3 else [(poly[0], poly[1], poly[2])] + ([(poly[0], poly[2], poly[3])] if len(poly) == 4 else [])
        mine = []
        for tri in tris:
            pts = [snap(c, cam, dtype) for c in tri]
            if any(p is None for p in pts):
                mine.append(None)
            else:
                mine.append(([p[0] for p in pts], [p[1] for p in pts], np.array([c[2] for c in tri], dtype=np.float32)))
        out.append(mine)
    return out


# ---- steps 4 to 6 ------------------------------------------------------------------------------------------------------
def edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def top_left(dx, dy):
    return dy < 0 or (dy == 0 and dx > 0)


def normalise(piece, cull_backfaces=False):
    """-> (X, Y, z, A) with A > 0, or None when the piece has no area or is culled."""
    X, Y, z = piece
    A = edge(X[0], Y[0], X[1], Y[1], X[2], Y[2])
    if A == 0:
        return None
    if A < 0:
        return [X[0], X[2], X[1]], [Y[0], Y[2], Y[1]], z[[0, 2, 1]], -A
    return None if cull_backfaces else (list(X), list(Y), z, A)


def box(X, Y, W, H):
    return (max(-(-min(X) // 256), 0), min(max(X) // 256, W - 1), max(-(-min(Y) // 256), 0), min(max(Y) // 256, H - 1))


def cover(piece, W, H, cull_backfaces=False):
    """Steps 4 and 5 of one piece -> (iy, ix, z float32) of the covered centres (three 1-D arrays)."""
    none = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32))
    n = normalise(piece, cull_backfaces)
    if n is None:
        return none
    X, Y, z, A = n
    x0, x1, y0, y1 = box(X, Y, W, H)
    if x0 > x1 or y0 > y1:
        return none
    iy, ix = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    px, py = ix * 256, iy * 256
    inside = np.ones(ix.shape, dtype=bool)
    E = []
    for a, b in ((1, 2), (2, 0), (0, 1)):
        e = edge(X[a], Y[a], X[b], Y[b], px, py)
        inside &= (e > 0) | ((e == 0) & top_left(X[b] - X[a], Y[b] - Y[a]))
        E.append(e)
    iy, ix = iy[inside], ix[inside]
    lam = [e[inside].astype(np.float64) / np.float64(A) for e in E]
    z64 = z.astype(np.float64)
    with np.errstate(all="ignore"):
        inv = (lam[0] / z64[0] + lam[1] / z64[1]) + lam[2] / z64[2]
        zf = (1.0 / inv).astype(np.float32)
    zf = np.where(zf < z.min(), z.min(), zf)
    zf = np.where(zf > z.max(), z.max(), zf).astype(np.float32)
    return iy, ix, zf


NONE_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def rasterize(vertices, faces, cam, near=NEAR, cull_backfaces=False, pieces=None):
    """-> a namespace: ``depth`` float32 [H,W], ``face_id`` int32 [H,W], ``keys`` uint64 [H,W], ``dropped``, ``layers``
    int32 [H,W] (how many pieces cover each centre) and ``queued`` (the pieces whose box exceeds LANE_PIXELS)."""
    H, W, _, _ = focal(cam)
    pieces = pieces_of(vertices, faces, cam, near) if pieces is None else pieces
    keys = np.full((H, W), NONE_KEY, dtype=np.uint64)
    layers = np.zeros((H, W), dtype=np.int32)
    dropped = queued = 0
    for f, mine in enumerate(pieces):
        for piece in mine:
            if piece is None:
                dropped += 1
                continue
            n = normalise(piece, cull_backfaces)
            if n is not None:
                x0, x1, y0, y1 = box(n[0], n[1], W, H)
                queued += x0 <= x1 and y0 <= y1 and (x1 - x0 + 1) * (y1 - y0 + 1) > LANE_PIXELS
            iy, ix, z = cover(piece, W, H, cull_backfaces)
            key = z.view(np.uint32).astype(np.uint64) << np.uint64(32) | np.uint64(f)
            keys[iy, ix] = np.minimum(keys[iy, ix], key)
            layers[iy, ix] += 1
    hit = keys != NONE_KEY
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0)).astype(np.float32)
    face_id = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return types.SimpleNamespace(depth=depth, face_id=face_id, keys=keys, dropped=dropped, layers=layers, queued=queued)


def fragile_pixels(vertices, faces, cam, near=NEAR):
    """bool [H,W]: the centres that a piece covers, in float32 or in float64, whose clipping or snapping float64 changes."""
    H, W, _, _ = focal(cam)
    p32, p64 = pieces_of(vertices, faces, cam, near, np.float32), pieces_of(vertices, faces, cam, near, np.float64)
    out = np.zeros((H, W), dtype=bool)
    for a, b in zip(p32, p64):
        same = len(a) == len(b) and all((p is None) == (q is None) and (p is None or (p[0] == q[0] and p[1] == q[1]))
                                        for p, q in zip(a, b))
        if same:
            continue
        for piece in a + b:
            if piece is not None:
                iy, ix, _ = cover(piece, W, H)
                out[iy, ix] = True
    return out


def face_counts(vertices, faces, cameras, near=NEAR):
    counts = np.zeros(len(faces), dtype=np.int32)
    for cam in cameras:
        ids = rasterize(vertices, faces, cam, near).face_id
        counts[np.unique(ids[ids >= 0])] += 1
    return counts


# ---- inputs ------------------------------------------------------------------------------------------------------------
def soup_mesh(tris):
    """[F,3,3] corners -> (vertices float32 [3F,3], faces int32 [F,3]): no vertex is shared."""
    tris = np.asarray(tris, dtype=np.float32)
    return tris.reshape(-1, 3).copy(), np.arange(3 * len(tris), dtype=np.int32).reshape(-1, 3)


def dyadic_camera(W, H, f=16.0, permute=False):
    """Identity, or the axis permutation (xv, yv, zv) = (y, z, x); fx = fy = f, a power of two."""
    M = np.eye(4)
    if permute:
        M = np.zeros((4, 4))
        M[1, 0] = M[2, 1] = M[0, 2] = M[3, 3] = 1.0
    return camera(M, W, H, f, f), permute


def to_world(view_tris, permute):
    """View-space corners to the world of dyadic_camera: exact, a permutation of the coordinates."""
    t = np.asarray(view_tris, dtype=np.float64)
    return t[..., [2, 0, 1]] if permute else t


def dyadic_soup(W=97, H=61, F=2000, seed=3, permute=False):
    """About F triangles for which steps 1-3 are exact in float32: xv, yv multiples of 1/64 with zv in {1, 2, 4}, or on a
    coarser grid that keeps xv / zv on it -- so fx xv / zv with fx = 16 is a multiple of 1/16 pixel and the snap is exact.
    With them: faces behind the camera, faces crossing ``near`` = 0.25 with one and with two corners inside (their
    far corners at z = 1 and near ones at z = -0.5: t = 1/2, exact), zero-area faces, a NaN corner, and coincident
    duplicates under different indices."""
    rng = np.random.default_rng(seed)
    cam, permute = dyadic_camera(W, H, 16.0, permute)
    tris = []
    for _ in range(F - 160):
        z = float(rng.choice((1.0, 2.0, 4.0)))
        # centre anywhere in the image and a little outside, size up to a few pixels; one depth per face keeps 1/z exact
        c = np.array((rng.integers(-60, W + 60), rng.integers(-40, H + 40)))
        c = (c - np.array(((W - 1) / 2, (H - 1) / 2))) * z / 16.0
        c = np.round(c * 64) / 64
        d = rng.integers(-24, 25, (3, 2)) * z / 64.0
        zs = np.full(3, z) if rng.random() < 0.7 else rng.choice((1.0, 2.0, 4.0), 3)
        tris.append(np.column_stack((c + d, zs)))
    base = len(tris)
    for k in range(40):                                               # behind the camera, and behind the near plane
        tris.append(np.column_stack((rng.integers(-64, 65, (3, 2)) / 64.0, np.full(3, (-1.0, 0.125, 0.25, 0.0)[k % 4]))))
    for k in range(60):                                               # crossing near: one inside (even k), two inside (odd k)
        xy = rng.integers(-11, 12, 2) / 16.0 * np.array((1.0, 0.625)) + rng.integers(-8, 9, (3, 2)) / 64.0
        zs = np.array((1.0, -0.5, -0.5)) if k % 2 == 0 else np.array((1.0, 1.0, -0.5))
        tris.append(np.column_stack((xy, np.roll(zs, k % 3))))
    for k in range(20):                                               # zero area: a repeated corner, or three on a line
        p = rng.integers(-64, 65, (2, 2)) / 16.0
        third = p[0] if k % 2 == 0 else 2 * p[1] - p[0]
        tris.append(np.column_stack((np.vstack((p, third)), np.full(3, 2.0))))
    for k in range(39):                                               # coincident duplicates of earlier faces
        tris.append(tris[7 * k + 3].copy())
    nan = np.column_stack((rng.integers(-64, 65, (3, 2)) / 64.0, np.full(3, 2.0)))
    nan[1, 0] = np.nan
    tris.append(nan)
    vertices, faces = soup_mesh(to_world(np.array(tris), permute))
    return types.SimpleNamespace(vertices=vertices, faces=faces, cam=cam, near=NEAR, base=base)


def general_soup(W=97, H=61, F=2000, seed=5):
    """The same counts with a random float32 pose and vertices: a look-at camera off every axis, triangles of a few pixels
    scattered through a slab in front of it, some of them crossing the near plane or lying behind the camera."""
    rng = np.random.default_rng(seed)
    eye = np.array((0.3, -0.2, -4.0)) + rng.normal(0, 0.1, 3)
    cam = camera(look_at(eye, (0.05, 0.02, 0.1), up=(0.08, 1.0, 0.03)), W, H, 52.3, 49.1)
    centres = np.column_stack((rng.uniform(-4.5, 4.5, F), rng.uniform(-3, 3, F), rng.uniform(-3.0, 3.0, F)))
    centres[:60, 2] = rng.uniform(-4.2, -3.4, 60)                     # around the camera's near plane and behind it
    size = rng.uniform(0.02, 0.3, (F, 1, 1))
    size[:60] = 0.8
    tris = centres[:, None, :] + rng.normal(0, 1, (F, 3, 3)) * size
    vertices, faces = soup_mesh(tris)
    return types.SimpleNamespace(vertices=vertices, faces=faces, cam=cam, near=NEAR)


def big_triangle_scene(W=70, H=50, seed=7):
    """One triangle that covers the whole image at z = 4, behind a layer of small ones at z = 1 and 2 (dyadic)."""
    rng = np.random.default_rng(seed)
    cam, _ = dyadic_camera(W, H, 16.0)
    tris = [np.array(((-40.0, -20.0, 4.0), (40.0, -20.0, 4.0), (0.0, 60.0, 4.0)))]
    for _ in range(400):
        z = float(rng.choice((1.0, 2.0)))
        c = (np.array((rng.integers(0, W), rng.integers(0, H))) - np.array(((W - 1) / 2, (H - 1) / 2))) * z / 16.0
        c = np.round(c * 64) / 64
        tris.append(np.column_stack((c + rng.integers(-20, 21, (3, 2)) * z / 64.0, np.full(3, z))))
    order = rng.permutation(len(tris))                                # the big one somewhere in the middle
    vertices, faces = soup_mesh(np.array(tris)[order])
    return types.SimpleNamespace(vertices=vertices, faces=faces, cam=cam, near=NEAR, big=int(np.nonzero(order == 0)[0][0]))


def queued_scene(W=64, H=48, F=300, seed=9):
    """About F triangles with 24 x 24-pixel boxes (dyadic, z = 1 or 2, either winding): every one exceeds the lane budget, and together they
    are more than the DRAIN_WAVES pieces that one pass of the drain grid takes."""
    rng = np.random.default_rng(seed)
    cam, _ = dyadic_camera(W, H, 16.0)
    tris = []
    for _ in range(F):
        z = float(rng.choice((1.0, 2.0)))
        x0, y0 = rng.integers(-8, W - 16), rng.integers(-8, H - 16)
        px = np.array(((x0, y0), (x0 + 24, y0 + rng.integers(0, 25)), (x0 + rng.integers(0, 25), y0 + 24)), dtype=np.float64)
        px[rng.integers(0, 3)] += rng.integers(0, 4, 2) / 4.0         # off the pixel grid, on the sub-pixel one
        xy = (px - np.array(((W - 1) / 2, (H - 1) / 2))) * z / 16.0
        tri = np.column_stack((xy, np.full(3, z)))
        tris.append(tri if rng.random() < 0.5 else tri[[0, 2, 1]])    # both windings
    vertices, faces = soup_mesh(np.array(tris))
    return types.SimpleNamespace(vertices=vertices, faces=faces, cam=cam, near=NEAR)


def quad(corners):
    """Four corners in order -> two triangles [2,3,3]."""
    c = np.asarray(corners, dtype=np.float64)
    return np.array(((c[0], c[1], c[2]), (c[0], c[2], c[3])))


def sphere_case(W=64, H=64, f=48.0):
    """The end-to-end case: the unit sphere at the origin seen by six cameras 4 away, one near every axis direction, and a
    32^3 volume of side 2.6 around it -> a namespace of ``cameras``, ``masks`` and ``depths`` (the analytic silhouette and
    depth of every view, ``mesh_cull_restate.sphere_maps``), ``origin``, ``voxel_size``, ``dims``, ``sdf_trunc``.  Every
    point just outside the sphere lies in front of it for the camera nearest its normal (at most 55 degrees off), so the
    fused field has no unobserved band along the surface."""
    from mesh_cull_restate import sphere_maps
    eyes = ((4, 0.3, 0.2), (-4, 0.2, -0.3), (0.3, 4, 0.2), (0.2, -4, 0.3), (0.2, 0.3, 4), (-0.3, 0.2, -4))
    cameras = [camera(look_at(e, (0, 0, 0), up=(0.1, 1.0, 0.05) if abs(e[1]) < 3 else (1.0, 0.1, 0.05)), W, H, f, f) for e in eyes]
    maps = [sphere_maps(c) for c in cameras]
    voxel = 2.6 / 31
    return types.SimpleNamespace(cameras=cameras, masks=[m for m, _ in maps], depths=[d for _, d in maps], origin=(-1.3,) * 3,
                                 voxel_size=voxel, dims=(32, 32, 32), sdf_trunc=3 * voxel)


def erode(mask):
    """Binary erosion by the 3 x 3 square; pixels outside the image count as unset."""
    m = np.pad(np.asarray(mask) != 0, 1)
    out = np.ones(np.asarray(mask).shape, dtype=bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out &= m[dy:dy + out.shape[0], dx:dx + out.shape[1]]
    return out
