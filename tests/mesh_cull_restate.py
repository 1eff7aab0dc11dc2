"""A numpy restatement of the view culling of csrc/mesh_cull.hip (``mesh.vertex_view_counts``, ``mesh.cull_mesh_by_views``,
``mesh.dilate_mask``), the inputs the tests run it on, and which (vertex, view) pairs no float32
implementation can be held to.

The rule per vertex ``(x, y, z)`` and view (csrc/mesh_cull_math.h)::

    (xv, yv, zv) = ((x M[0] + y M[4]) + z M[8]) + M[12], ...            row-vector convention
    next view unless zv > near
    cx = (W - 1) / 2, cy = (H - 1) / 2;  u = (fx xv) / zv + cx, v = (fy yv) / zv + cy
    ix = floor(u + 0.5), iy = floor(v + 0.5);  next view unless 0 <= ix <= W - 1 and 0 <= iy <= H - 1
    in_view += 1
    next view if mask and mask[iy, ix] == 0
    next view if depth and not (ds = depth[iy, ix]; ds > 0 and zv - ds <= depth_tol ds)
    visible += 1

``counts(..., dtype=np.float32)`` evaluates it in float32 with exactly that operation order -- the bits the kernel must
give, which tests/mesh_cull_host_check.cpp confirms for the kernel's own body on the host; ``dtype=np.float64`` evaluates
it on the same float32 inputs in float64 and marks a pair FRAGILE when an operand of one of its comparisons lies within a
margin of flipping it:

* ``zv`` against ``near``: ``|zv - near| <= MARGIN_Z``.  The three products and sums of a coordinate of magnitude up to 8
  carry at most 4 roundings of 2^-24 relative each: below 2e-6.  MARGIN_Z = 1e-4 is fifty times that.
* ``u + 0.5`` and ``v + 0.5`` against an integer: the distance to the nearest integer ``<= MARGIN_PIX``.  ``u`` is at most
  about 100 here and is formed by a transform (2e-6 on xv and on zv, relative 1e-6 of a quotient near 100: 1e-4 / 4), a
  product, a quotient and two sums (4 roundings of 2^-24 x 128 = 3e-5): below 6e-5.  MARGIN_PIX = 5e-4 is eight times that.
* ``zv - ds`` against ``depth_tol ds``: ``|(zv - ds) - depth_tol ds| <= MARGIN_D ds``; both sides carry a few 2^-24 of
  values below 8: MARGIN_D = 1e-4 is a hundred times that.

A pair one of whose earlier comparisons is fragile is fragile whatever the later ones say.  On every other pair float32
and float64 take the same branches and read the same pixel, so the counts must agree exactly; on a vertex with ``k``
fragile views each count may differ by at most ``k``.
"""
import math
import types

import numpy as np

MARGIN_Z, MARGIN_PIX, MARGIN_D = 1e-4, 5e-4, 1e-4
NEAR, DEPTH_TOL = 0.2, 0.05          # the scene's: see scene()


# ---- cameras -----------------------------------------------------------------------------------------------------------
def camera(world_to_view, width, height, fx, fy):
    """A camera as the package takes it: ``world_view_transform`` (float32 4 x 4, row-vector convention), ``FoVx``,
    ``FoVy``, ``image_width``, ``image_height``; the FoVs are those of the focal lengths asked for."""
    import torch
    M = np.asarray(world_to_view, dtype=np.float64).astype(np.float32)
    return types.SimpleNamespace(world_view_transform=torch.from_numpy(M.copy()), image_width=int(width), image_height=int(height),
                                 FoVx=2.0 * math.atan(width / (2.0 * fx)), FoVy=2.0 * math.atan(height / (2.0 * fy)))


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """world_to_view in the row-vector convention (``p_view = [x, y, z, 1] @ M``) of a camera at ``eye`` looking at
    ``target``: +z forward, +x right, +y down."""
    eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, up))
    f = target - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    R = np.stack((r, d, f))                     # rows: the camera's axes in world coordinates
    M = np.eye(4)
    M[:3, :3] = R.T
    M[3, :3] = -R @ eye
    return M


def focal(cam):
    """(H, W, fx, fy) as ``mvs._focal`` forms them, the focal lengths rounded to float32 as the table holds them."""
    H, W = int(cam.image_height), int(cam.image_width)
    return H, W, np.float32(W / (2.0 * math.tan(float(cam.FoVx) * 0.5))), np.float32(H / (2.0 * math.tan(float(cam.FoVy) * 0.5)))


# ---- the rule ----------------------------------------------------------------------------------------------------------
def view_pairs(vertices, cam, mask=None, depth=None, near=NEAR, depth_tol=DEPTH_TOL, dtype=np.float32):
    """One view over all vertices -> ``(in_view bool [V], visible bool [V], fragile bool [V])``; ``fragile`` is all False
    unless ``dtype`` is float64."""
    t = dtype
    H, W, fx, fy = focal(cam)
    M = cam.world_view_transform.numpy().astype(np.float32).reshape(-1).astype(t)
    x, y, z = (vertices[:, a].astype(np.float32).astype(t) for a in range(3))
    fx, fy, near_t, tol = t(fx), t(fy), t(np.float32(near)), t(np.float32(depth_tol))
    with np.errstate(all="ignore"):
        xv = ((x * M[0] + y * M[4]) + z * M[8]) + M[12]
        yv = ((x * M[1] + y * M[5]) + z * M[9]) + M[13]
        zv = ((x * M[2] + y * M[6]) + z * M[10]) + M[14]
        front = zv > near_t
        cx, cy = (t(W) - t(1)) * t(0.5), (t(H) - t(1)) * t(0.5)
        u = (fx * xv) / zv + cx
        v = (fy * yv) / zv + cy
        ub, vb = u + t(0.5), v + t(0.5)
        ix, iy = np.floor(ub), np.floor(vb)
        inside = front & (ix >= 0) & (ix <= t(W) - t(1)) & (iy >= 0) & (iy <= t(H) - t(1))
        jx = np.where(inside, ix, 0).astype(np.int64)
        jy = np.where(inside, iy, 0).astype(np.int64)
        visible = inside.copy()
        if mask is not None:
            visible &= np.asarray(mask)[jy, jx] != 0
        fragile = np.zeros(len(x), dtype=bool)
        if depth is not None:
            ds = np.asarray(depth, dtype=np.float32)[jy, jx].astype(t)
            visible &= (ds > 0) & (zv - ds <= tol * ds)
        if t is np.float64:
            fragile |= np.abs(zv - near_t) <= MARGIN_Z
            fragile |= front & ((np.abs(ub - np.round(ub)) <= MARGIN_PIX) | (np.abs(vb - np.round(vb)) <= MARGIN_PIX))
            if depth is not None:
                fragile |= inside & (ds > 0) & (np.abs((zv - ds) - tol * ds) <= MARGIN_D * ds)
    return inside, visible, fragile


def counts(vertices, cameras, masks=None, depths=None, near=NEAR, depth_tol=DEPTH_TOL, dtype=np.float32):
    """-> ``(in_view int32 [V], visible int32 [V], fragile int32 [V])``: the counts over the views in table order and, per
    vertex, the number of its fragile views (float64 only)."""
    V = len(vertices)
    n_in, n_vis, n_frag = (np.zeros(V, dtype=np.int32) for _ in range(3))
    for k, cam in enumerate(cameras):
        a, b, c = view_pairs(vertices, cam, None if masks is None else masks[k], None if depths is None else depths[k],
                             near, depth_tol, dtype)
        n_in += a
        n_vis += b
        n_frag += c
    return n_in, n_vis, n_frag


def dilate(mask, radius):
    """Binary dilation by a ``(2 radius + 1)^2`` square as two separable passes, pixels outside the image 0 -> uint8 0 / 1."""
    m = (np.asarray(mask) != 0)

    def along(a, axis):
        a = np.moveaxis(a, axis, 0)
        n = a.shape[0]
        c = np.concatenate((np.zeros((1,) + a.shape[1:], dtype=np.int64), np.cumsum(a, axis=0, dtype=np.int64)))
        i = np.arange(n)
        out = c[np.minimum(i + radius, n - 1) + 1] - c[np.maximum(i - radius, 0)] > 0
        return np.moveaxis(out, 0, axis)
    return along(along(m, 1), 0).astype(np.uint8)


def face_keep(faces, vkeep):
    """keep[f] = all three corners kept; an index outside 0..V-1 is an error (the device sets a status bit)."""
    faces = np.asarray(faces, dtype=np.int64)
    if len(faces) and (faces.min() < 0 or faces.max() >= len(vkeep)):
        raise ValueError("a face index lies outside 0..V-1")
    k = np.asarray(vkeep) != 0
    return (k[faces[:, 0]] & k[faces[:, 1]] & k[faces[:, 2]]).astype(np.uint8) if len(faces) else np.zeros(0, np.uint8)


def cull(vertices, faces, colors, in_view, visible, min_views):
    """The culling end to end on given counts -> ``(vertices, faces, colors or None, kept_vertices, kept_faces)``: kept
    rows in their original order, faces re-indexed."""
    threshold = in_view if min_views == "all" else min_views
    keep = face_keep(faces, visible >= threshold) != 0
    kept_faces = np.nonzero(keep)[0]
    mark = np.zeros(len(vertices), dtype=bool)
    mark[np.asarray(faces, dtype=np.int64)[keep].reshape(-1)] = True
    kept_vertices = np.nonzero(mark)[0]
    rename = np.cumsum(mark) - 1
    out_faces = rename[np.asarray(faces, dtype=np.int64)[keep]].astype(np.int32).reshape(-1, 3)
    return (vertices[kept_vertices], out_faces, None if colors is None else colors[kept_vertices], kept_vertices,
            kept_faces)


# ---- the analytic scene ------------------------------------------------------------------------------------------------
def uv_sphere(center, radius, rings, segments):
    """A closed UV sphere -> (vertices float64 [2 + (rings - 1) segments, 3], faces int32)."""
    c = np.asarray(center, dtype=np.float64)
    verts = [c + (0.0, radius, 0.0)]
    for i in range(1, rings):
        th = math.pi * i / rings
        for j in range(segments):
            ph = 2.0 * math.pi * (j + 0.37) / segments
            verts.append(c + radius * np.array((math.sin(th) * math.cos(ph), math.cos(th), math.sin(th) * math.sin(ph))))
    verts.append(c - (0.0, radius, 0.0))
    at = lambda i, j: 1 + (i - 1) * segments + j % segments                                  # noqa: E731
    faces = [(0, at(1, j + 1), at(1, j)) for j in range(segments)]
    for i in range(1, rings - 1):
        for j in range(segments):
            faces += [(at(i, j), at(i, j + 1), at(i + 1, j)), (at(i, j + 1), at(i + 1, j + 1), at(i + 1, j))]
    last = len(verts) - 1
    faces += [(last, at(rings - 1, j), at(rings - 1, j + 1)) for j in range(segments)]
    return np.array(verts), np.array(faces, dtype=np.int32)


def sphere_maps(cam, center=(0.0, 0.0, 0.0), radius=1.0):
    """The unit sphere as the camera sees it -> (mask uint8 [H,W], depth float32 [H,W]): per pixel centre the ray
    ((px - cx) / fx, (py - cy) / fy, 1) against the sphere in float64; depth is the z of the first hit, 0 where it misses."""
    H, W, fx, fy = focal(cam)
    M = cam.world_view_transform.numpy().astype(np.float64)
    c = np.append(np.asarray(center, dtype=np.float64), 1.0) @ M
    py, px = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.stack(((px - (W - 1) * 0.5) / float(fx), (py - (H - 1) * 0.5) / float(fy), np.ones((H, W))), axis=-1)
    a, b, cc = (d * d).sum(-1), d @ c[:3], c[:3] @ c[:3] - radius * radius
    disc = b * b - a * cc
    hit = disc > 0
    t = np.where(hit, (b - np.sqrt(np.where(hit, disc, 0.0))) / a, 0.0)
    return hit.astype(np.uint8), np.where(hit & (t > 0), t, 0.0).astype(np.float32)


SIZES = ((70, 37, 40.0, 41.5), (48, 40, 45.0, 44.0))        # (W, H, fx, fy): two sizes, four focal lengths
TARGET = (0.05, 0.02, -0.03)                                # what the cameras look at: off the y axis, where six poles lie
RING, HEIGHT, ANGLE0 = 4.0, 0.3, 0.13                       # the cameras' ring about the y axis; view 0's angle on it
SPHERE, INNER, FLOATER = "sphere", "inner", "floater"


def ring_eye(angle):
    """A little above the ring's plane, so that the scene's symmetry puts no vertex on a pixel boundary."""
    return (RING * math.sin(angle), HEIGHT, RING * math.cos(angle))


def scene(S=5):
    """The analytic scene -> a namespace of float32 ``vertices [829,3]``, ``faces``, ``colors``, ``part`` (per vertex: which
    shell it belongs to, or "extra"), ``cameras``, ``masks``, ``depths`` (per camera a map or ``None``).

    The unit UV sphere at the origin; an inner shell of radius 0.5, which every camera outside sees only through the
    sphere; a floater of radius 0.1 at (0, 1.45, 0), 20 degrees off the axis of every ring camera and so inside its
    image but outside the sphere's silhouette (14.5 degrees), dilated or not.  Then vertices no face refers to: two
    behind view 0 (one of them closer to view 1 than its near plane), three far outside every image, one NaN row, one
    unreferenced point on the sphere.  829
    vertices: three 256-lane workgroups and a ragged tail of 61.

    Cameras: view 0 plain; view 1 at the same place as view 0 but facing away; then on a ring of radius 4 about the y axis, 0.3 above the origin, at
    angles that are no multiple of anything, each looking at a point just off the origin, cycling through: a mask (the silhouette
    dilated by 2), a depth map with a hole of zeros, both, plain.  Sizes and focal lengths alternate (SIZES).
    The depth test runs at ``DEPTH_TOL`` = 0.05: a pixel is 1 / 40 of its depth wide, so on a surface slanted by up to
    45 degrees the depth at the pixel's centre and at the vertex differ by up to half of that, 1.25 %."""
    sv, sf = uv_sphere((0, 0, 0), 1.0, 20, 30)              # 572 vertices
    iv, jf = uv_sphere((0, 0, 0), 0.5, 10, 18)              # 164
    fv, ff = uv_sphere((0, 1.45, 0), 0.1, 7, 14)            # 86
    eye0 = np.array(ring_eye(ANGLE0))
    extra = np.array([tuple(eye0 * 1.025), tuple(eye0 * 2.25), (0.0, 40.0, 0.0), (0.0, -40.0, 0.0), (np.nan, 0.0, 0.0),
                      (0.6, 0.0, 0.8), (5.0, 60.0, 1.0)])
    vertices = np.concatenate((sv, iv, fv, extra)).astype(np.float32)
    faces = np.concatenate((sf, jf + len(sv), ff + len(sv) + len(iv))).astype(np.int32)
    part = np.array([SPHERE] * len(sv) + [INNER] * len(iv) + [FLOATER] * len(fv) + ["extra"] * len(extra))
    rng = np.random.default_rng(5)
    colors = rng.random((len(vertices), 3), dtype=np.float32)
    cameras, masks, depths = [], [], []
    for k in range(S):
        W, H, fx, fy = SIZES[k % 2]
        if k == 1:
            M = look_at(eye0, 2.0 * eye0)                               # faces away from everything but one extra
            kind = 3
        else:
            ang = ANGLE0 if k == 0 else 0.4 + 2.0 * math.pi * (k - 1) / max(S - 1, 1) * 0.97
            M = look_at(ring_eye(ang), TARGET)
            kind = 3 if k == 0 else (k - 2) % 4
        cam = camera(M, W, H, fx, fy)
        mask, depth = sphere_maps(cam)
        if kind in (1, 2):
            depth[H // 2 - 3:H // 2 + 2, W // 2 + 4:W // 2 + 11] = 0.0        # a hole of zeros on the sphere
        cameras.append(cam)
        masks.append(dilate(mask, 2) if kind in (0, 2) else None)
        depths.append(depth if kind in (1, 2) else None)
    return types.SimpleNamespace(vertices=vertices, faces=faces, colors=colors, part=part, cameras=cameras, masks=masks,
                                 depths=depths, near=NEAR, depth_tol=DEPTH_TOL)


def dyadic():
    """A case in which every quantity of the rule is exact in float32, so float32, float64 and the device agree on every
    pair, fragile or not: axis-aligned cameras 4 away (zv = coordinate + 4 in {2, 4, 8}), focal lengths 32 and 16,
    coordinates that are multiples of 1 / 8, a checkerboard mask and a constant depth of 4 with ``depth_tol`` = 0.25, so
    that ``zv - ds`` in {-2, 0, 4} meets ``depth_tol ds`` = 1 exactly never and ``u + 0.5`` is an integer often."""
    g = np.arange(-12, 13) / 8.0
    xs, ys = np.meshgrid(g, g, indexing="ij")
    layers = [np.stack((xs, ys, np.full_like(xs, z)), axis=-1).reshape(-1, 3) for z in (-2.0, 0.0, 4.0)]
    vertices = np.concatenate(layers).astype(np.float32)                                  # 1875 vertices
    A = np.eye(4)
    A[3, 2] = 4.0                                                                         # zv = z + 4
    B = np.zeros((4, 4))
    B[2, 0], B[1, 1], B[0, 2], B[3, 2], B[3, 3] = -1.0, 1.0, 1.0, 4.0, 1.0                # xv = -z, yv = y, zv = x + 4
    cameras = [camera(A, 64, 33, 32.0, 16.0), camera(B, 17, 48, 16.0, 32.0), camera(A, 40, 40, 16.0, 16.0)]
    yy, xx = np.mgrid[0:33, 0:64]
    masks = [((xx + yy) % 2).astype(np.uint8), None, ((np.mgrid[0:40, 0:40].sum(0) // 3) % 2).astype(np.uint8)]
    depths = [None, np.full((48, 17), 4.0, dtype=np.float32), np.full((40, 40), 4.0, dtype=np.float32)]
    return types.SimpleNamespace(vertices=vertices, cameras=cameras, masks=masks, depths=depths, near=0.25, depth_tol=0.25)
