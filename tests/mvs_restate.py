"""numpy restatement of the multi-view depth consistency check, of the back-projection and of the source selection
(csrc/mvs.hip; mvs.py), written from the definitions as whole-array arithmetic.  ``dtype=np.float64`` is
the truth the GPU tests compare against; ``dtype=np.float32`` runs the same operations rounded to float32 one by one and
gives the tests their bar (twice its own error against float64).  Both start from the same float32 inputs: the depth
maps, the focal lengths and the two float32 matrices per source.  Also the analytic scene the host and GPU tests share.
"""
import math

import numpy as np
import torch

MARGIN = 1e-4          # fragility margin: absolute for zs, zb against 0.2; pixels for the footprint and for the
#                        reprojection error against pix_thresh; relative to d for |zb - d| against depth_thresh * d
KINDS = ("behind", "outside", "hole", "back_behind", "pixel", "depth", "both", "ok")


# ---- cameras -----------------------------------------------------------------------------------------------------------
class Cam:
    """A camera as mvs.py reads it.  ``Rc2w``: columns right, down, forward in the world; ``pos``: the centre."""

    def __init__(self, Rc2w, pos, W, H, fx, fy):
        M = np.eye(4)
        M[:3, :3], M[3, :3] = Rc2w, -np.asarray(Rc2w).T @ np.asarray(pos, np.float64)      # p_view = p_world @ Rc2w - pos @ Rc2w
        self.world_view_transform = torch.from_numpy(M.astype(np.float32))
        self.image_width, self.image_height = int(W), int(H)
        self.FoVx, self.FoVy = 2.0 * math.atan(W / (2.0 * fx)), 2.0 * math.atan(H / (2.0 * fy))

    def to(self, dev):
        self.world_view_transform = self.world_view_transform.to(dev)
        return self


def look_at(pos, target, W, H, fx, fy, up=(0.0, -1.0, 0.0)):
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    fwd = (target - pos) / np.linalg.norm(target - pos)
    right = np.cross(np.asarray(up, np.float64), -fwd)
    right /= np.linalg.norm(right)
    return Cam(np.stack((right, np.cross(fwd, right), fwd), axis=1), pos, W, H, fx, fy)


def view64(cam):
    return cam.world_view_transform.detach().cpu().to(torch.float32).numpy().astype(np.float64)


def focal(cam):
    """(fx, fy) as float32, from the fields of view as the package forms them."""
    W, H = cam.image_width, cam.image_height
    return np.float32(W / (2.0 * math.tan(cam.FoVx * 0.5))), np.float32(H / (2.0 * math.tan(cam.FoVy * 0.5)))


def source_rows(ref_cam, src_cams, src_depths):
    """The table of the kernel: per source its depth, size, focal lengths and the float32 A = inv(V_r) V_s, B = inv(V_s) V_r."""
    Mr = view64(ref_cam)
    rows = []
    for cam, depth in zip(src_cams, src_depths):
        Ms = view64(cam)
        fx, fy = focal(cam)
        rows.append({"depth": np.asarray(depth, np.float32), "W": cam.image_width, "H": cam.image_height, "fx": fx, "fy": fy,
                     "A": (np.linalg.inv(Mr) @ Ms).astype(np.float32), "B": (np.linalg.inv(Ms) @ Mr).astype(np.float32)})
    return rows


# ---- the check ---------------------------------------------------------------------------------------------------------
def _through(M, x, y, z):
    col = lambda c: ((x * M[0, c] + y * M[1, c]) + z * M[2, c]) + M[3, c]      # noqa: E731
    return col(0), col(1), col(2)


def _cell(depth, x0, y0, W, H):
    """inside [H,W] bool: the cell (x0, y0) .. (x0 + 1, y0 + 1) lies in the image; the four depths (0 where it does not)."""
    with np.errstate(invalid="ignore"):
        inside = (x0 >= 0) & (x0 + 1 <= W - 1) & (y0 >= 0) & (y0 + 1 <= H - 1)
    xi = np.where(inside, x0, 0).astype(np.int64)
    yi = np.where(inside, y0, 0).astype(np.int64)
    four = [np.where(inside, depth[yi + dy, xi + dx], 0) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]
    return inside, four


def consistency(depth, fx, fy, rows, pix_thresh=1.0, depth_thresh=0.01, min_views=2, dtype=np.float64):
    """-> (count int64 [H,W], fused [H,W], fragile bool [H,W], kind int8 [S,H,W] indexing KINDS, -1 without depth).
    ``fragile``: a comparison of this run, for some source, lies within MARGIN of flipping (meaningful at float64)."""
    f = dtype
    d = np.asarray(depth, np.float32).astype(f)
    H, W = d.shape
    fx, fy = f(np.float32(fx)), f(np.float32(fy))
    pix_thresh, depth_thresh = f(np.float32(pix_thresh)), f(np.float32(depth_thresh))
    cx, cy = (f(W) - f(1)) * f(0.5), (f(H) - f(1)) * f(0.5)
    py, px = (a.astype(f) for a in np.meshgrid(np.arange(H), np.arange(W), indexing="ij"))
    has = d > 0
    xr, yr = ((px - cx) * d) / fx, ((py - cy) * d) / fy
    n = np.zeros((H, W), np.int64)
    total = np.zeros((H, W), f)
    fragile = np.zeros((H, W), bool)
    kinds = np.full((len(rows), H, W), -1, np.int8)
    with np.errstate(all="ignore"):
        for s, row in enumerate(rows):
            A, B = row["A"].astype(f), row["B"].astype(f)
            Ws, Hs, fxs, fys = row["W"], row["H"], f(row["fx"]), f(row["fy"])
            sd = row["depth"].astype(f)
            cxs, cys = (f(Ws) - f(1)) * f(0.5), (f(Hs) - f(1)) * f(0.5)
            xs, ys, zs = _through(A, xr, yr, d)
            live = has.copy()
            kind = np.full((H, W), -1, np.int8)
            fragile |= live & (np.abs(zs - f(0.2)) < MARGIN)
            step = live & ~(zs > f(0.2))
            kind[step] = KINDS.index("behind")
            live &= ~step
            us, vs = (fxs * xs) / zs + cxs, (fys * ys) / zs + cys
            x0, y0 = np.floor(us), np.floor(vs)
            ax, ay = us - x0, vs - y0
            inside, four = _cell(sd, x0, y0, Ws, Hs)
            valid = inside & (four[0] > 0) & (four[1] > 0) & (four[2] > 0) & (four[3] > 0)
            # the bilinear value is continuous across a cell border: fragile only where a neighbouring cell within MARGIN
            # of (us, vs) differs in validity (the image border is the cell that lies outside)
            for dx in (-1, 0, 1):
                near_x = (ax < MARGIN) if dx < 0 else ((1 - ax) < MARGIN) if dx > 0 else np.ones((H, W), bool)
                for dy in (-1, 0, 1):
                    near_y = (ay < MARGIN) if dy < 0 else ((1 - ay) < MARGIN) if dy > 0 else np.ones((H, W), bool)
                    if dx == 0 and dy == 0:
                        continue
                    ins2, four2 = _cell(sd, x0 + dx, y0 + dy, Ws, Hs)
                    valid2 = ins2 & (four2[0] > 0) & (four2[1] > 0) & (four2[2] > 0) & (four2[3] > 0)
                    fragile |= live & near_x & near_y & (valid2 != valid)
            step = live & ~inside
            kind[step] = KINDS.index("outside")
            live &= ~step
            step = live & ~valid
            kind[step] = KINDS.index("hole")
            live &= ~step
            ds = (four[0] * (1 - ax) + four[1] * ax) * (1 - ay) + (four[2] * (1 - ax) + four[3] * ax) * ay
            xb0, yb0 = ((us - cxs) * ds) / fxs, ((vs - cys) * ds) / fys
            xb, yb, zb = _through(B, xb0, yb0, ds)
            fragile |= live & (np.abs(zb - f(0.2)) < MARGIN)
            step = live & ~(zb > f(0.2))
            kind[step] = KINDS.index("back_behind")
            live &= ~step
            ub, vb = (fx * xb) / zb + cx, (fy * yb) / zb + cy
            du, dv = ub - px, vb - py
            e2 = du * du + dv * dv
            gap = np.abs(zb - d)
            fragile |= live & (np.abs(np.sqrt(e2.astype(np.float64)) - float(pix_thresh)) < MARGIN)
            fragile |= live & (np.abs(gap / d - depth_thresh) < MARGIN)
            pix_ok, depth_ok = e2 < pix_thresh * pix_thresh, gap < depth_thresh * d
            kind[live & ~pix_ok & depth_ok] = KINDS.index("pixel")
            kind[live & pix_ok & ~depth_ok] = KINDS.index("depth")
            kind[live & ~pix_ok & ~depth_ok] = KINDS.index("both")
            ok = live & pix_ok & depth_ok
            kind[ok] = KINDS.index("ok")
            n += ok
            total = np.where(ok, total + zb, total)
            kinds[s] = kind
    fused = np.where(has & (n >= min_views), (d + total) / (n + 1).astype(f), f(0))
    return n, fused, fragile, kinds


def backproject(depth, fx, fy, c2w, dtype=np.float64):
    """-> xyz [H W, 3]: zero rows where there is no depth.  ``c2w``: the float32 cam_to_world."""
    f = dtype
    d = np.asarray(depth, np.float32).astype(f)
    H, W = d.shape
    fx, fy = f(np.float32(fx)), f(np.float32(fy))
    M = np.asarray(c2w, np.float32).astype(f)
    cx, cy = (f(W) - f(1)) * f(0.5), (f(H) - f(1)) * f(0.5)
    py, px = (a.astype(f) for a in np.meshgrid(np.arange(H), np.arange(W), indexing="ij"))
    xr, yr = ((px - cx) * d) / fx, ((py - cy) * d) / fy
    x, y, z = _through(M, xr, yr, d)
    return np.where((d > 0)[..., None], np.stack((x, y, z), axis=-1), f(0)).reshape(-1, 3)


def cam_to_world32(cam):
    return np.linalg.inv(view64(cam)).astype(np.float32)


def select_source_views(cameras, n_sources, max_angle_deg=60.0):
    """The definition, camera by camera: candidates by the angle between forward directions, ordered by (distance, index)."""
    poses = []
    for cam in cameras:
        V = view64(cam).T
        R, t = V[:3, :3], V[:3, 3]
        poses.append((-R.T @ t, R[2] / np.linalg.norm(R[2])))
    out = []
    for i, (ci, fi) in enumerate(poses):
        cand = []
        for j, (cj, fj) in enumerate(poses):
            if j != i and math.degrees(math.acos(max(-1.0, min(1.0, float(fi @ fj))))) <= max_angle_deg:
                cand.append((float(np.linalg.norm(cj - ci)), j))
        out.append([j for _, j in sorted(cand)[:n_sources]])
    return out


# ---- the analytic scene: a plane and a sphere in front of it -----------------------------------------------------------
PLANE_N, PLANE_C = np.array([0.125, -0.0625, 1.0]), 4.0                   # n . p = c
SPHERE_O, SPHERE_R = np.array([0.5, 0.0625, 3.25]), 0.3125
TARGET = np.array([0.0, 0.0, 4.0])
REF_W, REF_H, REF_FX, REF_FY = 70, 37, 128.0, 120.0
PIX_THRESH, DEPTH_THRESH = 1.0, 0.01


def render_depth(cam, dtype=np.float64):
    """The analytic depth map of the scene in ``cam``: per pixel ray the nearest of plane and sphere (float64), 0 where
    the ray meets neither in front of the camera; rounded to float32."""
    W, H = cam.image_width, cam.image_height
    fx, fy = (np.float64(v) for v in focal(cam))
    c2w = np.linalg.inv(view64(cam))
    py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack(((px - (W - 1) / 2) / fx, (py - (H - 1) / 2) / fy, np.ones_like(px)), axis=-1) @ c2w[:3, :3]
    o = c2w[3, :3]
    with np.errstate(all="ignore"):
        t_plane = (PLANE_C - PLANE_N @ o) / (ray @ PLANE_N)
        t_plane = np.where(t_plane > 0, t_plane, np.inf)
        oc = o - SPHERE_O
        a, b, c = (ray * ray).sum(-1), 2.0 * (ray @ oc), oc @ oc - SPHERE_R ** 2
        disc = b * b - 4 * a * c
        t_sphere = np.where(disc > 0, (-b - np.sqrt(np.abs(disc))) / (2 * a), np.inf)
        t_sphere = np.where(t_sphere > 0, t_sphere, np.inf)
    t = np.minimum(t_plane, t_sphere)
    return np.where(np.isfinite(t), t, 0.0).astype(np.float32), (t_sphere < t_plane)


def _orbit(deg_y, deg_x, dist, W, H, fx, fy):
    ay, ax = math.radians(deg_y), math.radians(deg_x)
    off = np.array([math.sin(ay) * math.cos(ax), math.sin(ax), -math.cos(ay) * math.cos(ax)]) * dist
    return look_at(TARGET + off, TARGET, W, H, fx, fy)


def scene():
    """-> (reference camera, its depth [37,70], four source cameras, their depth maps).  Reference: identity pose at the
    origin.  Sources: 0, 48 x 40 with its own focal lengths, 40 degrees round the target, a patch scaled by 1.015 (fails
    the pixel test and passes the depth test); 1, a rectangular hole of zeros and a patch of depth 1/16 (its points lie
    beside the reference camera: zb <= 0.2); 2, scaled by 1.02 in its left half (fails the depth test at 0.01 and
    passes the pixel test at 1); 3, facing away: every zs <= 0.2."""
    ref = Cam(np.eye(3), np.zeros(3), REF_W, REF_H, REF_FX, REF_FY)
    cams = [_orbit(50.0, 4.0, 4.25, 48, 40, 80.0, 88.0), _orbit(-9.0, -5.0, 4.0, 64, 48, 104.0, 104.0),
            _orbit(5.0, 7.0, 4.0, 72, 44, 152.0, 144.0),
            look_at(np.array([0.5, 0.0, 0.0]), np.array([0.5, 0.0, -4.0]), 48, 40, 40.0, 40.0)]
    depth, _ = render_depth(ref)
    depths = [render_depth(c)[0] for c in cams]
    depths[0][20:32, 24:36] *= np.float32(1.014)
    depths[1][26:34, 8:24] = 0.0
    depths[1][10:20, 42:54] = np.float32(0.0625)
    depths[2][:, :34] *= np.float32(1.02)
    depth[3:6, 60:66] = 0.0                                                # reference pixels without depth
    return ref, depth, cams, depths


def exact_case():
    """Dyadic cameras and a fronto-parallel plane at depth 4: every operation of the sequence is exact in float32.
    Reference 70 x 37, f = 64, at the origin; source 48 x 40, f = 32, translated so that us = px / 2 + 12.5 and
    vs = py / 2 + 10.5: us is an integer at every odd px and us = W_s - 1 = 47 exactly at px = 69, where the footprint
    test x0 + 1 <= W_s - 1 refuses the pixel.  -> (ref camera, depth, [source camera], [source depth])."""
    ref = Cam(np.eye(3), np.zeros(3), 70, 37, 64.0, 64.0)
    src = Cam(np.eye(3), np.array([-0.78125, 0.0, 0.0]), 48, 40, 32.0, 32.0)      # p_src = p_ref + (25 / 32, 0, 0)
    return ref, np.full((37, 70), 4.0, np.float32), [src], [np.full((40, 48), 4.0, np.float32)]
