"""A numpy restatement of the mesh cleaning of ``mvs_gaussian_splatting_amd/mesh.py`` (csrc/mesh.hip): a
plain sequential union-find, a dictionary of edges, the numbering rule and ``clean_mesh``'s rule, sharing no code with
the package, and the cases the host and GPU tests run."""
import functools
import math

import numpy as np

import tsdf_restate as T


# ---- the restatement ---------------------------------------------------------------------------------------------------
class _UnionFind:
    def __init__(self, n):
        self.up = list(range(n))

    def find(self, x):
        root = x
        while self.up[root] != root:
            root = self.up[root]
        while self.up[x] != root:
            self.up[x], x = root, self.up[x]
        return root

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.up[b] = a                       # no rule about which becomes the root: the numbering does not use it


def components(faces, num_vertices, connectivity="edge"):
    """-> (face_component int32 [F], component_faces int64 [K]), components numbered by their smallest face index."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F = len(faces)
    if F and (faces.min() < 0 or faces.max() >= num_vertices):
        raise ValueError("a face index is out of range")
    if connectivity == "vertex":
        uf = _UnionFind(num_vertices)
        for a, b, c in faces.tolist():
            uf.union(a, b)
            uf.union(a, c)
        roots = [uf.find(int(f[0])) for f in faces]
    elif connectivity == "edge":
        uf = _UnionFind(F)
        seen = {}                                # undirected edge -> a face that has it
        for f, (a, b, c) in enumerate(faces.tolist()):
            for e in ((a, b), (b, c), (c, a)):
                key = (min(e), max(e))
                if key in seen:
                    uf.union(seen[key], f)
                else:
                    seen[key] = f
        roots = [uf.find(f) for f in range(F)]
    else:
        raise ValueError(connectivity)
    number = {}
    face_component = np.zeros(F, dtype=np.int32)
    for f, r in enumerate(roots):                # first met = smallest face index of the component
        face_component[f] = number.setdefault(r, len(number))
    return face_component, np.bincount(face_component, minlength=len(number)).astype(np.int64)


def keep_mask(component_faces, face_component, keep_largest=None, min_faces=0):
    K = len(component_faces)
    threshold = min_faces
    if keep_largest is not None and keep_largest < K:
        threshold = max(threshold, int(np.sort(component_faces)[::-1][keep_largest - 1]))
    return component_faces[face_component] >= threshold if K else np.zeros(0, dtype=bool)


def clean(vertices, faces, colors=None, keep_largest=None, min_faces=0, connectivity="edge"):
    """-> (vertices, faces int32, colors, kept vertex indices, kept face indices): rows in their original order."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    face_component, component_faces = components(faces, len(vertices), connectivity)
    keep = keep_mask(component_faces, face_component, keep_largest, min_faces)
    kept_faces = faces[keep]
    used = np.zeros(len(vertices), dtype=bool)
    used[kept_faces.reshape(-1)] = True
    new_index = np.cumsum(used) - 1
    kept_v = np.nonzero(used)[0]
    return (vertices[kept_v], new_index[kept_faces].astype(np.int32).reshape(-1, 3),
            None if colors is None else colors[kept_v], kept_v, np.nonzero(keep)[0])


def partition(face_component, order=None):
    """The partition of the faces as a set of frozensets of (original) face indices: independent of the numbering."""
    face_component = np.asarray(face_component)
    names = np.arange(len(face_component)) if order is None else np.asarray(order)
    groups = {}
    for f, c in zip(names.tolist(), face_component.tolist()):
        groups.setdefault(c, []).append(f)
    return {frozenset(g) for g in groups.values()}


def canonical(labels):
    """Labels renumbered in the order of first appearance."""
    number = {}
    return np.array([number.setdefault(int(l), len(number)) for l in labels], dtype=np.int64)


# ---- cases: name -> (faces int32 [F,3], V) ------------------------------------------------------------------------------
STRIP_FACES = 3000            # more than one 256-lane workgroup, many waves


def strip(n, numbering):
    """n faces (i, i+1, i+2) over n + 2 vertices, renumbered: 'descending' and 'permuted' put every component's smallest
    index far from where the faces start, which forces long parent chains and hook retries across workgroups."""
    V = n + 2
    base = np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], axis=1)
    base[1::2] = base[1::2][:, [1, 0, 2]]                                         # consistent winding
    rename = {"ascending": np.arange(V), "descending": np.arange(V)[::-1].copy(),
              "permuted": np.random.default_rng(11).permutation(V)}[numbering]
    return rename[base].astype(np.int32), V


def isolated(n):
    return np.arange(3 * n, dtype=np.int32).reshape(n, 3), 3 * n


def equal_components(count, faces_each):
    parts, V = [], 0
    for _ in range(count):
        f, v = strip(faces_each, "ascending")
        parts.append(f + V)
        V += v
    return np.concatenate(parts).astype(np.int32), V


def soup(V=500, F=700, seed=5):
    return np.random.default_rng(seed).integers(0, V, size=(F, 3)).astype(np.int32), V


@functools.lru_cache(maxsize=None)
def cases():
    out = {
        "one_face": (np.array([[0, 1, 2]], dtype=np.int32), 3),
        "two_faces_one_edge": (np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32), 4),
        "bow_tie": (np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int32), 5),
        "isolated_1000": isolated(1000),
        "forty_equal": equal_components(40, 7),
        # the first component's smallest vertex (0) appears in its last face only; another component lies in between
        "smallest_vertex_last": (np.array([[3, 4, 5], [5, 4, 6], [1, 2, 7], [6, 4, 8], [8, 4, 0]], dtype=np.int32), 9),
        # 0, 1 in front, 4, 7, 10 between, 12 behind: never referenced
        "unreferenced_vertices": (np.array([[2, 3, 5], [5, 3, 6], [8, 9, 11]], dtype=np.int32), 13),
        "three_faces_one_edge": (np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [5, 6, 7]], dtype=np.int32), 8),
        # (0,0,1) shares the edge {0,1} with its neighbour; (3,3,3) and (3,3,6) share the self-pair {3,3}; (4,5,5) alone
        "degenerate_faces": (np.array([[0, 0, 1], [0, 1, 2], [3, 3, 3], [4, 5, 5], [3, 3, 6]], dtype=np.int32), 7),
        "soup": soup(),
    }
    for numbering in ("ascending", "descending", "permuted"):
        out[f"strip_{numbering}"] = strip(STRIP_FACES, numbering)
    return out


def face_permutation(F, seed=23):
    return np.random.default_rng(seed).permutation(F)


# ---- the TSDF case: the sphere of the TSDF tests with two small blobs far from it ------------------------------------
BLOBS = (((21.4 + math.sqrt(2) / 40, 17.4 - math.sqrt(3) / 50, 19.4 + math.pi / 90), 1.2),
         ((2.3 + math.sqrt(5) / 60, 2.4 + math.sqrt(7) / 70, 2.6 - math.sqrt(2) / 80), 1.3))


@functools.lru_cache(maxsize=None)
def floater_field():
    """``tsdf_restate.sphere_field`` with the union (min) of two small spheres in opposite corners: three closed shells."""
    field = dict(T.sphere_field())
    nx, ny, nz = T.SPHERE_DIMS
    kk, jj, ii = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    tsdf = field["tsdf"].astype(np.float64)
    for (cx, cy, cz), r in BLOBS:
        dist = np.sqrt((ii - cx) ** 2 + (jj - cy) ** 2 + (kk - cz) ** 2)
        tsdf = np.minimum(tsdf, np.clip((dist - r) / T.SPHERE_TRUNC, -1.0, 1.0))
    field["tsdf"] = tsdf.astype(np.float32)
    assert not np.any(field["tsdf"] == 0)
    return field


@functools.lru_cache(maxsize=None)
def floater_mesh():
    """-> (vertices float64, faces int64, colors float64) of the floater field, in the order of ``extract_mesh``."""
    return T.extract(floater_field())
