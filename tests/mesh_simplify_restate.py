"""A sequential numpy restatement of the vertex clustering of ``mvs_gaussian_splatting_amd/mesh.py`` (``simplify_mesh``;
csrc/mesh_simplify.hip): dictionaries and loops over vertices and faces in ascending index, float64 means
in ascending vertex index, sharing no code with the package, and the cases the host and GPU tests run."""
import functools
import math
import types

import numpy as np

import tsdf_restate as T

CELL_BITS = 21


# ---- the restatement ---------------------------------------------------------------------------------------------------
def rotate(t):
    """The triple rotated so that its smallest entry comes first: the winding stays."""
    n = t.index(min(t))
    return t[n:] + t[:n]


def simplify(vertices, faces, colors=None, *, voxel_size, origin=None):
    """Steps 1-6 of ``simplify_mesh`` -> a namespace of ``vertices`` float32 [V',3], ``faces`` int32 [F',3], ``colors``
    float32 [V',3] or None, ``vertex_cluster`` int32 [V], and for the tests: ``origin`` (float64 [3]), ``cells`` int64
    [V',3], ``members`` (the input vertices of every output vertex, ascending), ``kept_faces`` (input face indices) and
    ``max_abs`` / ``max_abs_colors`` float64 [V',3] (the largest magnitude among the members, per component).
    ``ValueError`` where ``simplify_mesh`` raises ``GsrError``."""
    vertices = np.asarray(vertices)
    assert vertices.dtype == np.float32 and vertices.ndim == 2 and vertices.shape[1] == 3
    assert colors is None or (colors.dtype == np.float32 and colors.shape == vertices.shape)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V, h = len(vertices), np.float64(voxel_size)
    if len(faces) and (faces.min() < 0 or faces.max() >= V):
        raise ValueError("a face index is out of range")
    referenced = np.zeros(V, dtype=bool)
    referenced[faces.reshape(-1)] = True
    ref = np.nonzero(referenced)[0]
    if not np.isfinite(vertices[ref]).all():
        raise ValueError("a referenced coordinate is not finite")
    o = vertices[ref].min(axis=0).astype(np.float64) - h / 2 if origin is None else np.asarray(origin, dtype=np.float64)
    cell_of = {}
    for v in ref.tolist():
        cell = np.floor((vertices[v].astype(np.float64) - o) / h)
        if not np.all((cell >= 0) & (cell < 2 ** CELL_BITS)):
            raise ValueError("a cell index is out of range")
        cell_of[v] = tuple(int(c) for c in cell)
    key = lambda c: (c[0] << (2 * CELL_BITS)) | (c[1] << CELL_BITS) | c[2]                    # noqa: E731
    number = {k: n for n, k in enumerate(sorted({key(c) for c in cell_of.values()}))}
    cluster = {v: number[key(c)] for v, c in cell_of.items()}
    members = [[] for _ in number]
    for v in ref.tolist():                                   # ascending vertex index
        members[cluster[v]].append(v)

    def mean(rows, group):
        total = rows[group[0]].astype(np.float64)            # from the first member on, not from 0: -0.0 stays -0.0
        for v in group[1:]:
            total = total + rows[v].astype(np.float64)
        return (total / np.float64(len(group))).astype(np.float32)

    seen, kept, kept_index = set(), [], []
    for f, corners in enumerate(faces.tolist()):
        t = tuple(cluster[v] for v in corners)
        if len(set(t)) < 3 or rotate(t) in seen:
            continue
        seen.add(rotate(t))
        kept.append(t)
        kept_index.append(f)
    used = sorted({c for t in kept for c in t})
    final = {c: n for n, c in enumerate(used)}
    vertex_cluster = np.full(V, -1, dtype=np.int32)
    for v, c in cluster.items():
        vertex_cluster[v] = final.get(c, -1)
    cells = {c: cell_of[group[0]] for c, group in enumerate(members)}
    rows = lambda fn, width=3: np.array([fn(c) for c in used]).reshape(len(used), width)      # noqa: E731
    return types.SimpleNamespace(
        vertices=rows(lambda c: mean(vertices, members[c])).astype(np.float32),
        faces=np.array([[final[c] for c in t] for t in kept], dtype=np.int32).reshape(-1, 3),
        colors=None if colors is None else rows(lambda c: mean(colors, members[c])).astype(np.float32),
        vertex_cluster=vertex_cluster, origin=o, cells=rows(lambda c: cells[c]).astype(np.int64),
        members=[members[c] for c in used], kept_faces=np.array(kept_index, dtype=np.int64),
        max_abs=rows(lambda c: np.abs(vertices[members[c]].astype(np.float64)).max(axis=0)),
        max_abs_colors=None if colors is None else rows(lambda c: np.abs(colors[members[c]].astype(np.float64)).max(axis=0)))


def rotated_set(faces):
    """The faces as a set of rotated triples: independent of their order."""
    return {rotate(tuple(t)) for t in np.asarray(faces).tolist()}


def vertex_partition(vertex_cluster, names=None):
    """The partition of the vertices that took part, as a set of frozensets of (original) vertex indices, and the set of
    those that did not."""
    names = np.arange(len(vertex_cluster)) if names is None else np.asarray(names)
    groups, out = {}, set()
    for v, c in zip(names.tolist(), np.asarray(vertex_cluster).tolist()):
        if c < 0:
            out.add(v)
        else:
            groups.setdefault(c, []).append(v)
    return {frozenset(g) for g in groups.values()}, out


# ---- cases: name -> dict(vertices float32 [V,3], faces int32 [F,3], colors float32 [V,3], voxel_size, origin) ---------
def _colors(vertices, seed):
    return np.random.default_rng(seed).random(vertices.shape, dtype=np.float32)


def _case(vertices, faces, voxel_size, origin, seed):
    vertices = np.ascontiguousarray(vertices, dtype=np.float32)
    return {"vertices": vertices, "faces": np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3),
            "colors": _colors(vertices, seed), "voxel_size": voxel_size, "origin": origin}


def one_cell_fan(rim=64):
    """A fan of ``rim`` triangles about a centre, all inside the cell [0, 1)^3: one run of rim + 1 vertices."""
    angle = 2 * math.pi * np.arange(rim) / rim
    ring = np.stack((0.5 + 0.4 * np.cos(angle), 0.5 + 0.4 * np.sin(angle), 0.3 + 0.4 * np.arange(rim) / rim), axis=1)
    vertices = np.concatenate(([[0.5, 0.5, 0.5]], ring))
    faces = [(0, 1 + i, 1 + (i + 1) % rim) for i in range(rim)]
    return _case(vertices, faces, 1.0, (0.0, 0.0, 0.0), 65)


RING_CELLS = ((0, 0), (1, 0), (2, 0), (2, 1), (2, 2), (1, 2), (0, 2), (0, 1))       # counter-clockwise about cell (1, 1)


def run_257(inner=257):
    """``inner`` vertices inside the cell (1, 1, 1), ringed by eight cells of one vertex each; face i joins inner vertex i to
    two neighbouring ring vertices, so the faces collapse to eight triples, each many times over."""
    rng = np.random.default_rng(257)
    middle = 1.0 + 0.05 + 0.9 * rng.random((inner, 3))
    ring = np.array([(i + 0.5, j + 0.5, 1.5) for i, j in RING_CELLS])
    faces = [(i, inner + i % 8, inner + (i + 1) % 8) for i in range(inner)]
    return _case(np.concatenate((middle, ring)), faces, 1.0, (0.0, 0.0, 0.0), 257)


BOUNDARY_H, BOUNDARY_ORIGIN = 0.25, (-1.5, -1.5, -1.5)


def boundary_coordinates():
    """float32 coordinates on and next to cell boundaries of the grid of ``boundaries`` (h = 0.25 from -1.5: every
    boundary is a float32): the origin itself, multiples of h below and above zero, both zeros, and the float32
    neighbours of boundaries on either side."""
    f = np.float32
    on = [f(-1.5), f(-1.25), f(-0.25), f(-0.0), f(0.0), f(0.25), f(1.0), f(2.75)]
    below = [np.nextafter(f(-1.25), f(-2)), np.nextafter(f(-0.25), f(-2)), np.nextafter(f(0.0), f(-2)),
             np.nextafter(f(0.25), f(-2)), np.nextafter(f(1.0), f(-2))]
    above = [np.nextafter(f(-1.5), f(2)), np.nextafter(f(-0.25), f(2)), np.nextafter(f(0.0), f(2)), np.nextafter(f(1.0), f(2))]
    inside = [f(-1.4), f(-0.1), f(0.1), f(0.3)]
    return np.array(on + below + above + inside, dtype=np.float32)


def boundaries():
    """Every coordinate of ``boundary_coordinates`` on every axis in turn (the two other coordinates are 0.1), so that the
    floor, the half-open cell and the place of each axis in the key all decide which vertices meet: -0.0, 0.0 and 0.1 share
    a cell (with the subnormals next to 0, which the float64 subtraction absorbs); 0.25 and the float32 below it do not."""
    c = boundary_coordinates()
    m = len(c)
    vertices = np.full((3 * m, 3), 0.1, dtype=np.float32)
    for a in range(3):
        vertices[a * m:(a + 1) * m, a] = c
    faces = [(a * m + n, a * m + (n + 1) % m, a * m + (n + 2) % m) for a in range(3) for n in range(m)]
    faces += [(n, m + (n + 4) % m, 2 * m + (n + 11) % m) for n in range(m)]
    return _case(vertices, faces, BOUNDARY_H, BOUNDARY_ORIGIN, 3)


def _duplicates(opposite):
    """Cells A < B < C < D in key order; A holds two vertices.  Faces 0 and 1 collapse to the triple (A, B, C): with the
    same winding, or with opposite windings; face 2 stands apart."""
    vertices = [(0.2, 0.5, 0.5), (0.7, 0.4, 0.6), (1.5, 0.5, 0.5), (2.5, 0.5, 0.5), (3.5, 0.5, 0.5)]     # a0, a1, b, c, d
    second = (1, 3, 2) if opposite else (2, 3, 1)                   # (A, C, B) against (B, C, A) = (A, B, C) rotated
    return _case(vertices, [(0, 2, 3), second, (2, 4, 3)], 1.0, (0.0, 0.0, 0.0), 7)


def orphan_cluster():
    """Cells A < D < X < B < C in key order (D lies one cell up in y).  X holds two vertices, and its only face (x0, x1, b)
    has two corners in X: it vanishes, X is dropped, and B and C move down one index, while the faces (A, B, C) and
    (B, D, C) of its neighbours stay."""
    vertices = [(0.5, 0.5, 0.5), (1.2, 0.5, 0.5), (1.8, 0.5, 0.5), (2.5, 0.5, 0.5), (3.5, 0.5, 0.5), (0.5, 1.5, 0.5)]
    faces = [(1, 2, 3), (0, 3, 4), (3, 5, 4)]
    return _case(vertices, faces, 1.0, (0.0, 0.0, 0.0), 9)


def unreferenced_nan():
    """A strip of 40 triangles over cells of one or two vertices, with vertices that no face refers to in front, between and
    behind: NaN, infinities and a finite row far below every referenced one.  The default origin."""
    n = 42
    good = np.stack((0.7 * np.arange(n), 0.3 * (np.arange(n) % 2), 0.1 * np.arange(n)), axis=1).astype(np.float32)
    junk = np.array([[np.nan, 0, 0], [np.inf, -np.inf, 1], [-1e30, -1e30, -1e30], [0, np.nan, np.inf]], dtype=np.float32)
    slots = np.insert(np.arange(n), (0, 0, 17, 30, n, n), -1)         # -1: a junk row
    rename = np.full(n, -1)
    rename[slots[slots >= 0]] = np.nonzero(slots >= 0)[0]
    vertices = np.array([good[s] if s >= 0 else junk[i % len(junk)] for i, s in enumerate(slots)], dtype=np.float32)
    faces = [(rename[i], rename[i + 1], rename[i + 2]) if i % 2 == 0 else (rename[i + 1], rename[i], rename[i + 2])
             for i in range(n - 2)]
    case = _case(vertices, faces, 1.0, None, 11)
    case["colors"][slots < 0] = np.nan
    return case


def identity_small_h(V=300, F=520):
    """Random vertices in the unit cube, random faces without a repeated corner, a cell of 2^-14: every vertex is alone."""
    rng = np.random.default_rng(13)
    vertices = rng.random((V, 3), dtype=np.float32)
    vertices[7] = (-0.0, 0.5, -0.0)                                  # a bit-copy keeps the sign of a zero
    faces = np.array([rng.choice(V - 20, size=3, replace=False) for _ in range(F)])      # the last 20: unreferenced
    return _case(vertices, faces, 2.0 ** -14, (-0.25, -0.25, -0.25), 13)


GRID_N = 265


def grid_70k(n=GRID_N):
    """An n x n height field with unit steps, two triangles per square, and a cell of two steps (origin -0.5: a cell
    holds a 2 x 2 block of vertices, the last row and column half of one); the heights stay inside one cell."""
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    z = 0.75 + 0.7 * np.sin(0.05 * i) * np.cos(0.03 * j)
    vertices = np.stack((i, j, z), axis=-1).reshape(-1, 3)
    a = (j[:-1, :-1] * n + i[:-1, :-1]).reshape(-1)
    faces = np.concatenate((np.stack((a, a + 1, a + n), axis=1), np.stack((a + 1, a + n + 1, a + n), axis=1)))
    return _case(vertices, faces, 2.0, (-0.5, -0.5, 0.0), 70)


def sphere_tsdf():
    """The marching-tetrahedra mesh of the sphere of the TSDF tests (voxel 1), clustered at two voxels from the volume's
    origin: two of every vertex's coordinates are whole numbers, so many lie exactly on a cell boundary."""
    vertices, faces, colors = T.extract(T.sphere_field())
    case = _case(vertices, faces, 2.0, (0.0, 0.0, 0.0), 0)
    case["colors"] = np.ascontiguousarray(colors, dtype=np.float32)
    return case


@functools.lru_cache(maxsize=None)
def cases():
    return {"one_cell_fan_65": one_cell_fan(), "run_257": run_257(), "boundaries": boundaries(),
            "dup_same": _duplicates(False), "dup_opposite": _duplicates(True), "orphan_cluster": orphan_cluster(),
            "unreferenced_nan": unreferenced_nan(), "identity_small_h": identity_small_h(), "grid_70k": grid_70k(),
            "sphere_tsdf": sphere_tsdf()}


CASES = ("one_cell_fan_65", "run_257", "boundaries", "dup_same", "dup_opposite", "orphan_cluster", "unreferenced_nan",
         "identity_small_h", "grid_70k", "sphere_tsdf")


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's result for a case: computed once, never modified."""
    c = cases()[name]
    return simplify(c["vertices"], c["faces"], c["colors"], voxel_size=c["voxel_size"], origin=c["origin"])


def permutation(n, seed=29):
    return np.random.default_rng(seed).permutation(n)
