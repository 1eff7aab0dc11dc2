"""The on-disk interchange format of the model that feeds the rasterizer: the PLY written by
``GaussianModel.save_ply`` / read by ``load_ply`` (``scene/gaussian_model.py:279-358``; ``render.py`` loads it through
``scene/__init__.py:77-81``).  The reference uses the ``plyfile`` package (absent here); this is a dependency-free
numpy reader / writer of the same file: one ``vertex`` element, binary little-endian, every property ``float``,
in the order

    x y z nx ny nz f_dc_0..2 f_rest_0..(3*(deg+1)^2-4) opacity scale_0..2 rot_0..3

with RAW (pre-activation) values, SH coefficients channel-major (``_features_*`` transposed to ``[P, 3, k]`` and
flattened), normals all zero.  Pinned to the reference by ``tests/golden/ply_layout.npz``: the structured array the
reference's ``save_ply`` hands to ``plyfile`` (field names, order, formats, raw bytes) and the tensors its ``load_ply``
builds from it, captured with a recording stub (``tests/golden/make_golden_ply.py``); only the header text that
``plyfile`` itself writes in front of that array is restated from that package's published behaviour.
"""
from __future__ import annotations

import os
from typing import Dict, List, Tuple

import numpy as np
import torch

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def attribute_names(n_dc: int, n_rest: int, n_scale: int = 3, n_rot: int = 4) -> List[str]:
    """``construct_list_of_attributes`` (``scene/gaussian_model.py:279-291``)."""
    names = ["x", "y", "z", "nx", "ny", "nz"]
    names += [f"f_dc_{i}" for i in range(n_dc)]
    names += [f"f_rest_{i}" for i in range(n_rest)]
    names.append("opacity")
    names += [f"scale_{i}" for i in range(n_scale)]
    names += [f"rot_{i}" for i in range(n_rot)]
    return names


def save_ply(model, path: str, filter_3D=None) -> None:
    """Write ``model`` (anything with ``_xyz, _features_dc [P,1,3], _features_rest [P,k,3], _opacity, _scaling,
    _rotation``) exactly as ``GaussianModel.save_ply`` does.  ``filter_3D`` (``[P]``; Mip-Splatting's 3D smoothing
    filter): written as one more ``float`` property of that name behind ``rot_3``, as Mip-Splatting's ``save_ply`` does;
    None writes the standard file, byte for byte."""
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    xyz = model._xyz.detach().cpu().numpy().astype(np.float32)
    f_dc = model._features_dc.detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
    f_rest = model._features_rest.detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
    opac = model._opacity.detach().cpu().numpy().reshape(xyz.shape[0], -1)
    scale = model._scaling.detach().cpu().numpy()
    rot = model._rotation.detach().cpu().numpy()
    cols = np.concatenate((xyz, np.zeros_like(xyz), f_dc, f_rest, opac, scale, rot), axis=1).astype("<f4")
    names = attribute_names(f_dc.shape[1], f_rest.shape[1], scale.shape[1], rot.shape[1])
    if filter_3D is not None:
        extra = filter_3D.detach().cpu().numpy().reshape(-1, 1).astype("<f4")
        if extra.shape[0] != cols.shape[0]:
            raise ValueError(f"filter_3D has {extra.shape[0]} values for {cols.shape[0]} Gaussians")
        cols = np.concatenate((cols, extra), axis=1)
        names.append("filter_3D")
    assert cols.shape[1] == len(names)
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {cols.shape[0]}"]
    header += [f"property float {n}" for n in names]
    header.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(np.ascontiguousarray(cols).tobytes())


_PLY_NAMES = {"i1": "char", "u1": "uchar", "i2": "short", "u2": "ushort", "i4": "int", "u4": "uint", "f4": "float",
              "f8": "double"}


def write_ply_vertices(path: str, elements: np.ndarray) -> None:
    """``PlyData([PlyElement.describe(elements, 'vertex')]).write(path)``: the header ``plyfile`` writes for a structured
    array (binary little-endian, one ``property <type> <name>`` per field) and the array's bytes."""
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {elements.shape[0]}"]
    header += [f"property {_PLY_NAMES[elements.dtype[n].str[1:]]} {n}" for n in elements.dtype.names]
    header.append("end_header")
    packed = np.dtype([(n, "<" + elements.dtype[n].str[1:]) for n in elements.dtype.names])
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(np.ascontiguousarray(elements.astype(packed)).tobytes())


def write_ply_mesh(path: str, vertices, faces, colors=None) -> None:
    """A triangle mesh as binary little-endian PLY: a ``vertex`` element (float x, y, z and, with ``colors``, uchar red,
    green, blue) and a ``face`` element ``property list uchar int vertex_indices``.  ``vertices [V,3]`` float, ``faces
    [F,3]`` integer, ``colors [V,3]`` float in [0, 1] (clamped, times 255, rounded to nearest) or None; tensors or
    arrays, V and F may be 0.  Host code."""
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)      # noqa: E731
    v = host(vertices).astype("<f4").reshape(-1, 3)
    f = host(faces).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError(f"a face refers to a vertex outside 0..{v.shape[0] - 1}")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if colors is not None:
        c = host(colors).astype(np.float64).reshape(-1, 3)
        if c.shape[0] != v.shape[0]:
            raise ValueError(f"{c.shape[0]} colours for {v.shape[0]} vertices")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vert = np.zeros(v.shape[0], dtype=fields)
    vert["x"], vert["y"], vert["z"] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        c8 = np.floor(np.clip(c, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
        vert["red"], vert["green"], vert["blue"] = c8[:, 0], c8[:, 1], c8[:, 2]
    face = np.zeros(f.shape[0], dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    face["n"] = 3
    face["idx"] = f
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
    header += [f"property {_PLY_NAMES[t.lstrip('<')]} {n}" for n, t in fields]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(vert.tobytes())
        out.write(face.tobytes())


def read_ply_vertices(path: str) -> Tuple[np.ndarray, List[str]]:
    """Structured array of the ``vertex`` element of a binary-little-endian or ascii PLY, and its property names."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, count, props, in_vertex = None, 0, [], False
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: unterminated PLY header")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] == "comment":
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    count = int(tok[2])
                elif props:
                    raise ValueError(f"{path}: elements after 'vertex' are not supported")
            elif tok[0] == "property" and in_vertex:
                if tok[1] == "list":
                    raise ValueError(f"{path}: list properties are not supported")
                props.append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        if fmt == "binary_little_endian":
            data = np.frombuffer(f.read(), dtype=np.dtype([(n, "<" + t) for n, t in props]), count=count)
        elif fmt == "ascii":
            flat = np.loadtxt(f, dtype=np.float64, max_rows=count).reshape(count, len(props))
            data = np.zeros(count, dtype=[(n, "<" + t) for n, t in props])
            for i, (n, _) in enumerate(props):
                data[n] = flat[:, i]
        else:
            raise ValueError(f"{path}: unsupported PLY format {fmt!r}")
    return data, [n for n, _ in props]


def read_ply_mesh(path: str):
    """What ``write_ply_mesh`` writes, back: ``(vertices float32 [V,3], faces int32 [F,3], colors uint8 [V,3] or None)`` as
    numpy arrays.  Reads binary little-endian and ascii files, any scalar vertex properties (x, y, z and, if all three are
    there, red, green, blue are used), a face list of any integer count and index type (``uchar`` counts with ``int`` /
    ``uint`` indices are the common forms); further face properties and further elements after ``face`` are not supported.
    A face that is not a triangle is refused."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: unterminated PLY header")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == "property":
                if not elements:
                    raise ValueError(f"{path}: a property before any element")
                try:
                    if tok[1] == "list":
                        elements[-1][2].append((tok[4], _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]))
                    else:
                        elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]], None))
                except (KeyError, IndexError):
                    raise ValueError(f"{path}: cannot read the property line {line!r}") from None
            elif tok[0] == "end_header":
                break
        if fmt not in ("binary_little_endian", "ascii"):
            raise ValueError(f"{path}: unsupported PLY format {fmt!r}")
        names = [e[0] for e in elements]
        if names[:1] != ["vertex"]:
            raise ValueError(f"{path}: the first element must be 'vertex'")
        if len(names) > 2 or (len(names) == 2 and names[1] != "face"):
            raise ValueError(f"{path}: elements other than 'vertex' and 'face' are not supported")
        _, V, vprops = elements[0]
        if any(p[2] is not None for p in vprops):
            raise ValueError(f"{path}: list properties of the vertex element are not supported")
        F, fprops = (elements[1][1], elements[1][2]) if len(elements) == 2 else (0, [])
        if len(elements) == 2 and (len(fprops) != 1 or fprops[0][2] is None or fprops[0][1][0] not in "iu"
                                   or fprops[0][2][0] not in "iu"):
            raise ValueError(f"{path}: the face element must hold one integer list property")
        vdtype = np.dtype([(n, "<" + t) for n, t, _ in vprops])
        if fmt == "binary_little_endian":
            raw = f.read()
            if len(raw) < V * vdtype.itemsize:
                raise ValueError(f"{path}: the file ends inside the vertex element")
            vert = np.frombuffer(raw, dtype=vdtype, count=V)
            faces = np.zeros((F, 3), dtype=np.int32)
            if F:
                fdtype = np.dtype([("n", "<" + fprops[0][1]), ("idx", "<" + fprops[0][2], (3,))])
                body = raw[V * vdtype.itemsize:]
                first = np.frombuffer(body, dtype="<" + fprops[0][1], count=1) if len(body) >= fdtype["n"].itemsize else [3]
                if int(first[0]) != 3:
                    raise ValueError(f"{path}: face 0 has {int(first[0])} vertices; only triangles are supported")
                if len(body) < F * fdtype.itemsize:
                    raise ValueError(f"{path}: the file ends inside the face element (or a face is not a triangle)")
                face = np.frombuffer(body, dtype=fdtype, count=F)
                bad = np.flatnonzero(face["n"] != 3)
                if bad.size:
                    raise ValueError(f"{path}: face {int(bad[0])} is not a triangle; only triangles are supported")
                idx = face["idx"]
        else:
            rows = [ln.split() for ln in f.read().decode("ascii", "replace").splitlines() if ln.strip()]
            if len(rows) < V + F:
                raise ValueError(f"{path}: {len(rows)} data lines for {V} vertices and {F} faces")
            vert = np.zeros(V, dtype=vdtype)
            flat = np.array([r[:len(vprops)] for r in rows[:V]], dtype=np.float64).reshape(V, len(vprops))
            for i, (n, _, _) in enumerate(vprops):
                vert[n] = flat[:, i]
            faces = np.zeros((F, 3), dtype=np.int32)
            if F:
                for k, r in enumerate(rows[V:V + F]):
                    if int(r[0]) != 3 or len(r) < 4:
                        raise ValueError(f"{path}: face {k} has {r[0]} vertices; only triangles are supported")
                idx = np.array([r[1:4] for r in rows[V:V + F]], dtype=np.int64)
        if F:
            if idx.min() < 0 or idx.max() >= V or idx.max() > np.iinfo(np.int32).max:
                raise ValueError(f"{path}: a face refers to a vertex outside 0..{V - 1}")
            faces = np.array(idx, dtype=np.int32, order="C").reshape(F, 3).copy()      # packed rows: never a view
    have = set(vert.dtype.names or ())
    if not {"x", "y", "z"} <= have:
        raise ValueError(f"{path}: the vertex element has no x, y, z")
    vertices = np.stack([np.asarray(vert[n], dtype=np.float32) for n in ("x", "y", "z")], axis=1).reshape(V, 3)
    colors = None
    if {"red", "green", "blue"} <= have:
        colors = np.stack([np.asarray(vert[n], dtype=np.uint8) for n in ("red", "green", "blue")], axis=1).reshape(V, 3)
    return vertices, faces, colors


def load_ply(path: str, max_sh_degree: int = 3, device="cpu") -> Dict[str, torch.Tensor]:
    """``GaussianModel.load_ply``: returns the raw parameter tensors in the model's layout
    (``_features_dc [P,1,3]``, ``_features_rest [P,(deg+1)^2-1,3]``), float32, on ``device``."""
    v, names = read_ply_vertices(path)
    P = v.shape[0]
    col = lambda n: np.asarray(v[n], dtype=np.float32)  # noqa: E731
    xyz = np.stack([col("x"), col("y"), col("z")], axis=1)
    f_dc = np.stack([col("f_dc_0"), col("f_dc_1"), col("f_dc_2")], axis=1).reshape(P, 3, 1)
    rest = sorted((n for n in names if n.startswith("f_rest_")), key=lambda s: int(s.split("_")[-1]))
    if len(rest) != 3 * (max_sh_degree + 1) ** 2 - 3:
        raise ValueError(f"{path}: {len(rest)} f_rest_* properties do not match SH degree {max_sh_degree}")
    f_rest = np.stack([col(n) for n in rest], axis=1).reshape(P, 3, (max_sh_degree + 1) ** 2 - 1) if rest \
        else np.zeros((P, 3, 0), np.float32)
    scales = np.stack([col(n) for n in sorted((n for n in names if n.startswith("scale_")),
                                              key=lambda s: int(s.split("_")[-1]))], axis=1)
    rots = np.stack([col(n) for n in sorted((n for n in names if n.startswith("rot")),
                                            key=lambda s: int(s.split("_")[-1]))], axis=1)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=device)  # noqa: E731
    # Mip-Splatting's extra property, only when the file has it: a standard file gives the standard dict
    extra = {"filter_3D": t(col("filter_3D"))} if "filter_3D" in names else {}
    return {"_xyz": t(xyz), "_features_dc": t(f_dc).transpose(1, 2).contiguous(),
            "_features_rest": t(f_rest).transpose(1, 2).contiguous(), "_opacity": t(col("opacity")[:, None]),
            "_scaling": t(scales), "_rotation": t(rots), "active_sh_degree": max_sh_degree, **extra}
