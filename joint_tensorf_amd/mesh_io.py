"""Triangle meshes and camera sets on disk: what `python -m joint_tensorf_amd.export` leaves behind.

PLY, binary little-endian 1.0, the layout every mesh tool reads:
    element vertex N:  property float x / y / z  [property float nx / ny / nz]  [property uchar red / green / blue]
    element face M:    property list uchar int vertex_indices     (a count byte 3 and three int32 per triangle)
`comments` go into the header as `comment ...` lines (one line each, ASCII); the exporter records the iso-level, the lattice size,
the box and `space world|ndc` there.  Host code in NumPy: a file write is not a hot path."""
import json

import numpy as np

_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])     # packed: 13 bytes per triangle


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


_VERTEX_PROPS = ["property float x", "property float y", "property float z"]
_NORMAL_PROPS = ["property float nx", "property float ny", "property float nz"]
_COLOR_PROPS = ["property uchar red", "property uchar green", "property uchar blue"]


def quantise_colors(colors):
    """colours [n, 3] in [0, 1] -> uint8 floor(255 c + 0.5), clamped to 0 .. 255; a NaN is refused"""
    C = np.asarray(_host(colors), dtype=np.float64).reshape(-1, 3)
    if np.isnan(C).any():
        raise ValueError("write_ply: a colour is NaN")
    return np.clip(np.floor(255.0 * C + 0.5), 0, 255).astype(np.uint8)


def _vertex_dtype(normals, colors):
    fields = [("p", "<f4", (3,))]
    if normals:
        fields.append(("n", "<f4", (3,)))
    if colors:
        fields.append(("c", "u1", (3,)))
    return np.dtype(fields)                                  # packed: 12, 24, 15 or 27 bytes per vertex


def write_ply(path, vertices, triangles, comments=(), normals=None, colors=None):
    """vertices [nv, 3] floats, triangles [nt, 3] integers (tensors or arrays; either may be empty); optionally per vertex
    normals [nv, 3] floats (`float nx ny nz`) and colors [nv, 3] in [0, 1] (`uchar red green blue`, quantise_colors).
    Returns the path."""
    V = np.ascontiguousarray(_host(vertices).reshape(-1, 3), dtype="<f4")
    T = _host(triangles).reshape(-1, 3)
    if len(T) and (T.min() < 0 or T.max() >= len(V)):
        raise ValueError("write_ply: a triangle names vertex %d of %d" % (int(T.max() if T.max() >= len(V) else T.min()), len(V)))
    props = list(_VERTEX_PROPS)
    if normals is not None or colors is not None:
        rows = np.empty(len(V), dtype=_vertex_dtype(normals is not None, colors is not None))
        rows["p"] = V
        for name, a, plist in (("n", normals, _NORMAL_PROPS), ("c", colors, _COLOR_PROPS)):
            if a is None:
                continue
            a = quantise_colors(a) if name == "c" else np.asarray(_host(a), dtype="<f4").reshape(-1, 3)
            if len(a) != len(V):
                raise ValueError("write_ply: %d vertices, %d rows of %s" % (len(V), len(a), "colors" if name == "c" else "normals"))
            rows[name] = a
            props += plist
        V = rows
    faces = np.empty(len(T), dtype=_FACE)
    faces["n"] = 3
    faces["v"] = T
    lines = ["ply", "format binary_little_endian 1.0"]
    for c in comments:
        c = str(c)
        if "\n" in c or "\r" in c or not c.isascii():
            raise ValueError("write_ply: a comment is one ASCII line (got %r)" % c)
        lines.append("comment " + c)
    lines += ["element vertex %d" % len(V)] + props + ["element face %d" % len(T), "property list uchar int vertex_indices",
                                                       "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(lines) + "\n").encode("ascii"))
        f.write(V.tobytes())
        f.write(faces.tobytes())
    return path


def read_ply(path):
    """A file write_ply wrote (this header layout only, triangles only) -> (vertices [nv, 3] float32, triangles [nt, 3] int32,
    comments: list of str)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError("%s is not a PLY file" % path)
    head = data[:end].decode("ascii").split("\n")[1:]
    body = data[end + len(b"end_header\n"):]
    if not head or head[0] != "format binary_little_endian 1.0":
        raise ValueError("%s: only binary little-endian PLY is read" % path)
    comments = [ln[len("comment "):] for ln in head if ln.startswith("comment ")]
    rest = [ln for ln in head[1:] if ln and not ln.startswith("comment ")]
    nv, nt = int(rest[0].split()[2]), int(rest[4].split()[2])
    if rest != ["element vertex %d" % nv, "property float x", "property float y", "property float z", "element face %d" % nt,
                "property list uchar int vertex_indices"]:
        raise ValueError("%s: not the vertex / face layout write_ply writes" % path)
    if len(body) != 12 * nv + _FACE.itemsize * nt:
        raise ValueError("%s: %d payload bytes for %d vertices and %d triangles" % (path, len(body), nv, nt))
    V = np.frombuffer(body, dtype="<f4", count=3 * nv).reshape(nv, 3).astype(np.float32)
    faces = np.frombuffer(body, dtype=_FACE, count=nt, offset=12 * nv)
    if nt and not (faces["n"] == 3).all():
        raise ValueError("%s: a face that is not a triangle" % path)
    return V, np.ascontiguousarray(faces["v"], dtype=np.int32).reshape(nt, 3), comments


def read_ply_attributes(path):
    """A file write_ply wrote, in any of its four vertex layouts (plain, + normals, + colours, + both) -> dict(vertices [nv, 3]
    float32, triangles [nt, 3] int32, comments: list of str, normals [nv, 3] float32 or None, colors [nv, 3] uint8 or None)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError("%s is not a PLY file" % path)
    head = data[:end].decode("ascii").split("\n")[1:]
    body = data[end + len(b"end_header\n"):]
    if not head or head[0] != "format binary_little_endian 1.0":
        raise ValueError("%s: only binary little-endian PLY is read" % path)
    comments = [ln[len("comment "):] for ln in head if ln.startswith("comment ")]
    rest = [ln for ln in head[1:] if ln and not ln.startswith("comment ")]
    layouts = [(n, c, _VERTEX_PROPS + (_NORMAL_PROPS if n else []) + (_COLOR_PROPS if c else []))
               for n in (False, True) for c in (False, True)]
    match = [(n, c) for n, c, props in layouts if rest[1:-2] == props]
    if not match:
        raise ValueError("%s: not a vertex / face layout write_ply writes" % path)
    has_n, has_c = match[0]
    try:
        nv, nt = int(rest[0].split()[2]), int(rest[-2].split()[2])
    except (IndexError, ValueError):
        raise ValueError("%s: not a vertex / face layout write_ply writes" % path) from None
    if rest[0] != "element vertex %d" % nv or rest[-2:] != ["element face %d" % nt, "property list uchar int vertex_indices"]:
        raise ValueError("%s: not a vertex / face layout write_ply writes" % path)
    vdt = _vertex_dtype(has_n, has_c)
    if len(body) != vdt.itemsize * nv + _FACE.itemsize * nt:
        raise ValueError("%s: %d payload bytes for %d vertices and %d triangles" % (path, len(body), nv, nt))
    rows = np.frombuffer(body, dtype=vdt, count=nv)
    faces = np.frombuffer(body, dtype=_FACE, count=nt, offset=vdt.itemsize * nv)
    if nt and not (faces["n"] == 3).all():
        raise ValueError("%s: a face that is not a triangle" % path)
    return dict(vertices=np.ascontiguousarray(rows["p"], dtype=np.float32).reshape(nv, 3),
                triangles=np.ascontiguousarray(faces["v"], dtype=np.int32).reshape(nt, 3), comments=comments,
                normals=np.ascontiguousarray(rows["n"], dtype=np.float32).reshape(nv, 3) if has_n else None,
                colors=np.ascontiguousarray(rows["c"], dtype=np.uint8).reshape(nv, 3) if has_c else None)


def mesh_comments(level, shape, lo, hi, space):
    """the header lines of an exported mesh: iso-level, lattice size, box and coordinate space (`world` or `ndc`)"""
    if space not in ("world", "ndc"):
        raise ValueError("space is world or ndc (got %r)" % (space,))
    return ["joint_tensorf_amd mesh export", "level %r" % float(level), "lattice %d %d %d" % tuple(int(v) for v in shape),
            "box_lo %r %r %r" % tuple(float(v) for v in lo), "box_hi %r %r %r" % tuple(float(v) for v in hi), "space %s" % space]


def write_cameras(path, cameras):
    """cameras: a plain dict of lists / numbers / strings (Model.export_scene builds it) as indented JSON; floats are written
    with repr, so float32 values read back exactly."""
    with open(path, "w") as f:
        json.dump(cameras, f, indent=1)
        f.write("\n")
    return path


def read_cameras(path):
    with open(path) as f:
        return json.load(f)


def projection_matrices(pose, intr, size=None, image_size=None):
    """[V, 3, 4] matrices intr @ pose that take a homogeneous mesh-space point to (x w, y w, w) in pixel units -- what
    ops.rasterize draws through -- from world-to-camera poses [V, 3, 4] ([R | t]) and intrinsics [V, 3, 3], as the views of a
    cameras.json hold them (tensors or arrays; the result is of the kind of `pose`).  size = (H, W) renders at another size
    than the image_size = (H, W) the intrinsics belong to: their first row is scaled by W / W0 and their second by H / H0, as the
    loaders rescale them when they resize an image set (datasets.py).  Pixel centres are at half-integers, as for the ray
    generator, so a vertex lands where the field's rays see it."""
    if len(pose.shape) != 3 or tuple(pose.shape[1:]) != (3, 4) or tuple(intr.shape) != (pose.shape[0], 3, 3):
        raise ValueError("projection_matrices: pose is [V, 3, 4] and intr [V, 3, 3] (got %s, %s)" % (tuple(pose.shape), tuple(intr.shape)))
    P = intr @ pose
    if size is None:
        return P
    if image_size is None:
        raise ValueError("projection_matrices: size = %r needs the image_size the intrinsics belong to" % (size,))
    (H, W), (H0, W0) = (int(v) for v in size), (int(v) for v in image_size)
    if min(H, W, H0, W0) < 1:
        raise ValueError("projection_matrices: sizes are positive (got %r, %r)" % (size, image_size))
    if (H, W) == (H0, W0):
        return P
    scale = [W / W0, H / H0, 1.0]
    scale = P.new_tensor(scale) if hasattr(P, "new_tensor") else np.asarray(scale, dtype=P.dtype)
    return scale[None, :, None] * P
