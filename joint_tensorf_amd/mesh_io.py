"""Triangle meshes and camera sets on disk: what `python -m joint_tensorf_amd.export` leaves behind.

PLY, binary little-endian 1.0, the layout every mesh tool reads:
    element vertex N:  property float x / y / z
    element face M:    property list uchar int vertex_indices     (a count byte 3 and three int32 per triangle)
`comments` go into the header as `comment ...` lines (one line each, ASCII); the exporter records the iso-level, the lattice size,
the box and `space world|ndc` there.  Host code in NumPy: a file write is not a hot path."""
import json

import numpy as np

_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])     # packed: 13 bytes per triangle


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def write_ply(path, vertices, triangles, comments=()):
    """vertices [nv, 3] floats, triangles [nt, 3] integers (tensors or arrays; either may be empty).  Returns the path."""
    V = np.ascontiguousarray(_host(vertices).reshape(-1, 3), dtype="<f4")
    T = _host(triangles).reshape(-1, 3)
    if len(T) and (T.min() < 0 or T.max() >= len(V)):
        raise ValueError("write_ply: a triangle names vertex %d of %d" % (int(T.max() if T.max() >= len(V) else T.min()), len(V)))
    faces = np.empty(len(T), dtype=_FACE)
    faces["n"] = 3
    faces["v"] = T
    lines = ["ply", "format binary_little_endian 1.0"]
    for c in comments:
        c = str(c)
        if "\n" in c or "\r" in c or not c.isascii():
            raise ValueError("write_ply: a comment is one ASCII line (got %r)" % c)
        lines.append("comment " + c)
    lines += ["element vertex %d" % len(V), "property float x", "property float y", "property float z",
              "element face %d" % len(T), "property list uchar int vertex_indices", "end_header"]
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
