"""Triangle meshes and camera sets on disk: what `python -m joint_tensorf_amd.export` leaves behind.

PLY, binary little-endian 1.0, the layout every mesh tool reads:
    element vertex N:  property float x / y / z  [property float nx / ny / nz]  [property uchar red / green / blue]
    element face M:    property list uchar int vertex_indices     (a count byte 3 and three int32 per triangle)
`comments` go into the header as `comment ...` lines (one line each, ASCII); the exporter records the iso-level, the lattice size,
the box and `space world|ndc` there.  A textured mesh (texture_layout, texture_uv: one chart per triangle in an atlas baked on the
device) adds `property list uchar float texcoord` to the face element (a count byte 6 and six floats) and `comment TextureFile
atlas.png`; write_obj writes the same mesh as Wavefront OBJ + MTL.  Host code in NumPy: a file write is not a hot path."""
import collections
import json
import math
import os

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


# ---- the texture atlas of a mesh: one chart per triangle (include/jt_render.h: "Texture atlas") --------------------------------
TEXTURE_MIN_BLOCK, TEXTURE_MAX_BLOCK, TEXTURE_MAX_SIDE = 4, 64, 16384
TextureLayout = collections.namedtuple("TextureLayout", "block leg n_triangles n_blocks cols rows width height n_entries")
_FACE_UV = np.dtype([("n", "u1"), ("v", "<i4", (3,)), ("tn", "u1"), ("t", "<f4", (6,))])     # packed: 38 bytes per triangle


def texture_layout(n_triangles, block):
    """The atlas of n_triangles charts in square blocks of `block` = S texels (an integer from 4 to 64): every block holds the
    right-isosceles charts, of legs S - 3 texels, of two triangles -- TextureLayout(block S, leg L = S - 3, n_triangles, n_blocks =
    ceil(nt / 2), cols = the smallest integer with cols^2 >= n_blocks, rows = ceil(n_blocks / cols), width = cols S, height = rows S,
    n_entries = n_blocks S S).  Block b sits at column b % cols and row b // cols; texel (i, j) of it -- column, row -- is entry
    b S S + j S + i and belongs to triangle 2b when i + j <= S - 1, to triangle 2b + 1 otherwise.  Pure host arithmetic.
    ValueError for a block that is no such integer, for n_triangles < 1, and when a side exceeds 16384 texels or n_entries reaches
    2^31: a smaller block or a coarser mesh (--simplify.cell) is then needed."""
    S, nt = block, n_triangles
    if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not TEXTURE_MIN_BLOCK <= int(S) <= TEXTURE_MAX_BLOCK:
        raise ValueError("texture_layout: block is an integer from %d to %d, the edge of a block in texels (got %r)"
                         % (TEXTURE_MIN_BLOCK, TEXTURE_MAX_BLOCK, S))
    if isinstance(nt, bool) or not isinstance(nt, (int, np.integer)) or int(nt) < 1:
        raise ValueError("texture_layout: n_triangles is a positive integer (got %r)" % (nt,))
    S, nt = int(S), int(nt)
    n_blocks = (nt + 1) // 2
    cols = math.isqrt(n_blocks - 1) + 1
    rows = -(-n_blocks // cols)
    W, H, n = cols * S, rows * S, n_blocks * S * S
    if W > TEXTURE_MAX_SIDE or H > TEXTURE_MAX_SIDE or n >= 1 << 31:
        raise ValueError("texture_layout: %d triangles in blocks of %d texels need an atlas of %d x %d, beyond %d a side (or 2^31 "
                         "texels): take a smaller block (--texture.block) or a coarser mesh (--simplify.cell)"
                         % (nt, S, W, H, TEXTURE_MAX_SIDE))
    return TextureLayout(S, S - 3, nt, n_blocks, cols, rows, W, H, n)


def texture_uv(layout):
    """The corners of every chart in atlas pixel units, x right and y down: [nt, 3, 2] float32, all on texel centres.  Lower chart
    (even triangles): P0 = (bx S + 0.5, by S + 0.5), P1 = P0 + (L, 0), P2 = P0 + (0, L); upper chart (odd): P0 = ((bx + 1) S - 0.5,
    (by + 1) S - 0.5), P1 = P0 - (L, 0), P2 = P0 - (0, L)."""
    S, L = layout.block, layout.leg
    t = np.arange(layout.n_triangles, dtype=np.int64)
    b, upper = t // 2, (t % 2).astype(bool)
    bx, by = b % layout.cols, b // layout.cols
    p0 = np.where(upper[:, None], np.stack([(bx + 1) * S - 0.5, (by + 1) * S - 0.5], -1), np.stack([bx * S + 0.5, by * S + 0.5], -1))
    step = np.where(upper, -float(L), float(L))[:, None]
    uv = np.stack([p0, p0 + step * np.array([1.0, 0.0]), p0 + step * np.array([0.0, 1.0])], 1)
    return uv.astype(np.float32)


def _normalised_uv(texcoords, texture_size, n_triangles, who):
    """pixel-unit corners [nt, 3, 2] -> float32 (u, v) = (x / W, 1 - y / H), the convention of image-space textures (v up)"""
    if texture_size is None or len(texture_size) != 2 or min(int(s) for s in texture_size) < 1:
        raise ValueError("%s: texcoords are in pixel units and need texture_size = (W, H) of the atlas (got %r)" % (who, texture_size))
    uv = np.asarray(_host(texcoords), dtype=np.float64)
    if uv.shape != (n_triangles, 3, 2):
        raise ValueError("%s: texcoords are [nt, 3, 2] (got %s for %d triangles)" % (who, uv.shape, n_triangles))
    W, H = (int(s) for s in texture_size)
    return np.stack([uv[..., 0] / W, 1.0 - uv[..., 1] / H], -1).astype("<f4")


def write_ply(path, vertices, triangles, comments=(), normals=None, colors=None, texcoords=None, texture_file=None,
              texture_size=None):
    """vertices [nv, 3] floats, triangles [nt, 3] integers (tensors or arrays; either may be empty); optionally per vertex
    normals [nv, 3] floats (`float nx ny nz`) and colors [nv, 3] in [0, 1] (`uchar red green blue`, quantise_colors).
    texcoords [nt, 3, 2]: the corners of every triangle in the PIXEL units of an atlas of texture_size = (W, H), x right and y
    down (texture_uv) -- the face element gains `property list uchar float texcoord`, a count byte 6 and (u, v) = (x / W, 1 - y / H)
    per corner, and the header `comment TextureFile <texture_file>` (default atlas.png) after the given comments: what MeshLab,
    CloudCompare, Open3D and trimesh read.  Without texcoords the bytes are what they always were.  Returns the path."""
    V = np.ascontiguousarray(_host(vertices).reshape(-1, 3), dtype="<f4")
    T = _host(triangles).reshape(-1, 3)
    if len(T) and (T.min() < 0 or T.max() >= len(V)):
        raise ValueError("write_ply: a triangle names vertex %d of %d" % (int(T.max() if T.max() >= len(V) else T.min()), len(V)))
    if texcoords is None and (texture_file is not None or texture_size is not None):
        raise ValueError("write_ply: texture_file / texture_size describe texcoords, and none were given")
    if texcoords is not None:
        comments = list(comments) + ["TextureFile %s" % ("atlas.png" if texture_file is None else texture_file)]
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
    faces = np.empty(len(T), dtype=_FACE if texcoords is None else _FACE_UV)
    faces["n"] = 3
    faces["v"] = T
    face_props = ["property list uchar int vertex_indices"]
    if texcoords is not None:
        faces["tn"] = 6
        faces["t"] = _normalised_uv(texcoords, texture_size, len(T), "write_ply").reshape(len(T), 6)
        face_props.append("property list uchar float texcoord")
    lines = ["ply", "format binary_little_endian 1.0"]
    for c in comments:
        c = str(c)
        if "\n" in c or "\r" in c or not c.isascii():
            raise ValueError("write_ply: a comment is one ASCII line (got %r)" % c)
        lines.append("comment " + c)
    lines += ["element vertex %d" % len(V)] + props + ["element face %d" % len(T)] + face_props + ["end_header"]
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


def read_ply_textured(path):
    """A file write_ply wrote WITH texcoords, in any of its four vertex layouts -> read_ply_attributes' dict plus texcoords
    [nt, 3, 2] float32, the (u, v) of every corner as stored (u = x / W, v = 1 - y / H), and texture_file, the name the
    `comment TextureFile` line gives (None without one; the line stays among the comments)."""
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
    match = [(n, c) for n, c, props in layouts if rest[1:-3] == props]
    try:
        nv, nt = int(rest[0].split()[2]), int(rest[-3].split()[2])
    except (IndexError, ValueError):
        match = []
    if not match or rest[0] != "element vertex %d" % nv or rest[-3:] != ["element face %d" % nt,
                                                                          "property list uchar int vertex_indices",
                                                                          "property list uchar float texcoord"]:
        raise ValueError("%s: not a textured vertex / face layout write_ply writes" % path)
    has_n, has_c = match[0]
    vdt = _vertex_dtype(has_n, has_c)
    if len(body) != vdt.itemsize * nv + _FACE_UV.itemsize * nt:
        raise ValueError("%s: %d payload bytes for %d vertices and %d textured triangles" % (path, len(body), nv, nt))
    rows = np.frombuffer(body, dtype=vdt, count=nv)
    faces = np.frombuffer(body, dtype=_FACE_UV, count=nt, offset=vdt.itemsize * nv)
    if nt and not ((faces["n"] == 3).all() and (faces["tn"] == 6).all()):
        raise ValueError("%s: a face that is not a triangle with three texture coordinates" % path)
    names = [c[len("TextureFile "):] for c in comments if c.startswith("TextureFile ")]
    return dict(vertices=np.ascontiguousarray(rows["p"], dtype=np.float32).reshape(nv, 3),
                triangles=np.ascontiguousarray(faces["v"], dtype=np.int32).reshape(nt, 3), comments=comments,
                normals=np.ascontiguousarray(rows["n"], dtype=np.float32).reshape(nv, 3) if has_n else None,
                colors=np.ascontiguousarray(rows["c"], dtype=np.uint8).reshape(nv, 3) if has_c else None,
                texcoords=np.ascontiguousarray(faces["t"], dtype=np.float32).reshape(nt, 3, 2),
                texture_file=names[0] if names else None)


def write_obj(path, vertices, triangles, texcoords, texture_size, normals=None, texture_file="atlas.png"):
    """Wavefront OBJ with a material library beside it (what Blender reads): <path> holds `mtllib`, `usemtl atlas`, one `v` per
    vertex, one `vn` per vertex when normals [nv, 3] are given, one `vt` per CORNER -- texcoords [nt, 3, 2] in the pixel units of
    an atlas of texture_size = (W, H), written as (u, v) = (x / W, 1 - y / H) in float32 -- and `f a/ta/na b/tb/nb c/tc/nc` (`a/ta`
    without normals), indices from 1; <path with .mtl> names the picture with `map_Kd <texture_file>`.  Floats are written with
    repr, so float32 values read back exactly.  Returns (path, mtl path)."""
    V = np.asarray(_host(vertices), dtype=np.float32).reshape(-1, 3)
    T = np.asarray(_host(triangles)).reshape(-1, 3).astype(np.int64)
    if len(T) and (T.min() < 0 or T.max() >= len(V)):
        raise ValueError("write_obj: a triangle names vertex %d of %d" % (int(T.max() if T.max() >= len(V) else T.min()), len(V)))
    uv = _normalised_uv(texcoords, texture_size, len(T), "write_obj").reshape(-1, 2)
    N = None
    if normals is not None:
        N = np.asarray(_host(normals), dtype=np.float32).reshape(-1, 3)
        if len(N) != len(V):
            raise ValueError("write_obj: %d vertices, %d rows of normals" % (len(V), len(N)))
    mtl = os.path.splitext(path)[0] + ".mtl"
    lines = ["# joint_tensorf_amd mesh export", "mtllib %s" % os.path.basename(mtl), "usemtl atlas"]
    lines += ["v %r %r %r" % tuple(r) for r in V.astype(np.float64).tolist()]
    if N is not None:
        lines += ["vn %r %r %r" % tuple(r) for r in N.astype(np.float64).tolist()]
    lines += ["vt %r %r" % tuple(r) for r in uv.astype(np.float64).tolist()]
    for t, (a, b, c) in enumerate((T + 1).tolist()):
        k = 3 * t
        lines.append("f %d/%d/%d %d/%d/%d %d/%d/%d" % (a, k + 1, a, b, k + 2, b, c, k + 3, c) if N is not None
                     else "f %d/%d %d/%d %d/%d" % (a, k + 1, b, k + 2, c, k + 3))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(mtl, "w") as f:
        f.write("# joint_tensorf_amd mesh export\nnewmtl atlas\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd %s\n" % texture_file)
    return path, mtl


def read_obj(path):
    """A file write_obj wrote -> dict(vertices [nv, 3] float32, normals [nv, 3] float32 or None, texcoords [n_vt, 2] float32,
    faces [nt, 3, 3] int64: per corner the 0-based (vertex, texcoord, normal) ids, normal -1 without normals, mtllib, usemtl)."""
    rows = {"v": [], "vn": [], "vt": [], "f": []}
    names = {"mtllib": None, "usemtl": None}
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if not parts or parts[0].startswith("#"):
                continue
            if parts[0] in names:
                names[parts[0]] = parts[1]
            elif parts[0] == "f":
                rows["f"].append([[int(x) - 1 for x in (c.split("/") + ["0"])[:3]] for c in parts[1:]])
            elif parts[0] in rows:
                rows[parts[0]].append([float(x) for x in parts[1:]])
            else:
                raise ValueError("%s: a line write_obj does not write: %r" % (path, ln))
    return dict(vertices=np.asarray(rows["v"], dtype=np.float32).reshape(-1, 3),
                normals=np.asarray(rows["vn"], dtype=np.float32).reshape(-1, 3) if rows["vn"] else None,
                texcoords=np.asarray(rows["vt"], dtype=np.float32).reshape(-1, 2),
                faces=np.asarray(rows["f"], dtype=np.int64).reshape(-1, 3, 3), **names)


def read_mtl(path):
    """the `map_Kd` name of a material library write_obj wrote (None without one)"""
    with open(path) as f:
        maps = [ln.split(None, 1)[1].strip() for ln in f if ln.startswith("map_Kd ")]
    return maps[0] if maps else None


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
    mesh_ops.rasterize draws through -- from world-to-camera poses [V, 3, 4] ([R | t]) and intrinsics [V, 3, 3], as the views of a
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
