"""The export pipeline's wrappers over the C ABI (include/jt_render.h): lattice and extraction, NDC unwarp, compaction,
simplification, components, the rasteriser, the texture atlas, visibility and depth-map fusion.  No autograd, no training state: tensors in,
tensors out on torch's current stream.  `ops` re-exports every name of __all__, so `ops.X` is `mesh_ops.X`; this module never
imports `ops`.
"""
import ctypes
import math

import torch

from ._lib import _stream, check, lib, ptr

__all__ = [
    "mesh_count", "mesh_offsets", "mesh_emit", "mesh_from_lattice", "cap_lattice", "UNWARP_STATUS", "ndc_to_world", "compact_mesh",
    "SIMPLIFY_REGULAR", "SIMPLIFY_MAX_CELLS", "simplify_cells", "simplify_keys", "simplify_segments", "simplify_mesh",
    "simplify_index", "simplify_clusters", "simplify_triangles", "simplify_compact", "COMPONENTS_TILE", "COMPONENTS_MAX_SWEEPS",
    "last_components_stats", "lattice_components", "component_sizes", "keep_components", "RASTER_STATUS", "RASTER_MAX_ATTRS",
    "raster_project", "raster_draw", "raster_resolve", "texture_layout", "texture_texels", "texture_pack", "raster_resolve_texture",
    "rasterize", "visible_tally", "visible_fold", "triangle_visibility", "grow_triangles", "select_triangles", "visible_options",
    "visible_triangles", "fusion_state", "fusion_integrate", "fusion_lattice", "fused_cells", "mesh_from_fused_lattice", "fusion_options",
]


# ---- argument checks: `who` is the entry point the caller of the helper answers for, and heads the message ---------------
def _lattice_arg(vol, who):
    if vol.dim() != 3 or vol.dtype != torch.float32 or not vol.is_contiguous():
        raise ValueError("%s: the lattice must be contiguous fp32 [nx, ny, nz] (got %s %s)" % (who, vol.dtype, tuple(vol.shape)))
    return vol.shape


def _box_arg(who, lo, hi):
    lo = [float(v) for v in (lo.tolist() if torch.is_tensor(lo) else lo)]
    hi = [float(v) for v in (hi.tolist() if torch.is_tensor(hi) else hi)]
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("%s: lo and hi are three floats each" % who)
    return lo, hi


def _mesh_arg(who, vertices, triangles):
    """(vertices [nv, 3] fp32, triangles [nt, 3] int32), detached and contiguous"""
    if vertices.dim() != 2 or vertices.shape[1] != 3 or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError("%s: vertices are [nv, 3] and triangles [nt, 3] (got %s, %s)" % (who, tuple(vertices.shape), tuple(triangles.shape)))
    if triangles.dtype != torch.int32:
        raise ValueError("%s: triangles are int32 vertex ids (got %s)" % (who, triangles.dtype))
    return vertices.detach().contiguous().float(), triangles.detach().contiguous()


def _vertex_attr(who, name, a, nv):
    """optional normals or colours [nv, 3] as detached contiguous fp32, None staying None"""
    if a is None:
        return None
    if tuple(a.shape) != (nv, 3):
        raise ValueError("%s: %s are [nv, 3] (got %s for %d vertices)" % (who, name, tuple(a.shape), nv))
    return a.detach().contiguous().float()


def _empty_mesh(vertices, triangles, normals, colors):
    return (vertices.new_empty(0, 3), triangles.new_empty(0, 3), None if normals is None else normals.new_empty(0, 3),
            None if colors is None else colors.new_empty(0, 3))


def _byte_popcount(x):
    """bits set in every byte of a uint8 tensor, as uint8 (three element-wise folds: no [N] gather index)"""
    x = (x & 0x55) + ((x >> 1) & 0x55)
    x = (x & 0x33) + ((x >> 2) & 0x33)
    return (x & 0x0F) + (x >> 4)


def mesh_count(vol, level):
    """jt_mesh_count on a lattice vol [nx, ny, nz] fp32: (edge_flags [N] uint8, tri_count [N] uint8), one launch"""
    nx, ny, nz = _lattice_arg(vol, "mesh_from_lattice")
    flags = torch.empty(vol.numel(), device=vol.device, dtype=torch.uint8)
    tris = torch.empty(vol.numel(), device=vol.device, dtype=torch.uint8)
    check(lib.jt_mesh_count(ptr(vol), nx, ny, nz, float(level), ptr(flags), ptr(tris), _stream()), "jt_mesh_count")
    return flags, tris


def mesh_offsets(flags, tris):
    """the caller's scan between the two passes: (vert_offset [N] int64, tri_offset [N] int64, totals [2] int64 = (n_vertices,
    n_triangles)), all on the device -- no host read"""
    verts = _byte_popcount(flags)
    vert_end = torch.cumsum(verts, 0, dtype=torch.int64)
    tri_end = torch.cumsum(tris, 0, dtype=torch.int64)
    totals = torch.stack([vert_end[-1], tri_end[-1]])
    return vert_end.sub_(verts), tri_end.sub_(tris), totals


def mesh_emit(vol, level, lo, hi, flags, vert_offset, tri_offset, nv, nt):
    """jt_mesh_emit: (vertices [nv, 3] fp32, triangles [nt, 3] int32); nothing is launched for an empty mesh"""
    vertices = torch.empty(nv, 3, device=vol.device, dtype=torch.float32)
    triangles = torch.empty(nt, 3, device=vol.device, dtype=torch.int32)
    if nv:
        nx, ny, nz = vol.shape
        check(lib.jt_mesh_emit(ptr(vol), nx, ny, nz, float(level), (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*hi), ptr(flags),
                               ptr(vert_offset), ptr(tri_offset), nv, nt, ptr(vertices), ptr(triangles), _stream()),
              "jt_mesh_emit")
    return vertices, triangles


def mesh_from_lattice(vol, level, lo, hi):
    """The iso-surface {vol = level} of a lattice vol [nx, ny, nz] fp32 (z fastest, as getDenseAlpha returns it) over the box lo
    .. hi (three floats each) as a triangle mesh on the device: vertices [nv, 3] fp32, triangles [nt, 3] int32, normals
    (right-hand rule) from inside (vol > level) to outside.  Marching tetrahedra on the Kuhn triangulation (csrc/jt_mesh.hip):
    jt_mesh_count, two cumsums, ONE host read of the two totals, jt_mesh_emit.  No atomics: the order of vertices and
    triangles is a function of the lattice alone, two calls return the same bits.  Empty results are [0, 3] tensors."""
    lo, hi = _box_arg("mesh_from_lattice", lo, hi)
    vol = vol.detach().contiguous()
    flags, tris = mesh_count(vol, level)
    vert_offset, tri_offset, totals = mesh_offsets(flags, tris)
    nv, nt = (int(v) for v in totals.tolist())
    return mesh_emit(vol, level, lo, hi, flags, vert_offset, tri_offset, nv, nt)


def cap_lattice(vol, lo, hi):
    """One layer of zeros round a lattice and the box grown by one lattice spacing per side (fp32 arithmetic on the host): a
    surface {vol = level > 0} that reaches the box is closed there.  Returns (padded lattice, lo, hi)."""
    shape = torch.tensor(list(vol.shape), dtype=torch.float32)
    lo, hi = torch.as_tensor(lo, dtype=torch.float32).cpu().reshape(3), torch.as_tensor(hi, dtype=torch.float32).cpu().reshape(3)
    unit = (hi - lo) / (shape - 1)
    return torch.nn.functional.pad(vol, (1, 1, 1, 1, 1, 1)), (lo - unit).tolist(), (hi + unit).tolist()


# what jt_mesh_unwarp_ndc's status bytes say (include/jt_render.h: JT_UNWARP_*)
UNWARP_STATUS = ("kept", "beyond", "far")


def ndc_to_world(vertices, sx, sy, near, normals=None, max_depth=None):
    """Vertices [n, 3] fp32 of an NDC scene (xn = sx x/z, yn = sy y/z, zn = 1 - 2 near/z, as the ray generator has it) carried to
    world space on the device (jt_mesh_unwarp_ndc, one launch): (world [n, 3], world_normals [n, 3] or None without `normals`
    [n, 3], status [n] uint8: 0 kept, 1 beyond (non-finite, at or behind infinity: zn >= 1), 2 far (max_depth given and z >
    max_depth)).  u = 1 - zn, z = 2 near / u, x = xn z / sx, y = yn z / sy; a normal goes through J^T: (sx nx, sy ny, u nz - xn nx
    - yn ny) normalised, (0, 0, 0) staying (0, 0, 0).  A vertex that is not kept comes back as zeros."""
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.shape[0] < 1:
        raise ValueError("ndc_to_world: vertices are [n, 3] with n >= 1 (got %s)" % (tuple(vertices.shape),))
    vertices = vertices.detach().contiguous().float()
    n = vertices.shape[0]
    if normals is not None:
        if tuple(normals.shape) != (n, 3):
            raise ValueError("ndc_to_world: one normal per vertex (got %s for %d vertices)" % (tuple(normals.shape), n))
        normals = normals.detach().contiguous().float()
    if max_depth is not None and not (float(max_depth) > 0 and math.isfinite(float(max_depth))):
        raise ValueError("ndc_to_world: max_depth is a positive finite number or None (got %r)" % (max_depth,))
    world = torch.empty_like(vertices)
    world_normals = torch.empty_like(normals) if normals is not None else None
    status = torch.empty(n, device=vertices.device, dtype=torch.uint8)
    check(lib.jt_mesh_unwarp_ndc(ptr(vertices), ptr(normals), n, float(sx), float(sy), float(near),
                                 0.0 if max_depth is None else float(max_depth), ptr(world), ptr(world_normals), ptr(status),
                                 _stream()), "jt_mesh_unwarp_ndc")
    return world, world_normals, status


def _compact(vertices, normals, colors, triangles, keep, used, tallies=()):
    """The one compaction behind compact_mesh, simplify_compact and select_triangles: the triangles with keep[t] != 0 and the
    vertices with used[v] != 0 (both uint8, a count kernel's), in their order, ids remapped.  Two cumsums, ONE host read -- the
    two sizes and `tallies` (0-d device tensors that ride along) --, jt_mesh_filter_emit.  Returns (vertices', triangles',
    normals' or None, colors' or None, vert_offset [nv] int64, nv', the tallies as ints); the five arrays are None and
    nothing is emitted when no triangle is kept."""
    nv, nt, dev = vertices.shape[0], triangles.shape[0], vertices.device
    vert_end = torch.cumsum(used, 0, dtype=torch.int64)
    tri_end = torch.cumsum(keep, 0, dtype=torch.int64)
    nv_out, nt_out, *tallies = (int(v) for v in torch.stack([vert_end[-1], tri_end[-1], *tallies]).tolist())
    if nt_out == 0:
        return None, None, None, None, None, 0, tuple(tallies)
    vert_offset, tri_offset = vert_end.sub_(used), tri_end.sub_(keep)
    v_out = torch.empty(nv_out, 3, device=dev, dtype=torch.float32)
    t_out = torch.empty(nt_out, 3, device=dev, dtype=torch.int32)
    n_out = torch.empty(nv_out, 3, device=dev, dtype=torch.float32) if normals is not None else None
    c_out = torch.empty(nv_out, 3, device=dev, dtype=torch.float32) if colors is not None else None
    check(lib.jt_mesh_filter_emit(ptr(vertices), ptr(normals), ptr(colors), nv, ptr(triangles), nt, ptr(keep), ptr(used),
                                  ptr(vert_offset), ptr(tri_offset), nv_out, nt_out, ptr(v_out), ptr(n_out), ptr(c_out), ptr(t_out),
                                  _stream()), "jt_mesh_filter_emit")
    return v_out, t_out, n_out, c_out, vert_offset, nv_out, tuple(tallies)


def compact_mesh(vertices, triangles, status, normals=None, colors=None):
    """The mesh without the triangles that have a vertex of status != 0 (ndc_to_world's) or an id out of range, and without the
    vertices no kept triangle names: (vertices' [nv', 3], triangles' [nt', 3] int32 with remapped ids, normals' or None, colors' or
    None, (n_dropped_beyond, n_dropped_far)) -- a dropped triangle is counted once, by the first that applies of beyond, far.
    jt_mesh_filter_count, two cumsums, ONE host read (the two sizes and the two counts), jt_mesh_filter_emit: triangles and
    vertices keep their order, two calls return the same bits.  Empty results are [0, 3] tensors."""
    vertices, triangles = _mesh_arg("compact_mesh", vertices, triangles)
    nv, nt, dev = vertices.shape[0], triangles.shape[0], vertices.device
    if status.dtype != torch.uint8 or tuple(status.shape) != (nv,):
        raise ValueError("compact_mesh: status is uint8 [nv] (got %s %s for %d vertices)" % (status.dtype, tuple(status.shape), nv))
    status = status.contiguous()
    normals, colors = _vertex_attr("compact_mesh", "normals", normals, nv), _vertex_attr("compact_mesh", "colors", colors, nv)
    if nv == 0 or nt == 0:
        return _empty_mesh(vertices, triangles, normals, colors) + ((0, 0),)
    keep = torch.empty(nt, device=dev, dtype=torch.uint8)
    cause = torch.empty(nt, device=dev, dtype=torch.uint8)
    used = torch.zeros(nv, device=dev, dtype=torch.uint8)
    check(lib.jt_mesh_filter_count(ptr(triangles), nt, ptr(status), nv, ptr(keep), ptr(cause), ptr(used), _stream()),
          "jt_mesh_filter_count")
    out = _compact(vertices, normals, colors, triangles, keep, used, ((cause == 1).sum(), (cause == 2).sum()))
    return (_empty_mesh(vertices, triangles, normals, colors) if out[1] is None else out[:4]) + (out[6],)


# the regularisation of simplify_mesh's quadric towards the cluster mean (include/jt_render.h: lambda)
SIMPLIFY_REGULAR = 1.0 / 16.0
SIMPLIFY_MAX_CELLS = 1 << 20


def simplify_cells(cells):
    """`cells` of simplify_mesh as three ints: one int (the same on every axis) or three, each in 1 .. 2^20"""
    given = cells
    if torch.is_tensor(cells):
        cells = cells.tolist()
    if not isinstance(cells, (list, tuple)):
        cells = [cells] * 3
    if (len(cells) != 3 or any(isinstance(c, bool) or float(c) != int(c) for c in cells)
            or not all(1 <= int(c) <= SIMPLIFY_MAX_CELLS for c in cells)):
        raise ValueError("simplify_mesh: cells is one int or three, each from 1 to %d (got %r)" % (SIMPLIFY_MAX_CELLS, given))
    return [int(c) for c in cells]


def simplify_keys(vertices, lo, hi, cells):
    """jt_simplify_keys: the cell key [n] int64 of every vertex of vertices [n, 3] fp32 (cx cy cz for a non-finite one), one launch"""
    keys = torch.empty(vertices.shape[0], device=vertices.device, dtype=torch.int64)
    check(lib.jt_simplify_keys(ptr(vertices), vertices.shape[0], (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*hi),
                               (ctypes.c_int * 3)(*cells), ptr(keys), _stream()), "jt_simplify_keys")
    return keys


def simplify_segments(keys, none_key):
    """the caller's sort and scan between jt_simplify_keys and jt_simplify_clusters, all on the device: (order [n] int64: vertex
    ids sorted stably by key, head [n] bool: sorted positions where a cluster begins, cid [n] int64: cluster index of every
    sorted position, valid [n] bool: positions with a key below none_key, totals [2] int64 = (n_clusters, n_valid))"""
    ks, order = torch.sort(keys, stable=True)
    valid = ks < none_key
    head = torch.ones_like(valid)
    head[1:] = ks[1:] != ks[:-1]
    head &= valid
    cid = torch.cumsum(head, 0, dtype=torch.int64)
    totals = torch.stack([cid[-1], valid.sum()])
    return order, head, cid.sub_(1), valid, totals


def _masked_rows(values, mask, offsets, n_out):
    """values[mask] when offsets is the exclusive scan of mask and n_out its total, without the host read of a boolean index:
    rows that are not wanted go to a slot past the end"""
    out = values.new_empty((n_out + 1,) + tuple(values.shape[1:]))
    out[torch.where(mask, offsets, torch.full_like(offsets, n_out))] = values
    return out[:n_out]


def simplify_mesh(vertices, triangles, normals, lo, hi, cells, regular=SIMPLIFY_REGULAR):
    """The mesh simplified by vertex clustering on the device (csrc/jt_simplify.hip): vertices [nv, 3] fp32 are binned into a
    uniform grid of `cells` (one int or three, each 1 .. 2^20) cells over the box lo .. hi (three floats each; a vertex outside
    is clamped into the border cells), every occupied cell becomes one vertex -- where the planes (vertex, normal) of its members
    meet in the least-squares sense, regularised towards their mean by `regular`, never outside the members' bounding box --,
    triangles [nt, 3] int32 are re-indexed and the collapsed ones dropped.  normals [nv, 3] fp32 are required.

    Returns (vertices' [nv', 3], triangles' [nt', 3] int32, normals' [nv', 3]: the normalised sum of the members' normals,
    counts' [nv'] int32: members per vertex, (n_dropped_invalid, n_collapsed)): a dropped triangle is counted once, by the first
    that applies of invalid (an id out of range or a vertex with a non-finite coordinate) and collapsed (two corners in one
    cell).  Vertices come in the order of their cells (x slowest), kept triangles in their original order; duplicate triangles
    are not removed.  jt_simplify_keys, a stable sort and a scan, ONE host read (the cluster count), jt_simplify_clusters,
    jt_simplify_triangles, two cumsums, ONE host read (the two sizes and the two counts), jt_mesh_filter_emit.  No atomics: two
    calls return the same bits.  Eager only (the host reads size the outputs).  Empty results are [0, 3] tensors."""
    vertices, triangles = _mesh_arg("simplify_mesh", vertices, triangles)
    nv, nt, dev = vertices.shape[0], triangles.shape[0], vertices.device
    if normals is None or tuple(normals.shape) != (nv, 3):
        raise ValueError("simplify_mesh: one normal per vertex, [nv, 3] (got %s for %d vertices)"
                         % (None if normals is None else tuple(normals.shape), nv))
    lo, hi = _box_arg("simplify_mesh", lo, hi)
    cells = simplify_cells(cells)
    regular = float(regular)
    if not (regular > 0 and math.isfinite(regular)):
        raise ValueError("simplify_mesh: regular is a positive finite number (got %r)" % (regular,))
    normals = normals.detach().contiguous().float()

    def empty(counts):
        return (vertices.new_empty(0, 3), triangles.new_empty(0, 3), normals.new_empty(0, 3),
                torch.empty(0, device=dev, dtype=torch.int32), counts)
    if nv == 0 or nt == 0:
        return empty((0, 0))
    keys = simplify_keys(vertices, lo, hi, cells)
    order, head, cid, valid, totals = simplify_segments(keys, cells[0] * cells[1] * cells[2])
    nc, n_valid = (int(v) for v in totals.tolist())
    if nc == 0:
        return empty((nt, 0))          # every vertex is non-finite: every triangle is invalid
    seg_start, cluster = simplify_index(order, head, cid, valid, nc, n_valid)
    c_pos, c_nrm, c_cnt = simplify_clusters(vertices, normals, order, seg_start, regular)
    tri, keep, cause, used = simplify_triangles(triangles, cluster, nc)
    out = simplify_compact(c_pos, c_nrm, c_cnt, tri, keep, cause, used)
    return empty(out[4]) if out[1] is None else out


def simplify_index(order, head, cid, valid, nc, n_valid):
    """what the two kernels index with, from simplify_segments' scan and its two totals: (seg_start [nc + 1] int64: where the
    clusters begin in `order`, and the number of valid vertices; cluster [n] int32: the cluster of every vertex, -1 for none)"""
    pos = torch.arange(order.shape[0], device=order.device, dtype=torch.int64)
    seg_start = torch.cat([_masked_rows(pos, head, cid, nc), pos.new_tensor([n_valid])])
    cluster = torch.empty(order.shape[0], device=order.device, dtype=torch.int32)
    cluster[order] = torch.where(valid, cid, torch.full_like(cid, -1)).to(torch.int32)
    return seg_start, cluster


def simplify_clusters(vertices, normals, order, seg_start, regular=SIMPLIFY_REGULAR):
    """jt_simplify_clusters, one launch: (positions [nc, 3] fp32, normals [nc, 3] fp32, counts [nc] int32) of the clusters"""
    nc, dev = seg_start.shape[0] - 1, vertices.device
    c_pos = torch.empty(nc, 3, device=dev, dtype=torch.float32)
    c_nrm = torch.empty(nc, 3, device=dev, dtype=torch.float32)
    c_cnt = torch.empty(nc, device=dev, dtype=torch.int32)
    check(lib.jt_simplify_clusters(ptr(vertices), ptr(normals), vertices.shape[0], ptr(order), ptr(seg_start), nc, float(regular),
                                   ptr(c_pos), ptr(c_nrm), ptr(c_cnt), _stream()), "jt_simplify_clusters")
    return c_pos, c_nrm, c_cnt


def simplify_triangles(triangles, cluster, nc):
    """jt_simplify_triangles, one launch: (triangles in cluster ids [nt, 3] int32, keep [nt] uint8, cause [nt] uint8: 0 kept, 1
    invalid, 2 collapsed, used [nc] uint8)"""
    nt, dev = triangles.shape[0], triangles.device
    tri = torch.empty_like(triangles)
    keep = torch.empty(nt, device=dev, dtype=torch.uint8)
    cause = torch.empty(nt, device=dev, dtype=torch.uint8)
    used = torch.zeros(nc, device=dev, dtype=torch.uint8)
    check(lib.jt_simplify_triangles(ptr(triangles), nt, ptr(cluster), cluster.shape[0], nc, ptr(tri), ptr(keep), ptr(cause),
                                    ptr(used), _stream()), "jt_simplify_triangles")
    return tri, keep, cause, used


def simplify_compact(c_pos, c_nrm, c_cnt, tri, keep, cause, used):
    """the compaction behind jt_simplify_triangles: two cumsums, ONE host read (the two sizes and the two counts),
    jt_mesh_filter_emit: (vertices', triangles', normals', counts', (n_dropped_invalid, n_collapsed)); the four arrays are None
    when no triangle is kept"""
    v_out, t_out, n_out, _, vert_offset, nv_out, counts = _compact(c_pos, c_nrm, None, tri, keep, used,
                                                                   ((cause == 1).sum(), (cause == 2).sum()))
    if t_out is None:
        return None, None, None, None, counts
    return v_out, t_out, n_out, _masked_rows(c_cnt, used.bool(), vert_offset, nv_out), counts


# points per edge of the tile a workgroup of the component sweep owns (include/jt_render.h: JT_COMPONENTS_TILE)
COMPONENTS_TILE = 8
# Sweeps after which lattice_components gives up.  Measured with pointer jumping (profiles/mesh_surface_export.txt): the two
# snakes through 17 x 17 x 9 of tests/test_gpu_components.py converge at sweep 14, the 400^3 blob lattice at sweep 13 (35 and 41
# without the jumps).  The default is 64 times the larger count rounded up to 16: room for paths far longer than any surface of
# a trained field winds, and still a bound (0.28 ms per sweep and jump at 400^3: a third of a second).
COMPONENTS_MAX_SWEEPS = 1024
# what the last lattice_components call took: sweeps launched, and the first sweep that lowered nothing
last_components_stats = {}


def lattice_components(vol, level, max_sweeps=None, check_every=8, jump=True):
    """Connected components of the inside points (vol > level; a NaN is outside) of a lattice vol [nx, ny, nz] fp32 under the
    connectivity of the mesh (the 14 neighbours along the seven edge kinds of csrc/jt_mesh.hip): labels [nx, ny, nz] int32, -1
    outside, else the smallest flat index of the point's component -- the same bits on every run (csrc/jt_components.hip).

    The host loop: `check_every` sweeps (each followed by a pointer-jumping launch when `jump`), each with a flag word of its
    own, then ONE host read of the flags; done when a sweep lowered nothing.  After `max_sweeps` (COMPONENTS_MAX_SWEEPS) sweeps
    without that a RuntimeError: unconverged labels are never returned."""
    nx, ny, nz = _lattice_arg(vol, "lattice_components")
    max_sweeps = COMPONENTS_MAX_SWEEPS if max_sweeps is None else int(max_sweeps)
    check_every = int(check_every)
    if max_sweeps < 1 or check_every < 1:
        raise ValueError("lattice_components: max_sweeps and check_every are at least 1 (got %r, %r)" % (max_sweeps, check_every))
    st = _stream()
    labels = torch.empty(nx, ny, nz, device=vol.device, dtype=torch.int32)
    check(lib.jt_components_init(ptr(vol), nx, ny, nz, float(level), ptr(labels), st), "jt_components_init")
    flags = torch.empty(check_every, device=vol.device, dtype=torch.int32)
    done = 0
    while done < max_sweeps:
        batch = min(check_every, max_sweeps - done)
        flags.zero_()
        for s in range(batch):
            check(lib.jt_components_sweep(ptr(labels), nx, ny, nz, flags.data_ptr() + 4 * s, int(bool(jump)), st),
                  "jt_components_sweep")
        lowered = flags[:batch].tolist()
        if 0 in lowered:
            last_components_stats.update(sweeps=done + batch, converged_at=done + lowered.index(0) + 1)
            return labels
        done += batch
    raise RuntimeError("lattice_components: the labels of the %d x %d x %d lattice had not converged after %d sweeps "
                       "(max_sweeps)" % (nx, ny, nz, done))


def component_sizes(labels):
    """(roots [K] int64 ascending: the labels in use, counts [K] int32: their points), counted on the device from labels"""
    nx, ny, nz = labels.shape
    sizes = torch.zeros(labels.numel(), device=labels.device, dtype=torch.int32)
    check(lib.jt_component_sizes(ptr(labels), nx, ny, nz, ptr(sizes), _stream()), "jt_component_sizes")
    roots = torch.nonzero(sizes).view(-1)
    return roots, sizes[roots]


def keep_components(vol, level, keep_largest=None, min_points=None, fill=0.0, max_sweeps=None):
    """vol with the components (lattice_components) that fail a test set to `fill`: (vol', kept, dropped).  keep_largest = k: the
    k components of most points stay, ties go to the smaller label; min_points = m: components of fewer than m points go; with
    both a component must pass both.  fill must not exceed level (a dropped point must be outside).  None, None: vol itself,
    nothing launched, (vol, None, None)."""
    if keep_largest is None and min_points is None:
        return vol, None, None
    if keep_largest is not None and (int(keep_largest) != keep_largest or keep_largest < 1):
        raise ValueError("keep_components: keep_largest is a positive integer (got %r)" % (keep_largest,))
    if min_points is not None and (int(min_points) != min_points or min_points < 0):
        raise ValueError("keep_components: min_points is a non-negative integer (got %r)" % (min_points,))
    if not float(fill) <= float(level):
        raise ValueError("keep_components: fill = %r exceeds level = %r: a dropped point would stay inside" % (fill, level))
    labels = lattice_components(vol, level, max_sweeps=max_sweeps)
    roots, counts = component_sizes(labels)
    keep = torch.ones(roots.numel(), device=vol.device, dtype=torch.bool)
    if keep_largest is not None:
        # roots ascend: a stable descending sort by size leaves equal sizes in the order of their labels
        order = torch.sort(counts, descending=True, stable=True).indices
        keep.zero_()
        keep[order[:int(keep_largest)]] = True
    if min_points is not None:
        keep &= counts >= int(min_points)
    kept = int(keep.sum())
    table = torch.zeros(labels.numel() + 1, device=vol.device, dtype=torch.bool)      # (the last entry: label -1, outside)
    table[roots[~keep]] = True
    drop = table[labels.view(-1).long()].view(vol.shape)
    return torch.where(drop, torch.full_like(vol, float(fill)), vol), kept, int(roots.numel()) - kept


# what jt_raster_draw's status bytes say (include/jt_render.h: JT_RASTER_*), in the order of rasterize's status_counts columns
RASTER_STATUS = ("drawn", "near", "guard", "empty", "culled")
RASTER_MAX_ATTRS = 8


def raster_project(vertices, proj, near=1e-3):
    """jt_raster_project: screen [V, nv, 4] = (x, y, 1/w, w) of vertices [nv, 3] under proj [V, 3, 4]; one launch"""
    V, nv = proj.shape[0], vertices.shape[0]
    screen = torch.empty(V, nv, 4, device=vertices.device, dtype=torch.float32)
    check(lib.jt_raster_project(ptr(vertices), nv, ptr(proj), V, float(near), ptr(screen), _stream()), "jt_raster_project")
    return screen


def raster_draw(screen, triangles, H, W, cull=False):
    """jt_raster_draw into a fresh z-buffer: (zbuf [V, H, W] int64 holding the uint64 keys, all-ones bits where nothing was drawn;
    status [V, nt] uint8); a fill and one launch"""
    V, nv, nt = screen.shape[0], screen.shape[1], triangles.shape[0]
    zbuf = torch.full((V, H, W), -1, device=screen.device, dtype=torch.int64)
    status = torch.empty(V, nt, device=screen.device, dtype=torch.uint8)
    check(lib.jt_raster_draw(ptr(screen), nv, ptr(triangles), nt, V, H, W, int(bool(cull)), ptr(zbuf), ptr(status), _stream()),
          "jt_raster_draw")
    return zbuf, status


def raster_resolve(zbuf, screen, triangles, attrs=None, background=0.0):
    """jt_raster_resolve: (tri [V, H, W] int32, depth [V, H, W] fp32, out [V, H, W, C] fp32 or None without attrs); one launch"""
    V, H, W = zbuf.shape
    nv, nt = screen.shape[1], triangles.shape[0]
    dev = zbuf.device
    tri = torch.empty(V, H, W, device=dev, dtype=torch.int32)
    depth = torch.empty(V, H, W, device=dev, dtype=torch.float32)
    C = 0 if attrs is None else attrs.shape[1]
    out = torch.empty(V, H, W, C, device=dev, dtype=torch.float32) if C else None
    bg = None
    if C:
        bg = [float(background)] * C if not hasattr(background, "__len__") else [float(v) for v in background]
        if len(bg) != C:
            raise ValueError("rasterize: %d background values for %d attributes" % (len(bg), C))
        bg = (ctypes.c_float * C)(*bg)
    check(lib.jt_raster_resolve(ptr(zbuf), ptr(screen), nv, ptr(triangles), nt, V, H, W, ptr(attrs), C, bg, ptr(tri), ptr(depth),
                                ptr(out), _stream()), "jt_raster_resolve")
    return tri, depth, out


def _view_args(who, proj, H, W, views_per_call, device):
    """the cameras and image size rasterize and triangle_visibility take, checked: (proj [V, 3, 4] fp32 on `device`, H, W, step)"""
    H, W, step = int(H), int(W), int(views_per_call)
    if proj.dim() != 3 or tuple(proj.shape[1:]) != (3, 4) or proj.shape[0] < 1:
        raise ValueError("%s: proj is [V, 3, 4] with V >= 1 (got %s)" % (who, tuple(proj.shape)))
    if H < 1 or W < 1 or step < 1:
        raise ValueError("%s: H, W and views_per_call are at least 1 (got %d, %d, %d)" % (who, H, W, step))
    return proj.detach().to(device).contiguous().float(), H, W, step


def _draw_slabs(vertices, triangles, proj, H, W, near, cull, step, counts):
    """Per slab of `step` views: jt_raster_project and jt_raster_draw into a fresh z-buffer, (screen, zbuf) yielded for the
    caller's resolve or tally, then the slab's status histogram [V_slab, 5] int64 appended to `counts`.  The caller drops the two
    before it asks for the next slab: here they go as their successors arrive."""
    codes = torch.arange(len(RASTER_STATUS), device=vertices.device, dtype=torch.uint8)
    for v0 in range(0, proj.shape[0], step):
        screen = raster_project(vertices, proj[v0:v0 + step], near)
        zbuf, status = raster_draw(screen, triangles, H, W, cull)
        yield screen, zbuf
        counts.append(torch.stack([(status == c).sum(1) for c in codes], 1))


def texture_layout(n_triangles, block):
    """mesh_io.texture_layout: the atlas of n_triangles charts in blocks of `block` texels (pure host arithmetic, no GPU)"""
    from . import mesh_io
    return mesh_io.texture_layout(n_triangles, block)


def _texture_range(layout, start, count, who):
    start, count = int(start), int(count)
    if start < 0 or count < 1 or start + count > layout.n_entries:
        raise ValueError("%s: entries [%d, %d) are not within the atlas' %d" % (who, start, start + count, layout.n_entries))
    return start, count


def texture_texels(vertices, triangles, normals, layout, start=0, count=None):
    """jt_texture_texels, one launch: for the entries [start, start + count) of `layout` (texture_layout's; count None: to the
    end) the points xyz [count, 3] fp32 on the triangles (vertices [nv, 3] fp32, triangles [nt, 3] int32), the directions dirs
    [count, 3] fp32 they are looked at along (minus the interpolated normals [nv, 3], normalised; (0, 0, -1) where that is zero
    or not finite) and valid [count] uint8 (0: the empty half of the last block, or a triangle with a vertex id out of range).
    Any range: slabs compose to the bits of one call."""
    vertices, triangles = _mesh_arg("texture_texels", vertices, triangles)
    if tuple(normals.shape) != tuple(vertices.shape):
        raise ValueError("texture_texels: one normal per vertex, [nv, 3] (got %s for %d vertices)" % (tuple(normals.shape), vertices.shape[0]))
    if triangles.shape[0] != layout.n_triangles or vertices.shape[0] < 1:
        raise ValueError("texture_texels: the layout is of %d triangles, the mesh has %d (and %d vertices)"
                         % (layout.n_triangles, triangles.shape[0], vertices.shape[0]))
    start, count = _texture_range(layout, start, layout.n_entries - int(start) if count is None else count, "texture_texels")
    dev = vertices.device
    normals = normals.detach().contiguous().float()
    xyz = torch.empty(count, 3, device=dev, dtype=torch.float32)
    dirs = torch.empty(count, 3, device=dev, dtype=torch.float32)
    valid = torch.empty(count, device=dev, dtype=torch.uint8)
    check(lib.jt_texture_texels(ptr(vertices), ptr(normals), vertices.shape[0], ptr(triangles), triangles.shape[0], layout.block,
                                layout.cols, start, count, ptr(xyz), ptr(dirs), ptr(valid), _stream()), "jt_texture_texels")
    return xyz, dirs, valid


def texture_pack(rgb, valid, layout, atlas, start=0):
    """jt_texture_pack, one launch: colours rgb [count, 3] fp32 and valid [count] uint8 of the entries [start, start + count)
    into atlas [height, width, 3] uint8 (zeroed by the caller) as floor(255 c + 0.5) clamped to 0 .. 255, 0 for a NaN; an
    invalid entry writes nothing.  Returns atlas."""
    if rgb.dim() != 2 or rgb.shape[1] != 3 or tuple(valid.shape) != (rgb.shape[0],) or valid.dtype != torch.uint8:
        raise ValueError("texture_pack: rgb is [count, 3] and valid uint8 [count] (got %s, %s %s)"
                         % (tuple(rgb.shape), valid.dtype, tuple(valid.shape)))
    if atlas.dtype != torch.uint8 or tuple(atlas.shape) != (layout.height, layout.width, 3) or not atlas.is_contiguous():
        raise ValueError("texture_pack: the atlas is contiguous uint8 [%d, %d, 3] (got %s %s)"
                         % (layout.height, layout.width, atlas.dtype, tuple(atlas.shape)))
    start, count = _texture_range(layout, start, rgb.shape[0], "texture_pack")
    rgb, valid = rgb.detach().contiguous().float(), valid.contiguous()
    check(lib.jt_texture_pack(ptr(rgb), ptr(valid), layout.block, layout.cols, start, count, ptr(atlas), layout.height, layout.width,
                              _stream()), "jt_texture_pack")
    return atlas


def _texture_arg(texture, n_triangles, who):
    """(atlas, layout) of a mesh of n_triangles: a contiguous uint8 [height, width, 3] tensor and its texture_layout"""
    atlas, layout = texture
    if layout.n_triangles != n_triangles:
        raise ValueError("%s: the texture's layout is of %d triangles, the mesh has %d" % (who, layout.n_triangles, n_triangles))
    if atlas.dtype != torch.uint8 or tuple(atlas.shape) != (layout.height, layout.width, 3):
        raise ValueError("%s: the atlas is uint8 [%d, %d, 3] (got %s %s)" % (who, layout.height, layout.width, atlas.dtype, tuple(atlas.shape)))
    return atlas.detach().contiguous(), layout


def raster_resolve_texture(zbuf, screen, triangles, atlas, layout, background=0.0):
    """jt_raster_resolve_texture: (tri [V, H, W] int32, depth [V, H, W] fp32 -- the bits of raster_resolve -- and out [V, H, W, 3]
    fp32: the atlas sampled bilinearly inside the winner's chart, `background` (a number or three) elsewhere); one launch"""
    V, H, W = zbuf.shape
    nv, nt = screen.shape[1], triangles.shape[0]
    dev = zbuf.device
    atlas, layout = _texture_arg((atlas, layout), nt, "raster_resolve_texture")
    tri = torch.empty(V, H, W, device=dev, dtype=torch.int32)
    depth = torch.empty(V, H, W, device=dev, dtype=torch.float32)
    out = torch.empty(V, H, W, 3, device=dev, dtype=torch.float32)
    bg = [float(background)] * 3 if not hasattr(background, "__len__") else [float(v) for v in background]
    if len(bg) != 3:
        raise ValueError("rasterize: %d background values for the 3 channels of a texture" % len(bg))
    check(lib.jt_raster_resolve_texture(ptr(zbuf), ptr(screen), nv, ptr(triangles), nt, V, H, W, ptr(atlas), layout.block, layout.cols,
                                        layout.height, layout.width, (ctypes.c_float * 3)(*bg), ptr(tri), ptr(depth), ptr(out),
                                        _stream()), "jt_raster_resolve_texture")
    return tri, depth, out


def rasterize(vertices, triangles, proj, H, W, attrs=None, near=1e-3, cull=False, background=0.0, views_per_call=8, texture=None):
    """A triangle mesh (vertices [nv, 3] fp32, triangles [nt, 3] int32) seen through proj [V, 3, 4] -- one matrix per view that
    takes a homogeneous mesh-space point to (x w, y w, w) in pixel units, pixel centres at half-integers (mesh_io.
    projection_matrices builds it from cameras) -- at H x W (csrc/jt_raster.hip).  Returns Opt(tri [V, H, W] int32: the nearest
    triangle, -1 where none; depth [V, H, W] fp32: its w, +inf where none; attrs [V, H, W, C]: `attrs` [nv, C <= 8] interpolated
    perspective-correctly, `background` (a number or C numbers) where nothing was drawn, None without attrs; status_counts [V, 5]
    int64: triangles drawn / dropped behind `near` or non-finite / beyond the guard band / of zero area / culled as back faces).

    Per slab of `views_per_call` views: a z-buffer of 8 bytes per pixel is allocated and cleared, then jt_raster_project,
    jt_raster_draw, jt_raster_resolve.  Everything stays on the device and nothing is read back; coverage is decided in
    integers and depth by one 64-bit atomic minimum per pixel, so two calls return the same bits however the views are batched.

    texture = (atlas, layout) -- a uint8 [height, width, 3] atlas and its texture_layout, TensorVMSplit.bake_texture's -- in
    place of attrs (the two exclude each other): the resolve is jt_raster_resolve_texture and the result's attrs [V, H, W, 3]
    the atlas sampled bilinearly inside the winner's chart.  Without it nothing changes."""
    from .options import Opt
    vertices, triangles = _mesh_arg("rasterize", vertices, triangles)
    if vertices.shape[0] < 1 or triangles.shape[0] < 1:
        raise ValueError("rasterize: an empty mesh (%d vertices, %d triangles)" % (vertices.shape[0], triangles.shape[0]))
    proj, H, W, step = _view_args("rasterize", proj, H, W, views_per_call, vertices.device)
    if attrs is not None:
        attrs = attrs.detach().contiguous().float()
        if attrs.dim() != 2 or attrs.shape[0] != vertices.shape[0] or not 1 <= attrs.shape[1] <= RASTER_MAX_ATTRS:
            raise ValueError("rasterize: attrs are [nv, C] with 1 <= C <= %d (got %s for %d vertices)"
                             % (RASTER_MAX_ATTRS, tuple(attrs.shape), vertices.shape[0]))
    if texture is not None:
        if attrs is not None:
            raise ValueError("rasterize: attrs and texture exclude each other")
        texture = _texture_arg(texture, triangles.shape[0], "rasterize")
    tri, depth, out, counts = [], [], [], []
    for screen, zbuf in _draw_slabs(vertices, triangles, proj, H, W, near, cull, step, counts):
        if texture is not None:
            t, d, o = raster_resolve_texture(zbuf, screen, triangles, texture[0], texture[1], background)
        else:
            t, d, o = raster_resolve(zbuf, screen, triangles, attrs, background)
        tri.append(t)
        depth.append(d)
        out.append(o)
        del screen, zbuf        # (or this slab's screen would outlive the next slab's projection, a slab more at the peak)
    return Opt(tri=torch.cat(tri), depth=torch.cat(depth), attrs=torch.cat(out) if attrs is not None or texture is not None else None,
               status_counts=torch.cat(counts))


def visible_tally(zbuf, n_triangles):
    """jt_visible_tally: pix [V, nt] int32 (holding the uint32 counts) -- how many pixels of every view of zbuf [V, H, W]
    (raster_draw's) every triangle wins; a fill and one launch"""
    V, H, W = zbuf.shape
    pix = torch.zeros(V, n_triangles, device=zbuf.device, dtype=torch.int32)
    check(lib.jt_visible_tally(ptr(zbuf), V, H, W, n_triangles, ptr(pix), _stream()), "jt_visible_tally")
    return pix


def visible_fold(pix, min_pixels, views, pixels):
    """jt_visible_fold, one launch: views [nt] int32 += the views of pix [V, nt] with at least min_pixels pixels, pixels [nt]
    int64 += their sum"""
    check(lib.jt_visible_fold(ptr(pix), pix.shape[0], pix.shape[1], int(min_pixels), ptr(views), ptr(pixels), _stream()),
          "jt_visible_fold")


def triangle_visibility(vertices, triangles, proj, H, W, min_pixels=1, cull=False, near=1e-3, views_per_call=8):
    """Which triangles of a mesh (vertices [nv, 3] fp32, triangles [nt, 3] int32) the cameras proj [V, 3, 4] see at H x W
    (csrc/jt_visible.hip; proj, near and cull as rasterize takes them).  Returns Opt(views [nt] int32: in how many views the
    triangle is the nearest one at `min_pixels` pixel centres or more; pixels [nt] int64: at how many pixel centres over all
    views; status_counts [V, 5] int64: rasterize's).

    Per slab of `views_per_call` views: a z-buffer is allocated and cleared, then jt_raster_project, jt_raster_draw,
    jt_visible_tally (the winners counted per view and triangle, integer atomics) and jt_visible_fold (into views and pixels, no
    atomics).  No resolve: the winner is the low word of the z-buffer's key.  Everything stays on the device and nothing is read
    back; every step is integer work on the bits jt_raster_draw leaves, so two calls return the same bits however the views are
    batched.  A triangle is seen only where it wins a pixel CENTRE: one smaller than a pixel may win none."""
    from .options import Opt
    vertices, triangles = _mesh_arg("triangle_visibility", vertices, triangles)
    nt, dev = triangles.shape[0], vertices.device
    if vertices.shape[0] < 1 or nt < 1:
        raise ValueError("triangle_visibility: an empty mesh (%d vertices, %d triangles)" % (vertices.shape[0], nt))
    proj, H, W, step = _view_args("triangle_visibility", proj, H, W, views_per_call, dev)
    if isinstance(min_pixels, bool) or int(min_pixels) != min_pixels or int(min_pixels) < 1:
        raise ValueError("triangle_visibility: min_pixels is an integer >= 1 (got %r)" % (min_pixels,))
    views = torch.zeros(nt, device=dev, dtype=torch.int32)
    pixels = torch.zeros(nt, device=dev, dtype=torch.int64)
    counts = []
    for screen, zbuf in _draw_slabs(vertices, triangles, proj, H, W, near, cull, step, counts):
        visible_fold(visible_tally(zbuf, nt), min_pixels, views, pixels)
        del screen, zbuf        # (as in rasterize)
    return Opt(views=views, pixels=pixels, status_counts=torch.cat(counts))


def _triangle_mask(mask, nt, who, name):
    if mask.dtype not in (torch.uint8, torch.bool) or tuple(mask.shape) != (nt,):
        raise ValueError("%s: %s is uint8 (or bool) [nt] (got %s %s for %d triangles)" % (who, name, mask.dtype, tuple(mask.shape), nt))
    return mask.detach().to(torch.uint8).contiguous()


def grow_triangles(triangles, n_vertices, visible, rings):
    """`visible` [nt] uint8 (or bool; non-zero: in the set) grown by `rings` rings of vertex neighbours over triangles [nt, 3]
    int32 of a mesh of n_vertices vertices: uint8 [nt], per ring visible | (a vertex shared with a triangle of the set).  Two
    launches per ring -- jt_visible_mark flags the vertices of the set, jt_visible_spread takes every triangle that touches a
    flag; the step between them is a grid-wide dependency -- plain stores, no atomics, the same bits on every call.  A triangle
    with an id outside [0, n_vertices) flags nothing and is never taken.  rings = 0 returns its input's bits."""
    if triangles.dim() != 2 or triangles.shape[1] != 3 or triangles.dtype != torch.int32:
        raise ValueError("grow_triangles: triangles are int32 [nt, 3] (got %s %s)" % (triangles.dtype, tuple(triangles.shape)))
    nt, nv = triangles.shape[0], int(n_vertices)
    visible = _triangle_mask(visible, nt, "grow_triangles", "visible")
    if isinstance(rings, bool) or int(rings) != rings or int(rings) < 0:
        raise ValueError("grow_triangles: rings is an integer >= 0 (got %r)" % (rings,))
    if nv < 0:
        raise ValueError("grow_triangles: n_vertices is not negative (got %d)" % nv)
    cur = visible.clone()
    if nt == 0 or nv == 0:
        return cur
    triangles = triangles.detach().contiguous()
    for _ in range(int(rings)):
        flag = torch.zeros(nv, device=triangles.device, dtype=torch.uint8)
        out = torch.empty_like(cur)
        check(lib.jt_visible_mark(ptr(triangles), nt, nv, ptr(cur), ptr(flag), _stream()), "jt_visible_mark")
        check(lib.jt_visible_spread(ptr(triangles), nt, nv, ptr(cur), ptr(flag), ptr(out), _stream()), "jt_visible_spread")
        cur = out
    return cur


def select_triangles(vertices, triangles, keep, normals=None, colors=None):
    """The mesh of the triangles with keep[t] != 0 (keep [nt] uint8 or bool) and ids in range, without the vertices no kept
    triangle names: (vertices' [nv', 3], triangles' [nt', 3] int32 with remapped ids, normals' or None, colors' or None,
    n_dropped).  The per-triangle counterpart of compact_mesh: jt_mesh_select_count, two cumsums, ONE host read (the two
    sizes), jt_mesh_filter_emit: triangles and vertices keep their order, two calls return the same bits.  Empty results are
    [0, 3] tensors; an all-ones keep on a mesh without unused vertices returns the input's bits."""
    vertices, triangles = _mesh_arg("select_triangles", vertices, triangles)
    nv, nt, dev = vertices.shape[0], triangles.shape[0], vertices.device
    keep = _triangle_mask(keep, nt, "select_triangles", "keep")
    normals, colors = _vertex_attr("select_triangles", "normals", normals, nv), _vertex_attr("select_triangles", "colors", colors, nv)
    if nv == 0 or nt == 0:
        return _empty_mesh(vertices, triangles, normals, colors) + (nt,)
    kept = torch.empty(nt, device=dev, dtype=torch.uint8)
    used = torch.zeros(nv, device=dev, dtype=torch.uint8)
    check(lib.jt_mesh_select_count(ptr(triangles), nt, nv, ptr(keep), ptr(kept), ptr(used), _stream()), "jt_mesh_select_count")
    out = _compact(vertices, normals, colors, triangles, kept, used)
    if out[1] is None:
        return _empty_mesh(vertices, triangles, normals, colors) + (nt,)
    return out[:4] + (nt - out[1].shape[0],)


def visible_options(visible):
    """extract_mesh's `visible` argument checked and completed, before any work: Opt(proj [V, 3, 4], H, W, min_views, min_pixels,
    grow, cull, ndc: None or (sx, sy, near))"""
    from .options import Opt
    if not isinstance(visible, dict) or any(k not in visible for k in ("proj", "H", "W")):
        raise ValueError("visible: a dict of proj [V, 3, 4], H and W, and optionally min_views, min_pixels, grow, cull, ndc (got %r)"
                         % (type(visible).__name__,))
    unknown = sorted(set(visible) - {"proj", "H", "W", "min_views", "min_pixels", "grow", "cull", "ndc"})
    if unknown:
        raise ValueError("visible: unknown keys %s" % unknown)
    proj = visible["proj"]
    if not torch.is_tensor(proj) or proj.dim() != 3 or tuple(proj.shape[1:]) != (3, 4) or proj.shape[0] < 1:
        raise ValueError("visible: proj is a [V, 3, 4] tensor with V >= 1")
    out = Opt(proj=None, H=0, W=0, min_views=1, min_pixels=1, grow=1, cull=False, ndc=None)
    for key, least in (("H", 1), ("W", 1), ("min_views", 1), ("min_pixels", 1), ("grow", 0)):
        v = visible.get(key, out[key])
        if isinstance(v, bool) or not isinstance(v, (int, float)) or int(v) != v or int(v) < least:
            raise ValueError("visible: %s is an integer >= %d (got %r)" % (key, least, v))
        out[key] = int(v)
    out.cull = bool(visible.get("cull", False))
    ndc = visible.get("ndc", None)
    if ndc is not None:
        ndc = tuple(float(v) for v in ndc)
        if len(ndc) != 3 or not all(v > 0 and math.isfinite(v) for v in ndc):
            raise ValueError("visible: ndc is None or (sx, sy, near), three positive finite numbers (got %r)" % (visible["ndc"],))
    out.ndc = ndc
    dict.__setitem__(out, "proj", proj)
    return out


def visible_triangles(vertices, triangles, visible):
    """The triangles of the mesh that stay under `visible` (visible_options'): (kept [nt] uint8, seen [nt] uint8).
    seen = triangle_visibility(...).views >= min_views, kept = grow_triangles(seen, grow).  With ndc = (sx, sy, near) the vertices
    are carried through ndc_to_world (no max_depth) FOR DRAWING ONLY -- a vertex at or beyond infinity is handed to the
    rasteriser as NaN, so its triangles are not drawn, never seen, and taken out of `kept` again after the growth; the rings
    are grown on the mesh's own connectivity, which the map does not change.  Nothing is read back."""
    draw = vertices
    drawable = None
    if visible.ndc is not None:
        world, _, status = ndc_to_world(vertices, *visible.ndc)
        bad = status != 0
        draw = torch.where(bad[:, None], torch.full_like(world, float("nan")), world)
        ids = triangles.long().clamp(0, vertices.shape[0] - 1)
        drawable = ~bad[ids].any(-1)
    vis = triangle_visibility(draw, triangles, visible.proj, visible.H, visible.W, min_pixels=visible.min_pixels, cull=visible.cull)
    seen = (vis.views >= visible.min_views).to(torch.uint8)
    kept = grow_triangles(triangles, vertices.shape[0], seen, visible.grow)
    if drawable is not None:
        kept = kept * drawable.to(torch.uint8)
    return kept, seen


# ---- depth-map fusion (include/jt_render.h: "Depth-map fusion"; csrc/jt_fusion.hip) --------------------------------------
def _fusion_state_arg(state, who):
    """(sum fp32 [nx, ny, nz], count int32 [nx, ny, nz]) as fusion_state makes them, checked"""
    if not isinstance(state, (tuple, list)) or len(state) != 2:
        raise ValueError("%s: the state is fusion_state's (sum, count)" % who)
    acc, count = state
    _lattice_arg(acc, who)
    if count.dtype != torch.int32 or count.shape != acc.shape or not count.is_contiguous() or count.device != acc.device:
        raise ValueError("%s: count is contiguous int32 of the sum's shape, on its device (got %s %s)" % (who, count.dtype, tuple(count.shape)))
    if min(acc.shape) < 2:
        raise ValueError("%s: at least two lattice points per axis (got %s)" % (who, tuple(acc.shape)))
    return acc, count


def fusion_state(shape, device):
    """the zeroed running state of a fusion over a lattice of `shape` = (nx, ny, nz) points: (sum fp32, count int32)"""
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3 or min(shape) < 2:
        raise ValueError("fusion_state: shape is three point counts of at least 2 (got %r)" % (shape,))
    return (torch.zeros(shape, device=device, dtype=torch.float32), torch.zeros(shape, device=device, dtype=torch.int32))


def fusion_integrate(state, depth, opacity, proj, lo, hi, trunc, min_opacity=0.5, carve=True, near=1e-3):
    """jt_fusion_integrate, one launch: the views depth, opacity [V, H, W] fp32 (camera-axis depth and accumulated opacity, as the
    field renders them) seen through proj [V, 3, 4] (rasterize's) added, in ascending order, into `state` (fusion_state's, updated
    in place and returned) over the lattice's box lo .. hi (three floats each).  Per lattice point and view: the point is
    projected to its nearest pixel; where that ray found a surface (finite depth > 0, opacity >= min_opacity) the truncated
    signed distance (depth - w) / trunc, at most 1, is added unless it is below -1 (occluded); where it found none the point is
    counted as seen empty (distance 1) when `carve`.  trunc is in world units.  No atomics and one accumulator chain per point
    in view order: consecutive slabs of views give the bits of one call with all of them."""
    acc, count = _fusion_state_arg(state, "fusion_integrate")
    lo, hi = _box_arg("fusion_integrate", lo, hi)
    if depth.dim() != 3 or depth.shape != opacity.shape:
        raise ValueError("fusion_integrate: depth and opacity are [V, H, W] (got %s, %s)" % (tuple(depth.shape), tuple(opacity.shape)))
    V, H, W = depth.shape
    if proj.dim() != 3 or tuple(proj.shape) != (V, 3, 4):
        raise ValueError("fusion_integrate: proj is [V, 3, 4], one matrix per depth map (got %s for %d views)" % (tuple(proj.shape), V))
    if V and (H < 1 or W < 1):
        raise ValueError("fusion_integrate: H and W are at least 1 (got %d, %d)" % (H, W))
    trunc, min_opacity, near = float(trunc), float(min_opacity), float(near)
    if not (trunc > 0 and math.isfinite(trunc)):
        raise ValueError("fusion_integrate: trunc is a positive finite number, in world units (got %r)" % (trunc,))
    if math.isnan(min_opacity) or math.isnan(near):
        raise ValueError("fusion_integrate: min_opacity and near are numbers (got %r, %r)" % (min_opacity, near))
    if V == 0:
        return state
    dev = acc.device
    depth, opacity = depth.detach().to(dev).contiguous().float(), opacity.detach().to(dev).contiguous().float()
    proj = proj.detach().to(dev).contiguous().float()
    nx, ny, nz = acc.shape
    check(lib.jt_fusion_integrate(ptr(depth), ptr(opacity), ptr(proj), V, H, W, nx, ny, nz, (ctypes.c_float * 3)(*lo),
                                  (ctypes.c_float * 3)(*hi), trunc, min_opacity, int(bool(carve)), near, ptr(acc), ptr(count), _stream()),
          "jt_fusion_integrate")
    return state


def fusion_lattice(state, min_views=1):
    """jt_fusion_finish, one launch: (lattice [nx, ny, nz] fp32, seen [nx, ny, nz] uint8) of a fusion state -- where at least
    min_views views observed the point, 0.5 (1 - mean truncated distance) and 1, else 0 and 0.  Occupancy-like: 1 deep inside, 0
    outside or unknown, the surface at level 0.5."""
    acc, count = _fusion_state_arg(state, "fusion_lattice")
    if isinstance(min_views, bool) or int(min_views) != min_views or int(min_views) < 1:
        raise ValueError("fusion_lattice: min_views is an integer >= 1 (got %r)" % (min_views,))
    lattice = torch.empty_like(acc)
    seen = torch.empty(acc.shape, device=acc.device, dtype=torch.uint8)
    check(lib.jt_fusion_finish(ptr(acc), ptr(count), acc.numel(), int(min_views), ptr(lattice), ptr(seen), _stream()), "jt_fusion_finish")
    return lattice, seen


def fused_cells(seen):
    """uint8 [nx, ny, nz]: 1 at the minimum corner of every lattice cell whose eight corners are all seen (slices of `seen`, no
    index tensor), 0 elsewhere and where no cell begins"""
    s = seen != 0
    cells = torch.zeros(seen.shape, device=seen.device, dtype=torch.uint8)
    cells[:-1, :-1, :-1] = (s[:-1, :-1, :-1] & s[1:, :-1, :-1] & s[:-1, 1:, :-1] & s[1:, 1:, :-1]
                            & s[:-1, :-1, 1:] & s[1:, :-1, 1:] & s[:-1, 1:, 1:] & s[1:, 1:, 1:]).to(torch.uint8)
    return cells


def mesh_from_fused_lattice(vol, seen, level, lo, hi):
    """mesh_from_lattice for a fused lattice (fusion_lattice's vol and seen, both [nx, ny, nz]): the iso-surface {vol = level}
    without the triangles no depth map supports.  An unobserved point is 0, so next to a point of the truncation band it would
    grow a sheet -- the back of every band, walls at silhouettes.  A triangle stays iff all eight corners of its OWNER cell are
    seen: jt_mesh_count's tri_count[p] triangles of the cell with minimum corner p start at tri_offset[p], so fused_cells(seen)
    repeated tri_count times is the per-triangle mask, compacted by select_triangles.  No geometry test looks at a position.
    Returns (vertices [nv, 3] fp32, triangles [nt, 3] int32, (n_triangles_emitted, n_triangles_unobserved)); two calls return
    the same bits."""
    lo, hi = _box_arg("mesh_from_fused_lattice", lo, hi)
    vol = vol.detach().contiguous()
    _lattice_arg(vol, "mesh_from_fused_lattice")
    if seen.shape != vol.shape or seen.dtype not in (torch.uint8, torch.bool):
        raise ValueError("mesh_from_fused_lattice: seen is uint8 (or bool) of the lattice's shape (got %s %s for %s)"
                         % (seen.dtype, tuple(seen.shape), tuple(vol.shape)))
    flags, tris = mesh_count(vol, level)
    vert_offset, tri_offset, totals = mesh_offsets(flags, tris)
    nv, nt = (int(v) for v in totals.tolist())
    vertices, triangles = mesh_emit(vol, level, lo, hi, flags, vert_offset, tri_offset, nv, nt)
    if nt == 0:
        return vertices, triangles, (0, 0)
    keep = torch.repeat_interleave(fused_cells(seen).view(-1), tris.long(), output_size=nt)
    vertices, triangles, _, _, n_dropped = select_triangles(vertices, triangles, keep)
    return vertices, triangles, (nt - n_dropped, n_dropped)


def fusion_options(fusion):
    """extract_mesh's `fusion` argument checked and completed, before any work: Opt(slabs: an iterable of (depth [V, H, W], opacity
    [V, H, W], proj [V, 3, 4]), H, W, trunc (lattice spacings), min_opacity, min_views, carve)"""
    from .options import Opt
    known = {"depth", "opacity", "proj", "slabs", "H", "W", "trunc", "min_opacity", "min_views", "carve"}
    if not isinstance(fusion, dict) or any(k not in fusion for k in ("H", "W")):
        raise ValueError("fusion: a dict of depth [V, H, W], opacity [V, H, W] and proj [V, 3, 4] (or slabs: an iterable of such "
                         "triples), H and W, and optionally trunc, min_opacity, min_views, carve (got %r)" % (type(fusion).__name__,))
    unknown = sorted(set(fusion) - known)
    if unknown:
        raise ValueError("fusion: unknown keys %s" % unknown)
    whole = [k for k in ("depth", "opacity", "proj") if fusion.get(k, None) is not None]
    if (fusion.get("slabs", None) is None) == (len(whole) == 0) or len(whole) not in (0, 3):
        raise ValueError("fusion: either depth, opacity and proj, or slabs (an iterable of (depth, opacity, proj))")
    out = Opt(slabs=None, H=0, W=0, trunc=4.0, min_opacity=0.5, min_views=1, carve=True)
    for key in ("H", "W", "min_views"):
        v = fusion.get(key, out[key])
        if isinstance(v, bool) or not isinstance(v, (int, float)) or int(v) != v or int(v) < 1:
            raise ValueError("fusion: %s is an integer >= 1 (got %r)" % (key, v))
        out[key] = int(v)
    t = fusion.get("trunc", out.trunc)
    if isinstance(t, bool) or not isinstance(t, (int, float)) or not (t > 0 and math.isfinite(t)):
        raise ValueError("fusion: trunc is a positive finite number of lattice spacings (got %r)" % (t,))
    a = fusion.get("min_opacity", out.min_opacity)
    if isinstance(a, bool) or not isinstance(a, (int, float)) or not 0 < a <= 1:
        raise ValueError("fusion: min_opacity lies in (0, 1] (got %r)" % (a,))
    out.trunc, out.min_opacity, out.carve = float(t), float(a), bool(fusion.get("carve", True))
    slabs = fusion.get("slabs", None)
    if slabs is None:
        depth, opacity, proj = (fusion[k] for k in ("depth", "opacity", "proj"))
        if not all(torch.is_tensor(x) for x in (depth, opacity, proj)):
            raise ValueError("fusion: depth, opacity and proj are tensors")
        if depth.dim() != 3 or tuple(depth.shape[1:]) != (out.H, out.W) or depth.shape != opacity.shape or tuple(proj.shape) != (depth.shape[0], 3, 4):
            raise ValueError("fusion: depth and opacity are [V, H, W] = [V, %d, %d] and proj [V, 3, 4] (got %s, %s, %s)"
                             % (out.H, out.W, tuple(depth.shape), tuple(opacity.shape), tuple(proj.shape)))
        slabs = [(depth, opacity, proj)]
    dict.__setitem__(out, "slabs", slabs)
    return out
