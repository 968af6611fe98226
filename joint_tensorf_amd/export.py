"""`python -m joint_tensorf_amd.export --yaml=NAME --load=CKPT --output_path=OUT [--mesh.res=N | --mesh.res=[nx,ny,nz]]
[--mesh.level=0.005] [--mesh.cap=true] [--data.root=DIR --data.scene=lego ...]`: the trained field of a checkpoint as a triangle
mesh, OUT/mesh.ply (binary little-endian PLY), extracted on the device (Model.export_scene -> extract_mesh ->
csrc/jt_mesh.hip), and -- when the run's image set is given -- OUT/cameras.json: the refined cameras in the frame the mesh lives
in, their intrinsics, and the similarity transform to the dataset's frame.  What the upstream TensoRF calls --export_mesh; the
reference dropped the code and kept the option block.

The joint pose / field optimisation recovers the scene in the frame of the OPTIMISED poses, which differs from the dataset's by
a similarity transform: geometry is only usable together with the cameras of that same frame.  For `camera.ndc: true` (LLFF)
the field lives in the scene box's NDC coordinates and so does the mesh; the PLY comment and the JSON say `space ndc`.

`--surface.keep_largest=K` / `--surface.min_points=M` remove floaters before a triangle is emitted: the connected components of
the opacity lattice (csrc/jt_components.hip, the mesh's own connectivity) of which only the K largest, of at least M lattice
points, stay.  `--surface.normals=true` writes per-vertex normals (the normalised negative density gradient),
`--surface.colors=true` per-vertex colours (the appearance branch at the vertex, seen against its normal).  Without a
`--surface.*` option mesh.ply holds positions and triangles only.

`--preview.views=N|all` looks at the result: the mesh drawn from N training cameras of cameras.json (evenly spaced over the set)
by the device rasteriser (csrc/jt_raster.hip), OUT/preview/mesh_<idx>.png, at `--preview.size=[H,W]` (default
data.image_size), shaded by `--preview.shade=color|normal|depth|texture`; `--preview.cull=true` drops back faces.
`--preview.check=true` also renders the field at the same cameras (OUT/preview/field_<idx>.png) and writes OUT/report.json:
per view the coverage of mesh and field, their IoU, the median depth difference, the PSNR of the colours and what became of
every triangle.  It reports; it judges nothing.  The preview needs the run's image set and a world-space scene (not
`camera.ndc` whose mesh stays in NDC).  Without a `--preview.*` option the export writes what it always wrote, byte for byte.

`--frame.space=world` carries the mesh of a `camera.ndc` scene out of NDC on the device (mesh_ops.ndc_to_world, mesh_ops.compact_mesh;
csrc/jt_mesh.hip): mesh.ply then holds LLFF geometry in the frame of the refined cameras of cameras.json (`space world`, with
`unwarp near N sx SX sy SY` and `dropped beyond B far F` comments), and `--preview.*` draws it like any world-space mesh.
Triangles with a vertex at or behind infinity (zn >= 1: the far cap) are dropped and counted; `--frame.max_depth=D` also drops
what lies more than D world units along the reference axis away -- forward-facing backgrounds run out to thousands of near-plane
distances and ruin a viewer's framing.  The step needs the run's image set (sx = fx / cx, sy = fy / cy of its intrinsics).
`--frame.space=ndc` names what an NDC export does by default; without a `--frame.*` option nothing changes.

`--simplify.cell=K` (a number >= 1) simplifies the mesh on the device by vertex clustering (mesh_ops.simplify_mesh;
csrc/jt_simplify.hip): the vertices that fall into one cell of K lattice spacings -- ceil((points - 1) / K) cells per axis over
the box of the lattice -- become ONE vertex, placed where the planes (vertex, field normal) of its members meet in the
least-squares sense and never outside their bounding box; triangles are re-indexed and the collapsed ones dropped.  It runs in
the frame the field lives in, before `--frame.space=world` carries an NDC mesh out (cells are then perspective-sized);
`--surface.normals` writes the clusters' normals and `--surface.colors` evaluates the colours at the simplified vertices.
mesh.ply gains the comment `simplify cell K cells CX CY CZ from NV NT collapsed C`, report.json the same numbers, and
`--preview.*` / `--preview.check` draw and score the simplified mesh.  Without a `--simplify.*` option mesh.ply is what it was,
byte for byte.

`--texture.block=S` (an integer from 4 to 64) exports a TEXTURED mesh: a per-triangle texture atlas baked on the device from
the field (TensorVMSplit.bake_texture; csrc/jt_texture.hip) -- square blocks of S x S texels, two right-isosceles charts of legs
S - 3 texels per block, every texel the appearance branch at its point of the flat triangle seen against the interpolated
normal -- so colour resolution no longer depends on the vertex count, which `--simplify.cell` cuts.  It is baked last, on the
mesh as it is written (after `--surface.keep_largest` / `min_points` and `--simplify.cell`), in the frame the field lives in.
OUT gains atlas.png (RGB), mesh.obj + mesh.mtl (`map_Kd atlas.png`; what Blender reads), and mesh.ply carries per-face texture
coordinates (`property list uchar float texcoord`, `comment TextureFile atlas.png`: what MeshLab, CloudCompare, Open3D and
trimesh read) and the comment `texture block S atlas W H`; report.json repeats the numbers.  `--preview.shade=texture` draws
the mesh with its atlas (jt_raster_resolve_texture); with `--preview.check=true` report.json's psnr_color scores the textured
draw and psnr_vertex_color the same cameras drawn with vertex colours.  Together with `--frame.space=world` on a camera.ndc
scene it is refused: a chart that is linear in NDC is not linear in world space (perspective-correct charts are not built).
Without a `--texture.*` option the export writes what it wrote, byte for byte.

`--visible.views=N|all` writes only the surface the training cameras see (mesh_ops.visible_triangles; csrc/jt_visible.hip).  The
level set of a trained field is not one skin: behind the visible surface the field is unsupervised, and hollow interiors,
enclosed pockets and shells are extracted like everything else -- connected to the outer surface or larger than it, so
`--surface.keep_largest` keeps them.  The mesh is drawn from N training cameras (evenly spaced over the set, as
`--preview.views` picks them) at `--visible.size=[H,W]` (default data.image_size) by the device rasteriser; a triangle stays
when it is the nearest one at `--visible.min_pixels` (1) pixel centres or more in `--visible.min_views` (1) views or more, or
lies within `--visible.grow` (1) rings of vertex neighbours of such a triangle; `--visible.cull=true` drops back faces while
deciding.  The stage runs after `--simplify.cell` and before colours and `--texture.block`, which are then evaluated only for
what is written; on a camera.ndc scene the vertices are carried to world space for drawing only and the mask is applied in NDC,
so it combines with `--texture.block` there and with `--frame.space=world`.  It needs the run's image set.  mesh.ply gains the
comment `visible views V size H W min_views A min_pixels B grow G cull C from NV NT seen S grown G2 dropped D`, report.json the
same numbers.  A triangle is seen only if it wins a pixel CENTRE: on an unsimplified fine mesh a triangle is a pixel or two
across and may win none -- `--visible.grow` and a larger `--visible.size` are the remedies; after `--simplify.cell=4` a
triangle is tens of pixels across.  Without a `--visible.*` option the export writes what it wrote, byte for byte.

`--fusion.views=N|all` exports a second surface: not the level set of the opacity, which sits wherever the density ramp crosses
a small threshold and carries whatever the unsupervised interior holds, but the surface of the depth maps the field RENDERS from
its refined training cameras -- what the photometric loss shaped, and what the pose refinement made mutually consistent.  N
training views (evenly spaced over the set, as `--visible.views` picks them) are rendered at `--fusion.size=[H,W]` (default
data.image_size), their expected camera-axis depth (sum w z / sum w, the render's background term and offset undone) and opacity
are fused, `--fusion.views_per_call` (8) views per launch, into a truncated signed distance volume on the `--mesh.res` lattice
(mesh_ops.fusion_integrate; csrc/jt_fusion.hip): a lattice point is projected to its nearest pixel of every view; a ray of opacity
below `--fusion.min_opacity` (0.5) found no surface and, with `--fusion.carve` (true), carves the point empty; the distance is
truncated at `--fusion.trunc` (4) lattice spacings; a point that fewer than `--fusion.min_views` (1) views observed is unknown
and no triangle of a cell with such a corner is written.  The surface is the fused lattice's level 0.5 (`--mesh.level` cannot be
given with it); `--surface.*`, `--simplify.cell`, `--visible.*`, `--texture.block` and `--preview.*` then work on it as on the
level set, with normals, colours and the atlas still the field's, evaluated at the fused surface.  mesh.ply gains the comment
`fusion views V size H W trunc T min_opacity A min_views M carve C seen P unobserved D`, report.json the same numbers.  It needs the
run's image set and a world-space scene: `camera.ndc` scenes are refused (fusing forward-facing scenes, in NDC or in world
space, is not built).  Without a `--fusion.*` option the export writes what it wrote, byte for byte.

Every other `--key.sub=value` is one of the dotted overrides of joint_tensorf_amd.train."""
import sys

import torch

MESH_DEFAULTS = dict(res=None, level=0.005, cap=True)
# what is done to the surface beyond extracting it: floaters removed by connected component (keep the K largest, drop those of
# fewer than M lattice points), per-vertex normals (the density gradient) and colours (the appearance branch seen head-on)
SURFACE_DEFAULTS = dict(keep_largest=None, min_points=None, normals=False, colors=False)
# pictures of the mesh from the training cameras (views: how many, 0 = none, or "all"; size: [H, W], None = data.image_size;
# shade: what a pixel shows), back faces culled or not, and the check against the volume render of the same cameras
PREVIEW_DEFAULTS = dict(views=0, size=None, shade="color", check=False, cull=False)
PREVIEW_SHADES = ("color", "normal", "depth", "texture")
PREVIEW_MAX_SIZE = 16384        # what the rasteriser draws (include/jt_render.h)
# the coordinates mesh.ply is written in (space: "world" or "ndc"; None = what the scene lives in: ndc for camera.ndc, world
# otherwise) and, for an NDC scene exported to world, the depth along the reference axis beyond which geometry is dropped
FRAME_DEFAULTS = dict(space=None, max_depth=None)
FRAME_SPACES = ("world", "ndc")
# the simplification of the extracted mesh by vertex clustering (cell: the edge of a cell in lattice spacings, None = off)
SIMPLIFY_DEFAULTS = dict(cell=None)
# the texture atlas baked for the mesh (block: the edge of a block of two charts in texels, an integer from 4 to 64; None = off)
TEXTURE_DEFAULTS = dict(block=None)
# the surface the training cameras see (views: how many decide, 0 = off, or "all"; size: [H, W] they are drawn at, None =
# data.image_size; a triangle is seen when it wins min_pixels pixel centres in min_views views; grow: rings of vertex neighbours
# kept round the seen ones; cull: back faces are not drawn while deciding)
VISIBLE_DEFAULTS = dict(views=0, size=None, min_views=1, min_pixels=1, grow=1, cull=False)
# the surface fused from the depth maps the field renders (views: how many training views are rendered and fused, 0 = off, or
# "all"; size: [H, W] they are rendered at, None = data.image_size; trunc: the truncation distance in lattice spacings;
# min_opacity: below it a ray found no surface; min_views: observations a lattice point needs; carve: rays without a surface
# mark the points they pass as empty; views_per_call: views per launch of the integration)
FUSION_DEFAULTS = dict(views=0, size=None, trunc=4.0, min_opacity=0.5, min_views=1, carve=True, views_per_call=8)


def _option_group(over, name, defaults):
    """pop the dotted group --NAME.* from the overrides: Opt(defaults) with the given sub-keys; an unknown one is a KeyError"""
    from .options import Opt
    given = over.pop(name, None)
    if given is not None and not isinstance(given, dict):
        raise SystemExit("--%s takes sub-keys: %s" % (name, ", ".join("--%s.%s" % (name, k) for k in defaults)))
    group = Opt(defaults)
    for k, v in (given or {}).items():
        if k not in defaults:
            raise KeyError("unknown option --%s.%s (known: %s)" % (name, k, ", ".join(sorted(defaults))))
        group[k] = v
    return group


def build_options(argv):
    from .options import apply_overrides, load_options, parse_overrides
    over = parse_overrides(argv)
    name = over.pop("yaml", None)
    if not isinstance(name, str):
        raise SystemExit("usage: python -m joint_tensorf_amd.export --yaml=NAME --load=CKPT --output_path=OUT [--mesh.res=N] "
                         "[--mesh.level=L] [--mesh.cap=true|false] [--surface.keep_largest=K] [--surface.min_points=M] "
                         "[--surface.normals=true|false] [--surface.colors=true|false] [--preview.views=N|all] [--preview.size=[H,W]] "
                         "[--preview.shade=color|normal|depth|texture] [--preview.check=true|false] [--preview.cull=true|false] "
                         "[--frame.space=world|ndc] [--frame.max_depth=D] [--simplify.cell=K] [--texture.block=S] "
                         "[--visible.views=N|all] [--visible.size=[H,W]] [--visible.min_views=A] [--visible.min_pixels=B] "
                         "[--visible.grow=G] [--visible.cull=true|false] [--fusion.views=N|all] [--fusion.size=[H,W]] "
                         "[--fusion.trunc=T] [--fusion.min_opacity=A] [--fusion.min_views=M] [--fusion.carve=true|false] "
                         "[--fusion.views_per_call=K] "
                         "[--data.root=DIR --key.sub=value ...]")
    level_given = isinstance(over.get("mesh", None), dict) and "level" in over["mesh"]
    mesh = _option_group(over, "mesh", MESH_DEFAULTS)
    surface = _option_group(over, "surface", SURFACE_DEFAULTS)
    preview = _option_group(over, "preview", PREVIEW_DEFAULTS)
    frame = _option_group(over, "frame", FRAME_DEFAULTS)
    simplify = _option_group(over, "simplify", SIMPLIFY_DEFAULTS)
    texture = _option_group(over, "texture", TEXTURE_DEFAULTS)
    visible = _option_group(over, "visible", VISIBLE_DEFAULTS)
    fusion = _option_group(over, "fusion", FUSION_DEFAULTS)
    opt = apply_overrides(load_options(name), over)
    opt.mesh, opt.surface, opt.preview, opt.frame, opt.simplify = mesh, surface, preview, frame, simplify
    opt.texture = texture
    if visible != VISIBLE_DEFAULTS:
        # (absent: no opt.visible at all, and nothing new is called)
        _check_visible(visible)
        opt.visible = visible
    if fusion != FUSION_DEFAULTS:
        # (absent: no opt.fusion at all, and nothing new is called)
        _check_fusion(fusion, bool(opt.camera.ndc), level_given)
        opt.fusion = fusion
    _check_preview(preview)
    _check_simplify(simplify)
    _check_frame(frame, bool(opt.camera.ndc))
    _check_texture(texture, preview, frame, bool(opt.camera.ndc))
    for k in ("keep_largest", "min_points"):
        v = surface[k]
        if v is not None:
            if isinstance(v, bool) or not isinstance(v, (int, float)) or float(v) != int(v) or int(v) < 1:
                raise SystemExit("--surface.%s is a positive integer (got %r)" % (k, v))
            surface[k] = int(v)
    for k in ("normals", "colors"):
        if not isinstance(surface[k], bool):
            raise SystemExit("--surface.%s is true or false (got %r)" % (k, surface[k]))
    res = opt.mesh.res
    if res is not None:
        res = [res] * 3 if not isinstance(res, list) else res
        if len(res) != 3 or any(float(v) != int(v) or int(v) < 2 for v in res):
            raise SystemExit("--mesh.res is one integer or three, each at least 2 (got %r)" % (opt.mesh.res,))
        opt.mesh.res = [int(v) for v in res]
    opt.mesh.level = float(opt.mesh.level)
    if not isinstance(opt.mesh.cap, bool):
        raise SystemExit("--mesh.cap is true or false (got %r)" % (opt.mesh.cap,))
    if "device" not in opt:
        opt.device = "cuda:0"
    opt.H, opt.W = (int(v) for v in opt.data.image_size)
    return opt


def _check_preview(preview):
    v = preview.views
    if v != "all":
        if isinstance(v, bool) or not isinstance(v, (int, float)) or float(v) != int(v) or int(v) < 0:
            raise SystemExit("--preview.views is a non-negative integer or all (got %r)" % (v,))
        preview.views = int(v)
    size = preview.size
    if size is not None:
        size = [size] * 2 if not isinstance(size, list) else size
        if (len(size) != 2 or any(isinstance(s, bool) or not isinstance(s, (int, float)) or float(s) != int(s)
                                  or not 1 <= int(s) <= PREVIEW_MAX_SIZE for s in size)):
            raise SystemExit("--preview.size is one integer or [H, W], each from 1 to %d (got %r)" % (PREVIEW_MAX_SIZE, preview.size))
        preview.size = [int(s) for s in size]
    if preview.shade not in PREVIEW_SHADES:
        raise SystemExit("--preview.shade is one of %s (got %r)" % (", ".join(PREVIEW_SHADES), preview.shade))
    for k in ("check", "cull"):
        if not isinstance(preview[k], bool):
            raise SystemExit("--preview.%s is true or false (got %r)" % (k, preview[k]))
    if preview.views == 0 and any(preview[k] != PREVIEW_DEFAULTS[k] for k in PREVIEW_DEFAULTS):
        raise SystemExit("--preview.size / shade / check / cull say how the preview is made: name its views with "
                         "--preview.views=N or --preview.views=all")


def _check_frame(frame, ndc):
    import math
    if frame.space is not None and frame.space not in FRAME_SPACES:
        raise SystemExit("--frame.space is one of %s (got %r)" % (", ".join(FRAME_SPACES), frame.space))
    d = frame.max_depth
    if d is not None:
        if isinstance(d, bool) or not isinstance(d, (int, float)) or not math.isfinite(d) or not d > 0:
            raise SystemExit("--frame.max_depth is a positive finite number, in world units along the reference axis (got %r)" % (d,))
        frame.max_depth = float(d)
    if frame.space == "ndc" and not ndc:
        raise SystemExit("--frame.space=ndc needs a camera.ndc scene: this one lives in world space and has no NDC coordinates")
    if d is not None and not (ndc and frame.space == "world"):
        raise SystemExit("--frame.max_depth limits a camera.ndc scene that is exported to world space: give it with "
                         "--frame.space=world on such a scene")


def _check_simplify(simplify):
    import math
    k = simplify.cell
    if k is not None:
        if isinstance(k, bool) or not isinstance(k, (int, float)) or not math.isfinite(k) or not k >= 1:
            raise SystemExit("--simplify.cell is a finite number of at least 1, the edge of a cell in lattice spacings (got %r)" % (k,))
        simplify.cell = float(k)


def _check_texture(texture, preview, frame, ndc):
    from . import mesh_io
    s = texture.block
    if s is not None:
        if (isinstance(s, bool) or not isinstance(s, (int, float)) or float(s) != int(s)
                or not mesh_io.TEXTURE_MIN_BLOCK <= int(s) <= mesh_io.TEXTURE_MAX_BLOCK):
            raise SystemExit("--texture.block is an integer from %d to %d, the edge in texels of a block of two charts (got %r)"
                             % (mesh_io.TEXTURE_MIN_BLOCK, mesh_io.TEXTURE_MAX_BLOCK, s))
        texture.block = int(s)
        if ndc and frame.space == "world":
            raise SystemExit("--texture.block together with --frame.space=world is not available: the atlas is baked in NDC, where "
                             "the field lives, and a chart that is linear in NDC is not linear in world space (perspective-correct "
                             "charts are not built); export the textured mesh in NDC, or the world-space mesh with --surface.colors")
    elif preview.shade == "texture":
        raise SystemExit("--preview.shade=texture draws the mesh with its texture atlas: name the block size with --texture.block=S")


def _check_visible(visible):
    v = visible.views
    if v != "all":
        if isinstance(v, bool) or not isinstance(v, (int, float)) or float(v) != int(v) or int(v) < 0:
            raise SystemExit("--visible.views is a non-negative integer or all (got %r)" % (v,))
        visible.views = int(v)
    size = visible.size
    if size is not None:
        size = [size] * 2 if not isinstance(size, list) else size
        if (len(size) != 2 or any(isinstance(s, bool) or not isinstance(s, (int, float)) or float(s) != int(s)
                                  or not 1 <= int(s) <= PREVIEW_MAX_SIZE for s in size)):
            raise SystemExit("--visible.size is one integer or [H, W], each from 1 to %d (got %r)" % (PREVIEW_MAX_SIZE, visible.size))
        visible.size = [int(s) for s in size]
    for k, least in (("min_views", 1), ("min_pixels", 1), ("grow", 0)):
        n = visible[k]
        if isinstance(n, bool) or not isinstance(n, (int, float)) or float(n) != int(n) or int(n) < least:
            raise SystemExit("--visible.%s is an integer of at least %d (got %r)" % (k, least, n))
        visible[k] = int(n)
    if not isinstance(visible.cull, bool):
        raise SystemExit("--visible.cull is true or false (got %r)" % (visible.cull,))
    if visible.views == 0:
        raise SystemExit("--visible.size / min_views / min_pixels / grow / cull say how visibility is decided: name the deciding "
                         "views with --visible.views=N or --visible.views=all")


def _check_fusion(fusion, ndc=False, level_given=False):
    import math
    v = fusion.views
    if v != "all":
        if isinstance(v, bool) or not isinstance(v, (int, float)) or float(v) != int(v) or int(v) < 0:
            raise SystemExit("--fusion.views is a non-negative integer or all (got %r)" % (v,))
        fusion.views = int(v)
    size = fusion.size
    if size is not None:
        size = [size] * 2 if not isinstance(size, list) else size
        if (len(size) != 2 or any(isinstance(s, bool) or not isinstance(s, (int, float)) or float(s) != int(s)
                                  or not 1 <= int(s) <= PREVIEW_MAX_SIZE for s in size)):
            raise SystemExit("--fusion.size is one integer or [H, W], each from 1 to %d (got %r)" % (PREVIEW_MAX_SIZE, fusion.size))
        fusion.size = [int(s) for s in size]
    t = fusion.trunc
    if isinstance(t, bool) or not isinstance(t, (int, float)) or not math.isfinite(t) or not t > 0:
        raise SystemExit("--fusion.trunc is a positive finite number, the truncation distance in lattice spacings (got %r)" % (t,))
    fusion.trunc = float(t)
    a = fusion.min_opacity
    if isinstance(a, bool) or not isinstance(a, (int, float)) or not 0 < a <= 1:
        raise SystemExit("--fusion.min_opacity lies in (0, 1]: the opacity from which a ray has found a surface (got %r)" % (a,))
    fusion.min_opacity = float(a)
    for k in ("min_views", "views_per_call"):
        n = fusion[k]
        if isinstance(n, bool) or not isinstance(n, (int, float)) or float(n) != int(n) or int(n) < 1:
            raise SystemExit("--fusion.%s is an integer of at least 1 (got %r)" % (k, n))
        fusion[k] = int(n)
    if not isinstance(fusion.carve, bool):
        raise SystemExit("--fusion.carve is true or false (got %r)" % (fusion.carve,))
    if fusion.views == 0:
        raise SystemExit("--fusion.size / trunc / min_opacity / min_views / carve / views_per_call say how the depth maps are fused: "
                         "name the views to render with --fusion.views=N or --fusion.views=all")
    if ndc:
        raise SystemExit("--fusion.views is not available for camera.ndc scenes: the depth maps of a forward-facing scene are "
                         "parameters along NDC rays, and fusing them, in NDC or in world space, is not built")
    if level_given:
        raise SystemExit("--mesh.level cannot be given with --fusion.views: the fused surface is the level 0.5 of the fused lattice")


def unwarps(opt):
    """whether this export carries the mesh of an NDC scene to world space (opt.frame.space == "world" on camera.ndc)"""
    return bool(opt.camera.ndc) and (opt.get("frame", None) or {}).get("space", None) == "world"


def has_dataset(opt):
    """whether the run names an image set (a root for the native loaders, a synthetic scene, or ready-made views)"""
    d = opt.data
    return bool(d.get("root", None) or d.get("synthetic", False) or d.get("train_views", None) is not None)


def main(argv=None):
    """Returns what Model.export_scene returned (paths and counts)."""
    from . import checkpoint
    from .model import bat_hip
    opt = build_options(sys.argv[1:] if argv is None else list(argv))
    if not opt.get("load", None) or not opt.get("output_path", None):
        raise SystemExit("--load=CKPT and --output_path=OUT are required: the checkpoint to read, the directory to write to")
    if unwarps(opt) and not has_dataset(opt):
        # refused before any GPU work: the NDC map is made of the training views' intrinsics
        raise SystemExit("--frame.space=world needs the run's image set (--data.root=DIR, or --data.synthetic=true): sx = fx / cx "
                         "and sy = fy / cy of the NDC map are read from its intrinsics")
    if (opt.get("visible", None) or {}).get("views", 0) and not has_dataset(opt):
        # refused before any GPU work: the training cameras decide what is seen
        raise SystemExit("--visible.views needs the run's image set (--data.root=DIR, or --data.synthetic=true): its cameras "
                         "decide which triangles are seen")
    if (opt.get("fusion", None) or {}).get("views", 0) and not has_dataset(opt):
        # refused before any GPU work: the depth maps are rendered from the training cameras
        raise SystemExit("--fusion.views needs the run's image set (--data.root=DIR, or --data.synthetic=true): the depth maps "
                         "are rendered from its cameras")
    if opt.preview.views != 0:
        # refused before any GPU work: the preview draws the mesh from the cameras of cameras.json
        if not has_dataset(opt):
            raise SystemExit("--preview.views needs the run's image set (--data.root=DIR, or --data.synthetic=true): without it no "
                             "cameras.json is written and there is no camera to look from")
        if opt.camera.ndc and not unwarps(opt):
            raise SystemExit("--preview.views is not available for camera.ndc scenes (space ndc): the mesh lives in the scene "
                             "box's NDC coordinates and the rasteriser's depth cannot order it there; --frame.space=world "
                             "carries it to world space and enables the preview")
    dev = torch.device(opt.device)
    with torch.cuda.device(dev):
        m = bat_hip.Model(opt)
        if has_dataset(opt):
            m.load_dataset(opt, eval_split="test", train_split="train")
            m.build_networks(opt)
        else:
            weight = checkpoint._load(opt.load, "cpu")["graph"].get("se3_refine.weight")
            m.build_networks(opt, n_views=1 if weight is None else int(weight.shape[0]))
        m.restore_checkpoint(opt)
        out = m.export_scene(opt, opt.output_path)
    print("joint_tensorf_amd.export: %d vertices, %d triangles in %s%s"
          % (out.n_vertices, out.n_triangles, out.mesh, "; cameras in %s" % out.cameras if out.cameras else ""), flush=True)
    if out.get("preview", None) is not None:
        print("joint_tensorf_amd.export: " + out.preview.summary, flush=True)
    return out


if __name__ == "__main__":
    main()
