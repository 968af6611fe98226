"""Per-vertex normals and colours of the exported surface on the GPU, and the export end to end.

Gradient: k_density_gradient (jt_march.hip, ops.density_gradient) against fp64 autograd of the oracle's density_feature with the
sample geometry pinned to the product path's fp32 cells (tests/pinned_ref.py), within TOL_GRAD of the tensor's maximum; the
feature within TOL_VAL (tests/test_gpu_fullsize.py: the project's own bounds; test_density_feature_value's docstring says what
that bound asks of the kernel's tap fractions).  Colour: point_colors (the forward's record-free
k_shade_fwd<C, 0, B16> on rays of one sample) against the oracle's app_feature (pinned taps) -> mlp_fea / mlp_weakview in fp64 within
TOL_VAL; a point whose reference has a hidden pre-activation within TOL_RELU of zero is held to TOL_TIE, and such points are at
most 1 % of the points."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import tensorf_oracle as O
from tests import mesh_ref as R
from tests import pinned_ref as P
from tests.test_gpu_fullsize import TOL_GRAD, TOL_RELU, TOL_TIE, TOL_VAL
from tests.test_gpu_wgrad_edges import GRID

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("blender", "llff")
MAX_TIE_SHARE = 0.01
# The scene seed of the colour tests, chosen by the REFERENCE alone (fp64 on the CPU, before any kernel ran) so that its own share
# of points within TOL_RELU of a ReLU tie stays under MAX_TIE_SHARE for every n: seeds 0..7 give 20, 11, 25, 10, 12, 16, 20, 18
# such points of 2 045 for the blender kind, and seeds 0, 4 and 5 one of 33; seed 3: none of 1, 31 and 33, 10 of 2 045 (0.49 %),
# none for the llff kind.
COLOUR_SEED = 3


def _scene(kind, seed=0):
    aabb = P.thin_box(GRID)
    return P.build_scene(kind, GRID, aabb, DEV, seed=seed), aabb


def _points(aabb, n, seed):
    """n world points: off the texel nodes, on the far node of each axis, and up to 1.5 texels outside the box"""
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.tensor(aabb[:3]), torch.tensor(aabb[3:])
    p = P._off_node(lo, hi, hi - lo, n, g)
    which = torch.arange(n) % 8                        # 0..2: far node of that axis; 3, 4: outside; the rest stay off-node
    for a in range(3):
        p[which == a, a] = hi[a]
    out = (which == 3) | (which == 4)
    side = torch.where(torch.rand(n, 3, generator=g) < 0.5, -1.0, 1.0)
    push = 1.5 * P.UNIT * torch.rand(n, 3, generator=g) * (torch.rand(n, 3, generator=g) < 0.6)
    beyond = torch.where(side > 0, hi + push, lo - push)
    p = torch.where(out[:, None] & (push > 0), beyond, p)
    return p.float()


def _oracle(tf, kind):
    cfg = P.scene_cfg(tf.aabb.view(-1).tolist(), tf.gridSize.tolist(), [float(tf.near_far[0]), float(tf.near_far[1])], kind, 0.5,
                      1e-7, "cpu", torch.float64)
    params = P.params_of(tf)
    for _, v in O.flat_params(params):
        v.data = v.data.cpu()
        v.requires_grad_(False)
    return cfg, params


class _pinned:
    """the oracle's samplers replaced by the pinned ones of tests/pinned_ref.py (as pinned_ref.reference does)"""

    def __enter__(self):
        self.saved = (O._sample_plane, O._sample_line)
        O._sample_plane, O._sample_line = P._pinned_plane, P._pinned_line

    def __exit__(self, *exc):
        O._sample_plane, O._sample_line = self.saved


def _reference_gradient(tf, kind, xyz):
    cfg, params = _oracle(tf, kind)
    x = xyz.detach().cpu().double().requires_grad_(True)
    with _pinned():
        feat = O.density_feature(cfg, params, P._pinned_normalize(cfg, x))
        grad, = torch.autograd.grad(feat.sum(), x)
    return feat.detach(), grad


_GRADIENT_RUNS = {}    # (kind, n) -> (feat, grad, reference feat, reference grad): one launch and one reference for both tests


def _gradient_run(kind, n):
    from joint_tensorf_amd import ops
    if (kind, n) not in _GRADIENT_RUNS:
        tf, aabb = _scene(kind)
        xyz = _points(aabb, n, seed=n).to(DEV)
        feat, grad = ops.density_gradient(tf._density_cfg(), list(tf.density_plane), list(tf.density_line), xyz)
        none, g2 = ops.density_gradient(tf._density_cfg(), list(tf.density_plane), list(tf.density_line), xyz, want_feat=False)
        assert none is None and torch.equal(g2, grad)                         # feat is optional
        _GRADIENT_RUNS[(kind, n)] = (feat.cpu(), grad.cpu()) + _reference_gradient(tf, kind, xyz)
    return _GRADIENT_RUNS[(kind, n)]


N_GRADIENT = [1, 255, 256, 257, 4099]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", N_GRADIENT)
def test_density_gradient(kind, n):
    feat, grad, _, want = _gradient_run(kind, n)
    assert feat.shape == (n,) and grad.shape == (n, 3) and grad.dtype == torch.float32
    err = float((grad.double() - want).abs().max() / want.abs().max())
    print("\n[gradient] %s n = %d: grad %.2e of max %.3g (bound %.0e)" % (kind, n, err, float(want.abs().max()), TOL_GRAD))
    assert float(want.abs().max()) > 0 and err <= TOL_GRAD


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", N_GRADIENT)
def test_density_feature_value(kind, n):
    """The feature k_density_gradient returns, within TOL_VAL of the pinned reference.

    This value is sensitive to HOW the tap fraction is formed: the blender scene's feature (8.9) changes by its own size per
    texel, and at a texel coordinate ix up to 71 half an ulp of ix is 3.8e-6 texel.  With axis_taps' default fraction (the
    compiler contracts the product ix = X * (size - 1) into f = ix - floor(ix): the fraction of the unrounded product) the
    blender kind came out 2.15e-5, 2.12e-5, 2.37e-5 and 2.83e-5 from the reference at n = 255, 256, 257 and 4 099, above the bound,
    and the reference evaluated with that fraction moves by exactly as much.  The kernel therefore asks for axis_taps<true>: the
    fraction of the rounded product, the one pinned_ref._axis32 pins.  Emulated in fp32 on the CPU that arithmetic stays within
    1.5e-6 of the reference."""
    feat, _, want, _ = _gradient_run(kind, n)
    err = float((feat.double() - want).abs().max())
    print("\n[gradient] %s n = %d: feat %.2e of max %.3g (bound %.0e)" % (kind, n, err, float(want.abs().max()), TOL_VAL))
    assert err <= TOL_VAL


@pytest.mark.parametrize("i", [0, 1, 2])
def test_ramp_scenes(i):
    """density plane i channel 0 = 1, line i channel 0 a linear ramp, everything else 0: the gradient lies along axis vecMode[i]
    alone with the ramp's slope, and the normal is the negative unit axis"""
    from joint_tensorf_amd import ops
    from joint_tensorf_amd.tensorf_repr import VEC_MODE
    tf, aabb = _scene("blender")
    axis, per_texel = VEC_MODE[i], 0.25
    with torch.no_grad():
        for p in list(tf.density_plane) + list(tf.density_line):
            p.zero_()
        tf.density_plane[i][0, 0] = 1.0
        L = tf.density_line[i].shape[2]
        tf.density_line[i][0, 0, :, 0] = per_texel * torch.arange(L, device=DEV, dtype=torch.float32)
    g = torch.Generator().manual_seed(i)
    lo, hi = torch.tensor(aabb[:3]), torch.tensor(aabb[3:])
    xyz = P._off_node(lo, hi, hi - lo, 300, g).float().to(DEV)
    feat, grad = ops.density_gradient(tf._density_cfg(), list(tf.density_plane), list(tf.density_line), xyz)
    slope = per_texel / P.UNIT
    want = torch.zeros(300, 3, dtype=torch.float64)
    want[:, axis] = slope
    err = float((grad.cpu().double() - want).abs().max() / slope)
    want_f = per_texel * (xyz[:, axis].cpu().double() - aabb[axis]) / P.UNIT
    print("\n[ramp] plane %d, axis %d: gradient error %.2e of the slope, feature error %.2e" % (i, axis, err, float((feat.cpu().double() - want_f).abs().max())))
    assert err <= TOL_GRAD and float((feat.cpu().double() - want_f).abs().max()) <= TOL_VAL * max(1.0, float(want_f.max()))
    nrm, bad = tf.point_normals(xyz)
    unit = torch.zeros(3)
    unit[axis] = -1.0
    assert bad == 0 and float((nrm.cpu() - unit).abs().max()) <= 1e-4


@pytest.mark.parametrize("kind", KINDS)
def test_point_normals(kind):
    from joint_tensorf_amd import ops
    tf, aabb = _scene(kind)
    lo, hi = torch.tensor(aabb[:3]), torch.tensor(aabb[3:])
    g = torch.Generator().manual_seed(11)
    inside = P._off_node(lo, hi, hi - lo, 700, g).float()
    # outside on one, two and three axes, on either side
    out = inside[:7].clone()
    signs = torch.tensor([[1, 0, 0], [0, -1, 0], [0, 0, 1], [1, -1, 0], [0, 1, 1], [-1, 0, -1], [-1, 1, -1]], dtype=torch.float32)
    out = torch.where(signs > 0, hi + 0.7 * P.UNIT, torch.where(signs < 0, lo - 1.2 * P.UNIT, out))
    xyz = torch.cat([inside, out]).to(DEV)
    nrm, bad = tf.point_normals(xyz, slab_points=256)                      # three slabs, the last one short
    grad = ops.density_gradient(tf._density_cfg(), list(tf.density_plane), list(tf.density_line), xyz[:700])[1]
    want = -grad / torch.linalg.vector_norm(grad, dim=-1, keepdim=True)
    assert bad == 0 and float((nrm[:700] - want).abs().max()) <= 2.0 ** -22
    assert float((torch.linalg.vector_norm(nrm, dim=-1) - 1).abs().max()) <= 2.0 ** -22
    want_out = signs / torch.linalg.vector_norm(signs, dim=-1, keepdim=True)
    assert float((nrm[700:].cpu() - want_out).abs().max()) <= 2.0 ** -23, nrm[700:]
    assert torch.equal(nrm[700:703].cpu(), signs[:3])                       # one axis: the unit vector itself
    # an all-zero field: zeros, and every point counted
    with torch.no_grad():
        for p in list(tf.density_plane) + list(tf.density_line):
            p.zero_()
    nrm, bad = tf.point_normals(xyz)
    assert bad == 700 and bool((nrm[:700] == 0).all()) and float((nrm[700:].cpu() - want_out).abs().max()) <= 2.0 ** -23


def _reference_colors(tf, kind, xyz, viewdirs):
    """(rgb [n, 3] fp64, smallest |hidden pre-activation| per point)"""
    cfg, params = _oracle(tf, kind)
    x, v = xyz.detach().cpu().double(), viewdirs.detach().cpu().double()
    pre, linear = [], O._linear

    def recording(inp, w, b):
        out = linear(inp, w, b)
        pre.append(out)
        return out
    O._linear = recording
    try:
        with _pinned():
            feat = O.app_feature(cfg, params, P._pinned_normalize(cfg, x))
        mlp = O.mlp_fea if kind == "blender" else O.mlp_weakview
        rgb = mlp(cfg, params["mlp"], feat, v)
    finally:
        O._linear = linear
    assert len(pre) == 3
    return rgb, torch.minimum(pre[0].abs().min(-1).values, pre[1].abs().min(-1).values)


def _view_dirs(n, seed):
    v = torch.randn(n, 3, generator=torch.Generator().manual_seed(seed))
    return (v / v.norm(dim=-1, keepdim=True)).float()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 31, 33, 2045])
def test_point_colors(kind, n):
    tf, aabb = _scene(kind, seed=COLOUR_SEED)
    lo, hi = torch.tensor(aabb[:3]), torch.tensor(aabb[3:])
    xyz = P._off_node(lo, hi, hi - lo, n, torch.Generator().manual_seed(100 + n)).float().to(DEV)
    view = _view_dirs(n, 200 + n).to(DEV)
    want, margin = _reference_colors(tf, kind, xyz, view)
    tie = margin <= TOL_RELU
    print("\n[colour] %s n = %d: %d of the reference's points within %.0e of a ReLU tie (%.2f %%)"
          % (kind, n, int(tie.sum()), TOL_RELU, 100.0 * float(tie.float().mean())))
    got = tf.point_colors(xyz, view)
    assert got.shape == (n, 3) and got.dtype == torch.float32 and bool(((got > 0) & (got < 1)).all())
    err = (got.cpu().double() - want).abs().max(-1).values
    e_plain = float(err[~tie].max()) if bool((~tie).any()) else 0.0
    e_tie = float(err[tie].max()) if bool(tie.any()) else 0.0
    print("[colour] %s n = %d: error %.2e (bound %.0e), at ties %.2e (bound %.0e)" % (kind, n, e_plain, TOL_VAL, e_tie, TOL_TIE))
    assert int(tie.sum()) <= MAX_TIE_SHARE * n
    assert e_plain <= TOL_VAL and e_tie <= TOL_TIE


@pytest.mark.parametrize("kind", KINDS)
def test_point_colors_one_record_free_launch_and_the_clamp(kind):
    from torch.profiler import ProfilerActivity, profile as tprofile
    from tests.test_gpu_shade_fwd_edges import CFG, forward_kernels
    tf, aabb = _scene(kind)
    n = 333
    xyz = _points(aabb, n, seed=5).to(DEV)
    view = _view_dirs(n, 6).to(DEV)
    tf.point_colors(xyz[:8], view[:8])                                     # (module load and allocator warm-up stay out of the profile)
    torch.cuda.synchronize()
    with tprofile(activities=[ProfilerActivity.CUDA]) as prof:
        got = tf.point_colors(xyz, view)
        torch.cuda.synchronize()
    seen = forward_kernels(P._device_kernel_names(prof))
    print("\n[colour] %s: %s" % (kind, sorted(seen)))
    assert len(seen) == 1 and list(seen)[0].startswith("k_shade_fwd<%s, 0, " % CFG[kind]), sorted(seen)
    lo, hi = torch.tensor(aabb[:3], device=DEV), torch.tensor(aabb[3:], device=DEV)
    clamped = torch.minimum(torch.maximum(xyz, lo), hi)
    assert bool((clamped != xyz).any(-1).sum() > 20)
    assert torch.equal(got, tf.point_colors(clamped, view))                # a point outside: the colour of its clamped position
    assert torch.equal(got, tf.point_colors(xyz, view, slab_points=100))   # slabs, the last one short
    with pytest.raises(ValueError):
        tf.point_colors(xyz, view[:-1])
    assert tuple(tf.point_colors(xyz[:0], view[:0]).shape) == (0, 3)


def test_extract_mesh_attributes():
    """extract_mesh's new arguments on the blob scene of tests/test_gpu_mesh.py, with the appearance branch of the Blender
    configuration (the kind the shade kernels are built for): the defaults are today's mesh, to the bit"""
    from joint_tensorf_amd import synthetic, tensorf_repr
    torch.manual_seed(0)
    tf = tensorf_repr.TensorVMSplit([-1.0, -1.3, -0.8, 1.2, 1.1, 1.0], [20, 21, 19], DEV, density_n_comp=[8, 8, 8],
                                    appearance_n_comp=[48, 48, 48], app_dim=27, near_far=[2.0, 6.0], shadingMode="MLP_Fea",
                                    view_pe=2, fea_pe=2, featureC=64)
    with torch.no_grad():
        synthetic.bake_blobs(tf, n_blobs=5, seed=2)
    res = (17, 19, 23)
    plain = tf.extract_mesh(res=res)
    assert plain.normals is None and plain.colors is None and plain.n_components is None and plain.n_degenerate_normals is None
    assert plain._fields[:6] == ("vertices", "triangles", "lo", "hi", "shape", "level")
    full = tf.extract_mesh(res=res, min_points=1, normals=True, colors=True)    # a filter that drops nothing
    assert torch.equal(full.vertices, plain.vertices) and torch.equal(full.triangles, plain.triangles)
    assert full.n_components[0] >= 1 and full.n_components[1] == 0
    nrm, bad = tf.point_normals(full.vertices)
    assert torch.equal(full.normals, nrm) and full.n_degenerate_normals == bad
    length = torch.linalg.vector_norm(nrm, dim=-1)
    assert bool((((length - 1).abs() <= 2.0 ** -22) | (length == 0)).all())
    view = torch.where((nrm == 0).all(-1, keepdim=True), nrm.new_tensor([0.0, 0.0, -1.0]), -nrm)
    assert torch.equal(full.colors, tf.point_colors(full.vertices, view))
    only = tf.extract_mesh(res=res, colors=True)                                # colours imply the normals' computation, not their return
    assert only.normals is None and only.n_degenerate_normals is None and torch.equal(only.colors, full.colors)
    # the normals agree with the triangles' orientation: on average they point along the area-weighted face normals
    V, T = full.vertices.double(), full.triangles.long()
    face = torch.linalg.cross(V[T[:, 1]] - V[T[:, 0]], V[T[:, 2]] - V[T[:, 0]])
    vert = torch.zeros_like(V).index_add_(0, T.reshape(-1), face.repeat_interleave(3, 0))
    inside_box = ((full.vertices >= tf.aabb[0].to(DEV)) & (full.vertices <= tf.aabb[1].to(DEV))).all(-1) & (length > 0)
    agree = ((vert * nrm.double()).sum(-1) > 0)[inside_box].double().mean()
    print("\n[mesh] %d vertices, %d degenerate normals, %.1f %% of the normals on the side of their faces" % (len(V), bad, 100 * float(agree)))
    assert float(agree) > 0.9


def test_export_end_to_end_with_surface_options(tmp_path):
    """`python -m joint_tensorf_amd.export` in process with --surface.*: floaters dropped, normals and colours in the PLY; and
    without those options the file of today"""
    from joint_tensorf_amd import export, mesh_io, synthetic
    from tests.test_gpu_metrics import _trained_small_model
    from tests.test_lifecycle import _small_opt
    opt = _small_opt(device=DEV, output_path=str(tmp_path), max_iter=5, camera=dict(noise=0.15),
                     freq=dict(scalar=2, val=100, ckpt=100), optim=dict(test_iter=3))
    m = _trained_small_model(opt)
    tf = m.graph.nerf.tensorf
    with torch.no_grad():
        k = synthetic.bake_blobs(tf, n_blobs=5, seed=2)
        # one more blob, small and far from the rest: a floater in the corner of the box
        plane, line = tf.density_plane[0], tf.density_line[0]
        lo, hi = tf.aabb[0].to(DEV).float(), tf.aabb[1].to(DEV).float()
        c, s = lo + (hi - lo) * torch.tensor([0.07, 0.07, 0.93], device=DEV), 0.045 * float((hi - lo).mean())
        X = lo[0] + (hi[0] - lo[0]) * torch.linspace(0, 1, plane.shape[3], device=DEV)
        Y = lo[1] + (hi[1] - lo[1]) * torch.linspace(0, 1, plane.shape[2], device=DEV)
        Z = lo[2] + (hi[2] - lo[2]) * torch.linspace(0, 1, line.shape[2], device=DEV)
        plane[0, k] = 60.0 * torch.exp(-((X[None, :] - c[0]) ** 2 + (Y[:, None] - c[1]) ** 2) / (2 * s * s))
        line[0, k, :, 0] = torch.exp(-((Z - c[2]) ** 2) / (2 * s * s))
    ckpt = m.save_checkpoint(opt, ep=0, it=5, latest=True)
    res = [15, 14, 13]
    args = ["--yaml=bat_blender_VM", "--load=%s" % ckpt, "--device=%s" % DEV, "--mesh.res=%s" % json.dumps(res),
            "--data.image_size=[32,32]", "--train_schedule.n_voxel_init=1000", "--train_schedule.n_voxel_final=4096",
            "--train_schedule.upsample_iters=[2,50]", "--camera.noise=0.15"]
    out_dir = os.path.join(str(tmp_path), "export")
    out = export.main(args + ["--output_path=%s" % out_dir, "--surface.keep_largest=1", "--surface.normals=true",
                              "--surface.colors=true"])
    tf.kernel_density = tf.kernel_color = None          # a restored checkpoint has no blur state
    want = tf.extract_mesh(res=res, level=0.005, cap=True, keep_largest=1)
    whole = tf.extract_mesh(res=res, level=0.005, cap=True)
    got = mesh_io.read_ply_attributes(out.mesh)
    V, T = got["vertices"], got["triangles"]
    assert len(V) > 50 and np.array_equal(V, want.vertices.cpu().numpy()) and np.array_equal(T, want.triangles.cpu().numpy())
    assert len(V) < whole.vertices.shape[0]                                     # the floater's vertices are gone
    t = R.topology(V, T)
    assert t["closed"] and t["oriented"] and t["volume"] > 0
    kept, dropped = out.n_components
    print("\n[export] %d vertices (%d with the floaters), components kept %d dropped %d, degenerate normals %d"
          % (len(V), whole.vertices.shape[0], kept, dropped, out.n_degenerate_normals))
    assert kept == 1 and dropped >= 1 and want.n_components == (kept, dropped)
    assert "components kept 1 dropped %d" % dropped in got["comments"]
    assert "normals degenerate %d" % out.n_degenerate_normals in got["comments"] and "lattice 17 16 15" in got["comments"]
    length = np.linalg.norm(got["normals"].astype(np.float64), axis=1)
    assert ((np.abs(length - 1) <= 2.0 ** -22) | (length == 0)).all()
    assert int((length == 0).sum()) == out.n_degenerate_normals
    nrm, _ = tf.point_normals(want.vertices)
    assert np.array_equal(got["normals"], nrm.cpu().numpy())
    view = torch.where((nrm == 0).all(-1, keepdim=True), nrm.new_tensor([0.0, 0.0, -1.0]), -nrm)
    col = tf.point_colors(want.vertices, view).cpu().numpy().astype(np.float64)
    assert np.array_equal(got["colors"], np.floor(255.0 * col + 0.5).astype(np.uint8))
    # without the --surface.* options: write_ply of extract_mesh with defaults, byte for byte
    plain_dir = os.path.join(str(tmp_path), "plain")
    plain = export.main(args + ["--output_path=%s" % plain_dir])
    assert plain.n_components is None and plain.n_degenerate_normals is None and sorted(os.listdir(plain_dir)) == ["mesh.ply"]
    ref_path = mesh_io.write_ply(os.path.join(str(tmp_path), "ref.ply"), whole.vertices, whole.triangles,
                                 mesh_io.mesh_comments(whole.level, whole.shape, whole.lo, whole.hi, "world"))
    assert open(plain.mesh, "rb").read() == open(ref_path, "rb").read()
    # colours alone: no normals in the file, no `normals degenerate` line
    col_dir = os.path.join(str(tmp_path), "colours")
    only = mesh_io.read_ply_attributes(export.main(args + ["--output_path=%s" % col_dir, "--surface.colors=true"]).mesh)
    assert only["normals"] is None and only["colors"] is not None and not any(c.startswith("normals") for c in only["comments"])
