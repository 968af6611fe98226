"""Pinned fp64 reference for a hand-built BAT_VMSplit scene and hand-made rays, and the element-wise gradient criterion
of tests/test_gpu_scatter_shapes.py.

The HIP side runs one forward + backward with fixed random cotangents on rgb and opacity and reads back what its kernels
decided (the shading mask from last_render_cfg.shade_lists, the ReLU sign words from the record workspace).  The
reference side runs the oracle in float64 (on the CPU), on the HIP path's ray values, with those decisions pinned
(app_mask_override / relu_masks_override) and with the scene constants held as their fp32 values (as
fullsize_util.oracle_cfg does).  The sample geometry is pinned as well: the z values, the in-box test, the sample
positions, their normalised coordinates and the tap cells and fractions are the fp32 values the product path computes
(the same separately rounded operations, jt_common.h), taken as exact numbers, and everything after them is fp64.  The
derivatives with respect to the rays are those of the fp64 expressions (straight-through), so a sample within rounding
of a texel node takes the same cell -- the same slope -- on both sides.  Without that pinning an fp32 tap weight that
rounds to 0 (a sample on a node or on a box face) meets an fp64 weight of 1e-8, and the bilinear slope on either side of
a node differs by O(1).

Per factor (plane or line) it also returns, besides the fp64 gradient T:
  * M, the magnitude: the sum over contributions of |tap weight x upstream gradient|.  The map from a factor to its
    samples (_sample_plane / _sample_line) is linear with non-negative weights, so with U the fp64 gradient that reaches
    the samples, autograd.grad(samples, factor, grad_outputs=|U|) is M, and M >= |T| element by element;
  * F, the footprint: the same call with grad_outputs = ones, > 0.
A factor gradient G of an fp32 implementation is then judged element by element (factor_errors): G == 0 exactly
outside F (anything else is a stray write), |G - T| <= kappa 2^-24 M inside."""
import copy

import torch

from oracle import tensorf_oracle as O  # checker only

EPS32 = 2.0 ** -24
GROUPS = ("density_plane", "density_line", "app_plane", "app_line")
FACTORS = ["%s.%d" % (g, i) for g in GROUPS for i in range(3)]
DENSE = ["basis_mat.weight", "mlp.w1", "mlp.b1", "mlp.w2", "mlp.b2", "mlp.w3", "mlp.b3"]
# scene kinds of the two configurations: (appearance channels, app_dim, hidden units, shading, activation, shift)
KINDS = {"blender": (48, 27, 64, "MLP_Fea", "softplus", -10.0), "llff": (20, 20, 32, "MLP_Fea_WeakView", "relu", 0.0)}
UNIT = 1.0 / 128  # texel pitch of every axis of a thin scene (exact in fp32: sample positions on the faces are exact)


def thin_box(grid):
    """aabb of a scene whose three axes have the same texel pitch UNIT (stepSize = UNIT * step_ratio, exactly), centred"""
    h = [(g - 1) * UNIT / 2 for g in grid]
    return [-h[0], -h[1], -h[2], h[0], h[1], h[2]]


def scene_cfg(aabb, grid, near_far, kind, step_ratio, thres, device, dtype=torch.float32):
    """the oracle's SceneCfg of a scene of `kind`; with dtype = float64 the fp32 VALUES of the constants"""
    _, _, _, mode, act, shift = KINDS[kind]
    cfg = O.SceneCfg(aabb, grid, near_far, step_ratio=step_ratio, density_shift=shift, distance_scale=25.0,
                     fea2denseAct=act, rayMarch_weight_thres=thres, shadingMode=mode, view_pe=2, fea_pe=2).to(device)
    for k in ("aabb", "aabbSize", "invaabbSize", "units", "stepSize"):
        setattr(cfg, k, getattr(cfg, k).to(dtype))
    return cfg


def build_scene(kind, grid, aabb, dev, cd=16, near_far=(0.5, 40.0), step_ratio=0.5, thres=1e-7, depth=1.5, seed=0):
    """A BAT_VMSplit of the given kind with positive density factors whose field has about `depth` optical depth over
    the longest axis (so that the transmittance stays away from zero along it and every texel of the long line is in
    the footprint), random appearance factors and MLP."""
    import joint_tensorf_amd as jt
    ca, app_dim, hid, mode, act, shift = KINDS[kind]
    torch.manual_seed(seed)
    tf = jt.BAT_VMSplit(aabb, grid, dev, density_n_comp=[cd] * 3, appearance_n_comp=[ca] * 3, app_dim=app_dim,
                        near_far=list(near_far), shadingMode=mode, density_shift=shift, distance_scale=25.0, view_pe=2,
                        fea_pe=2, featureC=hid, step_ratio=step_ratio, fea2denseAct=act, rayMarch_weight_thres=thres,
                        volume_init_scale=0.1, volume_init_bias=0.0)
    extent = max(aabb[3 + a] - aabb[a] for a in range(3))
    sigma = depth / (25.0 * extent)
    feat = sigma if act == "relu" else 10.0 + float(torch.log(torch.expm1(torch.tensor(sigma, dtype=torch.float64))))
    a = (feat / (3 * cd)) ** 0.5  # feat = sum over 3 planes x cd channels of plane x line, both ~ a
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in list(tf.density_plane) + list(tf.density_line):
            p.copy_((a * (0.5 + torch.rand(p.shape, generator=g))).to(p.device))
    return tf


def _off_node(lo, hi, size, n, g):
    """n positions in the box a quarter to three quarters of a texel in from a random cell corner: off the texel nodes"""
    o = lo + size * torch.rand(n, 3, generator=g)
    o = torch.floor((o - lo) / UNIT) * UNIT + lo + UNIT * (0.25 + 0.5 * torch.rand(n, 3, generator=g))
    return torch.minimum(o, hi - UNIT / 4)


def ray_set(aabb, n_axial, n_oblique, n_graze, axis=2, seed=0, dist=3.0, n_miss=0, n_far_side=0, n_far_entry=0):
    """hand-made rays [R, 3] (fp32, CPU) for a scene box:
      * a bundle along `axis` entering through the end face (origin exactly 1 before the face, direction the unit axis:
        the unjittered first sample sits exactly on the face, the samples step UNIT * step_ratio along the line);
      * oblique rays at random points of the box from random directions;
      * grazing rays through the neighbourhood of the box's long edges, across the long axis;
      * rays that miss the box (they count towards the batch's size, which the walk's shape depends on);
      * far-side rays: a bundle along +`axis` like the first, whose coordinate on one of the two other axes (alternating)
        is exactly that axis' `hi`: every in-box sample sits on that axis' far node (floor(ix) == size - 1, the sample
        is in the box because the in-box test is !(p > hi)) -- and, like every full-length ray of the first bundle, the
        one sample on the far end face sits on the long axis' far node as well;
      * far-entry rays: along -`axis` from exactly 1 beyond the `hi` end face, cross-section off the nodes: the first
        sample sits exactly on the far node of `axis`, no other sample of the ray is on a far node.
    The last two families are appended behind the others and draw from a generator of their own: the rays of a call
    without them are bit for bit those of earlier versions."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.tensor(aabb[:3]), torch.tensor(aabb[3:])
    size = hi - lo
    os_, ds_ = [], []
    if n_axial:
        # cross-section positions off the texel nodes (a quarter texel in from a random cell corner)
        o = lo + size * torch.rand(n_axial, 3, generator=g)
        o = torch.floor((o - lo) / UNIT) * UNIT + lo + UNIT * (0.25 + 0.5 * torch.rand(n_axial, 3, generator=g))
        o = torch.minimum(o, hi - UNIT / 4)
        o[:, axis] = lo[axis] - 1.0
        d = torch.zeros(n_axial, 3)
        d[:, axis] = 1.0
        os_.append(o), ds_.append(d)
    if n_oblique:
        tgt = lo + size * torch.rand(n_oblique, 3, generator=g)
        d = torch.randn(n_oblique, 3, generator=g)
        d = d / d.norm(dim=-1, keepdim=True)
        os_.append(tgt - dist * d), ds_.append(d)
    if n_graze:
        tgt = lo + size * torch.rand(n_graze, 3, generator=g)
        side = [a for a in range(3) if a != axis]
        for a in side:  # onto one of the four long edges, a small random distance in or out
            pick = torch.rand(n_graze, generator=g) < 0.5
            tgt[:, a] = torch.where(pick, lo[a], hi[a]) + 0.3 * UNIT * torch.randn(n_graze, generator=g)
        d = torch.randn(n_graze, 3, generator=g)
        d[:, axis] = 0.1 * d[:, axis]
        d = d / d.norm(dim=-1, keepdim=True)
        os_.append(tgt - dist * d), ds_.append(d)
    if n_miss:
        tgt = lo + size * torch.rand(n_miss, 3, generator=g)
        d = torch.randn(n_miss, 3, generator=g)
        d = d / d.norm(dim=-1, keepdim=True)
        os_.append(tgt + (dist + size.norm()) * d), ds_.append(d)  # outside, looking away
    gf = torch.Generator().manual_seed(seed + 7919)
    if n_far_side:
        o = _off_node(lo, hi, size, n_far_side, gf)
        side = [a for a in range(3) if a != axis]
        for k, a in enumerate(side):
            o[k::2, a] = hi[a]
        o[:, axis] = lo[axis] - 1.0
        d = torch.zeros(n_far_side, 3)
        d[:, axis] = 1.0
        os_.append(o), ds_.append(d)
    if n_far_entry:
        o = _off_node(lo, hi, size, n_far_entry, gf)
        o[:, axis] = hi[axis] + 1.0
        d = torch.zeros(n_far_entry, 3)
        d[:, axis] = -1.0
        os_.append(o), ds_.append(d)
    return torch.cat(os_).float().contiguous(), torch.cat(ds_).float().contiguous()


def cotangents(R, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(R, 3, generator=g, dtype=torch.float64), torch.randn(R, generator=g, dtype=torch.float64)


def _device_kernel_names(prof):
    names = set()
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            names.add(e.name)
    return names


def run_hip(tf, o, d, S, ndc=False, white=True, cot_seed=0, profile=False, pose_only=False):
    """One forward + backward of tf through the HIP path (eval sampling: no jitter).  Returns the outputs, the 20
    parameter gradients, the ray gradients, the decisions the kernels took and (profile=True) the names of the device
    kernels that ran.  pose_only: no parameter wants a gradient for this step (requires_grad restored afterwards), only
    the rays do -- the render takes the pose-only kernels; `grads` is None, `param_grads` the number of parameters that
    received a gradient all the same (0), and the decisions are those of this run's own (pose-only) record set."""
    if pose_only:
        params = list(tf.parameters())
        keep = [p.requires_grad for p in params]
        for p in params:
            p.requires_grad_(False)
        try:
            return _run_hip(tf, o, d, S, ndc, white, cot_seed, profile, True)
        finally:
            for p, k in zip(params, keep):
                p.requires_grad_(k)
    return _run_hip(tf, o, d, S, ndc, white, cot_seed, profile, False)


GUARD_BYTES, GUARD_FILL = 512, 0xA5


class guard_band:
    """While active, every float32 / int32 / int16 device tensor that torch.empty(n0, n1, ..., device=, dtype=) hands out
    (the form in which joint_tensorf_amd.ops creates the buffers its kernels write) is a view of an allocation with
    GUARD_BYTES more behind it, filled with GUARD_FILL; violations() lists the tensors behind which a byte changed.  A
    kernel that writes up to GUARD_BYTES past its output -- a partial last tile treated as a full one is 31 entries of
    12 bytes -- is caught, and the stray write lands in memory that belongs to the test."""

    def __init__(self):
        self.held = []

    def __enter__(self):
        self.orig = torch.empty
        held, orig = self.held, self.orig

        def empty(*size, **kw):
            dt = kw.get("dtype")
            if (size and all(type(s) is int for s in size) and set(kw) == {"device", "dtype"}
                    and dt in (torch.float32, torch.int32, torch.int16) and torch.device(kw["device"]).type == "cuda"):
                n = 1
                for s in size:
                    n *= s
                base = orig(n + GUARD_BYTES // dt.itemsize, **kw)
                base[n:].view(torch.uint8).fill_(GUARD_FILL)
                held.append((tuple(size), base, n))
                return base[:n].view(*size)
            return orig(*size, **kw)
        torch.empty = empty
        return self

    def __exit__(self, *exc):
        torch.empty = self.orig
        return False

    def violations(self):
        return [(shape, int((base[n:].view(torch.uint8) != GUARD_FILL).sum())) for shape, base, n in self.held
                if bool((base[n:].view(torch.uint8) != GUARD_FILL).any())]


class deterministic:
    """with deterministic(on): the library's deterministic mode switched on (or off), restored on the way out"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from joint_tensorf_amd._lib import lib
        self.lib, self.prev = lib, lib.jt_set_deterministic(1 if self.on else 0)

    def __exit__(self, *exc):
        self.lib.jt_set_deterministic(self.prev)
        return False


def _run_hip(tf, o, d, S, ndc, white, cot_seed, profile, pose_only):
    import contextlib
    from tests.fullsize_util import read_relu_masks
    dev = tf.density_plane[0].device
    for p in tf.parameters():
        p.grad = None
    og, dg = o.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
    R = o.shape[0]
    cr, co = cotangents(R, cot_seed)
    guard = guard_band() if pose_only else None
    overruns = []

    def step():
        with (guard if guard is not None else contextlib.nullcontext()):
            out = tf(None, og, dg, white_bg=white, is_train=False, ndc_ray=ndc, N_samples=S)
            ((out[0] * cr.to(dev).float()).sum() + (out[2] * co.to(dev).float()).sum()).backward()
            torch.cuda.synchronize()
        if guard is not None:
            overruns.extend(guard.violations())
            del guard.held[:]
        return out

    kernels, attempts = None, 0
    if profile:
        from torch.profiler import ProfilerActivity, profile as tprofile
        # (the profiler has been seen to return a trace without this library's backward kernels once in ~40 rows on
        #  MI355X: the same deterministic step is then recorded once more, from zeroed gradients; the caller reports it)
        for attempts in range(1, 3):
            for p in tf.parameters():
                p.grad = None
            og.grad = dg.grad = None
            with tprofile(activities=[ProfilerActivity.CUDA]) as prof:
                out = step()
            kernels = _device_kernel_names(prof)
            if any("k_march_bwd_scan" in n for n in kernels):   # every backward launches the scan
                break
    else:
        out = step()
    grads, param_grads = None, sum(p.grad is not None for p in tf.parameters())
    if not pose_only:
        grads = {}
        for grp in GROUPS:
            for i in range(3):
                grads["%s.%d" % (grp, i)] = getattr(tf, grp)[i].grad.detach().clone()
        grads["basis_mat.weight"] = tf.basis_mat.weight.grad.detach().clone()
        for k, t in zip(("w1", "b1", "w2", "b2", "w3", "b3"), tf.renderModule.weights()):
            grads["mlp." + k] = t.grad.detach().clone()
    offset, sidx = tf.last_render_cfg.shade_lists
    cnt = (offset[1:] - offset[:-1]).long()
    sel = torch.arange(S, device=dev)[None] < cnt[:, None]
    mask = torch.zeros(R, S, dtype=torch.bool, device=dev)
    mask[sel.nonzero()[:, 0], (sidx.to(torch.int32) & 0xFFFF).long()[sel]] = True
    n = int(offset[-1])
    assert int(mask.sum()) == n
    relu = read_relu_masks(tf, n) if n else None
    return dict(rgb=out[0].detach(), depth=out[1].detach(), opacity=out[2].detach(), grads=grads,
                g_o=og.grad.detach() if og.grad is not None else torch.zeros_like(og),
                g_d=dg.grad.detach() if dg.grad is not None else torch.zeros_like(dg),
                shade_mask=mask, relu=relu, kernels=kernels, profile_attempts=attempts, param_grads=param_grads,
                overruns=overruns)


def fused_layout(scene, n_rays):
    """jt_pose_fused_scratch_layout (include/jt_fused.h) as a dict: where a launch of n_rays rays of `scene` (a JtScene)
    leaves its per-ray decisions.  None when the single-launch kernel does not take the scene."""
    import ctypes
    from joint_tensorf_amd._lib import fused_lib
    out = (ctypes.c_int64 * 8)()
    if fused_lib().jt_pose_fused_scratch_layout(ctypes.byref(scene), int(n_rays), ctypes.cast(out, ctypes.c_void_p)) != 0:
        return None
    keys = ("head", "slot", "Sp", "tile_rows", "row_sign", "row_rgb", "blocks", "waves")
    return dict(zip(keys, (int(v) for v in out)))


def fused_slot_of(lay, n_rays):
    """the slot index of every ray of a launch [n_rays] (long): in every round wave w of workgroup b renders ray
    round * blocks * waves + w * blocks + b and owns slot b * waves + w.  Rays of a later round reuse the slots of the
    first: after the launch a slot holds the data of the LAST ray that used it."""
    q = torch.arange(n_rays) % (lay["blocks"] * lay["waves"])
    return (q % lay["blocks"]) * lay["waves"] + q // lay["blocks"]


def decode_fused_scratch(ws, lay, n_rays, S, hidden):
    """The decisions a k_pose_fused launch left in its workspace `ws` (any dtype, viewed as 32-bit words): the shading
    mask [n_rays, S] (rank >= 0; rank is the sixth of the six per-sample arrays in front of a slot's tile blocks) and the
    ReLU signs of the two hidden layers, two bool tensors [n, hidden] over the shaded entries in ray-major order,
    ascending sample (the sign words' bit layout is the record tape's, fullsize_util.read_relu_masks; k_pose_fused's
    fused_tile_fwd writes relu_signs's word of lane half h to row row_sign + 2 * layer + h, column = entry % 32).  Each
    ray is read from its own slot (fused_slot_of): for a launch of more than one round the caller must know whose data a
    slot holds."""
    words = ws.contiguous().view(torch.int32)      # read where it lies: the workspace of a long-S scene is gigabytes
    take = lambda idx: words[idx.to(words.device)].cpu()  # noqa: E731
    Sp, rows = lay["Sp"], lay["tile_rows"]
    assert S <= Sp and words.numel() >= lay["head"] + lay["blocks"] * lay["waves"] * lay["slot"]
    base = lay["head"] + fused_slot_of(lay, n_rays) * lay["slot"]                 # [R]
    rank = take((base[:, None] + 5 * Sp + torch.arange(S)[None]).reshape(-1)).view(n_rays, S)
    mask = rank >= 0
    count = mask.sum(1)
    # a ray's ranks count its shaded samples in ascending order
    want = torch.cumsum(mask.long(), 1) - 1
    assert bool((rank[mask] == want[mask]).all()) and bool((rank[~mask] == -1).all()), "rank array is not a prefix count"
    r_idx = mask.nonzero()[:, 0]
    e = rank[mask].long()
    tile0 = base[r_idx] + 6 * Sp + (e // 32) * rows * 32 + e % 32
    n = int(e.numel())
    relu = []
    for layer in range(2):
        m = torch.zeros(n, hidden, dtype=torch.bool)
        for h in range(2):
            word = take(tile0 + (lay["row_sign"] + 2 * layer + h) * 32)
            for mt in range(hidden // 32):
                for r in range(16):
                    m[:, mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h] = ((word >> (mt * 16 + r)) & 1).bool()
        relu.append(m)
    return mask, relu, count


def run_fused(tf, o, d, S, image, ray_idx, rays_per_view, ndc=False, white=True):
    """One launch of the single-launch pose kernel (csrc/jt_fused.hip) through the product entry point
    ops.render_pose_fused, under guard_band, on a freshly zeroed workspace (the `pose_fused` entry of ops._WS is dropped
    first).  image [views, 3, H, W], ray_idx [rays_per_view] (long).  Returns rgb, depth, opacity, sqerr, loss, g_o, g_d,
    the shading mask and ReLU signs decoded from the scratch slots (decode_fused_scratch: meaningful as they stand while
    the launch is one round), the layout, the raw workspace (`ws`, the live tensor) and the guard violations."""
    from joint_tensorf_amd import ops
    dev = tf.density_plane[0].device
    ops._WS.pop((str(dev), "pose_fused"), None)
    return run_fused_again(tf, o, d, S, image, ray_idx, rays_per_view, ndc=ndc, white=white)


def run_fused_again(tf, o, d, S, image, ray_idx, rays_per_view, ndc=False, white=True):
    """run_fused on the workspace as the previous launch left it"""
    from joint_tensorf_amd import ops
    dev = tf.density_plane[0].device
    R = o.shape[0]
    og, dg = o.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
    near, far = float(tf.near_far[0]), float(tf.near_far[1])
    zvals = torch.linspace(near, far, S, device=dev, dtype=torch.float32) if ndc else None
    cfg = tf._render_cfg(S, ndc, bool(white))
    guard = guard_band()
    with guard:
        out = ops.render_pose_fused(cfg, og, dg, zvals, image.to(dev), ray_idx.to(dev), int(rays_per_view),
                                    list(tf.density_plane), list(tf.density_line), list(tf.app_plane), list(tf.app_line),
                                    tf.basis_mat.weight, tf.renderModule.weights())
        out[0].backward()
        torch.cuda.synchronize()
    overruns = guard.violations()
    bufs = [base for shape, base, n in guard.held if shape == (R * 12 + 1,)]   # the launch's one output allocation
    assert len(bufs) == 1
    buf = bufs[0]
    ws = ops._WS[(str(dev), "pose_fused")]
    lay = fused_layout(cfg.scene(), R)
    mask, relu, count = decode_fused_scratch(ws, lay, R, S, tf.featureC)
    return dict(rgb=out[1].detach().clone(), depth=out[2].detach().clone(), opacity=out[3].detach().clone(),
                sqerr=buf[5 * R:6 * R].clone(), loss=out[0].detach().clone(), g_o=og.grad.detach().clone(),
                g_d=dg.grad.detach().clone(), shade_mask=mask, relu=relu if int(mask.sum()) else None, count=count,
                layout=lay, ws=ws, overruns=overruns, loss_scale=1.0 / (3.0 * R))


def _cfg32(cfg):
    c = copy.copy(cfg)
    for k in ("aabb", "aabbSize", "invaabbSize", "units", "stepSize"):
        setattr(c, k, getattr(cfg, k).float())
    return c


def _pinned_samplers(decide_dev):
    """sample_ray / sample_ray_ndc that take the z values, the in-box decision and the positions in fp32 on
    `decide_dev` (as the product path does); the positions are returned in the rays' type with the fp32 values and the
    derivatives of o + d z"""
    plain, ndc = O.sample_ray, O.sample_ray_ndc

    def wrap(fn):
        def f(cfg, rays_o, rays_d, N_samples, jitter=None):
            dev = decide_dev or rays_o.device
            c32 = _cfg32(cfg).to(dev)
            p32, z32, valid = fn(c32, rays_o.detach().float().to(dev), rays_d.detach().float().to(dev), N_samples,
                                 None if jitter is None else jitter.float().to(dev))
            z, valid = z32.to(rays_o.device).to(rays_o.dtype), valid.to(rays_o.device)
            pts = rays_o[..., None, :] + rays_d[..., None, :] * z[..., None]
            pts = p32.to(rays_o.device).to(rays_o.dtype) + (pts - pts.detach())
            return pts, z, valid
        return f
    return wrap(plain), wrap(ndc)


def _pinned_normalize(cfg, xyz):
    """normalize_coord with the fp32 value of (xyz - aabb[0]) * invaabbSize - 1 (three separately rounded fp32
    operations, jt_common.h normalize) and the derivative of the expression in xyz's type"""
    n = (xyz - cfg.aabb[0]) * cfg.invaabbSize - 1
    n32 = (xyz.detach().float() - cfg.aabb[0].float()) * cfg.invaabbSize.float() - 1
    return n32.to(n.dtype) + (n - n.detach())


def _axis32(g, size):
    """floor cell and fraction of the normalised coordinates g along an axis of `size` texels: the fp32 values of
    ix = ((g + 1) * 0.5) * (size - 1) (jt_common.h axis_taps; g holds fp32 values), the derivative of the fp64 ix"""
    ix32 = ((g.detach().float() + 1.0) * 0.5) * float(size - 1)
    fl = torch.floor(ix32)
    ix = (g + 1) * 0.5 * (size - 1)
    return fl.long(), (ix32 - fl).to(g.dtype) + (ix - ix.detach())


def pinned_taps(plane, gx, gy):
    """bilinear_taps with the cells and fractions of the product path's fp32 arithmetic (_axis32); plane [1, C, H, W]
    at normalised (gx, gy) [P] -> [C, P]"""
    _, C, H, W = plane.shape
    x0, fx = _axis32(gx, W)
    y0, fy = _axis32(gy, H)
    out = 0
    p = plane[0]
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            xx, yy = x0 + dx, y0 + dy
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            v = p[:, yy.clamp(0, H - 1), xx.clamp(0, W - 1)]
            out = out + v * (wx * wy * ok)[None]
    return out


def _pinned_plane(plane, gx, gy, use_taps=False):
    return pinned_taps(plane, gx, gy)


def _pinned_line(line, g, use_taps=False):
    return pinned_taps(line, torch.zeros_like(g), g)


def _pinned_mask_sample(alpha_mask, xyz):
    """alpha_mask_sample whose `> 0` is tests/mask_ref.py's keep on the fp32 sample positions the pinned sampler produced
    (xyz holds fp32 values): 1 where the mask keeps the sample, 0 where it drops it"""
    from tests import mask_ref
    return mask_ref.keep(alpha_mask[0], alpha_mask[1], xyz).to(xyz.device).to(xyz.dtype)


def reference(cfg, params, o, d, S, cot, ndc=False, white=True, app_mask=None, relu=None, keep=False, decide_dev=None,
              ray_only=False, alpha_mask=None, loss=None):
    """The oracle in params' dtype on params' device for rays (o, d) with the discrete decisions pinned; returns outputs,
    gradients of every parameter (T), the ray gradients and per factor M and F (see the module docstring).  keep=True
    also returns the recorded samples: (factor name, factor, samples [C, P], U [C, P]) per sampling call.  ray_only: the
    outputs and the ray gradients alone (the parameters should then not require a gradient; T, M and F are empty).
    alpha_mask: (volume [Z, Y, X], aabb [2, 3]) of an alpha mask, handed on to O.render with its decision pinned as the
    geometry is (_pinned_mask_sample).
    loss = (target [R, 3], loss_scale): the scalar that is differentiated is loss_scale * ((rgb.clamp(0, 1) - target)^2).sum()
    instead of the cotangent form (cot is not used; torch's clamp passes the gradient on the closed interval [0, 1]); the
    result then carries `sqerr` [R] and `loss` as well."""
    dev, dt = params["density_plane"][0].device, params["density_plane"][0].dtype
    names = {} if ray_only else {id(v): n for n, v in O.flat_params(params)}
    rec = []
    saved = (O._sample_plane, O._sample_line, O.sample_ray, O.sample_ray_ndc, O.normalize_coord, O.alpha_mask_sample)

    def wrap(fn):
        def f(factor, *a):
            out = fn(factor, *a)
            if id(factor) in names and out.requires_grad:
                out.retain_grad()
                rec.append((names[id(factor)], factor, out))
            return out
        return f
    oc, dc = o.to(dev).to(dt).requires_grad_(True), d.to(dev).to(dt).requires_grad_(True)
    O._sample_plane, O._sample_line = wrap(_pinned_plane), wrap(_pinned_line)
    O.sample_ray, O.sample_ray_ndc = _pinned_samplers(decide_dev)
    O.normalize_coord = _pinned_normalize
    O.alpha_mask_sample = _pinned_mask_sample
    rep = {}
    try:
        rgb, depth, acc = O.render(cfg, params, oc, dc, S, white_bg=white, ndc_ray=ndc, app_mask_override=app_mask,
                                   relu_masks_override=relu, relu_report=rep, alpha_mask=alpha_mask)
    finally:
        O._sample_plane, O._sample_line, O.sample_ray, O.sample_ray_ndc, O.normalize_coord, O.alpha_mask_sample = saved
    extra = {}
    if loss is not None:
        sq = ((rgb.clamp(0, 1) - loss[0].to(dev).to(dt)) ** 2).sum(-1)
        tot = float(loss[1]) * sq.sum()
        extra = dict(sqerr=sq.detach(), loss=tot.detach())
    else:
        tot = (rgb * cot[0].to(dev).to(dt)).sum() + (acc * cot[1].to(dev).to(dt)).sum()
    if tot.requires_grad:
        tot.backward(retain_graph=not ray_only)
    if ray_only:
        return dict(samples=[], rgb=rgb.detach(), depth=depth.detach(), opacity=acc.detach(), T={}, M={}, F={},
                    g_o=torch.zeros_like(oc) if oc.grad is None else oc.grad.detach(),
                    g_d=torch.zeros_like(dc) if dc.grad is None else dc.grad.detach(), relu=rep, **extra)
    T = {n: (torch.zeros_like(v) if v.grad is None else v.grad.detach().clone()) for n, v in O.flat_params(params)}
    M = {n: torch.zeros_like(T[n]) for n in FACTORS}
    F = {n: torch.zeros_like(T[n]) for n in FACTORS}
    kept = []
    for n, factor, out in rec:
        U = out.grad if out.grad is not None else torch.zeros_like(out)
        M[n] += torch.autograd.grad(out, factor, grad_outputs=U.abs(), retain_graph=True)[0]
        F[n] += torch.autograd.grad(out, factor, grad_outputs=torch.ones_like(out), retain_graph=True)[0]
        if keep:
            kept.append((n, factor, out, U))
    del rec
    return dict(samples=kept, rgb=rgb.detach(), depth=depth.detach(), opacity=acc.detach(), T=T, M=M,
                F={n: v > 0 for n, v in F.items()},
                g_o=torch.zeros_like(oc) if oc.grad is None else oc.grad.detach(),
                g_d=torch.zeros_like(dc) if dc.grad is None else dc.grad.detach(), relu=rep, **extra)


def params_of(tf, dtype=torch.float64):
    sd = {k: v.detach().clone().contiguous().to(dtype) for k, v in tf.state_dict().items()}
    p = O.params_from_state_dict(sd, prefix="")
    for _, v in O.flat_params(p):
        v.requires_grad_(True)
    return p


def run_reference(tf, kind, hip, o, d, S, cot_seed=0, ndc=False, white=True, step_ratio=0.5, thres=1e-7, ray_only=False,
                  slice_entries=1 << 16, loss=None):
    """the fp64 reference of run_hip's iteration, pinned to its shading mask and ReLU signs.  It runs on the CPU (the
    same fp64 arithmetic; the GPU's fp64 atomics in grid_sample's backward made the long-line rows ten times slower),
    with the fp32 sample decisions taken on the GPU like the product path's.  ray_only (a pose-only iteration): outputs
    and ray gradients alone, the rays taken in slices of about slice_entries shaded samples (rays are independent).
    When tf carries an alpha mask (tf.alphaMask), the reference renders with it, its decision pinned (reference).
    loss = (target [R, 3], loss_scale): the loss form of `reference` (the result carries sqerr [R] and loss)."""
    am = None if tf.alphaMask is None else (tf.alphaMask.alpha_volume[0, 0].detach().cpu(), tf.alphaMask.aabb.detach().cpu())
    cfg = scene_cfg(tf.aabb.view(-1).tolist(), tf.gridSize.tolist(), [float(tf.near_far[0]), float(tf.near_far[1])], kind,
                    step_ratio, thres, "cpu", torch.float64)
    relu = None if hip["relu"] is None else [m.cpu() for m in hip["relu"]]
    params = params_of(tf)
    for _, v in O.flat_params(params):
        v.data = v.data.cpu()
    if ray_only:
        for _, v in O.flat_params(params):
            v.requires_grad_(False)
        mask = hip["shade_mask"].cpu()
        cot = cotangents(o.shape[0], cot_seed)
        ends = torch.cumsum(mask.sum(1), 0)             # shaded entries up to and including each ray (ray-major order)
        parts, rep, a = [], {}, 0
        while a < o.shape[0]:
            e0 = int(ends[a - 1]) if a else 0
            b = max(a + 1, int(torch.searchsorted(ends, torch.tensor(e0 + slice_entries), right=True)))
            b = min(b, o.shape[0])
            e1 = int(ends[b - 1])
            r = None if relu is None else [m[e0:e1] for m in relu]
            part = reference(cfg, params, o[a:b].cpu(), d[a:b].cpu(), S, (cot[0][a:b], cot[1][a:b]), ndc=ndc, white=white,
                             app_mask=mask[a:b], relu=r, decide_dev=tf.density_plane[0].device, ray_only=True,
                             alpha_mask=am, loss=None if loss is None else (loss[0][a:b], loss[1]))
            for k, v in part.pop("relu").items():
                rep[k] = max(rep.get(k, 0.0), v) if k == "max_abs" else rep.get(k, 0) + v
            parts.append(part)
            a = b
        out = {k: torch.cat([p[k] for p in parts]) for k in ("rgb", "depth", "opacity", "g_o", "g_d")}
        if loss is not None:
            out["sqerr"] = torch.cat([p["sqerr"] for p in parts])
            out["loss"] = sum(p["loss"] for p in parts)
        out["relu"] = rep
        return out
    return reference(cfg, params, o.cpu(), d.cpu(), S, cotangents(o.shape[0], cot_seed), ndc=ndc, white=white,
                     app_mask=hip["shade_mask"].cpu(), relu=relu, decide_dev=tf.density_plane[0].device, alpha_mask=am,
                     loss=loss)


def far_node_samples(aabb, grid, near_far, o, d, S, ndc=False, step_ratio=0.5, device="cpu"):
    """(valid [R, S], far [R, S, 3]) from the pinned fp32 geometry alone (the oracle's sampler and normalisation in
    fp32, _axis32's cell): far[r, s, a] says that in-box sample s of ray r sits on the far node of axis a,
    floor(ix) == size - 1 -- its upper tap is out of range, the case in which the kernels must mask taps (grid_sample's
    zero padding) instead of interpolating in the nested form."""
    cfg = scene_cfg(aabb, grid, list(near_far), "llff", step_ratio, 1e-7, device)   # (the kind does not enter the geometry)
    fn = O.sample_ray_ndc if ndc else O.sample_ray
    pts, _, valid = fn(cfg, o.float().to(device), d.float().to(device), S)
    n = O.normalize_coord(cfg, pts)
    far = torch.stack([_axis32(n[..., a], grid[a])[0] == grid[a] - 1 for a in range(3)], -1) & valid[..., None]
    return valid.cpu(), far.cpu()


def census(far, shade_mask, chunk=1 << 22):
    """Tile census of a pose-only backward from the reference side: the shaded entries in the kernels' order (ray-major,
    ascending sample), cut into backward chunks of `chunk` entries and 32-entry tiles within a chunk.  far [R, S] (or
    [R, S, 3]: any axis).  Returns the number of shaded entries, the tiles of every chunk, how many tiles hold at least
    one far-node sample, how many hold none, and the far-node entries."""
    if far.dim() == 3:
        far = far.any(-1)
    f = far.cpu()[shade_mask.cpu()]
    n = f.numel()
    e = torch.arange(n)
    per_chunk = (chunk + 31) // 32
    tile = (e // chunk) * per_chunk + (e % chunk) // 32
    tiles = [(min(chunk, n - c) + 31) // 32 for c in range(0, n, chunk)]
    hit = torch.zeros(max(1, per_chunk * len(tiles)), dtype=torch.bool)
    hit[tile[f]] = True
    nfar = int(hit.sum())
    return dict(shaded=n, tiles=tiles, far_tiles=nfar, plain_tiles=sum(tiles) - nfar, far_entries=int(f.sum()))


def factor_errors(G, T, M, F):
    """(number of writes outside F, worst |G - T| / (2^-24 M) inside F, its index).  An element of F with M == 0 takes
    ratio 0 when G == T and inf otherwise."""
    G, T, M = G.double(), T.double(), M.double()
    stray = int(((G != 0) & ~F).sum())
    diff = (G - T).abs()
    ratio = torch.where(M > 0, diff / (EPS32 * M).clamp_min(1e-300), torch.where(diff > 0, float("inf"), 0.0))
    ratio = torch.where(F, ratio, torch.zeros_like(ratio))
    k = int(ratio.flatten().argmax())
    return stray, float(ratio.flatten()[k]), k


def ray_atol(g, t, rtol):
    """the smallest atol (relative to max |t|) with |g - t| <= rtol |t| + atol max |t| element by element"""
    g, t = g.double(), t.double()
    scale = float(t.abs().max())
    if scale == 0.0:
        return 0.0 if float(g.abs().max()) == 0.0 else float("inf")
    return max(0.0, float(((g - t).abs() - rtol * t.abs()).max()) / scale)


def max_rel(g, t):
    g, t = g.double(), t.double()
    return float((g - t).abs().max() / t.abs().max().clamp_min(1e-30))
