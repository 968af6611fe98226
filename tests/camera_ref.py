"""fp64 reference, seeded inputs and the element-wise criterion for the camera kernels (jt_camera.hip): pose composition
and ray generation, rectangular and ragged.  CPU only; tests/test_camera_ref.py checks this module without a GPU and
tests/test_gpu_camera_paths.py judges the kernels with it.

The reference is the project's oracle (oracle/tensorf_oracle.py) evaluated in float64 on the fp32 VALUES of the inputs:
its functions follow the dtype of their arguments, and it uses the same nine-term Taylor series as the kernel, so the
fp64 result is the kernel's target (not the closed form of exp).

A gradient G of an fp32 implementation is judged element by element against the fp64 gradient T and a magnitude M >= |T|,
the sum of the absolute values of the contributions that form the element:  |G - T| <= kappa 2^-24 M  (kappa()).
  * ray generation: a pose entry's gradient is a sum over the view's rays; M is the sum over the rays of the absolute
    value of each ray's own contribution (raygen_terms: one autograd pass over a pose replicated per ray).  A lost ray of
    a view of r similar rays is of order 2^24 / r in these units.
  * pose composition: g_se3[b, e] = sum_ij dpose_ij / dwu_e cot_ij, M the same sum of absolute values (pose_terms: the
    fp64 Jacobian from twelve one-hot backward passes, batched over the views).
A forward output g is judged by  |g - t| <= kappa_f 2^-24 (|t| + s), with s the scale of the terms that form the output
(forward_error); the scales:
  * pose: R = R_base (I + A wx + B wx^2): s = 1 + |w| + |w|^2 for the nine rotation entries (|R_base| <= 1, A, B <= 1);
    t = R_base (V u) + t_base, V = I + B wx + C wx^2: s = (1 + |w| + |w|^2) |u|_1 + max |t_base| + 1;
  * ray centres without NDC, c_j = -sum_i t_i R_ij: s = max_i |t_i| + 1;
  * ray directions without NDC, d = (K^-1 p) R: s = |K^-1 p| (the Euclidean norm of the camera-space direction);
  * under NDC the outputs are sums and products of the quotients cx/cz, cy/cz, rx/rz, ry/rz and 2 near / cz (c the centre
    moved to the near plane): s_o = (sx |cx/cz|, sy |cy/cz|, 1 + |2 near/cz|), s_d = (sx (|rx/rz| + |cx/cz|),
    sy (|ry/rz| + |cy/cz|), |2 near/cz|), each plus the scale of the un-normalised ray it was formed from
    (max |t| + 1 for the centre, |K^-1 p| for the direction) times sx or sy or 2 near: the quotients inherit the
    rounding of c and r, which is relative to those scales and not to the quotient.

The kappa bounds are NOT fitted to the kernels: each is 4x what the float32 ORACLE on the CPU shows against the float64
oracle on the same inputs (ORACLE32 below, measured by tests/test_camera_ref.py, which also asserts that the fp32 oracle
stays within HALF of each bound).  4x because the kernel sums a view's rays as 256 sequential partial sums and a wave
tree where torch sums pairwise, and may contract to FMA where torch does not; the arithmetic is otherwise the same."""
import math

import torch

from oracle import tensorf_oracle as O  # checker only

EPS32 = 2.0 ** -24
H, W = 30, 40
NEAR = 1.0

# Worst kappa / kappa_f of the float32 oracle (torch on the CPU, same inputs as the GPU tests) against the float64 oracle,
# per input family, over every input set of POSE_CASES / RAYGEN_CASES / the ragged set (tests/test_camera_ref.py
# test_oracle32_kappa_table prints them).  Rounded up to two digits.
ORACLE32 = {
    "pose_grad": 20.0,        # fp32 O.train_pose backward vs pose_terms (measured 19.14, B = 65 with noise)
    "pose_fwd": 0.97,         # fp32 O.train_pose vs fp64 (measured 0.970)
    "raygen_grad": 5.9,      # fp32 O.rays_for_pixels backward vs raygen_terms, no NDC (measured 5.89, r = 1)
    "raygen_grad_ndc": 61.0,  # fp32 O.rays_for_pixels + O.convert_ndc backward vs raygen_terms (60.4, r = 1)
    "rays_o": 0.52,           # fp32 centres vs fp64, no NDC (0.514)
    "rays_d": 0.84,           # fp32 directions vs fp64, no NDC (0.831)
    "rays_o_ndc": 1.3,       # fp32 NDC origins vs fp64 (1.282)
    "rays_d_ndc": 0.65,       # fp32 NDC directions vs fp64 (0.642)
}
KAPPA = {k: 4.0 * v for k, v in ORACLE32.items()}   # what the kernels are allowed

POSE_B = (1, 63, 64, 65, 130)                 # k_pose_fwd / k_pose_bwd: 64 threads per block
POSE_FORMS = ("noise", "no-noise", "shared-gt")
RAYGEN_R = (1, 63, 64, 65, 255, 256, 257, 1025)   # k_raygen_bwd: 256-thread stride per view, 64-lane waves
# (B, r): B = 3 at every r; B = 1; and B r = 5 x 77 = 385, no multiple of the forward's 256-thread block
RAYGEN_CASES = tuple((3, r) for r in RAYGEN_R) + ((1, 257), (5, 77))
# empty first view, one ray, 256 rays, empty middle view, 257 rays, 1 025 rays, empty last view
RAGGED_SIZES = (0, 1, 256, 0, 257, 1025, 0)
W_MAGS = (2.5, 0.0, 1e-4, 1.0, math.pi)        # |w| of the special rows (row b takes W_MAGS[b % 6], every sixth is random)


def ragged_offsets(sizes=RAGGED_SIZES):
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return torch.tensor(off, dtype=torch.int32)


def pose_inputs(B, form, seed=0):
    """(se3 [B,6], noise [B,3,4] or None, gt [B,3,4] or [3,4], cot [B,3,4]) fp32 on the CPU.  Row b has |w| =
    W_MAGS[b % 6] (w = 0 exactly, 1e-4, 1, 2.5, pi; every sixth row a random |w| < pi) in a random direction, u uniform in
    [-4, 4]^3.  |w| <= pi in exact arithmetic on the fp32 values (the pi rows are shrunk by 1e-6): beyond pi the
    nine-term series cancels in fp32 and in the reference alike."""
    g = torch.Generator().manual_seed(1000 * B + 10 * POSE_FORMS.index(form) + seed)
    dirs = torch.randn(B, 3, generator=g, dtype=torch.float64)
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    mags = torch.rand(B, generator=g, dtype=torch.float64) * 3.0
    for b in range(B):
        if b % 6 < len(W_MAGS):
            mags[b] = W_MAGS[b % 6] * (1.0 - 1e-6 if W_MAGS[b % 6] > 3.0 else 1.0)
    w = (dirs * mags[:, None]).float()
    assert float(w.double().norm(dim=-1).max()) <= math.pi
    u = (torch.rand(B, 3, generator=g, dtype=torch.float64) * 8.0 - 4.0).float()
    se3 = torch.cat([w, u], -1).contiguous()
    noise = O.se3_to_SE3(torch.randn(B, 6, generator=g, dtype=torch.float64) * 0.15).float().contiguous()
    gt = O.se3_to_SE3(torch.randn(B, 6, generator=g, dtype=torch.float64)).float().contiguous()
    gt[..., 3] += torch.tensor([0.0, 0.0, 4.0])
    cot = torch.randn(B, 3, 4, generator=g)
    if form == "no-noise":
        noise = None
    if form == "shared-gt":
        gt = gt[0].clone()
    return se3, noise, gt, cot


def pose_forward(se3, noise, gt):
    """(pose [B,3,4] fp64, scale s [B,3,4]) of the fp32 values (module docstring)"""
    wu = se3.double()
    n64 = None if noise is None else noise.double()
    pose = O.train_pose(wu, n64, gt.double())
    base = gt.double() if n64 is None else O.compose_pair(n64, gt.double())
    base = base.expand(wu.shape[0], 3, 4)
    th = wu[:, :3].norm(dim=-1)
    sR = 1 + th + th * th
    st = sR * wu[:, 3:].abs().sum(-1) + base[..., 3].abs().amax(-1) + 1
    s = torch.cat([sR[:, None, None].expand(-1, 3, 3), st[:, None, None].expand(-1, 3, 1)], -1)
    return pose, s


def pose_terms(se3, noise, gt, cot):
    """(T, M) [B,6] fp64: T = d sum(pose cot) / d se3, M[b,e] = sum_ij |d pose_ij / d wu_e| |cot_ij| from the fp64 Jacobian
    (twelve one-hot backward passes; the views are independent, so each pass serves all of them)"""
    wu = se3.double().clone().requires_grad_(True)
    pose = O.train_pose(wu, None if noise is None else noise.double(), gt.double())
    c = cot.double()
    T = torch.zeros_like(wu)
    M = torch.zeros_like(wu)
    for i in range(3):
        for j in range(4):
            (J,) = torch.autograd.grad(pose[:, i, j].sum(), wu, retain_graph=True)
            T = T + J * c[:, i, j, None]
            M = M + J.abs() * c[:, i, j, None].abs()
    return T.detach(), M.detach()


def raygen_inputs(B, r, ndc, seed=0):
    """(pose [B,3,4], intr [B,3,3], intr_inv [B,3,3] as torch.linalg.inv returns it (column-major), ray_idx [r] int64,
    cot_o, cot_d [B,r,3]) fp32 on the CPU.  f = 0.8 W, cx = W / 2 + b; the pixel list has repeats and holds pixel H W - 1 and (r >= 2)
    pixel 0; under NDC the poses are near the identity (forward-facing)."""
    g = torch.Generator().manual_seed(100000 * int(ndc) + 1000 * B + r + 7 * seed)
    if ndc:
        pose = torch.eye(3, 4)[None].repeat(B, 1, 1) + 0.02 * torch.randn(B, 3, 4, generator=g)
    else:
        pose = O.se3_to_SE3(torch.randn(B, 6, generator=g, dtype=torch.float64)).float()
        pose[..., 3] += torch.tensor([0.0, 0.0, 4.0])
    pose = pose.contiguous()
    f = 0.8 * W
    intr = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]])[None].repeat(B, 1, 1)
    intr[:, 0, 2] += torch.arange(B).float()   # a principal point of its own per view: the kernels index intrinsics by view
    intr_inv = torch.linalg.inv(intr)
    ray_idx = torch.randint(0, H * W, (r,), generator=g)
    ray_idx[r // 2] = H * W - 1
    if r >= 2:
        ray_idx[r - 1] = 0
    cot_o, cot_d = torch.randn(B, r, 3, generator=g), torch.randn(B, r, 3, generator=g)
    return pose, intr, intr_inv, ray_idx, cot_o, cot_d


def ragged_inputs(ndc, sizes=RAGGED_SIZES, seed=0):
    """the ragged batch: (pose [V,3,4], intr, intr_inv, ray_idx [n], view_offset [V+1] int32, cot_o, cot_d [n,3])"""
    V, n = len(sizes), sum(sizes)
    pose, intr, intr_inv, _, _, _ = raygen_inputs(V, 1, ndc, seed=seed + 50)
    g = torch.Generator().manual_seed(31 + int(ndc) + 7 * seed)
    ray_idx = torch.randint(0, H * W, (n,), generator=g)
    ray_idx[0], ray_idx[n - 1] = H * W - 1, 0
    cot_o, cot_d = torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)
    return pose, intr, intr_inv, ray_idx, ragged_offsets(sizes), cot_o, cot_d


def _rays_per_ray(P, Ki, K, ray_idx, ndc, near):
    """rays of pseudo-views: P [r,3,4], Ki, K [r,3,3], ray k of pseudo-view k -> (o, d) [r,3] in P's dtype, and the
    un-normalised (centre, direction)"""
    c, d = O.rays_for_pixels(P, Ki, ray_idx, W)          # [r, r, 3]
    k = torch.arange(ray_idx.numel())
    c, d = c[k, k][:, None], d[k, k][:, None]            # [r, 1, 3]
    c0, d0 = c, d
    if ndc:
        c, d = O.convert_ndc(c, d, K, near=near)
    return c[:, 0], d[:, 0], c0[:, 0], d0[:, 0]


def raygen_forward(pose, intr, intr_inv, ray_idx, ndc, near=NEAR, dtype=torch.float64):
    """(o, d, s_o, s_d) [B,r,3] in `dtype` (float64: the reference and its scales; float32: the fp32 oracle) -- the scales
    of the module docstring, from the fp64 values"""
    B, r = pose.shape[0], ray_idx.numel()
    if r == 0:
        z = torch.zeros(B, 0, 3, dtype=dtype)
        return z, z, z, z
    p, k, ki = pose.to(dtype), intr.to(dtype), intr_inv.to(dtype)
    c0, d0 = O.rays_for_pixels(p, ki, ray_idx, W)
    o, d = (c0, d0) if not ndc else O.convert_ndc(c0, d0, k, near=near)
    x = (ray_idx % W).to(dtype) + 0.5
    y = torch.div(ray_idx, W, rounding_mode="floor").to(dtype) + 0.5
    gcam = torch.stack([x, y, torch.ones_like(x)], -1)[None] @ ki.transpose(-1, -2)
    sc = (p[..., 3].abs().amax(-1) + 1)[:, None, None].expand(B, r, 3)
    sd = gcam.norm(dim=-1, keepdim=True).expand(B, r, 3)
    if not ndc:
        return o.detach(), d.detach(), sc, sd
    shift = (near - c0[..., 2:]) / d0[..., 2:]
    c = c0 + shift * d0
    sx, sy = (k[:, 0, 0] / k[:, 0, 2])[:, None], (k[:, 1, 1] / k[:, 1, 2])[:, None]
    cxoz, cyoz, icz = (c[..., 0] / c[..., 2]).abs(), (c[..., 1] / c[..., 2]).abs(), (2 * near / c[..., 2]).abs()
    rxoz, ryoz = (d0[..., 0] / d0[..., 2]).abs(), (d0[..., 1] / d0[..., 2]).abs()
    amp = torch.stack([sx.expand(B, r), sy.expand(B, r), torch.full((B, r), 2 * near, dtype=dtype)], -1)
    s_o = torch.stack([sx * cxoz, sy * cyoz, 1 + icz], -1) + amp * sc
    s_d = torch.stack([sx * (rxoz + cxoz), sy * (ryoz + cyoz), icz], -1) + amp * (sc + sd)
    return o.detach(), d.detach(), s_o.detach(), s_d.detach()


def raygen_terms(pose, intr, ray_idx, W_, cot_o, cot_d, ndc, near=NEAR, intr_inv=None):
    """(T, M) [B,3,4] fp64: T the gradient of sum(o cot_o) + sum(d cot_d) with respect to the pose, M the sum over the
    view's rays of the absolute value of each ray's own contribution.  One autograd pass per view over that view's pose
    replicated per ray: ray k of pseudo-view k, .grad [r,3,4] holds the contributions.  For a ragged batch call it per
    view on that view's slice (ragged_terms)."""
    assert W_ == W
    B, r = pose.shape[0], ray_idx.numel()
    T = torch.zeros(B, 3, 4, dtype=torch.float64)
    M = torch.zeros(B, 3, 4, dtype=torch.float64)
    if r == 0:
        return T, M
    ki = (torch.linalg.inv(intr) if intr_inv is None else intr_inv).double()
    for b in range(B):
        P = pose[b].double().expand(r, 3, 4).clone().requires_grad_(True)
        o, d, _, _ = _rays_per_ray(P, ki[b].expand(r, 3, 3), intr[b].double().expand(r, 3, 3), ray_idx, ndc, near)
        ((o * cot_o[b].double()).sum() + (d * cot_d[b].double()).sum()).backward()
        T[b], M[b] = P.grad.sum(0), P.grad.abs().sum(0)
    return T, M


def ragged_views(voff):
    v = voff.tolist()
    return [(b, v[b], v[b + 1]) for b in range(len(v) - 1)]


def ragged_terms(pose, intr, intr_inv, ray_idx, voff, cot_o, cot_d, ndc, near=NEAR):
    """raygen_terms and raygen_forward view by view on a ragged batch: (o, d, s_o, s_d [n,3], T, M [V,3,4])"""
    V = pose.shape[0]
    T, M = torch.zeros(V, 3, 4, dtype=torch.float64), torch.zeros(V, 3, 4, dtype=torch.float64)
    outs = [[], [], [], []]
    for b, a, e in ragged_views(voff):
        sl = slice(b, b + 1)
        T[sl], M[sl] = raygen_terms(pose[sl], intr[sl], ray_idx[a:e], W, cot_o[None, a:e], cot_d[None, a:e], ndc, near,
                                    intr_inv=intr_inv[sl])
        for lst, t in zip(outs, raygen_forward(pose[sl], intr[sl], intr_inv[sl], ray_idx[a:e], ndc, near)):
            lst.append(t[0])
    return tuple(torch.cat(x) for x in outs) + (T, M)


def kappa(G, T, M):
    """max |G - T| / (2^-24 M) over the elements with M > 0; where M == 0, G must be exactly 0 (inf otherwise)"""
    G, T, M = G.detach().double().cpu(), T.double(), M.double()
    pos = M > 0
    worst = float(((G - T).abs()[pos] / (EPS32 * M[pos])).max()) if bool(pos.any()) else 0.0
    if bool((G[~pos] != 0).any()):
        return float("inf")
    return worst


def forward_error(g, t, s):
    """kappa_f of an output: max |g - t| / (2^-24 (|t| + s)), element by element"""
    if t.numel() == 0:
        return 0.0
    g, t = g.detach().double().cpu(), t.double()
    return float(((g - t).abs() / (EPS32 * (t.abs() + s.double()))).max())


def oracle32_pose(se3, noise, gt, cot):
    """the float32 oracle's pose and gradient (plain torch on the CPU)"""
    a = se3.clone().requires_grad_(True)
    pose = O.train_pose(a, noise, gt)
    (pose * cot).sum().backward()
    return pose.detach(), a.grad.detach()


def oracle32_raygen(pose, intr, intr_inv, ray_idx, cot_o, cot_d, ndc, near=NEAR):
    """the float32 oracle's rays [B,r,3] and pose gradient"""
    p = pose.clone().requires_grad_(True)
    o, d = O.rays_for_pixels(p, intr_inv, ray_idx, W)
    if ndc:
        o, d = O.convert_ndc(o, d, intr, near=near)
    ((o * cot_o).sum() + (d * cot_d).sum()).backward()
    return o.detach(), d.detach(), p.grad.detach()
