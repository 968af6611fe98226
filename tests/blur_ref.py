"""fp64 reference, magnitude and acceptance criterion for the separable blur (csrc/jt_blur.hip), for
tests/test_blur_ref.py (CPU) and tests/test_gpu_blur_paths.py (MI355X).  Nothing here needs a GPU except Arena.

Operator.  A factor is stored channel-last, [H][W][C].  One pass blurs one axis of length n with ntaps = 2 r + 1 taps k,
replicate padding, cross-correlation:
    forward   out[u] = sum_t k[t] in[clamp(u + t - r, 0, n - 1)]
    adjoint   gin[u] = sum_x g[x] ( k[u - x + r] + [u == 0] L_x + [u == n - 1] R_x ),
              L_x = sum_{t < r - x} k[t]   (the taps the padding sent to texel 0),
              R_x = sum_{t >= n - x + r} k[t]   (the taps it sent to texel n - 1).
A plane (H > 1 and W > 1) runs W then H forward and H then W in the adjoint; anything else has one pass (along H when
H > 1, else along W).

Reference.  oracle.tensorf_oracle.blur_plane / blur_line on double tensors, the fp32 taps promoted exactly; the adjoint
is autograd through them in double.  There is no second implementation of the operator here: the per-pass form used
for the magnitude is blur_line on a re-laid-out tensor (test_blur_ref.py holds its composition to blur_plane).

Magnitude M (from the inputs only, never from the output under test).  Forward: the same operator with |k| on |in|.
Adjoint: its transpose with |k| on |g|, plus a term for texel n - 1 of each pass.  Every kernel forms R_x as
    c_x = s_cum[ntaps] - s_cum[j_x],   j_x = min(n - x + r, ntaps),   s_cum[j] = fl(sum_{t < j} k[t]),
i.e. as the difference of two fp32 prefix sums.  Each prefix sum carries an error up to gamma_{ntaps-1} S_j with
S_j = sum_{t < j} |k[t]|, whatever the sign pattern, so c_x is only good to gamma (S_ntaps + S_{j_x}) while |k| on |g|
credits the texel with S_ntaps - S_{j_x} (what |R_x| can reach at most).  The difference, 2 S_{j_x}, is the magnitude of
what cancels in the subtraction -- it is the whole error budget for Gaussian taps, whose R_x is 1e-7 of S_ntaps -- so
    E[n - 1] = 2 sum_{x = max(n - r, 0)}^{n - 1} |g[x]| S_{j_x}
is added to M of texel n - 1 of that pass (and the second pass of a plane sees the first pass's M + E as its |g|).
The left fold needs nothing: L_x = s_cum[r - x] is a plain prefix sum, S_{r-x} |g[x]| is already in M.

Criterion.  |out - ref| <= kappa 2^-24 M on EVERY element; kappa is derived, not tuned.  With u = 2^-24 an fp32 sum of
m products accumulated in any order is within gamma_m sum|a_i b_i|, gamma_m = m u / (1 - m u) (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1); exact zeros among the addends cost nothing.  Addends per element, pass:
    k_blur_line, k_blur_axis, k_blur_batch   m = ntaps          (the other kLineP - 1 window inputs have weight 0)
    k_blur_mfma                              m = 4 kMfmaK = 80  (the whole band goes through the matrix cores)
On the two border texels of an adjoint pass a term goes through more roundings: ntaps for its coefficient (ntaps - 1
additions of the prefix sum and the subtraction), its product and accumulation (at most m: the fold loops of
k_blur_line / k_blur_mfma run over <= r addends, blur_axis_block folds the coefficient into the weight table and
accumulates <= ntaps of them), and the two additions that join the folds to the band: m + ntaps + 2.
Two passes: the first pass's error goes through the second operator (|A| M1 = M) and the second adds its own:
kappa u = (1 + gamma_1)(1 + gamma_2) - 1, i.e. kappa_1 + kappa_2 to first order.  Per element (y, x) of a plane's adjoint
the H pass counts as border when y is 0 or H - 1 and the W pass when x is 0 or W - 1.
    ntaps                     1    3    9    63    65    67    201
    vector, forward 2 passes  2    6   18   126   130   134    402
    vector, adjoint corner    8   16   40   256   264   272    808
    mfma,   forward 2 passes 160  160  160   160   160    -      -
    mfma,   adjoint corner   166  170  182   290   294    -      -
A correct fp32 implementation sits far below (torch.float32 conv1d: kappa <= 8.4 on the shapes of test_blur_ref.py; the
worst ratios measured on MI355X are in tests/test_gpu_blur_paths.py); the bound still decides, because one dropped tap
of order 1 is about 1e5 x 2^-24 M.

Exact rows.  Integer data, integer taps, integer upstream gradients, chosen so that M < 2^24 everywhere (asserted in
exact_magnitude_ok from the inputs; exact_kinds shrinks the ranges past 65 taps, and 201-tap adjoint rows are lines
or small planes: a corner texel of a plane collects the folds of r x r gradients): every product, partial sum and prefix sum is then an integer below 2^24, fp32 is
exact in any summation order (the matrix-core pass and s_cum included), and the output must equal the fp64 reference
bit for bit.  The cancellation term E is not part of that assertion: it bounds rounding, and nothing rounds here.
"""
import numpy as np
import torch

from oracle import tensorf_oracle as O

U = 2.0 ** -24
K_MFMA_ADDENDS = 80   # 4 * kMfmaK of jt_blur.hip
MFMA, LINE, AXIS, BATCH = "k_blur_mfma", "k_blur_line", "k_blur_axis", "k_blur_batch"


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def make_taps(kind, ntaps, seed=0):
    """fp32 tap vectors.  Every kind but "gauss:<sigma>" gives every tap weight.
    signed: asymmetric uniform(-1, 1), none smaller than 0.05;  flat: ones;  onehot:<t>;  ramp: (1 + t) / ntaps;
    int[:<hi>]: asymmetric integers in [-hi, hi], hi = 4 unless given (the two outermost taps non-zero);  gauss:<sigma>: the project's gaussian_kernel"""
    assert ntaps % 2 == 1
    g = torch.Generator().manual_seed(1000 + 7 * ntaps + seed)
    if kind == "signed":
        k = torch.rand(ntaps, generator=g) * 2 - 1
        k = torch.where(k.abs() < 0.05, torch.full_like(k, 0.5), k)
    elif kind == "flat":
        k = torch.ones(ntaps)
    elif kind.startswith("onehot:"):
        k = torch.zeros(ntaps)
        k[int(kind.split(":")[1])] = 1.0
    elif kind == "ramp":
        k = (1.0 + torch.arange(ntaps, dtype=torch.float32)) / ntaps
    elif kind.startswith("int"):
        hi = int(kind.split(":")[1]) if ":" in kind else 4
        k = torch.randint(-hi, hi + 1, (ntaps,), generator=g).float()
        k[0], k[-1] = float(hi), float(-max(hi - 1, 1))
    elif kind.startswith("gauss:"):
        k = O.gaussian_kernel(float(kind.split(":")[1]), ntaps - 1)
        assert k.numel() == ntaps
    else:
        raise ValueError(kind)
    return k.float().contiguous()


def make_data(shape, kind, seed=0):
    """[H, W, C] fp32: "randn", or "int[:<hi>]" (integers in [-hi, hi], hi = 8 unless given)"""
    g = torch.Generator().manual_seed(seed)
    if kind == "randn":
        return torch.randn(*shape, generator=g)
    if kind.startswith("int"):
        hi = int(kind.split(":")[1]) if ":" in kind else 8
        return torch.randint(-hi, hi + 1, tuple(shape), generator=g).float()
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------------------------
# reference (oracle in double)
# ---------------------------------------------------------------------------------------------------------------------
def passes(H, W, adjoint=False):
    """[(axis, n)] in execution order; axis 0 = along H, 1 = along W (launch_blur_batch / jt_blur_forward)"""
    if H > 1 and W > 1:
        return [(0, H), (1, W)] if adjoint else [(1, W), (0, H)]
    return [(0, H)] if H > 1 else [(1, W)]


def forward_ref(x, taps, dtype=torch.float64):
    """x [H, W, C] (any float type) -> [H, W, C]: oracle blur_plane / blur_line in double (dtype=torch.float32: the fp32
    oracle, a correct single-precision implementation to hold the criterion against)"""
    H, W, C = x.shape
    k = taps.to(dtype)
    xl = x.to(dtype).permute(2, 0, 1)[None].contiguous()         # logical [1, C, H, W]
    if H > 1 and W > 1:
        out = O.blur_plane(k, xl, H, W)                          # (the reshape of a contiguous [C, H, W] is the identity)
    elif H > 1:
        out = O.blur_line(k, xl)
    else:
        out = O.blur_line(k, xl.reshape(1, C, W, 1)).reshape(1, C, 1, W)
    return out[0].permute(1, 2, 0).contiguous()


def adjoint_ref(g, taps, dtype=torch.float64):
    """g [H, W, C] -> [H, W, C]: autograd through forward_ref in double"""
    x = torch.zeros(tuple(g.shape), dtype=dtype, requires_grad=True)
    (forward_ref(x, taps, dtype) * g.to(dtype)).sum().backward()
    return x.grad.detach()


def one_pass(x, k, axis):
    """one pass of the operator along `axis` of [H, W, C] as oracle blur_line on a re-laid-out tensor (differentiable)"""
    H, W, C = x.shape
    if axis == 1:
        return O.blur_line(k, x.permute(0, 2, 1).reshape(1, H * C, W, 1)).reshape(H, C, W).permute(0, 2, 1)
    return O.blur_line(k, x.permute(1, 2, 0).reshape(1, W * C, H, 1)).reshape(W, C, H).permute(2, 0, 1)


def _one_pass_adjoint(g, k, axis):
    x = torch.zeros(tuple(g.shape), dtype=torch.float64, requires_grad=True)
    (one_pass(x, k, axis) * g).sum().backward()
    return x.grad.detach()


def cancellation_term(g_abs, taps, axis):
    """E of the module docstring: zero but on texel n - 1 of `axis`, 2 sum_x |g[x]| S_{j_x}"""
    n = g_abs.shape[axis]
    ntaps = taps.numel()
    r = ntaps // 2
    S = torch.cat([torch.zeros(1, dtype=torch.float64), taps.double().abs().cumsum(0)])   # S[j] = sum_{t < j} |k[t]|
    xs = torch.arange(max(n - r, 0), n)
    if xs.numel() == 0:
        return torch.zeros_like(g_abs)
    w = 2.0 * S[torch.clamp(n - xs + r, max=ntaps)]
    shape = [1, 1, 1]
    shape[axis] = xs.numel()
    e = (g_abs.index_select(axis, xs) * w.reshape(shape)).sum(axis)
    E = torch.zeros_like(g_abs)
    E.select(axis, n - 1).copy_(e)
    return E


def magnitude_forward(x, taps):
    return forward_ref(x.double().abs(), taps.abs())


def magnitude_adjoint(g, taps, cancellation=True):
    """cancellation=False: |k|^T on |g| alone, what an exact row holds below 2^24"""
    H, W, _ = g.shape
    ka = taps.double().abs()
    m = g.double().abs()
    for axis, _n in passes(H, W, adjoint=True):
        m = _one_pass_adjoint(m, ka, axis) + (cancellation_term(m, taps, axis) if cancellation else 0.0)
    return m


def exact_kinds(ntaps):
    """(tap kind, data kind) of an integer row: the ranges shrink with the tap count, because the adjoint's border
    texels collect whole folds (texel 0 of a 201-tap line takes up to 100 gradients x 100 taps)"""
    if ntaps <= 9:
        return "int", "int"
    return ("int:2", "int:4") if ntaps <= 65 else ("int:1", "int:2")


# ---------------------------------------------------------------------------------------------------------------------
# criterion
# ---------------------------------------------------------------------------------------------------------------------
def addends(family, ntaps):
    return K_MFMA_ADDENDS if family == MFMA else ntaps


def _gamma(m):
    return m * U / (1.0 - m * U)


def kappa_forward(families, ntaps):
    """families: the kernel family of each pass in execution order -> scalar kappa"""
    f = 1.0
    for fam in families:
        f *= 1.0 + _gamma(addends(fam, ntaps))
    return (f - 1.0) / U


def kappa_adjoint(families, ntaps, H, W):
    """-> fp64 [H, W, 1]: per element, the border texels of each pass carry the fold terms"""
    f = torch.ones(H, W, 1, dtype=torch.float64)
    for fam, (axis, n) in zip(families, passes(H, W, adjoint=True)):
        m = addends(fam, ntaps)
        gm = torch.full((n,), _gamma(m), dtype=torch.float64)
        gm[0] = gm[n - 1] = _gamma(m + ntaps + 2)
        f = f * (1.0 + (gm.reshape(n, 1, 1) if axis == 0 else gm.reshape(1, n, 1)))
    return (f - 1.0) / U


def judge(out, ref, M, kappa):
    """-> (number of elements outside the bound, worst |out - ref| / (2^-24 M), flat index of the worst).  NaN fails."""
    d = (out.detach().cpu().double() - ref).abs()
    bad = ~(d <= kappa * U * M)
    ratio = torch.where(M > 0, d / (U * M).clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")),
                                                                         torch.zeros_like(d)))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    at = int(ratio.reshape(-1).argmax())
    return int(bad.sum()), float(ratio.reshape(-1)[at]), at


def exact_magnitude_ok(M, taps):
    """the precondition of an exact row, from the inputs alone"""
    return bool((M < 2.0 ** 24).all()) and float(taps.double().abs().sum()) < 2.0 ** 24


def exact_mismatches(out, ref):
    """number of elements that differ from the fp64 reference at all (NaN differs)"""
    return int((~(out.detach().cpu().double() == ref)).sum())


# ---------------------------------------------------------------------------------------------------------------------
# dispatch arithmetic of launch_line_batch (jt_blur.hip), restated for the tests that assert which kernel ran
# ---------------------------------------------------------------------------------------------------------------------
K_LINE_Q, K_LINE_P, K_MFMA_TAPS, K_MFMA_K, LDS_LIMIT = 4, 8, 65, 20, 64 * 1024


def mfma_lds_bytes(max_n):
    npos = (max_n + 15) // 16 * 16 + 4 * K_MFMA_K - 16
    return (npos * 16 + K_MFMA_TAPS + 1) * 4


def line_lds_bytes(max_n, max_taps):
    npad = (max_n + K_LINE_P - 1) // K_LINE_P * K_LINE_P + max_taps
    npad += (18 - npad % 16) % 16
    return (K_LINE_Q * npad * 4 + (K_LINE_P + max_taps - 1) * K_LINE_P + max_taps + 1) * 4


def family(max_n, max_taps, batch=False, mfma_on=True, lds_on=True):
    """the kernel one pass runs: max_n / max_taps over all items of the pass"""
    if lds_on:
        if mfma_on and max_taps <= K_MFMA_TAPS and mfma_lds_bytes(max_n) <= LDS_LIMIT:
            return MFMA
        if line_lds_bytes(max_n, max_taps) <= LDS_LIMIT:
            return LINE
    return BATCH if batch else AXIS


def workgroups(fam, max_n, max_taps, total_chunks):
    """grid of the persistent kernels (None for the general ones): min(chunks, 256 * workgroups per CU)"""
    if fam == MFMA:
        return min(total_chunks, 256 * max(1, min(5, 160 * 1024 // (mfma_lds_bytes(max_n) + 512))))
    if fam == LINE:
        return min(total_chunks, 256 * max(1, min(8, 160 * 1024 // (line_lds_bytes(max_n, max_taps) + 512))))
    return None


def chunks(H, W, C, axis):
    return (W if axis == 0 else H) * ((C // 4 + K_LINE_Q - 1) // K_LINE_Q)


# ---------------------------------------------------------------------------------------------------------------------
# guard arena (device)
# ---------------------------------------------------------------------------------------------------------------------
class Arena:
    """Buffers of one row as slices of ONE device allocation, NaN-filled guard bands before, between and after them.  A
    buffer that is not filled by the caller starts as NaN too, so an output element the kernel did not write, or a read
    of an unwritten intermediate, shows as NaN in the output; a write past a buffer shows as a guard that is not NaN."""
    GUARD = 2048   # floats (8 KB; a multiple of 4: every buffer stays 16-byte aligned)

    def __init__(self, sizes, device):
        self.spans = []
        off = self.GUARD
        for s in sizes:
            self.spans.append((off, int(s)))
            off += (int(s) + 3) // 4 * 4 + self.GUARD
        self.buf = torch.full((off,), float("nan"), dtype=torch.float32, device=device)
        self.is_guard = torch.ones(off, dtype=torch.bool, device=device)
        for o, s in self.spans:
            self.is_guard[o:o + s] = False

    def view(self, i, shape=None):
        o, s = self.spans[i]
        v = self.buf[o:o + s]
        return v if shape is None else v.view(*shape)

    def guards_intact(self):
        return bool(torch.isnan(self.buf[self.is_guard]).all())


# ---------------------------------------------------------------------------------------------------------------------
# a NumPy model of one pass with switchable faults (test_blur_ref.py: what the criterion catches, what the old recipe misses)
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("outer_tap_dropped", "taps_reversed", "left_fold_missing", "right_fold_one_tap_late", "zero_padding_forward",
          "last_position_not_written", "last_quad_of_partial_chunk_not_written")


def model_matrix(n, taps, fault=None, adjoint=False):
    """the n x n matrix A (out = A in) the faulty code applies in the forward, or whose transpose it applies in the
    adjoint; fp64"""
    k = np.asarray(taps, dtype=np.float64).copy()
    ntaps = k.size
    r = ntaps // 2
    if fault == "outer_tap_dropped":
        k[ntaps - 1] = 0.0
    if fault == "taps_reversed":
        k = k[::-1].copy()
    A = np.zeros((n, n))
    for u in range(n):
        for t in range(ntaps):
            q = u + t - r
            if q < 0:
                if (fault == "zero_padding_forward" and not adjoint) or (fault == "left_fold_missing" and adjoint):
                    continue
                q = 0
            elif q > n - 1:
                if fault == "zero_padding_forward" and not adjoint:
                    continue
                if fault == "right_fold_one_tap_late" and adjoint and u == n - r:   # the fold's loop over x starts at
                    continue                                                          # n - r + 1: R_{n-r} = k[2 r] is lost
                q = n - 1
            A[u, q] += k[t]
    return A


def model_apply(x, taps, fault=None, adjoint=False, dtype=np.float32):
    """x [H, W, C] -> [H, W, C] with the plane / line pass order, every pass rounded to `dtype` like the kernels' stores"""
    x = np.asarray(x, dtype=np.float64)
    H, W, C = x.shape
    for axis, n in passes(H, W, adjoint):
        A = model_matrix(n, taps, fault, adjoint)
        A = A.T if adjoint else A
        x = np.einsum("uq,qwc->uwc", A, x) if axis == 0 else np.einsum("uq,hqc->huc", A, x)
        if fault == "last_position_not_written":
            if axis == 0:
                x[n - 1] = 0.0
            else:
                x[:, n - 1] = 0.0
        # (a partial chunk BEHIND full ones, as the five quads of a 20-channel factor: C = 4, 8, 12 are one chunk)
        if fault == "last_quad_of_partial_chunk_not_written" and C // 4 > K_LINE_Q and (C // 4) % K_LINE_Q:
            x[:, :, C - 4:] = 0.0
        x = x.astype(dtype).astype(np.float64)
    return x
