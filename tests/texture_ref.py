"""The contract of csrc/jt_texture.hip and of jt_raster_resolve_texture (include/jt_render.h: "Texture atlas") in NumPy: the atlas
layout, the texel positions and directions in the kernel's own fp32 / fp64 operations (every one rounded on its own, which IEEE
754 defines to the bit), the quantising pack, the chart corners, and the bilinear sample in fp64 from the rasteriser reference's
integer edge values (tests/raster_ref.py)."""
import math

import numpy as np

from tests import raster_ref as R

MIN_BLOCK, MAX_BLOCK, MAX_SIDE = 4, 64, 16384


def layout(nt, S):
    """dict(S, L, nt, n_blocks, cols, rows, W, H, n_entries) as section "Texture atlas" defines them"""
    n_blocks = -(-nt // 2)
    cols = 1
    while cols * cols < n_blocks:
        cols += 1
    rows = -(-n_blocks // cols)
    return dict(S=S, L=S - 3, nt=nt, n_blocks=n_blocks, cols=cols, rows=rows, W=cols * S, H=rows * S, n_entries=n_blocks * S * S)


def entries(lay, start=0, count=None):
    """for the entries [start, start + count): (block, i, j, triangle id, chart i, chart j), int64 arrays"""
    S = lay["S"]
    e = np.arange(start, lay["n_entries"] if count is None else start + count, dtype=np.int64)
    b, r = e // (S * S), e % (S * S)
    j, i = r // S, r % S
    lower = i + j <= S - 1
    return b, i, j, 2 * b + np.where(lower, 0, 1), np.where(lower, i, S - 1 - i), np.where(lower, j, S - 1 - j)


def pixels(lay, start=0, count=None):
    """(column, row) of the atlas pixel of every entry"""
    b, i, j = entries(lay, start, count)[:3]
    return (b % lay["cols"]) * lay["S"] + i, (b // lay["cols"]) * lay["S"] + j


def uv(lay):
    """chart corners [nt, 3, 2] float64 in atlas pixel units, x right and y down"""
    S, L = lay["S"], lay["L"]
    out = np.empty((lay["nt"], 3, 2))
    for t in range(lay["nt"]):
        b = t // 2
        bx, by = b % lay["cols"], b // lay["cols"]
        if t % 2 == 0:
            p0 = np.array([bx * S + 0.5, by * S + 0.5])
            out[t] = [p0, p0 + (L, 0), p0 + (0, L)]
        else:
            p0 = np.array([(bx + 1) * S - 0.5, (by + 1) * S - 0.5])
            out[t] = [p0, p0 - (L, 0), p0 - (0, L)]
    return out


def _lerp2(x0, x1, x2, a, b):
    """(x0 + a (x1 - x0)) + b (x2 - x0) in fp32, one rounding per operation ([n, 3] rows, a and b [n, 1])"""
    f = np.float32
    e1 = (x1 - x0).astype(f)
    e2 = (x2 - x0).astype(f)
    p = (x0 + (a * e1).astype(f)).astype(f)
    return (p + (b * e2).astype(f)).astype(f)


def texels(V, N, T, lay, start=0, count=None):
    """(xyz [count, 3] float32, dirs [count, 3] float32, valid [count] uint8) of jt_texture_texels"""
    V, N = np.asarray(V, dtype=np.float32), np.asarray(N, dtype=np.float32)
    T = np.asarray(T, dtype=np.int64)
    nv, nt = len(V), len(T)
    _, _, _, tri, ci, cj = entries(lay, start, count)
    n = len(tri)
    ok = tri < nt
    ids = T[np.where(ok, tri, 0)]
    ok &= ((ids >= 0) & (ids < nv)).all(-1)
    ids = np.where(ok[:, None], ids, 0)
    L = np.float32(lay["L"])
    a = (ci.astype(np.float32) / L).astype(np.float32)[:, None]
    b = (cj.astype(np.float32) / L).astype(np.float32)[:, None]
    with np.errstate(all="ignore"):
        p = _lerp2(V[ids[:, 0]], V[ids[:, 1]], V[ids[:, 2]], a, b)
        m = _lerp2(N[ids[:, 0]], N[ids[:, 1]], N[ids[:, 2]], a, b).astype(np.float64)
        length = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        unit = np.isfinite(length) & (length > 0)
        d = ((-m) / np.where(unit, length, 1.0)[:, None]).astype(np.float32)
    fallback = np.array([0.0, 0.0, -1.0], dtype=np.float32)
    d = np.where((ok & unit)[:, None], d, fallback)
    p = np.where(ok[:, None], p, np.float32(0))
    assert p.shape == (n, 3) and p.dtype == np.float32 and d.dtype == np.float32
    return p, d, ok.astype(np.uint8)


def quantise(rgb):
    """floor(255 c + 0.5) clamped to 0 .. 255 in fp64, 0 for a NaN (mesh_io.quantise_colors refuses a NaN; the atlas takes it)"""
    c = np.asarray(rgb, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        v = np.floor(255.0 * c + 0.5)
    return np.where(np.isnan(v), 0.0, np.clip(v, 0.0, 255.0)).astype(np.uint8)


def pack(rgb, valid, lay, start=0, atlas=None):
    """jt_texture_pack into atlas [H, W, 3] uint8 (a zeroed one when not given); returns the atlas"""
    if atlas is None:
        atlas = np.zeros((lay["H"], lay["W"], 3), dtype=np.uint8)
    px, py = pixels(lay, start, len(rgb))
    keep = np.asarray(valid).astype(bool)
    atlas[py[keep], px[keep]] = quantise(rgb)[keep]
    return atlas


def footprint(S, a, b):
    """The chart coordinates (i, j) of the texels that carry non-zero weight when a viewer samples bilinearly, over texel
    centres, at the point of barycentrics (a, b) -- Fractions -- of a chart: the point is (a L + 0.5, b L + 0.5) in the chart's
    pixel units, texel (i, j) has its centre at (i + 0.5, j + 0.5)."""
    L = S - 3
    x, y = a * L, b * L                                         # in units of texels from the centre of texel (0, 0)
    out = []
    for k, fk in ((math.floor(x), 1 - (x - math.floor(x))), (math.floor(x) + 1, x - math.floor(x))):
        for m, fm in ((math.floor(y), 1 - (y - math.floor(y))), (math.floor(y) + 1, y - math.floor(y))):
            if fk * fm != 0:
                out.append((k, m))
    return out


def sample(screen, triangles, H, W, atlas, lay, background=0.0, cull=False):
    """One view of jt_raster_resolve_texture in fp64: the rasteriser reference's dict plus out [H, W, 3] -- at a pixel whose winner
    is t, chart t & 1 of block t >> 1 sampled bilinearly at (l1 L, l2 L), l the perspective-correct weights from the integer edge
    values, the four texels clamped into the block and fetched as byte / 255."""
    ref = R.rasterize(screen, triangles, H, W, cull=cull)
    X, Y, _ = R.snap(np.asarray(screen))
    q = np.asarray(screen)[:, 2].astype(np.float64)
    S, L, cols = lay["S"], lay["L"], lay["cols"]
    tex = atlas.astype(np.float64) / 255.0
    out = np.empty((H, W, 3))
    out[:] = np.broadcast_to(np.asarray(background, dtype=np.float64), (3,))
    for py, px in zip(*np.nonzero(ref["tri"] >= 0)):
        t = int(ref["tri"][py, px])
        tri = [int(k) for k in triangles[t]]
        b = R.edge_values(X, Y, tri, px, py)[0]
        w = [float(b[k]) * q[tri[k]] for k in range(3)]
        den = w[0] + w[1] + w[2]
        s, u = w[1] / den * L, w[2] / den * L
        i0, j0 = min(max(math.floor(s), 0), S - 2), min(max(math.floor(u), 0), S - 2)
        fx, fy = s - i0, u - j0
        x0, y0 = ((t >> 1) % cols) * S, ((t >> 1) // cols) * S

        def texel(i, j):
            return tex[y0 + (S - 1 - j if t & 1 else j), x0 + (S - 1 - i if t & 1 else i)]
        top = texel(i0, j0) + fx * (texel(i0 + 1, j0) - texel(i0, j0))
        bot = texel(i0, j0 + 1) + fx * (texel(i0 + 1, j0 + 1) - texel(i0, j0 + 1))
        out[py, px] = top + fy * (bot - top)
    ref["out"] = out
    return ref


def soup(nt, seed, nv=None):
    """a random triangle soup: (V [nv, 3] float32, N [nv, 3] float32 unnormalised normals, T [nt, 3] int32)"""
    g = np.random.default_rng(seed)
    nv = nv or max(3, (3 * nt) // 2)
    V = g.uniform(-1, 1, size=(nv, 3)).astype(np.float32)
    N = g.normal(size=(nv, 3)).astype(np.float32)
    T = np.stack([g.permutation(nv)[:3] for _ in range(nt)]).astype(np.int32)
    return V, N, T
