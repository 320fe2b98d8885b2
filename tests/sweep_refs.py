"""References, camera geometries and shapes of the plane-sweep edge tests (test_gpu_sweep_edges.py; test_sweep_refs.py runs every reference
and every geometry's situation without a GPU).

The plane sweep and its two backward kernels give a source view whose sample coordinate is NOT FINITE (ix = ((gx + 1) / 2) (W - 1) or iy
is inf or NaN in fp32: p2 == 0, or a projection that overflows) ZERO bilinear weights: the view contributes nothing to the voxel and is not
counted.  The CPU reference (ATen's grid_sample) returns NaN there, and so does the stand-alone homo_warp kernel.  `costvar_zero_tap` is the
oracle's build_volume_costvar[_img] with exactly that one change, bit for bit everywhere else; `costvar_f64` the differentiable float64
restatement the backward kernels are held to.  Everything here is CPU-only and deterministic."""
import functools

import torch
import torch.nn.functional as F

from oracle import mvsnerf_oracle as O

C = 32
U = 2.0 ** -24

# ------------------------------------------------------------------------------------------------------------------ shapes and geometries
SHAPES = [(2, 2, 0, 1),       # the smallest shape the entries accept
          (2, 3, 0, 5),
          (3, 2, 1, 3),       # Hp = 5: three of the eight row bands are empty
          (6, 7, 1, 5),
          (9, 17, 2, 6),      # Hp = 13: two rows per band, a short last band and an empty one
          (5, 40, 0, 4)]      # several 16-column chunks per band
# the backward walks 16 planes per geometry batch: D = 17, 33 cross it and are no multiple of it
BWD_SHAPES = [(2, 2, 0, 1), (3, 2, 1, 3), (6, 7, 1, 5), (9, 17, 2, 6), (5, 40, 0, 4), (6, 7, 1, 17), (5, 11, 1, 33)]


def depths(D):
    return torch.linspace(0.5, 8.0, D)


def _P(rows, T):
    return torch.tensor([list(r) + [t] for r, t in zip(rows, T)], dtype=torch.float32)


_I = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))


def _sign_change(H, W):
    # p2 = u - (W - 1) / 2 - 1/4 + 0.1 / depth: never 0 at an integer u (|p2| >= 0.05), negative on the left half of every row
    return _P(((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0, 0.0, -(W - 1) / 2.0 - 0.25)), (0.0, 0.0, 0.1))


# name -> (matrix of (H, W), the situations it exists for: keys of `situations`)
GEOMETRIES = {
    "identity": (lambda H, W: _P(_I, (0.0, 0.0, 0.0)), ("on_pixel", "on_mask_border")),
    "negated": (lambda H, W: -_P(_I, (0.0, 0.0, 0.0)), ("behind_with_taps",)),
    "half": (lambda H, W: _P(((1.0, 0.0, 0.5), (0.0, 1.0, 0.25), (0.0, 0.0, 1.0)), (0.0, 0.0, 0.0)), ("one_tap", "two_taps")),
    "half_neg": (lambda H, W: _P(((1.0, 0.0, -0.5), (0.0, 1.0, -0.25), (0.0, 0.0, 1.0)), (0.0, 0.0, 0.0)), ("one_tap", "two_taps")),
    "sign_change": (_sign_change, ("p2_both_signs",)),
    "p2_zero": (lambda H, W: _P(((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)), (0.0, 0.0, 0.0)), ("inf", "nan")),
    "far13": (lambda H, W: _P(_I, (1.0e13, -1.0e13, 0.0)), ("beyond_int",)),
    "far30": (lambda H, W: _P(_I, (-1.0e30, 1.0e30, 0.0)), ("beyond_int",)),
    "far_inf": (lambda H, W: _P(_I, (3.0e38, -3.0e38, 0.0)), ("inf",)),           # T / 0.5 overflows fp32
    "fast": (lambda H, W: _P(_I, (30.0, -20.0, 0.0)), ("tap_set_moves",)),
    # the same sweep scaled to the image: outside at depth 0.5, inside at depth 8, so every column crosses the image border
    "fast_fit": (lambda H, W: _P(_I, (0.5 * W, -0.5 * H, 0.0)), ("tap_set_crosses",)),
}
# the geometries that need more than one plane, or an image the fixed 30 / -20 px sweep can reach, are paired with the shapes that have them
PAIRED = {"fast": [(9, 17, 2, 6), (5, 40, 0, 4)],
          "fast_fit": [s for s in SHAPES if s[3] > 1]}


def paired_shapes(name):
    return PAIRED.get(name, SHAPES)


def proj_stack(names, H, W):
    """(1 + len(names), 3, 4): the reference view (its matrix is never read: identity) and one source view per name."""
    return torch.stack([GEOMETRIES["identity"][0](H, W)] + [GEOMETRIES[n][0](H, W) for n in names])


MIXED = {4: ("half", "p2_zero", "fast_fit"),
         8: ("negated", "half_neg", "sign_change", "p2_zero", "far13", "far_inf", "fast_fit")}
BWD_CORE = ("half", "fast_fit", "p2_zero", "sign_change", "half_neg", "negated", "fast")
BWD_FAR = ("far30", "far_inf", "far13")
BWD_START = (0, 2, 3, 4, 5, 1, 6)        # per backward shape; the two deep shapes start on the views whose taps move from plane to plane


def forward_cases(shape):
    """[(case name, source-view names)]: V = 1, every geometry alone (V = 2) where it is paired with the shape, and the mixed V = 4 and 8."""
    cases = [("V1", ())]
    cases += [(n, (n,)) for n in GEOMETRIES if shape in paired_shapes(n)]
    cases += [(f"mixed{V}", names) for V, names in MIXED.items()]
    return cases


def bwd_views(V, shape_index):
    """The V - 1 source views of a backward case: BWD_CORE rotated per shape, so that a small V meets another geometry at every shape, with one
    out-of-range view in fourth place (it receives no gradient at all: V >= 5 has it)."""
    k = BWD_START[shape_index]
    rot = BWD_CORE[k:] + BWD_CORE[:k]
    return (rot[:3] + (BWD_FAR[shape_index % 3],) + rot[3:])[:V - 1]


def make_inputs(V, H, W, seed):
    """feats (V, 32, H, W) with |f| <= 6 (the two-piece fp16 store cannot saturate), thumbnails (V, 3, H, W) in [0, 1)."""
    g = torch.Generator().manual_seed(seed)
    feats = (torch.randn((V, C, H, W), generator=g) * 2.0).clamp_(-6.0, 6.0)
    return feats, torch.rand((V, 3, H, W), generator=g)


# ------------------------------------------------------------------------------------------------------------------ fp32 chain
def grid_of(P_v, dv, H, W, pad):
    """The pinned fp32 sampling grid of one source view: (gx, gy), each (D, Hp, Wp)."""
    dummy = torch.zeros((1, 1, H, W))
    _, grid = O.homo_warp(dummy, P_v[None], dv[None], pad=pad)
    g = grid.view(dv.shape[0], H + 2 * pad, W + 2 * pad, 2)
    return g[..., 0], g[..., 1]


def chain(g, size):
    """grid_sample's un-normalisation (align_corners=True) as the kernels form it, in the dtype of g."""
    return ((g + 1.0) / 2.0) * float(size - 1)


def nonfinite(gx, gy, H, W):
    return ~(torch.isfinite(chain(gx, W)) & torch.isfinite(chain(gy, H)))


def inside(gx, gy):
    return (gx > -1.0) & (gx < 1.0) & (gy > -1.0) & (gy < 1.0)


def taps(gx, gy, H, W):
    """The four taps in the kernels' order nw, ne, sw, se: [(in-image (bool), clamped pixel index (long))], and `any`; NaN-safe.  The index is what
    the sweep kernels gather from: clamped into the image where any tap is inside, 0 otherwise."""
    ix, iy = chain(gx, W), chain(gy, H)
    fx, fy = ix.floor(), iy.floor()
    x_in = [(fx + k >= 0) & (fx + k <= W - 1) for k in (0.0, 1.0)]
    y_in = [(fy + k >= 0) & (fy + k <= H - 1) for k in (0.0, 1.0)]
    any_ = (x_in[0] | x_in[1]) & (y_in[0] | y_in[1])
    sx = torch.where(any_, fx, torch.zeros_like(fx)).long()
    sy = torch.where(any_, fy, torch.zeros_like(fy)).long()
    out = []
    for yc in (0, 1):
        for xc in (0, 1):
            idx = (sy + yc).clamp(0, H - 1) * W + (sx + xc).clamp(0, W - 1)
            out.append((x_in[xc] & y_in[yc], torch.where(any_, idx, torch.zeros_like(idx))))
    return out, any_


def situations(P_v, dv, H, W, pad):
    """How many voxels (columns for the last two) of one source view are in each situation the geometries exist for."""
    D, Hp, Wp = dv.shape[0], H + 2 * pad, W + 2 * pad
    gx, gy = grid_of(P_v, dv, H, W, pad)
    ys, xs = torch.meshgrid(torch.arange(Hp, dtype=torch.float32) - pad, torch.arange(Wp, dtype=torch.float32) - pad, indexing="ij")
    uv1 = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(Hp * Wp)], 0)[None]
    p2 = (O._sgemm_k3(P_v[None, :, :3], uv1)[0, 2][None] + (P_v[2, 3] / dv)[:, None]).view(D, Hp, Wp)
    ix, iy = chain(gx, W), chain(gy, H)
    nf = nonfinite(gx, gy, H, W)
    tp, any_ = taps(gx, gy, H, W)
    n_in = sum(ok.long() for ok, _ in tp) * (~nf)
    tapset = torch.stack([i for _, i in tp], -1)                                  # (D, Hp, Wp, 4)
    differs = (tapset[1:] != tapset[:-1]).any(-1)                                 # between consecutive planes of a column
    return {
        "on_pixel": int(((ix == ix.floor()) & (iy == iy.floor()) & (n_in > 0)).sum()),
        "on_mask_border": int((((gx.abs() == 1.0) | (gy.abs() == 1.0)) & ~nf).sum()),
        "behind_with_taps": int(((p2 < 0) & (n_in > 0)).sum()),
        "behind_inside": int(((p2 < 0) & inside(gx, gy)).sum()),
        "one_tap": int((n_in == 1).sum()),
        "two_taps": int((n_in == 2).sum()),
        "p2_both_signs": int(min((p2 < 0).sum(), (p2 > 0).sum())) if not bool(nf.any()) else 0,
        "inf": int((torch.isinf(ix) | torch.isinf(iy)).sum()),
        "nan": int((torch.isnan(ix) | torch.isnan(iy)).sum()),
        "nonfinite": int(nf.sum()),
        "beyond_int": int((~nf & ((ix.abs() > 2.0 ** 31) | (iy.abs() > 2.0 ** 31))).sum()),
        "tap_set_moves": int((differs & any_[1:] & any_[:-1]).sum()),
        "tap_set_crosses": int((differs & (any_[1:] != any_[:-1])).sum()),
    }


def hand_grid(H, W, pad, D):
    """A sampling grid (1, D, Wp, Hp, 2) filled by hand: every pair of the special values below first, random coordinates in [-1.3, 1.3) after."""
    one = torch.tensor(1.0)
    sp = torch.stack([one, -one, torch.nextafter(one, 2 * one), torch.nextafter(-one, -2 * one), torch.nextafter(one, 0 * one), 0 * one,
                      1.0e30 * one, -1.0e30 * one, one / 0, -one / 0, one * float("nan")])
    pairs = torch.cartesian_prod(sp, sp)
    n = D * (H + 2 * pad) * (W + 2 * pad)
    assert n > pairs.shape[0]
    g = torch.rand((n, 2), generator=torch.Generator().manual_seed(n)) * 2.6 - 1.3
    g[:pairs.shape[0]] = pairs
    return g.view(1, D, W + 2 * pad, H + 2 * pad, 2)


HAND_GRID_SHAPE = (5, 6, 1, 3)


# ------------------------------------------------------------------------------------------------------------------ references
def costvar_zero_tap(feats, P, dv, pad, imgs_small=None):
    """The oracle's build_volume_costvar (imgs_small None) / build_volume_costvar_img arithmetic, `warped` := 0 and the view not counted
    wherever the fp32 sample coordinate is not finite.  feats (V, 32, H, W), P (V, 3, 4), dv (D,), imgs_small (V, 3, H, W) = the thumbnails
    themselves (no resize).  Returns cost (n_ch, D, Hp, Wp) [ref rgb | warped src rgb .. | variance], masks (V, D, Hp, Wp) with thumbnails
    or the view count (D, Hp, Wp) without, and the zeroed voxels (V, D, Hp, Wp) bool.  s + 0 and s2 + 0^2 are exact: an fp32 reference on
    every voxel."""
    V, _, H, W = feats.shape
    D, Hp, Wp = dv.shape[0], H + 2 * pad, W + 2 * pad
    ref = F.pad(feats[0], (pad, pad, pad, pad)).unsqueeze(1).expand(-1, D, -1, -1)
    s, s2 = ref.clone(), ref ** 2
    masks = torch.ones(V, D, Hp, Wp)
    zeroed = torch.zeros(V, D, Hp, Wp, dtype=torch.bool)
    rgb = []
    if imgs_small is not None:
        r0 = torch.zeros(3, D, Hp, Wp)
        r0[:, :, pad:H + pad, pad:W + pad] = imgs_small[0].unsqueeze(1)
        rgb.append(r0)
    for v in range(1, V):
        warped, grid = O.homo_warp(feats[None, v], P[None, v], dv[None], pad=pad)
        g = grid.view(D, Hp, Wp, 2)
        nf = nonfinite(g[..., 0], g[..., 1], H, W)
        zeroed[v] = nf
        warped = torch.where(nf[None], torch.zeros(()), warped[0])
        if imgs_small is not None:
            th, _ = O.homo_warp(imgs_small[None, v], P[None, v], dv[None], src_grid=grid, pad=pad)
            rgb.append(torch.where(nf[None], torch.zeros(()), th[0]))
        masks[v] = inside(g[..., 0], g[..., 1]).float()
        s, s2 = s + warped, s2 + warped ** 2
    cnt = masks.sum(0)
    inv = 1.0 / cnt
    var = s2 * inv - (s * inv) ** 2
    if imgs_small is None:
        return var, cnt, zeroed
    return torch.cat(rgb + [var]), masks, zeroed


def costvar_f64(feats, P, dv, pad):
    """Differentiable float64 restatement: feats (V, 32, H, W) float64 (may require grad).  The sample coordinates are the fp32 chain on the
    fp32 grid of O.homo_warp; a tap counts iff its pixel is inside the image, a non-finite coordinate has no tap; the view counts are the
    strict inequalities on the fp32 grid; weights, sums and the variance in float64.  Returns var (32, D, Hp, Wp), count (D, Hp, Wp),
    E[x^2] + mean^2 (the scale of the variance's cancellation), and the same with every warped value replaced by its blend of |tap|s (the
    scale of the fp32 blend's own cancellation: four taps of size 3 can blend to 1e-3)."""
    V, _, H, W = feats.shape
    D, Hp, Wp = dv.shape[0], H + 2 * pad, W + 2 * pad
    P32, dv32 = P.float(), dv.float()
    ref = F.pad(feats[0], (pad, pad, pad, pad)).unsqueeze(1).expand(-1, D, -1, -1)
    s, s2 = ref, ref ** 2
    sa, sa2 = ref.detach().abs(), ref.detach() ** 2
    cnt = torch.ones(D, Hp, Wp, dtype=torch.float64)
    for v in range(1, V):
        gx, gy = grid_of(P32[v], dv32, H, W, pad)
        nf = nonfinite(gx, gy, H, W)
        ix = torch.where(nf, torch.zeros(()), chain(gx, W)).double()
        iy = torch.where(nf, torch.zeros(()), chain(gy, H)).double()
        wx1, wy1 = ix - ix.floor(), iy - iy.floor()
        tp, _ = taps(gx, gy, H, W)
        fv = feats[v].reshape(C, H * W)
        warped, wabs = 0.0, 0.0
        for (ok, idx), w in zip(tp, ((1 - wx1) * (1 - wy1), wx1 * (1 - wy1), (1 - wx1) * wy1, wx1 * wy1)):
            t = fv[:, idx.reshape(-1)].view(C, D, Hp, Wp) * (w * (ok & ~nf).double())
            warped, wabs = warped + t, wabs + t.detach().abs()
        cnt = cnt + inside(gx, gy).double()
        s, s2 = s + warped, s2 + warped ** 2
        sa, sa2 = sa + wabs, sa2 + wabs ** 2
    ex2, mean = s2 / cnt, s / cnt
    return ex2 - mean ** 2, cnt, ex2 + mean ** 2, sa2 / cnt + (sa / cnt) ** 2


def resize_f64(src, Ho, Wo):
    """F.interpolate(bilinear, align_corners=False) of src (..., Hi, Wi) fp32: source coordinates and weights in fp32 exactly as the kernels
    form them (scale (float)Hi / (float)Ho, f = fma(scale, o + 0.5, -0.5) in one rounding, clamp at 0, l = f - floor, h = 1 - l), the blend in
    float64."""
    Hi, Wi = src.shape[-2:]

    def axis(n_in, n_out):
        sc = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
        # the product of two fp32 numbers and its distance to 0.5 are exact in float64: one rounding, like the kernels' fmaf
        f = (sc.double() * (torch.arange(n_out, dtype=torch.float32) + 0.5).double() - 0.5).float().clamp_(min=0.0)
        i0 = f.floor()
        lo = f - i0
        hi = 1.0 - lo
        i0 = i0.long()
        return i0, i0 + (i0 < n_in - 1).long(), lo.double(), hi.double()
    y0, y1, ly, hy = axis(Hi, Ho)
    x0, x1, lx, hx = axis(Wi, Wo)
    s = src.double()
    top = s[..., y0, :][..., x0] * hx + s[..., y0, :][..., x1] * lx
    bot = s[..., y1, :][..., x0] * hx + s[..., y1, :][..., x1] * lx
    return top * hy[:, None] + bot * ly[:, None]


# ------------------------------------------------------------------------------------------------------------------ shared cases
@functools.lru_cache(maxsize=None)
def forward_case(shape, names, with_img):
    """Inputs and the zero-tap reference of one forward case, computed once and shared (read-only) by the tests that need it."""
    H, W, pad, D = shape
    V = 1 + len(names)
    feats, small = make_inputs(V, H, W, seed=1000 * H + 10 * W + V)
    P, dv = proj_stack(names, H, W), depths(D)
    cost, masks, zeroed = costvar_zero_tap(feats, P, dv, pad, small if with_img else None)
    return {"feats": feats, "small": small, "P": P, "dv": dv, "cost": cost, "masks": masks, "zeroed": zeroed}
