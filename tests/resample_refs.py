"""Plain-numpy restatement of Pillow's 8-bit resampler, `Image.resize(size, LANCZOS | BILINEAR)` without `box` or `reducing_gap` (Pillow's
src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc; Convert.c: rgbA2rgba and
rgba2rgbA around it for an image with alpha), and of csrc/resample.hip, which is held to these bytes.  No Pillow import: tests/golden/caseG_resample.npz
holds Pillow's own outputs for CASES (tests/gen_golden_resample.py) and tests/test_resample_refs.py pins this file to them."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caseG_resample.npz")
PRECISION_BITS = 22
FILTERS = ("lanczos", "bilinear")
SUPPORT = {"lanczos": 3.0, "bilinear": 1.0}
ALPHAS = (0, 255, 1, 7, 128, 200, 254)           # the copy branch of the unpremultiply (0, 255), the clamp at 255, small and large divisors
# (h, w) -> (H', W'): the six shapes checked against Pillow when the arithmetic was written down; a factor-4.2 window (ksize 27); rows and columns
# that cross a 256-thread block, both ways; the copy
CASES = (((37, 53), (12, 16)), ((24, 40), (9, 40)), ((50, 31), (50, 11)), ((12, 16), (23, 29)), ((64, 48), (16, 20)), ((7, 9), (2, 3)),
         ((20, 126), (20, 30)), ((5, 1100), (3, 300)), ((1100, 5), (300, 3)), ((9, 9), (9, 9)))


def pillow_order_differs(hw, out_hw):
    """Pillow 12's Image.resize runs the vertical pass first, as a resize of its own, for an image more than 100 times as tall as wide whose height
    shrinks (Image.py: `self.size[1] > self.size[0] * 100 and size[1] < self.size[1]`); earlier versions and csrc/resample.hip run the horizontal pass
    first for every shape.  Of CASES only (1100, 5) -> (300, 3) is such an image: it is held to this file, not to Pillow."""
    return hw[0] > hw[1] * 100 and out_hw[0] < hw[0]


GOLDEN_CASES = tuple(c for c in CASES if not pillow_order_differs(*c))


def case_name(hw, out_hw, channels):
    return f"{hw[0]}x{hw[1]}_{out_hw[0]}x{out_hw[1]}_c{channels}"


def case_image(hw, channels, seed=0):
    """The input of a case: random bytes; with alpha, every ALPHAS value in runs of random length, so that windows mix them."""
    g = np.random.default_rng([seed, hw[0], hw[1], channels])
    img = g.integers(0, 256, (hw[0], hw[1], channels), dtype=np.uint8)
    if channels == 4:
        a = np.repeat(g.choice(np.array(ALPHAS, dtype=np.uint8), hw[0] * hw[1]), g.integers(1, 6, hw[0] * hw[1]))[:hw[0] * hw[1]]
        img[..., 3] = a.reshape(hw)
    return img


def _filter(name, x):
    if name == "lanczos":
        if -3.0 <= x < 3.0:
            def sinc(v):
                if v == 0.0:
                    return 1.0
                v = v * math.pi
                return math.sin(v) / v
            return sinc(x) * sinc(x / 3)
        return 0.0
    x = -x if x < 0.0 else x
    return 1.0 - x if x < 1.0 else 0.0


def tables(n_in, n_out, name):
    """-> (win (n_out,2) int32 = (xmin, n), kk (n_out,ksize) int32, ksize): the windows and fixed-point coefficients of one axis."""
    if name not in FILTERS:
        raise ValueError(name)
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[name] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    win, kk = np.zeros((n_out, 2), dtype=np.int32), np.zeros((n_out, ksize), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = [_filter(name, (x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        win[xx] = xmin, n
        kk[xx, :n] = [int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5) for v in w]
    return win, kk, ksize


def _pass(src, win, kk, axis):
    """One pass along `axis` of src (H,W,C) uint8: clamp((2^21 + sum src * kk) >> 22, 0, 255) per channel, int32 as Pillow's accumulator is."""
    src = np.moveaxis(src, axis, 0).astype(np.int64)
    out = np.empty((win.shape[0],) + src.shape[1:], dtype=np.uint8)
    for xx in range(win.shape[0]):
        xmin, n = int(win[xx, 0]), int(win[xx, 1])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(kk[xx, :n].astype(np.int64), src[xmin:xmin + n], 1)
        assert np.abs(acc).max() < 2 ** 31
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def premultiply(img):
    """rgbA2rgba: c' = ((t >> 8) + t) >> 8 with t = c * a + 128; alpha unchanged."""
    out = img.copy()
    t = img[..., :3].astype(np.int32) * img[..., 3:].astype(np.int32) + 128
    out[..., :3] = ((t >> 8) + t) >> 8
    return out


def unpremultiply(img):
    """rgba2rgbA: c = c' when a is 0 or 255, else min(255 * c' // a, 255)."""
    out = img.copy()
    a = img[..., 3:].astype(np.int32)
    q = np.minimum(255 * img[..., :3].astype(np.int32) // np.maximum(a, 1), 255)
    out[..., :3] = np.where((a == 0) | (a == 255), img[..., :3], q)
    return out


def resize(img, out_hw, name):
    """img (H,W,3|4) uint8 -> (H',W',same): Image.fromarray(img).resize((W', H'), name).  Horizontal pass first, each only if its size changes."""
    H, W, C = img.shape
    Ho, Wo = out_hw
    if (Ho, Wo) == (H, W):
        return img.copy()
    x = premultiply(img) if C == 4 else img
    if Wo != W:
        win, kk, _ = tables(W, Wo, name)
        x = _pass(x, win, kk, 1)
    if Ho != H:
        win, kk, _ = tables(H, Ho, name)
        x = _pass(x, win, kk, 0)
    return unpremultiply(x) if C == 4 else x


def to_bank(img):
    """(…,H,W,3|4) -> (…,H,W,4): the bank's layout, alpha 255 for three channels."""
    if img.shape[-1] == 4:
        return img
    return np.concatenate((img, np.full(img.shape[:-1] + (1,), 255, dtype=np.uint8)), -1)


def golden():
    return {k: v for k, v in np.load(GOLDEN).items()}
