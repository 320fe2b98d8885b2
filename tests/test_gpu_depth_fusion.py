"""GPU: the depth-fusion kernels (csrc/depth_fusion.hip) against the float64 restatement of their definition (tests/depth_fusion_refs.py).

A threshold test cannot be compared bit for bit: a pair whose reprojection error lies within single-precision noise of pix_thr may fall on either side.
The seen bits are therefore compared on DECIDED pairs (depth_fusion_refs.decided): in float64 |err - pix_thr| > m_px and |rel - rel_thr| > m_rel, and
(u, v) further than m_px from the image border and from an integer grid line whose crossing changes the validity of the taps.  The margins are measured,
not assumed: m_px = 8 x the largest |err32 - err64|, |u32 - u64| or |v32 - v64| and m_rel = 8 x the largest |rel32 - rel64| that the float32 run of the
restatement shows against its float64 run on the very rig under test (the factor covers the contraction and operation-order freedom the kernel has and
numpy has not).  The fixture measures them again on every run; on the rigs below it finds (corrupted depths, every ordered pair of views)

    rig                     |err32-err64|   |uv32-uv64|   |rel32-rel64|   ->  m_px      m_rel     undecided / inside pairs
    24 x 40                 2.9e-05 px      7.7e-06 px    1.9e-06             2.4e-04   1.5e-05   0.024 %
    24 x 40, look-at        3.1e-05 px      8.7e-06 px    1.3e-06             2.5e-04   1.1e-05   0.000 %
    97 x 131                2.9e-04 px      3.0e-05 px    4.1e-06             2.3e-03   3.3e-05   0.018 %

and the test asserts that undecided pairs are at most 1 % of the inside pairs.  Fused depth, on pixels all of whose pairs are decided: relative tolerance
4 x the largest relative |fused32 - fused64| of the restatement (24 x 40: 4 x 2.1e-07; look-at: 4 x 2.9e-07; 97 x 131: 4 x 1.1e-06).  Points: absolute
tolerance 4 x the largest |o + d fused| difference between the float32 and the float64 restatement on the same fused depths (97 x 131: 4 x 5.3e-05 of
coordinates up to 800).  The 2 x 2 rig has a dozen pairs, too few to measure a noise floor on: it takes the 24 x 40 rig's figures (the same world, a
twentieth of the focal length, so its pixel noise is smaller and its relative noise the same).  On an MI355X the kernels' own figures were 2.9e-07,
2.9e-07 and 1.1e-06 relative on fused and 3.6e-05 on points.
"""
import numpy as np
import pytest
import torch

import depth_fusion_refs as R
from mvsnerf_amd import _lib, geometry, ops
from mvsnerf_amd.rays import SceneRays

pytestmark = pytest.mark.gpu
DEV = "cuda"
PIX, REL = 1.0, 0.01


def _corrupt(g):
    """float32 depths of a rig with a 1.03-scaled block, holes of every kind, a valid mask and an RGBA bank with an alpha-0 region"""
    M, H, W = g["depth"].shape
    d = g["depth"].astype(np.float32)
    d[2 % M, H // 4:H // 4 + H // 3, W // 5:W // 5 + W // 3] *= np.float32(1.03)
    v = 1 % M
    for k, hole in enumerate((0.0, -1.0, np.nan, np.inf, -np.inf)):
        y, x = (3 + 4 * k) % (H - 1), (5 + 7 * k) % (W - 1)
        d[v, y:y + 2, x:x + 2] = hole
        d[(v + 2) % M, (y + 2) % H, (x + 3) % W] = hole
    valid = np.ones((M, H, W), np.uint8)
    valid[3 % M, H // 2:H // 2 + 3, W // 2 - 2:W // 2 + 4] = 0
    valid[3 % M, 1, 1] = 7                                   # any non-zero byte is valid
    alpha = np.full((M, H, W), 255, np.uint8)
    alpha[0, :H // 3, W // 2:W // 2 + W // 4] = 0
    alpha[0, H - 2, 2] = 1                                   # alpha > 0 is foreground
    return d, valid, np.concatenate([g["images"], alpha[..., None]], -1)


class Case:
    """A rig on the device and its float64 / float32 restatements, with the measured margins."""

    def __init__(self, H, W, M=5, look_at=False, corrupt=True, g=None, like=None):
        self.like = like                                     # a Case whose noise figures are a floor for this one's (a rig too small to measure on)
        g = self.g = R.make_rig(H, W, M, look_at) if g is None else g
        M = self.M = g["depth"].shape[0]
        self.H, self.W = H, W
        if corrupt:
            self.d32, self.valid, self.rgba = _corrupt(g)
        else:
            self.d32, self.valid = g["depth"].astype(np.float32), None
            self.rgba = np.concatenate([g["images"], np.full((M, H, W, 1), 255, np.uint8)], -1)
        self.scene = SceneRays(self.rgba, g["c2w"], g["K"], (300.0, 1000.0), device=DEV)
        c2w32, w2c32 = R.rounded_cameras(g["c2w"])
        K32 = g["K"].astype(np.float32)
        assert (c2w32 == self.scene.c2ws.cpu().numpy()).all() and (K32 == self.scene.intrinsics.cpu().numpy()).all()
        a = (self.valid, self.rgba[..., 3])
        self.ref64, self.ref32 = R.Reference(self.d32, c2w32, w2c32, K32, *a), R.Reference(self.d32, c2w32, w2c32, K32, *a, dtype=np.float32)
        self.depths = torch.from_numpy(self.d32).to(DEV)
        self._pairs, self._noise = {}, None

    def pairs(self, r, s):
        if (r, s) not in self._pairs:
            self._pairs[r, s] = self.ref64.pairs(r, s)
        return self._pairs[r, s]

    def margins(self):
        """(m_px, m_rel) = 8 x the float32 restatement's noise over every ordered pair of views"""
        if self._noise is None:
            n_err = n_uv = n_rel = 0.0
            for r in range(self.M):
                for s in range(self.M):
                    if s == r:
                        continue
                    a, b = self.pairs(r, s), self.ref32.pairs(r, s)
                    fr = a["ref_ok"] & a["front"] & b["front"] & np.isfinite(a["u"]) & np.isfinite(b["u"]) & np.isfinite(a["v"]) & np.isfinite(b["v"])
                    if fr.any():
                        n_uv = max(n_uv, float(np.abs(b["u"][fr] - a["u"][fr]).max()), float(np.abs(b["v"][fr] - a["v"][fr]).max()))
                    both = a["ref_ok"] & a["taps_ok"] & b["taps_ok"] & (a["x0"] == b["x0"]) & (a["y0"] == b["y0"])
                    if both.any():
                        n_err = max(n_err, float(np.abs(b["err"][both] - a["err"][both]).max()))
                        n_rel = max(n_rel, float(np.abs(b["rel"][both] - a["rel"][both]).max()))
            self._noise = (n_err, n_uv, n_rel)
            print(f"\n[{self.H} x {self.W}] float32 restatement vs float64: |err| {n_err:.2e} px, |uv| {n_uv:.2e} px, |rel| {n_rel:.2e} "
                  f"-> m_px {8 * max(n_err, n_uv):.2e}, m_rel {8 * n_rel:.2e}")
        n_err, n_uv, n_rel = self._noise
        m = (8.0 * max(n_err, n_uv), 8.0 * n_rel)
        return m if self.like is None else tuple(max(a, b) for a, b in zip(m, self.like.margins()))

    def fused_noise(self, src, min_views):
        """the largest relative |fused32 - fused64| of the restatement where both runs see the same sources, and the float64 outputs"""
        s64, f64, _ = self.ref64.consistency(src, PIX, REL, min_views)
        s32, f32, _ = self.ref32.consistency(src, PIX, REL, min_views)
        same = (s32 == s64) & self.ref64.usable
        n = float(np.abs(f32[same].astype(np.float64) / f64[same] - 1.0).max())
        if self.like is not None:
            n = max(n, self.like.fused_noise(R.default_src_ids(self.like.M, 4), 3)[0])
        return n, s64, f64

    def fuse(self, src, **kw):
        kw.setdefault("valid", None if self.valid is None else torch.from_numpy(self.valid).to(DEV))
        return geometry.fuse_depths(self.scene, self.depths, src_ids=src, pix_thr=PIX, rel_thr=REL, **kw)

    def check_seen(self, seen, src, cap=None):
        """the GPU's seen bits equal the float64 verdict on every decided pair; returns the (M,H,W) map of pixels all of whose pairs are decided"""
        m_px, m_rel = self.margins()
        all_dec = np.ones(seen.shape, bool)
        inside = undecided = 0
        for r in range(self.M):
            for j, s in enumerate(src[r]):
                bit = ((seen[r] >> np.uint32(j)) & 1).astype(bool)
                if s < 0:
                    assert not bit.any(), (r, j)
                    continue
                p = self.pairs(r, int(s))
                want = self.ref64.consistent(p, PIX, REL)
                dec = R.decided(self.ref64, p, PIX, REL, m_px, m_rel, int(s))
                bad = dec & (bit != want)
                assert not bad.any(), (r, j, int(s), np.argwhere(bad)[:5].tolist(), p["err"][bad][:5], p["rel"][bad][:5])
                all_dec[r] &= dec
                inside += int((p["inside"] & p["ref_ok"]).sum())
                undecided += int((~dec & p["inside"] & p["ref_ok"]).sum())
        used = src.shape[1]
        assert (seen >> np.uint32(used) == 0).all() if used < 32 else True
        print(f"[{self.H} x {self.W}] undecided {undecided} of {inside} inside pairs ({100.0 * undecided / max(inside, 1):.3f} %)")
        if cap is not None:
            assert inside > 0 and undecided <= cap * inside, (undecided, inside)
        return all_dec

    def check_fused(self, cloud, src, all_dec, min_views):
        seen = cloud.seen.cpu().numpy().view(np.uint32)
        fused = cloud.depth.cpu().numpy()
        noise, s64, f64 = self.fused_noise(src, min_views)
        tol = 4.0 * noise
        ok = all_dec & self.ref64.usable
        assert (seen[ok] == s64[ok]).all()
        err = float(np.abs(fused[ok].astype(np.float64) / f64[ok] - 1.0).max())
        print(f"[{self.H} x {self.W}] fused: GPU rel err {err:.2e}, tolerance 4 x {tol / 4:.2e}")
        assert tol > 0 and err <= tol, (err, tol)
        bad = ~self.ref64.usable
        assert (seen[bad] == 0).all() and (fused[bad] == 0).all() and not cloud.mask.cpu().numpy()[bad].any()
        assert np.isfinite(fused).all()
        return seen, fused


@pytest.fixture(scope="module")
def big():
    return Case(97, 131)


@pytest.mark.parametrize("look_at", [False, True])
def test_pairs_match_the_float64_definition(look_at):
    c = Case(24, 40, look_at=look_at)
    src = R.default_src_ids(c.M, 4)
    cloud = c.fuse(src, min_views=3)
    assert cloud.seen.dtype == torch.int32 and cloud.mask.dtype == torch.bool and cloud.depth.dtype == torch.float32
    assert cloud.points.device == c.scene.images.device
    seen = cloud.seen.cpu().numpy().view(np.uint32)
    all_dec = c.check_seen(seen, src, cap=0.01)
    c.check_fused(cloud, src, all_dec, 3)
    assert R.popcount(seen).max() == 4 and (R.popcount(seen) == 0).any()                # the rig exercises both ends
    for mv in (0, 1, 3, 4):
        cl = c.fuse(src, min_views=mv)
        s = cl.seen.cpu().numpy().view(np.uint32)
        assert (s == seen).all()
        assert (cl.mask.cpu().numpy() == ((R.popcount(s) >= mv) & c.ref64.usable)).all(), mv
        assert int(cl.count.item()) == int(cl.mask.sum().item()) == cl.points.shape[0]


def test_one_source_and_padding():
    c = Case(24, 40)
    src = R.default_src_ids(c.M, 1)
    cloud = c.fuse(src, min_views=1)
    c.check_fused(cloud, src, c.check_seen(cloud.seen.cpu().numpy().view(np.uint32), src), 1)
    src = R.default_src_ids(c.M, 4)
    src[:, 1] = -1
    src[2] = -1
    src[4, 3] = -1
    cloud = c.fuse(src, min_views=2)
    seen, fused = c.check_fused(cloud, src, c.check_seen(cloud.seen.cpu().numpy().view(np.uint32), src), 2)
    assert (seen[2] == 0).all() and (fused[2][c.ref64.usable[2]] == c.d32[2][c.ref64.usable[2]]).all()     # no source: the depth itself
    # 32 sources: the last bit is a real one
    src = np.full((c.M, 32), -1, np.int32)
    src[:, 31] = R.default_src_ids(c.M, 1)[:, 0]
    cloud = c.fuse(src, min_views=1)
    seen32 = cloud.seen.cpu().numpy().view(np.uint32)
    c.check_seen(seen32, src)
    assert ((seen32 != 0) == (seen32 == np.uint32(1 << 31))).all() and (seen32 != 0).any()
    assert cloud.n_views.max().item() == 1


def test_views_that_cannot_agree():
    H, W = 24, 40
    g = R.make_rig(H, W, 4)
    flip = np.diag([-1.0, 1.0, -1.0, 1.0])                                              # view 1 turned by 180 degrees about its y axis: it looks away
    g["c2w"][1] = g["c2w"][1] @ flip
    g["depth"][1] = 500.0                                                               # valid depths whose points lie behind every other camera
    g["c2w"][3, 0, 3] += 50000.0                                                        # view 3 far to the side: its frustum misses the others'
    c = Case(H, W, corrupt=False, g=g)
    src = np.array([[1, 3], [0, 2], [1, 3], [0, 2]], np.int32)
    cloud = c.fuse(src, min_views=1)
    seen, fused = cloud.seen.cpu().numpy(), cloud.depth.cpu().numpy()
    for r, s in ((0, 1), (1, 0), (1, 2), (2, 1)):
        assert not (c.pairs(r, s)["front"] & c.ref64.usable[r]).any()                   # q.z <= 0 for every point, in float64
    for r, s in ((0, 3), (2, 3), (3, 0), (3, 2)):
        assert not (c.pairs(r, s)["inside"] & c.ref64.usable[r]).any()
    assert (seen == 0).all() and np.isfinite(fused).all() and (fused == np.where(c.ref64.usable, c.d32, 0)).all()
    assert not cloud.mask.any() and int(cloud.count.item()) == 0 and cloud.points.shape == (0, 3) and cloud.index.shape == (0,)


def test_two_by_two_views():
    c = Case(2, 2, M=3, corrupt=False, like=Case(24, 40))
    src = R.default_src_ids(3, 2)
    cloud = c.fuse(src, min_views=0)
    c.check_fused(cloud, src, c.check_seen(cloud.seen.cpu().numpy().view(np.uint32), src), 0)
    assert int(cloud.count.item()) == int(c.ref64.usable.sum()) == cloud.points.shape[0]


def test_error_codes():
    lib = _lib.lib()
    M, H, W, n = 2, 4, 6, 48
    f = torch.ones((64,), device=DEV)
    i32 = torch.zeros((64,), device=DEV, dtype=torch.int32)
    u8 = torch.zeros((256,), device=DEV, dtype=torch.uint8)
    i64 = torch.zeros((64,), device=DEV, dtype=torch.int64)
    P = lambda t, off=0: t.data_ptr() + off
    st = _lib.stream_ptr()

    def cons(depth=P(f), valid=0, img=P(u8), c2w=P(f), w2c=P(f), K=P(f), src=P(i32), M=M, H=H, W=W, n_src=1, pix=1.0, rel=0.01, mv=1, seen=P(i32), fused=P(f),
             mask=P(u8)):
        return lib.mvsnerf_depth_consistency_fwd(depth, valid, img, c2w, w2c, K, src, M, H, W, n_src, pix, rel, mv, seen, fused, mask, st)

    def cloud(img=P(u8), c2w=P(f), K=P(f), M=M, H=H, W=W, fused=P(f), seen=P(i32), mask=P(u8), cap=4, pts=P(f), col=P(u8), nv=P(u8), idx=P(i64), cnt=P(i64),
              ws=P(i32)):
        return lib.mvsnerf_point_cloud_fwd(img, c2w, K, M, H, W, fused, seen, mask, cap, pts, col, nv, idx, cnt, ws, st)

    EINVAL, EUNSUP, EALIGN = -1, -2, -3
    for kw in ({"depth": 0}, {"c2w": 0}, {"w2c": 0}, {"K": 0}, {"src": 0}, {"seen": 0}, {"fused": 0}, {"mask": 0}, {"M": 0}, {"H": 0}, {"W": -1},
               {"n_src": 0}, {"n_src": 33}, {"mv": -1}, {"pix": 0.0}, {"pix": float("nan")}, {"rel": -0.5}, {"rel": float("inf")}):
        assert cons(**kw) == EINVAL, kw
    for kw in ({"H": 1}, {"W": 1}, {"M": 1 << 15, "H": 1 << 8, "W": 1 << 8}, {"M": 1, "H": 1 << 16, "W": 1 << 15}):
        assert cons(**kw) == EUNSUP, kw
    for kw in ({"depth": P(f, 2)}, {"img": P(u8, 1)}, {"c2w": P(f, 1)}, {"w2c": P(f, 2)}, {"K": P(f, 3)}, {"src": P(i32, 2)}, {"seen": P(i32, 1)}, {"fused": P(f, 2)}):
        assert cons(**kw) == EALIGN, kw
    for kw in ({"mask": 0}, {"cnt": 0}, {"ws": 0}, {"cap": -1}, {"pts": 0}, {"col": 0}, {"nv": 0}, {"idx": 0}, {"img": 0}, {"fused": 0}, {"seen": 0}, {"M": 0}, {"W": 0}):
        assert cloud(**kw) == EINVAL, kw
    for kw in ({"H": 1}, {"W": 1}, {"M": 1 << 15, "H": 1 << 8, "W": 1 << 8}):
        assert cloud(**kw) == EUNSUP, kw
    for kw in ({"img": P(u8, 2)}, {"c2w": P(f, 2)}, {"K": P(f, 1)}, {"fused": P(f, 2)}, {"seen": P(i32, 2)}, {"pts": P(f, 2)}, {"idx": P(i64, 4)}, {"cnt": P(i64, 4)},
               {"ws": P(i32, 2)}):
        assert cloud(**kw) == EALIGN, kw
    torch.cuda.synchronize()
    assert (i32 == 0).all() and (f == 1).all() and (u8 == 0).all() and (i64 == 0).all()     # a refused call launches nothing
    assert lib.mvsnerf_point_cloud_workspace_bytes(0) == 0 and lib.mvsnerf_point_cloud_workspace_bytes(1 << 31) == 0
    assert lib.mvsnerf_point_cloud_workspace_bytes(n) == 8


@pytest.fixture(scope="module")
def big_cloud(big):
    src = R.default_src_ids(big.M, 4)
    return src, big.fuse(src, min_views=3)


def test_compaction(big, big_cloud):
    """97 x 131 x 5 = 63535 pixels: 63 workgroups of 1024 pixels feed the scan.  The scan has one level (a single workgroup owns every workgroup count, up to
    2^21 of them), so no pixel count reaches a second one."""
    c, (src, cloud) = big, big_cloud
    seen = cloud.seen.cpu().numpy().view(np.uint32)
    all_dec = c.check_seen(seen, src, cap=0.01)
    c.check_fused(cloud, src, all_dec, 3)
    mask = cloud.mask.reshape(-1)
    want = torch.nonzero(mask).reshape(-1)
    N = int(want.numel())
    assert 0 < N < mask.numel() and int(cloud.count.item()) == N
    assert cloud.points.shape == (N, 3) and cloud.colors.shape == (N, 3) and cloud.n_views.shape == (N,) and cloud.index.shape == (N,)
    assert cloud.index.dtype == torch.int64 and torch.equal(cloud.index, want)
    idx = want.cpu().numpy()
    assert (cloud.colors.cpu().numpy() == c.rgba.reshape(-1, 4)[idx, :3]).all()
    assert (cloud.n_views.cpu().numpy() == R.popcount(seen).reshape(-1)[idx]).all()
    fused = cloud.depth.cpu().numpy()
    p64 = c.ref64.compact(cloud.mask.cpu().numpy(), fused, seen, c.rgba)
    p32 = c.ref32.compact(cloud.mask.cpu().numpy(), fused, seen, c.rgba)
    assert (p64[3] == idx).all()
    tol = 4.0 * float(np.abs(p32[0].astype(np.float64) - p64[0]).max())
    err = float(np.abs(cloud.points.cpu().numpy().astype(np.float64) - p64[0]).max())
    print(f"[97 x 131] points: GPU abs err {err:.2e}, tolerance 4 x {tol / 4:.2e}")
    assert tol > 0 and err <= tol, (err, tol)

    bank = (c.scene.images, c.scene.c2ws, c.scene.intrinsics, cloud.depth, cloud.seen)
    m8 = cloud.mask.view(torch.uint8)
    # nothing kept, everything kept
    e = ops.point_cloud(*bank, torch.zeros_like(m8), 16)
    assert int(e[4].item()) == 0
    n_all = m8.numel()
    a = ops.point_cloud(*bank, torch.ones_like(m8), n_all)
    assert int(a[4].item()) == n_all and torch.equal(a[3], torch.arange(n_all, device=DEV))
    assert (a[1].cpu().numpy() == c.rgba.reshape(-1, 4)[:, :3]).all()
    # a capacity below the count: the true total, and no row past the capacity touched
    cap, rows = N // 3, N + 7
    out = (torch.full((rows, 3), -7.0, device=DEV), torch.full((rows, 3), 0xA5, device=DEV, dtype=torch.uint8),
           torch.full((rows,), 0xA5, device=DEV, dtype=torch.uint8), torch.full((rows,), -7, device=DEV, dtype=torch.int64))
    s = ops.point_cloud(*bank, m8, cap, out=out)
    assert int(s[4].item()) == N
    assert torch.equal(out[0][:cap], cloud.points[:cap]) and torch.equal(out[1][:cap], cloud.colors[:cap])
    assert torch.equal(out[2][:cap], cloud.n_views[:cap]) and torch.equal(out[3][:cap], cloud.index[:cap])
    assert (out[0][cap:] == -7.0).all() and (out[1][cap:] == 0xA5).all() and (out[2][cap:] == 0xA5).all() and (out[3][cap:] == -7).all()
    # an explicit, sufficient capacity: the same rows, the count left on the device
    big_cap = c.fuse(src, min_views=3, capacity=N + 100)
    assert big_cap.points.shape == (N + 100, 3) and big_cap.count.is_cuda and int(big_cap.count.item()) == N
    for x, y in ((big_cap.points, cloud.points), (big_cap.colors, cloud.colors), (big_cap.n_views, cloud.n_views), (big_cap.index, cloud.index)):
        assert torch.equal(x[:N], y)


def test_two_runs_give_the_same_bytes(big, big_cloud):
    src, a = big_cloud
    b = big.fuse(src, min_views=3)
    for name in ("points", "colors", "n_views", "index", "count", "depth", "mask", "seen"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), name


@pytest.mark.parametrize("M,H,W", [(5, 231, 229), (4, 256, 256), (5, 109, 481)])
def test_scan_runs_of_two(M, H, W):
    """The one-workgroup scan of the compaction (256 threads over the counts of 1024-pixel workgroups; csrc/scan_dev.h) where a thread owns more than one
    count.  5 x 231 x 229 = 264495 pixels: 259 counts, runs of c = 2, threads 130..255 own nothing.  4 x 256 x 256 = 256 x 1024 pixels: 256 counts, c = 1,
    every run full.  5 x 109 x 481 = 256 x 1024 + 1 pixels: 257 counts, the step to c = 2, the last non-empty run (thread 128) holds one count.  The mask
    is a seeded Bernoulli draw and fused / seen are arbitrary: ops.point_cloud takes them as they are.  Integer outputs are compared exactly; points as in
    test_compaction (4 x the float32 restatement's distance from the float64 one on the same fused depths)."""
    n = M * H * W
    assert (n + 1023) // 1024 == {264495: 259, 262144: 256, 262145: 257}[n]
    rs = np.random.RandomState(n % 1000)
    c2w, K = R.rig_cameras(H, W, M)
    c2w32, w2c32 = R.rounded_cameras(c2w)
    K32 = K.astype(np.float32)
    rgba = rs.randint(0, 256, (M, H, W, 4)).astype(np.uint8)
    fused = rs.uniform(300.0, 1000.0, (M, H, W)).astype(np.float32)
    seen = rs.randint(0, 1 << 31, (M, H, W)).astype(np.uint32)
    mask = (rs.random_sample((M, H, W)) < 0.5).astype(np.uint8)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    m8 = dev(mask)
    want = torch.nonzero(m8.reshape(-1)).reshape(-1)
    N = int(want.numel())
    assert 0 < N < n
    pts, col, nv, idx, count = ops.point_cloud(dev(rgba), dev(c2w32), dev(K32), dev(fused), dev(seen.view(np.int32)), m8, N + 3)
    assert int(count.item()) == N
    assert idx.dtype == torch.int64 and torch.equal(idx[:N], want)
    p64 = R.Reference(fused, c2w32, w2c32, K32).compact(mask, fused, seen, rgba)
    p32 = R.Reference(fused, c2w32, w2c32, K32, dtype=np.float32).compact(mask, fused, seen, rgba)
    assert torch.equal(idx[:N].cpu(), torch.from_numpy(p64[3]))
    assert torch.equal(col[:N].cpu(), torch.from_numpy(p64[1])) and torch.equal(nv[:N].cpu(), torch.from_numpy(p64[2]))
    tol = 4.0 * float(np.abs(p32[0].astype(np.float64) - p64[0]).max())
    err = float(np.abs(pts[:N].cpu().numpy().astype(np.float64) - p64[0]).max())
    print(f"[{M} x {H} x {W}] points: GPU abs err {err:.2e}, tolerance 4 x {tol / 4:.2e}")
    assert tol > 0 and err <= tol, (err, tol)


class _AnalyticSystem:
    """render_rays of a system whose scene is the rig's: the analytic depth of the rays it is handed"""

    def __init__(self):
        self.calls = []

    def render_rays(self, rays, scale=1.0, chunk=None):
        self.calls.append((tuple(rays.shape), scale, chunk))
        r = rays.cpu().numpy().astype(np.float64)
        t, _ = R.analytic_depth(r[:, :3], r[:, 3:6])
        return torch.zeros((rays.shape[0], 3), device=rays.device), torch.from_numpy(t * scale).to(rays.device, torch.float32)


def test_render_fuse_save(tmp_path):
    H, W = 24, 40
    c = Case(H, W, corrupt=False)
    sysm = _AnalyticSystem()
    depths = geometry.render_depths(sysm, c.scene, scale=1.0, chunk=4096)
    assert sysm.calls == [((H * W, 8), 1.0, 4096)] * c.M
    assert depths.shape == (c.M, H, W) and depths.dtype == torch.float32 and depths.is_cuda
    # the bank's fp32 rays against the float64 ray cast: the same surfaces up to the rounding of the cameras
    assert np.abs(depths.cpu().numpy() / c.g["depth"] - 1.0)[_one_label(c.g["label"])].max() < 1e-5
    cloud = geometry.fuse_depths(c.scene, depths)                                       # the defaults: 4 nearest views, 1 px, 1 %, 3 views
    assert (cloud.src_ids.cpu().numpy() == geometry.nearest_source_ids(c.scene, 4)).all()
    path = str(tmp_path / "rig.ply")
    N = geometry.save_ply(path, cloud)
    assert N == int(cloud.count.item()) > 0.3 * c.M * H * W
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert f"element vertex {N}\n".encode() in head and len(body) == 15 * N
    rec = np.frombuffer(body, dtype=np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
    assert rec["xyz"].tobytes() == cloud.points.cpu().numpy().tobytes() and rec["rgb"].tobytes() == cloud.colors.cpu().numpy().tobytes()
    # every point lies on the plane or the sphere.  A kept pixel's fused depth averages its own ray-cast depth z and depths z' with |z' - z| < rel_thr z,
    # so it is within rel_thr z of z along its ray, and the point within rel_thr z |d| of the surface.
    idx = cloud.index.cpu().numpy()
    z = depths.cpu().numpy().reshape(-1)[idx].astype(np.float64)
    dnorm = np.concatenate([np.linalg.norm(R.view_rays(c.g["c2w"][m], c.g["K"][m], H, W)[1], axis=-1).reshape(-1) for m in range(c.M)])[idx]
    P = rec["xyz"].astype(np.float64)
    dist = np.minimum(np.abs(P[:, 2] - R.PLANE_Z), np.abs(np.linalg.norm(P, axis=-1) - R.SPHERE_R))
    assert (dist <= 0.01 * z * dnorm + 1e-3).all(), float((dist - 0.01 * z * dnorm).max())


def _one_label(label):
    """pixels whose 3 x 3 neighbourhood carries one label (a rounded ray at the silhouette may hit the other surface)"""
    out = np.ones(label.shape, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out &= np.roll(label, (dy, dx), (1, 2)) == label
    return out
