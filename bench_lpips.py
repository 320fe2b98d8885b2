"""Time of LPIPS-VGG on the device (evaluate.LPIPS, csrc/lpips.hip) at the frame sizes the reference evaluates at:

    dtu     512 x 640
    llff    640 x 960

Per size, K = 1, medians over --reps repetitions after --warmup unrecorded ones, by device events, in alternating rounds:
    features          lp.features(img): the trunk on one image
    pair              lp(rgb, img): the trunk on prediction and target as one N = 2 batch, and the five heads
    torch_eager       the same network with the same weights through torch on the same GPU (F.conv2d / F.max_pool2d in NCHW and the heads in torch ops,
                      the (H,W,3) -> NCHW copies included): the baseline, since nothing in the library computed LPIPS before
    groups            the N = 2 trunk again, one event pair per block of convolutions (conv1_x .. conv5_x, each with the pool in front of it)
and the achieved TFLOP/s of the convolutions from 305 856 MAC per pixel and image (H, W divisible by 16) against the 157.3 TFLOP/s fp32 MFMA peak.
Weights are seeded random numbers (the pretrained files are not needed to time the arithmetic).  Nothing is asserted about the order of the
timings.  Prints one JSON line per size and writes them all to --out (default profiles/lpips.json)."""
import argparse
import json

import torch
import torch.nn.functional as F

SIZES = {"dtu": (512, 640), "llff": (640, 960), "tiny": (64, 96)}
WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
TAPS = (1, 3, 6, 9, 12)
POOL_BEFORE = (2, 4, 7, 10)
GROUPS = ((0, 1), (2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12))
PEAK_TFLOPS = 157.3
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)


def _median(v):
    return sorted(v)[len(v) // 2]


def seeded_weights(seed=0):
    g = torch.Generator().manual_seed(seed)
    convs, cin = [], 3
    for cout in WIDTHS:
        convs.append((torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5, torch.rand((cout,), generator=g) * 0.2 - 0.1))
        cin = cout
    lins = [torch.rand((WIDTHS[t],), generator=g) / WIDTHS[t] for t in TAPS]
    return convs, lins


def group_macs(H, W):
    """MAC per image of each block of convolutions"""
    out, cin, h, w = [], 3, H, W
    for grp in GROUPS:
        m = 0
        for i in grp:
            if i in POOL_BEFORE:
                h, w = h // 2, w // 2
            m += h * w * 9 * cin * WIDTHS[i]
            cin = WIDTHS[i]
        out.append(m)
    return out


def torch_eager(rgb, img, convs, lins):
    """(H,W,3) x 2 on the device -> (1,) float64: torch ops only"""
    dev = rgb.device
    shift, scale = torch.tensor(SHIFT, device=dev).view(1, 3, 1, 1), torch.tensor(SCALE, device=dev).view(1, 3, 1, 1)
    x = torch.stack([rgb, img]).permute(0, 3, 1, 2).contiguous()
    x = ((2 * x - 1) - shift) / scale
    total = torch.zeros((1,), device=dev, dtype=torch.float64)
    k = 0
    for i, (w, b) in enumerate(convs):
        if i in POOL_BEFORE:
            x = F.max_pool2d(x, 2, 2)
        x = F.relu(F.conv2d(x, w, b, padding=1))
        if i in TAPS:
            n = x / (torch.sqrt((x ** 2).sum(1, keepdim=True)) + 1e-10)
            d = ((n[0:1] - n[1:2]) ** 2 * lins[k].view(1, -1, 1, 1)).sum(1)
            total = total + d.double().mean(dim=(1, 2))
            k += 1
    return total


def measure(name, reps, warmup):
    from mvsnerf_amd import evaluate, ops
    H, W = SIZES[name]
    convs, lins = seeded_weights()
    vgg = {f"{idx}.{kind}": t for idx, wb in zip(CONVS, convs) for kind, t in zip(("weight", "bias"), wb)}
    lin = {f"lin{i}.model.1.weight": v.view(1, -1, 1, 1) for i, v in enumerate(lins)}
    lp = evaluate.LPIPS(vgg, lin, device="cuda")
    g = torch.Generator().manual_seed(1)
    rgb, img = torch.rand((H, W, 3), generator=g).cuda(), torch.rand((H, W, 3), generator=g).cuda()
    dconvs, dlins = [(w.cuda(), b.cuda()) for w, b in convs], [v.cuda() for v in lins]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        def run():
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        return run
    pair_in = torch.stack([rgb, img])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(GROUPS) + 1)]

    def groups():
        x = pair_in
        ev[0].record()
        for gi, grp in enumerate(GROUPS):
            for i in grp:
                if i in POOL_BEFORE:
                    x = ops.lpips_pool(x)
                x = ops.lpips_conv(x, lp.packed[i], WIDTHS[i])
            ev[gi + 1].record()
        ev[-1].synchronize()
        return [ev[gi].elapsed_time(ev[gi + 1]) for gi in range(len(GROUPS))]
    loops = {"features": timed(lambda: lp.features(img)), "pair": timed(lambda: lp(rgb, img)),
             "torch_eager": timed(lambda: torch_eager(rgb, img, dconvs, dlins))}
    ms = {k: [] for k in loops}
    gms = [[] for _ in GROUPS]
    with torch.no_grad():
        for i in range(warmup + reps):
            for k, fn in loops.items():
                t = fn()
                if i >= warmup:
                    ms[k].append(t)
            t = groups()
            if i >= warmup:
                for gi, v in enumerate(t):
                    gms[gi].append(v)
        theirs = float(torch_eager(rgb, img, dconvs, dlins)[0])
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ours = float(lp(rgb, img)[0])
        peak = int(torch.cuda.max_memory_allocated() - base)
    macs = group_macs(H, W)
    med = {k: _median(v) for k, v in ms.items()}
    gmed = [_median(v) for v in gms]

    def tflops(mac, n_img, t_ms):
        return round(2.0 * mac * n_img / (t_ms * 1e-3) / 1e12, 2)
    return dict(kind="lpips", size=name, hw=[H, W], K=1, reps=reps, mac_per_image=sum(macs), mac_per_pixel=sum(macs) / (H * W),
                median_ms={k: round(v, 3) for k, v in med.items()}, min_ms={k: round(min(v), 3) for k, v in ms.items()},
                max_ms={k: round(max(v), 3) for k, v in ms.items()},
                tflops={"features": tflops(sum(macs), 1, med["features"]), "pair": tflops(sum(macs), 2, med["pair"]),
                        "torch_eager": tflops(sum(macs), 2, med["torch_eager"])},
                groups=[dict(group=f"conv{gi + 1}_x", gmac_per_image=round(macs[gi] / 1e9, 3), median_ms=round(gmed[gi], 3),
                             tflops=tflops(macs[gi], 2, gmed[gi]), of_peak=round(tflops(macs[gi], 2, gmed[gi]) / PEAK_TFLOPS, 3)) for gi in range(len(GROUPS))],
                of_peak={"pair": round(tflops(sum(macs), 2, med["pair"]) / PEAK_TFLOPS, 3)}, peak_tflops=PEAK_TFLOPS,
                value={"hip": ours, "torch_eager": theirs}, pair_peak_bytes=peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="dtu,llff")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/lpips.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips.py measures on the GPU; none found")
    results = []
    for name in a.sizes.split(","):
        r = measure(name, a.reps, a.warmup)
        results.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
