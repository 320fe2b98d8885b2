"""Time per image of the device resampler (ops.resample_u8, csrc/resample.hip) against Pillow's `Image.resize(..., LANCZOS)` on the
same host, at the sizes the reference's per-scene datasets resize at:

    dtu       1600 x 1200 -> 640 x 512   RGB     (data/dtu_ft.py:108,163)
    llff      4032 x 3024 -> 960 x 640   RGB     (data/llff.py:241,344)
    blender    800 x  800 -> 400 x 400   RGBA    (data/blender.py:66,133)

Per size, medians over --reps repetitions of one random image, after --warmup unrecorded ones, in alternating rounds:
    pillow            Image.resize on the host's CPU (only where Pillow is importable; its version is recorded)
    upload_resize     the host image (pageable memory, as np.asarray(Image.open(p)) leaves it) to the device, the alpha byte of an RGB image, the
                      resize into a slot of a bank: what SceneRays.from_images does per image.  Host wall clock, ended by a device synchronise.
    resize            the resize alone, source already on the device, by device events
and the bytes each moves.  Nothing is asserted about their order.  Prints one JSON line per size and writes them all to --out.
"""
import argparse
import json
import time

import numpy as np
import torch

SIZES = {"dtu": ((1200, 1600), (512, 640), 3), "llff": ((3024, 4032), (640, 960), 3), "blender": ((800, 800), (400, 400), 4),
         "tiny": ((60, 80), (24, 32), 4)}


def _median(v):
    return sorted(v)[len(v) // 2]


def measure(name, resample, reps, warmup):
    from mvsnerf_amd import ops
    hw, out_hw, C = SIZES[name]
    img = np.random.default_rng(0).integers(0, 256, hw + (C,), dtype=np.uint8)
    bank = torch.empty((1,) + out_hw + (4,), dtype=torch.uint8, device="cuda")
    try:
        import PIL
        from PIL import Image
        flt = {"lanczos": Image.LANCZOS, "bilinear": Image.BILINEAR}[resample]
        pil = Image.fromarray(img)
        pil_version = PIL.__version__
    except ImportError:
        pil = pil_version = None

    def pillow():
        t0 = time.perf_counter()
        pil.resize((out_hw[1], out_hw[0]), flt)
        return (time.perf_counter() - t0) * 1e3

    def upload_resize():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        src = torch.from_numpy(img).to("cuda")
        if C == 3:
            src = torch.nn.functional.pad(src, (0, 1), value=255)
        ops.resample_u8(src[None], out_hw, resample=resample, premultiply=C == 4, out=bank)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    dev = torch.nn.functional.pad(torch.from_numpy(img).to("cuda"), (0, 4 - C), value=255)[None].contiguous()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def resize():
        e0.record()
        ops.resample_u8(dev, out_hw, resample=resample, premultiply=C == 4, out=bank)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    loops = {"upload_resize": upload_resize, "resize": resize}
    if pil is not None:
        loops["pillow"] = pillow
    ms = {k: [] for k in loops}
    for i in range(warmup + reps):
        for k, fn in loops.items():
            t = fn()
            if i >= warmup:
                ms[k].append(t)
    return dict(kind="resample", size=name, src_hw=list(hw), dst_hw=list(out_hw), channels=C, resample=resample, reps=reps, pillow_version=pil_version,
                upload_bytes=int(img.nbytes), intermediate_bytes=hw[0] * out_hw[1] * 4, median_ms={k: round(_median(v), 3) for k, v in ms.items()},
                min_ms={k: round(min(v), 3) for k, v in ms.items()}, max_ms={k: round(max(v), 3) for k, v in ms.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="dtu,llff,blender")
    ap.add_argument("--resample", default="lanczos", choices=("lanczos", "bilinear"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py measures on the GPU; none found")
    results = []
    for name in a.sizes.split(","):
        r = measure(name, a.resample, a.reps, a.warmup)
        results.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
