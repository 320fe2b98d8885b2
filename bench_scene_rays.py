"""Steps per second of a fine-tune fed by the device-resident ray bank (rays.SceneRays, MVSSystemFinetune.fit_scene) against the two
ways of feeding fit_steps.

  --mode loops    a config-4-sized fine-tune (BASELINE config 4 as far as a synthetic scene allows: 5 views of 800x800, all five the source views,
                  192 planes; 1024 rays x 128 samples per step), fp32 and use_amp.  Three loops over the same number of steps, host wall clock
                  between device synchronisations, in ONE process, after a warm-up of each, in alternating rounds:
                    (a) fit_scene                            one scene_rays_march launch per step, indices from a device randperm
                    (b) fit_steps over pre-staged batches    {'rays', 'rgbs'} already on the device: the best case of the batch path
                    (c) fit_steps fed by a DataLoader        torch.utils.data.DataLoader(shuffle=True, batch_size=1024, num_workers=8) over the CPU
                                                             all-rays buffer, as train_mvs_nerf_finetuning_pl.py:127-131 feeds the reference
                  Every round's three rates are reported, with their medians; nothing is asserted about their order.
  --mode trace    a few gather and march launches at the same shapes, nothing else: meant to run under `rocprofv3 --kernel-trace --stats`.

Prints one JSON line per measurement and writes them all to --out.
"""
import argparse
import json
import time

import torch

from bench_finetune_render import SIZES


class _AllRays(torch.utils.data.Dataset):
    """The train split of the reference's datasets (data/dtu_ft.py:195-208): one ray and its colour per item, from the CPU all-rays buffer."""

    def __init__(self, rays, rgbs):
        self.all_rays, self.all_rgbs = rays, rgbs

    def __len__(self):
        return len(self.all_rays)

    def __getitem__(self, idx):
        return {"rays": self.all_rays[idx], "rgbs": self.all_rgbs[idx]}


def _scene(size):
    """(SceneRays on the GPU, the same scene's all-rays buffer on the CPU as read_meta leaves it)."""
    from mvsnerf_amd.rays import SceneRays
    from mvsnerf_amd.synth import make_rig
    s = SIZES[size]
    base = (0.0, 0.25, -0.25, 0.12, -0.12, 0.1)
    rig = make_rig(s["H"], s["W"], n_views=s["V"], seed=9, baselines=base[:s["V"]], smooth=True)
    u8 = (rig["images_raw"][0].permute(0, 2, 3, 1) * 255).round().to(torch.uint8)
    scene = SceneRays(u8, rig["c2ws"][0], rig["intrinsics"][0], rig["near_fars"][0], device="cuda")
    views = [scene.view(m) for m in range(s["V"])]
    all_rays = torch.cat([v[0] for v in views], 0).cpu()
    all_rgbs = torch.cat([v[1].reshape(-1, 3) for v in views], 0).cpu()
    return scene, all_rays, all_rgbs


def _system(scene, size, use_amp, n_rays):
    from mvsnerf_amd import train
    s = SIZES[size]
    args = train.default_args(pad=24 if size != "tiny" else 4, N_samples=s["S"], n_views=s["V"], batch_size=n_rays, use_amp=use_amp)
    return train.MVSSystemFinetune(args, scene.source_views(range(s["V"])), n_depth_planes=s["D"]).to("cuda")


def _rate(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def _median(v):
    return sorted(v)[len(v) // 2]


def loops_mode(size, modes, steps, rounds, n_rays, workers, results):
    from mvsnerf_amd import ops, train
    scene, all_rays, all_rgbs = _scene(size)
    r0 = dict(kind="scene", size=size, views=scene.n_views, hw=list(scene.hw), n_rays=scene.n_rays, bank_bytes=scene.images.numel(),
              all_rays_buffer_bytes=all_rays.numel() * 4 + all_rgbs.numel() * 4)
    results.append(r0)
    print(json.dumps(r0), flush=True)
    loader = torch.utils.data.DataLoader(_AllRays(all_rays, all_rgbs), shuffle=True, num_workers=workers, batch_size=n_rays, pin_memory=True,
                                         persistent_workers=workers > 0)

    def loader_batches(n):
        done = 0
        while done < n:
            for b in loader:
                if done == n:
                    return
                done += 1
                yield b
    for mode in modes:
        ft = _system(scene, size, mode == "bf16", n_rays)
        opt = ft.configure_optimizers()[0][0]
        staged = [dict(zip(("rays", "rgbs"), (t[None] for t in scene.gather(i)))) for i in train._scene_index_batches(scene, steps, n_rays, 1)]
        loops = {"fit_scene": lambda: ft.fit_scene(scene, steps, n_rays, seed=2, optimizer=opt),
                 "fit_steps_prestaged": lambda: ft.fit_steps(staged, opt),
                 "fit_steps_dataloader": lambda: ft.fit_steps(loader_batches(steps), opt)}
        with ops.mlp_precision("fp32"):              # use_amp sets bf16 inside the step
            for fn in loops.values():                # warm-up of all three (the loader's workers start here)
                fn()
            rates = {k: [] for k in loops}
            for _ in range(rounds):
                for k, fn in loops.items():
                    rates[k].append(_rate(fn, steps))
        r = dict(kind="loops", size=size, mlp=mode, rays=n_rays, samples=n_rays * ft.args.N_samples, steps=steps, loader_workers=workers,
                 steps_per_s={k: [round(x, 1) for x in v] for k, v in rates.items()}, median_steps_per_s={k: round(_median(v), 1) for k, v in rates.items()},
                 median_ms_per_step={k: round(1e3 / _median(v), 3) for k, v in rates.items()})
        results.append(r)
        print(json.dumps(r), flush=True)
        del ft, opt, staged
        torch.cuda.empty_cache()


def trace_mode(size, n_rays):
    scene, _, _ = _scene(size)
    S = SIZES[size]["S"]
    H, W = scene.hw
    ref = (torch.eye(4, device="cuda"), scene.intrinsics[0], scene.near_far[0], (H, W), 24)
    g = torch.Generator(device="cuda").manual_seed(0)
    for idx in list(scene.epoch(n_rays, g))[:20]:
        scene.gather(idx)
        scene.march(idx, S, perturb=1.0, jitter=torch.rand((idx.shape[0], S), device="cuda"), ref=ref)
    scene.view(0)
    torch.cuda.synchronize()
    print(json.dumps(dict(kind="trace", size=size, rays=n_rays, samples=S, launches_each=20)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("loops", "trace"), default="loops")
    ap.add_argument("--size", default="config4", choices=sorted(SIZES))
    ap.add_argument("--mlp", default="fp32,bf16")
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_rays.py measures on the GPU; none found")
    results = []
    if a.mode == "loops":
        loops_mode(a.size, a.mlp.split(","), a.steps, a.rounds, a.rays, a.workers, results)
    else:
        trace_mode(a.size, a.rays)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
