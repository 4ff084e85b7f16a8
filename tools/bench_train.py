"""Bench tool: time optimizer steps of the CFG-DDPM trainer on the HIP path (fwd + bwd [+ gradient exchange] + clip + AdamW).

  python tools/bench_train.py --size 256 --batch 8 --steps 3                 one GPU (config C3 with --batch 64)
  python tools/bench_train.py --gpus 8 --size 256 --batch 64 --steps 3       config C4: data-parallel, batch per GPU --
                                                                             this process starts the 8 ranks itself
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29511 \\
      tools/bench_train.py --gpus 8 --size 256 --batch 64 --steps 3          the same under a launcher

Every rank trains on its own synthetic batch (seed = base + rank); the step adds the ONE collective of data-parallel
training (hdiff_amd.parallel.FlatGradients: reduce-scatter + all-gather of the 190.8 MB flat gradient buffer).  Timing:
barrier + synchronize on both sides, max over ranks; rank 0 prints one JSON line (samples/s = world * batch / time).
The step itself is bench.train_steps -- the same code bench.py runs for its `configs.C3` entry.
No 8-GPU run has been made from the build box (one GPU); the driver can run this.

  python tools/bench_train.py --tree b --size 256 --batch 2 --steps 10       the second tree (image-conditioned DynamicUNet,
                                                                             default config ch=128, ch_mult=[1,2,2,2], 2 res
                                                                             blocks, dropout 0.15): GaussianDiffusionTrainer
                                                                             fwd + bwd + clip(1.0) + native AdamW, one GPU;
                                                                             prints ms per optimizer step.  No DINOv2 term
                                                                             (not part of the package); --msssim native adds
                                                                             the MS-SSIM + L1 term (Loss.loss.MSSSIMLoss) and
                                                                             prints the line of --msssim none beside it, both
                                                                             measured in this call.
  python tools/bench_train.py --tree b --size 256 --batch 2 --steps 10 --ema   the same step with and without ema.update()
                                                                             (hdiff_amd.optim.EMA: one hdiff_ema_update launch
                                                                             over all tensors), the two arms alternating in one
                                                                             process (--alternate) with engine clock and board
                                                                             power, then the EMA launch and the AdamW launches
                                                                             alone by device events, with the parameter count and
                                                                             the bytes each streams (12 and 32 per parameter).
  python tools/bench_train.py --tree b --size 256 --batch 2 --steps 10 --prediction v [--loss-weighting min_snr]
                                                                             the same step with the eps trainer and with a
                                                                             prediction="v" trainer on the same model, the two
                                                                             arms alternating in one process (--alternate) with
                                                                             engine clock and board power."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--gpus", type=int, default=None, help="ranks (one per GPU); > 1 without a launcher: started from here")
ap.add_argument("--size", type=int, default=256); ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--steps", type=int, default=3); ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--dropout", type=float, default=0.15)
ap.add_argument("--tree", choices=("a", "b"), default="a", help="a: the CFG-DDPM UNet (default); b: the image-conditioned DynamicUNet")
ap.add_argument("--msssim", choices=("none", "native"), default="none",
                help="--tree b: none = no MS-SSIM term (default); native = the HIP MS-SSIM + L1 loss, reported beside a run without it")
ap.add_argument("--ema", action="store_true", help="--tree b: the step with and without hdiff_amd.optim.EMA.update(), alternating")
ap.add_argument("--ema-decay", type=float, default=0.9999)
ap.add_argument("--alternate", type=int, default=3, help="--ema / --prediction: repetitions of the pair of arms")
ap.add_argument("--prediction", choices=("eps", "v"), default="eps",
                help="--tree b: v = the step of a prediction='v' trainer beside the eps trainer's, alternating")
ap.add_argument("--loss-weighting", choices=("min_snr",), default=None, help="--tree b: the trainer's loss_weighting of the second arm")
ap.add_argument("--rehearse-one-gpu", action="store_true",
                help="dev: the data-parallel code path with every rank on cuda:0 over gloo (RCCL refuses two ranks on one device)")
a = ap.parse_args()


def tree_b_steps(size, batch, steps, warmup, dropout, msssim="none"):
    import time
    import warnings
    from hdiff_amd import optim as HO
    from hdiff_amd.diffusion.Diffusion import GaussianDiffusionTrainer
    from hdiff_amd.diffusion.Model import DynamicUNet
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = DynamicUNet(T=1000, ch=128, ch_mult=[1, 2, 2, 2], num_res_blocks=2, dropout=dropout).to(dev).train()
    msssim_loss = None
    if msssim == "native":
        from hdiff_amd.Loss.loss import MSSSIMLoss
        msssim_loss = MSSSIMLoss()
    tr = GaussianDiffusionTrainer(m, 1e-4, 0.02, 1000, msssim_loss=msssim_loss)
    opt = HO.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)
    g = torch.Generator().manual_seed(1)
    label = torch.randint(0, 256, (batch, 3, size, size), generator=g).to(torch.uint8).to(dev)
    inp = (label.float() * torch.tensor([0.4, 0.9, 1.0], device=dev).view(1, 3, 1, 1)).to(torch.uint8)   # underwater-like cast
    losses, times = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # "no DINO / MS-SSIM callable": by design here
        for k in range(warmup + steps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            opt.zero_grad()
            loss = tr(label, inp, 0)[0]                          # rotinas.py:441-443 shape: trainer -> mean -> backward -> step
            loss.mean().backward()
            opt.step(max_grad_norm=1.0)
            torch.cuda.synchronize(dev)
            if k >= warmup:
                times.append(time.perf_counter() - t0)
            losses.append(loss.mean().item())
    times.sort()
    return {"tree": "b", "msssim": msssim, "config": "ch=128,ch_mult=[1,2,2,2],num_res_blocks=2,dropout=%g" % dropout, "size": size, "batch": batch,
            "steps": steps, "warmup": warmup, "ms_per_step_median": round(1e3 * times[len(times) // 2], 2),
            "ms_per_step_min": round(1e3 * times[0], 2), "losses": [round(v, 5) for v in losses],
            "gpu": torch.cuda.get_device_name(dev)}


def tree_b_ema(size, batch, steps, warmup, dropout, decay, alternate):
    """The step of tree_b_steps with and without ema.update(), arms alternating on ONE model / optimizer / EMA; then the launches alone."""
    import time
    import warnings
    import bench
    from hdiff_amd import optim as HO
    from hdiff_amd.diffusion.Diffusion import GaussianDiffusionTrainer
    from hdiff_amd.diffusion.Model import DynamicUNet
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = DynamicUNet(T=1000, ch=128, ch_mult=[1, 2, 2, 2], num_res_blocks=2, dropout=dropout).to(dev).train()
    tr = GaussianDiffusionTrainer(m, 1e-4, 0.02, 1000)
    opt = HO.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)
    ema = HO.EMA(m.parameters(), decay=decay)
    g = torch.Generator().manual_seed(1)
    label = torch.randint(0, 256, (batch, 3, size, size), generator=g).to(torch.uint8).to(dev)
    inp = (label.float() * torch.tensor([0.4, 0.9, 1.0], device=dev).view(1, 3, 1, 1)).to(torch.uint8)
    nparam = sum(p.numel() for p in m.parameters())

    def arm(with_ema, count):
        times = []
        for _ in range(count):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            opt.zero_grad()
            tr(label, inp, 0)[0].mean().backward()
            opt.step(max_grad_norm=1.0)
            if with_ema:
                ema.update()
            torch.cuda.synchronize(dev)
            times.append(1e3 * (time.perf_counter() - t0))
        return sorted(times)

    def alone(fn, reps=50):
        for _ in range(5):
            fn()
        torch.cuda.synchronize(dev)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / reps

    out = {"tree": "b", "config": "ch=128,ch_mult=[1,2,2,2],num_res_blocks=2,dropout=%g" % dropout, "size": size, "batch": batch,
           "steps": steps, "warmup": warmup, "ema_decay": decay, "parameters": nparam, "tensors": len(ema.params),
           "ema_bytes": 12 * nparam, "gpu": torch.cuda.get_device_name(dev), "arms": []}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        arm(True, warmup)
        for rep in range(alternate):
            for name, with_ema in (("plain", False), ("ema", True)):
                clock = bench.ClockSampler(0)
                with clock:
                    t = arm(with_ema, steps)
                c = clock.summary()
                rec = {"arm": name, "rep": rep, "ms_per_step_median": round(t[len(t) // 2], 3), "ms_per_step_min": round(t[0], 3),
                       "sclk_mhz_mean": c.get("sclk_mhz_mean"), "board_power_w_mean": c.get("board_power_w_mean")}
                out["arms"].append(rec)
                print(json.dumps(rec), flush=True)
        # the launches alone, by device events: 50 back-to-back calls of the C entry on the tables the classes built (no host work between
        # the launches); the AdamW table holds the tensors that had a gradient on the last step (two middle blocks are gated off)
        import ctypes as C
        from hdiff_amd import _capi
        lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
        _, e_tab, e_chunks, e_n = ema._tables()
        _, a_tab, a_chunks, a_n, a_ps = opt._tables[0]
        n_adamw = sum(p.numel() for p in a_ps)
        out["adamw_parameters"], out["adamw_bytes"] = n_adamw, 32 * n_adamw

        def ema_launch():
            _capi.check(lib.hdiff_ema_update(e_tab.data_ptr(), e_chunks.data_ptr(), e_n, C.c_double(decay), stream), "ema_update")

        def adamw_launch():
            _capi.check(lib.hdiff_adamw_step(a_tab.data_ptr(), a_chunks.data_ptr(), a_n, None, 1e-4, 0.9, 0.999, 1e-8, 1e-4, 1000, stream),
                        "adamw_step")
        for rep in range(alternate):
            e_ms, a_ms = alone(ema_launch), alone(adamw_launch)
            rec = {"alone": rep, "ema_update_ms": round(e_ms, 4), "ema_gb_s": round(12 * nparam / e_ms / 1e6, 1),
                   "adamw_step_ms": round(a_ms, 4), "adamw_gb_s": round(32 * n_adamw / a_ms / 1e6, 1)}
            out["arms"].append(rec)
            print(json.dumps(rec), flush=True)
        out["ema_update_ms"] = sorted(r["ema_update_ms"] for r in out["arms"] if "alone" in r)[alternate // 2]
        out["adamw_step_ms"] = sorted(r["adamw_step_ms"] for r in out["arms"] if "alone" in r)[alternate // 2]
    med = lambda name: sorted(r["ms_per_step_median"] for r in out["arms"] if r.get("arm") == name)[alternate // 2]   # noqa: E731
    out["plain_ms_per_step"], out["ema_ms_per_step"] = med("plain"), med("ema")
    return out


def tree_b_prediction(size, batch, steps, warmup, dropout, prediction, weighting, alternate):
    """The step of tree_b_steps with the reference's eps trainer and with prediction= / loss_weighting=, arms alternating on ONE model
    and optimizer (two trainers around it), engine clock and board power beside each timing."""
    import time
    import warnings
    import bench
    from hdiff_amd import optim as HO
    from hdiff_amd.diffusion.Diffusion import GaussianDiffusionTrainer
    from hdiff_amd.diffusion.Model import DynamicUNet
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = DynamicUNet(T=1000, ch=128, ch_mult=[1, 2, 2, 2], num_res_blocks=2, dropout=dropout).to(dev).train()
    name = prediction + ("" if weighting is None else "+" + weighting)
    trainers = {"eps": GaussianDiffusionTrainer(m, 1e-4, 0.02, 1000),
                name: GaussianDiffusionTrainer(m, 1e-4, 0.02, 1000, prediction=prediction, loss_weighting=weighting)}
    opt = HO.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)
    g = torch.Generator().manual_seed(1)
    label = torch.randint(0, 256, (batch, 3, size, size), generator=g).to(torch.uint8).to(dev)
    inp = (label.float() * torch.tensor([0.4, 0.9, 1.0], device=dev).view(1, 3, 1, 1)).to(torch.uint8)

    def arm(tr, count):
        times = []
        for _ in range(count):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            opt.zero_grad()
            tr(label, inp, 0)[0].mean().backward()
            opt.step(max_grad_norm=1.0)
            torch.cuda.synchronize(dev)
            times.append(1e3 * (time.perf_counter() - t0))
        return sorted(times)

    out = {"tree": "b", "config": "ch=128,ch_mult=[1,2,2,2],num_res_blocks=2,dropout=%g" % dropout, "size": size, "batch": batch,
           "steps": steps, "warmup": warmup, "gpu": torch.cuda.get_device_name(dev), "arms": []}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for tr in trainers.values():
            arm(tr, warmup)
        for rep in range(alternate):
            for arm_name, tr in trainers.items():
                clock = bench.ClockSampler(0)
                with clock:
                    t = arm(tr, steps)
                c = clock.summary()
                rec = {"arm": arm_name, "rep": rep, "ms_per_step_median": round(t[len(t) // 2], 3), "ms_per_step_min": round(t[0], 3),
                       "sclk_mhz_mean": c.get("sclk_mhz_mean"), "board_power_w_mean": c.get("board_power_w_mean")}
                out["arms"].append(rec)
                print(json.dumps(rec), flush=True)
    for arm_name in trainers:
        out[arm_name + "_ms_per_step"] = sorted(r["ms_per_step_median"] for r in out["arms"] if r["arm"] == arm_name)[alternate // 2]
    return out


if a.tree == "b":
    if a.gpus not in (None, 1):
        sys.exit("bench_train.py --tree b: one GPU only (no data-parallel path for the second tree)")
    if a.prediction != "eps" or a.loss_weighting is not None:
        res = tree_b_prediction(a.size, a.batch, a.steps, a.warmup, a.dropout, a.prediction, a.loss_weighting, a.alternate)
        res.pop("arms")
        print(json.dumps(res), flush=True)
        sys.exit(0)
    if a.ema:
        res = tree_b_ema(a.size, a.batch, a.steps, a.warmup, a.dropout, a.ema_decay, a.alternate)
        res.pop("arms")
        print(json.dumps(res), flush=True)
        sys.exit(0)
    print(json.dumps(tree_b_steps(a.size, a.batch, a.steps, a.warmup, a.dropout)), flush=True)
    if a.msssim == "native":
        print(json.dumps(tree_b_steps(a.size, a.batch, a.steps, a.warmup, a.dropout, "native")), flush=True)
    sys.exit(0)
if a.gpus and a.gpus > 1 and "WORLD_SIZE" not in os.environ:      # plain start: become the launcher (the GPU is untouched so far)
    from hdiff_amd.parallel import launch_ranks
    sys.exit(launch_ranks(os.path.abspath(__file__), sys.argv[1:], a.gpus))
import bench
from hdiff_amd import parallel
rank, local, world = parallel.init_from_env(backend="gloo" if a.rehearse_one_gpu else None)
if a.gpus is not None and world != a.gpus:
    sys.exit(f"bench_train.py: --gpus {a.gpus} but WORLD_SIZE={world}")
if a.rehearse_one_gpu:
    local = 0
dev = torch.device("cuda", local if world > 1 else 0)
torch.cuda.set_device(dev)
res = bench.train_steps(a.size, a.batch, a.steps, a.warmup, a.dropout, dev, rank=rank, world=world, rehearse=a.rehearse_one_gpu)
if rank == 0:
    print(json.dumps(res), flush=True)
if world > 1: torch.distributed.destroy_process_group()
