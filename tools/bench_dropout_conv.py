"""Bench tool: forward + backward of ONE dropout conv -- conv(dropout(swish(GroupNorm(x)))) + residual, block2 of a ResBlock
(ModelCondition.py:184-186, 202) -- through hdiff_amd.autograd.fused_conv(..., drop_p=), as a training step runs it.

  python tools/bench_dropout_conv.py                       both shapes below, 50 timed iterations after 5 of warm-up
  python tools/bench_dropout_conv.py --iters 100 --drop 0.15

Shapes: 128 -> 128 at 256x256, batch 8 (first level of the 256x256 runs) and 256 -> 256 at 32x32, batch 80 (as the default
32x32 run's batch; its own 256-channel levels are 16x16 and below).  Device events around the timed iterations; prints one JSON
line per shape: ms per forward + backward, and the peak of torch.cuda.max_memory_allocated() over the timed iterations minus
what was allocated before them (inputs and parameters excluded: what the step itself holds)."""
import argparse, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50); ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--drop", type=float, default=0.15)
a = ap.parse_args()

import hdiff_amd
from hdiff_amd import autograd as A

dev = torch.device("cuda", 0)
for (cin, cout, size, batch) in ((128, 128, 256, 8), (256, 256, 32, 80)):
    g = torch.Generator().manual_seed(cin + size)
    x = torch.randn(batch, cin, size, size, generator=g).to(dev).requires_grad_(True)
    sc = torch.randn(batch, cout, size, size, generator=g).to(dev).requires_grad_(True)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)).to(dev).requires_grad_(True)
    b = torch.zeros(cout, device=dev, requires_grad=True)
    gw, gb = torch.ones(cin, device=dev, requires_grad=True), torch.zeros(cin, device=dev, requires_grad=True)
    dout = torch.randn(batch, cout, size, size, generator=g).to(dev)
    leaves = (x, sc, w, b, gw, gb)

    def step():
        for t in leaves:
            t.grad = None
        y = A.fused_conv(x, None, w, b, gw, gb, residual=sc, k=3, drop_p=a.drop)
        y.backward(dout)

    torch.manual_seed(0)
    for _ in range(a.warmup):
        step()
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.iters):
        step()
    t1.record()
    torch.cuda.synchronize()
    print(json.dumps({"bench": "dropout_conv_fwd_bwd", "shape": f"{cin}->{cout} {size}x{size} B{batch}", "drop": a.drop,
                      "contract": hdiff_amd.get_contraction_mode(), "iters": a.iters,
                      "ms": round(t0.elapsed_time(t1) / a.iters, 4),
                      "peak_step_bytes": int(torch.cuda.max_memory_allocated() - base),
                      "input_bytes": x.numel() * 4}))
    del x, sc, w, b, gw, gb, dout, leaves
    torch.cuda.empty_cache()
