"""Attention forward per launch at the two hot shapes of a 256x256 step, in chosen contraction modes, inside ONE process.

    python tools/bench_attn_fwd.py [--contract bf16x3,f16] [--alternate 3] [--batch 16] [--iters N]

The call is the inference call of a plan: hdiff_mha_flash_fwd_ws with lse2 = NULL and the workspace the library asks for, so the
split passes are inside the timed call in every mode.  --alternate N: the chosen modes are timed in turn N times (arm order
A B A B ...), each timing with the engine clock and board power sampled beside it (bench.ClockSampler).  Prints one line per
timing and a summary (mean, spread over the repetitions, ratio to the first mode) per shape."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import hdiff_amd  # noqa: E402
from bench import ClockSampler  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--contract", default="bf16x3", help="comma-separated list of f32, bf16x3, f16")
ap.add_argument("--alternate", type=int, default=1, help="time the chosen modes in turn this many times")
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--iters", type=int, default=0, help="launches per timing (default: 6 at L = 65 536, 16 at L = 16 384)")
a = ap.parse_args()
modes = a.contract.split(",")
assert all(m in ("f32", "bf16x3", "f16") for m in modes), modes
lib = hdiff_amd.lib()
s = torch.cuda.current_stream().cuda_stream
before = hdiff_amd.get_contraction_mode()
for (Cc, L) in [(128, 65536), (256, 16384)]:
    B = a.batch
    qkv = torch.randn(B, 3 * Cc, L, device="cuda")
    o = torch.empty(B, Cc, L, device="cuda")
    need = C.c_int64(0)
    assert lib.hdiff_mha_flash_fwd_workspace(B, Cc, 8, L, C.byref(need)) == 0
    ws = torch.empty(max(need.value, 16), dtype=torch.uint8, device="cuda")

    def run():
        rc = lib.hdiff_mha_flash_fwd_ws(qkv.data_ptr(), o.data_ptr(), None, B, Cc, 8, L, ws.data_ptr(), need.value, s)
        assert rc == 0, lib.hdiff_last_error()

    n = a.iters or (6 if L > 20000 else 16)
    times = {m: [] for m in modes}
    for rep in range(a.alternate):
        for m in modes:
            hdiff_amd.set_contraction_mode(m)
            run(); run()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            clock = ClockSampler(0)
            with clock:
                e0.record()
                for _ in range(n):
                    run()
                e1.record()
                torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / n
            c = clock.summary()
            times[m].append(ms)
            print(f"fwd {m:6s} B={B} C={Cc} L={L} rep {rep}: {ms:.3f} ms  {4.0 * L * L * Cc * B / ms / 1e9:.1f} TFLOP/s  "
                  f"sclk {c.get('sclk_mhz_mean')} MHz  board {c.get('board_power_w_mean')} W", flush=True)
    base = sum(times[modes[0]]) / len(times[modes[0]])
    for m in modes:
        t = times[m]
        mean = sum(t) / len(t)
        print(f"summary B={B} C={Cc} L={L} {m:6s}: mean {mean:.3f} ms, spread {max(t) - min(t):.3f} ms over {len(t)} repetitions, "
              f"{base / mean:.3f}x the speed of {modes[0]}", flush=True)
    del qkv, o, ws
hdiff_amd.set_contraction_mode(before)
