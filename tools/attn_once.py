"""Dev tool: launch the dominant attention kernel a few times at the bench shape (for rocprofv3 --pmc passes).
argv: [batch] [channels = 128] [L = 65536] [--routes a,b,... [--rounds N]]; the contraction mode comes from HDIFF_CONTRACT (default
bf16x3: the pre-split kernels, with their workspace).
--routes: an A/B of HDIFF_MHA_FWD_ROUTE_* values (hdiff_mha_flash_fwd_ws_as; 3,6 = the d_head 16 pair kernel with 256 / 384 queries per
workgroup) -- the routes take turns, N rounds (default 3) of 3 launches each, one line per turn with the engine clock and board power
sampled during that turn beside the time."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch, hdiff_amd
lib = hdiff_amd.lib()
routes, rounds = [None], 1
if "--routes" in sys.argv:
    i = sys.argv.index("--routes")
    routes, rounds = [int(r) for r in sys.argv[i + 1].split(",")], 3
    del sys.argv[i:i + 2]
if "--rounds" in sys.argv:
    i = sys.argv.index("--rounds")
    rounds = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
Cc = int(sys.argv[2]) if len(sys.argv) > 2 else 128
L = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
qkv = torch.randn(B, 3 * Cc, L, device="cuda")
o = torch.empty(B, Cc, L, device="cuda")
need = C.c_int64(0)
lib.hdiff_mha_flash_fwd_workspace(B, Cc, 8, L, C.byref(need))
ws = torch.empty(need.value // 4 + 1, device="cuda") if need.value > 0 else None
s = torch.cuda.current_stream().cuda_stream
def go(route=None):
    args = (qkv.data_ptr(), o.data_ptr(), None, B, Cc, 8, L, None if ws is None else ws.data_ptr(), need.value)
    rc = lib.hdiff_mha_flash_fwd_ws(*args, s) if route is None else lib.hdiff_mha_flash_fwd_ws_as(*args, route, s)
    assert rc == 0, lib.hdiff_last_error()
def timed(route):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        go(route)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 3
for r in routes:
    go(r)
torch.cuda.synchronize()
if routes == [None]:
    ms = timed(None)
    print(f"fwd B={B} C={Cc} L={L}: {ms:.3f} ms  {4.0 * L * L * Cc * B / ms / 1e9:.1f} TFLOP/s-eq (split pass included)")
else:
    from bench import ClockSampler
    for k in range(rounds):
        for r in routes:
            clock = ClockSampler(0)
            with clock:
                ms = timed(r)
            c = clock.summary()
            print(f"round {k} route {r} fwd B={B} C={Cc} L={L}: {ms:.3f} ms (split pass included); sclk {c.get('sclk_mhz_mean')} MHz, "
                  f"board {c.get('board_power_w_mean')} W", flush=True)
