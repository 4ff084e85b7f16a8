"""Dev tool: error of the fp32-input attention kernels (forward and backward, f32 mode) against float64 as ratios to the fp32 CPU
definition's error, per tensor (O, lse2, dQ, dK, dV), for every (case, family) of tests/_attn_f32_cases.py -- the table behind
tests/test_gpu_attention_f32.py's margins (profiles/attention_f32_error_ratio.txt).  The gate's other checks run too; a failure is
printed and the table goes on.
   python3 tools/attn_f32_error_ratio.py [family = all] [margin = the gate's]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, hdiff_amd
import _attn_f32_cases as F
import test_gpu_attention_f32 as T
lib = hdiff_amd.lib()
only = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "all" else None
margin = float(sys.argv[2]) if len(sys.argv) > 2 else None
if margin is not None:
    F.margin_of = lambda family, name: margin
worst = {}
for case, family in F.RUNS:
    if only and family != only: continue
    t0 = time.time()
    try:
        reports = T.check_run(lib, case, family)
    except AssertionError as e:
        print(f"{F.case_id(case)} {family}: FAILED {str(e)[:600]}", flush=True)
        continue
    row = {n: (max(r[n]["max_x"] for r in reports), max(r[n]["rms_x"] for r in reports), max(r[n]["max"] / r[n]["mag"] if r[n]["mag"] else 0.0 for r in reports))
           for n in F.TENSORS}
    for n, v in row.items():
        w = worst.setdefault((family, n), [0.0, 0.0, ""])
        if max(v[:2]) > max(w[:2]): w[2] = F.case_id(case)
        w[0], w[1] = max(w[0], v[0]), max(w[1], v[1])
    print(f"{F.case_id(case)} {family} ({time.time() - t0:.1f} s): " + " | ".join(f"{n} max x{v[0]:.2f} rms x{v[1]:.2f} (max / mag {v[2]:.1e})" for n, v in row.items()), flush=True)
print("\nworst ratio to the fp32 CPU definition per (family, tensor): max error, rms error, where")
for (family, n), w in worst.items():
    print(f"{family:14s} {n:5s} max x{w[0]:.2f} rms x{w[1]:.2f}   {w[2]}")
