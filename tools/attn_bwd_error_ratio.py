"""Dev tool (round 5): error class of the split-operand attention BACKWARD -- rms and worst error of dQ, dK, dV against float64 as
ratios to the fp32-input kernel's, over all (sample, head) pairs and for the worst pair, for plain and adversarial inputs; and the
denominator: the fp32-input kernel's own error as a ratio to the fp32 CPU definition's ("f32 kernel / fp32 CPU", tests/_attn_f32_cases.py)
(tests/_attn_bwd_cases.py; the gates of tests/test_gpu_backward.py come from this table).
   python3 tools/attn_bwd_error_ratio.py [d = 16] [L = 2048] [B = 2] [seed offset = 0] [case = all]     (HDIFF_LIB selects a variant library, e.g. a mutant)
   python3 tools/attn_bwd_error_ratio.py multiblock [file = profiles/attention_bwd_h2_multiblock_error_ratio.txt]
       the (case, family) runs of tests/_attn_bwd_h2_cases.py -- key ranges of 2, 3 and 4 blocks, the backward alone on O and lse2 from
       float64 -- per tensor: every ratio that tests/test_gpu_attn_bwd_h2.py gates, to the fp32-input kernel and to the fp32 CPU definition"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, hdiff_amd
import _attn_bwd_cases as K
lib = hdiff_amd.lib()
if len(sys.argv) > 1 and sys.argv[1] == "multiblock":
    import _attn_bwd_h2_cases as H
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "attention_bwd_h2_multiblock_error_ratio.txt")
    lines = ["# split-operand attention backward, key ranges of several blocks (tools/attn_bwd_error_ratio.py multiblock, " + torch.cuda.get_device_name(0) + ")",
             "# error against float64 of the referenced base pairs as a ratio: 'f32 kernel' to the fp32-input kernel's (the gates of",
             "# tests/test_gpu_attn_bwd_h2.py: all-rms 1.25, all-worst 3, pair-rms 1.25 plain / 4 else, pair-worst 4 plain, worst-of-mag 2e-5 else),",
             "# 'fp32 CPU' to the fp32 CPU definition's (torch float32); pair-*: the worst pair; worst-of-mag: worst error / max |ref|",
             "# case (nsplit ranges x per blocks) family tensor | f32 kernel: all-rms all-worst pair-rms pair-worst | fp32 CPU: all-rms all-worst pair-rms pair-worst | worst-of-mag"]
    for case, family in H.RUNS:
        rep, rep_yard, _ = H.measure(lib, case, family, with_yard=True)
        for n in H.TENSORS:
            cols = lambda r: " ".join(f"{r[n][ch]:8.3f}" for ch in H.CHECKS[:4])
            lines.append(f"{H.case_id(case):13s} ({case.nsplit:2d} x {case.per}) {family:14s} {n} | {cols(rep)} | {cols(rep_yard)} | {rep[n]['worst-of-mag']:.2e}")
            print(lines[-1], flush=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(0)
d = int(sys.argv[1]) if len(sys.argv) > 1 else 16
L = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
B = int(sys.argv[3]) if len(sys.argv) > 3 else 2
seed = int(sys.argv[4]) if len(sys.argv) > 4 else 0
only = sys.argv[5] if len(sys.argv) > 5 else None
heads = 8
for name in K.CASES:
    if only and name != only: continue
    g = torch.Generator().manual_seed(7 + d + 1000 * seed)
    qkv, d_o = K.make_case(name, d, L, B, heads, g)
    st = K.error_stats(lib, qkv.to(K.DEV), d_o.to(K.DEV), heads, yard=True)
    row = []
    for n, s in st.items():
        pr = max(p[2] / p[3] for p in s["pair"]); pw = max(p[4] / p[5] for p in s["pair"])
        row.append(f"{n}: all pairs rms x{s['rms'][0] / s['rms'][1]:.2f} worst x{s['worst'][0] / s['worst'][1]:.2f} (worst / mag {s['worst'][0] / s['mag']:.1e}); worst pair rms x{pr:.2f} worst x{pw:.2f}; f32 kernel / fp32 CPU rms x{s['rms'][1] / max(s['yard'][0], 1e-300):.2f} worst x{s['worst'][1] / max(s['yard'][1], 1e-300):.2f}")
    print(f"d {d} L {L} B {B} seed {seed} {name}: " + " | ".join(row), flush=True)
