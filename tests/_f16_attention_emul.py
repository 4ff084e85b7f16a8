"""The yardstick of the "f16" contraction mode: an emulation of the FORMAT (the text at the top of csrc/attention_f16.hip), in torch
float64, on CPU or GPU tensors -- never of the code under test.

    q = fp16(Q qscale 2^-a), k = fp16(K 2^a)     a per (sample, head) from the maxima of the head's Q and K rows
    v = fp16(V 2^s)                              s per channel row, max |V 2^s| in [2^14, 2^15)
    S = k . q, P = exp2(S - m)                   float64;  m = the row maximum - 8 + offset
    P -> 11 significant bits, unbounded exponent (the kernel's moving reference keeps every P that matters a normal fp16 number)
    O = v . P_rounded / sum(P) 2^-s

Its error against exact float64 attention of the UNROUNDED inputs is what the format costs; the kernel may add only fp32
accumulation.  Where m falls inside a binade changes how P rounds and the kernel's rows fall everywhere, so the yardstick is the
LARGEST error over the offsets k / 8, k = 0 .. 7 (`yardstick`).
"""
import contextlib
import math

import torch

OFFSETS8 = tuple(k / 8 for k in range(8))
_CHUNK_ELEMS = 1 << 26          # scores held at once (float64): 512 MiB per temporary


def _qscale32(d):
    return (torch.tensor(1.4426950408889634, dtype=torch.float32) / torch.sqrt(torch.tensor(float(d), dtype=torch.float32))).item()


def _exp_field(x32):
    """biased exponent field of a positive float32 scalar tensor (0: zero / denormal, 255: inf / NaN)"""
    return int((x32.reshape(1).view(torch.int32).item() >> 23) & 0xFF)


def balance(q_head, k_head, qscale):
    """a of one (sample, head): k 2^a, q 2^-a put the two maxima in the same binade (qk_split_h2_kernel's rule)"""
    mq = q_head.abs().amax().float() * torch.tensor(qscale, dtype=torch.float32, device=q_head.device)
    mk = k_head.abs().amax().float()
    eq, ek = _exp_field(mq), _exp_field(mk)
    if eq in (0, 255) or ek in (0, 255):
        return 0
    a = int(math.trunc((eq - ek) / 2))          # C integer division
    return max(-60, min(60, a))


def v_scale_exponent(v_head):
    """s per channel row of v_head [d, L]: 14 - clamp(exponent of max |v|, -100, 127)"""
    amax = v_head.abs().amax(dim=1).float()
    e = ((amax.view(torch.int32) >> 23) & 0xFF) - 127
    return 14 - e.clamp(-100, 127)


def round_sig11(p):
    """round to 11 significant bits (fp16's significand), exponent unbounded, ties to even"""
    mant, e = torch.frexp(p)
    return torch.ldexp(torch.round(mant * 2048.0) / 2048.0, e)


def _heads(qkv, heads):
    B, C3, L = qkv.shape
    Cc = C3 // 3
    d = Cc // heads
    q, k, v = [z.reshape(B, heads, d, L) for z in qkv.split(Cc, dim=1)]
    return B, Cc, L, d, q, k, v


def exact(qkv, heads):
    """float64 attention of the unrounded inputs, [B, C, L] float64 (chunked over the queries)"""
    B, Cc, L, d, q, k, v = _heads(qkv, heads)
    out = torch.empty(B, heads, d, L, dtype=torch.float64, device=qkv.device)
    step = max(1, _CHUNK_ELEMS // L)
    for b in range(B):
        for h in range(heads):
            qh, kh, vh = q[b, h].double(), k[b, h].double(), v[b, h].double()
            for q0 in range(0, L, step):
                s = (qh[:, q0:q0 + step].t() @ kh) / math.sqrt(d)
                w = torch.softmax(s, dim=-1)
                out[b, h, :, q0:q0 + step] = vh @ w.t()
    return out.reshape(B, Cc, L)


def emulate(qkv, heads, offset=0.0):
    """the format, [B, C, L] float64"""
    B, Cc, L, d, q, k, v = _heads(qkv, heads)
    qscale = _qscale32(d)
    out = torch.empty(B, heads, d, L, dtype=torch.float64, device=qkv.device)
    step = max(1, _CHUNK_ELEMS // L)
    for b in range(B):
        for h in range(heads):
            a = balance(q[b, h], k[b, h], qscale)
            qh = (q[b, h].double() * (qscale * 2.0 ** -a)).half().double()          # [d, L]
            kh = (k[b, h].double() * 2.0 ** a).half().double()
            s_exp = v_scale_exponent(v[b, h]).double()                               # [d]
            vh = (v[b, h].double() * torch.exp2(s_exp)[:, None]).half().double()
            for q0 in range(0, L, step):
                s = qh[:, q0:q0 + step].t() @ kh                                     # [queries, keys], log2 domain
                m = s.amax(dim=1, keepdim=True) - 8.0 + offset
                p = torch.exp2(s - m)
                l = p.sum(dim=1)
                o = vh @ round_sig11(p).t()                                          # [d, queries]
                out[b, h, :, q0:q0 + step] = o / l[None, :] * torch.exp2(-s_exp)[:, None]
    return out.reshape(B, Cc, L)


def errors(got, ref, per_pair_heads=None):
    """(rms, worst) of got - ref, each channel row divided by its largest |ref|; with per_pair_heads = heads also the lists per
    (sample, head)"""
    ref = ref.double()
    scale = ref.abs().amax(dim=2, keepdim=True).clamp_min(1e-300)
    e = (got.double().to(ref.device) - ref) / scale
    rms, worst = e.pow(2).mean().sqrt().item(), e.abs().max().item()
    if per_pair_heads is None:
        return rms, worst
    B, Cc, L = ref.shape
    ep = e.reshape(B * per_pair_heads, -1)
    return rms, worst, ep.pow(2).mean(dim=1).sqrt().tolist(), ep.abs().amax(dim=1).tolist()


def yardstick(qkv, heads, ref=None, offsets=OFFSETS8):
    """the largest emulation error over the offsets: (rms, worst, rms per pair, worst per pair)"""
    ref = exact(qkv, heads) if ref is None else ref
    best = None
    for off in offsets:
        r = errors(emulate(qkv, heads, off), ref, per_pair_heads=heads)
        if best is None:
            best = [r[0], r[1], list(r[2]), list(r[3])]
        else:
            best[0], best[1] = max(best[0], r[0]), max(best[1], r[1])
            best[2] = [max(x, y) for x, y in zip(best[2], r[2])]
            best[3] = [max(x, y) for x, y in zip(best[3], r[3])]
    return tuple(best)


@contextlib.contextmanager
def oracle_with_emulated_attention(offset):
    """oracle.cpu_path with the attention CORE of its mha_self_attention replaced by `emulate` where the f16 mode acts (L >= 512,
    L % 256 == 0, d_head 16 / 32); the projections stay the oracle's own.  The oracle's file is untouched: the module attribute is
    swapped for the duration of the block."""
    from oracle import cpu_path as O
    orig = O.mha_self_attention

    def mha(x_lbc, in_w, in_b, out_w, out_b, num_heads, q_chunk=1024):
        L, B, Cc = x_lbc.shape
        if L < 512 or L % 256 != 0 or Cc // num_heads not in (16, 32):
            return orig(x_lbc, in_w, in_b, out_w, out_b, num_heads, q_chunk)
        qkv = (x_lbc @ in_w.t() + in_b).permute(1, 2, 0).contiguous()            # (B, 3C, L): the kernels' layout
        o = emulate(qkv, num_heads, offset).to(x_lbc.dtype).permute(2, 0, 1)      # (L, B, C)
        return o @ out_w.t() + out_b

    O.mha_self_attention = mha
    try:
        yield
    finally:
        O.mha_self_attention = orig
