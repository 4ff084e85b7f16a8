"""The definitions the token-axis dense layer (hdiff_amd/dense.py, csrc/dense_tokens.hip) is held to.  Nothing of the package is imported.

``linear64``   Y[b, co, l] = bias[co] + sum_ci W[co, ci] X[b, ci, l] in float64: the reference.
``yardstick``  the same through torch's fp32 CPU ``F.linear``: the error an fp32 implementation is measured against (4x, as YARD in
               tests/test_gpu_dino.py).
``emulate``    the kernel's arithmetic in numpy: every fp32 operand as three bf16 pieces by truncation (``top16``: x = x0 + x1 + x2
               exactly), K padded to a multiple of 16 with zeros, per 16-channel chunk the six piece products with i + j <= 2, small ones
               first, each added to an fp32 accumulator (a product of two bf16 numbers is exact in fp32; the 16 products of one matrix
               instruction are summed in float64 here and rounded once with the accumulator -- the hardware's own order inside an
               instruction is not modelled), the bias added last in fp32.  ``drop=t`` leaves term ``t`` of ``TERMS`` out.
"""
import numpy as np
import torch
import torch.nn.functional as F

# (piece of W, piece of X) in the kernel's order
TERMS = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))

# (B, Cout, Cin, L): the smallest case; a batch with a short token axis; one below, at and one above each tile boundary (64 channels,
# 16 of K, 32 tokens); channels and tokens past one tile; the patch embedding's K; the real token count
SHAPES = ((1, 8, 12, 1), (2, 8, 12, 5), (3, 63, 15, 31), (3, 64, 16, 32), (3, 65, 17, 33), (2, 72, 48, 65), (1, 64, 588, 37),
          (2, 130, 64, 325))


def case(B, Cout, Cin, L):
    """seeded fp32 inputs: W ~ 0.05 N(0, 1), bias ~ 0.1 N(0, 1), X ~ N(0, 1)"""
    g = torch.Generator().manual_seed(((B * 1009 + Cout) * 1013 + Cin) * 1019 + L)
    w = 0.05 * torch.randn(Cout, Cin, generator=g)
    bias = 0.1 * torch.randn(Cout, generator=g)
    x = torch.randn(B, Cin, L, generator=g)
    return w, bias, x


def linear64(x, w, bias=None):
    y = torch.einsum("oc,bcl->bol", w.double(), x.double())
    return y if bias is None else y + bias.double().view(1, -1, 1)


def yardstick(x, w, bias=None):
    """torch's fp32 CPU F.linear on the token-major view -> (B, Cout, L)"""
    return F.linear(x.transpose(1, 2).contiguous(), w, bias).transpose(1, 2).contiguous()


def errors(got, ref):
    """(rms, max) of got - ref in float64"""
    e = (got.double() - ref).abs()
    return float(e.pow(2).mean().sqrt()), float(e.max())


def top16(a):
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def split3(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    p0 = top16(a)
    r = (a - p0).astype(np.float32)
    p1 = top16(r)
    s = (r - p1).astype(np.float32)
    return p0, p1, top16(s)


def emulate(x, w, bias=None, drop=None):
    xn, wn = x.numpy().astype(np.float32), w.numpy().astype(np.float32)
    B, Cin, L = xn.shape
    Cout = wn.shape[0]
    K = -(-Cin // 16) * 16
    xp = np.zeros((B, K, L), np.float32)
    xp[:, :Cin] = xn
    wp = np.zeros((Cout, K), np.float32)
    wp[:, :Cin] = wn
    xs, ws = split3(xp), split3(wp)
    assert np.array_equal((xs[0].astype(np.float64) + xs[1] + xs[2]).astype(np.float32), xp)       # the split is exact
    acc = np.zeros((B, Cout, L), np.float32)
    for c in range(K // 16):
        k = slice(16 * c, 16 * c + 16)
        for t, (i, j) in enumerate(TERMS):
            if t == drop:
                continue
            prod = np.einsum("ok,bkl->bol", ws[i][:, k].astype(np.float64), xs[j][:, k].astype(np.float64))
            acc = (acc.astype(np.float64) + prod).astype(np.float32)
    if bias is not None:
        acc = (acc + bias.numpy().astype(np.float32).reshape(1, -1, 1)).astype(np.float32)
    return torch.from_numpy(acc)
