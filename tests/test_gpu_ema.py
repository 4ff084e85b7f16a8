"""hdiff_ema_update (csrc/optimizer.hip) and hdiff_amd.optim.EMA on the GPU, the weight-pack cache after a raw-kernel write of the
weights (optim.AdamW.step, EMA swaps), and optim.AdamW.load_state_dict going on stepping."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hdiff_amd  # noqa: E402
from hdiff_amd import _capi  # noqa: E402
from hdiff_amd import optim as HO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 12345.0
SIZES = [1, 63, 4095, 4096, 4097, 2 * 4096 + 5] + [1 + (7 * i) % 23 for i in range(40)]


def odd_views(seed, scale):
    """One flat buffer per side, every tensor a view at an ODD element offset, the gaps (and both ends) filled with a sentinel."""
    offsets, pos = [], 1
    for n in SIZES:
        offsets.append(pos)
        pos += n + 2
        pos += 1 - pos % 2
    g = torch.Generator().manual_seed(seed)
    flat = torch.full((pos + 3,), SENTINEL)
    inside = torch.zeros(pos + 3, dtype=torch.bool)
    for off, n in zip(offsets, SIZES):
        flat[off:off + n] = torch.randn(n, generator=g) * scale
        inside[off:off + n] = True
    flat = flat.to(DEV)
    return flat, [flat[off:off + n] for off, n in zip(offsets, SIZES)], inside.to(DEV)


def launch(avg, p, decay):
    lib = _capi.lib()
    chunk = int(lib.hdiff_opt_chunk())
    assert chunk == 4096                     # the sizes above straddle it
    tab = np.array([(a.data_ptr(), q.data_ptr(), a.numel()) for a, q in zip(avg, p)], dtype=np.int64)
    chunks = [(i, c) for i, a in enumerate(avg) for c in range((a.numel() + chunk - 1) // chunk)]
    t_dev, c_dev = torch.from_numpy(tab).to(DEV), torch.tensor(chunks, dtype=torch.int32).to(DEV)
    _capi.check(lib.hdiff_ema_update(t_dev.data_ptr(), c_dev.data_ptr(), len(chunks), C.c_double(decay),
                                     torch.cuda.current_stream().cuda_stream), "ema_update")
    torch.cuda.synchronize()
    return len(chunks)


@pytest.mark.parametrize("decay", [0.9999, 0.5, 0.0, 1.0])
def test_kernel_bit_for_bit_against_separate_torch_operations(decay):
    """Three consecutive updates equal ``avg + (p - avg) * w`` evaluated as separate fp32 torch operations with
    w = float32(1.0 - decay); views at odd element offsets (4-byte alignment only), tensors of 1 .. 2 chunks + 5 elements and 40 small
    ones; nothing outside a view is written."""
    avg_flat, avg, inside = odd_views(1, 0.3)
    p_flat, p, _ = odd_views(2, 0.3)
    assert all(a.data_ptr() % 8 == 4 for a in avg) and all(q.data_ptr() % 8 == 4 for q in p)
    w = torch.tensor(np.float32(1.0 - decay), device=DEV)
    assert w.dtype == torch.float32
    want = [a.clone() for a in avg]
    start = [a.clone() for a in avg]
    g = torch.Generator().manual_seed(3)
    for k in range(3):
        for q in p:
            q.add_((torch.randn(q.numel(), generator=g) * 0.1).to(DEV))      # the weights move between updates
        nchunks = launch(avg, p, decay)
        assert nchunks == sum((n + 4095) // 4096 for n in SIZES)
        for i, (r, q) in enumerate(zip(want, p)):
            d = q - r
            u = d * w
            want[i] = r + u
        for i, (a, r) in enumerate(zip(avg, want)):
            assert torch.equal(a, r), (decay, k, SIZES[i], (a - r).abs().max().item())
    if decay == 1.0:
        assert all(torch.equal(a.view(torch.int32), s.view(torch.int32)) for a, s in zip(avg, start))       # untouched
    elif decay == 0.0:
        assert all((a - q).abs().max().item() <= 2 ** -22 for a, q in zip(avg, p))      # w = 1: a + (p - a), two roundings below 4
    else:
        assert not any(torch.equal(a, s) for a, s in zip(avg, start))
    assert bool((avg_flat[~inside] == SENTINEL).all()) and bool((p_flat[~inside] == SENTINEL).all())


def test_kernel_refuses_a_decay_outside_the_unit_interval():
    avg_flat, avg, _ = odd_views(1, 0.3)
    _, p, _ = odd_views(2, 0.3)
    before = avg_flat.clone()
    for bad in (-0.1, 1.0001, float("nan")):
        with pytest.raises(RuntimeError):
            launch(avg, p, bad)
    assert torch.equal(avg_flat, before)


def tiny_net(seed):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(5, 70), torch.nn.Linear(70, 61), torch.nn.Linear(61, 3)).to(DEV)
    net[1].weight.requires_grad_(False)
    return net


def drift(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.add_((torch.randn(p.shape, generator=g) * 0.05).to(DEV))


def test_class_shadow_covers_every_parameter_and_resumes():
    net = tiny_net(0)
    ema = HO.EMA(net.parameters(), decay=0.9)
    params = list(net.parameters())
    assert len(ema.shadow) == len(params) and all(torch.equal(s, p.detach()) for s, p in zip(ema.shadow, params))
    assert all(s.data_ptr() != p.data_ptr() for s, p in zip(ema.shadow, params))
    lo, hi = ema._flat.data_ptr(), ema._flat.data_ptr() + 4 * ema._flat.numel()
    assert all(lo <= s.data_ptr() < hi for s in ema.shadow) and ema._flat.numel() == sum(p.numel() for p in params)
    w = torch.tensor(np.float32(1.0 - 0.9), device=DEV)
    want = [s.clone() for s in ema.shadow]
    for k in range(2):
        drift(net, 10 + k)
        ema.update()
        want = [r + (p.detach() - r) * w for r, p in zip(want, params)]
    assert ema.num_updates == 2
    assert all(torch.equal(s, r) for s, r in zip(ema.shadow, want))
    frozen = [i for i, p in enumerate(params) if not p.requires_grad]
    assert frozen and not torch.equal(ema.shadow[frozen[0]], params[frozen[0]].detach())       # averaged, not skipped or copied
    # a per-call decay
    sd = ema.state_dict()
    assert set(sd) == {"decay", "num_updates", "shadow"} and sd["decay"] == 0.9 and sd["num_updates"] == 2
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(sd["shadow"], ema.shadow))
    # state_dict -> fresh EMA -> load_state_dict -> update equals the uninterrupted one
    fresh = HO.EMA(net.parameters(), decay=0.5)
    fresh.load_state_dict(sd)
    assert fresh.decay == 0.9 and fresh.num_updates == 2
    drift(net, 12)
    ema.update()
    fresh.update()
    assert fresh.num_updates == 3 and all(torch.equal(a, b) for a, b in zip(fresh.shadow, ema.shadow))
    half = torch.tensor(np.float32(0.5), device=DEV)
    want = [r + (p.detach() - r) * half for r, p in zip(ema.shadow, params)]
    ema.update(decay=0.5)
    assert ema.decay == 0.9 and all(torch.equal(s, r) for s, r in zip(ema.shadow, want))


def test_class_follows_reallocated_parameters():
    net = tiny_net(1)
    ema = HO.EMA(net.parameters(), decay=0.75)
    drift(net, 20)
    ema.update()
    old = [p.data for p in net.parameters()]          # kept alive: the new tensors cannot land on the old addresses
    for p, v in zip(net.parameters(), old):
        p.data = v.clone()                            # what load_state_dict into new tensors / a device round trip leaves
    assert all(p.data_ptr() != v.data_ptr() for p, v in zip(net.parameters(), old))
    drift(net, 21)
    w = torch.tensor(np.float32(0.25), device=DEV)
    want = [r + (p.detach() - r) * w for r, p in zip(ema.shadow, net.parameters())]
    ema.update()
    assert all(torch.equal(s, r) for s, r in zip(ema.shadow, want))
    # the swaps: inside the context the weights are the shadows, afterwards the originals, also through an exception
    before = [p.detach().clone() for p in net.parameters()]
    with pytest.raises(KeyError):
        with ema.average_parameters():
            assert all(torch.equal(p.detach(), s) for p, s in zip(net.parameters(), ema.shadow))
            raise KeyError("inside")
    assert all(torch.equal(p.detach(), b) for p, b in zip(net.parameters(), before))
    ema.copy_to()
    assert all(torch.equal(p.detach(), s) for p, s in zip(net.parameters(), ema.shadow))
    sd = ema.shadow_state_dict(net)
    assert list(sd) == list(net.state_dict()) and all(torch.equal(sd[k], v) for k, v in net.state_dict().items())


# -- no stale weight pack ---------------------------------------------------------------------------------------------------------
def small_unet():
    from _tree_b_small import load_small_dyn_unet
    d, cfg, m, _ = load_small_dyn_unet()
    x, t = torch.from_numpy(d["s16/x"]).to(DEV), torch.from_numpy(d["s16/t"]).to(DEV)
    return cfg, m.to(DEV).eval(), x, t


def fresh_output(cfg, state_dict, x, t):
    from hdiff_amd.diffusion.Model import DynamicUNet
    fresh = DynamicUNet(**cfg).to(DEV).eval()
    fresh.load_state_dict(state_dict)
    with torch.no_grad():
        return fresh(x, t)


def test_no_stale_pack_through_the_ema_swaps():
    cfg, m, x, t = small_unet()
    ema = HO.EMA(m.parameters(), decay=0.5)
    drift(m, 30)                              # the weights move away from the shadow
    ema.update()
    with torch.no_grad():
        before = m(x, t)                      # a pack of the raw weights exists from here on
        with ema.average_parameters():
            inside = m(x, t)
        after = m(x, t)
    want_inside = fresh_output(cfg, ema.shadow_state_dict(m), x, t)
    assert not torch.equal(before, want_inside)
    assert torch.equal(inside, want_inside)
    assert torch.equal(after, before)
    ema.copy_to()
    with torch.no_grad():
        assert torch.equal(m(x, t), want_inside)


def test_no_stale_pack_after_an_optimizer_step():
    cfg, m, x, t = small_unet()
    opt = HO.AdamW(m.parameters(), lr=1e-2, weight_decay=1e-4)
    with torch.no_grad():
        first = m(x, t)
    g = torch.Generator().manual_seed(31)
    for p in m.parameters():
        if p.requires_grad:                   # the forward above gated one pair of middle blocks off
            p.grad = torch.randn(p.shape, generator=g).to(DEV)
    opt.step(max_grad_norm=1.0)
    with torch.no_grad():
        second = m(x, t)
    want = fresh_output(cfg, m.state_dict(), x, t)
    assert not torch.equal(first, want)
    assert torch.equal(second, want)


# -- optimizer resume -------------------------------------------------------------------------------------------------------------
SHAPES = [(1,), (3, 7), (4097,), (16, 3, 3, 3), (2, 4096)]
LATE = 2                                      # this tensor receives its first gradient on step 2


def resume_params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(*s, generator=g) * 0.3).to(DEV)) for s in SHAPES]


def resume_grads():
    g = torch.Generator().manual_seed(41)
    return [[(torch.randn(*s, generator=g) * (10.0 ** (k % 3 - 1))).to(DEV) for s in SHAPES] for k in range(6)]


def take_steps(opt, params, grads, first, count, clip):
    for k in range(first, first + count):
        for i, p in enumerate(params):        # gradients are written in place, so their addresses stay (the device tables are reused)
            if i == LATE and k < 1:
                p.grad = None
                continue
            if p.grad is None:
                p.grad = torch.empty_like(p)
            p.grad.copy_(grads[k][i])
        opt.param_groups[0]["lr"] = 1e-3 * (1.0 + 0.5 * k)
        if isinstance(opt, HO.AdamW):
            opt.step(max_grad_norm=clip)
        else:
            torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], clip)
            opt.step()


def test_adamw_state_dict_loads_into_a_fresh_instance_and_goes_on():
    """3 steps, state_dict(), a fresh optimizer over fresh parameter tensors, 3 more steps: parameters, moments and step counts equal
    6 uninterrupted steps bit for bit.  The state dict goes through torch.save, as a checkpoint does."""
    import io
    grads = resume_grads()
    pa = resume_params(40)
    whole = HO.AdamW(pa, lr=1e-3, weight_decay=1e-4)
    take_steps(whole, pa, grads, 0, 6, 0.5)

    pb = resume_params(40)
    one = HO.AdamW(pb, lr=1e-3, weight_decay=1e-4)
    take_steps(one, pb, grads, 0, 3, 0.5)
    buf = io.BytesIO()
    torch.save({"opt": one.state_dict(), "params": [p.detach() for p in pb]}, buf)
    buf.seek(0)
    saved = torch.load(buf, map_location="cpu", weights_only=False)
    pc = [torch.nn.Parameter(v.to(DEV)) for v in saved["params"]]
    two = HO.AdamW(pc, lr=1e-3, weight_decay=1e-4)
    two.load_state_dict(saved["opt"])
    take_steps(one, pb, grads, 3, 1, 0.5)          # the first instance goes on: it shares nothing with the second
    take_steps(two, pc, grads, 3, 3, 0.5)
    for i, (x, y) in enumerate(zip(pa, pc)):
        assert torch.equal(x.detach(), y.detach()), i
        sx, sy = whole.state[x], two.state[y]
        assert torch.equal(sx["exp_avg"], sy["exp_avg"]) and torch.equal(sx["exp_avg_sq"], sy["exp_avg_sq"]), i
        assert int(sx["step"]) == int(sy["step"]) == (5 if i == LATE else 6), i

    # loading into an instance that has already stepped (its device tables are cached on the old state's pointers)
    take_steps(one, pb, grads, 4, 1, 0.5)
    pd = [torch.nn.Parameter(v.to(DEV)) for v in saved["params"]]
    again = HO.AdamW(pd, lr=1e-3, weight_decay=1e-4)
    for p in pd:
        p.grad = torch.zeros_like(p)
    again.step(max_grad_norm=0.5)
    with torch.no_grad():
        for p, v in zip(pd, saved["params"]):
            p.copy_(v)
    again.load_state_dict(saved["opt"])
    take_steps(again, pd, grads, 3, 3, 0.5)
    assert all(torch.equal(x.detach(), y.detach()) for x, y in zip(pa, pd))


def test_adamw_goes_on_from_a_torch_adamw_checkpoint():
    """3 steps of torch.optim.AdamW, its state dict (per-parameter CPU ``step`` tensors) loaded into the native class, 3 more steps
    on both sides: the criterion of test_gpu_optimizer.py's multi-step comparison (1e-6 of the tensor's scale)."""
    grads = resume_grads()
    pa, pb = resume_params(42), resume_params(42)
    ref = torch.optim.AdamW(pb, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    take_steps(ref, pb, grads, 0, 3, 0.5)
    with torch.no_grad():
        for x, y in zip(pa, pb):
            x.copy_(y)
    ours = HO.AdamW(pa, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    ours.load_state_dict(ref.state_dict())
    assert all(not ours.state[x]["step"].is_cuda for x in pa)
    for k in range(3, 6):
        take_steps(ref, pb, grads, k, 1, 0.5)
        take_steps(ours, pa, grads, k, 1, 0.5)
        for i, (x, y) in enumerate(zip(pa, pb)):
            scale = max(1e-3, y.detach().abs().max().item())
            assert (x.detach() - y.detach()).abs().max().item() <= 1e-6 * scale, (k, x.shape)
            sx, sy = ours.state[x], ref.state[y]
            assert (sx["exp_avg"] - sy["exp_avg"]).abs().max().item() <= 1e-6 * max(1e-30, sy["exp_avg"].abs().max().item())
            assert (sx["exp_avg_sq"] - sy["exp_avg_sq"]).abs().max().item() <= 1e-6 * max(1e-30, sy["exp_avg_sq"].abs().max().item())
            assert int(sx["step"].item()) == int(sy["step"].item()) == (k if i == LATE else k + 1)
    # the reference's moments were not written through (the loader copies them)
    assert all(ours.state[x]["exp_avg"].data_ptr() != ref.state[y]["exp_avg"].data_ptr() for x, y in zip(pa, pb))
