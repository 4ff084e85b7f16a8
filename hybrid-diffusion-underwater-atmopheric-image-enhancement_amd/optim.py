"""The optimizer tail of a training step on the HIP path: ``AdamW`` with the gradient clipping fused in.

Reference: ``TrainCondition.py:39-40`` builds ``torch.optim.AdamW(net_model.parameters(), lr, weight_decay=1e-4)`` and ``:61-63`` runs
``torch.nn.utils.clip_grad_norm_(net_model.parameters(), grad_clip); optimizer.step()`` after every backward.  Through round 5 this
harness did the same with torch's own kernels ("may stay torch-native at first"); this class is the native form:

    opt = hdiff_amd.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-4)
    ...
    loss.backward()
    total_norm = opt.step(max_grad_norm=1.0)      # == clip_grad_norm_(params, 1.0); optimizer.step(): three launches for all tensors

It is a ``torch.optim.Optimizer`` (param groups, ``zero_grad``, LR schedulers -- ``Scheduler.GradualWarmupScheduler`` and
``CosineAnnealingLR`` set ``group["lr"]`` -- and ``state_dict`` work as for torch's AdamW: per-parameter ``step`` / ``exp_avg`` /
``exp_avg_sq``, the moments being views into one flat buffer per group).  The arithmetic is torch's single-tensor AdamW in its order of
operations (``csrc/optimizer.hip``); the norm is ONE sum over all elements (fixed order, float64 final sum) instead of torch's norm of
per-tensor norms: the same number to fp32 rounding.  No CPU path: CPU parameters raise.

``step`` writes the parameters from a raw kernel, which autograd does not see; it then bumps their version counters (host only, no
launch), so a weight pack cached on ``p._version`` (``DynamicUNet.plan_for``, ``UNet.plan_for``) is rebuilt by the next forward.
``load_state_dict`` takes a state dict of this class or of ``torch.optim.AdamW`` (per-parameter ``step`` tensors on the CPU), copies the
moments into fresh flat buffers and drops the cached device tables, so a resumed run goes on exactly where the saved one stopped.

``EMA`` is the exponential moving average of the weights that a diffusion run samples from: the shadows are views into one flat fp32
buffer, ``update()`` is ONE ``hdiff_ema_update`` launch over all tensors.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch

from . import _capi


class AdamW(torch.optim.Optimizer):
    def __init__(self, params: Iterable, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2):
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0) or not (0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid hyper-parameters: lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self._lib = _capi.lib()
        self._chunk = int(self._lib.hdiff_opt_chunk())
        self._tables: dict = {}          # group index -> (signature, table tensor, chunk tensor, nchunks)
        self._scratch: Optional[torch.Tensor] = None
        self._norm_coef: Optional[torch.Tensor] = None
        self._chunk_cache: dict = {}     # (group, chunk table, cohort) -> the cohort's chunk list on the device

    # -- state: one flat buffer per group for each moment, the per-parameter entries are views (torch's state layout) ------------
    def _ensure_state(self, gi: int, group: dict) -> None:
        need = [p for p in group["params"] if p.requires_grad and "exp_avg" not in self.state[p]]
        if not need:
            return
        dev = need[0].device
        n = sum(p.numel() for p in need)
        m_flat, v_flat = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
        off = 0
        shared_step = torch.tensor(0.0)      # one counter object for the parameters that start together; a parameter that
        for p in need:                       # skips a step leaves it (step(): counts advance only with a gradient)
            st = self.state[p]
            st["step"] = shared_step
            st["exp_avg"] = m_flat[off:off + p.numel()].view_as(p)
            st["exp_avg_sq"] = v_flat[off:off + p.numel()].view_as(p)
            off += p.numel()

    def load_state_dict(self, state_dict) -> None:
        """A state dict of this class or of ``torch.optim.AdamW``.  The moments are copied into fresh flat buffers (torch's loader
        hands back the caller's own tensors where device and dtype already match), step counters become CPU tensors of their own
        -- those that were one object stay one object -- and the cached device tables are dropped."""
        super().load_state_dict(state_dict)
        self._tables.clear()
        self._chunk_cache.clear()
        counters: dict = {}
        for group in self.param_groups:
            have = [p for p in group["params"] if "exp_avg" in self.state.get(p, {})]
            if not have:
                continue
            n = sum(p.numel() for p in have)
            m_flat = torch.empty(n, dtype=torch.float32, device=have[0].device)
            v_flat = torch.empty(n, dtype=torch.float32, device=have[0].device)
            off = 0
            for p in have:
                st = self.state[p]
                for key, flat in (("exp_avg", m_flat), ("exp_avg_sq", v_flat)):
                    view = flat[off:off + p.numel()].view_as(p)
                    view.copy_(st[key])
                    st[key] = view
                off += p.numel()
                c = st["step"]
                if id(c) not in counters:
                    counters[id(c)] = (c, torch.tensor(float(c.item() if torch.is_tensor(c) else c)))
                st["step"] = counters[id(c)][1]

    def _table(self, gi: int, group: dict):
        ps = [p for p in group["params"] if p.grad is not None]
        for p in ps:
            if not p.is_cuda or p.dtype != torch.float32 or p.grad.dtype != torch.float32:
                raise RuntimeError("hdiff_amd.optim.AdamW runs on the GPU in fp32 only (there is no CPU path)")
            if not (p.is_contiguous() and p.grad.is_contiguous()):
                raise RuntimeError("hdiff_amd.optim.AdamW: parameters and gradients must be contiguous")
        sig = tuple((p.data_ptr(), p.grad.data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr(),
                     p.numel()) for p in ps)
        hit = self._tables.get(gi)
        if hit is not None and hit[0] == sig:
            return hit
        if not ps:
            self._tables[gi] = (sig, None, None, 0, ps)
            return self._tables[gi]
        tab = np.zeros((len(ps), 5), dtype=np.int64)
        chunks: List[Tuple[int, int]] = []
        for i, p in enumerate(ps):
            st = self.state[p]
            tab[i] = (p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel())
            chunks.extend((i, c) for c in range((p.numel() + self._chunk - 1) // self._chunk))
        dev = ps[0].device
        t_dev = torch.from_numpy(tab).to(dev)
        c_dev = torch.tensor(chunks, dtype=torch.int32).to(dev)
        self._tables[gi] = (sig, t_dev, c_dev, len(chunks), ps)
        return self._tables[gi]

    def _cohorts(self, group: dict, ps) -> List[Tuple[int, List[int], list]]:
        """[(next step count, indices into ps, [(counter, indices into ps, shared with a parameter outside ps?)])] in increasing
        count order.  Parameters that start together share one counter object while they keep stepping together."""
        holders: dict = {}
        for p in group["params"]:
            st = self.state.get(p)
            if st is not None and "step" in st:
                holders[id(st["step"])] = holders.get(id(st["step"]), 0) + 1
        objs: dict = {}
        for i, p in enumerate(ps):
            c = self.state[p]["step"]
            objs.setdefault(id(c), (c, []))[1].append(i)
        by: dict = {}
        for c, idx in objs.values():
            k = int(c.item()) if torch.is_tensor(c) else int(c)
            ent = by.setdefault(k, ([], []))
            ent[0].extend(idx)
            ent[1].append((c, idx, holders.get(id(c), 0) > len(idx)))
        return [(k + 1, sorted(by[k][0]), by[k][1]) for k in sorted(by)]

    def _cohort_chunks(self, gi: int, ps, idx: List[int], c_dev: torch.Tensor) -> torch.Tensor:
        """The chunk list of the tensors ``idx`` of the group's table (cached per table and cohort)."""
        key = (gi, c_dev.data_ptr(), tuple(idx))
        hit = self._chunk_cache.get(key)
        if hit is None:
            ch = [(i, c) for i in idx for c in range((ps[i].numel() + self._chunk - 1) // self._chunk)]
            hit = torch.tensor(ch, dtype=torch.int32).to(c_dev.device)
            if len(self._chunk_cache) > 64:
                self._chunk_cache.clear()
            self._chunk_cache[key] = hit
        return hit

    @torch.no_grad()
    def step(self, closure=None, max_grad_norm: Optional[float] = None):
        """One AdamW step; with ``max_grad_norm`` the gradients of ALL groups are first clipped to that global norm (in place, like
        ``clip_grad_norm_``) and the total norm (0-dim device tensor) is returned, otherwise the closure's loss / None."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        tables = []
        for gi, group in enumerate(self.param_groups):
            self._ensure_state(gi, group)
            tables.append(self._table(gi, group))
        total = sum(t[3] for t in tables)
        if total == 0:
            return loss
        dev = next(t[1] for t in tables if t[1] is not None).device
        stream = torch.cuda.current_stream(dev).cuda_stream
        coef_ptr = None
        if max_grad_norm is not None:
            if self._scratch is None or self._scratch.numel() < total or self._scratch.device != dev:
                self._scratch = torch.empty(total, dtype=torch.float32, device=dev)
                self._norm_coef = torch.empty(2, dtype=torch.float32, device=dev)
            if len([t for t in tables if t[3]]) == 1:
                _, t_dev, c_dev, n, _ = next(t for t in tables if t[3])
                _capi.check(self._lib.hdiff_grad_norm_clip_coef(t_dev.data_ptr(), c_dev.data_ptr(), n, self._scratch.data_ptr(),
                                                                C.c_float(float(max_grad_norm)), self._norm_coef.data_ptr(), stream),
                            "grad_norm_clip_coef")
            else:      # several groups: one table over all of them for the norm (built per call: rare, small)
                ps = [p for t in tables for p in t[4]]
                tab = np.array([(p.data_ptr(), p.grad.data_ptr(), 0, 0, p.numel()) for p in ps], dtype=np.int64)
                ch = [(i, c) for i, p in enumerate(ps) for c in range((p.numel() + self._chunk - 1) // self._chunk)]
                t_dev, c_dev = torch.from_numpy(tab).to(dev), torch.tensor(ch, dtype=torch.int32).to(dev)
                _capi.check(self._lib.hdiff_grad_norm_clip_coef(t_dev.data_ptr(), c_dev.data_ptr(), len(ch), self._scratch.data_ptr(),
                                                                C.c_float(float(max_grad_norm)), self._norm_coef.data_ptr(), stream),
                            "grad_norm_clip_coef")
                self._keep = (t_dev, c_dev)
            coef_ptr = self._norm_coef.data_ptr()
        for gi, (group, (_, t_dev, c_dev, n, ps)) in enumerate(zip(self.param_groups, tables)):
            if n == 0:
                continue
            b1, b2 = group["betas"]
            # cohorts of equal step count (torch's AdamW keeps one count per parameter and advances only those with a gradient:
            # a parameter that skips steps -- DynamicUNet's gated middle blocks -- falls behind), one launch per cohort
            for step, idx, counters in self._cohorts(group, ps):
                chunks = c_dev if len(idx) == len(ps) else self._cohort_chunks(gi, ps, idx, c_dev)
                _capi.check(self._lib.hdiff_adamw_step(t_dev.data_ptr(), chunks.data_ptr(), int(chunks.shape[0]), coef_ptr,
                                                       float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                                       float(group["weight_decay"]), step, stream), "adamw_step")
                for c, cidx, shared_outside in counters:
                    if torch.is_tensor(c) and not shared_outside:
                        c.fill_(float(step))
                    else:       # the counter's other holders took no step: these parameters go on with a counter of their own
                        fresh = torch.tensor(float(step))
                        for i in cidx:
                            self.state[ps[i]]["step"] = fresh
            torch.autograd.graph.increment_version(ps)      # the kernel wrote p behind autograd's back: caches keyed on p._version see it
        if max_grad_norm is not None:
            return self._norm_coef[0].clone()
        return loss


class EMA:
    """Exponential moving average of a list of parameters: ``shadow = shadow + (p - shadow) * (1 - decay)`` per ``update()``.

        ema = EMA(model.parameters(), decay=0.9999)    # shadow = a copy of the weights now
        ema.update()                                   # after every optimizer step; update(decay=d) overrides for this call
        with ema.average_parameters():                 # weights <- shadow inside, restored on exit (also on an exception)
            out = sampler(...)
        ema.copy_to()                                  # weights <- shadow, for good

    It covers ALL parameters handed in, whatever ``requires_grad`` says at that moment (``DynamicUNet`` flips it per batch).  GPU and
    fp32 only.  The weights are swapped with copies autograd sees, so weight packs cached on ``p._version`` are rebuilt."""

    def __init__(self, params: Iterable, decay: float = 0.9999):
        self.params: List[torch.Tensor] = [p for p in params]
        if not self.params:
            raise ValueError("hdiff_amd.optim.EMA: no parameters")
        self.decay = self._checked(decay)
        self.num_updates = 0
        self._check_params()
        self._lib = _capi.lib()
        self._chunk = int(self._lib.hdiff_opt_chunk())
        dev = self.params[0].device
        self._flat = torch.empty(sum(p.numel() for p in self.params), dtype=torch.float32, device=dev)
        self.shadow: List[torch.Tensor] = []
        off = 0
        for p in self.params:
            self.shadow.append(self._flat[off:off + p.numel()].view(p.shape))
            off += p.numel()
        with torch.no_grad():
            torch._foreach_copy_(self.shadow, [p.detach() for p in self.params])
        self._table = None            # (signature, table tensor, chunk tensor, nchunks)

    @staticmethod
    def _checked(decay) -> float:
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"hdiff_amd.optim.EMA: decay must be in [0, 1], got {decay}")
        return decay

    def _check_params(self) -> None:
        for p in self.params:
            if not p.is_cuda or p.dtype != torch.float32:
                raise RuntimeError("hdiff_amd.optim.EMA runs on the GPU in fp32 only (there is no CPU path)")
            if not p.is_contiguous():
                raise RuntimeError("hdiff_amd.optim.EMA: parameters must be contiguous")
            if p.device != self.params[0].device:
                raise RuntimeError("hdiff_amd.optim.EMA: parameters must be on one device")

    def _tables(self):
        sig = tuple((p.data_ptr(), s.data_ptr(), p.numel()) for p, s in zip(self.params, self.shadow))
        if self._table is not None and self._table[0] == sig:
            return self._table
        self._check_params()
        ps = [(p, s) for p, s in zip(self.params, self.shadow) if p.numel()]
        tab = np.array([(s.data_ptr(), p.data_ptr(), p.numel()) for p, s in ps], dtype=np.int64).reshape(len(ps), 3)
        chunks = [(i, c) for i, (p, _) in enumerate(ps) for c in range((p.numel() + self._chunk - 1) // self._chunk)]
        dev = self._flat.device
        self._table = (sig, torch.from_numpy(tab).to(dev), torch.tensor(chunks, dtype=torch.int32).reshape(len(chunks), 2).to(dev),
                       len(chunks))
        return self._table

    @torch.no_grad()
    def update(self, decay: Optional[float] = None) -> None:
        """One ``hdiff_ema_update`` launch over all tensors, on the current stream of the parameters' device."""
        d = self.decay if decay is None else self._checked(decay)
        _, t_dev, c_dev, n = self._tables()
        if n:
            stream = torch.cuda.current_stream(self._flat.device).cuda_stream
            with torch.cuda.device(self._flat.device):
                _capi.check(self._lib.hdiff_ema_update(t_dev.data_ptr(), c_dev.data_ptr(), n, C.c_double(d), stream), "ema_update")
        self.num_updates += 1

    @torch.no_grad()
    def copy_to(self, params: Optional[Iterable] = None) -> None:
        """weights <- shadow (``params``: another list of the same shapes, default the averaged parameters themselves)."""
        dst = self.params if params is None else [p for p in params]
        if len(dst) != len(self.shadow):
            raise ValueError(f"hdiff_amd.optim.EMA.copy_to: {len(dst)} parameters for {len(self.shadow)} shadows")
        torch._foreach_copy_([p for p in dst], self.shadow)      # in-place writes autograd sees: p._version moves

    @contextlib.contextmanager
    def average_parameters(self):
        """Inside: the parameters hold the shadow values.  On exit, also through an exception, they hold what they held before."""
        with torch.no_grad():
            flat, backup, off = torch.empty_like(self._flat), [], 0
            for p in self.params:
                backup.append(flat[off:off + p.numel()].view(p.shape))
                off += p.numel()
            torch._foreach_copy_(backup, [p.detach() for p in self.params])
            torch._foreach_copy_(self.params, self.shadow)
        try:
            yield self
        finally:
            with torch.no_grad():
                torch._foreach_copy_(self.params, backup)

    def state_dict(self) -> dict:
        return {"decay": self.decay, "num_updates": self.num_updates, "shadow": [s.clone() for s in self.shadow]}

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        shadow = list(sd["shadow"])
        if len(shadow) != len(self.shadow) or any(tuple(a.shape) != tuple(b.shape) for a, b in zip(shadow, self.shadow)):
            raise ValueError("hdiff_amd.optim.EMA.load_state_dict: the shadows do not match the parameters")
        self.decay = self._checked(sd["decay"])
        self.num_updates = int(sd["num_updates"])
        for dst, src in zip(self.shadow, shadow):
            dst.copy_(src)
        self._table = None

    def shadow_state_dict(self, model: torch.nn.Module) -> Dict[str, torch.Tensor]:
        """``model.state_dict()`` with every averaged parameter replaced by its shadow (clones; buffers and parameters that are not
        averaged are copied through): what a checkpoint file of the averaged weights holds."""
        by_id = {id(p): s for p, s in zip(self.params, self.shadow)}
        names = {name: by_id[id(p)] for name, p in model.named_parameters(remove_duplicate=False) if id(p) in by_id}
        if len({id(s) for s in names.values()}) != len(self.shadow):
            raise ValueError("hdiff_amd.optim.EMA.shadow_state_dict: the model does not hold every averaged parameter")
        return {k: (names[k] if k in names else v).detach().clone() for k, v in model.state_dict().items()}
