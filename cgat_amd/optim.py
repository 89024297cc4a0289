"""Fused optimiser steps, losses with step metrics and the cyclical learning-rate schedule -- the
per-step work after the hot path, behind the reference's own names.

  FusedSGD    <->  torch.optim.SGD(parameters, lr, weight_decay, momentum)  CGAT/lightning_module.py:320-323
  FusedAdam   <->  torch.optim.Adam(parameters, lr, weight_decay)         CGAT/lightning_module.py:325-327
  FusedAdamW  <->  torch.optim.AdamW(parameters, lr, weight_decay)        CGAT/lightning_module.py:328-331
  FusedLamb   <->  CGAT.lambs.JITLamb(parameters, lr, weight_decay)       CGAT/lightning_module.py:332-335, lambs.py:155-262
  RobustL1 / RobustL2                                                     CGAT/utils.py:30-47
  L1Loss / MSELoss  <->  nn.L1Loss() / nn.MSELoss()                       CGAT/lightning_module.py:137-142
  criterion_with_metrics: criterion + mae + rmse of a step in one launch  CGAT/lightning_module.py:153-159, 240-243
  cyclical_lr                                                             CGAT/utils.py:50-64

Each optimiser step is ONE kernel launch over all parameter tensors (three for LAMB, which needs per-tensor norms)
through the C ABI (`cgat_sgd_step`, `cgat_adam_step`, `cgat_adamw_step`, `cgat_lamb_step`): a device table of
(param, grad, first moment or momentum buffer, second moment, n) plus a list of fixed-size chunks.  No CPU fallback."""
import math

import numpy as np
import torch

from . import _lib

C = _lib.C


class _MultiTensor(torch.optim.Optimizer):
    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._plan = {}
        self._live_grads = []

    def _tensors(self, group):
        ps = [p for p in group["params"] if p.grad is not None]
        for p in ps:
            if not p.is_cuda or p.dtype != torch.float32 or p.grad.is_sparse:
                raise RuntimeError(f"{type(self).__name__} handles dense fp32 parameters on the GPU (no CPU fallback)")
            if not p.is_contiguous():
                raise RuntimeError("parameters must be contiguous")
            self._advance_state(p, group)
        return ps

    def _advance_state(self, p, group):
        """Per-class state: create what is missing and count the step.  This one is the Adam family's."""
        st = self.state[p]
        if len(st) == 0:
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        # a state loaded from torch.optim.Adam(W) carries `step` as a tensor: same name, normalised to an int here
        st["step"] = int(st["step"]) + 1

    def _moment_ptrs(self, p, group):
        """The table's (m, v) pointers of one parameter; 0 where the step kernel reads no such buffer."""
        st = self.state[p]
        return st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()

    def _launch_plan(self, ps, group):
        """Chunk list (cached per set of parameter sizes) and the per-step pointer table."""
        key = tuple(p.numel() for p in ps)
        dev = ps[0].device
        if key not in self._plan:
            ch = _lib.lib.cgat_mt_chunk_elems()
            ct, co, first = [], [], [0]
            for i, n in enumerate(key):
                offs = np.arange(0, max(n, 1), ch, dtype=np.int64) if n > 0 else np.zeros(0, np.int64)
                ct.append(np.full(offs.size, i, np.int32)); co.append(offs)
                first.append(first[-1] + offs.size)
            self._plan[key] = (torch.from_numpy(np.concatenate(ct)).to(dev), torch.from_numpy(np.concatenate(co)).to(dev),
                               torch.from_numpy(np.asarray(first, np.int32)).to(dev), first[-1])
        tab = np.empty((len(ps), 5), np.int64)
        # re-laid (non-contiguous) gradients stay alive until the NEXT step's launch has been queued; not in
        # self.state: state_dict() must hold exactly torch's entries (AdamW: step, exp_avg, exp_avg_sq)
        live = []
        for i, p in enumerate(ps):
            g = p.grad
            if not g.is_contiguous():
                g = g.contiguous()
                live.append(g)
            tab[i] = (p.data_ptr(), g.data_ptr(), *self._moment_ptrs(p, group), p.numel())
        self._live_grads = live
        # pinned staging: from pageable memory the upload is a synchronous copy -- the one host synchronisation a training
        # step still had (tools/sync_probe.py); the caching host allocator keeps the pinned block until the copy has run
        return self._plan[key], torch.from_numpy(tab).pin_memory().to(dev, non_blocking=True)


def _refuse_options(name, group, **unused):
    """Options of torch's optimisers that the reference's harness never sets: refused, also when a loaded state dict
    brings them in its param_groups."""
    for k, off in unused.items():
        if group.get(k, off) != off:
            raise NotImplementedError(f"{k}={group[k]!r} is not used by the reference's harness: {name} does not build it")


class _AdamFamily(_MultiTensor):
    """The step shared by FusedAdam and FusedAdamW: one launch of `_entry`, which differ in the decay form only."""

    _entry = None
    _UNUSED = {}

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        for group in self.param_groups:
            _refuse_options(type(self).__name__, group, **self._UNUSED)
            ps = self._tensors(group)
            if not ps:
                continue
            steps = {self.state[p]["step"] for p in ps}
            if len(steps) != 1:
                raise RuntimeError(f"{type(self).__name__}: parameters of a group must share their step count")
            (ct, co, _, n_chunks), tab = self._launch_plan(ps, group)
            b1, b2 = group["betas"]
            with torch.cuda.device(ps[0].device):
                _lib.check(getattr(_lib.lib, self._entry)(tab.data_ptr(), ct.data_ptr(), co.data_ptr(), n_chunks,
                                                          group["lr"], b1, b2, group["eps"], group["weight_decay"],
                                                          steps.pop(), torch.cuda.current_stream().cuda_stream),
                           self._entry)
        return loss


class FusedAdamW(_AdamFamily):
    """torch.optim.AdamW semantics (lr, betas, eps, weight_decay; no amsgrad / maximize), one launch per step."""

    _entry = "cgat_adamw_step"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))


class FusedAdam(_AdamFamily):
    """torch.optim.Adam semantics (lr, betas, eps, L2 weight_decay coupled into the gradient; no amsgrad / maximize),
    one launch per step.  State and its names are FusedAdamW's, which are torch's."""

    _entry = "cgat_adam_step"
    # decoupled_weight_decay=True (newer torch) is AdamW under Adam's name: a state dict that carries it wants FusedAdamW
    _UNUSED = dict(amsgrad=False, maximize=False, decoupled_weight_decay=False)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False,
                 decoupled_weight_decay=False):
        _refuse_options("FusedAdam", dict(amsgrad=amsgrad, maximize=maximize, decoupled_weight_decay=decoupled_weight_decay),
                        **self._UNUSED)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **self._UNUSED))


class FusedSGD(_MultiTensor):
    """torch.optim.SGD semantics (lr, momentum, weight_decay; dampening 0, no Nesterov / maximize), one launch per step.
    State per parameter is torch's: {"momentum_buffer"}, and none at momentum == 0."""

    _UNUSED = dict(dampening=0, nesterov=False, maximize=False)

    def __init__(self, params, lr=1e-3, momentum=0, weight_decay=0, dampening=0, nesterov=False, maximize=False):
        _refuse_options("FusedSGD", dict(dampening=dampening, nesterov=nesterov, maximize=maximize), **self._UNUSED)
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, **self._UNUSED))

    def _advance_state(self, p, group):
        if group["momentum"] == 0:
            return                                      # no entry in self.state at all, as torch.optim.SGD
        st = self.state[p]
        # a zero buffer gives the bits of torch's first step (buf = clone(g')); torch may also have stored None
        if st.get("momentum_buffer") is None:
            st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)

    def _moment_ptrs(self, p, group):
        return (self.state[p]["momentum_buffer"].data_ptr() if group["momentum"] != 0 else 0), 0

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        for group in self.param_groups:
            _refuse_options("FusedSGD", group, **self._UNUSED)
            ps = self._tensors(group)
            if not ps:
                continue
            (ct, co, _, n_chunks), tab = self._launch_plan(ps, group)
            with torch.cuda.device(ps[0].device):
                _lib.check(_lib.lib.cgat_sgd_step(tab.data_ptr(), ct.data_ptr(), co.data_ptr(), n_chunks, group["lr"],
                                                  group["momentum"], group["weight_decay"],
                                                  torch.cuda.current_stream().cuda_stream), "cgat_sgd_step")
        return loss


class FusedLamb(_MultiTensor):
    """The reference's JITLamb (CGAT/lambs.py): LAMB without bias correction, weight norm clamped to [0, 10]."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0, adam=False):
        if adam:
            raise NotImplementedError("adam=True (trust ratio forced to 1) is not used by the reference's harness")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        for group in self.param_groups:
            ps = self._tensors(group)
            if not ps:
                continue
            (ct, co, first, n_chunks), tab = self._launch_plan(ps, group)
            ws = torch.empty(2 * n_chunks + len(ps), dtype=torch.float32, device=ps[0].device)
            b1, b2 = group["betas"]
            with torch.cuda.device(ps[0].device):
                _lib.check(_lib.lib.cgat_lamb_step(tab.data_ptr(), ct.data_ptr(), co.data_ptr(), n_chunks, first.data_ptr(),
                                                   len(ps), group["lr"], b1, b2, group["eps"], group["weight_decay"],
                                                   ws.data_ptr(), torch.cuda.current_stream().cuda_stream),
                           "cgat_lamb_step")
        return loss


class _RobustLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, log_std, target, kind):
        for t in (output, log_std, target):
            if not t.is_cuda:
                raise RuntimeError("robust losses run on the GPU (no CPU fallback)")
        shape = torch.broadcast_shapes(output.shape, log_std.shape, target.shape)
        o, s, t = (x.to(torch.float32).expand(shape).contiguous().reshape(-1) for x in (output, log_std, target))
        n = o.numel()
        terms, go, gs = (torch.empty(n, dtype=torch.float32, device=o.device) for _ in range(3))
        with torch.cuda.device(o.device):
            _lib.check(_lib.lib.cgat_robust_loss(o.data_ptr(), s.data_ptr(), t.data_ptr(), n, kind, terms.data_ptr(),
                                                 go.data_ptr(), gs.data_ptr(), torch.cuda.current_stream().cuda_stream),
                       "cgat_robust_loss")
        ctx.save_for_backward(go, gs)
        ctx.shapes = (output.shape, log_std.shape, shape, n)
        return terms.mean()

    @staticmethod
    def backward(ctx, g):
        go, gs = ctx.saved_tensors
        so, ss, shape, n = ctx.shapes
        scale = g / n
        return ((go * scale).reshape(shape).sum_to_size(so), (gs * scale).reshape(shape).sum_to_size(ss), None, None)


def RobustL1(output, log_std, target):
    """mean( sqrt(2) |output - target| exp(-log_std) + log_std )      (CGAT/utils.py:30-37)"""
    return _RobustLoss.apply(output, log_std, target, 1)


def RobustL2(output, log_std, target):
    """mean( 0.5 (output - target)^2 exp(-2 log_std) + log_std )      (CGAT/utils.py:40-47)"""
    return _RobustLoss.apply(output, log_std, target, 2)


_KINDS = {"RobustL1": 1, "RobustL2": 2, "L1": 3, "L2": 4}


class _CriterionMetrics(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, log_std, target, kind, mean, std):
        robust = kind <= 2
        ins = (output, log_std, target) if robust else (output, target)
        for t in ins:
            if not t.is_cuda:
                raise RuntimeError("losses and step metrics run on the GPU (no CPU fallback)")
        shape = torch.broadcast_shapes(*(x.shape for x in ins))
        flat = [x.to(torch.float32).expand(shape).contiguous().reshape(-1) for x in ins]
        o, t = flat[0], flat[-1]
        n = o.numel()
        go = torch.empty(n, dtype=torch.float32, device=o.device)
        gs = torch.empty(n, dtype=torch.float32, device=o.device) if robust else None
        out3 = torch.empty(3, dtype=torch.float32, device=o.device)
        with torch.cuda.device(o.device):
            _lib.check(_lib.lib.cgat_loss_metrics(o.data_ptr(), flat[1].data_ptr() if robust else 0, t.data_ptr(), n, kind,
                                                  mean, std, go.data_ptr(), gs.data_ptr() if robust else 0,
                                                  out3.data_ptr(), torch.cuda.current_stream().cuda_stream),
                       "cgat_loss_metrics")
        ctx.save_for_backward(go, gs)
        ctx.shapes = (output.shape, log_std.shape if robust else None, shape)
        loss, mae, rmse = out3.unbind(0)
        ctx.mark_non_differentiable(mae, rmse)
        return loss, mae, rmse

    @staticmethod
    def backward(ctx, g, _g_mae, _g_rmse):
        go, gs = ctx.saved_tensors                      # gradients of the MEAN loss: the kernel has divided by n
        so, ss, shape = ctx.shapes
        return ((g * go).reshape(shape).sum_to_size(so), (g * gs).reshape(shape).sum_to_size(ss) if ss is not None else None,
                None, None, None, None)


def criterion_with_metrics(kind, output, log_std, target, mean=0.0, std=1.0):
    """(loss, mae, rmse) of one step in one launch (CGAT/lightning_module.py:153-159, 240-243): `target` is the RAW
    target, loss = criterion(output[, log_std], (target - mean) / std) with `kind` in "RobustL1" | "RobustL2" | "L1" |
    "L2", mae = mean |pred - target| and rmse = sqrt(mean (pred - target)^2) on pred = output * std + mean.  `loss`
    carries the gradient to output and log_std ("L1" / "L2" do not read log_std: it may be None); mae and rmse are
    detached 0-d device tensors.  Shapes broadcast as in RobustL1.  No host synchronisation."""
    if kind not in _KINDS:
        raise ValueError(f"kind must be one of {sorted(_KINDS)}, got {kind!r}")
    if _KINDS[kind] <= 2 and log_std is None:
        raise ValueError(f"{kind} needs log_std")
    return _CriterionMetrics.apply(output, log_std, target, _KINDS[kind], float(mean), float(std))


def L1Loss(output, target):
    """mean |output - target|                                          (nn.L1Loss(), CGAT/lightning_module.py:140)"""
    return criterion_with_metrics("L1", output, None, target)[0]


def MSELoss(output, target):
    """mean (output - target)^2                                        (nn.MSELoss(), CGAT/lightning_module.py:142)"""
    return criterion_with_metrics("L2", output, None, target)[0]


def cyclical_lr(period=100, cycle_mul=0.2, tune_mul=0.05):
    """Triangular cyclical schedule as a LambdaLR multiplier (CGAT/utils.py:50-64); `tune_mul` is accepted and unused,
    as in the reference."""
    def relative(it):
        cycle = math.floor(1 + it / period)
        x = abs(2 * (it / period - cycle) + 1)
        return max(0, (1 - x))

    return lambda it: cycle_mul + (1. - cycle_mul) * relative(it)
