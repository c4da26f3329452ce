"""Optimizers + LR schedule.

* ``SGD`` — fused multi-tensor SGD/momentum (reference: torch.optim.SGD at
  ddp.py:183, stepped at ddp.py:240).  On ROCm devices the whole step is a
  single multi-tensor HIP kernel sweep (one launch per chunk list, not one
  per parameter); supports bf16 params with fp32 master weights (the
  reference's apex-O2 slot, ddp.py:165-181, reincarnated natively).
* ``AdamW`` — fused multi-tensor AdamW on the same chunk/plan machinery,
  with fp32 master weights, the device-side overflow skip and the
  device-scalar lr of ``SGD``; ``param_groups_no_decay`` builds its usual
  two groups (no decay on biases, norm params and names the model excludes).
* ``clip_grad_norm_`` — global L2 norm + scale (reference ddp.py:238-239)
  via the multi-tensor l2norm/scale kernels.
* ``get_linear_schedule_with_warmup`` — linear warmup then linear decay to 0
  (reference ddp.py:52-61), same LambdaLR shape.
"""

from __future__ import annotations

import torch
from torch.optim.lr_scheduler import LambdaLR

from .ops import grad_l2_norm, scale_grads_
from .ops.native import native, use_native


def get_linear_schedule_with_warmup(optimizer, num_warmup_steps, num_training_steps, last_epoch=-1):
    """Reference ddp.py:52-61."""

    def lr_lambda(current_step: int):
        if current_step < num_warmup_steps:
            return float(current_step) / float(max(1, num_warmup_steps))
        return max(
            0.0,
            float(num_training_steps - current_step)
            / float(max(1, num_training_steps - num_warmup_steps)),
        )

    return LambdaLR(optimizer, lr_lambda, last_epoch)


def clip_grad_norm_(parameters, max_norm: float) -> torch.Tensor:
    """Global-L2 gradient clipping (reference ddp.py:238-239)."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    total_norm = grad_l2_norm(grads)
    if max_norm > 0:
        # host-side compare against a device scalar would sync; compute the
        # clip coefficient on device and always scale (coef clamped to 1).
        if grads and grads[0].is_cuda:
            coef = (max_norm / (total_norm + 1e-6)).clamp(max=1.0)
            native().scale_by_tensor_(list(grads), coef)
        else:
            coef = float(max_norm / (float(total_norm) + 1e-6))
            if coef < 1.0:
                scale_grads_(grads, coef)
    return total_norm


class SGD(torch.optim.Optimizer):
    """Fused multi-tensor SGD with momentum / weight decay / nesterov.

    With ``master_weights=True`` and bf16 parameters, keeps an fp32 master
    copy per parameter; the fused kernel updates master in fp32 and writes
    the bf16 working copy in the same pass.
    """

    def __init__(
        self,
        params,
        lr: float,
        momentum: float = 0.0,
        weight_decay: float = 0.0,
        dampening: float = 0.0,
        nesterov: bool = False,
        master_weights: bool = False,
    ):
        defaults = dict(
            lr=lr,
            momentum=momentum,
            weight_decay=weight_decay,
            dampening=dampening,
            nesterov=nesterov,
            master_weights=master_weights,
        )
        super().__init__(params, defaults)

    def load_state_dict(self, state_dict):
        """torch's Optimizer.load_state_dict casts floating-point state to
        each param's dtype — with bf16 params that silently rounds the fp32
        master weights and momentum through bf16 (destroying the master
        precision) and then crashes the fused kernel, which requires fp32
        state.  Restore the fp32 slots from the ORIGINAL (on-disk) tensors
        after the structural load."""
        super().load_state_dict(state_dict)
        id_map = {}
        for g_saved, g in zip(state_dict["param_groups"], self.param_groups):
            for pid, p in zip(g_saved["params"], g["params"]):
                id_map[pid] = p
        for pid, st_saved in state_dict["state"].items():
            p = id_map.get(pid)
            if p is None:
                continue
            st = self.state[p]
            for k in ("momentum_buffer", "master"):
                if k in st_saved and isinstance(st_saved[k], torch.Tensor):
                    st[k] = st_saved[k].to(
                        device=p.device, dtype=torch.float32
                    )

    @torch.no_grad()
    def step(self, closure=None, guard=None, skip_count=None, lr_tensor=None):
        """``guard`` (f32 device scalar, e.g. the pre-clip grad norm): when
        non-finite the fused kernel skips the whole update ON DEVICE and
        ticks ``skip_count`` — no host sync (the fp16 loss-scaler path).
        ``lr_tensor`` (f32 device scalar): the kernel reads lr from the
        device, so a hipGraph-captured step follows the live schedule."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._guard, self._skip_count = guard, skip_count
        self._lr_tensor = lr_tensor
        for group in self.param_groups:
            params, grads, moms, masters = [], [], [], []
            momentum = group["momentum"]
            use_master = group["master_weights"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if momentum != 0 and "momentum_buffer" not in state:
                    state["momentum_buffer"] = torch.zeros_like(
                        p, dtype=torch.float32
                    )
                if use_master and p.dtype != torch.float32 and "master" not in state:
                    state["master"] = p.detach().float().clone()
                params.append(p)
                grads.append(p.grad)
                moms.append(state["momentum_buffer"] if momentum != 0 else None)
                masters.append(state.get("master") if use_master else None)
            if not params:
                continue
            self._fused_step(group, params, grads, moms, masters)
        self._guard = self._skip_count = self._lr_tensor = None
        return loss

    def _fused_step(self, group, params, grads, moms, masters):
        lr = group["lr"]
        momentum = group["momentum"]
        wd = group["weight_decay"]
        damp = group["dampening"]
        nesterov = group["nesterov"]
        if use_native(*params):
            native().sgd_step(
                params,
                grads,
                [m if m is not None else torch.Tensor() for m in moms],
                [m if m is not None else torch.Tensor() for m in masters],
                lr,
                momentum,
                wd,
                damp,
                nesterov,
                getattr(self, "_guard", None),
                getattr(self, "_skip_count", None),
                getattr(self, "_lr_tensor", None),
            )
            return
        # CPU reference path (also the numerics reference for the kernel)
        lrt = getattr(self, "_lr_tensor", None)
        if lrt is not None:
            lr = float(lrt)
        guard = getattr(self, "_guard", None)
        if guard is not None and not bool(torch.isfinite(guard).all()):
            sc = getattr(self, "_skip_count", None)
            if sc is not None:
                sc.add_(1)
            return
        for p, g, m, mw in zip(params, grads, moms, masters):
            work = mw if mw is not None else p
            gf = g.float()
            if wd != 0:
                gf = gf.add(work.float(), alpha=wd)
            if momentum != 0:
                m.mul_(momentum).add_(gf, alpha=1 - damp)
                gf = gf.add(m, alpha=momentum) if nesterov else m
            if mw is not None:
                mw.add_(gf, alpha=-lr)
                p.copy_(mw.to(p.dtype))
            else:
                p.add_(gf.to(p.dtype), alpha=-lr)


class AdamW(torch.optim.Optimizer):
    """Fused multi-tensor AdamW (decoupled weight decay, the
    ``torch.optim.AdamW`` update rule) with the same extras as ``SGD``: fp32
    master weights for bf16/fp16 params, a device-side overflow skip and a
    device-scalar learning rate.

    Per-parameter state is ``exp_avg`` and ``exp_avg_sq`` (plus ``master``
    with ``master_weights=True`` and a non-fp32 param), always fp32.

    The step count ``t`` of the bias corrections is ONE f32 scalar per
    optimizer on the parameters' device.  ``step()`` advances it once, before
    any launch, with plain torch ops that are legal under stream capture, and
    the kernel reads it from the device — so a hipGraph-captured step sees
    the live ``t``, a skipped step advances neither ``t`` nor the moments,
    and ``t`` (and ``skip_count``) tick once per step however many param
    groups or >512-tensor plans the step launches.  f32 counts exactly up to
    2^24 steps.

    Deliberate difference from torch: a parameter whose grad is ``None`` on
    some steps shares the optimizer-wide ``t`` (torch counts per parameter).
    """

    def __init__(
        self,
        params,
        lr: float,
        betas=(0.9, 0.999),
        eps: float = 1e-8,
        weight_decay: float = 1e-2,
        master_weights: bool = False,
    ):
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"betas must be in [0, 1): {betas}")
        defaults = dict(
            lr=lr,
            betas=tuple(betas),
            eps=eps,
            weight_decay=weight_decay,
            master_weights=master_weights,
        )
        super().__init__(params, defaults)
        self._step_t = None  # f32 device scalar, created on the first step

    def _step_scalar(self, device):
        if self._step_t is None or self._step_t.device != device:
            old = self._step_t
            self._step_t = torch.zeros((), dtype=torch.float32, device=device)
            if old is not None:
                self._step_t.copy_(old)
        return self._step_t

    def state_dict(self):
        """Adds the step scalar as the top-level key ``"step"``."""
        sd = super().state_dict()
        sd["step"] = (
            torch.zeros((), dtype=torch.float32)
            if self._step_t is None
            else self._step_t.detach().clone()
        )
        return sd

    def load_state_dict(self, state_dict):
        """As ``SGD.load_state_dict``: torch casts floating-point state to the
        param's dtype, which would round the fp32 moments and master through
        bf16; restore them (and the step scalar) in fp32 on the param's
        device from the saved tensors."""
        super().load_state_dict(state_dict)
        id_map = {}
        for g_saved, g in zip(state_dict["param_groups"], self.param_groups):
            for pid, p in zip(g_saved["params"], g["params"]):
                id_map[pid] = p
        for pid, st_saved in state_dict["state"].items():
            p = id_map.get(pid)
            if p is None:
                continue
            st = self.state[p]
            for k in ("exp_avg", "exp_avg_sq", "master"):
                if k in st_saved and isinstance(st_saved[k], torch.Tensor):
                    st[k] = st_saved[k].to(
                        device=p.device, dtype=torch.float32
                    )
        device = self.param_groups[0]["params"][0].device
        saved = state_dict.get("step")
        if saved is None:
            saved = torch.zeros(())
        # in place: a captured graph keeps reading the same scalar
        self._step_scalar(device).copy_(
            torch.as_tensor(saved, dtype=torch.float32).reshape(())
        )

    @torch.no_grad()
    def step(self, closure=None, guard=None, skip_count=None, lr_tensor=None):
        """Same keywords as ``SGD.step``.  ``guard`` (f32 device scalar):
        when non-finite the whole update is skipped on device, ``t`` stays
        and ``skip_count`` ticks once — no host sync.  ``lr_tensor`` (f32
        device scalar) overrides the groups' ``lr`` on device."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        buckets = []  # (group, params, grads, exp_avgs, exp_avg_sqs, masters)
        for group in self.param_groups:
            use_master = group["master_weights"]
            by_dtype = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if "exp_avg" not in state:
                    state["exp_avg"] = torch.zeros_like(p, dtype=torch.float32)
                    state["exp_avg_sq"] = torch.zeros_like(
                        p, dtype=torch.float32
                    )
                if use_master and p.dtype != torch.float32 and "master" not in state:
                    state["master"] = p.detach().float().clone()
                b = by_dtype.setdefault(p.dtype, ([], [], [], [], []))
                b[0].append(p)
                b[1].append(p.grad)
                b[2].append(state["exp_avg"])
                b[3].append(state["exp_avg_sq"])
                b[4].append(state.get("master") if use_master else None)
            buckets.extend((group, *b) for b in by_dtype.values())
        if not buckets:
            return loss
        # advance t once per step, before any launch; capture-legal torch ops
        step_t = self._step_scalar(buckets[0][1][0].device)
        if guard is None:
            step_t += 1
        else:
            ok = torch.isfinite(guard).float().reshape(())
            step_t += ok
            if skip_count is not None:
                skip_count += (1 - ok).reshape(skip_count.shape)
        for group, params, grads, ms, vs, masters in buckets:
            self._fused_step(
                group, params, grads, ms, vs, masters, step_t, guard,
                skip_count, lr_tensor,
            )
        return loss

    def _fused_step(self, group, params, grads, ms, vs, masters, step_t,
                    guard, skip_count, lr_tensor):
        lr = group["lr"]
        beta1, beta2 = group["betas"]
        eps = group["eps"]
        wd = group["weight_decay"]
        if use_native(*params):
            native().adamw_step(
                params,
                grads,
                ms,
                vs,
                [m if m is not None else torch.Tensor() for m in masters],
                lr,
                beta1,
                beta2,
                eps,
                wd,
                step_t,
                guard,
                skip_count,
                lr_tensor,
            )
            return
        # CPU reference path: torch.optim.AdamW's single-tensor update, op
        # for op, with t from the optimizer-wide scalar
        if guard is not None and not bool(torch.isfinite(guard).all()):
            return
        if lr_tensor is not None:
            lr = float(lr_tensor)
        t = float(step_t)
        step_size = lr / (1 - beta1 ** t)
        bc2_sqrt = (1 - beta2 ** t) ** 0.5
        for p, g, m, v, mw in zip(params, grads, ms, vs, masters):
            # fp32 throughout; a low-precision param is rounded once, at the end
            w = mw if mw is not None else p.float()
            gf = g.float()
            if wd != 0:
                w.mul_(1 - lr * wd)
            m.lerp_(gf, 1 - beta1)
            v.mul_(beta2).addcmul_(gf, gf, value=1 - beta2)
            denom = (v.sqrt() / bc2_sqrt).add_(eps)
            w.addcdiv_(m, denom, value=-step_size)
            if w is not p:
                p.copy_(w.to(p.dtype))


def param_groups_no_decay(model, weight_decay: float):
    """Two param groups for ``AdamW``: ``weight_decay=0`` for every parameter
    with ``ndim <= 1`` (biases, BN/LayerNorm gains and shifts) and for every
    name the model lists in an optional ``no_weight_decay()`` method;
    ``weight_decay`` for the rest.  Returned as ``[decay, no_decay]``."""
    skip = set(model.no_weight_decay()) if hasattr(model, "no_weight_decay") else set()
    decay, no_decay = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        (no_decay if p.ndim <= 1 or name in skip else decay).append(p)
    return [
        {"params": decay, "weight_decay": weight_decay},
        {"params": no_decay, "weight_decay": 0.0},
    ]
