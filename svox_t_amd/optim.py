"""Optimizers for feature tables: SGD, RMSprop and Adam whose update is one HIP kernel over the table
(csrc/svoxt_optim.hip) and which can skip the rows a backward did not touch.

    opt = svox_t_amd.FeatureAdam([tree.features], lr=1e-2)          # lazy=True
    out = renderer(tree.features, rays); loss(out).backward(); opt.step(); opt.zero_grad()

They are torch.optim.Optimizer subclasses -- param_groups, state_dict() / load_state_dict(), zero_grad() and the lr
schedulers work as with torch's -- with torch's constructor arguments and torch's state keys (`momentum_buffer`,
`square_avg`, `exp_avg`, `exp_avg_sq`, `step`), so a state dict moves to and from the torch optimizer of the same name.

The arithmetic is float32, one correctly rounded operation at a time, in the order include/svoxt.h writes out
(DESIGN.md 4.14): FeatureAdam is torch.optim.Adam's form, eps added after the bias correction.  A row is TOUCHED iff
some element of its gradient row is != 0 (a NaN touches, -0.0 does not).  With lazy=True (the default) an untouched
row keeps every bit of the parameter and of the state and is not read; `step` still counts every call.  With
lazy=False every row is updated, torch.optim's dense semantics: moments decay where the gradient is zero.  Weight
decay, Nesterov momentum, dampening, amsgrad, centered RMSprop, RMSprop's momentum and maximize are refused, not ignored.

After tree surgery that replaces `tree.features` (prune, merge, quantize) call `rebind(old, new, row_map)`.

gauss_newton_step_(features, grad, hessdiag, lr=, damping=) is the damped Newton step that consumes
VolumeRenderer.se_grad's gradient and Gauss-Newton diagonal: one kernel over the table, no state.
"""
from __future__ import annotations

import math

import torch

from svox_t_amd import csrc as _C

__all__ = ["FeatureSGD", "FeatureRMSprop", "FeatureAdam", "gauss_newton_step_"]


def _check_table(p, what: str) -> None:
    """A parameter these optimizers take: a float32, contiguous, 2-D GPU tensor."""
    if not isinstance(p, torch.Tensor):
        raise RuntimeError(f"{what} must be a tensor")
    if p.layout != torch.strided or p.dtype != torch.float32 or p.dim() != 2:
        raise RuntimeError(f"{what} must be a dense float32 [M, K] table, not {p.dtype} {tuple(p.shape)}")
    if not p.is_cuda:
        raise RuntimeError(f"{what} must be on a GPU: the feature-table optimizers are HIP kernels, there is no CPU path")
    if not p.is_contiguous():
        raise RuntimeError(f"{what} must be contiguous")
    if p.shape[0] < 1 or p.shape[1] < 1:
        raise RuntimeError(f"{what} must have at least one row and one column")


def _refuse(cls: str, **options) -> None:
    for name, value in options.items():
        if isinstance(value, torch.Tensor) or value:
            raise RuntimeError(f"{cls} does not implement {name} (got {value!r}): use torch.optim for it")


def _number(cls: str, name: str, value, lo: float, hi: float = math.inf, hi_open: bool = False) -> float:
    if isinstance(value, torch.Tensor) or isinstance(value, bool):
        raise RuntimeError(f"{cls}: {name} must be a Python number")
    v = float(value)
    if not (lo <= v and (v < hi if hi_open else v <= hi)):
        raise RuntimeError(f"{cls}: invalid {name}: {value!r}")
    return v


class _FeatureOptimizer(torch.optim.Optimizer):
    """What the three share: the checks, the walk over the parameters, the step count, rebind."""

    _state_keys: tuple = ()                       # the per-row state tables, in the order of state1, state2

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)
            for pi, p in enumerate(group["params"]):
                _check_table(p, f"parameter {pi} of group {gi}")

    # -- per kind ---------------------------------------------------------------------------------------------------
    def _check_group(self, group) -> None:
        raise NotImplementedError

    def _kind(self, group) -> str:
        raise NotImplementedError

    def _hyper(self, group, t: int) -> dict:
        """The scalars of svoxt_optim_hyper for step t: double precision here, rounded to float32 once by the call."""
        raise NotImplementedError

    def _tables(self, group) -> tuple:
        return self._state_keys

    # -- the step ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _step_count(state) -> int:
        t = state["step"]
        return int(t.item()) if isinstance(t, torch.Tensor) else int(t)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)
            kind, keys = self._kind(group), self._tables(group)
            for pi, p in enumerate(group["params"]):
                if p.grad is None:
                    continue
                what = f"parameter {pi} of group {gi}"
                _check_table(p, what)
                g = p.grad
                if g.layout != torch.strided:
                    raise RuntimeError(f"{what}: a sparse gradient is not supported (the kernel finds the touched rows itself)")
                if g.dtype != torch.float32 or g.shape != p.shape or g.device != p.device:
                    raise RuntimeError(f"{what}: the gradient must be float32 {tuple(p.shape)} on {p.device}")
                if not g.is_contiguous():
                    g = g.contiguous()
                state = self.state[p]
                if "step" not in state:
                    # torch's representation of the count: a float32 scalar on the host
                    state["step"] = torch.zeros((), dtype=torch.float32)
                for k in keys:
                    if k not in state or state[k] is None:
                        state[k] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    elif not state[k].is_contiguous():
                        state[k] = state[k].contiguous()
                t = self._step_count(state) + 1
                state["step"] = torch.tensor(float(t), dtype=torch.float32)        # (a new tensor: state dicts taken earlier keep theirs)
                tabs = [state[k] for k in keys] + [None, None]
                _C.optim_step(kind, p, g, tabs[0], tabs[1], self._hyper(group, t), bool(group["lazy"]))
        return loss

    def __setstate__(self, state) -> None:
        # load_state_dict replaces every param group by the saved one: a group saved by torch.optim's optimizer of the
        # same name has no `lazy` (or any other key only these classes know), which then takes the constructor's value
        super().__setstate__(state)
        for group in self.param_groups:
            for k, v in self.defaults.items():
                group.setdefault(k, v)

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)            # (ends in __setstate__)
        for state in self.state.values():          # a count kept on the device (torch's fused / capturable) comes to the host once
            if isinstance(state.get("step"), torch.Tensor) and state["step"].is_cuda:
                state["step"] = state["step"].to("cpu", torch.float32)

    # -- tree surgery -----------------------------------------------------------------------------------------------
    def rebind(self, old_param, new_param, row_map=None) -> None:
        """Put `new_param` in the place of `old_param` -- after N3Tree.prune / merge / quantize, which replace
        `tree.features` by a new nn.Parameter -- keeping its param group and that group's options.

        row_map (int64 [M'], as PruneResult.row_map / MergeResult.row_map give it: the old row of every new row): every
        per-row state table becomes table[row_map] (one gather kernel each) and `step` is kept; new_param must be
        [M', K] with the old K.  Without row_map the parameter starts with fresh state (zeros, step 0): the case after
        quantize, or after a merge that made new rows.  RuntimeError if old_param is not held, or the shapes disagree with row_map."""
        where = [(group, i) for group in self.param_groups for i, p in enumerate(group["params"]) if p is old_param]
        if not where:
            raise RuntimeError("rebind: old_param is not a parameter of this optimizer")
        if new_param is not old_param and any(p is new_param for group in self.param_groups for p in group["params"]):
            raise RuntimeError("rebind: new_param is already a parameter of this optimizer")
        _check_table(new_param, "rebind: new_param")
        if row_map is not None:
            if not isinstance(row_map, torch.Tensor) or row_map.dtype != torch.int64 or row_map.dim() != 1:
                raise RuntimeError("rebind: row_map must be an int64 [M'] tensor")
            if tuple(new_param.shape) != (row_map.shape[0], old_param.shape[1]):
                raise RuntimeError(f"rebind: new_param is {tuple(new_param.shape)}, but row_map [{row_map.shape[0]}] over the old "
                                   f"{tuple(old_param.shape)} table gives {(row_map.shape[0], old_param.shape[1])}")
            if int(row_map.min()) < 0 or int(row_map.max()) >= old_param.shape[0]:
                raise RuntimeError("rebind: row_map names rows outside the old table")
        old_state = self.state.pop(old_param, {})
        for group, i in where:
            group["params"][i] = new_param
        if row_map is not None and old_state:
            per_row = lambda v: isinstance(v, torch.Tensor) and tuple(v.shape) == tuple(old_param.shape)   # noqa: E731
            self.state[new_param] = {k: _C.gather_rows(v.contiguous(), row_map) if per_row(v) else v for k, v in old_state.items()}


class FeatureSGD(_FeatureOptimizer):
    """torch.optim.SGD on feature tables as one HIP kernel: p += -lr * g, or with momentum b = momentum * b + g,
    p += -lr * b (`momentum_buffer` starts at zero, so b = g on the first step, as torch's).  lazy: skip rows whose
    gradient is all zeros -- without momentum that changes no bit, it only saves traffic."""

    _state_keys = ("momentum_buffer",)

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, lazy=True):
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov, maximize=maximize, lazy=lazy))

    def _check_group(self, group):
        _number("FeatureSGD", "lr", group["lr"], 0.0)
        _number("FeatureSGD", "momentum", group["momentum"], 0.0)
        _refuse("FeatureSGD", dampening=group.get("dampening", 0), weight_decay=group.get("weight_decay", 0),
                nesterov=group.get("nesterov", False), maximize=group.get("maximize", False))

    def _kind(self, group):
        return "sgd_momentum" if group["momentum"] != 0 else "sgd"

    def _tables(self, group):
        return self._state_keys if group["momentum"] != 0 else ()

    def _hyper(self, group, t):
        return {"neg_step": -float(group["lr"]), "momentum": float(group["momentum"])}


class FeatureRMSprop(_FeatureOptimizer):
    """torch.optim.RMSprop (plain: no momentum, not centered) on feature tables as one HIP kernel:
    v = alpha * v + (1 - alpha) * g^2, p += -lr * g / (sqrt(v) + eps); `square_avg` is v."""

    _state_keys = ("square_avg",)

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, *, maximize=False,
                 lazy=True):
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum,
                                      centered=centered, maximize=maximize, lazy=lazy))

    def _check_group(self, group):
        _number("FeatureRMSprop", "lr", group["lr"], 0.0)
        _number("FeatureRMSprop", "alpha", group["alpha"], 0.0)
        _number("FeatureRMSprop", "eps", group["eps"], 0.0)
        _refuse("FeatureRMSprop", weight_decay=group.get("weight_decay", 0), momentum=group.get("momentum", 0),
                centered=group.get("centered", False), maximize=group.get("maximize", False))

    def _kind(self, group):
        return "rmsprop"

    def _hyper(self, group, t):
        alpha = float(group["alpha"])
        return {"neg_step": -float(group["lr"]), "beta2": alpha, "one_minus_beta2": 1.0 - alpha, "eps": float(group["eps"])}


class FeatureAdam(_FeatureOptimizer):
    """torch.optim.Adam on feature tables as one HIP kernel: m += (g - m) * (1 - b1), v = b2 * v + (1 - b2) * g^2,
    p += -lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps); `exp_avg` is m, `exp_avg_sq` is v, `step` is t.
    With lazy=True the moments of an untouched row do not decay and its parameter does not move (torch's dense Adam
    keeps moving it along the old momentum): the row is as it was, bit for bit, and costs one read of its gradient."""

    _state_keys = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False, lazy=True):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                                      maximize=maximize, lazy=lazy))

    def _check_group(self, group):
        _number("FeatureAdam", "lr", group["lr"], 0.0)
        _number("FeatureAdam", "eps", group["eps"], 0.0)
        betas = group["betas"]
        if not isinstance(betas, (tuple, list)) or len(betas) != 2:
            raise RuntimeError(f"FeatureAdam: betas must be a pair of numbers, got {betas!r}")
        _number("FeatureAdam", "betas[0]", betas[0], 0.0, 1.0, hi_open=True)
        _number("FeatureAdam", "betas[1]", betas[1], 0.0, 1.0, hi_open=True)
        _refuse("FeatureAdam", weight_decay=group.get("weight_decay", 0), amsgrad=group.get("amsgrad", False),
                maximize=group.get("maximize", False))

    def _kind(self, group):
        return "adam"

    def _hyper(self, group, t):
        b1, b2 = (float(b) for b in group["betas"])
        return {"neg_step": -float(group["lr"]) / (1.0 - b1 ** t), "one_minus_beta1": 1.0 - b1, "beta2": b2,
                "one_minus_beta2": 1.0 - b2, "bias2_sqrt": math.sqrt(1.0 - b2 ** t), "eps": float(group["eps"])}


def gauss_newton_step_(features, grad, hessdiag, *, lr: float = 1.0, damping: float = 0.0, lazy: bool = True):
    """features -= lr * grad / (hessdiag + damping), IN PLACE, as one HIP kernel over the table: the damped Newton step
    of PlenOctree-style fine-tuning on what VolumeRenderer.se_grad returns.

    Per entry, in float32, each operation correctly rounded: d = hessdiag + damping; where d > 0 the entry becomes
    p - lr * (grad / d) -- the bits of the same three torch ops -- and otherwise (no curvature and no damping) it is
    left as it is.  lazy=True (the optimizers' convention): a row whose grad row is all zeros -- no ray of the batch
    met it -- is read no further and not written.  The version counter of `features` is bumped, as by every operator
    that writes the table behind torch's back.  Returns `features`."""
    p = features
    _check_table(p, "features")
    for name, x in (("grad", grad), ("hessdiag", hessdiag)):
        _check_table(x, name)
        if x.shape != p.shape or x.device != p.device:
            raise RuntimeError(f"{name} must be float32 {tuple(p.shape)} on {p.device}")
    _C._extras.gauss_newton_step(p, grad, hessdiag, lr, damping, lazy)
    return features
