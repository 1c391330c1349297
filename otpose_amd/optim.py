"""Optimizer step of the reference training loop on flat HBM buffers: ``torch.nn.utils.clip_grad_norm_`` followed by
``torch.optim.AdamW.step()`` or ``torch.optim.SGD.step()`` (script/Common.py:138-143; built by
thirdparty/utils/train_utils.py:62-137) as two HIP passes - a sum of squares over the flat gradients and one fused clip +
update per hyper-parameter group - with no host synchronisation (the clip coefficient is read from device memory).
:func:`make_optimizer` is the reference's factory of the same name: its three parameter groups under ``cfg.TRAIN.OPTIMIZER``.

``FusedAdamW`` / ``FusedSGD`` take the same parameter groups as ``torch.optim.AdamW`` / ``torch.optim.SGD`` (so
``make_optimizer``'s three groups carry over unchanged) and re-home parameters and gradients into one flat fp32 buffer per group: ``p.data`` and ``p.grad`` become views,
autograd keeps accumulating into them, and ``flat_grads()`` hands the few large buffers to the RCCL all-reduce
(:mod:`otpose_amd.parallel`) - large messages are what the point-to-point xGMI links want.
"""
from __future__ import annotations

import torch

from . import hip


def _bump_versions(tensors):
    """The kernels write parameters through raw pointers; tell autograd / the inference engine's staleness check."""
    try:
        torch._C._increment_version(tensors)
    except TypeError:                                   # older signature: one tensor at a time
        for t in tensors:
            torch._C._increment_version(t)


class _FlatOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share: parameters, gradients and per-element state re-homed into one flat fp32 buffer per
    hyper-parameter group (``_flat[i]``: ``p``, ``g``, the state buffers named by ``_BUFFERS``, ``params``, ``gptr``), the
    gradient slots the backward kernels write into, and the sum of squares behind the clip.  A subclass names its state
    buffers, fills ``state[p]`` / its own keys of ``_flat[i]`` in ``_init_group`` and launches its update in ``step()``."""

    _BUFFERS = ()             # (key of a flat state buffer in _flat[i], key of its per-parameter view in state[p])

    def _init_flat(self, max_grad_norm):
        self.max_grad_norm = float(max_grad_norm)
        self._flat = []                                  # per group: dict(p, g, <state buffers>, params, gptr, ...)
        # [epoch, clean]: zero_grad() opens an epoch in which every slot is known to be zero (train_ops.grad_slot hands a
        # slot out once per epoch); step() closes it.  One cell shared by all parameters of this optimizer.
        self._slot_epoch = [0, False]
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.requires_grad]
            if not ps:
                self._flat.append(None)
                continue
            dev = ps[0].device
            if dev.type != "cuda" or any(p.device != dev or p.dtype != torch.float32 for p in ps):
                raise RuntimeError(f"{type(self).__name__} needs float32 parameters on one CUDA (HIP) device; there is no CPU path")
            total = sum(p.numel() for p in ps)
            fp = torch.empty(total, dtype=torch.float32, device=dev)
            fg = torch.zeros_like(fp)
            f = {"p": fp, "g": fg, "params": ps}
            for key, _ in self._BUFFERS:
                f[key] = torch.zeros_like(fp)
            off = 0
            for p in ps:
                n = p.numel()
                fp[off:off + n].copy_(p.data.reshape(-1))
                p.data = fp[off:off + n].view_as(p)
                if p.grad is not None:
                    fg[off:off + n].copy_(p.grad.reshape(-1))
                p.grad = fg[off:off + n].view_as(p)
                # destination of this parameter's gradient inside the flat buffer: the backward kernels of otpose_amd write
                # there directly (grad_slot() below), so autograd neither allocates nor accumulates per-parameter tensors
                p._otp_grad_slot = p.grad
                p._otp_slot_epoch = self._slot_epoch
                off += n
            f["gptr"] = [p._otp_grad_slot.data_ptr() for p in ps]
            self._init_group(group, f)
            self._flat.append(f)
        devs = {f["p"].device for f in self._flat if f}
        # [0]: the squared norm; behind it the scratch of otp_grad_sumsq's fixed-order reduction
        scratch = int(hip.lib().otp_grad_sumsq_scratch())
        self._normsq = {d: torch.zeros(1 + scratch, dtype=torch.float64, device=d) for d in devs}

    def _init_group(self, group, f):
        raise NotImplementedError

    @staticmethod
    def _views(f, key):
        """(parameter, its view into the flat buffer ``f[key]``) for every parameter of the group."""
        off = 0
        for p in f["params"]:
            n = p.numel()
            yield p, f[key][off:off + n].view_as(p)
            off += n

    def _rehome_grads(self):
        """``p.grad`` must stay a view of the flat gradient buffer.  ``model.zero_grad()`` (set_to_none=True by default)
        or any ``p.grad = ...`` detaches it, after which autograd accumulates outside the buffer and step() /
        allreduce_flat_grads() would see zeros: copy such a gradient back and re-point the view.  A parameter whose
        gradient is None keeps a zero slot (its weight decay / moment update then match torch.optim.AdamW only if the
        caller really meant "zero gradient"; likewise FusedSGD's momentum buffer of such a parameter decays where
        torch.optim.SGD would skip the parameter; use this optimizer's own zero_grad() to keep the views)."""
        from .bf16_ops import join_wgrad_streams
        join_wgrad_streams()                  # weight gradients enqueued on side streams (bf16_ops.conv_wgrad)
        for f in self._flat:
            if not f:
                continue
            # fast path (every step): one pointer comparison per parameter, no tensor objects created
            for p, ptr in zip(f["params"], f["gptr"]):
                g = p.grad
                if g is not None and g.data_ptr() == ptr:
                    continue
                slot = p._otp_grad_slot
                if g is None:
                    slot.zero_()
                else:
                    slot.copy_(g.reshape(slot.shape))
                p.grad = slot.view(slot.shape)

    def flat_grads(self):
        """The flat gradient buffers (one per group) - the units to all-reduce."""
        self._rehome_grads()
        return [f["g"] for f in self._flat if f]

    def zero_grad(self, set_to_none: bool = False):
        """One memset per group.  ``p.grad`` is dropped so that the next backward hands each parameter its gradient
        exactly once: the otpose_amd backward kernels write straight into the parameter's slot of the flat buffer and return
        that view (autograd adopts it - no allocation, no ``grad += new`` launch per parameter, ~2000 tiny kernels per step
        at W48); gradients that arrive as ordinary tensors are copied into their slot by step() / flat_grads()."""
        for f in self._flat:
            if f:
                f["g"].zero_()
                for p in f["params"]:
                    p.grad = None
        self._slot_epoch[0] += 1
        self._slot_epoch[1] = True

    @torch.no_grad()
    def grad_norm(self, _rehomed=False):
        """Global L2 norm of all gradients as a device scalar (what clip_grad_norm_ returns), no host sync."""
        L = hip.lib()
        if not _rehomed:
            self._rehome_grads()
        for acc in self._normsq.values():
            acc[:1].zero_()
        for f in self._flat:
            if f:
                hip.check(L.otp_grad_sumsq(hip.ptr(f["g"]), f["g"].numel(), hip.ptr(self._normsq[f["g"].device]),
                                           hip.stream_of(f["g"])), "otp_grad_sumsq")
        accs = list(self._normsq.values())
        return accs[0][:1].sqrt() if len(accs) == 1 else torch.stack([a[:1].cpu() for a in accs]).sum().sqrt()

    def _begin_step(self):
        """Gradients into their slots, the slot epoch closed, the squared norm on the device: True when step() clips."""
        self._rehome_grads()
        self._slot_epoch[1] = False                      # the slots now hold this step's gradients: not clean until zero_grad()
        clip = self.max_grad_norm > 0.0
        if clip:
            self.grad_norm(_rehomed=True)
        return clip


class FusedAdamW(_FlatOptimizer):
    _BUFFERS = (("m", "exp_avg"), ("v", "exp_avg_sq"))

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=0.0):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("invalid AdamW hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._init_flat(max_grad_norm)

    def _init_group(self, group, f):
        f["step"] = 0
        for (p, m), (_, v) in zip(self._views(f, "m"), self._views(f, "v")):
            self.state[p] = {"step": 0, "exp_avg": m, "exp_avg_sq": v}

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        L = hip.lib()
        clip = self._begin_step()
        for group, f in zip(self.param_groups, self._flat):
            if not f:
                continue
            f["step"] += 1
            b1, b2 = group["betas"]
            acc = self._normsq[f["g"].device]
            hip.check(L.otp_adamw_step(hip.ptr(f["p"]), hip.ptr(f["g"]), hip.ptr(f["m"]), hip.ptr(f["v"]), f["p"].numel(),
                                       float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                       float(group["weight_decay"]), f["step"], hip.ptr(acc) if clip else None,
                                       self.max_grad_norm, hip.stream_of(f["p"])), "otp_adamw_step")
            _bump_versions(f["params"])
        return loss

    def _sync_state_steps(self):
        """``state[p]["step"]`` of every parameter from its group's counter (kept per group on the hot path)."""
        for f in self._flat:
            if f:
                for p in f["params"]:
                    self.state[p]["step"] = f["step"]

    def state_dict(self):
        self._sync_state_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # the base class re-creates the state tensors: copy them back into the flat moment buffers and re-point the views
        for f in self._flat:
            if not f:
                continue
            off = 0
            for p in f["params"]:
                n = p.numel()
                st = self.state[p]
                for key, flat in (("exp_avg", f["m"]), ("exp_avg_sq", f["v"])):
                    flat[off:off + n].copy_(st[key].reshape(-1))
                    st[key] = flat[off:off + n].view_as(p)
                f["step"] = int(st.get("step", f["step"]))
                st["step"] = f["step"]
                off += n


class FusedSGD(_FlatOptimizer):
    """``clip_grad_norm_`` + ``torch.optim.SGD.step()`` (TRAIN.OPTIMIZER = SGD, train_utils.py:123-128) on the flat buffers:
    one otp_sgd_step launch per group.  Hyper-parameters are per group as in torch; ``state[p]["momentum_buffer"]`` is a
    view into the group's flat buffer ``_flat[i]["b"]`` and exists, as in torch, from the group's first step on (the first
    step writes ``buf = d``, every later one runs the recurrence), so ``state_dict()`` / ``load_state_dict()`` interchange
    with ``torch.optim.SGD`` over the same groups.  A parameter without a gradient keeps a zero slot: see _rehome_grads."""

    _BUFFERS = ()             # "b" is allocated for the groups that have a momentum (_init_group)

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, max_grad_norm=0.0):
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov))
        for group in self.param_groups:                  # torch.optim.SGD's checks, on every group
            if group["lr"] < 0.0:
                raise ValueError(f"Invalid learning rate: {group['lr']}")
            if group["momentum"] < 0.0:
                raise ValueError(f"Invalid momentum value: {group['momentum']}")
            if group["weight_decay"] < 0.0:
                raise ValueError(f"Invalid weight_decay value: {group['weight_decay']}")
            if group["nesterov"] and (group["momentum"] <= 0 or group["dampening"] != 0):
                raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self._init_flat(max_grad_norm)

    def _init_group(self, group, f):
        f["b"] = torch.zeros_like(f["p"]) if group["momentum"] != 0 else None
        f["first"] = True                                # no step has written the momentum buffer yet

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        L = hip.lib()
        clip = self._begin_step()
        for group, f in zip(self.param_groups, self._flat):
            if not f:
                continue
            momentum = float(group["momentum"])
            if momentum != 0 and f["b"] is None:         # a momentum switched on after construction
                f["b"], f["first"] = torch.zeros_like(f["p"]), True
            acc = self._normsq[f["g"].device]
            hip.check(L.otp_sgd_step(hip.ptr(f["p"]), hip.ptr(f["g"]), hip.ptr(f["b"]) if momentum != 0 else None,
                                     f["p"].numel(), float(group["lr"]), momentum, float(group["dampening"]),
                                     float(group["weight_decay"]), int(bool(group["nesterov"])), int(f["first"]),
                                     hip.ptr(acc) if clip else None, self.max_grad_norm, hip.stream_of(f["p"])),
                      "otp_sgd_step")
            if momentum != 0 and f["first"]:
                for p, view in self._views(f, "b"):
                    self.state[p]["momentum_buffer"] = view
                f["first"] = False
            _bump_versions(f["params"])
        return loss

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # the base class re-creates the state tensors: copy them back into the flat momentum buffer and re-point the views;
        # a group that arrives with buffers is past its first step (a parameter of it without one starts from zero)
        for group, f in zip(self.param_groups, self._flat):
            if not f:
                continue
            if group.get("maximize"):
                raise ValueError("FusedSGD has no maximize mode")
            loaded = [self.state[p].get("momentum_buffer") if p in self.state else None for p in f["params"]]
            if all(b is None for b in loaded):
                f["first"] = True
                continue
            if f["b"] is None:
                f["b"] = torch.zeros_like(f["p"])
            for (p, view), b in zip(self._views(f, "b"), loaded):
                if b is None:
                    view.zero_()
                else:
                    view.copy_(b.reshape(view.shape))
                self.state[p]["momentum_buffer"] = view
            f["first"] = False


def reference_param_groups(model, cfg):
    """The three parameter groups of the reference's ``make_optimizer`` (thirdparty/utils/train_utils.py:66-121) on this
    package's module classes: decay / no-decay / pretrained in that order, each sorted by full parameter name; ``weight_decay`` = TRAIN.WD, 0 and TRAIN.WD, and ``lr`` = TRAIN.LR / 100 for the pretrained group (the
    HRNet backbone).  Frozen parameters (MODEL.FREEZE_HRNET_WEIGHTS) stay in their group, as in the reference."""
    from torch import nn

    from . import modules as M
    from .model import DeformableCONV

    # RSN_ATTENTION: the MODEL.PRM modules go where the chains they follow go (def_fuse_prm.* also matches the prefix rule below)
    white = (nn.Linear, nn.Conv1d, DeformableCONV, M.CHAIN_RSB_BLOCKS, M.RSN_ATTENTION, nn.ConvTranspose1d)
    # the token encoders (MODEL.TOKEN_LAYERS / FLOW_TOKEN_LAYERS; the reference's make_optimizer has no rule for them and would
    # assert): in_proj_weight, out_proj.weight, linear{1,2}.weight decay; every bias, norm*.weight and the positional tables do not
    black = (M.LayerNorm, nn.GroupNorm, nn.LayerNorm)
    decay, no_decay, pretrained = set(), set(), set()
    for mn, m in model.named_modules():
        for pn, _ in m.named_parameters():
            fpn = f"{mn}.{pn}" if mn else pn
            if isinstance(m, M.HRNet) or fpn.startswith(("teacher", "rough_pose_estimation_net")):
                pretrained.add(fpn)
            elif pn.endswith("bias"):
                no_decay.add(fpn)
            elif pn.startswith("def_fuse") or (pn.endswith("weight") and isinstance(m, white)):
                decay.add(fpn)
            elif pn.endswith("weight") and isinstance(m, black):
                no_decay.add(fpn)
            elif pn.endswith("scale") and isinstance(m, M.AffineDropPath):
                no_decay.add(fpn)
            elif pn.endswith("rel_pe") or pn in ("temporal_pos_embedding", "flow_pos_embedding"):
                no_decay.add(fpn)
            elif pn == "in_proj_weight" and isinstance(m, M._SelfAttnParams):
                decay.add(fpn)
            elif pn == "weight" and isinstance(m, nn.Conv2d) and ".embd." in f".{mn}.":
                decay.add(fpn)          # conv embedding of a ConvTransformer (its bias and embd_norm.* fall under the rules above)
            elif pn.startswith(("offsets_list", "masks_list", "final_layer")):
                decay.add(fpn)
    named = dict(model.named_parameters())
    for a, b, what in ((decay, no_decay, "decay/no_decay"), (pretrained, no_decay, "pretrained/no_decay"),
                       (decay, pretrained, "decay/pretrained")):
        assert not (a & b), f"parameters {sorted(a & b)} made it into both {what} sets!"
    left = named.keys() - (decay | no_decay | pretrained)
    assert not left, f"parameters {sorted(left)} were not separated into either decay/no_decay set!"
    return [{"params": [named[n] for n in sorted(decay)], "weight_decay": cfg.TRAIN.WD},
            {"params": [named[n] for n in sorted(no_decay)], "weight_decay": 0.0},
            {"params": [named[n] for n in sorted(pretrained)], "weight_decay": cfg.TRAIN.WD, "lr": cfg.TRAIN.LR / 100}]


def make_optimizer(model, cfg, fused=None, max_grad_norm=1.0):
    """The reference's ``make_optimizer(model, cfg)`` (train.py:57, thirdparty/utils/train_utils.py:62-137): the three groups
    of :func:`reference_param_groups` under ``cfg.TRAIN.OPTIMIZER``:

    * ``"AdamW"``: ``lr = TRAIN.LR``, everything else ``torch.optim.AdamW``'s defaults;
    * ``"SGD"``: ``lr = TRAIN.LR``, ``momentum = TRAIN.MOMENTUM`` and nothing else - the reference does not pass
      ``TRAIN.NESTEROV`` on, so it is ignored there and here;
    * anything else: ``TypeError("Unsupported optimizer!")``.

    ``fused=False`` returns the plain ``torch.optim`` object the reference would build.  ``fused=True`` returns
    :class:`FusedAdamW` / :class:`FusedSGD` with the clip of script/Common.py:138-142 folded into ``step()``
    (``max_grad_norm``; 1.0 is ``clip_grad_l2norm``'s default at Common.py:79, 0 switches the clip off) - do not call
    ``clip_grad_norm_`` as well.  ``fused=None`` (default): fused when every parameter is on a GPU."""
    groups = reference_param_groups(model, cfg)
    if fused is None:
        fused = all(p.is_cuda for g in groups for p in g["params"])
    name = cfg.TRAIN.OPTIMIZER
    if name == "SGD":
        if fused:
            return FusedSGD(groups, lr=cfg.TRAIN.LR, momentum=cfg.TRAIN.MOMENTUM, max_grad_norm=max_grad_norm)
        return torch.optim.SGD(groups, lr=cfg.TRAIN.LR, momentum=cfg.TRAIN.MOMENTUM)
    if name == "AdamW":
        if fused:
            return FusedAdamW(groups, lr=cfg.TRAIN.LR, max_grad_norm=max_grad_norm)
        return torch.optim.AdamW(groups, lr=cfg.TRAIN.LR)
    raise TypeError("Unsupported optimizer!")
