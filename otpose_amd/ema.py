"""Exponential moving average of a model's weights - the reference's ``ModelEma`` (thirdparty/utils/train_utils.py:240-262)
with its per-tensor loop ``ema_v.copy_(decay * ema_v + (1. - decay) * model_v)`` over ``state_dict()`` (2725 entries at W48:
some 8000 tiny launches and 2725 temporaries per step) replaced by at most two HIP launches per ``update()``:

* tensors of the model that tile one storage without a gap - the parameters of a group of ``FusedAdamW`` / ``FusedSGD``, which
  live in the group's flat buffer - are averaged into a MIRROR buffer of the same layout (the copy's tensors become views of
  it) by ``otp_ema_update`` on the whole region.  One region: one flat launch.  Several (the three groups of
  ``make_optimizer``): the regions become jobs of the table, still one 16-byte-vector pass each;
* everything else (BatchNorm running statistics, the int64 ``num_batches_tracked``, frozen parameters, every parameter when
  there is no flat optimizer) is one job each of a device table that ``otp_ema_update_table`` walks in one launch.

The arithmetic is the reference's to the bit: ``float32(decay) * ema`` and ``float32(1. - decay) * model`` each rounded, then
their rounded sum; int64 entries go through float32 and back by truncation (``Tensor.copy_`` from float into long).

The job table holds raw device pointers, so every ``update()`` / ``set()`` first compares the storage address of each tensor
of both models with the addresses the table was built from (a Python loop over the modules' own parameter / buffer
dictionaries; its cost is in DESIGN.md section 0) and rebuilds when one moved: an optimizer built AFTER the ``ModelEma``
re-points ``param.data`` into its flat buffer, ``model.to(...)`` replaces buffers, ``load_state_dict`` copies in place (no
move; nothing to do).  The copy is an ``OTPose`` whose eval forward runs from packed weight images: the kernels write through
raw pointers, so after every ``update()`` / ``set()`` the copy's engine is dropped (``invalidate_engine()``) and the next eval
forward of ``.module`` packs the averaged weights - once, at that forward.

There is no CPU path and no second device: ``device`` other than ``None`` / the model's own raises ``NotImplementedError``."""
from __future__ import annotations

import ctypes
import weakref
from copy import deepcopy

import torch

from . import hip
from .optim import _bump_versions


def _slots(model):
    """(dictionary, key) of every parameter and buffer slot of ``model`` that holds a tensor, each tensor once: reading the
    slot again later sees a re-pointed ``.data`` as well as a replaced tensor object."""
    out, seen = [], set()
    for m in model.modules():
        for d in (m._parameters, m._buffers):
            for k, t in d.items():
                if t is not None and id(t) not in seen:
                    seen.add(id(t))
                    out.append((d, k))
    return out


def _addresses(slots):
    return [d[k].data_ptr() for d, k in slots]


def _dtype_code(t):
    if t.dtype == torch.float32:
        return hip.CONSTANTS["OTP_DTYPE_F32"]
    if t.dtype == torch.int64:
        return hip.CONSTANTS["OTP_DTYPE_I64"]
    raise TypeError(f"ModelEma averages float32 tensors and int64 counters; the state_dict holds a {t.dtype} tensor")


class ModelEma(torch.nn.Module):
    """``ModelEma(model, decay=0.999, device=None)``: ``.module`` is a deep copy of ``model`` in eval mode whose ``state_dict()``
    tensors hold the average; ``update(model)`` folds the model's current state in, ``set(model)`` copies it.  Validate with
    ``ema.module`` (a full ``OTPose``: ``ema.module(x, margin=...)``, ``.predict``, ``.state_dict()``)."""

    def __init__(self, model, decay=0.999, device=None):
        super().__init__()
        own = next((t.device for t in model.state_dict().values()), None)
        if device is not None:
            dev = torch.device(device)
            if dev.type != "cuda" or own is None or dev.type != own.type or (dev.index is not None and dev != own):
                raise NotImplementedError(f"ModelEma averages on the model's own GPU; device={device!r} is not implemented "
                                          "(otpose_amd has no CPU path)")
        for k, v in model.state_dict().items():
            if v.is_floating_point() and v.dtype != torch.float32:
                raise TypeError(f"ModelEma needs a float32 state_dict: {k} is {v.dtype}")
            if not v.is_floating_point() and v.dtype != torch.int64:
                raise TypeError(f"ModelEma averages float32 tensors and int64 counters: {k} is {v.dtype}")
        engine = model.__dict__.get("_engine")                    # packed weights, static buffers, a captured graph: not copied
        if engine is not None:
            model._engine = None
        try:
            self.module = deepcopy(model)
        finally:
            if engine is not None:
                model._engine = engine
        self.module.eval()
        self.decay = decay
        self.device = device
        self._plan = None              # what update() launches: built on first use, rebuilt when storage moved

    # ---- the launch plan -------------------------------------------------------------------------------------------------------
    def _build(self, model):
        ema_sd, src_sd = self.module.state_dict(keep_vars=True), model.state_dict(keep_vars=True)
        if len(ema_sd) != len(src_sd):
            raise ValueError(f"ModelEma: the model's state_dict has {len(src_sd)} entries, the copy's {len(ema_sd)}")
        pairs, seen = [], set()
        for (ke, e), (ks, s) in zip(ema_sd.items(), src_sd.items()):
            if e.shape != s.shape or e.dtype != s.dtype:
                raise ValueError(f"ModelEma: entry {ke} of the copy is {tuple(e.shape)} {e.dtype}, {ks} of the model "
                                 f"{tuple(s.shape)} {s.dtype}")
            if not s.is_cuda or e.device != s.device:
                raise RuntimeError(f"ModelEma needs the model and its copy on one GPU ({ks}: {s.device}, copy: {e.device}); "
                                   "otpose_amd has no CPU path")
            if not (e.is_contiguous() and s.is_contiguous()):
                raise ValueError(f"ModelEma: entry {ks} is not contiguous")
            if e.numel() and e.data_ptr() not in seen:           # a tensor under two names is averaged once
                seen.add(e.data_ptr())
                pairs.append((e, s))
        # regions: float32 tensors of the model that share one storage and tile a span of it without a gap
        by_storage = {}
        for i, (e, s) in enumerate(pairs):
            if s.dtype == torch.float32:
                by_storage.setdefault(s.untyped_storage().data_ptr(), []).append(i)
        regions, in_region = [], set()
        for idx in by_storage.values():
            if len(idx) < 2:
                continue
            idx.sort(key=lambda i: pairs[i][1].data_ptr())
            lo = pairs[idx[0]][1].data_ptr()
            end = lo
            for i in idx:
                if pairs[i][1].data_ptr() != end:
                    break
                end += 4 * pairs[i][1].numel()
            else:
                regions.append((lo, (end - lo) // 4, idx))
                in_region.update(idx)
        keep = []                                                 # tensors the raw pointers of the plan rely on
        flat = []                                                 # (mirror, source address, elements)
        for lo, n, idx in regions:
            first = pairs[idx[0]][0]
            mirror = getattr(first, "_otp_ema_mirror", None)
            if mirror is None or mirror.numel() != n or mirror.device != first.device or \
                    any(pairs[i][0].data_ptr() != mirror.data_ptr() + pairs[i][1].data_ptr() - lo for i in idx):
                mirror = torch.empty(n, dtype=torch.float32, device=first.device)
                for i in idx:
                    e, s = pairs[i]
                    view = mirror[(s.data_ptr() - lo) // 4:][:e.numel()].view(e.shape)
                    view.copy_(e)
                    e.data = view
                    e._otp_ema_mirror = mirror
            flat.append((mirror, lo, n))
            keep.append(mirror)
        L = hip.lib()
        nb = int(L.otp_ema_job_bytes())
        jobs, prev = bytearray(), None

        def add(e_ptr, s_ptr, n, code, what):
            nonlocal prev
            job = ctypes.create_string_buffer(nb)
            hip.check(L.otp_ema_job(ctypes.c_void_p(e_ptr), ctypes.c_void_p(s_ptr), n, code, prev, job), f"otp_ema_job({what})")
            jobs.extend(job.raw)
            prev = job

        single = flat[0] if len(flat) == 1 else None
        if single is None:
            for mirror, lo, n in flat:
                add(mirror.data_ptr(), lo, n, hip.CONSTANTS["OTP_DTYPE_F32"], "flat region")
        n_jobs = 0 if single is not None else len(flat)
        for i, (e, s) in enumerate(pairs):
            if i not in in_region:
                add(e.data_ptr(), s.data_ptr(), e.numel(), _dtype_code(s), "tensor")
                keep.append(e)
                n_jobs += 1
        dev = pairs[0][0].device if pairs else None
        table = torch.frombuffer(jobs, dtype=torch.uint8).to(dev) if n_jobs else None
        ema_slots, src_slots = _slots(self.module), _slots(model)
        self._plan = {"model": weakref.ref(model), "single": single, "table": table, "n_jobs": n_jobs, "keep": keep,
                      "ema_slots": ema_slots, "src_slots": src_slots, "ema_addr": _addresses(ema_slots),
                      "src_addr": _addresses(src_slots), "written": [e for e, _ in pairs]}

    def _current_plan(self, model):
        """The plan for ``model``, rebuilt when a tensor of either side is no longer where the plan's pointers say."""
        p = self._plan
        if p is None or p["model"]() is not model or _addresses(p["src_slots"]) != p["src_addr"] or \
                _addresses(p["ema_slots"]) != p["ema_addr"]:
            self._build(model)
            p = self._plan
        return p

    def _launch(self, model, decay):
        p = self._current_plan(model)
        d, omd = float(decay), float(1. - decay)                  # (the subtraction in double; the kernels take float32 of both)
        L = hip.lib()
        if p["single"] is not None:
            mirror, src_ptr, n = p["single"]
            hip.check(L.otp_ema_update(hip.ptr(mirror), ctypes.c_void_p(src_ptr), n, d, omd, hip.stream_of(mirror)), "otp_ema_update")
        if p["n_jobs"]:
            hip.check(L.otp_ema_update_table(hip.ptr(p["table"]), p["n_jobs"], d, omd, hip.stream_of(p["table"])),
                      "otp_ema_update_table")
        _bump_versions(p["written"])
        if hasattr(self.module, "invalidate_engine"):
            self.module.invalidate_engine()                       # packed weight images of the copy are stale now

    # ---- the reference's methods -----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self, model):
        """``ema = decay * ema + (1 - decay) * model`` over every entry of ``state_dict()``: at most two launches."""
        self._launch(model, self.decay)

    @torch.no_grad()
    def set(self, model):
        """``ema = model``, exactly (also for infinities and NaN, which ``0 * ema`` would not pass through)."""
        torch._foreach_copy_(list(self.module.state_dict().values()), list(model.state_dict().values()))
        if hasattr(self.module, "invalidate_engine"):
            self.module.invalidate_engine()
