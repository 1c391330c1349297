"""Person detector: the reference's Darknet YOLOv3 (object_detector/YOLOv3), uint8 video frames in, ``xywh`` person boxes out.

``PersonDetector`` keeps the reference ``Darknet``'s parameters under its ``state_dict`` names and runs on the GPU only: the
letterbox, the activation passes, the head decode and the merging NMS are the kernels of csrc/detect.hip, the convolutions
run on the exact-fp32 ``otp_conv2d`` with BatchNorm folded into its scale / shift.  No frame, feature map or candidate list
goes through the host between the frame pool and the boxes.  DESIGN.md section 3.12.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn

from . import ops

YOLOV3_ANCHORS = ((10, 13), (16, 30), (33, 23), (30, 61), (62, 45), (59, 119), (116, 90), (156, 198), (373, 326))
_SUPPORTED = ("convolutional", "shortcut", "route", "upsample", "yolo")


def parse_darknet_cfg(path):
    """The block dicts of a Darknet ``.cfg`` file as the reference's ``parse_model_config`` returns them: every value a
    stripped string, ``type`` from the ``[header]``, and ``batch_normalize`` preset to the integer 0 in convolutional blocks
    (a line of the file replaces it by a string).  Block 0 is ``[net]``."""
    defs = []
    with open(path) as f:
        for raw in f.read().split("\n"):
            if not raw or raw.startswith("#"):
                continue
            line = raw.strip()
            if line.startswith("["):
                defs.append({"type": line[1:-1].rstrip()})
                if defs[-1]["type"] == "convolutional":
                    defs[-1]["batch_normalize"] = 0
            else:
                key, value = line.split("=")
                defs[-1][key.rstrip()] = value.strip()
    return defs


def _conv(filters, size, stride=1, leaky=True):
    if leaky:
        return {"type": "convolutional", "batch_normalize": "1", "filters": str(filters), "size": str(size),
                "stride": str(stride), "pad": "1", "activation": "leaky"}
    return {"type": "convolutional", "batch_normalize": 0, "size": str(size), "stride": str(stride), "pad": "1",
            "filters": str(filters), "activation": "linear"}


def yolov3_defs(num_classes=80, img_size=416):
    """The block list of the reference's ``config/yolov3.cfg`` (Darknet-53 and three heads), built in code; with the
    defaults it equals ``parse_darknet_cfg`` of that file."""
    net = {"type": "net", "batch": "16", "subdivisions": "1", "width": str(img_size), "height": str(img_size), "channels": "3",
           "momentum": "0.9", "decay": "0.0005", "angle": "0", "saturation": "1.5", "exposure": "1.5", "hue": ".1",
           "learning_rate": "0.001", "burn_in": "1000", "max_batches": "500200", "policy": "steps",
           "steps": "400000,450000", "scales": ".1,.1"}
    defs = [net, _conv(32, 3)]
    for width, blocks in ((64, 1), (128, 2), (256, 8), (512, 8), (1024, 4)):
        defs.append(_conv(width, 3, stride=2))
        for _ in range(blocks):
            defs += [_conv(width // 2, 1), _conv(width, 3), {"type": "shortcut", "from": "-3", "activation": "linear"}]
    anchors = ",  ".join(f"{w},{h}" for w, h in YOLOV3_ANCHORS)
    for width, mask, lateral in ((512, "6,7,8", None), (256, "3,4,5", "61"), (128, "0,1,2", "36")):
        if lateral is not None:
            defs += [{"type": "route", "layers": "-4"}, _conv(width, 1), {"type": "upsample", "stride": "2"},
                     {"type": "route", "layers": f"-1, {lateral}"}]
        for _ in range(3):
            defs += [_conv(width, 1), _conv(2 * width, 3)]
        defs.append(_conv(3 * (5 + num_classes), 1, leaky=False))
        defs.append({"type": "yolo", "mask": mask, "anchors": anchors, "classes": str(num_classes), "num": "9", "jitter": ".3",
                     "ignore_thresh": ".7", "truth_thresh": "1", "random": "1"})
    return defs


class _Plan:
    """Shapes and data flow of a block list (without ``[net]``): per layer ``(C, H, W)``, the layers it reads, and which
    activation passes fold into their neighbours."""

    def __init__(self, blocks, channels, img_size):
        self.blocks = blocks
        self.shape, self.src = [], []
        for i, d in enumerate(blocks):
            t = d["type"]
            if t not in _SUPPORTED:
                raise NotImplementedError(f"Darknet block {i} [{t}] is not supported (supported: {', '.join(_SUPPORTED)})")
            prev = self.shape[-1] if i else (channels, img_size, img_size)
            if t == "convolutional":
                k, s = int(d["size"]), int(d["stride"])
                pad = (k - 1) // 2 if int(d["pad"]) else 0
                if d["activation"] not in ("leaky", "linear"):
                    raise NotImplementedError(f"Darknet block {i}: activation {d['activation']!r}")
                ho, wo = ops.out_hw(prev[1], prev[2], k, k, s, pad, 1)
                self.shape.append((int(d["filters"]), ho, wo))
                self.src.append([i - 1])
            elif t == "upsample":
                if int(d["stride"]) != 2:
                    raise NotImplementedError(f"Darknet block {i}: upsample stride {d['stride']} (only 2)")
                self.shape.append((prev[0], 2 * prev[1], 2 * prev[2]))
                self.src.append([i - 1])
            elif t == "route":
                ls = [self._index(i, int(v)) for v in d["layers"].split(",")]
                if not 1 <= len(ls) <= 2 or any(self.shape[j][1:] != self.shape[ls[0]][1:] for j in ls):
                    raise NotImplementedError(f"Darknet block {i}: route over {d['layers']!r}")
                self.shape.append((sum(self.shape[j][0] for j in ls),) + self.shape[ls[0]][1:])
                self.src.append(ls)
            elif t == "shortcut":
                j = self._index(i, int(d["from"]))
                if self.shape[j] != prev:
                    raise ValueError(f"Darknet block {i}: shortcut from {d['from']} joins {self.shape[j]} and {prev}")
                self.shape.append(prev)
                self.src.append([i - 1, j])
            else:                                                   # yolo
                mask = [int(v) for v in d["mask"].split(",")]
                flat = [int(v) for v in d["anchors"].split(",")]
                d = dict(d, _anchors=[(flat[2 * m], flat[2 * m + 1]) for m in mask], _classes=int(d["classes"]))
                blocks[i] = d
                if prev[0] != len(mask) * (5 + d["_classes"]) or prev[1] != prev[2]:
                    raise ValueError(f"Darknet block {i}: yolo layer over a {prev} map")
                self.shape.append((len(mask) * prev[1] * prev[2], 5 + d["_classes"], 0))       # rows, row length
                self.src.append([i - 1])
            if any(blocks[j]["type"] == "yolo" for j in self.src[-1] if j >= 0) and t != "yolo":
                raise NotImplementedError(f"Darknet block {i} reads the output of a yolo layer")
        if not any(d["type"] == "yolo" for d in blocks):
            raise ValueError("the block list has no yolo layer")
        readers = [[] for _ in blocks]
        for i, ss in enumerate(self.src):
            for j in ss:
                if j >= 0:
                    readers[j].append(i)
        # a leaky conv read by nothing but the shortcut / upsample behind it hands its activation pass to that block
        self.fused_into = {}
        for i, d in enumerate(blocks[:-1]):
            if d["type"] == "convolutional" and d["activation"] == "leaky" and readers[i] == [i + 1] and \
                    blocks[i + 1]["type"] in ("shortcut", "upsample"):
                self.fused_into[i] = i + 1
        self.readers = readers

    def _index(self, i, v):
        j = i + v if v < 0 else v
        if not 0 <= j < i:
            raise ValueError(f"Darknet block {i} refers to layer {v}")
        return j


class PersonDetector(nn.Module):
    """YOLOv3 person detector with the reference ``Darknet``'s parameters (``module_list.{i}.conv_{i}.weight``,
    ``module_list.{i}.batch_norm_{i}.*``) and its eval arithmetic.  ``defs_or_cfg_path``: a block list (``yolov3_defs()``,
    ``parse_darknet_cfg(...)``; block 0 is ``[net]``) or the path of a ``.cfg`` file.  GPU only; eval only."""

    def __init__(self, defs_or_cfg_path=None, img_size=416, conf_thres=0.4, nms_thres=0.4, person_class=0):
        super().__init__()
        if defs_or_cfg_path is None:
            defs = yolov3_defs(img_size=img_size)
        elif isinstance(defs_or_cfg_path, (list, tuple)):
            defs = [dict(d) for d in defs_or_cfg_path]
        else:
            defs = parse_darknet_cfg(defs_or_cfg_path)
        if not defs or defs[0].get("type") != "net":
            raise ValueError("block 0 of a Darknet block list is [net]")
        self.hyperparams, self.module_defs = defs[0], defs[1:]
        self.img_size, self.conf_thres, self.nms_thres, self.person_class = int(img_size), float(conf_thres), float(nms_thres), int(person_class)
        # the reference's yolo layers scale by hyperparams["height"] (models.py:78); the letterbox fills img_size
        self.net_size = int(self.hyperparams.get("height", img_size))
        if self.net_size != self.img_size:
            raise ValueError(f"img_size {self.img_size} differs from the cfg's height {self.net_size}")
        self._plan = _Plan(self.module_defs, int(self.hyperparams.get("channels", 3)), self.img_size)
        self.module_list = nn.ModuleList()
        cin = int(self.hyperparams.get("channels", 3))
        chans = []
        for i, d in enumerate(self.module_defs):
            seq = nn.Sequential()
            if d["type"] == "convolutional":
                bn, k = int(d["batch_normalize"]), int(d["size"])
                seq.add_module(f"conv_{i}", nn.Conv2d(chans[-1] if chans else cin, int(d["filters"]), k, int(d["stride"]),
                                                      (k - 1) // 2 if int(d["pad"]) else 0, bias=not bn))
                if bn:
                    seq.add_module(f"batch_norm_{i}", nn.BatchNorm2d(int(d["filters"])))
            self.module_list.append(seq)
            chans.append(self._plan.shape[i][0])
        self.num_rows = sum(self._plan.shape[i][0] for i, d in enumerate(self.module_defs) if d["type"] == "yolo")
        self.num_classes = next(d["_classes"] for d in self.module_defs if d["type"] == "yolo")
        if any(d["_classes"] != self.num_classes for d in self.module_defs if d["type"] == "yolo"):
            raise ValueError("the yolo layers disagree on the number of classes")
        self.header_info = np.array([0, 0, 0, 0, 0], dtype=np.int32)
        self._engine = None
        self.eval()

    # ---- weights --------------------------------------------------------------------------------------------------------------
    def invalidate_engine(self):
        """Drop the folded and packed weights (call after changing parameters in place)."""
        self._engine = None

    def load_state_dict(self, *a, **k):
        self._engine = None
        return super().load_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        self._engine = None
        return super()._apply(fn, *a, **k)

    def load_darknet_weights(self, path):
        """Read a binary Darknet ``.weights`` file: 5 int32 of header, then per convolution the BatchNorm ``bias, weight,
        running_mean, running_var`` (or the conv bias where there is no BatchNorm) and the conv weights, all float32."""
        with open(path, "rb") as f:
            header = np.fromfile(f, dtype=np.int32, count=5)
            w = np.fromfile(f, dtype=np.float32)
        if header.size != 5:
            raise ValueError(f"{path}: no Darknet header")
        self.header_info = header
        ptr = 0

        def take(t):
            nonlocal ptr
            n = t.numel()
            if ptr + n > w.size:
                raise ValueError(f"{path}: {w.size} floats, the network needs more")
            t.data.copy_(torch.from_numpy(w[ptr:ptr + n].copy()).view_as(t))
            ptr += n

        for seq in self.module_list:
            if len(seq) == 0:
                continue
            conv = seq[0]
            if len(seq) > 1:
                bn = seq[1]
                for t in (bn.bias, bn.weight, bn.running_mean, bn.running_var):
                    take(t)
            else:
                take(conv.bias)
            take(conv.weight)
        if ptr != w.size:
            raise ValueError(f"{path}: {w.size} floats, the network takes {ptr}")
        self._engine = None

    def save_darknet_weights(self, path):
        """Write the parameters in the format :meth:`load_darknet_weights` reads."""
        with open(path, "wb") as f:
            np.asarray(self.header_info, dtype=np.int32).tofile(f)
            for seq in self.module_list:
                if len(seq) == 0:
                    continue
                conv = seq[0]
                ts = (seq[1].bias, seq[1].weight, seq[1].running_mean, seq[1].running_var) if len(seq) > 1 else (conv.bias,)
                for t in ts + (conv.weight,):
                    t.detach().cpu().numpy().astype(np.float32).tofile(f)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("PersonDetector is an inference module (the reference only ever runs it in eval mode)")
        return super().train(False)

    # ---- forward ----------------------------------------------------------------------------------------------------------------
    def _get_engine(self, batch, device):
        e = self._engine
        if e is None or e.batch != batch or e.device != device:
            e = self._engine = _Engine(self, batch, device)
        return e

    def forward(self, x, return_heads=False):
        """The reference's eval output (B, N, 5 + C) for a letterboxed batch ``x`` (B, channels, img_size, img_size); with
        ``return_heads`` also the list of the raw maps the yolo layers decode."""
        ops.require_gpu(x)
        ops.check_f32(x)
        c = int(self.hyperparams.get("channels", 3))
        if x.dim() != 4 or tuple(x.shape[1:]) != (c, self.img_size, self.img_size):
            raise ValueError(f"x must be (B, {c}, {self.img_size}, {self.img_size}), got {tuple(x.shape)}")
        with torch.no_grad():
            e = self._get_engine(x.shape[0], x.device)
            pred = e.run(x.contiguous())
            return (pred, [h.clone() for h in e.heads]) if return_heads else pred

    def detect(self, frames_u8):
        """uint8 RGB frames (B, H, W, 3) on the GPU -> ``(boxes_xywh (B, K, 4) float64, scores (B, K) float32, counts (B,)
        int32)`` on the device: the person boxes of each frame in frame pixels (``x, y`` the top-left corner), in the
        reference's keep order, zeros past a frame's count; ``K`` is the largest count (read back: one synchronisation)."""
        x = ops.letterbox(frames_u8, self.img_size)
        pred = self.forward(x)
        _, _, pcounts, pboxes, pscores = ops.box_nms_merge(pred, self.conf_thres, self.nms_thres, tuple(frames_u8.shape[1:3]),
                                                           self.img_size, self.person_class)
        k = int(pcounts.max())
        return pboxes[:, :k], pscores[:, :k], pcounts

    def detect_list(self, frames_u8):
        """The reference's ``human_candidates`` of every frame: a list of ``[x, y, w, h]`` lists of Python floats."""
        boxes, _, counts = self.detect(frames_u8)
        boxes, counts = boxes.cpu().tolist(), counts.cpu().tolist()
        return [[list(b) for b in boxes[i][:counts[i]]] for i in range(len(counts))]


class _Engine:
    """Folded, packed weights, the buffers of one batch size and the launch list of a :class:`PersonDetector`."""

    def __init__(self, model, batch, device):
        plan, blocks = model._plan, model.module_defs
        self.batch, self.device = batch, device
        f32 = dict(dtype=torch.float32, device=device)
        cin = int(model.hyperparams.get("channels", 3))
        self.inp = torch.empty((batch, cin, model.img_size, model.img_size), **f32)
        self.pred = torch.empty((batch, model.num_rows, 5 + model.num_classes), **f32)
        self.heads, self.steps = [], []
        # ---- where every layer's output lives: a slice of the concat buffer of the first two-layer route that reads it, a
        # one-layer route is the view of its source, everything else owns a tensor
        home = {}
        for i, d in enumerate(blocks):
            if d["type"] == "route" and len(plan.src[i]) == 2:
                c, h, w = plan.shape[i]
                buf, off = torch.empty((batch, c, h, w), **f32), 0
                home[i] = ops.View(buf)
                for j in plan.src[i]:
                    cj = plan.shape[j][0]
                    if j not in home and blocks[j]["type"] != "route" and j not in plan.fused_into:
                        home[j] = ops.View(buf, off, cj)
                    off += cj
        scratch_elems = max([batch * math.prod(plan.shape[i]) for i, d in enumerate(blocks)
                             if d["type"] == "convolutional" and d["activation"] == "leaky"] + [1])
        scratch = torch.empty(scratch_elems, **f32)
        views = []

        def own(i):
            if i not in home:
                home[i] = ops.View(torch.empty((batch,) + plan.shape[i], **f32))
            return home[i]

        def copy_into(dst_buf, off, v):
            self.steps.append(("pass", ops.leaky_pass_args(v, ops.View(dst_buf, off, v.C), None, False, 1)))

        row_off = 0
        pending = None                                              # (raw View of a leaky conv whose pass the next block runs)
        for i, d in enumerate(blocks):
            t = d["type"]
            src = [views[j] if j >= 0 else ops.View(self.inp) for j in plan.src[i]]
            if t == "convolutional":
                seq = model.module_list[i]
                conv = seq[0]
                w = conv.weight.detach().to(**f32).contiguous()
                if len(seq) > 1:
                    bn = seq[1]
                    scale = (bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps))
                    shift = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
                    scale, shift = scale.to(**f32).contiguous(), shift.to(**f32).contiguous()
                else:
                    scale, shift = None, conv.bias.detach().to(**f32).contiguous()
                wp = ops.pack_conv_weight(w)
                cout, ho, wo = plan.shape[i]
                k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
                if d["activation"] == "leaky":
                    raw = ops.View(scratch[:batch * cout * ho * wo].view(batch, cout, ho, wo))
                    desc = ops.conv_desc(src[0], raw, cout, k, k, s, p, 1)
                    self.steps.append(("conv", ops.conv2d_args(src[0], wp, scale, shift, raw, desc), (wp, scale, shift, desc)))
                    if i in plan.fused_into:
                        pending = raw
                        views.append(None)
                    else:
                        self.steps.append(("pass", ops.leaky_pass_args(raw, own(i), None, True, 1)))
                        views.append(home[i])
                else:
                    out = own(i)
                    desc = ops.conv_desc(src[0], out, cout, k, k, s, p, 1)
                    self.steps.append(("conv", ops.conv2d_args(src[0], wp, scale, shift, out, desc), (wp, scale, shift, desc)))
                    views.append(out)
            elif t == "shortcut":
                if pending is not None:
                    self.steps.append(("pass", ops.leaky_pass_args(pending, own(i), src[1], True, 1)))
                else:
                    self.steps.append(("pass", ops.leaky_pass_args(src[0], own(i), src[1], False, 1)))
                pending = None
                views.append(home[i])
            elif t == "upsample":
                if pending is not None:
                    self.steps.append(("pass", ops.leaky_pass_args(pending, own(i), None, True, 2)))
                else:
                    self.steps.append(("pass", ops.leaky_pass_args(src[0], own(i), None, False, 2)))
                pending = None
                views.append(home[i])
            elif t == "route":
                if len(src) == 1:
                    views.append(src[0])
                else:
                    cat, off = home[i], 0
                    for j, v in zip(plan.src[i], src):
                        if not (v.t is cat.t and v.coff == off):
                            copy_into(cat.t, off, v)                # a source that lives elsewhere (read by two routes, a route)
                        off += v.C
                    views.append(cat)
            else:                                                   # yolo
                v = src[0]
                if v.coff != 0 or v.C != v.ctot:
                    dense = ops.View(torch.empty((batch, v.C) + tuple(v.t.shape[2:]), **f32))
                    copy_into(dense.t, 0, v)
                    v = dense
                args, keep = ops.yolo_decode_args(v.t, self.pred, d["_anchors"], d["_classes"], model.net_size, row_off)
                self.steps.append(("decode", args, keep))
                self.heads.append(v.t)
                row_off += plan.shape[i][0]
                views.append(None)
        # the launch list holds raw pointers: the tensors behind them live as long as the engine
        self._buffers = (scratch, [v.t for v in home.values()], [v.t for v in views if v is not None])
        self.launches = len(self.steps)

    def run(self, x):
        from . import hip
        lib = hip.lib()
        fns = {"conv": (lib.otp_conv2d, "otp_conv2d"), "pass": (lib.otp_leaky_pass, "otp_leaky_pass"),
               "decode": (lib.otp_yolo_decode, "otp_yolo_decode")}
        self.inp.copy_(x)
        stream = hip.stream_of(self.inp)
        for step in self.steps:
            fn, name = fns[step[0]]
            hip.check(fn(*step[1], stream), name)
        return self.pred.clone()
