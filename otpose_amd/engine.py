"""Inference engine: the OTPose forward (reference model/OTPose.py:307-394) as a fixed list of HIP
launches over pre-allocated HBM buffers, replayed as one hipGraph.

Built once per (model, batch size): BatchNorm (eval statistics) and conv biases are folded into the
per-channel scale/shift epilogue of ``otp_conv2d``, weights are re-laid-out for the kernels
(``otp_conv2d_pack_weight``), every activation gets a static buffer (288 GB of HBM: nothing is
recycled inside a forward, so the whole launch sequence is capturable), channel concatenations and
splits become channel-offset views, residual adds / ReLU / GELU / nearest-upsample-accumulate /
residual-scale live in conv epilogues, and the 5-dilation weighted sum is folded into the DCN store.

Data layout: everything NCHW float32, frames of a clip stacked on the batch axis in the reference's
order [cur | prev | next | pprev | nnext] x B (OTPose.py:317) without materialising the re-layout
(``frame_split`` addressing in the stem conv).

Which kernel runs a layer is decided by the layer's shape and by :class:`Routes`, the ``OTPOSE_*`` switches read once per engine;
what a launch is handed is stated once, by the ``*_args`` functions of :mod:`ops` that the eager wrappers use too.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
import os
import sys
import warnings
from typing import Callable, List, Optional, Tuple

import torch

from . import hip, ops
from .ops import ACT_GELU, ACT_NONE, ACT_RELU, View

def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def plain_conv(cv, k, stride=1, pad="same", dil=1, groups=1, bias=False, cin=None, cout=None) -> bool:
    """``cv`` is a k x k Conv2d with this stride, padding ("same": dil * (k // 2)), dilation, group count, presence of a bias and
    (when given) channel counts.  ``None`` leaves a field untested."""
    if pad == "same":
        pad = (dil or 1) * (k // 2)
    return (cv.kernel_size == (k, k) and (stride is None or cv.stride == (stride, stride))
            and (pad is None or tuple(cv.padding) == (pad, pad)) and (dil is None or tuple(cv.dilation) == (dil, dil))
            and (groups is None or cv.groups == groups) and (bias is None or (cv.bias is not None) == bias)
            and (cin is None or cv.in_channels == cin) and (cout is None or cv.out_channels == cout))


@dataclasses.dataclass(frozen=True)
class Routes:
    """The ``OTPOSE_*`` switches of the two inference engines, read once (:meth:`from_env`) when an engine is built.  The field
    defaults are the defaults of the switches; every route stays reachable through its switch (tests/test_gpu_e2e.py)."""
    use_graph: bool = True            # OTPOSE_HIP_GRAPH: replay the launch list as one captured hipGraph
    use_winograd: bool = True         # OTPOSE_WINOGRAD: 3x3 stride-1 convs via csrc/wino.hip
    # OTPOSE_CONV_MATH: "x3" = fp32 operands split into two bf16 pieces, three bf16 MFMAs per product, fp32 accumulate
    # (csrc/convx.hip); "f32" = the f32 MFMA kernels only (Winograd / direct)
    use_x3: bool = True
    # OTPOSE_DCN_FUSED (needs x3): offset / mask convs + DCN gathers of all dilations in one launch
    use_dcn_fused: bool = True
    # OTPOSE_S8 (needs x3): HRNet branches (chains of BasicBlocks) on split-record activations fed by the LDS-DMA (csrc/convs.hip)
    use_s8: bool = True
    use_flow_fused: bool = True       # OTPOSE_FLOW_FUSED: flow-encoder blocks via csrc/flowenc.hip
    use_small_conv: bool = True       # OTPOSE_SMALL_CONV: RSB staircase convs via csrc/conv_small.hip
    use_fused_mlp: bool = True        # OTPOSE_FUSED_MLP: transformer MLP via csrc/mlp.hip
    fuse_shortcut: bool = True        # OTPOSE_FUSE_SHORTCUT: layer1 shortcut folded into conv3
    fuse_upsample: bool = True        # OTPOSE_FUSE_UPSAMPLE: a fuse row's upsampled terms in one pass
    use_dense_cc: bool = True         # OTPOSE_DENSE_CC: q / k / v / proj via csrc/dense.hip
    use_qkv_front: bool = True        # OTPOSE_QKV_FRONT: + dwconv / LayerNorm fused in front of them
    use_pointx: bool = True           # OTPOSE_POINTX (needs x3): layer1's 1x1 convs via csrc/pointx.hip
    pointx_fuse: bool = True          # OTPOSE_POINTX_FUSE: ... and the fuse layers' (any multiple of 16 input channels)
    pointx_any: bool = False          # OTPOSE_POINTX_ANY=1 (opt-in: the RSB heads' and the final 1x1 convs too - 26.69 against
    #                                   26.72 ms, and they leave exact fp32)
    # OTPOSE_STREAMS: independent sub-graphs (the HRNet branches of a stage, the rows of its fuse layer, the two temporal
    # encoders) are emitted on side HIP streams: inside the captured graph they become parallel branches, so the small-map
    # launches (640-960 workgroups on 512 resident slots) fill each other's tails
    multi_stream: bool = True
    # OTPOSE_F32_TAIL (0 without x3): the last n HighResolutionModules of stage 4 and the backbone's final 1x1 conv on the exact-fp32
    # MFMA kernels (Winograd / direct) instead of split products: the layers whose rounding reaches `rough` un-attenuated
    # 
    f32_tail: int = 0
    # OTPOSE_H16_TAIL: fp16 engine (engine_h16.py) - the encoders' matrix kernels also take their operands as halves rounded once
    # (csrc/mlpx.hip, csrc/densex.hip: the *_h1 entry points); 0 keeps their split products
    h16_tail: bool = True
    # OTPOSE_RANGE_CHECK: range guard of the half-piece arithmetic (csrc/range.hip, csrc/common.h:75): "defer" (default) raises at
    # the NEXT forward / at check_range() and NaN-fills this forward's heat-maps on the device; "sync" synchronises and raises in
    # the forward that overflowed; "off" only keeps the device-side NaN fill
    range_check: str = "defer"
    s8_residual: bool = True          # OTPOSE_S8_RESIDUAL: a BasicBlock's residual from its input's S8 records, not a C4 fp32 image
    s8_lazy_nchw: bool = True         # OTPOSE_S8_LAZY_NCHW: see :attr:`lazy_nchw`
    s8_stride2: bool = True           # OTPOSE_S8_STRIDE2: stride-2 conv chains on S8 records (csrc/convs2.hip)
    t1_s8: bool = True                # OTPOSE_T1_S8: transition1's convs read layer1's result as S8 records
    l1_s8: bool = True                # OTPOSE_L1_S8: a Bottleneck's conv1 -> conv2 intermediate as S8 records
    l1_pair: bool = True              # OTPOSE_L1_PAIR: a Bottleneck's conv3 and the next one's conv1 in one launch
    stem_x3: bool = True              # OTPOSE_STEM_X3: the stem's first conv via csrc/stem.hip
    chain_modules: bool = True        # OTPOSE_CHAIN_MODULES: consecutive modules of a stage chained stream by stream
    up_any_width: bool = True         # OTPOSE_UP_ANY_WIDTH: otp_upsample_add for widths that are no multiple of 4
    # development aids
    conv_log: bool = False            # OTPOSE_CONV_LOG: one line per emitted convolution
    poison: Optional[Tuple[int, int]] = None   # OTPOSE_POISON="lo:hi": NaN-fill the activation buffers with these indices
    te_serial: bool = False           # OTPOSE_TE_SERIAL=1: both temporal encoders on the main stream

    @classmethod
    def from_env(cls) -> "Routes":
        env = os.environ.get
        on = lambda name: env("OTPOSE_" + name, "1") != "0"                         # noqa: E731
        x3 = env("OTPOSE_CONV_MATH", "x3") != "f32"
        poison = env("OTPOSE_POISON")
        return cls(use_graph=on("HIP_GRAPH"), use_winograd=on("WINOGRAD"), use_x3=x3, use_dcn_fused=x3 and on("DCN_FUSED"),
                   use_s8=x3 and on("S8"), use_flow_fused=on("FLOW_FUSED"), use_small_conv=on("SMALL_CONV"),
                   use_fused_mlp=on("FUSED_MLP"), fuse_shortcut=on("FUSE_SHORTCUT"), fuse_upsample=on("FUSE_UPSAMPLE"),
                   use_dense_cc=on("DENSE_CC"), use_qkv_front=on("QKV_FRONT"), use_pointx=x3 and on("POINTX"),
                   pointx_fuse=on("POINTX_FUSE"), pointx_any=env("OTPOSE_POINTX_ANY", "0") == "1", multi_stream=on("STREAMS"),
                   f32_tail=int(env("OTPOSE_F32_TAIL", "0")) if x3 else 0, h16_tail=on("H16_TAIL"),
                   range_check=env("OTPOSE_RANGE_CHECK", "defer"), s8_residual=on("S8_RESIDUAL"), s8_lazy_nchw=on("S8_LAZY_NCHW"),
                   s8_stride2=on("S8_STRIDE2"), t1_s8=on("T1_S8"), l1_s8=on("L1_S8"), l1_pair=on("L1_PAIR"), stem_x3=on("STEM_X3"),
                   chain_modules=on("CHAIN_MODULES"), up_any_width=on("UP_ANY_WIDTH"), conv_log=bool(env("OTPOSE_CONV_LOG")),
                   poison=tuple(int(v) for v in poison.split(":")) if poison else None, te_serial=env("OTPOSE_TE_SERIAL") == "1")

    @property
    def lazy_nchw(self) -> bool:
        """A tensor that also exists as S8 records gets its NCHW form written only if some consumer asks for it before the first
        launch (``InferenceEngine._needs_nchw``); needs the S8 residual - the C4 residual chain reads the NCHW-born images."""
        return self.s8_residual and self.s8_lazy_nchw


class Aux:
    """The S8 / C4 images of an NCHW activation written by its producer, and whether any consumer reads the NCHW tensor itself."""
    __slots__ = ("s8", "c4", "nchw_needed")

    def __init__(self, s8=None, c4=None, nchw_needed=False):
        self.s8, self.c4, self.nchw_needed = s8, c4, nchw_needed


class InferenceEngine:
    h16 = False

    def __init__(self, model, batch: int, device, use_graph: bool | None = None, stream_set: int = 0, inp=None, margin=None):
        routes = Routes.from_env()
        self._init(device, routes, routes.use_graph if use_graph is None else use_graph, stream_set)
        self.B = batch
        self.model = model
        cfg = model.cfg
        self.J = model.num_joints
        self.F = getattr(model, "window_frames", 5)             # frames per clip window
        self.W_img, self.H_img = cfg.MODEL.IMAGE_SIZE
        self.h, self.w = model.pe_h, model.pe_w
        self._given = (inp, margin)
        self.param_version = self._param_version()
        with torch.no_grad():
            self._build()

    def _init(self, device, routes: Routes, use_graph: bool, stream_set: int = 0):
        """State shared by a full engine and a :meth:`bare` one."""
        device = torch.device(device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("otpose_amd.OTPose runs on an MI355X through libotpose_hip.so; "
                               f"got device '{device}' (there is no CPU or PyTorch-op fallback)")
        self.lib, self.dev, self.routes = hip.lib(), device, routes
        self.model, self.B, self.inp, self.margin = None, 0, None, None
        self.ops: List[Callable] = []
        self._pair_s8 = {}                    # id(NCHW tensor) -> S8 image of the next Bottleneck's conv1, written with it (pointx_pair)
        self.l1_pairs = 0                     # conv3 + next conv1 pair launches emitted (tests)
        self._aux = {}                        # id(NCHW tensor) -> Aux: S8 / C4 images written by its producer
        self._keep = []                       # parameter-derived tensors that must outlive the ops
        self._bufs = []                       # every activation buffer (see new())
        self._stream = None
        self.use_graph, self.graph = use_graph, None
        self._exact = False                   # this part of the backbone runs on the exact-fp32 kernels (Routes.f32_tail)
        self._sid = 0
        # process-wide pool (see hip.side_streams); stream_set > 0: the streams of another sub-batch of a PipelinedEngine
        self._side = hip.side_streams(device, 3, 4 * stream_set) if routes.multi_stream else []

    @classmethod
    def bare(cls, device, multi_stream=False):
        """An engine with NO model behind it, for tests of one sub-module: the caller emits that module's launches with the
        engine's own emitters (``rsb_chain``, ``tblock``, ...) on buffers from :meth:`new`, sets ``inp`` to any of them (its
        stream is the launch stream) and runs the list with :meth:`_launch_all` - exactly the launches a full engine would
        issue for that module, without building an OTPose around it.  Never captures a graph."""
        self = cls.__new__(cls)
        self._init(device, dataclasses.replace(Routes.from_env(), multi_stream=bool(multi_stream)), use_graph=False)
        return self

    # ---- routes: what callers and tests read, and the conditions that combine a route with the per-module ``_exact`` state ------
    use_x3 = property(lambda self: self.routes.use_x3)
    use_dcn_fused = property(lambda self: self.routes.use_dcn_fused)
    multi_stream = property(lambda self: self.routes.multi_stream)
    f32_tail = property(lambda self: self.routes.f32_tail)
    range_check = property(lambda self: self.routes.range_check)
    half_products = property(lambda self: self.h16 and self.routes.use_x3 and self.routes.h16_tail)

    @property
    def s8_here(self) -> bool:
        """Split-record (S8) kernels for the layer being emitted."""
        return self.routes.use_s8 and not self._exact

    @property
    def s2_here(self) -> bool:
        """Stride-2 conv chains on S8 records for the layer being emitted."""
        return self.routes.use_s8 and not self._exact and self.routes.s8_stride2

    # ---------------------------------------------------------------------------------------------
    def matches(self, x) -> bool:
        return (x.shape[0] == self.B and x.device == self.dev and tuple(x.shape[2:]) == (self.H_img, self.W_img)
                and self._param_version() == self.param_version)

    def matches_shape(self, b, c, h, w, dev) -> bool:
        return (b == self.B and dev == self.dev and (h, w) == (self.H_img, self.W_img) and c == 3 * self.F
                and self._param_version() == self.param_version)

    def _param_version(self):
        """Staleness key of the packed weights: (storage address, autograd version) of every parameter AND buffer
        (BatchNorm running statistics are folded into the conv epilogues), so in-place updates (optimizer steps,
        ``load_state_dict``, ``running_mean.copy_``), re-pointed ``.data`` and module surgery are all seen.  Writes
        through ``p.data`` / raw pointers bump no version: call ``OTPose.invalidate_engine()`` after those."""
        ts = getattr(self, "_tracked", None)
        if ts is None:
            ts = self._tracked = list(self.model.parameters()) + list(self.model.buffers())
        v = a = 0
        for t in ts:
            v += t._version
            a ^= t.data_ptr()
        return (len(ts), v, a)

    def new(self, *shape):
        """A static activation / scratch buffer.  The engine owns it for its whole life: the launch list holds
        raw device pointers, and torch.cuda.graph() empties the allocator cache before capturing."""
        t = torch.empty(shape, dtype=torch.float32, device=self.dev)
        rng = self.routes.poison                               # development aid: find a kernel that reads memory nothing wrote
        if rng and rng[0] <= len(self._bufs) < rng[1]:         # (tools/poison_engine.py)
            t.fill_(float("nan"))
        self._bufs.append(t)
        return t

    def dev_param(self, t):
        t = t.detach().to(self.dev, torch.float32).contiguous()
        self._keep.append(t)
        return t

    winograd_pays = staticmethod(ops.winograd_pays)            # (kept under this name for its callers)

    # ---- op emitters ----------------------------------------------------------------------------
    def _emit(self, fn):
        self.ops.append((fn, self._sid))

    def fork(self, sids):
        """Side streams ``sids`` (1-based) start after everything emitted so far on the main stream."""
        if not self.multi_stream:
            return
        sids = [s for s in sids if 0 < s <= len(self._side)]

        def run():
            main = torch.cuda.current_stream(self.dev)
            for s_ in sids:
                self._side[s_ - 1].wait_stream(main)
        self.ops.append((run, -1))

    def join(self, sids):
        """The main stream waits for everything emitted on side streams ``sids``."""
        if not self.multi_stream:
            return
        sids = [s for s in sids if 0 < s <= len(self._side)]

        def run():
            main = torch.cuda.current_stream(self.dev)
            for s_ in sids:
                main.wait_stream(self._side[s_ - 1])
        self.ops.append((run, -1))

    def on_stream(self, sid):
        """Ops emitted from now on go to side stream ``sid`` (0 = main; ids past the pool fall back to main)."""
        self._sid = sid if (self.multi_stream and 0 <= sid <= len(self._side)) else 0

    def call(self, fn, name, *args):
        """Record one launch: ``args`` (an ``ops.*_args`` tuple) are fixed now, the stream is the one the op is replayed on."""
        def run():
            hip.check(fn(*args, self._stream), name)
        self._emit(run)

    def call_lazy_nchw(self, aux: Aux, fn, name, args_of, unpack=None):
        """Record one launch whose NCHW output pointer is decided at the first launch: ``args_of(nchw)`` states its arguments
        with (True) and without (False) that pointer, and the tensor is written only if a consumer has asked for it by then
        (:meth:`_needs_nchw`).  ``unpack``: the arguments of an ``otp_s8_unpack`` pass behind a launch that cannot write the
        NCHW tensor itself."""
        full, lean = args_of(True), args_of(False)
        if unpack is None:
            def run():
                hip.check(fn(*(full if aux.nchw_needed else lean), self._stream), name)
        else:
            s8_unpack = self.lib.otp_s8_unpack

            def run():
                hip.check(fn(*lean, self._stream), name)
                if aux.nchw_needed:                         # (a consumer without an S8 path: hi + lo back to fp32 NCHW)
                    hip.check(s8_unpack(*unpack, self._stream), "otp_s8_unpack")
        self._emit(run)

    def _bn_fold(self, bn, bias=None):
        """BatchNorm (eval) as a per-channel scale and shift, a conv bias in front of it folded into the shift."""
        g, b = self.dev_param(bn.weight), self.dev_param(bn.bias)
        mu, var = self.dev_param(bn.running_mean), self.dev_param(bn.running_var)
        sc = (g / torch.sqrt(var + bn.eps)).contiguous()
        sh = b - mu * sc
        if bias is not None:
            sh = sh + self.dev_param(bias) * sc
        sh = sh.contiguous()
        self._keep += [sc, sh]
        return sc, sh

    def conv(self, inp: View, weight, out: View, stride=1, pad=0, dil=1, bn=None, bias=None, act=ACT_NONE,
             res: View = None, in2: View = None, res_up=1, frame_split=0, cin=None, scale=None, shift=None):
        """Emit act(scale*conv(inp (+in2)) + shift (+res)) with BN / bias folded into scale / shift."""
        for v_ in (inp, in2, res):
            self._needs_nchw(v_)
        r = self.routes
        w = self.dev_param(weight)
        if w.dim() == 3:
            w = w.unsqueeze(-1)
        cout, cin_w, kh, kw = w.shape
        if bn is not None:
            sc, sh = self._bn_fold(bn, bias)
        else:
            sc = self.dev_param(scale) if scale is not None else None
            sh = shift if shift is not None else bias
            sh = self.dev_param(sh) if sh is not None else None
        d = ops.conv_desc(inp, out, cout, kh, kw, stride, pad, dil, act, in2, res, res_up, frame_split, cin)
        self._keep.append(d)
        L = self.lib
        route = self._conv_route(d, inp, cin_w, res, in2)
        if r.conv_log:                                              # development aid: one line per emitted convolution
            print(f"conv {d.N}x{d.Cin}->{cout} k{kh} s{stride} p{pad} d{dil} {d.H}x{d.W} in2={in2 is not None} "
                  f"res={res is not None} up={res_up} fs={frame_split} {route}", file=sys.stderr)
        if route == "small":
            # RSB staircase convs (a few channels, pre-added second input): one thread per pixel, exact fp32 (csrc/conv_small.hip)
            wc = ops.pack_small_conv_weight(w)
            self._keep.append(wc)
            self.call(L.otp_conv3x3_small, "otp_conv3x3_small", *ops.conv3x3_small_args(inp, in2, wc, sc, sh, out, d))
        elif route == "pointx":
            # HRNet layer1's and the fuse layers' 1x1 convs (<= 256 channels in and out): register-resident pixels, streamed weights
            # (csrc/pointx.hip) - bound by their HBM streams, which the implicit-GEMM kernel ran at a third of the rate
            pk = ops.pack_pointwise_x3(w, sc, sh)
            self._keep.append(pk)
            self.call(L.otp_pointwise_x3, "otp_pointwise_x3", *ops.pointwise_x3_args(inp, pk, out, res, act == ACT_RELU))
        elif route == "x3":
            # 3x3 / stride 1 with Cin % 16 == 0: split-half (f16x3) products on the 16-bit matrix cores, fp32 storage and
            # accumulation (csrc/convx.hip); the per-channel scale is folded into the packed weights
            e = ops.x3_weight_exponent(w, sc)         # weights stored times 2^e, the sum multiplied by 2^-e (otp_conv_desc.out_scale)
            d.out_scale = 2.0 ** -e
            xp = ops.pack_x3_weight(w, sc, stride, e)
            self._keep.append(xp)
            self.call(L.otp_conv2d_x3, "otp_conv2d_x3", *ops.conv2d_x3_args(inp, xp, sh, out, d, res))
        elif route == "wino":
            # 3x3 / stride 1 / pad 1 with enough channels: Winograd F(2x2,3x3) kernel (csrc/wino.hip), same epilogue
            up = ops.pack_wino_weight(w)
            self._keep.append(up)
            self.call(L.otp_conv2d_wino, "otp_conv2d_wino", *ops.conv2d_wino_args(inp, up, sc, sh, out, d, res))
        else:
            wp = ops.pack_conv_weight(w)
            self._keep.append(wp)
            self.call(L.otp_conv2d, "otp_conv2d", *ops.conv2d_args(inp, wp, sc, sh, out, d, in2, res))
        return out

    def _conv_route(self, d, inp: View, cin_w, res: View, in2: View):
        """Which kernel runs the convolution ``d``: "small" | "pointx" | "x3" | "wino" | "direct", first match wins."""
        r = self.routes
        k, cout = (d.kh, d.kw), d.Cout
        if r.use_small_conv and in2 is not None and res is None and k == (3, 3) and ops.small_conv_supported(d):
            return "small"
        if (r.use_pointx and not self._exact and in2 is None and k == (1, 1) and d.stride == 1 and d.pad == 0 and d.res_up <= 1
                and not d.frame_split and d.act in (ACT_NONE, ACT_RELU) and inp.C == cin_w
                and (cin_w in (64, 128, 256) or (r.pointx_fuse and cin_w % 16 == 0) or r.pointx_any)
                and ops.pointwise_x3_supported(cin_w, cout, inp.t.shape[2] * inp.t.shape[3])):
            return "pointx"
        if r.use_x3 and not self._exact and in2 is None and k in ((3, 3), (1, 1)) and ops.x3_supported(d):
            return "x3"
        if in2 is None and ops.runs_winograd(r.use_winograd, cin_w, cout, d):
            return "wino"
        return "direct"

    def conv_bn(self, inp: View, conv_mod, bn_mod, act=ACT_NONE, res=None, out=None, res_up=1, **kw):
        n, _, h, w = inp.t.shape
        if kw.get("frame_split"):
            n = n * (inp.ctot // kw["cin"])
        k, s, p, dl = conv_mod.kernel_size[0], conv_mod.stride[0], conv_mod.padding[0], conv_mod.dilation[0]
        ho = (h + 2 * p - (dl * (k - 1) + 1)) // s + 1
        wo = (w + 2 * p - (dl * (k - 1) + 1)) // s + 1
        if out is None:
            f = max(res_up, 1)
            out = View(self.new(n, conv_mod.out_channels, ho * f, wo * f))
        return self.conv(inp, conv_mod.weight, out, s, p, dl, bn=bn_mod, bias=conv_mod.bias, act=act, res=res,
                         res_up=res_up, **kw)

    def dense(self, xs, packs, ress, outs, B, C, T):
        """Emit one otp_dense_cc (or, with split-half products, otp_dense_x3) launch over len(xs) problems."""
        ax, ap, ar, ao = ops.dense_cc_args(xs, packs, ress, outs)
        self._keep += [ax, ap, ar, ao, *packs]
        x3 = self.use_x3 and ops.dense_x3_supported(C, T)
        fn = (self.lib.otp_dense_h1 if self.half_products else self.lib.otp_dense_x3) if x3 else self.lib.otp_dense_cc
        self.call(fn, "otp_dense_cc", ax, ap, ar, ao, len(xs), B, C, T)

    # ---- HRNet (reference model/HRNet.py:116-152) -------------------------------------------------
    def basic_block(self, blk, x: View) -> View:
        y = self.conv_bn(x, blk.conv1, blk.bn1, ACT_RELU)
        res = x
        if blk.downsample is not None:
            res = self.conv_bn(x, blk.downsample[0], blk.downsample[1])
        return self.conv_bn(y, blk.conv2, blk.bn2, ACT_RELU, res=res)

    def _needs_nchw(self, v):
        """A consumer reads the NCHW tensor of ``v``: its producer must write it (see fuse_s8)."""
        a = self._aux.get(id(v.t)) if v is not None else None
        if a is not None:
            a.nchw_needed = True

    def fuse_s8(self, lows, factors, res: View, tgt: View):
        """Last op of a fuse row whose tail is upsampled terms (HRNet.py:487-494): relu(res + up(low0) + ...) written as the
        S8 and C4 images the next module's branch reads (csrc/convs.hip, otp_s8_upsample_add); the NCHW tensor ``tgt`` is
        written only if some other consumer asks for it before the first launch.  Returns False when the row is not eligible."""
        n_, c_, hh, wh = tgt.t.shape
        if not self.s8_here or tgt.coff != 0 or tgt.C != c_ or c_ % 16 or wh % 4 or (hh * wh) % 4:
            return False
        if not ops.s8_conv_supported(ops.s8_conv_desc(n_, c_, c_, hh, wh, ACT_RELU)):
            return False
        r = self.routes
        # the identity term: the S8 image of `res` when its producer wrote one (a branch output: hi + lo of the records, 2^-22) -
        # `res` then needs no NCHW tensor on this account - else the fp32 NCHW tensor
        raux = self._aux.get(id(res.t)) if (r.lazy_nchw and res.coff == 0 and res.C == c_ and res.ctot == c_) else None
        res_img = raux.s8 if raux is not None else None
        if res_img is None:
            self._needs_nchw(res)
        # (the C4 fp32 image only when the next module's branch reads its residual from it: OTPOSE_S8_RESIDUAL=0)
        s8 = self.new(n_ * c_ * hh * wh)
        c4 = None if r.s8_residual else self.new(n_ * c_ * hh * wh)
        aux = self._aux[id(tgt.t)] = Aux(s8, c4)
        lp = (ctypes.c_void_p * len(lows))(*[hip.ptr(v.t) for v in lows])
        fp = (ctypes.c_int * len(lows))(*factors)
        self._keep += [lp, fp]
        self.call_lazy_nchw(aux, self.lib.otp_s8_upsample_add_ex, "otp_s8_upsample_add", lambda nchw: (
            lp, fp, len(lows), hip.ptr(res_img if res_img is not None else res.t), int(res_img is not None),
            hip.ptr(tgt.t) if nchw else None, hip.ptr(s8), hip.ptr(c4), n_, c_, hh, wh, 1, res.ctot, res.coff, tgt.ctot, tgt.coff))
        return True

    def s8_image(self, v: View, want_c4=False):
        """The S8 image (and, on request, the C4 image) of a full NCHW tensor: what its producer already wrote (``_aux``), or one
        ``otp_s8_pack`` pass emitted here, on the current stream, and cached for later consumers.  None when the tensor is not
        eligible (channel slice, channels % 16, pixels % 4)."""
        n, c, h, w = v.t.shape
        if not self.routes.use_s8 or v.coff != 0 or v.C != c or c % 16 or (h * w) % 4:
            return None
        aux = self._aux.get(id(v.t))
        if aux is not None and aux.s8 is not None and (not want_c4 or aux.c4 is not None):
            return aux
        self._needs_nchw(v)
        s8 = aux.s8 if aux is not None and aux.s8 is not None else self.new(n * c * h * w)
        c4 = self.new(n * c * h * w) if want_c4 else None
        self.call(self.lib.otp_s8_pack, "otp_s8_pack", hip.ptr(v.t), hip.ptr(s8), hip.ptr(c4), n, c, h, w, v.ctot, v.coff)
        if aux is None:
            aux = self._aux[id(v.t)] = Aux(nchw_needed=True)
        aux.s8 = s8
        if c4 is not None:
            aux.c4 = c4
        return aux

    def s2_chain_s8(self, layers, x: View, act_last, res: View = None, out: View = None):
        """A chain of 3x3 / stride 2 conv + BN (+ ReLU) layers (a fuse layer's down-sampling path, model/HRNet.py:442-470, or a
        transition layer's new branch, :213-229) on S8 records (csrc/convs2.hip): every intermediate exists only as its S8 image,
        the last layer writes act(conv + shift (+ res)) into the fp32 NCHW tensor ``out``.  ``layers`` = [(conv, bn, relu)].
        Returns the output view, or None (nothing emitted) when a layer is not of that shape."""
        if not self.s2_here:
            return None
        n, c, h, w = x.t.shape
        if x.coff != 0 or x.C != c:
            return None
        hh, ww, cin = h, w, c
        descs = []
        for li, (cv, bn, relu) in enumerate(layers):
            last = li == len(layers) - 1
            if not plain_conv(cv, 3, stride=2, cin=cin) or hh % 2 or ww % 2:
                return None
            co = cv.out_channels
            if last:
                if out is None:
                    out = View(self.new(n, co, hh // 2, ww // 2))
                d = ops.s8_s2_conv_desc(n, cin, co, hh, ww, act_last, out, res)
            else:
                d = ops.s8_s2_conv_desc(n, cin, co, hh, ww, ACT_RELU if relu else ACT_NONE)
            if not ops.s8_s2_conv_supported(d, last):
                return None
            descs.append(d)
            hh, ww, cin = hh // 2, ww // 2, co
        aux = self.s8_image(x)
        if aux is None:
            return None
        self._needs_nchw(res)
        cur = aux.s8
        hh, ww = h, w
        for (cv, bn, relu), d in zip(layers, descs):
            wp, sh = self._pack_s8(cv, bn, d)
            if d is descs[-1]:
                args = ops.conv3x3_s2_s8_args(cur, wp, sh, d, res, out)
            else:
                nxt = self.new(n * cv.out_channels * (hh // 2) * (ww // 2))
                args = ops.conv3x3_s2_s8_args(cur, wp, sh, d, out_s8=nxt)
                cur = nxt
            self.call(self.lib.otp_conv3x3_s2_s8, "otp_conv3x3_s2_s8", *args)
            hh, ww = hh // 2, ww // 2
        return out

    def _pack_s8(self, conv, bn, desc):
        """Packed split-product weights of a 3x3 conv + BN for csrc/convs.hip / convs2.hip, stored times the layer's power of two
        (ops.x3_weight_exponent) with the inverse in ``desc.out_scale``, and the BN shift."""
        sc, sh = self._bn_fold(bn)
        w = self.dev_param(conv.weight)
        e = ops.x3_weight_exponent(w, sc)
        desc.out_scale = 2.0 ** -e
        wp = ops.pack_s8_weight(w, sc, e)
        self._keep += [wp, desc]
        return wp, sh

    def conv_s8(self, x8, conv, bn, d, **outputs):
        """Emit one otp_conv3x3_s8 launch: bn(conv(S8 image ``x8``)) by descriptor ``d``; ``outputs``: the residual and output
        arguments of ``ops.conv3x3_s8_args``."""
        wp, sh = self._pack_s8(conv, bn, d)
        self.call(self.lib.otp_conv3x3_s8, "otp_conv3x3_s8", *ops.conv3x3_s8_args(x8, wp, sh, d, **outputs))

    def conv_s8_lazy(self, x8, conv, bn, d, out: View, o8, res=None):
        """:meth:`conv_s8` writing the S8 image ``o8`` (if any) and, registered as lazily written when there is one and
        ``Routes.lazy_nchw``, the NCHW tensor ``out``."""
        wp, sh = self._pack_s8(conv, bn, d)
        aux = Aux(o8, nchw_needed=o8 is None or not self.routes.lazy_nchw)
        if o8 is not None:
            self._aux[id(out.t)] = aux
        self.call_lazy_nchw(aux, self.lib.otp_conv3x3_s8, "otp_conv3x3_s8", lambda nchw: ops.conv3x3_s8_args(
            x8, wp, sh, d, res, out.t if nchw else None, ops.S8_F32_NCHW, o8))

    def branch_s8(self, blocks, x: View, want_s8=False):
        """A branch of a HighResolutionModule (HRNet.py:478-496: 4 BasicBlocks, :500-530) on split-record activations
        (csrc/convs.hip).  The branch input is converted once to its S8 image (the MFMA operand records): conv input AND
        residual (round 4; before: a C4 fp32 image next to it); inside the branch conv1 goes S8 -> S8, conv2 S8 + S8 residual ->
        S8; the last conv2 writes the NCHW tensor the fuse layer reads.  Returns None when the branch is not of that
        shape (the caller then emits the blocks one convolution at a time)."""
        n, c, h, w = x.t.shape
        if not self.s8_here or x.coff != 0 or x.C != c:
            return None
        for blk in blocks:
            convs = (getattr(blk, "conv1", None), getattr(blk, "conv2", None))
            if (getattr(blk, "downsample", None) is not None or hasattr(blk, "conv3")
                    or any(cv is None or not plain_conv(cv, 3, cin=c, cout=c) for cv in convs)):
                return None
        if not ops.s8_conv_supported(ops.s8_conv_desc(n, c, c, h, w, ACT_RELU)):
            return None
        new_img = lambda: self.new(n * c * h * w)                          # noqa: E731  (S8 and C4 images are 4 bytes per element)
        # residual of a block: its input's S8 records (hi + lo holds the value to 2^-22: otp_conv_desc.res_layout = 1) - no fp32 (C4)
        # image exists between the blocks of a branch; OTPOSE_S8_RESIDUAL=0: the exact fp32 residual chain of round 3
        res_s8 = self.routes.s8_residual
        aux = self.s8_image(x, want_c4=not res_s8)                         # written by the producer (a fuse row), or packed here
        if aux is None:
            return None
        x8, xres = aux.s8, (aux.s8 if res_s8 else aux.c4)
        for b, blk in enumerate(blocks):
            y8 = new_img()
            self.conv_s8(x8, blk.conv1, blk.bn1, ops.s8_conv_desc(n, c, c, h, w, ACT_RELU), out_s8=y8)
            if b == len(blocks) - 1:
                out = View(self.new(n, c, h, w))
                d2 = ops.s8_conv_desc(n, c, c, h, w, ACT_RELU, out)
                d2.res_layout = int(res_s8)
                # a stride-2 consumer in the fuse layer (csrc/convs2.hip) reads the S8 image: written here, next to the NCHW tensor.
                # Consumers that can read the S8 image (stride-2 chains, the fuse row's identity term) do; the NCHW tensor is
                # written only if some consumer asks for it before the first launch (_needs_nchw)
                self.conv_s8_lazy(y8, blk.conv2, blk.bn2, d2, out, new_img() if want_s8 else None, res=xres)
                return out
            oc4, o8 = (None if res_s8 else new_img()), new_img()
            d2 = ops.s8_conv_desc(n, c, c, h, w, ACT_RELU)
            d2.res_layout = int(res_s8)
            self.conv_s8(y8, blk.conv2, blk.bn2, d2, res=xres, out_f32=oc4, out_s8=o8)
            x8, xres = o8, (o8 if res_s8 else oc4)
        return None

    def conv_bn_s8(self, x: View, conv, bn, act=ACT_RELU):
        """act(bn(conv3x3 stride 1 pad 1 (x))) on csrc/convs.hip from the S8 image of ``x`` (packed here unless its producer wrote
        one), result as S8 records for the branch that follows and as the NCHW tensor only if another consumer asks for it.
        Returns None (nothing emitted) when the layer is not of that shape."""
        n, c, h, w = x.t.shape
        if not self.s8_here or not plain_conv(conv, 3, cin=c) or x.coff != 0 or x.C != c or conv.out_channels % 16:
            return None
        co = conv.out_channels
        out = View(self.new(n, co, h, w))
        d = ops.s8_conv_desc(n, c, co, h, w, act, out)
        if not ops.s8_conv_supported(d):
            return None
        aux = self.s8_image(x)
        if aux is None:
            return None
        self.conv_s8_lazy(aux.s8, conv, bn, d, out, self.new(n * co * h * w))
        return out

    def _conv1_conv2_s8_ok(self, xc, n, h, w, conv1, conv2) -> bool:
        """Shape test of :meth:`conv1_conv2_s8` for an input of ``xc`` channels (the conv's own buffer as output)."""
        r = self.routes
        if not (r.use_s8 and r.use_pointx and r.l1_s8):
            return False
        c1o = conv1.out_channels
        if not (plain_conv(conv1, 1, cin=xc) and plain_conv(conv2, 3, cin=c1o) and ops.pointwise_x3_s8_supported(xc, c1o, h * w)):
            return False
        return bool(ops.s8_conv_supported(ops.s8_conv_desc(n, c1o, conv2.out_channels, h, w, ACT_RELU)))

    def pointx_pair(self, inp: View, weight, sc, sh, res: View, nxt):
        """relu(sc * conv1x1(inp) + sh (+ res)) in front of Bottleneck ``nxt`` (a layer1 block boundary, HRNet.py:551-571) with
        nxt's conv1 + bn1 + relu in the same launch (csrc/pointx.hip, pointx_pair_kernel): the 256-channel tensor is written for
        nxt's residual and not read back, nxt's conv1_conv2_s8 finds the S8 image of its conv1 ready.  The same bits as the two
        launches; OTPOSE_L1_PAIR=0 keeps those.  Returns None when either convolution is not of that shape."""
        if not (self.routes.use_pointx and not self._exact and self.routes.l1_pair):
            return None
        w = self.dev_param(weight)
        n, _, h, wd = inp.t.shape
        cmid, cin = w.shape[:2]
        c1 = nxt.conv1
        if (w.dim() == 4 and tuple(w.shape[2:]) != (1, 1)) or inp.C != cin or (res is not None and res.C != cmid) \
                or not ops.pointwise_x3_supported(cin, cmid, h * wd) or not self._conv1_conv2_s8_ok(cmid, n, h, wd, c1, nxt.conv2) \
                or not ops.pointwise_x3_pair_supported(cin, cmid, c1.out_channels, h * wd) or (cin == 64) != (res is not None):
            return None
        for v_ in (inp, res):
            self._needs_nchw(v_)
        sc1, sh1 = self._bn_fold(nxt.bn1)
        pk = ops.pack_pointwise_x3_pair(w, sc, sh, self.dev_param(c1.weight), sc1, sh1)
        out = View(self.new(n, cmid, h, wd))
        y8 = self.new(n * c1.out_channels * h * wd)
        self._keep.append(pk)
        self._pair_s8[id(out.t)] = y8
        self.l1_pairs += 1
        self.call(self.lib.otp_pointwise_x3_pair, "otp_pointwise_x3_pair",
                  *ops.pointwise_x3_pair_args(inp, pk, out, c1.out_channels, y8, res))
        return out

    def conv1_conv2_s8(self, x: View, conv1, bn1, conv2, bn2, out: View = None):
        """relu(bn2(conv2(relu(bn1(conv1(x)))))) of a Bottleneck (HRNet.py:551-571: 1x1 then 3x3) with the intermediate kept as S8
        records: conv1 on csrc/pointx.hip writes the operand records of csrc/convs.hip, conv2 reads them and writes fp32 NCHW -
        no fp32 round trip of the 64-channel tensor and the S8 conv kernel instead of the implicit-GEMM one (179 -> 115 us at
        cfg2).  Returns None when the pair is not of that shape."""
        n, _, h, w = x.t.shape
        c1i, c1o, c2o = conv1.in_channels, conv1.out_channels, conv2.out_channels
        if not self._conv1_conv2_s8_ok(x.C, n, h, w, conv1, conv2):
            return None
        if out is None:
            out = View(self.new(n, c2o, h, w))
        d2 = ops.s8_conv_desc(n, c1o, c2o, h, w, ACT_RELU, out)
        if not ops.s8_conv_supported(d2):
            return None
        y8 = self._pair_s8.pop(id(x.t), None)          # conv1's S8 image, already written by the launch that wrote x (pointx_pair)
        if y8 is None:
            self._needs_nchw(x)
            sc1, sh1 = self._bn_fold(bn1)
            pk = ops.pack_pointwise_x3_s8(self.dev_param(conv1.weight), sc1, sh1)
            y8 = self.new(n * c1o * h * w)
            self._keep.append(pk)
            self.call(self.lib.otp_pointwise_x3_s8, "otp_pointwise_x3_s8", hip.ptr(x.t), hip.ptr(pk), hip.ptr(y8), n, c1i, c1o, h * w,
                      x.ctot, x.coff, 1)
        self.conv_s8(y8, conv2, bn2, d2, out_f32=out.t, f32_layout=ops.S8_F32_NCHW)
        return out

    def bottleneck(self, blk, x: View, s8_only=False, nxt=None) -> View:
        """One Bottleneck (model/HRNet.py:551-571).  ``s8_only``: the result is wanted as S8 records (transition1's convs read
        them) - conv3 writes them straight from its accumulators (csrc/pointx.hip) and the NCHW tensor of the returned view is
        filled, by a conversion pass, only if some consumer asks for it.  ``nxt``: the Bottleneck that follows - its conv1 rides
        on this block's conv3 launch (:meth:`pointx_pair`)."""
        res = x
        if blk.downsample is not None:
            # the 1x1 shortcut only needs x: a side stream next to conv1 / conv2
            self.fork((1,))
            self.on_stream(1)
            res = self.conv_bn(x, blk.downsample[0], blk.downsample[1])
            self.on_stream(0)
        y = self.conv1_conv2_s8(x, blk.conv1, blk.bn1, blk.conv2, blk.bn2)
        if y is None:
            y = self.conv_bn(x, blk.conv1, blk.bn1, ACT_RELU)
            y = self.conv_bn(y, blk.conv2, blk.bn2, ACT_RELU)
        if blk.downsample is not None:
            self.join((1,))
        n, _, h, w = y.t.shape
        c3 = blk.conv3
        co = c3.out_channels
        if (s8_only and self.s8_here and self.routes.use_pointx and plain_conv(c3, 1, cin=y.C, cout=res.C)
                and ops.pointwise_x3_s8_supported(c3.in_channels, co, h * w)):
            for v_ in (y, res):
                self._needs_nchw(v_)
            sc, sh = self._bn_fold(blk.bn3)
            pk = ops.pack_pointwise_x3_s8(self.dev_param(c3.weight), sc, sh)
            out = View(self.new(n, co, h, w))
            o8 = self.new(n * co * h * w)
            aux = self._aux[id(out.t)] = Aux(o8)
            self._keep.append(pk)
            self.call_lazy_nchw(aux, self.lib.otp_pointwise_x3_s8_res, "otp_pointwise_x3_s8_res",
                                lambda nchw: ops.pointwise_x3_s8_res_args(y, pk, co, o8, res, True),
                                unpack=(hip.ptr(o8), hip.ptr(out.t), n, co, h, w))
            return out
        if nxt is not None and plain_conv(c3, 1):
            sc, sh = self._bn_fold(blk.bn3)
            out = self.pointx_pair(y, c3.weight, sc, sh, res, nxt)
            if out is not None:
                return out
        return self.conv_bn(y, blk.conv3, blk.bn3, ACT_RELU, res=res)

    def hr_module(self, mod, xs: List[View], fork_in=True, join_out=True) -> List[View]:
        """One HighResolutionModule (model/HRNet.py:478-496).  ``fork_in`` / ``join_out`` = False chain consecutive modules of
        a stage stream by stream: branch i of the next module only reads row i of this module's fuse layer, which ran on stream
        i, so neither the join behind the rows nor the fork in front of the next branches is needed - a branch starts as soon
        as ITS row is done instead of when the slowest row is."""
        n = mod.num_branches
        xs = list(xs)
        r = self.routes
        if fork_in:
            self.fork(range(1, n))
        for i in range(n):
            self.on_stream(i)                                     # branch i is independent of the others until the fuse
            # branch i feeds the stride-2 chains of the fuse rows below it
            y = self.branch_s8(list(mod.branches[i]), xs[i], want_s8=i < len(mod.fuse_layers) - 1 and self.s2_here)
            if y is not None:
                xs[i] = y
                continue
            for blk in mod.branches[i]:
                xs[i] = self.basic_block(blk, xs[i])
        self.on_stream(0)
        self.join(range(1, n))
        if n == 1:
            return xs
        outs = []
        if self.s2_here:
            for j in range(min(n, len(mod.fuse_layers) - 1)):     # S8 images the rows below read, made before the rows fork
                self.s8_image(xs[j])
        self.fork(range(1, len(mod.fuse_layers)))
        for i in range(len(mod.fuse_layers)):
            self.on_stream(i)                                     # fuse row i reads every branch, writes only y_i
            # y_i = sum_j f_ij(x_j), then ReLU (HRNet.py:487-494).  The identity term rides on the first
            # emitted conv as its residual; later terms accumulate in place; the last one applies the ReLU.
            terms = [j for j in range(n) if j != i]
            y = None
            # two or three upsampled terms (the j > i tail of the row): their convs run at low resolution and ONE streaming pass
            # adds them all to the high-resolution tensor (same summation order as chaining them)
            ups = [j for j in terms if j > i]
            hi_w = xs[i].t.shape[3]
            if r.fuse_upsample and len(ups) >= 2 and hi_w % 4 == 0:
                terms = [j for j in terms if j < i]
            else:
                ups = []
            for idx, j in enumerate(terms):
                last = idx == len(terms) - 1 and not ups
                act = ACT_RELU if last else ACT_NONE
                res = xs[i] if y is None else y
                fl = mod.fuse_layers[i][j]
                tgt = y if y is not None else View(self.new(*xs[i].t.shape))
                if j > i:
                    f = 2 ** (j - i)
                    if f >= 2 and ((xs[j].t.shape[3] * f) % 4 == 0 or r.up_any_width):
                        # (any width: otp_upsample_add has a one-element form - rows of 18 at 384x288 used to send the 384 -> 192
                        #  term of stage 4's row 2 to the generic conv kernel's upsample epilogue, 195 us on the row's critical path)
                        # the upsampled tensor is f*f x the conv result: conv at low resolution, then one streaming
                        # accumulate kernel (measured faster than the conv kernel's element-wise upsample epilogue)
                        low = self.conv_bn(xs[j], fl[0], fl[1], ACT_NONE)
                        if act == ACT_RELU and low.coff == 0 and low.C == low.ctot and self.fuse_s8([low], [f], res, tgt):
                            y = tgt
                            continue
                        self._needs_nchw(res)
                        self.call(self.lib.otp_upsample_add, "otp_upsample_add", *ops.upsample_add_args(low, res, tgt, f, act == ACT_RELU))
                        y = tgt
                    else:
                        y = self.conv_bn(xs[j], fl[0], fl[1], act, res=res, out=tgt, res_up=f)
                else:
                    chain = [(fl[k][0], fl[k][1], k < len(fl) - 1) for k in range(len(fl))]
                    if self.s2_chain_s8(chain, xs[j], act, res=res, out=tgt) is not None:
                        y = tgt
                        continue
                    t = xs[j]
                    for k in range(len(fl) - 1):
                        t = self.conv_bn(t, fl[k][0], fl[k][1], ACT_RELU)
                    y = self.conv_bn(t, fl[-1][0], fl[-1][1], act, res=res, out=tgt)
            if ups:
                res = xs[i] if y is None else y
                tgt = y if y is not None else View(self.new(*xs[i].t.shape))
                lows = [self.conv_bn(xs[j], mod.fuse_layers[i][j][0], mod.fuse_layers[i][j][1], ACT_NONE) for j in ups]
                factors = [2 ** (j - i) for j in ups]
                if self.fuse_s8(lows, factors, res, tgt):
                    outs.append(tgt)
                    continue
                self._needs_nchw(res)
                args, arrays = ops.upsample_add_multi_args(lows, factors, res, tgt, relu=True)
                self._keep += arrays
                self.call(self.lib.otp_upsample_add_multi, "otp_upsample_add_multi", *args)
                y = tgt
            outs.append(y)
        self.on_stream(0)
        if join_out:
            self.join(range(1, len(mod.fuse_layers)))
        return outs

    def hr_stages(self, net, x, width_change, new_branch, module, before_fork=None):
        """Transitions and stages 2 - 4 of an HRNet (model/HRNet.py:131-152), the walk both engines share: the convs of a
        transition only share their inputs and run on a stream each; consecutive modules of a stage are chained stream by
        stream (see :meth:`hr_module`).  The engine's emitters: ``width_change(s, x, tr)`` and ``new_branch(s, x, tr)`` for the
        two kinds of transition layer (:213-229), ``module(s, mi, n_mods, mod, xs, fork_in, join_out)`` for module ``mi`` of
        the ``n_mods`` of stage ``s``, ``before_fork(s, xs)`` ahead of a transition's fork."""
        ys = [x]
        for s in (2, 3, 4):
            trans = getattr(net, f"transition{s - 1}")
            live = [i for i, tr in enumerate(trans) if tr is not None]
            if before_fork is not None:
                before_fork(s, ys)
            self.fork(range(1, len(live)))                         # the transition convs only share their inputs
            xs = []
            for i, tr in enumerate(trans):
                if tr is None:
                    xs.append(ys[i])
                    continue
                self.on_stream(live.index(i))
                if isinstance(tr[0], torch.nn.Conv2d):            # same-resolution width change (:213-220)
                    xs.append(width_change(s, ys[i], tr))
                else:                                              # new branch from the last tensor (:221-229)
                    xs.append(new_branch(s, ys[-1], tr))
            self.on_stream(0)
            self.join(range(1, len(live)))
            ys = xs
            mods = list(getattr(net, f"stage{s}"))
            cont = False
            for mi, mod in enumerate(mods):
                # the next module's branch i continues on the stream of this module's row i (same count of rows and branches)
                fork_in, nxt = not cont, (mods[mi + 1] if mi + 1 < len(mods) else None)
                cont = (self.routes.chain_modules and nxt is not None and len(mod.fuse_layers) == nxt.num_branches
                        and mod.num_branches > 1)
                ys = module(s, mi, len(mods), mod, ys, fork_in, not cont)
        return ys

    def hrnet(self, net, x_in: View) -> View:
        c1 = net.conv1
        r = self.routes
        n_in, c_in, h_in, w_in = x_in.t.shape
        if (r.use_x3 and r.stem_x3 and x_in.coff == 0 and x_in.C == c_in and c_in == 3 * self.F and plain_conv(c1, 3, stride=2, cin=3)
                and ops.stem_conv_x3_supported(n_in, self.F, h_in, w_in, c1.out_channels)):
            # conv1 + bn1 + relu on the frames of the clip (HRNet.py:118-120 after OTPose.py:317): one k-step of split products per
            # 16 pixels x 16 channels, gathered straight from the image (csrc/stem.hip), stored through an LDS slab as 256-byte runs
            # per channel: 202 against 426 us for the direct kernel (tools/stem_time.py), forward -0.3 ... -0.5 ms
            sc, sh = self._bn_fold(net.bn1)
            pk = ops.pack_stem_conv_x3(self.dev_param(c1.weight), sc, sh)
            self._keep.append(pk)
            x = View(self.new(self.F * n_in, c1.out_channels, (h_in - 1) // 2 + 1, (w_in - 1) // 2 + 1))
            self.call(self.lib.otp_stem_conv_x3, "otp_stem_conv_x3", *ops.stem_conv_x3_args(x_in.t, pk, x.t, self.F, c1.out_channels))
        else:
            x = self.conv_bn(x_in, net.conv1, net.bn1, ACT_RELU, frame_split=self.B, cin=3)
        blocks = list(net.layer1)
        b0 = blocks[0]
        if (r.fuse_shortcut and b0.downsample is not None and plain_conv(b0.conv3, 1) and plain_conv(b0.downsample[0], 1)):
            # first Bottleneck (HRNet.py:551-571 with the 1x1 shortcut of :240-247): relu(bn3(conv3(y)) + bn_d(conv_d(x))) is
            # one 1x1 conv over the channel concatenation [x, y] with both BatchNorm scales folded into the weights - the
            # 256-channel shortcut tensor (566 MB at cfg2) is neither written nor read back.  x (stem conv2) and y
            # (Bottleneck conv2) are written straight into the two channel slices of one buffer.
            n, _, h, w = x.t.shape
            c2 = net.conv2
            ho = (h + 2 * c2.padding[0] - c2.kernel_size[0]) // c2.stride[0] + 1
            wo = (w + 2 * c2.padding[0] - c2.kernel_size[0]) // c2.stride[0] + 1
            cx, cy = c2.out_channels, b0.conv2.out_channels
            cat = self.new(n, cx + cy, ho, wo)
            xin = self.conv_bn(x, c2, net.bn2, ACT_RELU, out=View(cat, 0, cx))
            if self.conv1_conv2_s8(xin, b0.conv1, b0.bn1, b0.conv2, b0.bn2, out=View(cat, cx, cy)) is None:
                y = self.conv_bn(xin, b0.conv1, b0.bn1, ACT_RELU)
                self.conv_bn(y, b0.conv2, b0.bn2, ACT_RELU, out=View(cat, cx, cy))

            def fold(conv, bn):
                sc, sh = self._bn_fold(bn)
                return self.dev_param(conv.weight) * sc[:, None, None, None], sh
            wd, shd = fold(b0.downsample[0], b0.downsample[1])
            w3, sh3 = fold(b0.conv3, b0.bn3)
            cout = b0.conv3.out_channels
            wcat, ones, shcat = torch.cat([wd, w3], 1), torch.ones(cout, device=self.dev), shd + sh3
            x = self.pointx_pair(View(cat), wcat, ones, shcat, None, blocks[1]) if len(blocks) > 1 else None
            if x is None:
                x = self.conv(View(cat), wcat, View(self.new(n, cout, ho, wo)), scale=ones, shift=shcat, act=ACT_RELU)
            blocks = blocks[1:]
        else:
            x = self.conv_bn(x, net.conv2, net.bn2, ACT_RELU)
        for bi, blk in enumerate(blocks):
            # (the last Bottleneck's result as S8 records only: transition1's convs read them)
            x = self.bottleneck(blk, x, s8_only=self.s2_here and r.t1_s8 and bi == len(blocks) - 1,
                                nxt=blocks[bi + 1] if bi + 1 < len(blocks) else None)

        def t1_s8(s):
            return s == 2 and self.s8_here and r.t1_s8

        def before_fork(s, ys):
            if (s >= 3 or t1_s8(s)) and self.s2_here:
                # the lowest-resolution tensor feeds the new branch's stride-2 conv AND its own branch of the next module (s >= 3) /
                # the width-change conv of transition1 (s = 2: 256 -> 48 and 256 -> 96 stride 2 ran at 100-160 TFLOP/s on the
                # fp32-input kernel): one pack pass before the streams fork serves both
                self.s8_image(ys[-1], want_c4=s >= 3 and not r.s8_residual)

        def width_change(s, x, tr):
            y = self.conv_bn_s8(x, tr[0], tr[1], ACT_RELU) if t1_s8(s) else None
            return y if y is not None else self.conv_bn(x, tr[0], tr[1], ACT_RELU)

        def new_branch(s, z, tr):
            zs = self.s2_chain_s8([(step[0], step[1], True) for step in tr], z, ACT_RELU) if (s >= 3 or t1_s8(s)) else None
            if zs is not None:
                return zs
            for step in tr:
                z = self.conv_bn(z, step[0], step[1], ACT_RELU)
            return z

        def module(s, mi, n_mods, mod, xs, fork_in, join_out):
            self._exact = s == 4 and mi >= n_mods - r.f32_tail          # the exact-fp32 tail (Routes.f32_tail)
            return self.hr_module(mod, xs, fork_in, join_out)
        ys = self.hr_stages(net, x, width_change, new_branch, module, before_fork)
        fl = net.final_layer
        rough = View(self.new(self.F * self.B, self.J, self.h, self.w))
        self._exact = r.f32_tail > 0
        out = self.conv(ys[0], fl.weight, rough, 1, fl.padding[0], 1, bias=fl.bias)
        self._exact = False
        return out

    # ---- ConvTransformer (reference model/ConvVideoTransformer.py:123-184, model/blocks.py:264-280,400-453) ----
    def v3(self, t3):
        """(B, C, T) tensor as a 4-D view for the conv kernel."""
        b, c, t = t3.shape
        return View(t3.view(b, c, 1, t))

    def tblock(self, blk, x, stride):
        B, C, T = x.shape
        To = T if stride == 1 else (T + 2 - 3) // 2 + 1
        L = self.lib
        a = blk.attn
        r = self.routes
        if r.use_flow_fused and stride == 1 and ops.flow_block_supported(blk, C, T):
            # the C = 17 flow encoder: per-token chains in two launches around the attention (csrc/flowenc.hip); the generic
            # kernels below are latency bound at this width (12 launches per block on the serial path)
            fp, bp = ops.pack_flow_front(blk, self.dev), ops.pack_flow_back(blk, self.dev)
            self._keep += [fp, bp]
            q, k, v, att, out = (self.new(B, C, T) for _ in range(5))
            self.call(L.otp_flow_front, "otp_flow_front", *ops.flow_front_args(x, fp, q, k, v, blk.ln1.eps))
            self.attention(q, k, v, att, a)
            self.call(L.otp_flow_back, "otp_flow_back", *ops.flow_back_args(x, att, bp, out, blk.mlp[0].out_channels, blk.ln2.eps))
            return out
        ln1 = self.new(B, C, T)
        skip = self.new(B, C, To) if stride > 1 else None
        p = self.dev_param
        self.call(L.otp_ln_channel, "otp_ln_channel", hip.ptr(x), hip.ptr(p(blk.ln1.weight)), hip.ptr(p(blk.ln1.bias)),
                  hip.ptr(ln1), hip.ptr(skip), B, C, T, blk.ln1.eps)
        q, k, v = self.new(B, C, To), self.new(B, C, To), self.new(B, C, To)
        # (the split-product kernels of csrc/densex.hip also hold C = 204, the 7-frame window of BASELINE configs[4]; the exact-fp32
        #  ones of csrc/dense.hip only C = 136 - until round 4 this line asked the fp32 predicate first and cfg5 ran its
        #  projections and the q / k / v front end on the generic kernels: 23 ms of kernel time per forward)
        dx3 = r.use_dense_cc and r.use_x3 and ops.dense_x3_supported(C, To)
        dense = dx3 or (r.use_dense_cc and ops.dense_cc_supported(C, To))
        if dense:
            packs = [ops.pack_dense_cc(m.weight.to(self.dev), None, m.bias.to(self.dev), x3=dx3)
                     for m in (a.query, a.key, a.value)]
        if dense and stride == 1 and r.use_qkv_front:
            # depthwise convs + LayerNorms + the three projections in one launch (csrc/dense.hip, qkv_front_kernel)
            table = ops.pack_qkv_table(*[p(t) for t in (a.query_conv.weight, a.key_conv.weight, a.value_conv.weight,
                                                         a.query_norm.weight, a.query_norm.bias, a.key_norm.weight,
                                                         a.key_norm.bias, a.value_norm.weight, a.value_norm.bias)])
            self._keep += [table, *packs]
            self.call((L.otp_qkv_front_h1 if self.half_products else L.otp_qkv_front_x3) if dx3 else L.otp_qkv_front, "otp_qkv_front",
                      *ops.qkv_front_args(ln1, table, packs, (q, k, v), a.query_norm.eps))
        else:
            qn, kn, vn = self.new(B, C, To), self.new(B, C, To), self.new(B, C, To)
            self.call(L.otp_dwconv_ln3, "otp_dwconv_ln3", hip.ptr(ln1), hip.ptr(p(a.query_conv.weight)),
                      hip.ptr(p(a.key_conv.weight)), hip.ptr(p(a.value_conv.weight)),
                      hip.ptr(p(a.query_norm.weight)), hip.ptr(p(a.query_norm.bias)),
                      hip.ptr(p(a.key_norm.weight)), hip.ptr(p(a.key_norm.bias)),
                      hip.ptr(p(a.value_norm.weight)), hip.ptr(p(a.value_norm.bias)),
                      hip.ptr(qn), hip.ptr(kn), hip.ptr(vn), B, C, T, stride, a.query_norm.eps)
            if dense:
                # the three projections as one launch of the register-resident-input kernel (csrc/dense.hip)
                self.dense((qn, kn, vn), packs, None, (q, k, v), B, C, To)
            else:
                self.conv(self.v3(qn), a.query.weight, self.v3(q), bias=a.query.bias)
                self.conv(self.v3(kn), a.key.weight, self.v3(k), bias=a.key.bias)
                self.conv(self.v3(vn), a.value.weight, self.v3(v), bias=a.value.bias)
        att = self.new(B, C, To)
        self.attention(q, k, v, att, a)
        # y = pool_skip(x) + scale_attn * (proj(att) + b)   (eval: dropout / drop-path are identities)
        sa = blk.drop_path_attn.scale.detach().reshape(-1)
        y = self.new(B, C, To)
        if dense:
            sad = sa.to(self.dev, torch.float32)
            pk = ops.pack_dense_cc(a.proj.weight.to(self.dev), sad, a.proj.bias.detach().to(self.dev) * sad,
                                   x3=r.use_x3 and ops.dense_x3_supported(C, To))
            self.dense((att,), [pk], (skip if stride > 1 else x,), (y,), B, C, To)
        else:
            self.conv(self.v3(att), a.proj.weight, self.v3(y), scale=sa,
                      shift=a.proj.bias.detach() * sa.to(a.proj.bias.device), res=self.v3(skip if stride > 1 else x))
        sm = blk.drop_path_mlp.scale.detach().reshape(-1)
        out = self.new(B, C, To)
        hid = blk.mlp[0].out_channels
        # ln2 -> Conv1d -> GELU -> Conv1d + residual as one launch, hidden activation kept on chip: with split-half products on
        # the 16-bit matrix cores (csrc/mlpx.hip), else in exact fp32 (csrc/mlp.hip)
        mlp_x3 = r.use_fused_mlp and r.use_x3 and ops.mlp_x3_supported(C, hid, To)
        if mlp_x3 or (r.use_fused_mlp and ops.mlp_fused_supported(C, hid, To)):
            dev = lambda t: t.detach().to(self.dev, torch.float32)     # noqa: E731
            w1, b1, w2 = dev(blk.mlp[0].weight), dev(blk.mlp[0].bias), dev(blk.mlp[3].weight)
            packed = ops.pack_mlp_x3_weights(w1, b1, w2, half=self.half_products) if mlp_x3 else ops.pack_mlp_weights(w1, b1, w2)
            scd = dev(sm).contiguous()
            shd = (dev(blk.mlp[3].bias) * scd).contiguous()
            self._keep += [packed, scd, shd]
            fn, name = ((L.otp_ln_mlp_h1 if self.half_products else L.otp_ln_mlp_x3, "otp_ln_mlp_x3") if mlp_x3
                        else (L.otp_ln_mlp_fused, "otp_ln_mlp_fused"))
            self.call(fn, name, *ops.ln_mlp_args(y, p(blk.ln2.weight), p(blk.ln2.bias), blk.ln2.eps, packed, scd, shd, out, hid))
            return out
        ln2 = self.new(B, C, To)
        self.call(L.otp_ln_channel, "otp_ln_channel", hip.ptr(y), hip.ptr(p(blk.ln2.weight)), hip.ptr(p(blk.ln2.bias)),
                  hip.ptr(ln2), None, B, C, To, blk.ln2.eps)
        hdn = self.new(B, 4 * C, To)
        self.conv(self.v3(ln2), blk.mlp[0].weight, self.v3(hdn), bias=blk.mlp[0].bias, act=ACT_GELU)
        self.conv(self.v3(hdn), blk.mlp[3].weight, self.v3(out), scale=sm,
                  shift=blk.mlp[3].bias.detach() * sm.to(blk.mlp[3].bias.device), res=self.v3(y))
        return out

    def attention(self, q, k, v, att, a):
        """The attention product of attention module ``a`` as one launch: the local window of a LocalMaskedMHCA
        (csrc/localattn.hip; ``att`` in the natural layout), else the channel attention.  q, k, v are fp32 in both engines."""
        if getattr(a, "window_size", 0) > 1:
            B, C, T = q.shape
            ops.check_local_attn(C, T, a.n_head, a.window_size)
            rel = ops.rel_pe_table(getattr(a, "rel_pe", None), a.n_head, a.window_size, q)
            if rel is not None:
                self._keep.append(rel)
            self.call(self.lib.otp_local_attn, "otp_local_attn",
                      *ops.local_attn_args(q, k, v, rel, att, None, a.n_head, a.window_size, a.scale))
        else:
            self.chan_attn(q, k, v, att, a)

    def chan_attn(self, q, k, v, att, a):
        """Channel attention of a MaskedMHCA ``a`` (csrc/attn.hip) with its workspace."""
        B, C, T = q.shape
        nbytes = self.lib.otp_chan_attn_workspace(B, C, T, a.n_head)
        ws = self.new(max(nbytes // 4, 1))
        self.call(self.lib.otp_chan_attn, "otp_chan_attn", *ops.chan_attn_args(q, k, v, att, ws, nbytes, a.n_head, a.scale))

    def encoder_pe(self, ct, T):
        """The (C, T) table the glue kernels add into encoder ``ct``'s input: its positional table, or - for an encoder with conv
        embedding layers, which adds the table behind its last layer - one cached all-zero table per shape."""
        if len(ct.embd) == 0:
            return self.dev_param(ct.pos_embd[0, :, :T])
        zeros = getattr(self, "_zero_pe", None)
        if zeros is None:
            zeros = self._zero_pe = {}
        key = (ct.n_in, T)
        if key not in zeros:
            zeros[key] = torch.zeros((ct.n_in, T), dtype=torch.float32, device=self.dev)
        return zeros[key]

    def conv_embd(self, ct, x):
        """The ``arch[0]`` conv embedding layers of ``ct`` (ConvVideoTransformer.py:129-135) on x (B, n_in, T): one otp_conv_embd
        launch per layer on ping-pong buffers, the last one adding the positional table.  No layer: x itself, no launch."""
        n = len(ct.embd)
        if n == 0:
            return x
        B, cin, T = x.shape
        h = int(ct.h)
        if T % h or T > ct.max_len:
            raise ValueError(f"conv embedding: {T} tokens do not form an h = {h} grid of at most max_len = {ct.max_len} tokens")
        C = ct.n_embd
        pe = self.dev_param(ct.pos_embd[0, :, :T])
        bufs = [self.new(B, C, T) for _ in range(min(n, 2))]
        for i, (conv, norm) in enumerate(zip(ct.embd, ct.embd_norm)):
            ln = hasattr(norm, "weight")                       # modules.LayerNorm, or nn.Identity without the norm
            wt = self.dev_param(conv.weight)
            bias, gamma, beta, _ = ops.conv_embd_params((B, cin, h, T // h), wt, conv.bias, norm.weight if ln else None,
                                                        norm.bias if ln else None, None, self.dev)
            packed = ops.pack_conv_embd_weight(wt)
            self._keep += [packed, bias, gamma, beta]
            out = bufs[i % 2]
            self.call(self.lib.otp_conv_embd, "otp_conv_embd",
                      *ops.conv_embd_args(x.view(B, cin, h, T // h), packed, bias, gamma, beta, pe if i == n - 1 else None, out,
                                          None, C, conv.kernel_size[0], norm.eps if ln else 1e-5))
            x, cin = out, C
        return x

    def _ln(self, norm, x):
        B, C, T = x.shape
        y = self.new(B, C, T)
        p = self.dev_param
        self.call(self.lib.otp_ln_channel, "otp_ln_channel", hip.ptr(x), hip.ptr(p(norm.weight)), hip.ptr(p(norm.bias)), hip.ptr(y),
                  None, B, C, T, norm.eps)
        return y

    def token_encoder(self, name, pos_name, x):
        """Extension keys MODEL.TOKEN_LAYERS / FLOW_TOKEN_LAYERS: the model's ``modules.TransformerEncoder`` ``name`` (eval mode)
        on x (B, C, T) as T tokens of width C, when the model has one; else x itself and no launch.  Per layer: three 1x1
        projections, ``otp_token_attn_forward``, the out-projection with the residual in its epilogue, the two channel
        LayerNorms, and the FFN as two 1x1 convolutions with bias + activation / bias + residual epilogues.  ``pos`` goes to
        q and k only; W (x + pos) + b is launched as W x + b + (W pos), the last term a table built once per engine and added
        as the epilogue's residual, so the sum x + pos never costs a pass of its own."""
        enc = getattr(self.model, name, None)
        if enc is None:
            return x
        B, C, T = x.shape
        pos = getattr(self.model, pos_name, None)
        if pos is not None:
            if pos.shape[1] != T:
                raise ValueError(f"{pos_name}: a table of {pos.shape[1]} tokens for {T} tokens")
            pos = pos.detach().to(self.dev, torch.float32)[0].t().contiguous()                   # (C, T)
        for layer in enc.layers:
            a, E = layer.self_attn, layer.d_model
            w, b = a.in_proj_weight.detach(), a.in_proj_bias.detach()
            src = self._ln(layer.norm1, x) if layer.normalize_before else x
            q, k, v, att, y = (self.new(B, C, T) for _ in range(5))
            for out, lo in ((q, 0), (k, E)):
                res = None
                if pos is not None:
                    res = (w[lo:lo + E].to(self.dev, torch.float32) @ pos).unsqueeze(0).expand(B, C, T).contiguous()
                    self._keep.append(res)
                self.conv(self.v3(src), w[lo:lo + E].reshape(E, E, 1, 1), self.v3(out), bias=b[lo:lo + E],
                          res=None if res is None else self.v3(res))
            self.conv(self.v3(x), w[2 * E:].reshape(E, E, 1, 1), self.v3(v), bias=b[2 * E:])
            if getattr(layer, "products", "f32") == "half":
                # MODEL.TOKEN_PRODUCTS = "half": the same launch slot on the 16-bit matrix cores (csrc/tokattn_h.hip); no dropout
                # in eval, and the guard word is the library's sticky one, which :meth:`_finish` / :meth:`run` read
                self._half_tokens = True
                self.call(self.lib.otp_token_attn_forward_h1, "otp_token_attn_forward_h1", hip.ptr(q), hip.ptr(k), hip.ptr(v), None,
                          hip.ptr(att), None, B, C, layer.nhead, T, 1.0 / math.sqrt(E // layer.nhead), 0.0, 0, None)
            else:
                self.call(self.lib.otp_token_attn_forward, "otp_token_attn_forward", hip.ptr(q), hip.ptr(k), hip.ptr(v), None,
                          hip.ptr(att), None, B, C, layer.nhead, T, 1.0 / math.sqrt(E // layer.nhead))
            self.conv(self.v3(att), a.out_proj.weight.reshape(E, E, 1, 1), self.v3(y), bias=a.out_proj.bias, res=self.v3(x))
            act = ACT_GELU if layer.activation == "gelu" else ACT_RELU
            F = layer.linear1.out_features
            hdn, z = self.new(B, F, T), self.new(B, C, T)
            if layer.normalize_before:
                self.conv(self.v3(self._ln(layer.norm2, y)), layer.linear1.weight.reshape(F, E, 1, 1), self.v3(hdn),
                          bias=layer.linear1.bias, act=act)
                self.conv(self.v3(hdn), layer.linear2.weight.reshape(E, F, 1, 1), self.v3(z), bias=layer.linear2.bias, res=self.v3(y))
                x = z
            else:
                y = self._ln(layer.norm1, y)
                self.conv(self.v3(y), layer.linear1.weight.reshape(F, E, 1, 1), self.v3(hdn), bias=layer.linear1.bias, act=act)
                self.conv(self.v3(hdn), layer.linear2.weight.reshape(E, F, 1, 1), self.v3(z), bias=layer.linear2.bias, res=self.v3(y))
                x = self._ln(layer.norm2, z)
            if enc.pe_only_at_begin:
                pos = None
        return x if enc.norm is None else self._ln(enc.norm, x)

    def conv_transformer(self, ct, x, stacked):
        """x (B, C, T) already holds input + positional table (:meth:`encoder_pe`; the bare input for an encoder with conv
        embedding layers, whose last launch adds the table); writes levels into stacked (B, L*C, T)."""
        x = self.conv_embd(ct, x)
        _, C, T = x.shape
        L = self.lib
        for blk in ct.stem:
            x = self.tblock(blk, x, 1)
        self.call(L.otp_upsample_linear, "otp_upsample_linear", *ops.upsample_linear_args(x, stacked, 1, 0))
        for i, blk in enumerate(ct.branch):
            x = self.tblock(blk, x, 2)
            f = 2 ** (i + 1)
            if x.shape[2] * f != T:
                raise RuntimeError("heat-map size must make every pyramid level divide evenly (T % 4 == 0)")
            self.call(L.otp_upsample_linear, "otp_upsample_linear", *ops.upsample_linear_args(x, stacked, f, (i + 1) * C))

    # ---- RSB heads (reference model/RSB.py:77-103) --------------------------------------------------
    def rsb_block(self, blk, x: View) -> View:
        n, _, h, w = x.t.shape
        bc = blk.branch_ch
        cbr = lambda m, inp, out, act, in2=None, res=None: self.conv(   # noqa: E731
            inp, m.conv.weight, out, 1, m.conv.padding[0], 1, bn=m.bn, bias=m.conv.bias, act=act, in2=in2, res=res)
        t = self.new(n, 4 * bc, h, w)
        cat = self.new(n, 4 * bc, h, w)
        cbr(blk.conv_bn_relu1, x, View(t), ACT_RELU)
        s = [View(t, i * bc, bc) for i in range(4)]
        tmp = lambda: View(self.new(n, bc, h, w))                       # noqa: E731
        # the staircase of RSB.py:80-92 is a DAG of depth 7, not a chain of 10: on the main stream the three convs off the
        # critical path (2_2, 3_2, 3_3) run on a side stream (these launches are tiny and latency-bound)
        par = self.multi_stream and self._sid == 0
        side = (lambda: (self.fork((1,)), self.on_stream(1))) if par else (lambda: None)      # noqa: E731
        main = (lambda: self.on_stream(0)) if par else (lambda: None)                          # noqa: E731
        o11 = cbr(blk.conv_bn_relu2_1_1, s[0], View(cat, 0, bc), ACT_RELU)
        o21 = cbr(blk.conv_bn_relu2_2_1, s[1], tmp(), ACT_RELU, in2=o11)
        side()
        o22 = cbr(blk.conv_bn_relu2_2_2, o21, View(cat, bc, bc), ACT_RELU)
        main()
        o31 = cbr(blk.conv_bn_relu2_3_1, s[2], tmp(), ACT_RELU, in2=o21)
        side()
        o32 = cbr(blk.conv_bn_relu2_3_2, o31, tmp(), ACT_RELU, in2=o22)
        main()
        o41 = cbr(blk.conv_bn_relu2_4_1, s[3], tmp(), ACT_RELU, in2=o31)
        if par:
            self.join((1,))
        o42 = cbr(blk.conv_bn_relu2_4_2, o41, tmp(), ACT_RELU, in2=o32)
        if par:
            self.on_stream(1)
        o33 = cbr(blk.conv_bn_relu2_3_3, o32, View(cat, 2 * bc, bc), ACT_RELU)
        if par:
            self.on_stream(0)
            self.join((1,))
        o43 = cbr(blk.conv_bn_relu2_4_3, o42, tmp(), ACT_RELU, in2=o33)
        cbr(blk.conv_bn_relu2_4_4, o43, View(cat, 3 * bc, bc), ACT_RELU)
        res = x
        if blk.downsample is not None:
            res = cbr(blk.downsample, x, View(self.new(n, blk.conv_bn_relu3.conv.out_channels, h, w)), ACT_NONE)
        out = View(self.new(n, blk.conv_bn_relu3.conv.out_channels, h, w))
        return cbr(blk.conv_bn_relu3, View(cat), out, ACT_RELU, res=res)

    def rsb_chain(self, chain, x: View) -> View:
        for blk in chain.layers:
            x = self.rsb_block(blk, x)
        return x

    # ---- RSN attention / weight vector (reference model/RSB.py:142-203, csrc/prm.hip) -----------------
    def _prm_front(self, layer, x: View) -> View:
        """The leading 3x3 conv-BN-ReLU through :meth:`conv`, the route of the RSB convs."""
        n, _, h, w = x.t.shape
        ops.check_prm(layer.conv.out_channels, h, w)
        f = View(self.new(n, layer.conv.out_channels, h, w))
        return self.conv(x, layer.conv.weight, f, 1, 1, 1, bn=layer.bn, bias=layer.conv.bias, act=ACT_RELU)

    def _prm_layer(self, layer, taps):
        folded = ops.prm_layer(layer, taps, self.dev)
        self._keep += list(folded)
        return folded

    def _prm_gate(self, f: View, l1, l2, residual):
        gate = self.new(f.t.shape[0], f.C, 1, 1)
        self.call(self.lib.otp_prm_gate, "otp_prm_gate",
                  *ops.prm_gate_args(f.t, self._prm_layer(l1, f.C), self._prm_layer(l2, f.C), gate, residual))
        return gate

    def rsn_attention(self, m, x: View) -> View:
        """``modules.RSN_ATTENTION`` on the stream being emitted on: the 3x3 conv, otp_prm_gate, otp_prm_apply."""
        f = self._prm_front(m.conv_bn_relu_prm_1, x)
        gate = self._prm_gate(f, m.conv_bn_relu_prm_2_1, m.conv_bn_relu_prm_2_2, False)
        out = View(self.new(*f.t.shape))
        self.call(self.lib.otp_prm_apply, "otp_prm_apply",
                  *ops.prm_apply_args(f.t, gate, self._prm_layer(m.conv_bn_relu_prm_3_1, f.C),
                                      self._prm_layer(m.conv_bn_relu_prm_3_2, 81), out.t))
        return out

    def rsn_weight_vector(self, m, x: View):
        """``modules.RSN_WEIGHT_VECTOR`` -> the (N, C, 1, 1) gate tensor."""
        f = self._prm_front(m.conv_bn_relu_1, x)
        return self._prm_gate(f, m.conv_bn_relu_2, m.conv_bn_relu_3, True)

    def _prm_after(self, name, x: View) -> View:
        """Extension key MODEL.PRM: the chain's output through the model's ``<name>_prm`` module when it has one."""
        m = getattr(self.model, name, None)
        return x if m is None else self.rsn_attention(m, x)

    # ---- whole forward ------------------------------------------------------------------------------
    def _build(self):
        m, B, J, h, w = self.model, self.B, self.J, self.h, self.w
        L, T = self.lib, self.h * self.w
        self.inp = self._given[0] if self._given[0] is not None else self.new(B, 3 * self.F, self.H_img, self.W_img)
        self.margin = self._given[1] if self._given[1] is not None else self.new(B, self.F - 1)
        assert tuple(self.inp.shape) == (B, 3 * self.F, self.H_img, self.W_img) and self.inp.is_contiguous()
        rough = self.hrnet(m.rough_pose_estimation_net, View(self.inp)).t
        self.hr_end = len(self.ops)               # launches [0, hr_end) = the backbone, the rest = everything behind it

        total, squeezed, inter = self.new(B, J, h, w), self.new(B, J, h, w), self.new(B, J, h, w)
        flow_in = self.new(B, J, T)
        pe_f = self.encoder_pe(m.flow_encoder, T)
        self.call(L.otp_glue_total_n, "otp_glue_total", hip.ptr(rough), hip.ptr(total), hip.ptr(squeezed), hip.ptr(inter),
                  hip.ptr(flow_in), hip.ptr(pe_f), B, J, T, self.F)
        ctx = self.new(B, J, T)
        # def_fuse only needs `total`: it runs on a side stream next to the flow encoder and the temporal encoders
        self.fork((2,))
        self.on_stream(2)
        def_h = self._prm_after("def_fuse_prm", self.rsb_chain(m.def_fuse, View(total)))
        self.on_stream(0)
        self.conv_transformer(m.flow_encoder, self.token_encoder("flow_token_encoder", "flow_pos_embedding", flow_in), ctx)
        D = m.num_frames * J                      # stacked maps per joint: 8 (5-frame window) or 12 (7 frames)
        x1, x2, prev_b = self.new(B, D, T), self.new(B, D, T), self.new(B, J, h, w)
        pe1 = self.encoder_pe(m.temporal_encoder1, T)
        pe2 = self.encoder_pe(m.temporal_encoder2, T)
        self.call(L.otp_glue_stack_n, "otp_glue_stack", hip.ptr(rough), hip.ptr(self.margin), hip.ptr(squeezed),
                  hip.ptr(inter), hip.ptr(ctx), hip.ptr(pe1), hip.ptr(pe2), hip.ptr(x1), hip.ptr(x2), hip.ptr(prev_b),
                  B, J, T, self.F)
        levels = m.scale_arch[-1] + 1
        # the stacked pyramid levels (3 x 136 = 408 channels) feed the final 1x1 layers; padded with zero channels to a multiple
        # of 32 so that those run on the split-product pointwise kernel (432 workgroups, ~45 us) instead of the generic
        # direct kernel (408 -> 17 is one 240-workgroup launch of 13 dependent chunks there: 129 us on the critical path)
        cs_ = levels * D
        cpad = (-cs_) % 32 if (self.use_x3 and m.final_layer1.kernel_size == (1, 1)) else 0
        s1, s2 = self.new(B, cs_ + cpad, T), self.new(B, cs_ + cpad, T)
        if cpad:
            s1[:, cs_:].zero_()
            s2[:, cs_:].zero_()
        # the two temporal encoders are independent: two streams.  Each is followed on its own stream by its final 1x1 layer,
        # which writes straight into the channel-concatenated tensor (OTPose.py:372-378); def_heatmaps feeds the DCN as a
        # dense (B, J, h, w) tensor and the concat as a channel slice: copied once, on def_fuse's stream
        cat3 = self.new(B, 3 * J, h, w)
        def final(fl, s, i):
            wt = fl.weight
            if cpad:
                wt = torch.cat([wt.detach().to(self.dev, torch.float32),
                                torch.zeros(wt.shape[0], cpad, 1, 1, device=self.dev)], 1)
            self.conv(View(s.view(B, cs_ + cpad, h, w)), wt, View(cat3, i * J, J), 1, fl.padding[0], 1, bias=fl.bias)

        self.on_stream(2)
        self.copy_into(def_h, View(cat3, 2 * J, J))
        self.on_stream(0)
        self.fork((1,))
        self.conv_transformer(m.temporal_encoder1, self.token_encoder("token_encoder1", "temporal_pos_embedding", x1), s1)
        final(m.final_layer1, s1, 0)
        self.on_stream(0 if self.routes.te_serial else 1)
        self.conv_transformer(m.temporal_encoder2, self.token_encoder("token_encoder2", "temporal_pos_embedding", x2), s2)
        final(m.final_layer2, s2, 1)
        self.on_stream(0)
        self.join((1, 2))
        trans = self.rsb_chain(m.offset_mask_combine_conv, View(cat3))
        trans = self._prm_after("offset_mask_combine_prm", trans)
        out = self.new(B, J, h, w)
        nd = len(m.deformable_conv_dilations)
        dils = [int(d) for d in m.deformable_conv_dilations]
        cin_t = trans.C
        if (self.use_dcn_fused and trans.coff == 0 and trans.C == trans.ctot and ops.dcn_fused_supported(cin_t, J, h, w, nd)
                and all(plain_conv(c[0], 3, dil=d, groups=None) for cs in (m.offsets_list, m.masks_list) for c, d in zip(cs, dils))
                and all(tuple(mm.deform_conv.weight.shape) == (J, J, 3, 3) and mm.deform_conv.deformable_groups == J
                        and mm.deform_conv.groups == 1 and _pair(mm.deform_conv.stride) == (1, 1)
                        and _pair(mm.deform_conv.padding) == (d, d) == _pair(mm.deform_conv.dilation)
                        for mm, d in zip(m.modulated_deform_conv_list, dils))):
            # the ten offset / mask convs and the five DCN gathers as ONE launch; the 459
            # offset / mask channels per pixel and dilation never reach HBM (csrc/dcn_fused.hip)
            dcs = [mm.deform_conv for mm in m.modulated_deform_conv_list]
            packed = ops.pack_dcn_fused([self.dev_param(c[0].weight) for c in m.offsets_list],
                                        [self.dev_param(c[0].weight) for c in m.masks_list],
                                        [self.dev_param(dc.weight) for dc in dcs],
                                        [None if dc.bias is None else self.dev_param(dc.bias) for dc in dcs])
            # the split NHWC copy of trans (128 bytes per pixel) + the zero-bordered copy of the heat-map planes
            ws = self.new(int(L.otp_dcn_fused_workspace(B, h, w)) // 4)
            dl = (ctypes.c_int * nd)(*dils)
            self._keep += [packed, dl]
            self.call(L.otp_dcn_fused_forward, "otp_dcn_fused_forward", hip.ptr(trans.t), hip.ptr(def_h.t), hip.ptr(packed),
                      hip.ptr(out), hip.ptr(ws), ws.numel() * 4, B, cin_t, J, h, w, dl, nd, 1.0 / nd)
            self._finish(out, rough, inter, prev_b, ctx, squeezed, total)
            return
        off_buf, msk_buf = self.new(B, J * 18, h, w), self.new(B, J * 9, h, w)
        for i, d in enumerate(m.deformable_conv_dilations):
            self.conv(trans, m.offsets_list[i][0].weight, View(off_buf), 1, d, d)
            self.conv(trans, m.masks_list[i][0].weight, View(msk_buf), 1, d, d)
            dc = m.modulated_deform_conv_list[i].deform_conv
            wt, bs = self.dev_param(dc.weight), self.dev_param(dc.bias)
            self.call(L.otp_mdcn_forward, "otp_mdcn_forward", hip.ptr(def_h.t), hip.ptr(off_buf), hip.ptr(msk_buf),
                      hip.ptr(wt), hip.ptr(bs), hip.ptr(out), B, J, h, w, J, 3, 3, 1, d, d, 1, J,
                      1.0 / nd, 0.0 if i == 0 else 1.0, 0)
        self._finish(out, rough, inter, prev_b, ctx, squeezed, total)

    def _finish(self, out, rough, inter, prev_b, ctx, squeezed, total):
        """Last launch of the forward: the range guard's device side (csrc/range.hip) - if any 16-bit-operand kernel of this
        process saw a value beyond a half's range, the heat-maps leave as NaN instead of as finite numbers computed from an
        overflowed operand (the host side raises: :meth:`run`, :meth:`check_range`)."""
        B, J, h, w = self.B, self.J, self.h, self.w
        if self.use_x3 or self.h16 or getattr(self, "_half_tokens", False):
            self.call(self.lib.otp_range_poison, "otp_range_poison", hip.ptr(out), out.numel())
        self.outputs = (out, rough, inter, prev_b, ctx.view(B, J, h, w), squeezed, total)
        torch.cuda.synchronize(self.dev)

    _RANGE_KERNELS = {1: "convx (3x3 / 1x1 convolutions from fp32 NCHW)", 2: "convs (BasicBlock convolutions on S8 records)",
                      3: "convs2 (stride-2 convolutions on S8 records)", 4: "pointx (1x1 convolutions)", 5: "stem convolution",
                      6: "S8 conversion / fuse passes", 7: "mlpx (TransformerBlock MLP)", 8: "densex (q / k / v / proj projections)",
                      9: "channel attention", 10: "dcn_fused (warping head)", 11: "fp16 engine kernels",
                      12: "token attention with half products (MODEL.TOKEN_PRODUCTS)"}

    def _raise_range(self, code):
        raise FloatingPointError(
            "otpose_amd: a value left the range of the half-precision operand pieces (|x| >= 65504, or a non-finite sum) in the "
            f"{self._RANGE_KERNELS.get(code, 'kernel family %d' % code)} of an eval forward; the heat-maps of that forward were "
            "NaN-filled on the device.  The reference computes these layers in fp32: rescale the input / check the checkpoint's "
            "BatchNorm statistics, or run the exact-fp32 kernels (OTPOSE_CONV_MATH=f32).")

    def check_range(self):
        """Synchronise and raise FloatingPointError if a forward since the last check overflowed the half-piece arithmetic."""
        torch.cuda.synchronize(self.dev)
        code = self.lib.otp_range_flag_read(1)
        if code:
            self._raise_range(code)

    def __del__(self):
        try:
            if getattr(self, "graph", None) is not None:
                torch.cuda.synchronize(self.dev)
        except Exception:                           # interpreter shutdown
            pass

    def copy_into(self, src: View, dst: View):
        """dst channels <- src (per-sample strided copy through the upsample kernel with f = 1)."""
        assert src.coff == 0 and src.C == src.ctot
        self.call(self.lib.otp_upsample_linear, "otp_upsample_linear", *ops.upsample_linear_args(src.t, dst.t, 1, dst.coff))

    # ---------------------------------------------------------------------------------------------
    def _launch_all(self, first=0, last=None):
        """Enqueue launches [first, last) of the list on the current stream (and the side streams they were emitted on)."""
        main = hip.stream_of(self.inp)
        handles = [main] + [s_.cuda_stream for s_ in self._side]
        for op, sid in self.ops[first:last]:
            self._stream = handles[sid] if sid > 0 else main
            op()
        self._stream = main

    def run(self, x, margin, alias_outputs: bool = False):
        """One forward.  Returns fresh tensors like the reference's ``OTPose.forward`` (7 clones, 85 MB at batch 16:
        ~30 us of device copies next to a 57 ms forward); ``alias_outputs=True`` hands out the engine's static
        buffers instead, which the NEXT ``run`` overwrites (benchmark loops, callers that consume at once)."""
        if not x.is_cuda:
            raise RuntimeError("OTPose.forward expects CUDA (HIP) tensors; there is no CPU path")
        if self.range_check != "off":
            # deferred half of the range guard: a violation recorded by any forward that has completed by now (no synchronisation)
            code = self.lib.otp_range_flag_read(1)
            if code:
                self._raise_range(code)
        if x.dtype == torch.uint8:
            # (B, 5, H, W, 3) uint8 frames: normalise + concatenate straight into the stem conv's input buffer
            ops.frames_to_clip(x, out=self.inp)
        elif x.data_ptr() != self.inp.data_ptr():         # (a caller that fills OTPose.input_buffers() in place skips the copy)
            self.inp.copy_(x)
        if margin.data_ptr() != self.margin.data_ptr():
            self.margin.copy_(margin.to(torch.float32))
        if self.use_graph:
            from . import parallel
            if not parallel.graph_replay_safe():
                # an RCCL communicator of this process was destroyed: replaying a hipGraph after that segfaults inside the
                # runtime (torch 2.10 / ROCm 7.2) - eager launches from here on.  A graph already captured is kept alive,
                # never replayed (tearing it down before eager launches on its streams is the other known crash)
                self.use_graph = False
                self._parked_graph, self.graph = self.graph, None
        if self.use_graph and self.graph is None:
            self._launch_all()                      # warm-up (sets kernel attributes) before capture
            torch.cuda.synchronize(self.dev)
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._launch_all()
                self.graph = g
            except Exception as e:                  # pragma: no cover - depends on the runtime
                warnings.warn(f"hipGraph capture failed ({e}); launching eagerly")
                self.use_graph = False
                torch.cuda.synchronize(self.dev)
        if self.graph is not None:
            self.graph.replay()
        else:
            self._launch_all()
        if self.range_check == "sync":
            self.check_range()
        if alias_outputs:
            return self.outputs
        return tuple(o.clone() for o in self.outputs)
