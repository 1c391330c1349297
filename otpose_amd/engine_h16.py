"""fp16-storage inference engine: ``cfg.MODEL.DTYPE = "fp16"`` (BASELINE.json configs[4]).

The HRNet backbone (reference model/HRNet.py:116-152 - 86 % of the forward's FLOPs and almost all of its activation bytes) runs
on H8 images - every activation between its layers is IEEE half, [N][C / 8][H * W] records of 8 channels (csrc/h16.hip) - with
ONE f16 MFMA product per multiply where the fp32 engine spends three on two-piece operands, fp32 accumulation, BatchNorm (eval)
folded into the half weights (times a per-layer power of two) and an fp32 shift.  ``rough`` leaves the backbone as fp32 NCHW
heat-maps; the temporal encoders, RSB heads and the warping head behind it are the parent engine's launches (fp32 tensors; with
``MODEL.DTYPE = "fp16"`` their matrix products also take half operands once - see ``InferenceEngine.half_products``).

The reference never runs below fp32 (no AMP anywhere: SURVEY.md), although its native DCN op dispatches half
(thirdparty/deform_conv/src/deform_conv_cuda_kernel.cu:719), so this engine is an extension: validated against the fp32 engine
and the oracle with a stated tolerance (tests/test_gpu_h16_engine.py), never the default of cfg2.  There is no fallback inside:
a layer the fp16 kernels do not cover raises at build time.
"""
from __future__ import annotations

from typing import List

from . import ops
from .engine import InferenceEngine, plain_conv
from .ops import ACT_NONE, ACT_RELU, H8, View


class InferenceEngineH16(InferenceEngine):
    h16 = True

    def _build(self):
        """The fp16-storage engine does not carry the token-encoder keys: ``ValueError`` at construction, before any launch."""
        if any(getattr(self.model, n, None) is not None for n in ("token_encoder1", "token_encoder2", "flow_token_encoder")):
            raise ValueError("MODEL.TOKEN_LAYERS / MODEL.FLOW_TOKEN_LAYERS: the fp16-storage engine does not carry the token "
                             "encoders (exact-fp32 attention); use the fp32 engine")
        super()._build()

    # ---- emitters -------------------------------------------------------------------------------------------------------------
    def h8(self, n, c, h, w) -> H8:
        """A static H8 activation buffer (2 bytes per element)."""
        return H8(self.new((n * c * h * w + 1) // 2), n, c, h, w)

    def h_conv3(self, x: H8, conv, bn, act, res: H8 = None) -> H8:
        """act(bn(conv3x3(x)) (+ res)) on H8 images (csrc/h16.hip: otp_h16_conv3x3)."""
        s = conv.stride[0]
        if s not in (1, 2) or not plain_conv(conv, 3, stride=s, cin=x.C):
            raise RuntimeError(f"fp16 engine: no kernel for {conv}")
        sc, sh = self._bn_fold(bn)
        w = self.dev_param(conv.weight)
        k = ops.h16_weight_exponent(w, sc)
        wp = ops.pack_h16_conv_weight(w, sc, k)
        out = self.h8(x.N, conv.out_channels, x.H // s, x.W // s)
        d = ops.h16_conv_desc(x, conv.out_channels, s, act, out, res, k)
        if not ops.h16_conv_supported(d):
            raise RuntimeError(f"fp16 engine: otp_h16_conv3x3 does not cover {conv} on a {x.N} x {x.C} x {x.H} x {x.W} input")
        self._keep += [wp, d]
        self.call(self.lib.otp_h16_conv3x3, "otp_h16_conv3x3", *ops.h16_conv3x3_args(x, wp, sh, out, d, res))
        return out

    def h_pw(self, x: H8, conv, bn, relu, res: H8 = None, out=None):
        """act(bn(conv1x1(x)) (+ res)): H8 -> H8, or -> an fp32 NCHW :class:`View` (``out``)."""
        if not plain_conv(conv, 1, dil=None, bias=None, cin=x.C):
            raise RuntimeError(f"fp16 engine: no kernel for {conv}")
        cout = conv.out_channels
        if not ops.h16_pointwise_supported(x.C, cout):
            raise RuntimeError(f"fp16 engine: otp_h16_pointwise does not cover {conv}")
        w = self.dev_param(conv.weight)
        if bn is not None:
            sc, sh = self._bn_fold(bn, conv.bias)
        else:
            sc, sh = None, (self.dev_param(conv.bias) if conv.bias is not None else None)
        k = ops.h16_weight_exponent(w, sc)
        pk = ops.pack_h16_pointwise(w, sc, sh, k)
        self._keep += [pk, sh]
        if out is None:
            out = self.h8(x.N, cout, x.H, x.W)
        self.call(self.lib.otp_h16_pointwise, "otp_h16_pointwise", *ops.h16_pointwise_args(x, pk, cout, out, relu, res, k))
        return out

    def h_upsample_add(self, lows: List[H8], factors, res: H8, relu=True) -> H8:
        out = self.h8(res.N, res.C, res.H, res.W)
        args, arrays = ops.h16_upsample_add_args(lows, factors, res, out, relu)
        self._keep += arrays
        self.call(self.lib.otp_h16_upsample_add, "otp_h16_upsample_add", *args)
        return out

    # ---- HRNet (reference model/HRNet.py:116-152) ------------------------------------------------------------------------------
    def h_bottleneck(self, blk, x: H8) -> H8:
        """model/HRNet.py:551-571: 1x1 -> 3x3 -> 1x1 (+ shortcut), ReLU after each."""
        res = x
        if blk.downsample is not None:
            self.fork((1,))                                      # the 1x1 shortcut only needs x: beside conv1 / conv2
            self.on_stream(1)
            res = self.h_pw(x, blk.downsample[0], blk.downsample[1], relu=False)
            self.on_stream(0)
        y = self.h_pw(x, blk.conv1, blk.bn1, relu=True)
        y = self.h_conv3(y, blk.conv2, blk.bn2, ACT_RELU)
        if blk.downsample is not None:
            self.join((1,))
        return self.h_pw(y, blk.conv3, blk.bn3, relu=True, res=res)

    def h_module(self, mod, xs: List[H8], fork_in=True, join_out=True) -> List[H8]:
        """One HighResolutionModule (model/HRNet.py:478-496): branches of four BasicBlocks (:500-530), then the fuse rows
        y_i = relu(sum_j f_ij(x_j)) (:487-494).  Branch i and row i run on stream i (see InferenceEngine.hr_module)."""
        n = mod.num_branches
        xs = list(xs)
        if fork_in:
            self.fork(range(1, n))
        for i in range(n):
            self.on_stream(i)
            x = xs[i]
            for blk in mod.branches[i]:
                if getattr(blk, "downsample", None) is not None or hasattr(blk, "conv3"):
                    raise RuntimeError("fp16 engine: HighResolutionModule branches are BasicBlocks")
                y = self.h_conv3(x, blk.conv1, blk.bn1, ACT_RELU)
                x = self.h_conv3(y, blk.conv2, blk.bn2, ACT_RELU, res=x)
            xs[i] = x
        self.on_stream(0)
        self.join(range(1, n))
        if n == 1:
            return xs
        self.fork(range(1, len(mod.fuse_layers)))
        outs = []
        for i in range(len(mod.fuse_layers)):
            self.on_stream(i)
            # the identity term starts the sum; the down-sampling chains (j < i) add to it in their last conv's epilogue, the
            # up-sampled terms (j > i: 1x1 conv + BN at low resolution, :426-439) all at once in the row's tail, which applies the ReLU
            y = xs[i]
            downs, ups = [j for j in range(n) if j < i], [j for j in range(n) if j > i]
            for idx, j in enumerate(downs):
                fl = mod.fuse_layers[i][j]
                t = xs[j]
                for k in range(len(fl) - 1):
                    t = self.h_conv3(t, fl[k][0], fl[k][1], ACT_RELU)
                last = idx == len(downs) - 1 and not ups
                y = self.h_conv3(t, fl[-1][0], fl[-1][1], ACT_RELU if last else ACT_NONE, res=y)
            if ups:
                lows = [self.h_pw(xs[j], mod.fuse_layers[i][j][0], mod.fuse_layers[i][j][1], relu=False) for j in ups]
                y = self.h_upsample_add(lows, [2 ** (j - i) for j in ups], y, relu=True)
            outs.append(y)
        self.on_stream(0)
        if join_out:
            self.join(range(1, len(mod.fuse_layers)))
        return outs

    def hrnet(self, net, x_in: View) -> View:
        L = self.lib
        c1 = net.conv1
        n_in, c_in, h_in, w_in = x_in.t.shape
        if not (x_in.coff == 0 and x_in.C == c_in == 3 * self.F and plain_conv(c1, 3, stride=2, dil=None, groups=None, cin=3)
                and L.otp_h16_stem_supported(n_in, self.F, h_in, w_in, c1.out_channels)):
            raise RuntimeError("fp16 engine: the stem kernel does not cover this input")
        sc, sh = self._bn_fold(net.bn1)
        pk = ops.pack_h16_stem(self.dev_param(c1.weight), sc, sh)
        self._keep.append(pk)
        x = self.h8(self.F * n_in, c1.out_channels, (h_in - 1) // 2 + 1, (w_in - 1) // 2 + 1)
        self.call(L.otp_h16_stem, "otp_h16_stem", *ops.stem_conv_x3_args(x_in.t, pk, x, self.F, c1.out_channels))
        x = self.h_conv3(x, net.conv2, net.bn2, ACT_RELU)
        for blk in net.layer1:
            x = self.h_bottleneck(blk, x)

        def new_branch(s, z, tr):
            for step in tr:
                z = self.h_conv3(z, step[0], step[1], ACT_RELU)
            return z
        ys = self.hr_stages(net, x, lambda s, y, tr: self.h_conv3(y, tr[0], tr[1], ACT_RELU), new_branch,
                            lambda s, mi, n_mods, mod, xs, fork_in, join_out: self.h_module(mod, xs, fork_in, join_out))
        fl = net.final_layer
        rough = View(self.new(self.F * self.B, self.J, self.h, self.w))
        self.h_pw(ys[0], fl, None, relu=False, out=rough)          # final 1x1 conv with bias (:108-114): fp32 heat-maps
        return rough
