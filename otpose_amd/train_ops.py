"""Training-mode operators over the C-ABI (building blocks of the OTPose training step, reference
script/Common.py:91,136-144 runs the model under ``model.train()``).

``conv2d`` / ``batch_norm_relu`` are ``torch.autograd.Function``s whose forward AND backward are HIP launches
(conv forward / dgrad: ``otp_conv2d``; wgrad: ``otp_conv2d_wgrad``; bias grad: ``otp_channel_sum``; BatchNorm with
batch statistics fused with the residual add + ReLU that follow it in HRNet / RSB blocks: ``otp_bn_train_*``).
PyTorch supplies memory, streams and the autograd tape only; CPU tensors raise like every operator here.
"""
from __future__ import annotations

import contextlib
import dataclasses
import os

import torch
from torch.autograd import Function

from . import attn_dropout, hip, ops
from .ops import (ACT_NONE, View, check_f32, out_hw, require_gpu, conv2d_launch, conv2d_wino_launch, conv_desc,
                  pack_conv_weight, pack_wino_weight)


def grad_slot(param):
    """Where the gradient of ``param`` should be written: its slot inside the optimizer's flat gradient buffer
    (:class:`otpose_amd.optim.FusedAdamW`) when that slot is known to be zero-filled AND this is the first request for it in
    the current step, else None (the caller allocates; autograd accumulates as usual).

    Some backward kernels accumulate into their destination (conv2d_grad_weight, dwconv3) and others overwrite, so a slot
    is handed out only while the optimizer vouches for it: ``FusedAdamW.zero_grad()`` opens a new epoch (slots memset),
    ``step()`` closes it.  ``model.zero_grad()`` / ``p.grad = None`` do not open one - the slot then still holds the last
    step's gradient and ordinary tensors are used instead (``FusedAdamW._rehome_grads`` copies them in).  A parameter that
    feeds two autograd nodes of one backward (two forwards summed, shared weights) gets the slot for the first node only:
    autograd sums the second gradient as an ordinary tensor instead of seeing the same memory twice."""
    slot = getattr(param, "_otp_grad_slot", None)
    if slot is None or slot.shape != param.shape:
        return None
    owner = getattr(param, "_otp_grad_owner", param)        # a reshaped view of a parameter names its owner (TrainGraph.conv1d)
    epoch = getattr(owner, "_otp_slot_epoch", None)          # shared [epoch, clean] cell of the owning optimizer
    if epoch is None or not epoch[1] or owner.grad is not None or getattr(owner, "_otp_slot_taken", -1) == epoch[0]:
        return None
    owner._otp_slot_taken = epoch[0]
    # a fresh tensor object over the same memory: autograd adopts an incoming gradient without cloning it only when nobody
    # else holds a reference to that tensor object
    return slot.view(slot.shape)


@dataclasses.dataclass(frozen=True)
class TrainRoutes:
    """The ``OTPOSE_*`` switches of the training step, read once per forward (:meth:`from_env`, ``train.TrainGraph``); the field
    defaults are the switches'.  A Function keeps them on ``ctx``: its backward follows the routes its forward was built with."""
    train_streams: bool = True        # OTPOSE_TRAIN_STREAMS: HRNet branches, def_fuse and encoder 1 on side streams
    recompute: bool = True            # OTPOSE_TRAIN_RECOMPUTE: the attention front as one node that rebuilds its intermediates
    pack_batch: bool = True           # OTPOSE_PACK_BATCH: one launch re-packs every bf16 conv operator (bf16_ops.PackCache)
    block_fuse: bool = True           # OTPOSE_BLOCK_FUSE: a bf16 BasicBlock as one autograd node
    bf16_offsets: bool = True         # OTPOSE_BF16_OFFSETS: the offset / mask convs in front of the DCNs on the bf16 path
    bf16_mlp: bool = True             # OTPOSE_BF16_MLP: the transformer MLP interior on the bf16 path
    mlp_fused_train: bool = False     # OTPOSE_MLP_FUSED_TRAIN=1 (opt-in): GELU / dropout inside the projections' launches
    use_dense_cc: bool = True         # OTPOSE_DENSE_CC: pointwise C -> C layers via csrc/dense.hip, forward and input gradient
    use_x3: bool = True               # OTPOSE_CONV_MATH != "f32": those layers on split products (csrc/densex.hip)
    use_winograd: bool = True         # OTPOSE_WINOGRAD: 3x3 stride-1 convs via csrc/wino.hip, forward and input gradient
    wgrad_stream: bool = True         # OTPOSE_WGRAD_STREAM: bf16 weight gradients on a side stream of the launching stream

    @classmethod
    def from_env(cls) -> "TrainRoutes":
        env = os.environ.get
        on = lambda name: env("OTPOSE_" + name, "1") != "0"                         # noqa: E731
        return cls(train_streams=on("TRAIN_STREAMS"), recompute=on("TRAIN_RECOMPUTE"), pack_batch=on("PACK_BATCH"),
                   block_fuse=on("BLOCK_FUSE"), bf16_offsets=on("BF16_OFFSETS"), bf16_mlp=on("BF16_MLP"),
                   mlp_fused_train=env("OTPOSE_MLP_FUSED_TRAIN", "0") == "1", use_dense_cc=on("DENSE_CC"),
                   use_x3=env("OTPOSE_CONV_MATH", "x3") != "f32", use_winograd=on("WINOGRAD"), wgrad_stream=on("WGRAD_STREAM"))


_ACTIVE_ROUTES = []           # the routes of the training forward(s) being built (train.TrainGraph.forward), innermost last


@contextlib.contextmanager
def active_routes(routes):
    _ACTIVE_ROUTES.append(routes)
    try:
        yield
    finally:
        _ACTIVE_ROUTES.pop()


def current_routes():
    """For ``Function.forward`` only: the active routes, else (a direct call from a test or tool) the environment as it is now.  A
    backward passes what its ``ctx`` holds; the helpers below take routes as an argument (None: called by hand, as above)."""
    return _ACTIVE_ROUTES[-1] if _ACTIVE_ROUTES else TrainRoutes.from_env()


def conv_route(routes, cin, cout, d, hw):
    """The kernel of the fp32 convolution ``d``, forward or (``cin`` / ``cout`` exchanged) input gradient: "dense" - pointwise C -> C
    layers of the temporal encoders (query / key / value / proj) on csrc/dense.hip; "wino" - ops.runs_winograd; else "direct"."""
    if routes.use_dense_cc and d.kh == 1 and d.stride == 1 and d.pad == 0 and cin == cout and ops.dense_cc_supported(cin, hw):
        return "dense"
    return "wino" if ops.runs_winograd(routes.use_winograd, cin, cout, d) else "direct"


def conv2d_forward(x, weight, bias, stride, pad, dil, routes=None):
    routes = routes or TrainRoutes.from_env()
    cout, cin, kh, kw = weight.shape
    ho, wo = out_hw(x.shape[2], x.shape[3], kh, kw, stride, pad, dil)
    out = torch.empty((x.shape[0], cout, ho, wo), dtype=torch.float32, device=x.device)
    iv, ov = View(x), View(out)
    d = conv_desc(iv, ov, cout, kh, kw, stride, pad, dil, ACT_NONE)
    route = conv_route(routes, cin, cout, d, x.shape[2] * x.shape[3])
    if route == "dense":
        _dense_cc_launch(routes, x, weight.reshape(cout, cin), bias, out)
    elif route == "wino":
        conv2d_wino_launch(iv, pack_wino_weight(weight), None, bias, ov, d)
    else:
        conv2d_launch(iv, pack_conv_weight(weight), None, bias, ov, d)
    return out


def _dense_cc_launch(routes, x4, w2, bias, out4, grad=False):
    n, c = x4.shape[:2]
    # split products (csrc/densex.hip) unless the exact-fp32 kernels are asked for, as in the inference engine; ``grad``: x4 is a
    # gradient - bfloat16 pieces (otp_bf16_pieces in csrc/densex.hip), an IEEE-half piece would flush the small ones to zero
    x3 = routes.use_x3 and ops.dense_x3_supported(c, x4.shape[2] * x4.shape[3])
    pk = ops.pack_dense_cc(w2, None, bias, x3=x3, grad=grad)
    ops.dense_cc([x4.view(n, c, -1)], [pk], None, [out4.view(n, c, -1)], x3=x3, grad=grad)


def conv2d_grad_input(grad_out, weight, in_shape, stride, pad, dil, routes=None):
    """dL/dx: a stride-1 convolution of (zero-inserted) grad_out with the flipped, channel-transposed weights."""
    routes = routes or TrainRoutes.from_env()
    cout, cin, kh, kw = weight.shape
    n, _, h, w = in_shape
    L = hip.lib()
    g = grad_out.contiguous()
    if stride > 1:
        # zero-insert to the resolution a stride-1 "full" correlation needs: H + 2*pad - dil*(k-1)
        hd, wd = h + 2 * pad - dil * (kh - 1), w + 2 * pad - dil * (kw - 1)
        gd = torch.empty((n, cout, hd, wd), dtype=torch.float32, device=g.device)
        hip.check(L.otp_dilate(hip.ptr(g), hip.ptr(gd), n * cout, g.shape[2], g.shape[3], stride, hd, wd,
                               hip.stream_of(g)), "otp_dilate")
        g = gd
    gx = torch.empty(in_shape, dtype=torch.float32, device=g.device)
    iv, ov = View(g), View(gx)
    d = conv_desc(iv, ov, cin, kh, kw, 1, dil * (kh - 1) - pad, dil, ACT_NONE)
    route = conv_route(routes, cout, cin, d, h * w) if stride == 1 else "direct"
    if route == "dense":
        _dense_cc_launch(routes, g, weight.reshape(cout, cin).t(), None, gx, grad=True)         # dx = W^T . dy
    elif route == "wino":
        # the transposed convolution as a Winograd conv: weights flipped and channel-transposed, then G g G^T
        wt = weight.flip(2, 3).transpose(0, 1).contiguous()
        conv2d_wino_launch(iv, pack_wino_weight(wt), None, None, ov, d)
    else:
        cin16 = (cin + 15) // 16 * 16
        wp = torch.empty(kh * kw * cout * cin16, dtype=torch.float32, device=g.device)
        hip.check(L.otp_conv2d_pack_weight_dgrad(hip.ptr(weight.contiguous()), hip.ptr(wp), cout, cin, kh, kw,
                                                 hip.stream_of(g)), "otp_conv2d_pack_weight_dgrad")
        conv2d_launch(iv, wp, None, None, ov, d)
    return gx


_WS = {}


def _workspace(device, nbytes):
    """One grow-only scratch buffer per (device, stream) for the wgrad partial sums: every user launches on the current
    stream, so reuse is stream-ordered; the independent paths of a training step run on several streams and each has its own."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    buf = _WS.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
        _WS[key] = buf
    return buf


def conv2d_grad_weight(x, grad_out, weight_shape, stride, pad, dil, out=None):
    """``out``: a zero-filled (Cout, Cin, kh, kw) destination (the kernel accumulates), e.g. a :func:`grad_slot`."""
    cout, cin, kh, kw = weight_shape
    gw = out if out is not None else torch.zeros(weight_shape, dtype=torch.float32, device=x.device)
    x, g = x.contiguous(), grad_out.contiguous()
    L = hip.lib()
    nbytes = L.otp_conv2d_wgrad_workspace(cin, cout)
    ws = _workspace(x.device, nbytes)
    hip.check(L.otp_conv2d_wgrad(hip.ptr(x), hip.ptr(g), hip.ptr(gw), x.shape[0], cin, x.shape[2], x.shape[3],
                                 cout, kh, kw, stride, pad, dil, cin, 0, cout, 0, hip.ptr(ws), nbytes,
                                 hip.stream_of(x)), "otp_conv2d_wgrad")
    return gw


def channel_sum(t, out=None):
    """Per-channel sum over (N, H, W) of a contiguous (N, C, H, W) tensor (bias gradients)."""
    n, c, h, w = t.shape
    L = hip.lib()
    nbytes = L.otp_bn_workspace(n, c, h * w) + 4 * c
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=t.device)
    if out is None:
        out = torch.empty(c, dtype=torch.float32, device=t.device)
    hip.check(L.otp_channel_sum(hip.ptr(t), hip.ptr(out), hip.ptr(ws), nbytes, n, c, h * w, c, 0, hip.stream_of(t)),
              "otp_channel_sum")
    return out


class Conv2dFunction(Function):
    """``F.conv2d(x, weight, bias, stride, padding, dilation)`` (groups = 1, square 1x1 / 3x3 kernels)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, dil):
        require_gpu(x, weight)
        check_f32(x, weight)
        x, weight = x.contiguous(), weight.contiguous()
        ctx.save_for_backward(x, weight)
        ctx.cfg = (stride, pad, dil, bias is not None)
        ctx.params = (weight, bias)                    # gradient slots are looked up at backward time
        ctx.routes = current_routes()                  # ... and the input gradient follows the forward's routes
        return conv2d_forward(x, weight, bias, stride, pad, dil, ctx.routes)

    @staticmethod
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        stride, pad, dil, has_bias = ctx.cfg
        pw, pb = ctx.params
        grad_out = grad_out.contiguous()
        gx = (conv2d_grad_input(grad_out, weight, x.shape, stride, pad, dil, ctx.routes)
              if ctx.needs_input_grad[0] else None)
        gw = (conv2d_grad_weight(x, grad_out, weight.shape, stride, pad, dil, grad_slot(pw))
              if ctx.needs_input_grad[1] else None)
        gb = channel_sum(grad_out, grad_slot(pb)) if has_bias and ctx.needs_input_grad[2] else None
        return gx, gw, gb, None, None, None


def conv2d(x, weight, bias=None, stride=1, padding=0, dilation=1):
    return Conv2dFunction.apply(x, weight, bias, stride, padding, dilation)


class BatchNormReluFunction(Function):
    """``relu?(F.batch_norm(x, running_mean, running_var, gamma, beta, training=True, momentum, eps) (+ res))``;
    the running statistics are updated in place like ``nn.BatchNorm2d`` does."""

    @staticmethod
    def forward(ctx, x, gamma, beta, res, running_mean, running_var, momentum, eps, relu):
        require_gpu(x, gamma, beta)
        check_f32(x, gamma, beta)
        x = x.contiguous()
        n, c, h, w = x.shape
        L = hip.lib()
        nbytes = L.otp_bn_workspace(n, c, h * w)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device)
        y = torch.empty_like(x)
        mean = torch.empty(c, dtype=torch.float32, device=x.device)
        rstd = torch.empty(c, dtype=torch.float32, device=x.device)
        r = res.contiguous() if res is not None else None
        hip.check(L.otp_bn_train_forward(hip.ptr(x), hip.ptr(gamma), hip.ptr(beta), hip.ptr(r), hip.ptr(y), hip.ptr(mean),
                                         hip.ptr(rstd), hip.ptr(running_mean), hip.ptr(running_var), hip.ptr(ws), nbytes,
                                         n, c, h * w, eps, momentum, int(relu), c, 0, c, 0, c, 0, hip.stream_of(x)),
                  "otp_bn_train_forward")
        ctx.save_for_backward(x, gamma, mean, rstd, y if relu else None)
        ctx.has_res = res is not None
        ctx.params = (gamma, beta)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        x, gamma, mean, rstd, y = ctx.saved_tensors
        grad_y = grad_y.contiguous()
        n, c, h, w = x.shape
        L = hip.lib()
        nbytes = L.otp_bn_workspace(n, c, h * w)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device)
        gx = torch.empty_like(x)
        gres = torch.empty_like(x) if ctx.has_res else None
        sg, sb = grad_slot(ctx.params[0]), grad_slot(ctx.params[1])
        gg = sg if sg is not None else torch.empty(c, dtype=torch.float32, device=x.device)
        gb = sb if sb is not None else torch.empty(c, dtype=torch.float32, device=x.device)
        hip.check(L.otp_bn_train_backward(hip.ptr(grad_y), hip.ptr(x), hip.ptr(y), hip.ptr(mean), hip.ptr(rstd),
                                          hip.ptr(gamma), hip.ptr(gx), hip.ptr(gres), hip.ptr(gg), hip.ptr(gb),
                                          hip.ptr(ws), nbytes, n, c, h * w, c, 0, c, 0, c, 0, hip.stream_of(x)),
                  "otp_bn_train_backward")
        return gx, gg, gb, gres, None, None, None, None, None


def batch_norm_relu(x, gamma, beta, res=None, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, relu=True):
    return BatchNormReluFunction.apply(x, gamma, beta, res, running_mean, running_var, momentum, eps, relu)


# ------------------------------------------------------------------------------------------------
# ConvTransformer pieces (reference model/blocks.py), tensors (B, C, T)
# ------------------------------------------------------------------------------------------------
def _chan_sum3(t):
    b, c, n = t.shape
    return channel_sum(t.reshape(b, c, 1, n))


def _ln_fwd(x, gamma, beta, eps):
    """y = channel LayerNorm of a contiguous (B, C, T) tensor; gamma / beta flat (C)."""
    b, c, t = x.shape
    y = torch.empty_like(x)
    hip.check(hip.lib().otp_ln_channel(hip.ptr(x), hip.ptr(gamma), hip.ptr(beta), hip.ptr(y), None, b, c, t, eps,
                                       hip.stream_of(x)), "otp_ln_channel")
    return y


def _ln_bwd(x, g, gy, eps, pgamma, pbeta):
    """(dx, dgamma (C), dbeta (C)) of :func:`_ln_fwd`; the parameter gradients land in the optimizer's slots when free."""
    gy = gy.contiguous()
    b, c, t = x.shape
    L = hip.lib()
    nbytes = L.otp_ln_channel_backward_workspace(b, c, t)
    if nbytes:
        # dx, dgamma and dbeta from one pass over x and dy
        gx = torch.empty_like(x)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
        sg, sb = grad_slot(pgamma), grad_slot(pbeta)
        gg = sg if sg is not None else torch.empty(c, dtype=torch.float32, device=x.device)
        gb = sb if sb is not None else torch.empty(c, dtype=torch.float32, device=x.device)
        hip.check(L.otp_ln_channel_backward_params(hip.ptr(x), hip.ptr(gy), hip.ptr(g), hip.ptr(gx), hip.ptr(gg), hip.ptr(gb),
                                                   hip.ptr(ws), nbytes, b, c, t, eps, hip.stream_of(x)),
                  "otp_ln_channel_backward_params")
        return gx, gg, gb
    gx, dyxh = torch.empty_like(x), torch.empty_like(x)
    hip.check(L.otp_ln_channel_backward(hip.ptr(x), hip.ptr(gy), hip.ptr(g), hip.ptr(gx), hip.ptr(dyxh), b, c, t,
                                        eps, hip.stream_of(x)), "otp_ln_channel_backward")
    return gx, _chan_sum3(dyxh), _chan_sum3(gy)


class LayerNormFunction(Function):
    """Channel LayerNorm of (B, C, T) (model/blocks.py:95-110): biased variance over C, weight / bias (C)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        require_gpu(x)
        check_f32(x)
        x = x.contiguous()
        g, be = gamma.reshape(-1).contiguous(), beta.reshape(-1).contiguous()
        y = _ln_fwd(x, g, be, eps)
        ctx.save_for_backward(x, g)
        ctx.eps, ctx.pshape = eps, gamma.shape
        ctx.params = (gamma, beta)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, g = ctx.saved_tensors
        gx, gg, gb = _ln_bwd(x, g, gy, ctx.eps, ctx.params[0], ctx.params[1])
        return gx, gg.reshape(ctx.pshape), gb.reshape(ctx.pshape), None


def layer_norm(x, gamma, beta, eps=1e-5):
    return LayerNormFunction.apply(x, gamma, beta, eps)


def _dw_fwd(x, w, stride):
    b, c, t = x.shape
    to = (t + 2 - 3) // stride + 1
    y = torch.empty((b, c, to), dtype=torch.float32, device=x.device)
    hip.check(hip.lib().otp_dwconv3_forward(hip.ptr(x), hip.ptr(w), hip.ptr(y), b, c, t, stride, hip.stream_of(x)),
              "otp_dwconv3_forward")
    return y


def _dw_bwd(x, w, gy, stride, pw):
    b, c, t = x.shape
    sw = grad_slot(pw)                                     # zero-filled by the optimizer's zero_grad; the kernel accumulates
    gx, gw = torch.empty_like(x), (sw if sw is not None else torch.zeros_like(w))
    hip.check(hip.lib().otp_dwconv3_backward(hip.ptr(x), hip.ptr(w), hip.ptr(gy.contiguous()), hip.ptr(gx), hip.ptr(gw),
                                             b, c, t, stride, hip.stream_of(x)), "otp_dwconv3_backward")
    return gx, gw


class DwConv3Function(Function):
    """``F.conv1d(x, w (C,1,3), None, stride, 1, 1, groups=C)`` (model/blocks.py:359-381)."""

    @staticmethod
    def forward(ctx, x, w, stride):
        require_gpu(x, w)
        x, w = x.contiguous(), w.contiguous()
        y = _dw_fwd(x, w, stride)
        ctx.save_for_backward(x, w)
        ctx.stride = stride
        ctx.params = (w,)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gx, gw = _dw_bwd(x, w, gy, ctx.stride, ctx.params[0])
        return gx, gw, None


def dwconv3(x, w, stride=1):
    return DwConv3Function.apply(x, w, stride)


class AttnFrontFunction(Function):
    """The front of MultiHeadConvAttention (model/blocks.py:400-440) as one node: ``xn = ln1(x)`` and, for query / key /
    value, ``conv1d_1x1(LayerNorm(dwconv3(xn)))``.  Only ``x`` is kept for the backward; ``xn``, the three depthwise-conv
    outputs and the three LayerNorm outputs (seven (B, C, T) tensors, 420 MB per block at cfg2 - 5 GB over the two temporal
    encoders) are rebuilt there by the same seven launches (~160 us per block), branch by branch, so at most three of them are
    alive at a time.  Arguments after ``eps``: ln1 weight / bias, then per branch (dwconv weight, LayerNorm weight, bias,
    projection weight as (C, C, 1, 1), projection bias or None)."""

    @staticmethod
    def forward(ctx, x, stride, eps, g1, b1, *bp):
        require_gpu(x)
        check_f32(x)
        x = x.contiguous()
        ctx.cfg = (stride, eps)
        ctx.params = (g1, b1) + tuple(bp)
        ctx.routes = current_routes()
        xn = _ln_fwd(x, g1.reshape(-1).contiguous(), b1.reshape(-1).contiguous(), eps)
        outs = []
        for i in range(3):
            dw, lg, lb, w4, bias = bp[5 * i: 5 * i + 5]
            z = _ln_fwd(_dw_fwd(xn, dw.contiguous(), stride), lg.reshape(-1).contiguous(), lb.reshape(-1).contiguous(), eps)
            outs.append(conv2d_forward(z.unsqueeze(2), w4.contiguous(), bias, 1, 0, 1, ctx.routes).squeeze(2))
        ctx.save_for_backward(x)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        (x,) = ctx.saved_tensors
        stride, eps = ctx.cfg
        g1, b1 = ctx.params[:2]
        bp = ctx.params[2:]
        g1f = g1.reshape(-1).contiguous()
        xn = _ln_fwd(x, g1f, b1.reshape(-1).contiguous(), eps)
        gxn, out = None, [None] * 15
        for i in (2, 1, 0):                   # value, key, query: the order autograd would run (and sum) the per-layer nodes in
            dw, lg, lb, w4, bias = bp[5 * i: 5 * i + 5]
            if grads[i] is None:
                continue
            g4 = grads[i].contiguous().unsqueeze(2)
            lgf = lg.reshape(-1).contiguous()
            y = _dw_fwd(xn, dw.contiguous(), stride)
            z4 = _ln_fwd(y, lgf, lb.reshape(-1).contiguous(), eps).unsqueeze(2)
            gz = conv2d_grad_input(g4, w4.contiguous(), z4.shape, 1, 0, 1, ctx.routes).squeeze(2)
            gw = conv2d_grad_weight(z4, g4, w4.shape, 1, 0, 1, grad_slot(w4))
            gb = channel_sum(g4, grad_slot(bias)) if bias is not None else None
            del z4
            gy, glg, glb = _ln_bwd(y, lgf, gz, eps, lg, lb)
            del y, gz
            gxi, gdw = _dw_bwd(xn, dw.contiguous(), gy, stride, dw)
            gxn = gxi if gxn is None else gxn.add_(gxi)
            out[5 * i: 5 * i + 5] = [gdw, glg.reshape(lg.shape), glb.reshape(lb.shape), gw, gb]
        if gxn is None:
            return (None,) * (5 + 15)
        gx, gg1, gb1 = _ln_bwd(x, g1f, gxn, eps, g1, b1)
        return (gx, None, None, gg1.reshape(g1.shape), gb1.reshape(b1.shape)) + tuple(out)


def attn_front(x, stride, eps, ln1, branches):
    """``branches``: three (dwconv weight, LayerNorm weight, LayerNorm bias, projection weight (C, C, 1, 1), bias) tuples
    (query, key, value); ``ln1`` = (weight, bias).  Returns (q, k, v)."""
    flat = [t for br in branches for t in br]
    return AttnFrontFunction.apply(x, stride, eps, ln1[0], ln1[1], *flat)


class GeluFunction(Function):
    @staticmethod
    def forward(ctx, x):
        require_gpu(x)
        x = x.contiguous()
        y = torch.empty_like(x)
        hip.check(hip.lib().otp_gelu_forward(hip.ptr(x), hip.ptr(y), x.numel(), hip.stream_of(x)), "otp_gelu_forward")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        gx = torch.empty_like(x)
        hip.check(hip.lib().otp_gelu_backward(hip.ptr(x), hip.ptr(gy.contiguous()), hip.ptr(gx), x.numel(),
                                              hip.stream_of(x)), "otp_gelu_backward")
        return gx


gelu = GeluFunction.apply


class MaxPool3s2Function(Function):
    """``nn.MaxPool1d(3, 2, 1)`` on (B, C, T) (model/blocks.py:234-238)."""

    @staticmethod
    def forward(ctx, x):
        require_gpu(x)
        x = x.contiguous()
        b, c, t = x.shape
        y = torch.empty((b, c, (t + 2 - 3) // 2 + 1), dtype=torch.float32, device=x.device)
        hip.check(hip.lib().otp_maxpool3s2_forward(hip.ptr(x), hip.ptr(y), b * c, t, hip.stream_of(x)),
                  "otp_maxpool3s2_forward")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        b, c, t = x.shape
        gx = torch.empty_like(x)
        hip.check(hip.lib().otp_maxpool3s2_backward(hip.ptr(x), hip.ptr(gy.contiguous()), hip.ptr(gx), b * c, t,
                                                    hip.stream_of(x)), "otp_maxpool3s2_backward")
        return gx


maxpool3s2 = MaxPool3s2Function.apply


class UpsampleLinearFunction(Function):
    """``nn.Upsample(scale_factor=f, mode='linear', align_corners=False)`` on (B, C, T)."""

    @staticmethod
    def forward(ctx, x, f):
        require_gpu(x)
        x = x.contiguous()
        b, c, t = x.shape
        y = torch.empty((b, c, t * f), dtype=torch.float32, device=x.device)
        hip.check(hip.lib().otp_upsample_linear(hip.ptr(x), hip.ptr(y), b, c, t, f, c, 0, hip.stream_of(x)),
                  "otp_upsample_linear")
        ctx.f, ctx.shape = f, (b, c, t)
        return y

    @staticmethod
    def backward(ctx, gy):
        b, c, t = ctx.shape
        gy = gy.contiguous()
        gx = torch.empty((b, c, t), dtype=torch.float32, device=gy.device)
        hip.check(hip.lib().otp_upsample_linear_backward(hip.ptr(gy), hip.ptr(gx), b, c, t, ctx.f, c, 0,
                                                         hip.stream_of(gy)), "otp_upsample_linear_backward")
        return gx, None


def upsample_linear(x, f):
    return UpsampleLinearFunction.apply(x, f)


class ChanAttnFunction(Function):
    """Channel attention of model/blocks.py:427-447: per (b, head) S = (q*scale) k^T (hs x hs, contraction over T),
    P = softmax(S), O = P v, returned in the ``transpose(2,3).contiguous().view(B, C, T)`` memory image."""

    @staticmethod
    def forward(ctx, q, k, v, n_head, scale, p=0.0, seed=0):
        require_gpu(q, k, v)
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        b, c, t = q.shape
        L = hip.lib()
        out = torch.empty_like(q)
        if p > 0.0:                                            # m P goes to a third region of the workspace, P stays undropped
            nbytes = L.otp_chan_attn_dropout_workspace(b, c, t, n_head)
            ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=q.device)
            hip.check(L.otp_chan_attn_dropout(hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(out), hip.ptr(ws), nbytes, b, c, t,
                                              n_head, scale, p, seed, hip.stream_of(q)), "otp_chan_attn_dropout")
        else:
            nbytes = L.otp_chan_attn_workspace(b, c, t, n_head)
            ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=q.device)
            hip.check(L.otp_chan_attn(hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(out), hip.ptr(ws), nbytes, b, c, t, n_head,
                                      scale, hip.stream_of(q)), "otp_chan_attn")
        bh, hs = b * n_head, c // n_head
        hsp = (hs + 15) // 16 * 16
        ns = L.otp_chan_attn_splits(bh, t)
        # the workspace is slabs (bh ns matrices) | P | m P: attn_workspace in csrc/chanattn.hip states the layout
        probs = ws[bh * ns * hsp * hsp: bh * ns * hsp * hsp + bh * hsp * hsp].clone()    # softmax matrix (undropped), zero padded
        ctx.save_for_backward(q, k, v, probs)
        ctx.cfg, ctx.drop = (n_head, scale), (p, seed)
        return out

    @staticmethod
    def backward(ctx, gout):
        q, k, v, p = ctx.saved_tensors
        n_head, scale = ctx.cfg
        b, c, t = q.shape
        bh, hs = b * n_head, c // n_head
        hsp = (hs + 15) // 16 * 16
        L = hip.lib()
        st = hip.stream_of(q)
        dev = q.device
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)       # noqa: E731
        gout = gout.contiguous()
        d_o = new(bh, hs, t)                                   # dO[bh][i][t] from the [bh][t][i] image
        hip.check(L.otp_transpose_scale(hip.ptr(gout), hip.ptr(d_o), bh, t, hs, 1.0, st), "otp_transpose_scale")
        ns = L.otp_chan_attn_splits(bh, t)
        slabs = new(bh * ns * hsp * hsp)
        # (every product of the backward has a gradient operand: bfloat16 pieces - otp_bf16_pieces in csrc/chanattn.hip)
        hip.check(L.otp_chan_attn_scores_bf16p(hip.ptr(d_o), hip.ptr(v), hip.ptr(slabs), bh, hs, t, st), "otp_chan_attn_scores_bf16p")
        d_s, d_st, p_t = new(bh, hsp, hsp), new(bh, hsp, hsp), new(bh, hsp, hsp)
        drop_p, seed = ctx.drop
        if drop_p > 0.0:
            hip.check(L.otp_softmax_backward_dropout(hip.ptr(slabs), hip.ptr(p), hip.ptr(d_s), hip.ptr(d_st), hip.ptr(p_t), bh, hs,
                                                     ns, drop_p, seed, st), "otp_softmax_backward_dropout")
        else:
            hip.check(L.otp_softmax_backward(hip.ptr(slabs), hip.ptr(p), hip.ptr(d_s), hip.ptr(d_st), hip.ptr(p_t), bh, hs, ns,
                                             st), "otp_softmax_backward")
        tmp = new(bh, t, hs)
        grads = []
        for src, mat, sc in ((k, d_s, scale), (q, d_st, scale), (d_o, p_t, 1.0)):
            hip.check(L.otp_chan_attn_apply_bf16p(hip.ptr(src), hip.ptr(mat), hip.ptr(tmp), bh, hs, t, st), "otp_chan_attn_apply_bf16p")
            g = new(b, c, t)
            hip.check(L.otp_transpose_scale(hip.ptr(tmp), hip.ptr(g), bh, t, hs, sc, st), "otp_transpose_scale")
            grads.append(g)
        return grads[0], grads[1], grads[2], None, None, None, None


def chan_attn(q, k, v, n_head, scale, dropout_p=0.0, seed=None):
    """``dropout_p`` in [0, 1): attention-probability dropout on the hs x hs matrix between the softmax and the apply step
    (blocks.py:392; the mask of otpose_amd/attn_dropout.py, ``seed`` None = one draw from the CUDA generator per call)."""
    p, seed = attn_dropout.resolve(dropout_p, seed, q.device, "chan_attn: dropout_p")
    return ChanAttnFunction.apply(q, k, v, n_head, scale, p, seed)


class LocalAttnFunction(Function):
    """Local-window attention of model/blocks.py:479-833 (``ops.local_attn``): the forward also writes the softmax band P
    (B n_head, T, window) and keeps it with q, k, v; the backward is ``otp_local_attn_backward`` (two gather-form launches and a
    fixed-order fold for ``rel_pe``: deterministic, no atomics)."""

    @staticmethod
    def forward(ctx, q, k, v, rel_pe, n_head, window_size, scale, p=0.0, seed=0):
        require_gpu(q, k, v)
        check_f32(q, k, v)
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        b, c, t = q.shape
        ops.check_local_attn(c, t, n_head, window_size)
        rel = ops.rel_pe_table(rel_pe, n_head, window_size, q)
        out = torch.empty_like(q)
        probs = torch.empty((b * n_head, t, window_size), dtype=torch.float32, device=q.device)
        args = ops.local_attn_args(q, k, v, rel, out, probs, n_head, window_size, scale)
        if p > 0.0:                                            # probs keeps the undropped band
            hip.check(hip.lib().otp_local_attn_dropout(*args, p, seed, hip.stream_of(q)), "otp_local_attn_dropout")
        else:
            hip.check(hip.lib().otp_local_attn(*args, hip.stream_of(q)), "otp_local_attn")
        ctx.save_for_backward(q, k, v, probs)
        ctx.cfg, ctx.drop = (n_head, int(window_size), scale), (p, seed)
        ctx.params = (rel_pe,)
        return out

    @staticmethod
    def backward(ctx, gout):
        q, k, v, probs = ctx.saved_tensors
        n_head, window, scale = ctx.cfg
        rel_pe = ctx.params[0]
        b, c, t = q.shape
        L = hip.lib()
        gout = gout.contiguous()
        gq, gk, gv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
        grel = None
        if rel_pe is not None and ctx.needs_input_grad[3]:
            slot = grad_slot(rel_pe)
            grel = slot if slot is not None else torch.empty(rel_pe.shape, dtype=torch.float32, device=q.device)
        nbytes = L.otp_local_attn_backward_workspace(b, c, t, n_head, window)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=q.device)
        p, seed = ctx.drop
        if p > 0.0:
            hip.check(L.otp_local_attn_backward_dropout(hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(probs), hip.ptr(gout),
                                                        hip.ptr(gq), hip.ptr(gk), hip.ptr(gv), hip.ptr(grel), hip.ptr(ws), nbytes,
                                                        b, c, t, n_head, window, scale, p, seed, hip.stream_of(q)),
                      "otp_local_attn_backward_dropout")
        else:
            hip.check(L.otp_local_attn_backward(hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(probs), hip.ptr(gout), hip.ptr(gq),
                                                hip.ptr(gk), hip.ptr(gv), hip.ptr(grel), hip.ptr(ws), nbytes, b, c, t, n_head,
                                                window, scale, hip.stream_of(q)), "otp_local_attn_backward")
        return gq, gk, gv, grel, None, None, None, None, None


def local_attn(q, k, v, n_head, window_size, scale, rel_pe=None, dropout_p=0.0, seed=None):
    """``dropout_p`` in [0, 1): attention-probability dropout on the band (blocks.py:572; the mask of otpose_amd/attn_dropout.py,
    ``seed`` None = one draw from the CUDA generator per call)."""
    p, seed = attn_dropout.resolve(dropout_p, seed, q.device, "local_attn: dropout_p")
    return LocalAttnFunction.apply(q, k, v, rel_pe, n_head, window_size, scale, p, seed)


CONV_EMBD_TRAIN_KS = (1, 3)           # the kernel sizes conv2d_grad_weight (otp_conv2d_wgrad) takes
CONV_EMBD_DGRAD_BLOCK = 32            # output channels per conv2d_grad_input launch of the conv embedding's backward


def check_conv_embd_train(weight_shape):
    """Raise ``ValueError`` for a conv embedding layer whose convolution gradients are not built: ``otp_conv2d_wgrad`` takes 1x1
    and 3x3 kernels (the forward, ``ops.conv_embd``, also 5x5)."""
    if weight_shape[2] not in CONV_EMBD_TRAIN_KS:
        raise ValueError(f"conv_embd: training needs a kernel size in {CONV_EMBD_TRAIN_KS} (the weight gradient kernel), got a "
                         f"{tuple(weight_shape)} weight")


class ConvEmbdFunction(Function):
    """One conv embedding layer (``ops.conv_embd``): the forward launch also writes z, the convolution result in front of the
    norm, and keeps it with x and the parameters.  The backward is ``otp_conv_embd_backward_pre`` (grad_z, grad of the LayerNorm
    parameters: fixed-order sums, deterministic), then ``conv2d_grad_input`` / ``conv2d_grad_weight`` on the exact-fp32 direct
    kernels and ``channel_sum`` for a bias."""

    @staticmethod
    def forward(ctx, x, weight, bias, ln_weight, ln_bias, pe, eps):
        require_gpu(x, weight)
        check_f32(x, weight)
        check_conv_embd_train(weight.shape)
        x, weight = x.contiguous(), weight.contiguous()
        b_, gamma, beta, pe_ = ops.conv_embd_params(x.shape, weight, bias, ln_weight, ln_bias, pe, x.device)
        cout, ks = weight.shape[0], weight.shape[2]
        n, _, h, w = x.shape
        out = torch.empty((n, cout, h * w), dtype=torch.float32, device=x.device)
        z = torch.empty_like(out)
        hip.check(hip.lib().otp_conv_embd(*ops.conv_embd_args(x, ops.pack_conv_embd_weight(weight), b_, gamma, beta, pe_, out, z,
                                                              cout, ks, eps), hip.stream_of(x)), "otp_conv_embd")
        ctx.save_for_backward(x, weight, z, b_, gamma, beta)
        ctx.eps = float(eps)
        ctx.params = (weight, bias, ln_weight, ln_bias)
        # the layer is exact fp32 in both directions: no Winograd transform, no split products in its input gradient
        ctx.routes = dataclasses.replace(current_routes(), use_winograd=False, use_x3=False, use_dense_cc=False)
        return out

    @staticmethod
    def backward(ctx, gy):
        x, weight, z, b_, gamma, beta = ctx.saved_tensors
        pw, pb, pg, pbt = ctx.params
        n, cout, t = z.shape
        ks = weight.shape[2]
        L = hip.lib()
        gy = gy.contiguous()
        gz = torch.empty_like(z)
        gg = gb_ln = ws = None
        nbytes = 0
        if gamma is not None:
            def slot(p):
                s = grad_slot(p)
                return s.view(-1) if s is not None else torch.empty(cout, dtype=torch.float32, device=z.device)
            gg, gb_ln = slot(pg), slot(pbt)
            nbytes = L.otp_conv_embd_backward_pre_workspace(n, cout, t)
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=z.device)
        hip.check(L.otp_conv_embd_backward_pre(hip.ptr(z), hip.ptr(b_), hip.ptr(gamma), hip.ptr(beta), hip.ptr(gy), hip.ptr(gz),
                                               hip.ptr(gg), hip.ptr(gb_ln), hip.ptr(ws), nbytes, n, cout, t, ctx.eps,
                                               hip.stream_of(z)), "otp_conv_embd_backward_pre")
        gz4 = gz.view(n, cout, x.shape[2], x.shape[3])
        gx = None
        if ctx.needs_input_grad[0]:
            # blocked summation over the output channels: the input-gradient kernel sums its Cout ks^2 terms as one fmaf chain
            # (1224 terms at 136 channels and 3x3 - four times the rounding error of a vectorised fp32 convolution), so it runs on
            # slices of CONV_EMBD_DGRAD_BLOCK channels and the slice results are added
            for c0 in range(0, cout, CONV_EMBD_DGRAD_BLOCK):
                c1 = min(cout, c0 + CONV_EMBD_DGRAD_BLOCK)
                part = conv2d_grad_input(gz4[:, c0:c1].contiguous(), weight[c0:c1].contiguous(), x.shape, 1, ks // 2, 1, ctx.routes)
                gx = part if gx is None else gx.add_(part)
        gw = conv2d_grad_weight(x, gz4, weight.shape, 1, ks // 2, 1, grad_slot(pw)) if ctx.needs_input_grad[1] else None
        gbias = channel_sum(gz4, grad_slot(pb)).reshape(pb.shape) if pb is not None and ctx.needs_input_grad[2] else None
        if gamma is not None:
            gg, gb_ln = gg.reshape(pg.shape), gb_ln.reshape(pbt.shape)
        return gx, gw, gbias, gg, gb_ln, None, None


def conv_embd(x, weight, bias, ln_weight, ln_bias, pe=None, eps=1e-5):
    return ConvEmbdFunction.apply(x, weight, bias, ln_weight, ln_bias, pe, eps)


class SpatialMeanFunction(Function):
    """``F.adaptive_avg_pool2d(x, (1, 1))``: (N, C, H, W) -> (N, C, 1, 1), thread-strided sums added in a fixed order
    (csrc/prm.hip); the backward broadcasts ``g / (H W)``."""

    @staticmethod
    def forward(ctx, x):
        require_gpu(x)
        check_f32(x)
        if x.dim() != 4:
            raise ValueError(f"spatial_mean: x must be (N, C, H, W), got {tuple(x.shape)}")
        x = x.contiguous()
        n, c, h, w = x.shape
        out = torch.empty((n, c, 1, 1), dtype=torch.float32, device=x.device)
        hip.check(hip.lib().otp_spatial_mean(hip.ptr(x), hip.ptr(out), n, c, h * w, hip.stream_of(x)), "otp_spatial_mean")
        ctx.shape = tuple(x.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        n, c, h, w = ctx.shape
        g = g.contiguous()
        gx = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
        hip.check(hip.lib().otp_spatial_mean_backward(hip.ptr(g), hip.ptr(gx), n, c, h * w, hip.stream_of(g)),
                  "otp_spatial_mean_backward")
        return gx


def spatial_mean(x):
    return SpatialMeanFunction.apply(x)


DWCONV2D_KS = (9,)                    # the kernel sizes csrc/prm.hip instantiates


class DwConv2dFunction(Function):
    """``F.conv2d(x, w (C, 1, k, k), bias, 1, k // 2, 1, groups=C)`` for k = 9 (RSB.py:187-189).  The input gradient is the same
    gather with the taps reversed, the weight gradient comes from per-workgroup partial sums added in a fixed order, the bias
    gradient from ``channel_sum``: deterministic."""

    @staticmethod
    def forward(ctx, x, w, bias):
        require_gpu(x, w)
        check_f32(x, w)
        if x.dim() != 4 or w.dim() != 4 or w.shape[1] != 1 or w.shape[0] != x.shape[1] or w.shape[2] != w.shape[3]:
            raise ValueError(f"dwconv2d: x must be (N, C, H, W) and w (C, 1, k, k), got {tuple(x.shape)} and {tuple(w.shape)}")
        if w.shape[2] not in DWCONV2D_KS:
            raise ValueError(f"dwconv2d: the kernel size must be one of {DWCONV2D_KS}, got {w.shape[2]}")
        if bias is not None and bias.numel() != w.shape[0]:
            raise ValueError(f"dwconv2d: bias has {bias.numel()} entries, the layer has {w.shape[0]} channels")
        x, w = x.contiguous(), w.contiguous()
        n, c, h, wd = x.shape
        y = torch.empty_like(x)
        b_ = None if bias is None else bias.detach().contiguous()
        hip.check(hip.lib().otp_dwconv2d(hip.ptr(x), hip.ptr(w), hip.ptr(b_), hip.ptr(y), n, c, h, wd, w.shape[2], 0,
                                         hip.stream_of(x)), "otp_dwconv2d")
        ctx.save_for_backward(x, w)
        ctx.params = (w, bias)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        pw, pb = ctx.params
        n, c, h, wd = x.shape
        ks = w.shape[2]
        L = hip.lib()
        gy = gy.contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            hip.check(L.otp_dwconv2d(hip.ptr(gy), hip.ptr(w), None, hip.ptr(gx), n, c, h, wd, ks, 1, hip.stream_of(x)),
                      "otp_dwconv2d")
        if ctx.needs_input_grad[1]:
            slot = grad_slot(pw)
            gw = slot if slot is not None else torch.empty_like(w)
            nbytes = L.otp_dwconv2d_wgrad_workspace(n, c, h, wd, ks)
            ws = _workspace(x.device, nbytes)
            hip.check(L.otp_dwconv2d_wgrad(hip.ptr(x), hip.ptr(gy), hip.ptr(gw), hip.ptr(ws), nbytes, n, c, h, wd, ks,
                                           hip.stream_of(x)), "otp_dwconv2d_wgrad")
        if pb is not None and ctx.needs_input_grad[2]:
            gb = channel_sum(gy, grad_slot(pb))
        return gx, gw, gb


def dwconv2d(x, w, bias=None):
    return DwConv2dFunction.apply(x, w, bias)


class PrmCombineFunction(Function):
    """``f * (1 + sigmoid(a) * sigmoid(s))`` (RSB.py:198, 201-202): f, s (N, C, H, W), a (N, C, 1, 1), both gates pre-sigmoid.
    The backward is one launch; the per-(n, c) sum of grad_a runs in a fixed order."""

    @staticmethod
    def forward(ctx, f, a, s):
        require_gpu(f, a, s)
        check_f32(f, a, s)
        if f.dim() != 4 or s.shape != f.shape or a.numel() != f.shape[0] * f.shape[1]:
            raise ValueError(f"prm_combine: f and s must be (N, C, H, W) and a (N, C, 1, 1), got {tuple(f.shape)}, {tuple(s.shape)}, "
                             f"{tuple(a.shape)}")
        f, a, s = f.contiguous(), a.contiguous(), s.contiguous()
        n, c, h, w = f.shape
        out = torch.empty_like(f)
        hip.check(hip.lib().otp_prm_combine(hip.ptr(f), hip.ptr(a), hip.ptr(s), hip.ptr(out), n, c, h * w, hip.stream_of(f)),
                  "otp_prm_combine")
        ctx.save_for_backward(f, a, s)
        return out

    @staticmethod
    def backward(ctx, g):
        f, a, s = ctx.saved_tensors
        n, c, h, w = f.shape
        g = g.contiguous()
        gf, ga, gs = torch.empty_like(f), torch.empty_like(a), torch.empty_like(s)
        hip.check(hip.lib().otp_prm_combine_backward(hip.ptr(f), hip.ptr(a), hip.ptr(s), hip.ptr(g), hip.ptr(gf), hip.ptr(ga),
                                                     hip.ptr(gs), n, c, h * w, hip.stream_of(f)), "otp_prm_combine_backward")
        return gf, ga, gs


def prm_combine(f, a, s):
    return PrmCombineFunction.apply(f, a, s)


class ScaleResidualFunction(Function):
    """``x + drop_path(scale * a)`` of a TransformerBlock (model/blocks.py:277-279, AffineDropPath :283-316): ``scale`` is the
    (1, C, 1) AffineDropPath parameter, ``mask`` (B,) the per-sample Bernoulli(keep) / keep factors (None: no drop-path)."""

    @staticmethod
    def forward(ctx, x, a, scale, mask):
        require_gpu(x, a, scale)
        check_f32(x, a)
        x, a = x.contiguous(), a.contiguous()
        b, c, t = x.shape
        sc = scale.reshape(-1).contiguous()
        out = torch.empty_like(x)
        hip.check(hip.lib().otp_scale_residual(hip.ptr(x), hip.ptr(a), hip.ptr(sc), hip.ptr(mask), hip.ptr(out), b, c, t,
                                               hip.stream_of(x)), "otp_scale_residual")
        ctx.save_for_backward(a, sc, mask)
        ctx.pshape = scale.shape
        ctx.params = (scale,)
        return out

    @staticmethod
    def backward(ctx, g):
        a, sc, mask = ctx.saved_tensors
        g = g.contiguous()
        b, c, t = a.shape
        L = hip.lib()
        nbytes = L.otp_scale_residual_backward_workspace(b, c, t)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=a.device)
        ga = torch.empty_like(a)
        ss = grad_slot(ctx.params[0])
        gs = ss if ss is not None else torch.empty(c, dtype=torch.float32, device=a.device)
        hip.check(L.otp_scale_residual_backward(hip.ptr(g), hip.ptr(a), hip.ptr(sc), hip.ptr(mask), hip.ptr(ga), hip.ptr(gs),
                                                hip.ptr(ws), nbytes, b, c, t, hip.stream_of(a)), "otp_scale_residual_backward")
        return g, ga, gs.reshape(ctx.pshape), None


def scale_residual(x, a, scale, mask=None):
    return ScaleResidualFunction.apply(x, a, scale, mask)
