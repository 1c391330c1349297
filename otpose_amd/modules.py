"""Parameter tree of OTPose with the reference's module/parameter names.

This file defines *containers*: every sub-module below owns exactly the parameters and buffers
the corresponding reference module owns, under the same attribute names, so that
``state_dict()`` / ``load_state_dict()`` round-trip with reference checkpoints and so that the
reference's optimizer grouping (thirdparty/utils/train_utils.py:62-113, which keys on the types
``HRNet``, ``LayerNorm``, ``AffineDropPath``, ``DeformableCONV``, ``CHAIN_RSB_BLOCKS``,
``nn.Conv1d`` and on name prefixes) classifies every parameter.  None of the containers computes
anything: the arithmetic lives in the HIP library behind ``include/otpose_hip.h`` and is driven by
:mod:`otpose_amd.engine` (whole forward) and :mod:`otpose_amd.ops` (operator level).

Key-set parity with the reference is checked by tests/test_state_dict_parity.py against
tests/golden/state_dict_w32.json (generated from the reference import).

Reference structure followed (names only): model/HRNet.py:57-114,160-250,341-473,500-571;
model/ConvVideoTransformer.py:21-111; model/blocks.py:67-93,185-262,283-295,336-396;
model/RSB.py:10-75,106-118; model/layers.py:9-26; model/OTPose.py:181-255.
"""
from __future__ import annotations

import math
from typing import List, Sequence

import numpy as np
import torch
from torch import nn

BN_MOMENTUM = 0.1


# ----------------------------------------------------------------------------------------------
# small helpers
# ----------------------------------------------------------------------------------------------
class _Container(nn.Module):
    """A module that only owns parameters; calling it is a programming error."""

    def forward(self, *a, **k):  # pragma: no cover - guard
        raise RuntimeError(
            f"{type(self).__name__} is a parameter container; run the model through "
            "otpose_amd.OTPose.forward (HIP engine)")


class ReLU(_Container):
    """Parameter-free placeholder that keeps Sequential indices aligned with the reference."""


class Interpolate(_Container):
    """Nearest up-sampling marker inside HRNet fuse layers (reference model/HRNet.py:574-583)."""

    def __init__(self, scale_factor: int, mode: str = "nearest"):
        super().__init__()
        self.scale_factor = scale_factor
        self.mode = mode


def _conv(cin, cout, k, stride=1, pad=0, dil=1, bias=False):
    return nn.Conv2d(cin, cout, k, stride, pad, dilation=dil, bias=bias)


def _bn(c):
    return nn.BatchNorm2d(c, momentum=BN_MOMENTUM)


def _seq_conv_bn(cin, cout, k, stride, pad, relu: bool) -> nn.Sequential:
    mods: List[nn.Module] = [_conv(cin, cout, k, stride, pad), _bn(cout)]
    if relu:
        mods.append(ReLU())
    return nn.Sequential(*mods)


# ----------------------------------------------------------------------------------------------
# HRNet (reference model/HRNet.py)
# ----------------------------------------------------------------------------------------------
class BasicBlock(_Container):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = _conv(inplanes, planes, 3, stride, 1)
        self.bn1 = _bn(planes)
        self.conv2 = _conv(planes, planes, 3, 1, 1)
        self.bn2 = _bn(planes)
        self.downsample = downsample
        self.stride = stride


class Bottleneck(_Container):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = _conv(inplanes, planes, 1)
        self.bn1 = _bn(planes)
        self.conv2 = _conv(planes, planes, 3, stride, 1)
        self.bn2 = _bn(planes)
        self.conv3 = _conv(planes, planes * 4, 1)
        self.bn3 = _bn(planes * 4)
        self.downsample = downsample
        self.stride = stride


_BLOCKS = {"BASIC": BasicBlock, "BOTTLENECK": Bottleneck}


def _block_chain(block, inplanes, planes, count, stride=1) -> nn.Sequential:
    down = None
    if stride != 1 or inplanes != planes * block.expansion:
        down = nn.Sequential(_conv(inplanes, planes * block.expansion, 1, stride), _bn(planes * block.expansion))
    chain = [block(inplanes, planes, stride, down)]
    chain += [block(planes * block.expansion, planes) for _ in range(1, count)]
    return nn.Sequential(*chain)


class HighResolutionModule(_Container):
    """Parallel branches + cross-resolution fuse (reference model/HRNet.py:341-473)."""

    def __init__(self, num_branches, block, num_blocks, num_inchannels, num_channels,
                 multi_scale_output=True):
        super().__init__()
        self.num_branches = num_branches
        self.multi_scale_output = multi_scale_output
        self.num_inchannels = list(num_inchannels)
        branches = []
        for i in range(num_branches):
            branches.append(_block_chain(block, self.num_inchannels[i], num_channels[i], num_blocks[i]))
            self.num_inchannels[i] = num_channels[i] * block.expansion
        self.branches = nn.ModuleList(branches)
        self.fuse_layers = self._fuse_layers() if num_branches > 1 else None

    def _fuse_layers(self):
        ch = self.num_inchannels
        rows = []
        for i in range(self.num_branches if self.multi_scale_output else 1):
            row: List[nn.Module | None] = []
            for j in range(self.num_branches):
                if j > i:   # lower resolution -> 1x1 conv, BN, nearest x2^(j-i)
                    row.append(nn.Sequential(_conv(ch[j], ch[i], 1), _bn(ch[i]), Interpolate(2 ** (j - i))))
                elif j == i:
                    row.append(None)
                else:       # higher resolution -> (i-j) stride-2 3x3 convs
                    steps = [_seq_conv_bn(ch[j], ch[j], 3, 2, 1, relu=True) for _ in range(i - j - 1)]
                    steps.append(_seq_conv_bn(ch[j], ch[i], 3, 2, 1, relu=False))
                    row.append(nn.Sequential(*steps))
            rows.append(nn.ModuleList(row))
        return nn.ModuleList(rows)


class HRNet(_Container):
    """HRNet pose backbone container (reference model/HRNet.py:57-114)."""

    def __init__(self, cfg, **kwargs):
        super().__init__()
        extra = cfg["MODEL"]["EXTRA"]
        self.conv1 = _conv(3, 64, 3, 2, 1)
        self.bn1 = _bn(64)
        self.conv2 = _conv(64, 64, 3, 2, 1)
        self.bn2 = _bn(64)
        self.layer1 = _block_chain(Bottleneck, 64, 64, 4)

        pre = [256]
        self.stage_cfgs = []
        for s in (2, 3, 4):
            scfg = extra[f"STAGE{s}"]
            block = _BLOCKS[scfg["BLOCK"]]
            cur = [c * block.expansion for c in scfg["NUM_CHANNELS"]]
            setattr(self, f"transition{s - 1}", self._transition(pre, cur))
            stage, pre = self._stage(scfg, block, cur, multi_scale_output=(s != 4))
            setattr(self, f"stage{s}", stage)
            self.stage_cfgs.append(scfg)
        self.pre_stage_channels = pre
        k = extra["FINAL_CONV_KERNEL"]
        self.final_layer = _conv(pre[0], cfg["MODEL"]["NUM_JOINTS"], k, 1, 1 if k == 3 else 0, bias=True)

    @staticmethod
    def _transition(pre: Sequence[int], cur: Sequence[int]) -> nn.ModuleList:
        layers: List[nn.Module | None] = []
        for i, c in enumerate(cur):
            if i < len(pre):
                layers.append(_seq_conv_bn(pre[i], c, 3, 1, 1, relu=True) if c != pre[i] else None)
            else:
                n_new = i + 1 - len(pre)
                steps = [_seq_conv_bn(pre[-1], c if j == n_new - 1 else pre[-1], 3, 2, 1, relu=True)
                         for j in range(n_new)]
                layers.append(nn.Sequential(*steps))
        return nn.ModuleList(layers)

    @staticmethod
    def _stage(scfg, block, inch, multi_scale_output=True):
        mods = []
        n = scfg["NUM_MODULES"]
        for i in range(n):
            mso = multi_scale_output or i != n - 1
            m = HighResolutionModule(scfg["NUM_BRANCHES"], block, scfg["NUM_BLOCKS"], inch,
                                     scfg["NUM_CHANNELS"], mso)
            inch = m.num_inchannels
            mods.append(m)
        return nn.Sequential(*mods), inch

    def freeze_weight(self):
        """reference model/HRNet.py:154-158"""
        for p in self.parameters():
            p.requires_grad = False


# ----------------------------------------------------------------------------------------------
# ConvTransformer (reference model/ConvVideoTransformer.py, model/blocks.py)
# ----------------------------------------------------------------------------------------------
class LayerNorm(_Container):
    """Channel LayerNorm over (B, C, T); weight/bias are (1, C, 1) (reference model/blocks.py:67-93)."""

    def __init__(self, num_channels, eps=1e-5):
        super().__init__()
        self.num_channels = num_channels
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(1, num_channels, 1))
        self.bias = nn.Parameter(torch.zeros(1, num_channels, 1))


class AffineDropPath(_Container):
    """Per-channel residual scale (+ stochastic depth in training) (reference model/blocks.py:283-298)."""

    def __init__(self, num_dim, drop_prob=0.0, init_scale_value=1e-4):
        super().__init__()
        self.scale = nn.Parameter(init_scale_value * torch.ones(1, num_dim, 1))
        self.drop_prob = drop_prob


class MaskedMHCA(_Container):
    """Depthwise-conv + channel-attention parameters (reference model/blocks.py:336-396)."""

    def __init__(self, n_embd, n_head, n_qx_stride=1, n_kv_stride=1, attn_pdrop=0.0, proj_pdrop=0.0):
        super().__init__()
        assert n_embd % n_head == 0
        self.n_embd, self.n_head = n_embd, n_head
        self.n_channels = n_embd // n_head
        self.scale = 1.0 / math.sqrt(self.n_channels)
        self.n_qx_stride, self.n_kv_stride = n_qx_stride, n_kv_stride
        self.attn_pdrop, self.proj_pdrop = attn_pdrop, proj_pdrop

        def dw(stride_src):
            ks = stride_src + 1 if stride_src > 1 else 3
            return nn.Conv1d(n_embd, n_embd, ks, stride=n_kv_stride, padding=ks // 2, groups=n_embd, bias=False)

        self.query_conv = dw(n_qx_stride)
        self.query_norm = LayerNorm(n_embd)
        self.key_conv = dw(n_kv_stride)
        self.key_norm = LayerNorm(n_embd)
        self.value_conv = dw(n_kv_stride)
        self.value_norm = LayerNorm(n_embd)
        self.key = nn.Conv1d(n_embd, n_embd, 1)
        self.query = nn.Conv1d(n_embd, n_embd, 1)
        self.value = nn.Conv1d(n_embd, n_embd, 1)
        self.proj = nn.Conv1d(n_embd, n_embd, 1)


LOCAL_WINDOW_MIN, LOCAL_WINDOW_MAX = 5, 33          # the windows csrc/localattn.hip is built for (w = window // 2 = 2 .. 16)


def check_local_window(window_size, what="window_size"):
    """Raise ``ValueError`` unless ``window_size`` is one the local attention supports: odd, 5 .. 33.  (The reference's own
    chunking fails at 3 - blocks.py:710 slices an empty range - and with an even size its ``rel_pe`` no longer matches the
    band.)"""
    if not isinstance(window_size, (int, np.integer)) or isinstance(window_size, bool):
        raise ValueError(f"{what} must be an int, got {window_size!r}")
    if window_size % 2 == 0 or not LOCAL_WINDOW_MIN <= window_size <= LOCAL_WINDOW_MAX:
        raise ValueError(f"{what} must be odd and in [{LOCAL_WINDOW_MIN}, {LOCAL_WINDOW_MAX}], got {window_size}")


def check_local_length(t, window_size, what="sequence length"):
    """Raise ``ValueError`` unless ``t`` tokens divide into the reference's chunks of ``2 * (window_size // 2)``
    (blocks.py:667)."""
    if t <= 0 or t % (window_size - 1):
        raise ValueError(f"{what} {t} is not a multiple of {window_size - 1} (local attention window {window_size})")


class LocalMaskedMHCA(MaskedMHCA):
    """Depthwise-conv + local-window attention parameters (reference model/blocks.py:479-583): the front end and the
    projection of :class:`MaskedMHCA` under the same names, plus ``rel_pe`` (1, 1, n_head, window_size) when ``use_rel_pe``.
    Every token attends to the ``window_size`` positions centred on it (csrc/localattn.hip)."""

    def __init__(self, n_embd, n_head, window_size, n_qx_stride=1, n_kv_stride=1, attn_pdrop=0.0, proj_pdrop=0.0,
                 use_rel_pe=False):
        check_local_window(window_size)
        super().__init__(n_embd, n_head, n_qx_stride, n_kv_stride, attn_pdrop, proj_pdrop)
        self.window_size = int(window_size)
        self.window_overlap = self.window_size // 2
        self.use_rel_pe = bool(use_rel_pe)
        if self.use_rel_pe:
            self.rel_pe = nn.Parameter(torch.zeros(1, 1, n_head, self.window_size))
            std = (2.0 / n_embd) ** 0.5
            nn.init.trunc_normal_(self.rel_pe, std=std, a=-2 * std, b=2 * std)


class _Marker(_Container):
    """Parameter-free slot (GELU / Dropout positions inside the reference's mlp Sequential)."""


class TransformerBlock(_Container):
    """reference model/blocks.py:191-262; ``mha_win_size > 1`` selects :class:`LocalMaskedMHCA` (blocks.py:212-231)."""

    def __init__(self, n_embd, n_head, n_ds_strides=(1, 1), attn_pdrop=0.0, proj_pdrop=0.0, path_pdrop=0.0,
                 mha_win_size=-1, use_rel_pe=False):
        super().__init__()
        self.stride = n_ds_strides[0]
        self.ln1 = LayerNorm(n_embd)
        self.ln2 = LayerNorm(n_embd)
        if mha_win_size > 1:
            self.attn = LocalMaskedMHCA(n_embd, n_head, mha_win_size, n_ds_strides[0], n_ds_strides[1], attn_pdrop, proj_pdrop,
                                        use_rel_pe)
        else:
            self.attn = MaskedMHCA(n_embd, n_head, n_ds_strides[0], n_ds_strides[1], attn_pdrop, proj_pdrop)
        self.pool_skip = _Marker()
        self.mlp = nn.Sequential(nn.Conv1d(n_embd, 4 * n_embd, 1), _Marker(), _Marker(),
                                 nn.Conv1d(4 * n_embd, n_embd, 1), _Marker())
        self.proj_pdrop, self.path_pdrop = proj_pdrop, path_pdrop
        if path_pdrop > 0.0:
            self.drop_path_attn = AffineDropPath(n_embd, path_pdrop)
            self.drop_path_mlp = AffineDropPath(n_embd, path_pdrop)
        else:
            self.drop_path_attn = _Marker()
            self.drop_path_mlp = _Marker()


def sinusoid_table(n_position: int, d_hid: int) -> torch.Tensor:
    """(1, d_hid, n_position) float32 table, evaluated in float64 like reference model/blocks.py:114-125."""
    pos = np.arange(n_position, dtype=np.float64)[:, None]
    hid = np.arange(d_hid)[None, :]
    angle = pos / np.power(10000.0, 2.0 * (hid // 2) / d_hid)
    table = np.where(hid % 2 == 0, np.sin(angle), np.cos(angle))
    return torch.from_numpy(table.astype(np.float32)).unsqueeze(0).transpose(1, 2).contiguous()


CONV_EMBD_KS = (1, 3, 5)                            # the kernel sizes csrc/convembd.hip is built for
CONV_EMBD_MAX_CHANNELS = 256


def check_conv_embd(n_in, n_embd, ks, layers, what="ConvTransformer"):
    """Raise ``ValueError`` unless ``layers`` conv embedding layers ``n_in -> n_embd`` with ``ks x ks`` kernels are ones the
    conv embedding supports; without a layer nothing maps ``n_in`` to ``n_embd``, so the two must be equal (the reference
    fails later, in the first block's LayerNorm)."""
    for name, v in (("n_in", n_in), ("n_embd", n_embd), ("arch[0]", layers)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
            raise ValueError(f"{what}: {name} must be an int, got {v!r}")
    if layers < 0:
        raise ValueError(f"{what}: the number of conv embedding layers must be >= 0, got {layers}")
    if layers == 0:
        if n_in != n_embd:
            raise ValueError(f"{what}: n_in {n_in} != n_embd {n_embd} needs at least one conv embedding layer (arch[0] > 0)")
        return
    if isinstance(ks, bool) or not isinstance(ks, (int, np.integer)) or ks not in CONV_EMBD_KS:
        raise ValueError(f"{what}: the conv embedding kernel size must be one of {CONV_EMBD_KS}, got {ks!r}")
    if not (1 <= n_in <= CONV_EMBD_MAX_CHANNELS and 1 <= n_embd <= CONV_EMBD_MAX_CHANNELS):
        raise ValueError(f"{what}: the conv embedding takes 1 .. {CONV_EMBD_MAX_CHANNELS} channels, got {n_in} -> {n_embd}")


class ConvTransformer(_Container):
    """reference model/ConvVideoTransformer.py:21-111.  ``arch[0]`` conv embedding layers in front of the stem (:60-78): ``embd[i]``
    a ``ks x ks`` Conv2d over the (h, w) token grid (bias only without the norm), ``embd_norm[i]`` the channel LayerNorm
    (``with_ln``; nn.Identity otherwise), then a ReLU (csrc/convembd.hip)."""

    def __init__(self, n_in, n_embd, n_head, n_embd_ks, max_len, arch, h=72, scale_factor=2,
                 attn_pdrop=0.0, proj_pdrop=0.0, path_pdrop=0.0, mha_win_size=-1, use_rel_pe=False, with_ln=True):
        super().__init__()
        if len(arch) != 3:
            raise ValueError(f"ConvTransformer: arch is (embedding layers, stem blocks, branch blocks), got {arch!r}")
        check_conv_embd(n_in, n_embd, n_embd_ks, arch[0])
        self.n_in, self.n_embd_ks, self.with_ln, self.h = n_in, int(n_embd_ks), bool(with_ln), h
        self.arch, self.max_len, self.n_embd, self.n_head = tuple(arch), max_len, n_embd, n_head
        self.scale_factor = scale_factor
        # local attention window per pyramid level: [0] the stem, [1 + i] branch i (ConvVideoTransformer.py:29,48-49,89,104);
        # entries <= 1 mean channel attention
        if isinstance(mha_win_size, (int, np.integer)):
            mha_win_size = [int(mha_win_size)] * (arch[2] + 1)
        self.mha_win_size = [int(s) for s in mha_win_size]
        if len(self.mha_win_size) < arch[2] + 1:
            raise ValueError(f"mha_win_size needs {arch[2] + 1} entries (stem + {arch[2]} branch levels), got {self.mha_win_size}")
        self.use_rel_pe = bool(use_rel_pe)
        self.register_buffer("pos_embd", sinusoid_table(max_len, n_embd) / (n_embd ** 0.5))
        self.embd = nn.ModuleList()
        self.embd_norm = nn.ModuleList()
        for i in range(arch[0]):
            self.embd.append(_conv(n_in if i == 0 else n_embd, n_embd, self.n_embd_ks, 1, self.n_embd_ks // 2,
                                   bias=not self.with_ln))
            self.embd_norm.append(LayerNorm(n_embd) if self.with_ln else nn.Identity())
        kw = dict(attn_pdrop=attn_pdrop, proj_pdrop=proj_pdrop, path_pdrop=path_pdrop, use_rel_pe=use_rel_pe)
        self.stem = nn.ModuleList([TransformerBlock(n_embd, n_head, (1, 1), mha_win_size=self.mha_win_size[0], **kw)
                                   for _ in range(arch[1])])
        self.branch = nn.ModuleList(
            [TransformerBlock(n_embd, n_head, (scale_factor, scale_factor), mha_win_size=self.mha_win_size[1 + i], **kw)
             for i in range(arch[2])])
        self.upsample = nn.ModuleList([_Marker() for _ in range(arch[2])])


# ----------------------------------------------------------------------------------------------
# RSB heads (reference model/RSB.py)
# ----------------------------------------------------------------------------------------------
class conv_bn_relu(_Container):  # noqa: N801 - reference class name
    def __init__(self, in_planes, out_planes, kernel_size, stride, padding, has_bn=True, has_relu=True, efficient=False, groups=1):
        super().__init__()
        # ``efficient`` is the reference's activation checkpointing (RSB.py:134-135): accepted, nothing to do here
        self.conv = nn.Conv2d(in_planes, out_planes, kernel_size, stride, padding, groups=groups)  # bias=True
        self.bn = nn.BatchNorm2d(out_planes)
        self.has_bn, self.has_relu = has_bn, has_relu


_RSB_STEPS = ("1_1", "2_1", "2_2", "3_1", "3_2", "3_3", "4_1", "4_2", "4_3", "4_4")


class RSB_BLOCK(_Container):  # noqa: N801
    expansion = 1

    def __init__(self, in_planes, planes, stride=1, downsample=None):
        super().__init__()
        self.branch_ch = in_planes * 26 // 64
        bc = self.branch_ch
        self.conv_bn_relu1 = conv_bn_relu(in_planes, 4 * bc, 1, stride, 0)
        for s in _RSB_STEPS:
            setattr(self, f"conv_bn_relu2_{s}", conv_bn_relu(bc, bc, 3, 1, 1))
        self.conv_bn_relu3 = conv_bn_relu(4 * bc, planes, 1, 1, 0, has_relu=False)
        self.downsample = downsample


class CHAIN_RSB_BLOCKS(_Container):  # noqa: N801
    def __init__(self, in_planes, out_planes, num_blocks):
        super().__init__()
        down = conv_bn_relu(in_planes, out_planes, 1, 1, 0, has_relu=False)
        blocks = [RSB_BLOCK(in_planes, out_planes, 1, downsample=down)]
        blocks += [RSB_BLOCK(out_planes, out_planes, 1) for _ in range(1, num_blocks)]
        self.layers = nn.Sequential(*blocks)


PRM_MAX_CHANNELS = 64                               # what csrc/prm.hip takes (otp_prm_supported)


def check_prm_channels(c, what):
    """Raise ``ValueError`` unless ``c`` is a channel count the PRM kernels take."""
    if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 1 <= c <= PRM_MAX_CHANNELS:
        raise ValueError(f"{what}: the channel count must be an int in 1 .. {PRM_MAX_CHANNELS}, got {c!r}")


class RSN_WEIGHT_VECTOR(_Container):  # noqa: N801
    """reference model/RSB.py:142-165: 3x3 conv-BN-ReLU, global average pool, two 1x1 conv-BN-ReLU with an inner residual, sigmoid
    -> (N, C, 1, 1) (``ops.rsn_weight_vector``, csrc/prm.hip)."""

    def __init__(self, input_chn_num, output_chl_num):
        super().__init__()
        check_prm_channels(output_chl_num, "RSN_WEIGHT_VECTOR")
        self.input_chm_num, self.output_chl_num = input_chn_num, output_chl_num
        c = output_chl_num
        self.conv_bn_relu_1 = conv_bn_relu(input_chn_num, c, 3, 1, 1)
        self.conv_bn_relu_2 = conv_bn_relu(c, c, 1, 1, 0)
        self.conv_bn_relu_3 = conv_bn_relu(c, c, 1, 1, 0)


class RSN_ATTENTION(_Container):  # noqa: N801
    """reference model/RSB.py:168-203, RSN's Pose Refine Machine: f = 3x3 conv-BN-ReLU; a channel gate (global average pool, two
    1x1 conv-BN-ReLU, sigmoid); a spatial gate (1x1 conv-BN-ReLU, depthwise 9x9 conv-BN-ReLU, sigmoid); f (1 + gate_c gate_s)
    (``ops.rsn_attention``, csrc/prm.hip)."""

    def __init__(self, output_chl_num, efficient=False):
        super().__init__()
        check_prm_channels(output_chl_num, "RSN_ATTENTION")
        self.output_chl_num = c = output_chl_num
        self.conv_bn_relu_prm_1 = conv_bn_relu(c, c, 3, 1, 1)
        self.conv_bn_relu_prm_2_1 = conv_bn_relu(c, c, 1, 1, 0)
        self.conv_bn_relu_prm_2_2 = conv_bn_relu(c, c, 1, 1, 0)
        self.conv_bn_relu_prm_3_1 = conv_bn_relu(c, c, 1, 1, 0)
        self.conv_bn_relu_prm_3_2 = conv_bn_relu(c, c, 9, 1, 4, groups=c)


# ----------------------------------------------------------------------------------------------
# DETR-style token encoder (reference model/OTPose.py:26-159): unlike the containers above these two
# modules can run themselves on the library's launches (the training graph calls forward_cm); inside
# OTPose in eval mode the inference engine emits their launches (InferenceEngine.token_encoder)
# ----------------------------------------------------------------------------------------------
class _SelfAttnParams(nn.Module):
    """The parameters of ``nn.MultiheadAttention(E, nhead)`` under its names: ``in_proj_weight`` (3E, E), ``in_proj_bias`` (3E),
    ``out_proj.weight`` (E, E), ``out_proj.bias`` (E), with its initialisation (xavier-uniform in-projection, zero biases)."""

    def __init__(self, d_model):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * d_model, d_model))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * d_model))
        self.out_proj = nn.Linear(d_model, d_model)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.out_proj.bias)


def _pointwise(x, weight, bias):
    """``F.linear`` over the channel axis of (N, Cin, L) as a 1x1 convolution launch (``train_ops.conv2d``: forward and backward
    in HIP) -> (N, Cout, L)."""
    from . import train_ops as T
    n, c, length = x.shape
    return T.conv2d(x.reshape(n, c, 1, length), weight.reshape(weight.shape[0], c, 1, 1), bias).reshape(n, weight.shape[0], length)


class TransformerEncoderLayer(nn.Module):
    """reference model/OTPose.py:84-159 with its constructor signature, ``state_dict`` keys and ``forward`` on sequence-first
    (L, N, E) tensors.  Inside, the layer works channel-major on (N, E, L) (:meth:`forward_cm`): the in-projection, the
    out-projection and the two FFN linears are 1x1 convolutions (``train_ops.conv2d``, exact fp32: the scores feed an exp, so
    the split-product route of the C -> C layers is switched off for this module), the two LayerNorms the channel LayerNorm
    (``train_ops.layer_norm``, eps 1e-5, biased variance, as ``nn.LayerNorm(E)``), GELU ``train_ops.gelu``, the attention core
    ``token_attn`` (csrc/tokattn.hip).  Residual adds, the ``pos`` add, ReLU and dropout are PyTorch element-wise operators.

    Deviations, each raising: a dense ``src_mask`` -> ``NotImplementedError``; ``activation`` is ``relu`` or ``gelu`` (``glu``
    halves the width in the reference and then fails in ``linear2``) -> ``ValueError``.  ``dropout`` acts at the reference's three
    ``nn.Dropout`` places only, and the constructor argument ``attn_dropout`` must stay 0 (``ValueError``; the reference hands
    ``dropout`` to ``nn.MultiheadAttention`` as well).  Attention-probability dropout is switched on for a built layer with
    :meth:`set_attn_dropout` (what ``OTPose`` does for ``MODEL.TOKEN_ATTN_DROPOUT``): it is applied inside ``token_attn`` when the
    layer runs stochastically, with this library's own counter-based mask (otpose_amd/attn_dropout.py), not PyTorch's.
    With ``return_atten_map`` the map comes from ``token_attn_map``: no gradient, and the undropped probabilities.
    :meth:`set_products` (``"f32"``, the default, or ``"half"``; ``OTPose``: ``MODEL.TOKEN_PRODUCTS``) chooses the arithmetic of the
    attention products, ``token_attn``'s ``products``; the attribute ``products`` is no parameter and adds no ``state_dict`` key."""

    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation="gelu", normalize_before=False,
                 return_atten_map=False, attn_dropout=0.0):
        super().__init__()
        from .token_attn import MAX_HEAD_WIDTH
        for name, val in (("d_model", d_model), ("nhead", nhead), ("dim_feedforward", dim_feedforward)):
            if isinstance(val, bool) or not isinstance(val, (int, np.integer)) or val < 1:
                raise ValueError(f"TransformerEncoderLayer: {name} must be a positive int, got {val!r}")
        if d_model % nhead or d_model // nhead > MAX_HEAD_WIDTH:
            raise ValueError(f"TransformerEncoderLayer: nhead = {nhead} must divide d_model = {d_model} into heads of at most "
                             f"{MAX_HEAD_WIDTH} channels")
        if activation not in ("relu", "gelu"):
            raise ValueError(f"TransformerEncoderLayer: activation must be 'relu' or 'gelu', got {activation!r}")
        if attn_dropout != 0.0:
            raise ValueError("TransformerEncoderLayer: attn_dropout must be 0 at construction; attention-probability dropout is "
                             "set on a built layer with set_attn_dropout(p)")
        self.attn_dropout = 0.0
        self.products = "f32"
        self.self_attn = _SelfAttnParams(d_model)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.d_model, self.nhead, self.p_drop, self.activation = d_model, nhead, float(dropout), activation
        self.normalize_before, self.return_atten_map = normalize_before, return_atten_map

    def set_attn_dropout(self, p):
        """Attention-probability dropout rate of this layer, a float in [0, 1) (``ValueError`` otherwise); returns the layer."""
        from .attn_dropout import check_rate
        self.attn_dropout = check_rate(p, "TransformerEncoderLayer: attn_dropout")
        return self

    def set_products(self, mode):
        """Arithmetic of this layer's attention products: ``"f32"`` (default, exact) or ``"half"`` (``token_attn``'s
        ``products``; what ``OTPose`` does for ``MODEL.TOKEN_PRODUCTS``); ``ValueError`` otherwise; returns the layer."""
        from .token_attn import check_products
        self.products = check_products(mode, "TransformerEncoderLayer: products")
        return self

    def _drop(self, x):
        return torch.nn.functional.dropout(x, self.p_drop, True) if self._stochastic and self.p_drop > 0 else x

    def _norm(self, norm, x):
        from . import train_ops as T
        return T.layer_norm(x, norm.weight, norm.bias, norm.eps)

    def _attention(self, qk, value, mask):
        """q = k from ``qk``, v from ``value`` (both (N, E, L)) -> (attention output after the out-projection, map or None)."""
        from .token_attn import token_attn, token_attn_map
        e, a = self.d_model, self.self_attn
        w, b = a.in_proj_weight, a.in_proj_bias
        q = _pointwise(qk, w[:e], b[:e])
        k = _pointwise(qk, w[e:2 * e], b[e:2 * e])
        v = _pointwise(value, w[2 * e:], b[2 * e:])
        scale = 1.0 / math.sqrt(e // self.nhead)
        p_attn = self.attn_dropout if self._stochastic else 0.0
        out = _pointwise(token_attn(q, k, v, self.nhead, scale, mask, dropout_p=p_attn, products=getattr(self, "products", "f32")),
                         a.out_proj.weight, a.out_proj.bias)
        amap = token_attn_map(q.detach(), k.detach(), self.nhead, scale, mask) if self.return_atten_map else None
        return out, amap

    def _ffn(self, x):
        from . import train_ops as T
        h = _pointwise(x, self.linear1.weight, self.linear1.bias)
        h = T.gelu(h) if self.activation == "gelu" else torch.relu(h)
        return _pointwise(self._drop(h), self.linear2.weight, self.linear2.bias)

    def forward_cm(self, x, mask=None, pos=None, stochastic=None):
        """The layer on channel-major tensors: ``x`` (N, E, L), ``pos`` None or broadcastable to it, ``mask`` (N, L) bool
        (True = padding) -> (output (N, E, L), attention map (N, L, L) or None).  The reference's forward_post / forward_pre."""
        import dataclasses
        from . import train_ops as T
        self._stochastic = self.training if stochastic is None else bool(stochastic)   # dropout on (the training graph decides)
        with T.active_routes(dataclasses.replace(T.current_routes(), use_x3=False)):
            if self.normalize_before:
                y = self._norm(self.norm1, x)
                a, amap = self._attention(y if pos is None else (y + pos).contiguous(), x, mask)
                x = x + self._drop(a)
                return x + self._drop(self._ffn(self._norm(self.norm2, x))), amap
            a, amap = self._attention(x if pos is None else (x + pos).contiguous(), x, mask)
            x = self._norm(self.norm1, x + self._drop(a))
            return self._norm(self.norm2, x + self._drop(self._ffn(x))), amap

    def forward(self, src, src_mask=None, src_key_padding_mask=None, pos=None):
        out, amap = _encoder_forward([self], None, False, src, src_mask, src_key_padding_mask, pos)
        return (out, amap[0]) if self.return_atten_map else out


def _encoder_forward(layers, norm, pe_only_at_begin, src, mask, key_padding_mask, pos):
    """(L, N, E) -> (N, E, L) once, the layers, the optional final LayerNorm, and back once; ``pos`` (L, 1 or N, E) likewise."""
    if mask is not None:
        raise NotImplementedError("TransformerEncoder: a dense attention mask (attn_mask, L x L) is not built; "
                                  "use src_key_padding_mask")
    if src.dim() != 3:
        raise ValueError(f"TransformerEncoder: src is (L, N, E), got {tuple(src.shape)}")
    x = src.permute(1, 2, 0).contiguous()
    p = None if pos is None else pos.permute(1, 2, 0).contiguous()
    maps = []
    for layer in layers:
        x, amap = layer.forward_cm(x, key_padding_mask, p)
        maps.append(amap)
        if pe_only_at_begin:
            p = None
    if norm is not None:
        from . import train_ops as T
        x = T.layer_norm(x, norm.weight, norm.bias, norm.eps)
    return x.permute(2, 0, 1).contiguous(), maps


class TransformerEncoder(nn.Module):
    """reference model/OTPose.py:26-66: ``num_layers`` deep copies of ``encoder_layer``, an optional final ``norm``
    (``nn.LayerNorm(E)``), xavier-uniform on every parameter of more than one dimension.  ``forward`` moves to (N, E, L) once at
    entry and back once at exit; with ``return_atten_map`` it also returns the (layers, N, L, L) stack of maps."""

    def __init__(self, encoder_layer, num_layers, norm=None, pe_only_at_begin=False, return_atten_map=False):
        super().__init__()
        import copy
        if not isinstance(encoder_layer, TransformerEncoderLayer):
            raise ValueError("TransformerEncoder: encoder_layer must be a modules.TransformerEncoderLayer")
        if isinstance(num_layers, bool) or not isinstance(num_layers, (int, np.integer)) or num_layers < 1:
            raise ValueError(f"TransformerEncoder: num_layers must be a positive int, got {num_layers!r}")
        if norm is not None and not isinstance(norm, nn.LayerNorm):
            raise ValueError("TransformerEncoder: norm must be None or an nn.LayerNorm")
        self.layers = nn.ModuleList([copy.deepcopy(encoder_layer) for _ in range(num_layers)])
        self.num_layers, self.norm = num_layers, norm
        self.pe_only_at_begin, self.return_atten_map = pe_only_at_begin, return_atten_map
        for layer in self.layers:
            layer.return_atten_map = return_atten_map
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def forward(self, src, mask=None, src_key_padding_mask=None, pos=None):
        out, maps = _encoder_forward(self.layers, self.norm, self.pe_only_at_begin, src, mask, src_key_padding_mask, pos)
        return (out, torch.stack(maps)) if self.return_atten_map else out
