"""``OTPose`` - drop-in for reference model/OTPose.py:180 behind the HIP engine.

Constructor, ``forward(x, margin=...)`` signature, 7-tuple output order and ``state_dict`` key set
follow reference model/OTPose.py:181-257, 307-394.  The forward itself is a sequence of launches
into the C-ABI library declared in include/otpose_hip.h (see :mod:`otpose_amd.engine`); there is
no PyTorch-op or CPU fallback: without a GPU or without the built library the call raises.
"""
from __future__ import annotations

import logging
import math
import os

import torch
from torch import nn

from .modules import (CHAIN_RSB_BLOCKS, RSN_ATTENTION, ConvTransformer, HRNet, TransformerEncoder, TransformerEncoderLayer,
                      _Container)
from .token_attn import sine_position_embedding
from . import ops


class ModulatedDeformConv(nn.Module):
    """Modulated deformable convolution module (reference
    thirdparty/deform_conv/modules/deform_conv.py:85-131): owns ``weight`` (Cout, Cin/groups, kh, kw)
    and ``bias`` (Cout); ``forward(x, offset, mask)`` calls the HIP operator."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1,
                 groups=1, deformable_groups=1, bias=True):
        super().__init__()
        ks = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, ks
        self.stride, self.padding, self.dilation = stride, padding, dilation
        self.groups, self.deformable_groups, self.with_bias = groups, deformable_groups, bias
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, *ks))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        n = self.in_channels * self.kernel_size[0] * self.kernel_size[1]
        bound = n ** -0.5
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)
            if self.bias is not None:
                self.bias.zero_()

    def forward(self, x, offset, mask):
        return ops.modulated_deform_conv(x, offset, mask, self.weight, self.bias, self.stride,
                                         self.padding, self.dilation, self.groups, self.deformable_groups)


class DeformConv(nn.Module):
    """DCN v1 module (reference thirdparty/deform_conv/modules/deform_conv.py:10-60): no mask, no bias."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 deformable_groups=1, bias=False):
        super().__init__()
        assert not bias
        assert in_channels % groups == 0 and out_channels % groups == 0
        k = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, k
        self.stride, self.padding, self.dilation = stride, padding, dilation
        self.groups, self.deformable_groups = groups, deformable_groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, *k))
        stdv = 1.0 / math.sqrt(in_channels * k[0] * k[1])
        with torch.no_grad():
            self.weight.uniform_(-stdv, stdv)

    def forward(self, x, offset):
        from . import ops
        return ops.deform_conv(x, offset, self.weight, self.stride, self.padding, self.dilation, self.groups,
                               self.deformable_groups)


class DeformableCONV(nn.Module):
    """reference model/layers.py:22-29: 3x3 modulated DCN, one deformable group per joint."""

    def __init__(self, num_joints, k, dilation):
        super().__init__()
        self.deform_conv = ModulatedDeformConv(num_joints, num_joints, (k, k), stride=1,
                                               padding=(k // 2) * dilation, dilation=dilation,
                                               deformable_groups=num_joints)

    def forward(self, x, offsets, mask):
        return self.deform_conv(x, offsets, mask)


def _host(x):
    """A tensor's values as a host numpy array (other array-likes pass through): the crop matrices are built on the host."""
    return x.detach().cpu().numpy() if torch.is_tensor(x) else x


# TRAIN.* of the reference's PoseTrack18 config (configs/Base_PoseTrack18.yaml), for cfgs that do not set them
_TRAIN_AUGMENT = {"SCALE_FACTOR": 0.35, "ROT_FACTOR": 45, "FLIP": True, "PROB_HALF_BODY": 0.3, "NUM_JOINTS_HALF_BODY": 8}


def _train_augment_cfg(cfg):
    """The keyword arguments of augment.sample_augmentation from ``cfg.TRAIN``."""
    t = {k: cfg.get("TRAIN", {}).get(k, v) for k, v in _TRAIN_AUGMENT.items()}
    return {"scale_factor": t["SCALE_FACTOR"], "rotation_factor": t["ROT_FACTOR"], "flip": bool(t["FLIP"]),
            "prob_half_body": t["PROB_HALF_BODY"], "num_joints_half_body": t["NUM_JOINTS_HALF_BODY"]}


def _plain_conv(cin, cout, dilation):
    return nn.Conv2d(cin, cout, 3, 1, padding=dilation, dilation=dilation, bias=False)


class OTPose(nn.Module):
    def __init__(self, cfg, **kwargs):
        super().__init__()
        self.logger = logging.getLogger(__name__)
        self.cfg = cfg
        m = cfg.MODEL
        extra = cfg["MODEL"]["EXTRA"]
        # frames per clip window: 5 in the reference (OTPose.py:309,320-321); 7 = the BASELINE configs[4] extension
        self.window_frames = int(m.get("WINDOW_FRAMES", 5)) if hasattr(m, "get") else 5
        if self.window_frames not in (5, 7):
            raise ValueError("MODEL.WINDOW_FRAMES must be 5 (reference) or 7 (extension)")
        self.num_frames = 8 if self.window_frames == 5 else 12    # feature maps stacked per joint (OTPose.py:188)
        self.pe_w, self.pe_h = m.HEATMAP_SIZE
        self.num_joints = m.NUM_JOINTS
        self.num_patches = self.pe_h * self.pe_w
        self.patch_dim = self.num_joints
        self.temporal_encoding_dim = self.patch_dim * self.num_frames
        self.freeze_hrnet_weights = m.FREEZE_HRNET_WEIGHTS
        self.pretrained = m.PRETRAINED
        self.pretrained_layers = extra["PRETRAINED_LAYERS"]

        self.rough_pose_estimation_net = HRNet(cfg)
        self.scale_arch, self.flow_scale_arch = (0, 6, 2), (0, 6, 0)
        tkw = dict(n_embd_ks=3, max_len=self.num_patches, h=self.pe_h, proj_pdrop=0.1, path_pdrop=0.1)
        d = self.temporal_encoding_dim
        # extension keys (the reference's OTPose.py:209-216 builds its encoders without a window): MODEL.MHA_WIN_SIZE / MODEL.USE_REL_PE
        # for the two temporal encoders, MODEL.FLOW_MHA_WIN_SIZE for the flow encoder; absent or <= 1 = channel attention
        get = m.get if hasattr(m, "get") else (lambda k, dflt: getattr(m, k, dflt))
        rel = bool(get("USE_REL_PE", False))
        win = self._local_windows(get("MHA_WIN_SIZE", -1), self.scale_arch, "MODEL.MHA_WIN_SIZE")
        fwin = self._local_windows(get("FLOW_MHA_WIN_SIZE", -1), self.flow_scale_arch, "MODEL.FLOW_MHA_WIN_SIZE")
        # extension keys: conv embedding layers in front of the encoders (ConvVideoTransformer.py:60-78; the reference builds its
        # encoders with arch[0] = 0): MODEL.EMBD_LAYERS for the two temporal encoders, MODEL.FLOW_EMBD_LAYERS for the flow encoder,
        # MODEL.EMBD_KS / MODEL.EMBD_WITH_LN for all three
        ekw = self._embd_keys(get, d)
        # extension keys, training only (the inference engines read none of them: eval is the identity): attention-probability
        # dropout, which the reference's blocks take as attn_pdrop (blocks.py:392,572) and its OTPose.py:209-216 leaves at 0 -
        # MODEL.ATTN_PDROP for the two temporal encoders, MODEL.FLOW_ATTN_PDROP for the flow encoder, MODEL.TOKEN_ATTN_DROPOUT
        # for the token encoders (what OTPose.py:93 hands to nn.MultiheadAttention); all 0.0 by default
        pdrop, flow_pdrop, token_pdrop = (self._rate_key(get, k) for k in ("ATTN_PDROP", "FLOW_ATTN_PDROP", "TOKEN_ATTN_DROPOUT"))
        # the training graph passes a rate to the channel attention only (TrainGraph.attention): a windowed encoder with one could
        # not take its first training step, so the pair of keys is refused here, by name
        for key, rate, wkey, windows in (("ATTN_PDROP", pdrop, "MHA_WIN_SIZE", win), ("FLOW_ATTN_PDROP", flow_pdrop, "FLOW_MHA_WIN_SIZE", fwin)):
            if rate > 0.0 and windows is not None:
                raise ValueError(f"MODEL.{key} = {rate} with MODEL.{wkey} = {windows}: the training graph does not drop the "
                                 "probabilities of the local-window attention (train_ops.local_attn takes dropout_p; "
                                 "TrainGraph.attention does not pass it)")
        if ekw:
            self.scale_arch = (ekw.pop("layers"),) + self.scale_arch[1:]
            self.flow_scale_arch = (ekw.pop("flow_layers"),) + self.flow_scale_arch[1:]
            tkw.update(ekw)
        self.temporal_encoder1 = ConvTransformer(d, d, n_head=2, arch=self.scale_arch, attn_pdrop=pdrop, **tkw,
                                                 **self._local_kw(win, rel))
        self.temporal_encoder2 = ConvTransformer(d, d, n_head=2, arch=self.scale_arch, attn_pdrop=pdrop, **tkw,
                                                 **self._local_kw(win, rel))
        self.flow_encoder = ConvTransformer(self.patch_dim, self.patch_dim, n_head=1, arch=self.flow_scale_arch,
                                            attn_pdrop=flow_pdrop, **tkw, **self._local_kw(fwin, False))

        # extension keys: a DETR-style TransformerEncoder (OTPose.py:26-159, exported and never called by the reference) over the
        # h w heat-map tokens in front of each ConvTransformer, on exactly the tensor the ConvTransformer is handed; all off by
        # default.  The positional tables keep the reference's names (OTPose.py:259-279).
        tk = self._token_keys(get, d)
        self.token_keys = tk
        for name, width, layers, heads, ffn in (("token_encoder1", d, tk["layers"], tk["heads"], tk["ffn"]),
                                                ("token_encoder2", d, tk["layers"], tk["heads"], tk["ffn"]),
                                                ("flow_token_encoder", self.patch_dim, tk["flow_layers"], 1, tk["flow_ffn"])):
            if layers > 0:
                layer = TransformerEncoderLayer(width, heads, ffn, dropout=0.1, activation="gelu", normalize_before=tk["pre_norm"])
                # MODEL.TOKEN_PRODUCTS: "half" puts the attention products of all three encoders on the 16-bit matrix cores
                setattr(self, name, TransformerEncoder(layer.set_attn_dropout(token_pdrop).set_products(tk["products"]), layers))
        pe, flow_pe = tk["pe"], tk["pe"]
        if flow_pe == "sine" and tk["flow_layers"] > 0:
            flow_pe = "none"                   # width 17 has no sine table (d_model % 4), in the reference either
            self.logger.info("MODEL.TOKEN_PE = 'sine': the flow token encoder runs without a positional table (width %d)",
                             self.patch_dim)
        for name, width, layers, kind in (("temporal_pos_embedding", d, tk["layers"], pe),
                                          ("flow_pos_embedding", self.patch_dim, tk["flow_layers"], flow_pe)):
            if layers > 0 and kind == "learnable":
                setattr(self, name, nn.Parameter(torch.randn(1, self.num_patches, width)))
            elif layers > 0 and kind == "sine":
                setattr(self, name, nn.Parameter(sine_position_embedding(self.pe_h, self.pe_w, width), requires_grad=False))

        self.deformable_conv_dilations = list(m.DEFORMABLE_CONV.DILATION)
        self.deformable_aggregation_type = m.DEFORMABLE_CONV.AGGREGATION_TYPE
        assert self.deformable_aggregation_type == "weighted_sum"
        fk = extra["FINAL_CONV_KERNEL"]
        levels = self.scale_arch[-1] + 1
        self.final_layer1 = nn.Conv2d(d * levels, self.num_joints, fk, 1, 1 if fk == 3 else 0)
        self.final_layer2 = nn.Conv2d(d * levels, self.num_joints, fk, 1, 1 if fk == 3 else 0)

        def_ch, n_blocks = m.DEFORMABLE_CONV_CH, m.OFFSET_MASK_COMBINE_CONV
        self.offset_mask_combine_conv = CHAIN_RSB_BLOCKS(self.num_joints * 3, def_ch, n_blocks)
        self.def_fuse = CHAIN_RSB_BLOCKS(self.num_joints, self.num_joints, n_blocks)
        # extension key MODEL.PRM: the output of a named chain goes through an RSN_ATTENTION of its channel count (RSB.py:168-203, a
        # class the reference exports and never calls); () = the reference's model
        self.prm = self._prm_keys(get("PRM", ()))
        if "def_fuse" in self.prm:
            self.def_fuse_prm = RSN_ATTENTION(self.num_joints)
        if "offset_mask_combine_conv" in self.prm:
            self.offset_mask_combine_prm = RSN_ATTENTION(def_ch)
        k, j = 3, self.num_joints
        self.offsets_list = nn.ModuleList(
            [nn.Sequential(_plain_conv(def_ch, j * 2 * k * k, dd)) for dd in self.deformable_conv_dilations])
        self.masks_list = nn.ModuleList(
            [nn.Sequential(_plain_conv(def_ch, j * k * k, dd)) for dd in self.deformable_conv_dilations])
        self.modulated_deform_conv_list = nn.ModuleList(
            [DeformableCONV(j, k, dd) for dd in self.deformable_conv_dilations])

        self._engine = None
        # eval outputs are fresh tensors (reference semantics); True returns the engine's static buffers, valid until
        # the next forward (bench.py's timed loop)
        self.alias_outputs = False
        self.init_weights()

    def _local_windows(self, value, arch, key):
        """The per-level local attention windows of an encoder of ``arch`` from cfg value ``value`` (an int for every level, or a
        sequence: [0] the stem, [1 + i] branch i), validated against the token count of every level - T, T/2, T/4 of the
        configured heat-map.  None when every level keeps the channel attention."""
        from .modules import check_local_length, check_local_window
        levels = arch[2] + 1
        sizes = list(value) if isinstance(value, (list, tuple)) else [value] * levels
        if len(sizes) < levels:
            raise ValueError(f"{key} needs {levels} entries (stem + {arch[2]} branch levels), got {sizes}")
        sizes = sizes[:levels]
        if all(s <= 1 for s in sizes):
            return None
        for i, s in enumerate(sizes):
            if s > 1:
                t = self.num_patches // 2 ** i
                check_local_window(s, f"{key}[{i}]")
                check_local_length(t if self.num_patches % 2 ** i == 0 else 0, s,
                                   f"{key}[{i}]: level {i} of the {self.pe_w}x{self.pe_h} heat-map: sequence length")
        return sizes

    @staticmethod
    def _rate_key(get, key):
        """``MODEL.<key>`` validated as a dropout rate: a float in [0, 1), 0.0 where absent."""
        from .attn_dropout import check_rate
        return check_rate(get(key, 0.0), f"MODEL.{key}")

    PRM_CHAINS = ("def_fuse", "offset_mask_combine_conv")

    @classmethod
    def _prm_keys(cls, value):
        """MODEL.PRM validated: a tuple / list of distinct names out of :attr:`PRM_CHAINS`."""
        if not isinstance(value, (tuple, list)) or any(not isinstance(v, str) or v not in cls.PRM_CHAINS for v in value) \
                or len(set(value)) != len(value):
            raise ValueError(f"MODEL.PRM must be a tuple of distinct names out of {cls.PRM_CHAINS}, got {value!r}")
        return tuple(value)

    TOKEN_PE_KINDS = ("sine", "learnable", "none")

    def _token_keys(self, get, d):
        """The token-encoder keys of the cfg, validated (also when no layer is asked for: a bad key does not wait for the day a
        layer is): layer counts, heads, FFN widths, pre-norm flag and the kind of positional table."""
        from .token_attn import MAX_HEAD_WIDTH

        def integer(key, default, low):
            v = get(key, default)
            if isinstance(v, bool) or not isinstance(v, int) or v < low:
                raise ValueError(f"MODEL.{key} must be an int of at least {low}, got {v!r}")
            return v
        layers, flow_layers = integer("TOKEN_LAYERS", 0, 0), integer("FLOW_TOKEN_LAYERS", 0, 0)
        heads = integer("TOKEN_HEADS", 2, 1)
        if d % heads or d // heads > MAX_HEAD_WIDTH:
            raise ValueError(f"MODEL.TOKEN_HEADS = {heads} must divide the token width {d} into heads of at most {MAX_HEAD_WIDTH} "
                             "channels")
        ffn, flow_ffn = integer("TOKEN_FFN", 2 * d, 1), 2 * self.patch_dim
        pre = get("TOKEN_PRE_NORM", False)
        if not isinstance(pre, bool):
            raise ValueError(f"MODEL.TOKEN_PRE_NORM must be a bool, got {pre!r}")
        pe = get("TOKEN_PE", "sine")
        if not isinstance(pe, str) or pe not in self.TOKEN_PE_KINDS:
            raise ValueError(f"MODEL.TOKEN_PE must be one of {self.TOKEN_PE_KINDS}, got {pe!r}")
        if pe == "sine" and layers > 0 and d % 4:
            raise ValueError(f"MODEL.TOKEN_PE = 'sine' needs a token width that is a multiple of 4, got {d}")
        from .token_attn import PRODUCTS
        products = get("TOKEN_PRODUCTS", "f32")
        if not isinstance(products, str) or products not in PRODUCTS:
            raise ValueError(f"MODEL.TOKEN_PRODUCTS must be one of {PRODUCTS}, got {products!r}")
        return {"layers": layers, "flow_layers": flow_layers, "heads": heads, "ffn": ffn, "flow_ffn": flow_ffn, "pre_norm": pre,
                "pe": pe, "products": products}

    def _embd_keys(self, get, d):
        """The conv embedding keys of the cfg, validated: {} at the defaults (no layer anywhere), else the layer counts and the
        ConvTransformer keyword arguments."""
        from .modules import check_conv_embd
        layers, flow_layers = get("EMBD_LAYERS", 0), get("FLOW_EMBD_LAYERS", 0)
        ks, with_ln = get("EMBD_KS", 3), get("EMBD_WITH_LN", True)
        if not isinstance(with_ln, bool):
            raise ValueError(f"MODEL.EMBD_WITH_LN must be a bool, got {with_ln!r}")
        # the kernel size is checked even when no layer is asked for: a bad key does not wait for the day a layer is
        check_conv_embd(d, d, ks, 1, "MODEL.EMBD_KS")
        check_conv_embd(d, d, ks, layers, "MODEL.EMBD_LAYERS")
        check_conv_embd(self.patch_dim, self.patch_dim, ks, flow_layers, "MODEL.FLOW_EMBD_LAYERS")
        if layers == 0 and flow_layers == 0:
            return {}
        return {"layers": int(layers), "flow_layers": int(flow_layers), "n_embd_ks": int(ks), "with_ln": with_ln}

    @staticmethod
    def _local_kw(windows, use_rel_pe):
        """ConvTransformer keyword arguments of :meth:`_local_windows`' result (none at the defaults)."""
        return {} if windows is None else {"mha_win_size": windows, "use_rel_pe": use_rel_pe}

    # ---- initialisation (reference model/OTPose.py:431-503) ---------------------------------
    def init_weights(self):
        with torch.no_grad():
            for mod in self.modules():
                if isinstance(mod, nn.Conv2d):
                    mod.weight.normal_(0.0, 0.001)
                    if mod.bias is not None:
                        mod.bias.zero_()
                elif isinstance(mod, nn.BatchNorm2d):
                    mod.weight.fill_(1.0)
                    mod.bias.zero_()
                elif isinstance(mod, ModulatedDeformConv):
                    mod.weight.zero_()
                    c = mod.kernel_size[0] // 2
                    for o in range(min(mod.weight.shape[0], mod.weight.shape[1])):
                        mod.weight[o, o, c, c] = 1.0
                    if mod.bias is not None:
                        mod.bias.zero_()
                elif isinstance(mod, nn.Conv1d) and mod.bias is not None:
                    mod.bias.zero_()
        if self.pretrained and os.path.isfile(self.pretrained):
            self._load_pretrained(self.pretrained)
        elif self.pretrained:
            raise ValueError("{} is not exist!".format(self.pretrained))
        if self.freeze_hrnet_weights:
            self.rough_pose_estimation_net.freeze_weight()

    def _load_pretrained(self, path):
        """HRNet checkpoint import with the reference's prefix remap (model/OTPose.py:477-496)."""
        sd = torch.load(path, map_location="cpu")
        sd = sd.get("state_dict", sd)
        tops = {n.split(".")[1] for n, _ in self.rough_pose_estimation_net.named_modules(prefix="r") if "." in n}
        take = {}
        for name, t in sd.items():
            head = name.split(".")[0]
            if not (head in self.pretrained_layers or self.pretrained_layers[0] == "*"):
                continue
            if head == "rough_pose_estimation_net":
                take[name] = t
            elif head in tops:
                take["rough_pose_estimation_net." + name] = t
        self.load_state_dict(take, strict=False)

    # ---- forward -------------------------------------------------------------------------------
    def forward(self, x, **kwargs):
        assert "margin" in kwargs
        margin = kwargs["margin"]
        if self.training:
            # model.train(): BatchNorm batch statistics + an autograd tape over HIP kernels (otpose_amd/train.py);
            # self.train_dropout = False switches Dropout / drop-path off (deterministic comparison with the oracle)
            from .train import forward_train
            self._engine = None
            return forward_train(self, x, margin)
        if self._engine is None or not self._engine.matches(x):
            self._engine = self._engine_class()(self, x.shape[0], x.device)
        return self._engine.run(x, margin, self.alias_outputs)

    def forward_frames(self, frames_u8, margin):
        """Eval forward from raw uint8 RGB crops (B, 5, H, W, 3) in the order cur, prev, next, pprev, nnext: the
        ToTensor + Normalize + concat of the reference data pipeline (dataset/PoseTrackDataset.py:397-406,
        script/Common.py:117) run as one HIP kernel writing the stem's input buffer."""
        if self.training:
            from . import ops
            return self.forward(ops.frames_to_clip(frames_u8), margin=margin)
        b, f, h, w, _ = frames_u8.shape
        if self._engine is None or not self._engine.matches_shape(b, 3 * f, h, w, frames_u8.device):
            self._engine = self._engine_class()(self, b, frames_u8.device)
        return self._engine.run(frames_u8, margin, self.alias_outputs)

    def forward_video(self, pool, frame_idx, center, scale, margin, rotation=None, flip=None, blur=None):
        """Forward from whole video frames: ``pool`` (S, Hp, Wp, 3) uint8 RGB frames on the GPU, ``frame_idx`` (B, F) the
        pool frame of every window slot (F = ``window_frames``, slots in the order cur, prev, next, pprev, nnext - see
        otpose_amd.crop.window), ``center`` / ``scale`` (B, 2) of each person (otpose_amd.crop.box_to_center_scale),
        ``margin`` (B, F - 1), optional ``rotation`` degrees (scalar or (B,)) and ``flip`` (B) (the caller mirrors
        ``center`` to ``Wp - 1 - x`` itself, as the reference's training flip does), optional ``blur``: the training blur as
        (B, F, 9, 5) tables (every slot blurred) or a ``(tables, blur_on)`` pair (otpose_amd.augment.Augmentation.
        blur_tables).  The crops (dataset/PoseTrackDataset.py:386-406) are cut on the GPU: in eval straight into the
        engine's input buffer (no copy), in ``model.train()`` into a fresh tensor for the training forward."""
        from . import crop
        w_img, h_img = self.cfg.MODEL.IMAGE_SIZE
        fi = torch.as_tensor(frame_idx)
        if fi.dim() != 2 or fi.shape[1] != self.window_frames:
            raise ValueError(f"frame_idx must be (B, {self.window_frames})")
        b = fi.shape[0]
        M = crop.crop_matrix(_host(center), _host(scale), 0.0 if rotation is None else _host(rotation), (w_img, h_img))
        margin = torch.as_tensor(margin, dtype=torch.float32).to(pool.device)
        tab, on = blur if isinstance(blur, (tuple, list)) else (blur, None)
        if self.training:
            x = ops.crop_clips(pool, fi, M, flip, size=(w_img, h_img), blur=tab, blur_on=on)
            return self.forward(x, margin=margin)
        x, _ = self.input_buffers(b, pool.device)
        ops.crop_clips(pool, fi, M, flip, out=x, blur=tab, blur_on=on)
        return self.forward(x, margin=margin)

    def training_batch(self, pool, frame_idx, margin, joints, joints_vis, center, scale, augment=None):
        """One augmented training batch from whole video frames - the training branch of the reference's
        ``_get_spatio_temporal_window`` (dataset/PoseTrackDataset.py:343-420) for B persons at once.

        ``pool`` (S, Hp, Wp, 3) uint8 RGB frames on the GPU, ``frame_idx`` (B, F) and ``margin`` (B, F - 1) as for
        :meth:`forward_video`, ``joints`` / ``joints_vis`` (B, J, 3) and ``center`` / ``scale`` (B, 2) of the data items.
        ``augment``: an :class:`otpose_amd.augment.Augmentation`, or None to draw one with
        :func:`otpose_amd.augment.sample_augmentation` (the global ``np.random`` / ``random`` / ``torch`` generators, as
        the reference) from ``cfg.TRAIN`` (SCALE_FACTOR, ROT_FACTOR, FLIP, PROB_HALF_BODY, NUM_JOINTS_HALF_BODY; the
        PoseTrack18 values where absent).  The crops are cut with the flip and the blur on the GPU, and the targets drawn
        from the flipped joints (``cfg.MODEL.SIGMA``, 3 where absent).  The flip and the blur mirror and reflect at the
        pool's width, so every frame of the pool must be Wp wide (not a narrower frame zero-padded into it).

        Returns ``(x (B, 3F, H, W), margin (B, F - 1), target (B, J, h, w), target_weight (B, J, 1))`` float32 on the
        pool's device, the arguments of ``parallel.train_step_dp`` / ``train.forward_train`` + ``train.criterion``."""
        from . import augment as A
        from . import crop
        m = self.cfg.MODEL
        w_img, h_img = m.IMAGE_SIZE
        fi = torch.as_tensor(frame_idx)
        if fi.dim() != 2 or fi.shape[1] != self.window_frames:
            raise ValueError(f"frame_idx must be (B, {self.window_frames})")
        if augment is None:
            t = _train_augment_cfg(self.cfg)
            augment = A.sample_augmentation(_host(joints), _host(joints_vis), _host(center), _host(scale),
                                            int(pool.shape[2]), aspect_ratio=w_img * 1.0 / h_img,
                                            frames=self.window_frames, **t)
        if augment.blur_sigma.shape != tuple(fi.shape):
            raise ValueError(f"augment is for {augment.blur_sigma.shape} slots, frame_idx is {tuple(fi.shape)}")
        M = crop.crop_matrix(augment.center, augment.scale, augment.rotation, (w_img, h_img))
        tab, on = augment.blur_tables()
        x = ops.crop_clips(pool, fi, M, augment.flip, size=(w_img, h_img), blur=tab, blur_on=on)
        target, weight = ops.pose_targets(augment.joints, augment.joints_vis, torch.from_numpy(M).to(pool.device),
                                          int(m.get("SIGMA", 3)), (w_img, h_img), m.HEATMAP_SIZE)
        margin = torch.as_tensor(margin, dtype=torch.float32).to(pool.device)
        return x, margin, target, weight

    def predict(self, pool, frame_idx, center, scale, margin, flip_test=False, shift_heatmap=False):
        """Keypoints in source-image pixels for B persons: the eval :meth:`forward_video` (no rotation, no flip), then the
        argmax + quarter-pixel refinement + inverse crop transform of ``ops.get_final_preds`` on the output heat-maps.
        Returns ``(preds (B, J, 2), maxvals (B, J, 1))`` float32 device tensors.

        ``flip_test=True`` is HRNet's flip test (the reference's ``TEST.FLIP_TEST``; ``shift_heatmap`` its
        ``TEST.SHIFT_HEATMAP``): the crops and their column mirrors are cut as one 2B batch straight into the engine's
        input buffer, one forward runs with the margins repeated, and ``ops.flip_test_merge`` flips the mirrored maps
        back, swaps ``augment.FLIP_PAIRS``, averages and decodes in one kernel.  The engine is built for 2B clips, so
        alternating flip and plain calls rebuilds it each time."""
        if self.training:
            raise RuntimeError("OTPose.predict runs in eval mode (call model.eval())")
        c = torch.as_tensor(_host(center), dtype=torch.float32)
        s = torch.as_tensor(_host(scale), dtype=torch.float32)
        if not flip_test:
            out = self.forward_video(pool, frame_idx, center, scale, margin)
            return ops.get_final_preds(out[0], c, s)
        from . import crop
        w_img, h_img = self.cfg.MODEL.IMAGE_SIZE
        fi = torch.as_tensor(frame_idx)
        if fi.dim() != 2 or fi.shape[1] != self.window_frames:
            raise ValueError(f"frame_idx must be (B, {self.window_frames})")
        b = fi.shape[0]
        M = crop.crop_matrix(_host(center), _host(scale), 0.0, (w_img, h_img))
        x, mg = self.input_buffers(2 * b, pool.device)
        ops.crop_clips(pool, fi, M, out=x, mirror_pair=True)
        _, preds, maxvals = self._flip_forward(x, mg, margin, shift_heatmap, c, s)
        return preds, maxvals

    def flip_test_heatmaps(self, x, margin, shift_heatmap=False):
        """The flip-test heat-maps of normalised clips ``x`` (B, 3F, H, W) on the GPU with ``margin`` (B, F - 1): ``x`` and
        its mirror ``x.flip(3)`` go through one 2B forward (``ops.mirror_pair`` writes both into the engine's input
        buffer), and the merged (B, J, h, w) maps of ``ops.flip_test_merge`` come back - what HRNet's ``validate`` feeds
        to ``get_final_preds`` under ``TEST.FLIP_TEST`` (``shift_heatmap``: ``TEST.SHIFT_HEATMAP``)."""
        if self.training:
            raise RuntimeError("OTPose.flip_test_heatmaps runs in eval mode (call model.eval())")
        if x.dim() != 4:
            raise ValueError("x must be a (B, 3F, H, W) clip tensor")
        xin, mg = self.input_buffers(2 * x.shape[0], x.device)
        ops.mirror_pair(x, out=xin)
        return self._flip_forward(xin, mg, margin, shift_heatmap)[0]

    def _flip_forward(self, x2, mg2, margin, shift_heatmap, center=None, scale=None):
        """One eval forward of the engine's own 2B input ``x2`` with the B margins repeated into ``mg2``, then the fused
        flip-back merge + decode of its heat-maps."""
        b = x2.shape[0] // 2
        margin = torch.as_tensor(margin, dtype=torch.float32).to(x2.device)
        if tuple(margin.shape) != (b, mg2.shape[1]):
            raise ValueError(f"margin must be ({b}, {mg2.shape[1]})")
        mg2[:b].copy_(margin)
        mg2[b:].copy_(margin)
        out = self._engine.run(x2, mg2, alias_outputs=True)
        return ops.flip_test_merge(out[0], shift_heatmap=shift_heatmap, center=center, scale=scale)

    def input_buffers(self, batch, device):
        """The eval engine's own input tensors for ``batch`` clips on ``device``: ``(x (B, 3 F, H, W) fp32, margin (B, F - 1)
        fp32)``.  A data loader that writes the next batch straight into them and passes them to ``forward`` saves the
        per-call device-to-device copy (106 MB at cfg2) - ``forward`` recognises its own buffers by address."""
        device = torch.device(device)
        w_img, h_img = self.cfg.MODEL.IMAGE_SIZE
        f = getattr(self, "window_frames", 5)
        if self._engine is None or not self._engine.matches_shape(batch, 3 * f, h_img, w_img, device):
            self._engine = self._engine_class()(self, batch, device)
        return self._engine.inp, self._engine.margin

    def eval_dtype(self) -> str:
        """``cfg.MODEL.DTYPE`` of the eval forward: "fp32" (default: fp32 tensors, the reference's arithmetic contract) or "fp16"
        (BASELINE configs[4]: the backbone on half activations, csrc/h16.hip - an extension, the reference never runs below fp32)."""
        m = self.cfg.MODEL
        dt = str(m.get("DTYPE", "fp32") if hasattr(m, "get") else getattr(m, "DTYPE", "fp32")).lower()
        if dt in ("fp32", "float32", "f32"):
            return "fp32"
        if dt in ("fp16", "float16", "half", "f16"):
            return "fp16"
        raise ValueError(f"MODEL.DTYPE must be 'fp32' or 'fp16', got {dt!r}")

    def _engine_class(self):
        if self.eval_dtype() == "fp16":
            from .engine_h16 import InferenceEngineH16
            return InferenceEngineH16
        from .engine import InferenceEngine
        return InferenceEngine

    def check_range(self):
        """Synchronise and raise ``FloatingPointError`` if an eval forward since the last check drove a value beyond the range of
        the half-precision operand pieces (|x| >= 65504: csrc/common.h, csrc/range.hip).  The engine also checks, without
        synchronising, at the start of every forward (``OTPOSE_RANGE_CHECK=sync``: at the end of the forward itself)."""
        if self._engine is not None:
            self._engine.check_range()

    def invalidate_engine(self):
        """Drop packed weights (call after changing parameters, e.g. load_state_dict)."""
        self._engine = None

    def load_state_dict(self, *a, **k):
        self._engine = None
        return super().load_state_dict(*a, **k)
