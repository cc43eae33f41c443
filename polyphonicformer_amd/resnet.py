"""`ResNet` (mmdet/models/backbones/resnet.py:305-658) as the reference configures it (configs/_base_/models/polyphonic_former.py:12-21):
depth 50, four stages, `out_indices=(0, 1, 2, 3)`, `frozen_stages=1`, BatchNorm with `norm_eval=True`, `style='pytorch'`.

Same constructor keywords and the reference's state_dict keys (`conv1.weight`, `bn1.*`, `layer{1..4}.{j}.conv{1,2,3}.weight`,
`.bn{1,2,3}.*`, `.downsample.{0,1}.*`; 318 entries at depth 50).  Supported: depths 50 / 101 / 152, `style='pytorch'`,
`strides=(1, 2, 2, 2)`, dilations 1, any `out_indices`; everything else raises NotImplementedError naming the argument.

Inference (`forward` on the device with no gradient asked for) runs in libpolyhead (csrc/ph_resnet.hip): every BatchNorm is folded
into its convolution in float64 (`fold_bn`), activations are one 16-bit channels-last plane ('bf16', the default, or 'fp16'), and the
stages come back as NCHW tensors (fp32 by default; `set_stage_dtype` for the 16-bit hand-off `ph_fpn_lateral` also takes).
`forward_planes` hands the stages out as the plan's own channels-last planes instead (engine.StagePlanes), which fpn.FPN reads
directly (`ph_fpn_lateral_cl`): the same levels without an NCHW stage in between.
`use_native_plan(True)` moves the fold, the packing and the launch sequence into the library as well (ph_resnet_pack,
engine.NativeResNetPlan: one native call per forward, the same bits).  `_forward_torch` is the same arithmetic in torch ops: CPU tensors, and by default whenever grad is enabled and a parameter or the
input requires grad, as with fpn.FPN's default.

Training on the device is opt-in (`train_on_device()`): the training-mode `forward` then runs `train.resnet_forward_train` -- the
inference launch sequence with every activation kept, and a backward of data and weight gradients (csrc/ph_resnet_train.hip) from
layer4 down to the first stage behind the frozen ones, through the BatchNorm fold back to `conv.weight`, `bn.weight` and `bn.bias`.
Its scope is the shipped configuration: `frozen_stages >= 1`, `norm_eval=True`, grade 'bf16', an image that does not require grad;
anything else raises NotImplementedError naming the argument, never a fall-back to torch.

Keywords taken for the signature's sake only: `with_cp` (activation checkpointing trades memory for time and changes no value; it is
stored and not applied), `stage_with_dcn` (stored; without `dcn` it selects nothing), `pretrained` and `init_cfg` (loading a checkpoint
is the caller's `load_state_dict`; `init_cfg` is stored, `pretrained` is not, and `init_weights` applies the reference's default
initialisation, with `zero_init_residual` deciding whether each block's last norm starts at zero)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, engine as E
from .pack import pack_b32
from .registry import register_everywhere

ARCH = E.RESNET_ARCH
STEM_K = 176            # 7 kernel rows x 24 (21 values (kw, c) + 3 zeros) = 168, padded to a multiple of 16


def fold_bn(weight, bn):
    """(w', b') in float64 of conv `weight` [out][in][kh][kw] followed by the BatchNorm `bn` in eval mode:
    w' = w g / sqrt(var + eps), b' = beta - mu g / sqrt(var + eps)"""
    s = bn.weight.detach().to("cpu", torch.float64) / torch.sqrt(bn.running_var.detach().to("cpu", torch.float64) + bn.eps)
    w = weight.detach().to("cpu", torch.float64) * s[:, None, None, None]
    return w, bn.bias.detach().to("cpu", torch.float64) - bn.running_mean.detach().to("cpu", torch.float64) * s


def stem_matrix(w):
    """folded stem weight [64][3][7][7] -> W2 [64][176] in the kernel's K order k = 24 kh + 3 kw + c (zero where kw >= 7 or k >= 168)"""
    t = F.pad(w.permute(0, 2, 3, 1).reshape(64, 7, 21), (0, 3)).reshape(64, 168)
    return F.pad(t, (0, STEM_K - 168))


class Bottleneck(nn.Module):
    """resnet.py:96-302, style 'pytorch' (the stride on the 3x3), no dcn, no plugins"""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.inplanes, self.planes, self.stride = inplanes, planes, stride
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = downsample

    def forward(self, x):
        out = F.relu(self.bn1(self.conv1(x)))
        out = F.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return F.relu(out + (x if self.downsample is None else self.downsample(x)))


class ResNet(nn.Module):
    MAX_PLANS = 8            # device plans kept (one per batch size, image size, grade, hand-off dtype, out_indices)

    def __init__(self, depth, in_channels=3, stem_channels=None, base_channels=64, num_stages=4, strides=(1, 2, 2, 2),
                 dilations=(1, 1, 1, 1), out_indices=(0, 1, 2, 3), style="pytorch", deep_stem=False, avg_down=False, frozen_stages=-1,
                 conv_cfg=None, norm_cfg=dict(type="BN", requires_grad=True), norm_eval=True, dcn=None,
                 stage_with_dcn=(False, False, False, False), plugins=None, with_cp=False, zero_init_residual=True, pretrained=None,
                 init_cfg=None):
        super().__init__()

        def no(arg, why):
            raise NotImplementedError(f"ResNet: {arg}: libpolyhead implements the shipped backbone ({why})")
        if depth in (18, 34):
            no("depth", "Bottleneck depths 50 / 101 / 152; BasicBlock depths are not built")
        if depth not in ARCH:
            raise KeyError(f"invalid depth {depth} for resnet")
        if in_channels != 3:
            no("in_channels", "three image channels")
        if stem_channels not in (None, 64) or base_channels != 64:
            no("stem_channels" if stem_channels not in (None, 64) else "base_channels", "a 64-channel stem and base width")
        if num_stages != 4:
            no("num_stages", "four stages")
        if tuple(strides) != (1, 2, 2, 2):
            no("strides", "strides (1, 2, 2, 2)")
        if tuple(dilations) != (1, 1, 1, 1):
            no("dilations", "dilation 1 in every stage")
        if style != "pytorch":
            no("style", "style 'pytorch': the stride on the 3x3 convolution")
        if deep_stem:
            no("deep_stem", "the 7x7 stem")
        if avg_down:
            no("avg_down", "a strided 1x1 downsample")
        if conv_cfg is not None:
            no("conv_cfg", "plain Conv2d")
        if dict(norm_cfg).get("type") != "BN":
            no("norm_cfg", "BatchNorm")
        if dcn is not None:
            no("dcn", "no deformable convolution")
        if plugins is not None:
            no("plugins", "no plugins")
        if not out_indices or max(out_indices) >= 4 or min(out_indices) < 0:
            raise AssertionError("out_indices must lie in [0, num_stages)")
        self.depth, self.stem_channels, self.base_channels, self.num_stages = depth, 64, 64, 4
        self.strides, self.dilations, self.out_indices, self.style = tuple(strides), tuple(dilations), tuple(out_indices), style
        self.deep_stem, self.avg_down, self.frozen_stages, self.conv_cfg, self.norm_cfg = False, False, frozen_stages, None, dict(norm_cfg)
        self.with_cp, self.norm_eval, self.dcn, self.stage_with_dcn, self.plugins = with_cp, norm_eval, None, tuple(stage_with_dcn), None
        self.zero_init_residual, self.init_cfg = zero_init_residual, init_cfg
        self.stage_blocks = ARCH[depth]

        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64, eps=self.norm_cfg.get("eps", 1e-5))
        self.res_layers, inplanes = [], 64
        for i, nb in enumerate(self.stage_blocks):
            planes, stride = 64 * 2 ** i, self.strides[i]
            down = None
            if stride != 1 or inplanes != planes * 4:
                down = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4))
            blocks = [Bottleneck(inplanes, planes, stride, down)] + [Bottleneck(planes * 4, planes) for _ in range(1, nb)]
            inplanes = planes * 4
            self.add_module(f"layer{i + 1}", nn.Sequential(*blocks))
            self.res_layers.append(f"layer{i + 1}")
        eps = self.norm_cfg.get("eps", 1e-5)
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eps = eps
                for p in m.parameters():
                    p.requires_grad = self.norm_cfg.get("requires_grad", True)
        self.feat_dim = 2048
        self.precision, self.stage_dtype = "bf16", torch.float32
        self._packs, self._plans = {}, {}
        self._native, self._native_packs, self._native_plans = False, {}, {}
        self.device_training = False
        self._freeze_stages()

    def init_weights(self):
        for m in self.modules():                       # the default init_cfg: Kaiming on Conv2d, 1 on the norms, 0 on each block's norm3
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if self.zero_init_residual:
            for m in self.modules():
                if isinstance(m, Bottleneck):
                    nn.init.constant_(m.bn3.weight, 0)

    def set_precision(self, precision):
        """'bf16' (default) / 'fp16': the 16-bit format of the activation planes and the folded weights"""
        if precision not in ("bf16", "fp16"):
            raise ValueError(f"ResNet.set_precision: 'bf16' or 'fp16', not {precision!r} (a hi + lo grade is not built)")
        self.precision = precision
        self._packs.clear(); self._plans.clear()
        self._native_packs.clear(); self._native_plans.clear()
        return self

    def set_stage_dtype(self, dtype):
        """dtype of the NCHW stages `forward` returns on the device: torch.float32 (default), torch.bfloat16 or torch.float16"""
        if dtype not in E.OUT_CODE:
            raise ValueError("ResNet.set_stage_dtype: torch.float32, torch.bfloat16 or torch.float16")
        self.stage_dtype = dtype
        self._plans.clear(); self._native_plans.clear()
        return self

    def use_native_plan(self, flag=True):
        """opt in: `forward` on the device folds and packs with ph_resnet_pack and runs engine.NativeResNetPlan -- one native call per
        forward, the same launches and the same bits as the default path"""
        self._native = bool(flag)
        return self

    def train_on_device(self, flag=True):
        """opt in: `forward` with grad enabled and a parameter that requires grad runs `train.resnet_forward_train` (the library's
        forward with every activation kept, and its backward) instead of torch ops; off by default.  Out of its scope --
        frozen_stages < 1, norm_eval=False, grade 'fp16', an image that requires grad -- it raises NotImplementedError"""
        self.device_training = bool(flag)
        return self

    # ---- resnet.py:613-658
    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            self.bn1.eval()
            for m in (self.conv1, self.bn1):
                for p in m.parameters():
                    p.requires_grad = False
        for i in range(1, self.frozen_stages + 1):
            m = getattr(self, f"layer{i}")
            m.eval()
            for p in m.parameters():
                p.requires_grad = False

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, nn.modules.batchnorm._BatchNorm):
                    m.eval()
        return self

    def _forward_torch(self, x):
        """resnet.py:631-646 on the module's own parameters, differentiable"""
        x = F.max_pool2d(F.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        outs = []
        for i, name in enumerate(self.res_layers):
            x = getattr(self, name)(x)
            if i in self.out_indices:
                outs.append(x)
        return tuple(outs)

    # ---- folded, packed parameters: keyed on the versions of every parameter AND buffer (the running statistics are part of the fold)
    def _versions(self):
        return tuple((id(t), t._version) for _, m in _lib._tree(self) for d in (m._parameters, m._buffers) for t in d.values()
                     if t is not None)

    def _pack(self, dev):
        key = (str(dev), self.precision, self._versions())
        if key not in self._packs:
            self._packs.clear()
            f16 = self.precision == "fp16"

            def one(conv, bn, matrix=None):
                w, b = fold_bn(conv.weight, bn)
                w2 = matrix(w) if matrix else w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)         # K order (tap, channel)
                return pack_b32(E._planes_of(w2, 1, f16)[0]).contiguous().to(dev), b.float().contiguous().to(dev)
            blocks = []
            for name in self.res_layers:
                blocks.append([dict(conv1=one(m.conv1, m.bn1), conv2=one(m.conv2, m.bn2), conv3=one(m.conv3, m.bn3),
                                    downsample=None if m.downsample is None else one(m.downsample[0], m.downsample[1]))
                               for m in getattr(self, name)])
            self._packs[key] = dict(stem=one(self.conv1, self.bn1, stem_matrix), blocks=blocks)
        return self._packs[key]

    def _native_pack(self, dev, cfg):
        key = (str(dev), self.precision, self._versions())
        if key not in self._native_packs:
            self._native_packs.clear(); self._native_plans.clear()           # a plan is created over its pack
            self._native_packs[key] = E.native_resnet_pack(self, cfg, dev)
        return self._native_packs[key]

    def _native_plan_of(self, x):
        """`_plan_of` for the native path: (the NativeResNetPlan of this input, its pack, the input as the plan takes it)"""
        E._require_gpu(x, "x")
        if x.dim() != 4 or x.shape[1] != 3:
            raise _lib.PolyheadError("ResNet: x must be [B, 3, H, W]")
        eps = {m.eps for m in self.modules() if isinstance(m, nn.BatchNorm2d)}
        if len(eps) != 1:
            raise _lib.PolyheadError("ResNet.use_native_plan: ph_resnet_cfg carries one BatchNorm eps; this module's norms have several")
        dev, (B, _, H, W) = x.device, x.shape
        cfg = E.native_resnet_cfg(B, H, W, self.depth, self.precision, torch.float32, self.stage_dtype, self.out_indices, eps.pop())
        with torch.cuda.device(dev):
            pack = self._native_pack(dev, cfg)
            key = (B, H, W, str(dev), self.stage_dtype, tuple(self.out_indices))
            plan = self._native_plans.get(key)
            if plan is None:
                if len(self._native_plans) >= self.MAX_PLANS:
                    self._native_plans.clear()
                plan = self._native_plans[key] = E.NativeResNetPlan(pack, B, H, W, dev, cfg=cfg)
        return plan, pack, x.contiguous() if x.dtype in (torch.float32, torch.bfloat16) else x.contiguous().float()

    def block_table(self):
        """per stage a list of (cin, planes, stride, has_downsample): what engine.ResNetPlan sizes its buffers from"""
        return [[(m.inplanes, m.planes, m.stride, m.downsample is not None) for m in getattr(self, name)] for name in self.res_layers]

    def _plan_of(self, x, stage_planes=False):
        """(the device plan of this input, the packed parameters, the input as the plan takes it); stage_planes: the plan that keeps
        every output stage as a plane of its own (`forward_planes`)"""
        E._require_gpu(x, "x")
        if x.dim() != 4 or x.shape[1] != 3:
            raise _lib.PolyheadError("ResNet: x must be [B, 3, H, W]")
        dev, (B, _, H, W) = x.device, x.shape
        pk = self._pack(dev)
        key = (B, H, W, str(dev), self.precision, self.stage_dtype, tuple(self.out_indices), tuple(map(tuple, self.block_table())),
               stage_planes)
        plan = self._plans.get(key)
        if plan is None:
            if len(self._plans) >= self.MAX_PLANS:               # a plan holds every activation plane of its size: keep a few, not all
                self._plans.clear()
            with torch.cuda.device(dev):
                plan = self._plans[key] = E.ResNetPlan(B, H, W, self.block_table(), self.out_indices, E.KHEAD_PREC[self.precision],
                                                       self.stage_dtype, dev, stage_planes=stage_planes)
        return plan, pk, x.contiguous() if x.dtype in (torch.float32, torch.bfloat16) else x.contiguous().float()

    def forward(self, x):
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            if self.device_training:
                from .train import resnet_forward_train
                return resnet_forward_train(self, x)
            return self._forward_torch(x)
        if not x.is_cuda:
            return self._forward_torch(x)
        plan, pk, xin = self._native_plan_of(x) if self._native else self._plan_of(x)
        with torch.cuda.device(x.device):
            return plan.run(xin, pk)


    def forward_planes(self, x):
        """`forward` without the NCHW hand-off: the output stages as the engine.StagePlanes of the plan's own channels-last 16-bit
        planes, which fpn.FPN.forward and SemanticFPNWrapper.forward_from_fpn take in place of the tensors (ph_fpn_lateral_cl reads
        them: the same levels as `fpn(backbone(x))`, bit for bit, without the stages crossing memory as fp32 NCHW).  The planes are
        overwritten by the next call at this size.  Inference on the device, Python plan only."""
        if self._native:
            raise _lib.PolyheadError("ResNet.forward_planes: the native plan hands out NCHW stages only; use_native_plan(False)")
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise _lib.PolyheadError("ResNet.forward_planes is the inference hand-over; with grad enabled call forward")
        plan, pk, xin = self._plan_of(x, stage_planes=True)
        with torch.cuda.device(x.device):
            plan.run(xin, pk, nchw=False)
        return E.StagePlanes([plan.stage_plane(i) for i in self.out_indices], [plan.stage_shapes[i] for i in self.out_indices], plan.prec)


register_everywhere(ResNet, kind="backbone")
