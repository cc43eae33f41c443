"""`FPN` (mmdet/models/necks/fpn.py:11-203) as the reference configures it (configs/_base_/models/polyphonic_former.py:22-29):
four backbone stages (256 / 512 / 1024 / 2048 channels) -> four 256-channel pyramid levels through four 1x1 lateral convolutions,
a nearest-neighbour top-down add and four 3x3 output convolutions, every convolution with bias and without norm or activation.

Same constructor keywords and the reference's 16 state_dict keys (`lateral_convs.{i}.conv.{weight,bias}`,
`fpn_convs.{i}.conv.{weight,bias}`).  Inference runs in libpolyhead (csrc/ph_fpn.hip + the neck's 3x3 kernel): the laterals read the
backbone's NCHW maps as they are (fp32, bf16 or fp16) and write channels-last 16-bit planes, the 3x3 convolutions run on those.

Training: in training mode with grad enabled `forward` runs the reference's statements on the module's own parameters with torch ops
(`F.conv2d`, `F.interpolate`), on whatever device the inputs live -- the default.  `train_on_device()` switches that branch to the
library's own autograd nodes (`train.fpn_forward_train`: csrc/ph_fpntrain.hip + the training kernels of the neck), fp32 NCHW on
the GPU, whose gradients are summed in a fixed order; it is opt-in because it is not the faster of the two."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, engine as E
from .pack import pack_b32
from .registry import MODELS


class _Conv(nn.Module):
    """parameter container with ConvModule's tree (`conv`): a convolution with bias, no norm, no activation"""

    def __init__(self, cin, cout, k):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, padding=k // 2)


class FPN(nn.Module):
    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, add_extra_convs=False,
                 relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None, norm_cfg=None, act_cfg=None,
                 upsample_cfg=dict(mode="nearest"), init_cfg=dict(type="Xavier", layer="Conv2d", distribution="uniform")):
        super().__init__()

        def no(arg, why):
            raise NotImplementedError(f"FPN: {arg}: libpolyhead implements the shipped FPN ({why})")
        if not isinstance(in_channels, (list, tuple)) or len(in_channels) != 4:
            no("in_channels", "four input levels")
        if any(c % 64 or not 64 <= c <= 4096 for c in in_channels):
            no("in_channels", "every input width a multiple of 64 in [64, 4096]")
        if out_channels != 256:
            no("out_channels", "256 output channels")
        if start_level != 0:
            no("start_level", "start_level 0")
        if end_level not in (-1, 4):
            no("end_level", "all four levels")
        if num_outs != 4:
            no("num_outs", "four outputs, so that add_extra_convs never builds a layer")
        if not isinstance(add_extra_convs, (str, bool)) or (isinstance(add_extra_convs, str) and
                                                             add_extra_convs not in ("on_input", "on_lateral", "on_output")):
            no("add_extra_convs", "a bool or 'on_input' / 'on_lateral' / 'on_output'")
        if conv_cfg is not None:
            no("conv_cfg", "plain Conv2d")
        if norm_cfg is not None:
            no("norm_cfg", "no norm")
        if act_cfg is not None:
            no("act_cfg", "no activation")
        if dict(upsample_cfg) != dict(mode="nearest"):
            no("upsample_cfg", "nearest upsampling to the finer level's size, without scale_factor")
        self.in_channels, self.out_channels, self.num_ins, self.num_outs = list(in_channels), out_channels, 4, num_outs
        self.start_level, self.end_level, self.backbone_end_level = start_level, end_level, 4
        self.add_extra_convs = "on_input" if add_extra_convs is True else add_extra_convs
        self.relu_before_extra_convs, self.no_norm_on_lateral = relu_before_extra_convs, no_norm_on_lateral
        self.upsample_cfg = dict(upsample_cfg)
        self.init_cfg = init_cfg
        self.lateral_convs = nn.ModuleList([_Conv(c, 256, 1) for c in in_channels])
        self.fpn_convs = nn.ModuleList([_Conv(256, 256, 3) for _ in in_channels])
        self.precision = "fp32"
        self.device_training = False
        self._packs, self._plans = {}, {}

    def init_weights(self):
        for m in self.modules():                       # init_cfg: Xavier, uniform, on every Conv2d
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_uniform_(m.weight)
                nn.init.constant_(m.bias, 0)

    def set_precision(self, precision):
        """'bf16' / 'fp16': one 16-bit plane of activations and weights; 'fp32' (default): hi + lo bf16 planes of both"""
        assert precision in E.PREC
        self.precision = precision
        self._packs.clear(); self._plans.clear()

    def train_on_device(self, flag=True):
        """training-mode `forward` on the library's nodes (`train.fpn_forward_train`) instead of torch ops; off by default.  On that
        path the stages must live on the GPU and the parameters be fp32 (`PolyheadError` names the argument otherwise)."""
        self.device_training = bool(flag)
        return self

    # ---- packed parameters: keyed on the parameter versions (load_state_dict / an optimizer step after a first forward re-pack)
    def _pack(self, dev):
        key = (str(dev), self.precision, _lib.param_versions(self))
        if key not in self._packs:
            self._packs.clear()
            prec = E.KHEAD_PREC[self.precision]
            P = 2 if prec == _lib.PH_PREC_SPLIT else 1

            def one(m, k):
                w = m.conv.weight.detach().to("cpu", torch.float64)                   # [out][in][kh][kw]
                w2 = w.permute(0, 2, 3, 1).reshape(256, -1)                           # K order (tap, channel)
                planes = E._planes_of(w2, P, prec == _lib.PH_PREC_F16)               # [P][256][K]
                wp = torch.stack([pack_b32(planes[p]) for p in range(P)], 0).contiguous().to(dev)
                return dict(wp=wp, bias=m.conv.bias.detach().float().contiguous().to(dev), k=k, s=1)
            self._packs[key] = dict(lateral=[one(m, 1) for m in self.lateral_convs], output=[one(m, 3) for m in self.fpn_convs])
        return self._packs[key]

    def _forward_torch(self, inputs):
        """fpn.py:151-203 for this structure, differentiable"""
        lat = [F.conv2d(inputs[i], m.conv.weight, m.conv.bias) for i, m in enumerate(self.lateral_convs)]
        for i in range(3, 0, -1):
            lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=lat[i - 1].shape[2:], mode="nearest")
        return tuple(F.conv2d(lat[i], m.conv.weight, m.conv.bias, padding=1) for i, m in enumerate(self.fpn_convs))

    def forward(self, inputs):
        """inputs: the four backbone stages, or an engine.StagePlanes (resnet.ResNet.forward_planes: the laterals then read the
        backbone's channels-last planes directly -- the same levels, bit for bit; inference on the device only)"""
        assert len(inputs) == len(self.in_channels)
        if self.training and torch.is_grad_enabled():
            if isinstance(inputs, E.StagePlanes):
                raise _lib.PolyheadError("FPN: StagePlanes are the inference hand-over; in training mode with grad enabled pass the stages")
            if self.device_training:
                from .train import fpn_forward_train
                return fpn_forward_train(self, inputs)
            return self._forward_torch(inputs)
        plan, pk, feats = self._plan_of(inputs)
        with torch.cuda.device(plan.y.device):
            return tuple(plan.run(feats, pk))

    def _plan_of(self, inputs):
        """(the device plan of these stages, the packed parameters, the stages as the plan takes them): what `forward` runs, and
        what SemanticFPNWrapper.forward_from_fpn runs with the neck's plan as the receiver of the levels"""
        planes = isinstance(inputs, E.StagePlanes)
        x0 = inputs.planes[0] if planes else inputs[0]
        E._require_gpu(x0, "inputs[0]")
        dev, B = x0.device, x0.shape[0]
        shapes = tuple(s[1:] for s in inputs.shapes) if planes else tuple(tuple(t.shape[-2:]) for t in inputs)
        prec = E.KHEAD_PREC[self.precision]
        pk = self._pack(dev)
        key = (B, shapes, str(dev), self.precision)
        plan = self._plans.get(key)
        if plan is None:
            with torch.cuda.device(dev):
                plan = self._plans[key] = E.FpnPlan(B, shapes, self.in_channels, prec, dev)
        if planes:
            return plan, pk, inputs
        return plan, pk, [t.contiguous() if t.dtype in E.OUT_CODE else t.contiguous().float() for t in inputs]


MODELS.register_module(module=FPN, force=True)       # this package's registry only: mmdet's own FPN stays mmdet's
