"""Track embedding head and RoI extraction -- drop-ins for `QuasiDenseMaskEmbedHeadGTMask`
(polyphonic/video/track_heads.py:12-162) and the `SingleRoIExtractor` + RoIAlign call of
`PolyphonicVideo._track_forward` (polyphonic_former_video.py:408-419), on libpolyhead (csrc/ph_track.hip).
Same registry name, constructor kwargs and state_dict keys (convs.{i}.conv.weight, convs.{i}.gn.*, fcs.0.*,
fc_embed.*).

Inference (eval mode or no_grad) runs the packed 16-bit kernels (`forward_planes`).  In training mode with grad enabled `forward`
runs the fp32 training form on the nodes of train.py (`_Conv3x3`, `_GNReLU`) and the linear layers on `ph_gemm32`; `track_loss` is
the reference's `loss(*match(...), *get_track_targets(...))` as ONE autograd node on `ph_track_loss` (csrc/ph_trackloss.hip)."""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib, engine as E
from .bricks import _LossStub
from .pack import pack_b_fragments
from .registry import LOSSES, register_everywhere

for _n in ("MultiPosCrossEntropyLoss", "L2Loss"):
    if _n not in LOSSES:
        LOSSES.register_module(name=_n, module=type(_n, (_LossStub,), {}))


LOSS_TRACK_DEFAULT = dict(type="MultiPosCrossEntropyLoss", loss_weight=0.25)
LOSS_TRACK_AUX_DEFAULT = dict(type="L2Loss", neg_pos_ub=3, pos_margin=0, neg_margin=0.1, hard_mining=True, loss_weight=1.0)


def _gemm32(A, lda, kcA, B, ldb, kcB, M, N, K, ksplit=1, bias=None):
    """C [M, N] = A(m, k) B(k, n) (+ bias[n]) on the training side's fp32-MFMA GEMM; kc: the operand is stored [row][k], else [k][row].
    ksplit > 1: the partial products are added in split order"""
    Cm = torch.empty((ksplit, M, N), dtype=torch.float32, device=A.device)
    _lib.check(_lib.load().ph_gemm32(_lib.ptr(A), lda, kcA, _lib.ptr(B), ldb, kcB, _lib.ptr(Cm), N, M, N, K, ksplit, _lib.ptr(bias),
                                     _lib.stream_ptr()), "ph_gemm32")
    return Cm[0] if ksplit == 1 else Cm.sum(0)


def _ksplit(K, want):
    """a split of K's 32-wide steps that leaves no part empty"""
    steps = (K + 31) // 32
    ks = max(1, min(want, steps))
    per = (steps + ks - 1) // ks
    return (steps + per - 1) // per


class _FcEmbed(torch.autograd.Function):
    """fc_embed(relu(fcs.0(x))) (track_heads.py:96-101) as one node: x [n, 12544] (the NCHW flatten), fp32 MFMA products.
    backward: dX, both weight gradients (dW1 [F][12544] tiled over its 12 544 columns) and the bias gradients.  Every operand's
    vectorised axis (k, or the row index of a transposed operand) is a multiple of 4 here, which is all ph_gemm32 asks."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2):
        from .train import _gpu32, _param32
        x = _gpu32(x, "x")
        W1, b1, W2, b2 = (_param32(p, "track head linear parameter") for p in (W1, b1, W2, b2))
        n, K1 = x.shape
        F_, Ee = W1.shape[0], W2.shape[0]
        if K1 % 4 or F_ % 4 or Ee % 4:
            raise _lib.PolyheadError("track head linear layers: widths must be multiples of 4")
        h = _gemm32(x, K1, 1, W1, K1, 1, n, F_, K1, _ksplit(K1, 16), b1).clamp_(min=0)
        out = _gemm32(h, F_, 1, W2, F_, 1, n, Ee, F_, _ksplit(F_, 8), b2)
        ctx.save_for_backward(x, h, W1, W2)
        return out

    @staticmethod
    def backward(ctx, g):
        from .train import _gpu32
        x, h, W1, W2 = ctx.saved_tensors
        g = _gpu32(g, "grad")
        n, K1 = x.shape
        F_, Ee = W1.shape[0], W2.shape[0]
        gW2 = _gemm32(g, Ee, 0, h, F_, 0, Ee, F_, n)                    # dE^T h
        gh = _gemm32(g, Ee, 1, W2, F_, 0, n, F_, Ee)                     # dE W2
        gh = gh * (h > 0)
        gW1 = _gemm32(gh, F_, 0, x, K1, 0, F_, K1, n)                    # dH^T x
        gx = _gemm32(gh, F_, 1, W1, K1, 0, n, K1, F_) if ctx.needs_input_grad[0] else None
        return gx, gW1, gh.sum(0), gW2, g.sum(0)


class _TrackLoss(torch.autograd.Function):
    """`ph_track_loss` as one node: -> (loss_track + loss_track_aux, the two values); backward hands the stored gradients on"""

    @staticmethod
    def forward(ctx, cfg, host, key_gt, ref_gt, gt_match, key, ref):
        from .train import _gpu32
        lib = _lib.load()
        key, ref = _gpu32(key, "key embeddings"), _gpu32(ref, "reference embeddings")
        losses = torch.empty((2,), dtype=torch.float32, device=key.device)
        gk, gr = torch.empty_like(key), torch.empty_like(ref)
        scratch = torch.empty((max(lib.ph_track_loss_scratch_bytes(C.byref(cfg), key.shape[0], ref.shape[0]), 16),), dtype=torch.uint8,
                              device=key.device)
        _lib.check(lib.ph_track_loss(C.byref(cfg), _lib.ptr(key), _lib.ptr(ref), host[0], host[1], _lib.ptr(key_gt), _lib.ptr(ref_gt), host[2],
                                     _lib.ptr(gt_match), _lib.ptr(losses), _lib.ptr(gk), _lib.ptr(gr), _lib.ptr(scratch), scratch.numel(),
                                     _lib.stream_ptr()), "ph_track_loss")
        ctx.save_for_backward(gk, gr)
        ctx.mark_non_differentiable(losses)
        return (losses[0].double() + losses[1].double()).float(), losses

    @staticmethod
    def backward(ctx, g, _):
        gk, gr = ctx.saved_tensors
        return None, None, None, None, None, g * gk, g * gr


def segment_boxes(pan, nseg):
    """int32 id map [H,W] on the GPU, ids 1..nseg -> (rois [nseg,5], extent boxes [nseg,4]) fp32 on the GPU"""
    E._require_gpu(pan, "panoptic map")
    lib = _lib.load()
    pan = pan.to(torch.int32).contiguous()
    H, W = pan.shape
    rois = torch.empty((nseg, 5), dtype=torch.float32, device=pan.device)
    ext = torch.empty((nseg, 4), dtype=torch.float32, device=pan.device)
    ws = torch.empty((lib.ph_segment_boxes_workspace_bytes(nseg),), dtype=torch.uint8, device=pan.device)
    _lib.check(lib.ph_segment_boxes(_lib.ptr(pan), H, W, nseg, _lib.ptr(rois), _lib.ptr(ext), _lib.ptr(ws), ws.numel(),
                                    _lib.stream_ptr()), "ph_segment_boxes")
    return rois, ext


def gt_mask_rois(masks, match, n, out_hw, num_proposals=None, mode="bilinear"):
    """The RoIs of the sampled ground-truth masks of a training step (polyphonic_former_video.py:283-305 + 413-415) from the masks at the
    assign resolution, selection included: `ph_gtmask_boxes` (csrc/ph_gtbox.hip), launches only.  Per frame b: masks[b] fp32 [G, h, w]
    on the GPU (non-negative), match[b] int32 [>= G] on the GPU -- the prediction row of every ground truth or -1, as `ph_assign_solve`
    leaves it (or one [frames, ld] tensor) --, n[b] = min(G, num_proposals) matched ground truths (host ints).  out_hw: the padded
    image size.  -> per-frame lists (rois [n, 5] fp32 (0, x1, y1, x2, y2) in ascending prediction row, pos_gt [n] int32, count [n] int64:
    the on pixels of the upsampled mask), views of ONE allocation."""
    lib = _lib.load()
    F_ = len(masks)
    if F_ == 0 or len(n) != F_ or (not torch.is_tensor(match) and len(match) != F_):
        raise ValueError("gt_mask_rois: one masks / match / n entry per frame")
    for m in masks:
        E._require_gpu(m, "ground-truth masks")
        if m.dim() != 3 or m.dtype != torch.float32 or not m.is_contiguous() or m.shape[1:] != masks[0].shape[1:]:
            raise _lib.PolyheadError("gt_mask_rois: masks are fp32 contiguous [G, h, w] of one size per call")
    dev = masks[0].device
    h, w = (int(v) for v in masks[0].shape[1:])
    H, W = int(out_hw[0]), int(out_hw[1])
    G = [int(m.shape[0]) for m in masks]
    n = [int(v) for v in n]
    if num_proposals is None:             # any Np >= max G is consistent with n == G everywhere; a frame with n < G names it
        cut = [v for v, g in zip(n, G) if v < g]
        num_proposals = cut[0] if cut else max(G + [0])
    if torch.is_tensor(match) and match.dim() == 2 and match.dtype == torch.int32 and match.is_contiguous() and match.shape[0] == F_:
        mt = match
    else:
        mt = torch.full((F_, max(G + [1])), -1, dtype=torch.int32, device=dev)
        for b in range(F_):
            if G[b]:
                mt[b, :G[b]] = match[b].reshape(-1)[:G[b]]
    E._require_gpu(mt, "match")
    total = sum(max(v, 0) for v in n)
    buf = torch.empty((max(total, 1) * 32,), dtype=torch.uint8, device=dev)        # count [total] int64 | rois [total][5] | pos_gt [total]
    count = buf[:8 * total].view(torch.int64)
    rois = buf[8 * total:28 * total].view(torch.float32).view(total, 5)
    pos_gt = buf[28 * total:32 * total].view(torch.int32)
    start = [0]
    for v in n:
        start.append(start[-1] + max(v, 0))
    i32 = lambda a: (C.c_int32 * len(a))(*a)
    md = {"bilinear": _lib.PH_GTBOX_BILINEAR, "nearest": _lib.PH_GTBOX_NEAREST}[mode]
    for b0 in range(0, F_, _lib.PH_GTBOX_MAX_FRAMES):
        b1 = min(F_, b0 + _lib.PH_GTBOX_MAX_FRAMES)
        Gc = i32(G[b0:b1])
        need = lib.ph_gtmask_boxes_workspace_bytes(b1 - b0, Gc, H, W)
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
        ptrs = (C.c_void_p * (b1 - b0))(*[m.data_ptr() if m.shape[0] else None for m in masks[b0:b1]])
        _lib.check(lib.ph_gtmask_boxes(ptrs, Gc, i32(n[b0:b1]), i32(start[b0:b1]), _lib.ptr(mt[b0:]), mt.stride(0), int(num_proposals), b1 - b0,
                                       h, w, H, W, md, _lib.ptr(rois), _lib.ptr(pos_gt), _lib.ptr(count), _lib.ptr(ws), need,
                                       _lib.stream_ptr()), "ph_gtmask_boxes")
    cut = lambda t: [t[start[b]:start[b + 1]] for b in range(F_)]
    return cut(rois), cut(pos_gt), cut(count)


def roi_extract(feats, rois, prec, strides=(4, 8, 16, 32), finest_scale=56.0, want_f32=False):
    """feats: list of fp32 [1,256,H_l,W_l] GPU tensors (the FPN levels), rois [n,5] GPU.
    Returns channels-last bf16 planes int16 [P,n,49,256] (and fp32 [n,256,7,7] if asked)."""
    lib = _lib.load()
    n, dev = rois.shape[0], rois.device
    feats = [f.float().contiguous() for f in feats]
    for f in feats:
        if f.shape[0] != 1 or f.shape[1] != 256:
            raise _lib.PolyheadError("roi_extract: one image, 256 channels per level")
    P = 2 if prec == _lib.PH_PREC_SPLIT else 1
    out = torch.empty((P, n, 49, 256), dtype=torch.int16, device=dev)
    f32 = torch.empty((n, 256, 7, 7), dtype=torch.float32, device=dev) if want_f32 else None
    L = len(feats)
    ptrs = (C.c_void_p * L)(*[f.data_ptr() for f in feats])
    hw = (C.c_int32 * (2 * L))(*[v for f in feats for v in f.shape[-2:]])
    sc = (C.c_float * L)(*[1.0 / s for s in strides[:L]])
    rois_f = rois.float().contiguous()                 # named: alive until the launch is queued
    _lib.check(lib.ph_roi_align_fpn(ptrs, hw, sc, L, _lib.ptr(rois_f), n, finest_scale, _lib.ptr(out),
                                    _lib.ptr(f32), prec, _lib.stream_ptr()), "ph_roi_align_fpn")
    return (out, f32) if want_f32 else out


def _planes(w64, P):
    w = w64.to(torch.float32)
    hi = w.to(torch.bfloat16)
    out = [hi.view(torch.int16)]
    if P == 2:
        out.append((w - hi.float()).to(torch.bfloat16).view(torch.int16))
    return torch.stack(out, 0).contiguous()


class QuasiDenseMaskEmbedHeadGTMask(nn.Module):

    def __init__(self, num_convs=4, num_fcs=1, roi_feat_size=7, in_channels=256, conv_out_channels=256,
                 fc_out_channels=1024, embed_channels=256, conv_cfg=None, norm_cfg=None, softmax_temp=-1,
                 loss_track=None, loss_track_aux=None):
        super().__init__()
        if not (roi_feat_size == 7 and in_channels == 256 and conv_out_channels == 256 and num_fcs == 1 and num_convs >= 1
                and norm_cfg is not None and norm_cfg.get("type") == "GN" and fc_out_channels % 16 == 0
                and embed_channels % 16 == 0):
            raise NotImplementedError("libpolyhead implements the shipped track head (4 x conv3x3+GN+ReLU on 7x7x256, one fc)")
        self.num_convs, self.num_fcs, self.roi_feat_size = num_convs, num_fcs, roi_feat_size
        self.in_channels, self.conv_out_channels = in_channels, conv_out_channels
        self.fc_out_channels, self.embed_channels = fc_out_channels, embed_channels
        self.norm_cfg, self.softmax_temp = norm_cfg, softmax_temp
        self.groups = norm_cfg.get("num_groups", 32)
        self.convs = nn.ModuleList()
        for _ in range(num_convs):
            m = nn.Module()
            m.conv = nn.Conv2d(256, 256, 3, padding=1, bias=False)
            m.gn = nn.GroupNorm(self.groups, 256)
            self.convs.append(m)
        self.fcs = nn.ModuleList([nn.Linear(256 * 49, fc_out_channels)])
        self.fc_embed = nn.Linear(fc_out_channels, embed_channels)
        self.precision = "fp32"
        self._pack = None
        # the loss configs are read for their numbers (track_loss); nothing is built from them
        self.loss_track_cfg = dict(LOSS_TRACK_DEFAULT if loss_track is None else loss_track)
        self.loss_track_aux_cfg = None if loss_track_aux is None else dict(loss_track_aux)

    def init_weights(self):
        for m in self.fcs:
            nn.init.xavier_uniform_(m.weight)
            nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.fc_embed.weight, 0, 0.01)
        nn.init.constant_(self.fc_embed.bias, 0)

    def _get_pack(self, device):
        prec = E.PREC[self.precision]
        ver = _lib.param_versions(self)
        key = (prec, str(device), ver)
        if self._pack is None or self._pack[0] != key:
            P = 2 if prec == _lib.PH_PREC_SPLIT else 1
            d = lambda t: t.detach().to("cpu", torch.float64)
            convs = []
            for m in self.convs:
                w = d(m.conv.weight).permute(0, 2, 3, 1).reshape(256, 9 * 256)        # K order (tap, channel)
                convs.append(_planes(pack_b_fragments(w), P).to(device))
            # fc consumes the NCHW flatten (ci*49 + pos) of the reference; our activations are (pos*256 + ci)
            wfc = d(self.fcs[0].weight).reshape(self.fc_out_channels, 256, 49).permute(0, 2, 1).reshape(self.fc_out_channels, -1)
            pk = dict(convs=convs, fc=_planes(pack_b_fragments(wfc), P).to(device),
                      emb=_planes(pack_b_fragments(d(self.fc_embed.weight)), P).to(device),
                      gn=[(m.gn.weight.detach().float().contiguous().to(device), m.gn.bias.detach().float().contiguous().to(device))
                          for m in self.convs],
                      fc_b=self.fcs[0].bias.detach().float().contiguous().to(device),
                      emb_b=self.fc_embed.bias.detach().float().contiguous().to(device), prec=prec, P=P)
            self._pack = (key, pk)
        return self._pack[1]

    def forward_planes(self, x_cl):
        """x_cl: channels-last bf16 planes int16 [P,n,49,256] (what `roi_extract` produces) -> embeddings [n,256] fp32"""
        lib, dev = _lib.load(), x_cl.device
        pk = self._get_pack(dev)
        P, n = x_cl.shape[0], x_cl.shape[1]
        if P != pk["P"]:
            raise _lib.PolyheadError("RoI feature planes were produced in a different precision than the head's")
        prec, s = pk["prec"], _lib.stream_ptr
        M, F_ = n * 49, self.fc_out_channels
        # split-K GEMMs (a dozen RoIs leave 16-68 workgroups otherwise); the convs gather their 3x3 patches in the operand loads
        ws = torch.empty((max(lib.ph_gemm_rows_workspace_bytes(M, 256, 2304), lib.ph_gemm_rows_workspace_bytes(n, F_, 49 * 256),
                              lib.ph_gemm_rows_workspace_bytes(n, self.embed_channels, F_)),), dtype=torch.uint8, device=dev)
        y = torch.empty((M, 256), dtype=torch.float32, device=dev)
        cur = x_cl.contiguous()
        for wp, (ga, be) in zip(pk["convs"], pk["gn"]):
            _lib.check(lib.ph_gemm_rows_splitk(_lib.ptr(cur), 1, _lib.ptr(wp), wp.shape[1], None, 0, _lib.ptr(y), None, M, 256, 2304, prec,
                                               _lib.ptr(ws), ws.numel(), s()), "ph_gemm_rows_splitk(conv)")
            nxt = torch.empty((P, n, 49, 256), dtype=torch.int16, device=dev)
            _lib.check(lib.ph_gn_relu_cl(_lib.ptr(y), _lib.ptr(ga), _lib.ptr(be), self.groups, 1e-5, _lib.ptr(nxt), n, prec, s()),
                       "ph_gn_relu_cl")
            cur = nxt
        h = torch.empty((P, n, F_), dtype=torch.int16, device=dev)
        _lib.check(lib.ph_gemm_rows_splitk(_lib.ptr(cur), 0, _lib.ptr(pk["fc"]), pk["fc"].shape[1], _lib.ptr(pk["fc_b"]), 1, None, _lib.ptr(h),
                                           n, F_, 49 * 256, prec, _lib.ptr(ws), ws.numel(), s()), "ph_gemm_rows_splitk(fc)")
        out = torch.empty((n, self.embed_channels), dtype=torch.float32, device=dev)
        _lib.check(lib.ph_gemm_rows_splitk(_lib.ptr(h), 0, _lib.ptr(pk["emb"]), pk["emb"].shape[1], _lib.ptr(pk["emb_b"]), 0, _lib.ptr(out),
                                           None, n, self.embed_channels, F_, prec, _lib.ptr(ws), ws.numel(), s()),
                   "ph_gemm_rows_splitk(fc_embed)")
        return out

    def forward(self, x):
        """track_heads.py:92-102: x fp32 [n,256,7,7] (RoI features) -> [n, embed_channels]"""
        E._require_gpu(x, "roi feats")
        if self.training and torch.is_grad_enabled():
            return self.forward_train(x)
        n = x.shape[0]
        P = 2 if E.PREC[self.precision] == _lib.PH_PREC_SPLIT else 1
        xc = x.float().permute(0, 2, 3, 1).reshape(n, 49, 256)            # layout change only (channels last)
        hi = xc.to(torch.bfloat16)
        planes = [hi.view(torch.int16)]
        if P == 2:
            planes.append((xc - hi.float()).to(torch.bfloat16).view(torch.int16))
        return self.forward_planes(torch.stack(planes, 0).contiguous())

    def forward_train(self, x):
        """the fp32 training form of `forward`, differentiable: 4 x (`_Conv3x3` -> `_GNReLU`), the NCHW flatten, `_FcEmbed`"""
        from .train import _Conv3x3, _GNReLU
        E._require_gpu(x, "roi feats")
        t = x.float()
        for m in self.convs:
            t = _GNReLU.apply(_Conv3x3.apply(t, m.conv.weight, 1), m.gn.weight, m.gn.bias, self.groups, None)
        return _FcEmbed.apply(t.reshape(t.shape[0], -1), self.fcs[0].weight, self.fcs[0].bias, self.fc_embed.weight, self.fc_embed.bias)

    def get_track_targets(self, gt_match_indices, key_sampling_results, ref_sampling_results):
        """track_heads.py:104-121 -> (targets: int [Nk, Nr] per pair, weights: float [Nk]); integer torch ops, any device.  For
        inspection and tests: the training path forms the targets inside `ph_track_loss`."""
        targets, weights = [], []
        for gm, kr, rr in zip(gt_match_indices, key_sampling_results, ref_sampling_results):
            m = gm[kr.pos_assigned_gt_inds.long()]
            t = (m.view(-1, 1) == rr.pos_assigned_gt_inds.view(1, -1)).int()
            targets.append(t)
            weights.append((t.sum(dim=1) > 0).float())
        return targets, weights

    def _track_loss_cfg(self, pairs, E_):
        if self.softmax_temp > 0:
            raise NotImplementedError("track_loss: softmax_temp > 0 (cosine logits) is not implemented; the shipped value is -1")
        lt, la = self.loss_track_cfg, self.loss_track_aux_cfg
        if lt.get("type") != "MultiPosCrossEntropyLoss" or lt.get("reduction", "mean") != "mean":
            raise NotImplementedError(f"track_loss: loss_track must be MultiPosCrossEntropyLoss with mean reduction, got {lt}")
        if la is None or la.get("type") != "L2Loss" or la.get("reduction", "mean") != "mean":
            raise NotImplementedError(f"track_loss: loss_track_aux must be L2Loss with mean reduction, got {la}")
        unknown = set(la) - {"type", "neg_pos_ub", "pos_margin", "neg_margin", "hard_mining", "reduction", "loss_weight"}
        if unknown:
            raise NotImplementedError(f"track_loss: L2Loss arguments {sorted(unknown)} are not the reference class's")
        ub = la.get("neg_pos_ub", -1)
        if ub != int(ub):
            raise NotImplementedError("track_loss: neg_pos_ub must be an integer")
        return _lib.TrackLossCfg(pairs=pairs, E=E_, lw_track=float(lt.get("loss_weight", 1.0)), lw_aux=float(la.get("loss_weight", 1.0)),
                                 neg_pos_ub=int(ub), pos_margin=float(la.get("pos_margin", -1)), neg_margin=float(la.get("neg_margin", -1)),
                                 hard_mining=int(bool(la.get("hard_mining", False))))

    def track_loss(self, key_embeds, ref_embeds, gt_match_indices, key_sampling_results, ref_sampling_results):
        """The reference's `loss(*match(key_embeds, ref_embeds, ...), *get_track_targets(...))` (track_heads.py:104-162) in one call:
        key_embeds [sum Nk, E], ref_embeds [sum Nr, E] on the GPU, per pair gt_match_indices and the two sampling results (their
        `pos_assigned_gt_inds`).  -> {'loss_track', 'loss_track_aux'} attached to the graph; their SUM carries the gradient (one
        node, `train._attach`)."""
        from .train import _attach
        E._require_gpu(key_embeds, "key embeddings")
        dev = key_embeds.device
        kg = [r.pos_assigned_gt_inds for r in key_sampling_results]
        rg = [r.pos_assigned_gt_inds for r in ref_sampling_results]
        pairs = len(kg)
        if not (pairs == len(rg) == len(gt_match_indices)) or pairs == 0:
            raise ValueError("track_loss: one gt_match_indices, key and reference sampling result per pair")
        cfg = self._track_loss_cfg(pairs, key_embeds.shape[1])

        def starts(parts):
            arr = (C.c_int32 * (pairs + 1))()
            for i, t in enumerate(parts):
                arr[i + 1] = arr[i] + int(t.numel())
            return arr

        def dev32(parts):
            if not sum(int(t.numel()) for t in parts):                  # no ground truth at all: a readable placeholder
                return torch.zeros((1,), dtype=torch.int32, device=dev)
            return torch.cat([torch.as_tensor(t).reshape(-1).to(dev, torch.int32) for t in parts]).contiguous()

        host = (starts(kg), starts(rg), starts(gt_match_indices))
        if host[0][pairs] != key_embeds.shape[0] or host[1][pairs] != ref_embeds.shape[0]:
            raise ValueError("track_loss: the sampling results' RoI counts do not add up to the embedding rows")
        total, values = _TrackLoss.apply(cfg, host, dev32(kg), dev32(rg), dev32(gt_match_indices), key_embeds, ref_embeds)
        return _attach({"loss_track": values[0], "loss_track_aux": values[1]}, total)

    def match(self, *a, **k):
        raise NotImplementedError("match() returns similarity matrices the training path never forms: use track_loss(key_embeds, ref_embeds, "
                                  "gt_match_indices, key_sampling_results, ref_sampling_results)")

    def loss(self, *a, **k):
        raise NotImplementedError("loss() takes similarity matrices the training path never forms: use track_loss(key_embeds, ref_embeds, "
                                  "gt_match_indices, key_sampling_results, ref_sampling_results)")


register_everywhere(QuasiDenseMaskEmbedHeadGTMask)
