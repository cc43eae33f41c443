"""One training step of the path: forward in training mode, the objective, backward.

What `PolyphonicFormer.forward_train` runs after `extract_feat` (polyphonic_former.py:96-129) and what mmdet's
`BaseDetector._parse_losses` + `loss.backward()` do with its result (mmdet/models/detectors/base.py:176-199):

    rpn_head.forward_train -> roi_head.forward_train -> objective = sum of the entries whose key contains 'loss' -> backward

How the work is split on the MI355X (round 5: every tensor operation of the step that touches a map or a weight is a
libpolyhead kernel, forward and backward; torch is the autograd bookkeeping between four kinds of nodes):

  * `_Rpn`: KernelHead after the neck -- three 1x1 conv + GroupNorm + ReLU towers, x = sem + loc, the static 1x1 convs,
    the hard-mask pooling (csrc/ph_train.hip products, csrc/ph_gntrain.hip GroupNorm forward / backward);
  * `_Stage` (one per KernelUpdateHead): hard-mask pooling, the whole query side -- KernelUpdator x2, attention + LN x2,
    FFN + LN x2, the fc towers, 4 MB of weights against a few hundred rows -- as ONE forward and ONE backward call
    (csrc/ph_qtrain.hip: fp32-MFMA job tables, 19 + 21 launches), the two dynamic convolutions; `feat_transform` is folded
    as in the inference path (pooling and the dynamic convolution are linear in it), gradients included;
  * `_Upsample2x`; `_Objective`: a head's or stage's losses with d(losses)/d(predictions) from the loss kernels
    (csrc/ph_loss.hip);
  * in front of the neck, on request (`fpn_forward_train`, `VideoTrainStep(fpn=...)`): the FPN as `_Lateral`, `_NearestUpAdd` and
    `_Conv3x3Bias` nodes (csrc/ph_fpntrain.hip), so that the step starts at the backbone stages and ends with their gradients;
  * the discrete parts (Hungarian assignment -- scipy on the host, or `device_assign`: csrc/ph_assign.hip --, targets) in between.

The result is checked against the reference's own forward + autograd backward (tests/golden/train_step.npz:
every loss, the objective and the gradient of every parameter and of the three input maps)."""
import ctypes as C
import types
import weakref

import torch

from . import _lib, engine as E, losses as Lo

LN_EPS = 1e-5
BIN_THR = 1.5 * 2.0 ** -24          # sigmoid(z) > 0.5 in fp32 (csrc/ph_common.h PH_BIN_THR)


def _gpu32(t, name):
    Lo._gpu(t, name)
    return t.detach().contiguous().float()


def _param32(p, name="parameter"):
    """a parameter whose storage a kernel reads through a raw pointer: fp32, contiguous, on the GPU -- anything else would be read as
    fp32 garbage with no error (a head cast to half / bf16, a non-contiguous view), so it is refused"""
    Lo._gpu(p, name)
    if p.dtype != torch.float32 or not p.is_contiguous():
        raise _lib.PolyheadError(f"training forward: fp32 contiguous parameters only ({name}: {p.dtype}, contiguous={p.is_contiguous()})")
    return p.detach()


# Test aid (None in production): `hard_mask_hook(site, logits) -> logits` is consulted wherever the training forward is about to
# BINARISE mask logits for pooling -- site = the KernelHead module or the KernelUpdateHead stage module.  The tests hand the
# reference's hard decisions in (+-1 logits) so that a comparison with the reference's gradients measures arithmetic, not a logit
# that sits within rounding of the threshold (the inference tests do the converse: the oracle follows the device's hard masks).
hard_mask_hook = None


# ---- raw calls -------------------------------------------------------------------------------------------------------------
def rows_x_map(A, X, binarize_x=False, bias=None, out=None, accumulate=False, add=None):
    """Y[b, m, p] = sum_k A[b, m, k] X[b, k, p] (+ bias[b, m]) (+ add[b, m, p]);  A [B or 1, M, K], X [B, K, *spatial] ->
    [B, M, *spatial].  `out` + accumulate: Y += (a gradient contribution added where an earlier one already lies)"""
    X = _gpu32(X, "X")
    B, K = X.shape[:2]
    HW = X[0, 0].numel()
    Ab, M, Ka = A.shape
    assert Ka == K and Ab in (1, B), (A.shape, X.shape)
    Mpad, lda = (M + 15) // 16 * 16, (K + 7) // 8 * 8
    if Mpad == M and lda == K and A.is_contiguous() and A.dtype == torch.float32:
        Ap = A.detach()
    else:
        Ap = torch.zeros((Ab, Mpad, lda), dtype=torch.float32, device=X.device)
        Ap[:, :M, :K] = A.detach()
    Y = torch.empty((B, M) + tuple(X.shape[2:]), dtype=torch.float32, device=X.device) if out is None else out
    assert Y.is_contiguous() and Y.numel() == B * M * HW and (out is not None or not accumulate) and not (accumulate and add is not None)
    if accumulate:
        add = Y
    elif add is not None:
        add = _gpu32(add, "add")
        assert add.numel() == Y.numel()
    if bias is not None:
        bias = bias.detach().contiguous().float()
        assert bias.numel() == B * M
    _lib.check(_lib.load().ph_rows_x_map_ex(_lib.ptr(Ap), Mpad * lda if Ab > 1 else 0, lda, Mpad, M, K, _lib.ptr(X), _lib.ptr(Y), B, HW,
                                            int(binarize_x), _lib.ptr(bias), _lib.ptr(add), _lib.stream_ptr()), "ph_rows_x_map")
    return Y


def map_x_mapT(G, X, binarize_g=False, out=None, rowsum=None, sum_batch=False):
    """O[b, m, k] = sum_p G[b, m, p] X[b, k, p];  G [B, M, *spatial], X [B, K, *spatial] -> [B, M, K].
    rowsum [B, M] (optional): sum_p G[b, m, p] from the same pass (binarised: the hard masks' pixel counts).
    sum_batch: summed over the images too -> [M, K] / rowsum [M] (the gradient of a static kernel and of its bias)"""
    G, X = _gpu32(G, "G"), _gpu32(X, "X")
    B, M = G.shape[:2]
    K = X.shape[1]
    HW = X[0, 0].numel()
    assert G[0, 0].numel() == HW and X.shape[0] == B
    lib = _lib.load()
    ns = lib.ph_map_x_map_t_nsplit(B, M, HW)
    part = torch.empty((B, ns, M, K), dtype=torch.float32, device=X.device)
    Bo = 1 if sum_batch else B
    if out is None:
        out = torch.empty((M, K) if sum_batch else (B, M, K), dtype=torch.float32, device=X.device)
    assert out.is_contiguous() and out.numel() == Bo * M * K
    rsp = None
    if rowsum is not None:
        assert rowsum.is_contiguous() and rowsum.numel() == Bo * M and rowsum.dtype == torch.float32
        rsp = torch.empty((B, ns, M), dtype=torch.float32, device=X.device)
    _lib.check(lib.ph_map_x_map_t_ex(_lib.ptr(G), _lib.ptr(X), _lib.ptr(part), _lib.ptr(out), B, M, K, HW, ns, int(binarize_g),
                                    _lib.ptr(rsp), _lib.ptr(rowsum), int(sum_batch), _lib.stream_ptr()), "ph_map_x_map_t")
    return out


def pool_hard_counts(m, x, dfe, pooled, cnt):
    """pooled[0] = sum_p M x, pooled[1] = sum_p M depth_feats (M = the hard masks of the logits m), cnt = pixels per mask:
    kernel_update_head.py:236-242 with feat_transform folded out (train._Stage)"""
    map_x_mapT(m, x, binarize_g=True, out=pooled[0], rowsum=cnt)
    map_x_mapT(m, dfe, binarize_g=True, out=pooled[1])


# ---- differentiable map-sized operations -------------------------------------------------------------------------------------
class _Upsample2x(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return E.upsample2x(_gpu32(t, "t"))

    @staticmethod
    def backward(ctx, g):
        g = _gpu32(g, "g")
        B, N, H2, W2 = g.shape
        out = torch.empty((B, N, H2 // 2, W2 // 2), dtype=torch.float32, device=g.device)
        _lib.check(_lib.load().ph_upsample2x_bwd(_lib.ptr(g), _lib.ptr(out), B * N, H2 // 2, W2 // 2, _lib.stream_ptr()),
                   "ph_upsample2x_bwd")
        return out


class _Objective(torch.autograd.Function):
    """The loss kernels as one differentiable scalar: forward evaluates `fn(*preds)` -> (dict of losses, dict of
    d(sum of the 'loss' entries) / d(pred)); backward hands the stored gradients on, scaled by the incoming one."""

    @staticmethod
    def forward(ctx, fn, box, *preds):
        losses, grads = fn(*[p.detach() for p in preds])
        box.update(losses)
        ctx.save_for_backward(*grads)
        total = sum(v.double() for k, v in losses.items() if "loss" in k)
        return total.float()

    @staticmethod
    def backward(ctx, g):
        return (None, None) + tuple(None if t is None else g * t for t in ctx.saved_tensors)      # no depth items: no depth gradient


upsample2x = _Upsample2x.apply


# ---- one KernelUpdateHead stage: ONE autograd node, forward and backward in libpolyhead ---------------------------------------
def _qt_names():
    """parameter names in the order of include/polyhead.h's PH_QTRAIN table: (mask branch [44], depth branch [39])"""
    def upd(u):
        return [f"{u}.dynamic_layer.weight", f"{u}.dynamic_layer.bias", f"{u}.input_layer.weight", f"{u}.input_layer.bias",
                f"{u}.input_gate.weight", f"{u}.input_gate.bias", f"{u}.update_gate.weight", f"{u}.update_gate.bias",
                f"{u}.input_norm_in.weight", f"{u}.input_norm_in.bias", f"{u}.norm_in.weight", f"{u}.norm_in.bias",
                f"{u}.norm_out.weight", f"{u}.norm_out.bias", f"{u}.input_norm_out.weight", f"{u}.input_norm_out.bias",
                f"{u}.fc_layer.weight", f"{u}.fc_layer.bias", f"{u}.fc_norm.weight", f"{u}.fc_norm.bias"]

    def rest(sfx):
        return [f"attention{sfx}.attn.in_proj_weight", f"attention{sfx}.attn.in_proj_bias", f"attention{sfx}.attn.out_proj.weight",
                f"attention{sfx}.attn.out_proj.bias", f"attention_norm{sfx}.weight", f"attention_norm{sfx}.bias",
                f"ffn{sfx}.layers.0.0.weight", f"ffn{sfx}.layers.0.0.bias", f"ffn{sfx}.layers.1.weight", f"ffn{sfx}.layers.1.bias",
                f"ffn_norm{sfx}.weight", f"ffn_norm{sfx}.bias"]
    mask = (["feat_transform.conv.weight", "feat_transform.conv.bias"] + upd("kernel_update_conv") + rest("") +
            ["mask_fcs.0.weight", "mask_fcs.1.weight", "mask_fcs.1.bias", "fc_mask.weight", "fc_mask.bias",
             "cls_fcs.0.weight", "cls_fcs.1.weight", "cls_fcs.1.bias", "fc_cls.weight", "fc_cls.bias"])
    depth = (["feat_depth_transform.conv.weight", "feat_depth_transform.conv.bias"] + upd("kernel_update_conv_depth") + rest("_depth") +
             ["depth_regs.0.weight", "depth_regs.1.weight", "depth_regs.1.bias", "fc_depth.weight", "fc_depth.bias"])
    return mask, depth


QT_MASK_NAMES, QT_DEPTH_NAMES = _qt_names()
QT_NPARAM = 44
assert len(QT_MASK_NAMES) == QT_NPARAM and len(QT_DEPTH_NAMES) == 39


def _ptr_table(tensors_mask, tensors_depth):
    """HOST array [2][44] of device pointers (the depth branch has no classification tower: 5 nulls)"""
    arr = (C.c_void_p * (2 * QT_NPARAM))()
    for i, t in enumerate(tensors_mask):
        arr[i] = t.data_ptr()
    for i, t in enumerate(tensors_depth):
        arr[QT_NPARAM + i] = t.data_ptr()
    return arr


_QT_SCRATCH = {}


def _qt_scratch(dev, n):
    """the backward's scratch (a few tens of MB): one buffer per device, reused by every stage and step -- the stages'
    backwards run one after the other on the same stream"""
    t = _QT_SCRATCH.get(dev)
    if t is None or t.numel() < n:
        t = _QT_SCRATCH[dev] = torch.empty((n,), dtype=torch.float32, device=dev)
    return t


class _Stage(torch.autograd.Function):
    """KernelUpdateHead.forward (kernel_update_head.py:212-353) in training form as ONE autograd node: hard-mask pooling of
    x / depth_feats (`ph_map_x_map_t`, feat_transform folded), the whole query side (`ph_qtrain_forward`: updators, attention,
    FFN, towers -- csrc/ph_qtrain.hip), the two dynamic convolutions (`ph_rows_x_map`); backward likewise
    (`ph_qtrain_backward` + the transposed map products).  No gradient through the hard masks (piecewise constant)."""

    @staticmethod
    def forward(ctx, meta, x, dfe, k, m, q, *params):
        lib = _lib.load()
        x, dfe, m = _gpu32(x, "x"), _gpu32(dfe, "depth_feats"), _gpu32(m, "mask_preds")
        if hard_mask_hook is not None:
            m = _gpu32(hard_mask_hook(meta["module"](), m), "mask_preds")
        k, q = _gpu32(k, "proposal_feat"), _gpu32(q, "depth_proposal")
        params = [p.detach() for p in params]
        pm, pd = params[:QT_NPARAM], params[QT_NPARAM:]
        B, N, Cc = k.shape
        L, F = meta["L"], meta["F"]
        dev, R = x.device, B * N
        pooled = torch.empty((2, B, N, Cc), dtype=torch.float32, device=dev)
        cnt = torch.empty((B, N), dtype=torch.float32, device=dev)
        pool_hard_counts(m, x, dfe, pooled, cnt)
        cls = torch.empty((B, N, L), dtype=torch.float32, device=dev)
        kern = torch.empty((2, B, N, Cc), dtype=torch.float32, device=dev)
        kbias = torch.empty((2, B, N), dtype=torch.float32, device=dev)
        obj = torch.empty((2, B, N, Cc), dtype=torch.float32, device=dev)
        saved = torch.empty((lib.ph_qtrain_saved_floats(B, N, L, F),), dtype=torch.float32, device=dev)
        ptab = _ptr_table(pm, pd)
        _lib.check(lib.ph_qtrain_forward(ptab, _lib.ptr(pooled), _lib.ptr(cnt), _lib.ptr(k), _lib.ptr(q), _lib.ptr(cls), _lib.ptr(kern),
                                         _lib.ptr(kbias), _lib.ptr(obj), _lib.ptr(saved), B, N, L, F, _lib.stream_ptr()),
                   "ph_qtrain_forward")
        mask = rows_x_map(kern[0], x, bias=kbias[0])                   # = conv(feat_transform(x), fc_mask(...)) (:317-322)
        depth = rows_x_map(kern[1], dfe, bias=kbias[1])
        ctx.meta, ctx.params = meta, params
        ctx.save_for_backward(x, dfe, m, k, q, pooled, cnt, kern, saved)
        return cls, mask, obj[0], depth, obj[1]

    @staticmethod
    def backward(ctx, gcls, gmask, gobj, gdepth, gdobj):
        lib = _lib.load()
        x, dfe, m, k, q, pooled, cnt, kern, saved = ctx.saved_tensors
        params, meta = ctx.params, ctx.meta
        pm, pd = params[:QT_NPARAM], params[QT_NPARAM:]
        B, N, Cc = k.shape
        L, F = meta["L"], meta["F"]
        dev = x.device
        gmask, gdepth = _gpu32(gmask, "grad"), _gpu32(gdepth, "grad")
        # the dynamic convolutions: d kernels (+ d bias = row sums of the map gradient), d maps
        gkern = torch.empty((2, B, N, Cc), dtype=torch.float32, device=dev)
        gkbias = torch.empty((2, B, N), dtype=torch.float32, device=dev)
        map_x_mapT(gmask, x, out=gkern[0], rowsum=gkbias[0])
        map_x_mapT(gdepth, dfe, out=gkern[1], rowsum=gkbias[1])
        need_x, need_d = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        gx = rows_x_map(kern[0].transpose(1, 2), gmask) if need_x else None
        gd = rows_x_map(kern[1].transpose(1, 2), gdepth) if need_d else None
        gobj2 = torch.stack([_gpu32(gobj, "grad"), _gpu32(gdobj, "grad")], 0)
        # the query side
        sizes = meta["sizes"]
        gflat = torch.empty((meta["total"],), dtype=torch.float32, device=dev)
        gtab = (C.c_void_p * (2 * QT_NPARAM))()
        base = gflat.data_ptr()
        for i, off in enumerate(meta["offsets"]):
            if off >= 0:
                gtab[i] = base + 4 * off
        g_pooled = torch.empty_like(pooled)
        gk, gq = torch.empty_like(k), torch.empty_like(q)
        scratch = _qt_scratch(dev, lib.ph_qtrain_scratch_floats(B, N, L, F))
        _lib.check(lib.ph_qtrain_backward(_ptr_table(pm, pd), _lib.ptr(pooled), _lib.ptr(cnt), _lib.ptr(k), _lib.ptr(q), _lib.ptr(saved),
                                          _lib.ptr(_gpu32(gcls, "grad")), _lib.ptr(gkern), _lib.ptr(gkbias), _lib.ptr(gobj2), gtab,
                                          _lib.ptr(g_pooled), _lib.ptr(gk), _lib.ptr(gq), _lib.ptr(scratch), B, N, L, F,
                                          _lib.stream_ptr()), "ph_qtrain_backward")
        # the pooling: d map[c, p] += sum_n d pooled[n, c] M[n, p]
        if need_x:
            rows_x_map(g_pooled[0].transpose(1, 2), m, binarize_x=True, out=gx, accumulate=True)
        if need_d:
            rows_x_map(g_pooled[1].transpose(1, 2), m, binarize_x=True, out=gd, accumulate=True)
        pgrads = []
        for i, off in enumerate(meta["offsets"]):
            if off >= 0:
                pgrads.append(gflat[off:off + sizes[i]].view(meta["shapes"][i]))
        return (None, gx, gd, gk, None, gq) + tuple(pgrads)


def _stage_meta(head):
    """per-head constants of `_Stage`: parameter order, sizes and offsets of the flat gradient buffer (cached on the module)"""
    P = _lib.named_params(head)
    c = head.__dict__.get("_ph_stage_meta")
    plist = [P[n] for n in QT_MASK_NAMES] + [P[n] for n in QT_DEPTH_NAMES]
    key = tuple(id(p) for p in plist)
    if c is None or c["key"] != key:
        for p in plist:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise _lib.PolyheadError("training forward: fp32 contiguous parameters only")
        offsets, sizes, shapes, off = [], [], [], 0
        for i in range(2 * QT_NPARAM):
            j = i if i < QT_NPARAM else i - QT_NPARAM
            have = i < QT_NPARAM or j < len(QT_DEPTH_NAMES)
            if not have:
                offsets.append(-1); sizes.append(0); shapes.append(None)
                continue
            p = plist[i if i < QT_NPARAM else QT_NPARAM + j]
            offsets.append(off); sizes.append(p.numel()); shapes.append(tuple(p.shape))
            off += (p.numel() + 3) // 4 * 4
        c = dict(key=key, L=head.num_classes, F=P["ffn.layers.0.0.weight"].shape[0], offsets=offsets, sizes=sizes, shapes=shapes, total=off,
                 module=weakref.ref(head))
        if P["fc_cls.weight"].shape[0] != c["L"] or P["feat_transform.conv.weight"].shape[:2] != (256, 256) or head.attention.attn.num_heads != 8:
            raise NotImplementedError("training forward: 256 channels, 8 heads, fc_cls of num_classes rows (the shipped configuration)")
        head.__dict__["_ph_stage_meta"] = c
    return c, plist


def stage_forward(head, x, dfe, k, m, q):
    """KernelUpdateHead.forward (kernel_update_head.py:212-353) in training form.  x, dfe [B, C, H, W] (gradients flow),
    k / q [B, N, C] kernels and depth kernels, m [B, N, H, W] mask logits (used through the hard mask only).
    -> cls [B, N, L], mask [B, N, H, W], obj [B, N, C], depth [B, N, H, W], dobj [B, N, C]"""
    meta, plist = _stage_meta(head)
    return _Stage.apply(meta, x, dfe, k, m, q.expand_as(k), *plist)


# ---- KernelHead after the neck: ONE autograd node -----------------------------------------------------------------------------
def gn_relu_fwd(y, gamma, beta, groups, add=None, eps=1e-5, want_out=True):
    """relu(GroupNorm(y)) of a ConvModule, fp32 NCHW (`ph_gn_train_fwd`) -> (out, out + add or None, stats [B, groups, 2])"""
    lib = _lib.load()
    B, Cc = y.shape[:2]
    HW = y[0, 0].numel()
    out = torch.empty_like(y) if (want_out or add is None) else None
    osum = torch.empty_like(y) if add is not None else None
    stats = torch.empty((B, groups, 2), dtype=torch.float32, device=y.device)
    part = torch.empty((B * groups * lib.ph_gn_train_nsplit(HW, Cc // groups) * 2,), dtype=torch.float64, device=y.device)
    _lib.check(lib.ph_gn_train_fwd(_lib.ptr(y), _lib.ptr(gamma), _lib.ptr(beta), groups, eps, _lib.ptr(add), _lib.ptr(out), _lib.ptr(osum),
                                   _lib.ptr(stats), _lib.ptr(part), B, Cc, HW, _lib.stream_ptr()), "ph_gn_train_fwd")
    return out, osum, stats


def gn_relu_bwd(y, stats, gamma, beta, groups, dyA, dyB=None):
    """backward of `gn_relu_fwd` for dy = dyA (+ dyB) -> (dx, dgamma, dbeta)"""
    lib = _lib.load()
    B, Cc = y.shape[:2]
    HW = y[0, 0].numel()
    dx = torch.empty_like(y)
    dg = torch.empty((2, Cc), dtype=torch.float32, device=y.device)
    part = torch.empty((B * Cc * lib.ph_gn_train_bwd_nsplit(HW) * 2,), dtype=torch.float64, device=y.device)
    _lib.check(lib.ph_gn_train_bwd(_lib.ptr(y), _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta), groups, _lib.ptr(dyA), _lib.ptr(dyB),
                                   _lib.ptr(dx), _lib.ptr(dg[0]), _lib.ptr(dg[1]), _lib.ptr(part), B, Cc, HW, _lib.stream_ptr()),
               "ph_gn_train_bwd")
    return dx, dg[0], dg[1]


RPN_NAMES = ["loc_convs.0.conv.weight", "loc_convs.0.gn.weight", "loc_convs.0.gn.bias",
             "seg_convs.0.conv.weight", "seg_convs.0.gn.weight", "seg_convs.0.gn.bias",
             "depth_convs.0.conv.weight", "depth_convs.0.gn.weight", "depth_convs.0.gn.bias",
             "init_kernels.weight", "conv_seg.weight", "conv_seg.bias", "conv_direct_depth.weight", "conv_direct_depth.bias"]


class _Rpn(torch.autograd.Function):
    """KernelHead._decode_init_proposals after the neck (kernel_head.py:245-326), training form, as ONE autograd node: three
    1x1 conv + GroupNorm + ReLU towers (`ph_rows_x_map`, `ph_gn_train_fwd`), x = sem + loc from the same pass that normalises
    sem, the static 1x1 convs with their biases in the epilogue, the hard-mask pooling; backward by hand: every second gradient
    contribution enters a kernel as an operand (no map-sized ATen add), static-kernel gradients are summed over the batch inside
    the split reduction."""

    @staticmethod
    def forward(ctx, groups, site, f0, f1, f2, *params):
        f = [_gpu32(t, "post-neck map") for t in (f0, f1, f2)]
        P = [_param32(p, n) for p, n in zip(params, RPN_NAMES)]
        W = [P[0].flatten(1), P[3].flatten(1), P[6].flatten(1)]
        B = f[0].shape[0]
        y = [rows_x_map(W[t][None], f[t]) for t in range(3)]
        loc, _, st0 = gn_relu_fwd(y[0], P[1], P[2], groups)
        sem, x, st1 = gn_relu_fwd(y[1], P[4], P[5], groups, add=loc)                   # x = sem + loc (:303)
        dfe, _, st2 = gn_relu_fwd(y[2], P[7], P[8], groups)
        W_init, W_seg, w_dd = P[9].flatten(1), P[10].flatten(1), P[12].flatten(1)
        mask_preds = rows_x_map(W_init[None], loc)                                      # :256
        seg_preds = rows_x_map(W_seg[None], sem, bias=P[11][None].expand(B, -1))        # :295
        depth_pred = rows_x_map(w_dd[None], dfe, bias=P[13][None].expand(B, -1))        # :285
        hard_src = mask_preds if hard_mask_hook is None else _gpu32(hard_mask_hook(site, mask_preds), "mask_preds")
        proposal = map_x_mapT(hard_src, x, binarize_g=True)                             # :314-320 (use_binary)
        proposal += W_init[None]                                                        # :299-300,324-326
        ctx.groups, ctx.P = groups, P
        ctx.save_for_backward(f[0], f[1], f[2], y[0], y[1], y[2], st0, st1, st2, loc, sem, dfe, x, hard_src)
        return proposal, x, mask_preds, seg_preds, dfe, depth_pred

    @staticmethod
    def backward(ctx, g_prop, g_x, g_mp, g_seg, g_dfe, g_dp):
        f0, f1, f2, y0, y1, y2, st0, st1, st2, loc, sem, dfe, x, mask_preds = ctx.saved_tensors
        P, groups = ctx.P, ctx.groups
        g_prop, g_x, g_mp, g_seg, g_dfe, g_dp = [_gpu32(t, "grad") for t in (g_prop, g_x, g_mp, g_seg, g_dfe, g_dp)]
        W_init, W_seg, w_dd = P[9].flatten(1), P[10].flatten(1), P[12].flatten(1)
        # d / d x: what arrives + the pooling's share (d pooled^T M), in one pass; sem and loc both receive it
        gxs = rows_x_map(g_prop.transpose(1, 2), mask_preds, binarize_x=True, add=g_x)
        dy = [rows_x_map(W_init.t()[None], g_mp), rows_x_map(W_seg.t()[None], g_seg), rows_x_map(w_dd.t()[None], g_dp)]
        gy0, dg0, db0 = gn_relu_bwd(y0, st0, P[1], P[2], groups, dy[0], gxs)
        gy1, dg1, db1 = gn_relu_bwd(y1, st1, P[4], P[5], groups, dy[1], gxs)
        gy2, dg2, db2 = gn_relu_bwd(y2, st2, P[7], P[8], groups, dy[2], g_dfe)
        gW_init = map_x_mapT(g_mp, loc, sum_batch=True)
        gW_init += g_prop.sum(0)
        L = W_seg.shape[0]
        gb_seg = torch.empty((L,), dtype=torch.float32, device=x.device)
        gW_seg = map_x_mapT(g_seg, sem, rowsum=gb_seg, sum_batch=True)
        gb_dd = torch.empty((1,), dtype=torch.float32, device=x.device)
        gw_dd = map_x_mapT(g_dp, dfe, rowsum=gb_dd, sum_batch=True)
        gf, gW = [], []
        for t, (gy, ft) in enumerate(((gy0, f0), (gy1, f1), (gy2, f2))):
            gf.append(rows_x_map(P[3 * t].flatten(1).t()[None], gy) if ctx.needs_input_grad[2 + t] else None)
            gW.append(map_x_mapT(gy, ft, sum_batch=True).view(P[3 * t].shape))
        return (None, None, gf[0], gf[1], gf[2], gW[0], dg0, db0, gW[1], dg1, db1, gW[2], dg2, db2, gW_init.view(P[9].shape),
                gW_seg.view(P[10].shape), gb_seg, gw_dd.view(P[12].shape), gb_dd)


def rpn_forward(head, feats):
    """KernelHead._decode_init_proposals after the neck (kernel_head.py:245-336), training form (no stuff rows)"""
    P = _lib.named_params(head)
    plist = [P[n] for n in RPN_NAMES]
    groups = head.norm_cfg.get("num_groups", 32)
    proposal, x, mask_preds, seg_preds, dfe, depth_pred = _Rpn.apply(groups, head, feats[0], feats[1], feats[2], *plist)
    B = x.shape[0]
    depth_proposal = P["conv_direct_depth.weight"].flatten(1)[None].expand(B, 1, -1)           # :286-289
    return dict(proposal=proposal, x=x, mask_preds=mask_preds, seg_preds=seg_preds, dfe=dfe, depth_proposal=depth_proposal,
                depth_pred=depth_pred)


# ---- SemanticFPNWrapper in training: the neck's forward as differentiable libpolyhead nodes (round 5) ------------------------------
class _Conv3x3(torch.autograd.Function):
    """F.conv2d(X, W [M, K, 3, 3], stride, padding 1) on `ph_conv3x3_train` (nine shifted rows-x-map products); backward: the input
    gradient is the same kernel on flipped / transposed taps (stride 2: its transposed-stride mode), the weight gradient nine
    shifted map x map^T products summed over the batch (`ph_conv3x3_wgrad`)"""

    @staticmethod
    def _taps(W, transpose, flip):
        M, K = W.shape[:2]
        t = torch.empty((9, K, M) if transpose else (9, M, K), dtype=torch.float32, device=W.device)
        _lib.check(_lib.load().ph_conv3x3_taps(_lib.ptr(W), _lib.ptr(t), M, K, int(transpose), int(flip), 0, _lib.stream_ptr()), "ph_conv3x3_taps")
        return t

    @staticmethod
    def forward(ctx, X, W, stride):
        X, Wd = _gpu32(X, "X"), _gpu32(W, "W")
        B, K, Hi, Wi = X.shape
        M = Wd.shape[0]
        Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
        Y = torch.empty((B, M, Ho, Wo), dtype=torch.float32, device=X.device)
        _lib.check(_lib.load().ph_conv3x3_train(_lib.ptr(_Conv3x3._taps(Wd, False, False)), M, K, _lib.ptr(X), _lib.ptr(Y), B, Hi, Wi, Ho, Wo,
                                                stride, 0, _lib.stream_ptr()), "ph_conv3x3_train")
        ctx.stride = stride
        ctx.save_for_backward(X, Wd)
        return Y

    @staticmethod
    def backward(ctx, gY):
        X, W = ctx.saved_tensors
        lib, s = _lib.load(), ctx.stride
        gY = _gpu32(gY, "grad")
        B, K, Hi, Wi = X.shape
        M, Ho, Wo = W.shape[0], gY.shape[2], gY.shape[3]
        gX = gW = None
        if ctx.needs_input_grad[0]:
            # the kernel writes whole 16-row tiles of its output channels -- here the conv's INPUT channels: K % 16 != 0 (the forward
            # only asks for K % 8 == 0) runs on zero-padded taps into a padded gradient (the shipped 256-channel towers never do)
            Kp = (K + 15) // 16 * 16
            taps = _Conv3x3._taps(W, True, s == 1)
            if Kp != K:
                padded = torch.zeros((9, Kp, M), dtype=torch.float32, device=X.device)
                padded[:, :K] = taps
                taps = padded
            gX = torch.empty((B, Kp, Hi, Wi), dtype=torch.float32, device=X.device)
            if s == 1:
                _lib.check(lib.ph_conv3x3_train(_lib.ptr(taps), Kp, M, _lib.ptr(gY), _lib.ptr(gX), B, Ho, Wo, Hi, Wi, 1, 0,
                                                _lib.stream_ptr()), "ph_conv3x3_train(dgrad)")
            else:
                _lib.check(lib.ph_conv3x3_train(_lib.ptr(taps), Kp, M, _lib.ptr(gY), _lib.ptr(gX), B, Ho, Wo, Hi, Wi, 2, 1,
                                                _lib.stream_ptr()), "ph_conv3x3_train(dgrad, stride 2)")
            if Kp != K:
                gX = gX[:, :K].contiguous()
        if ctx.needs_input_grad[1]:
            ns = lib.ph_map_x_map_t_nsplit(B, M, Ho * Wo)
            part = torch.empty((B, ns, M, K), dtype=torch.float32, device=X.device)
            taps = torch.empty((9, M, K), dtype=torch.float32, device=X.device)
            _lib.check(lib.ph_conv3x3_wgrad(_lib.ptr(gY), _lib.ptr(X), _lib.ptr(part), _lib.ptr(taps), B, M, K, Hi, Wi, Ho, Wo, s, ns,
                                            _lib.stream_ptr()), "ph_conv3x3_wgrad")
            gW = torch.empty_like(W)
            _lib.check(lib.ph_conv3x3_taps(_lib.ptr(gW), _lib.ptr(taps), M, K, 0, 0, 1, _lib.stream_ptr()), "ph_conv3x3_taps")
        return gX, gW, None


class _GNReLU(torch.autograd.Function):
    """relu(GroupNorm(y)) (+ add: the running sum over the neck's towers, semantic_fpn.py:217-220) -- csrc/ph_gntrain.hip"""

    @staticmethod
    def forward(ctx, y, gamma, beta, groups, add):
        y = _gpu32(y, "y")
        g, b = _param32(gamma, "GroupNorm weight"), _param32(beta, "GroupNorm bias")
        out, osum, stats = gn_relu_fwd(y, g, b, groups, add=None if add is None else _gpu32(add, "add"), want_out=False)
        ctx.groups, ctx.has_add = groups, add is not None
        ctx.save_for_backward(y, stats, g, b)
        return out if add is None else osum

    @staticmethod
    def backward(ctx, gout):
        y, stats, g, b = ctx.saved_tensors
        gout = _gpu32(gout, "grad")
        dx, dg, db = gn_relu_bwd(y, stats, g, b, ctx.groups, gout)
        return dx, dg, db, None, (gout if ctx.has_add else None)


class _NeckOuts(torch.autograd.Function):
    """conv_pred + the aux convs (semantic_fpn.py:152-178, 222-229): 1x1 conv + GroupNorm + ReLU each, on the tower sum; backward
    in one node so that the three input-gradient contributions land in ONE buffer (the second and third as the product's add source)"""

    @staticmethod
    def forward(ctx, groups, s, *params):
        s = _gpu32(s, "tower sum")
        P = [_param32(p, "neck output conv parameter") for p in params]
        n = len(P) // 3
        ys, sts, outs = [], [], []
        for j in range(n):
            y = rows_x_map(P[3 * j].flatten(1)[None], s)
            o, _, st = gn_relu_fwd(y, P[3 * j + 1], P[3 * j + 2], groups)
            ys.append(y); sts.append(st); outs.append(o)
        ctx.groups, ctx.P, ctx.n = groups, P, n
        ctx.save_for_backward(s, *ys, *sts)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gouts):
        sv = ctx.saved_tensors
        P, n, s = ctx.P, ctx.n, sv[0]
        ys, sts = sv[1:1 + n], sv[1 + n:1 + 2 * n]
        gs, grads = None, []
        for j in range(n):
            gy, dg, db = gn_relu_bwd(ys[j], sts[j], P[3 * j + 1], P[3 * j + 2], ctx.groups, _gpu32(gouts[j], "grad"))
            if ctx.needs_input_grad[1]:
                W = P[3 * j].flatten(1)
                gs = rows_x_map(W.t()[None], gy) if gs is None else rows_x_map(W.t()[None], gy, out=gs, accumulate=True)
            grads += [map_x_mapT(gy, s, sum_batch=True).view(P[3 * j].shape), dg, db]
        return (None, gs) + tuple(grads)


def neck_forward_train(neck, inputs):
    """SemanticFPNWrapper.forward (funcs/semantic_fpn.py:198-235) for the shipped configuration, every operation a differentiable
    libpolyhead node: per level 3x3 conv (level 0: stride 2) + GroupNorm + ReLU, x2 bilinear upsamples in between, the towers'
    outputs summed inside the last GroupNorm pass of each level, conv_pred / aux convs.  fp32 NCHW, the reference's arithmetic
    (products on hi + lo bf16 MFMA like the heads' map products).  Gradients flow to every parameter and to the four FPN inputs."""
    G = neck.groups
    total = None
    for lvl, level in enumerate(neck.convs_all_levels):
        t = inputs[lvl].float()
        if lvl == neck.cat_coors_level and neck.pos_cfg is not None:
            t = t + neck._posenc(t.shape[-2], t.shape[-1], t.device)[None]                    # semantic_fpn.py:202-209
        for j in range(level.n):
            m = getattr(level, f"conv{j}")
            y = _Conv3x3.apply(t, m.conv.weight, m.stride)
            last = j == level.n - 1
            t = _GNReLU.apply(y, m.gn.weight, m.gn.bias, G, total if (last and total is not None) else None)
            if not last:                              # levels 2, 3: an x2 upsample follows every conv but the last (:117-150)
                t = upsample2x(t)
        total = t
    outs = [neck.conv_pred] + list(neck.aux_convs)
    plist = []
    for m in outs:
        plist += [m.conv.weight, m.gn.weight, m.gn.bias]
    res = _NeckOuts.apply(G, total, *plist)
    return list(res)


# ---- FPN in training: backbone stages -> the four pyramid levels as differentiable libpolyhead nodes (csrc/ph_fpntrain.hip) ------
def map_x_mapT_wide(G, X, out=None, rowsum=None, sum_batch=False):
    """`map_x_mapT` without binarisation for K up to 4096 (`ph_map_x_map_t_wide`: K tiles of 256 columns); for K <= 256 the same bits"""
    G, X = _gpu32(G, "G"), _gpu32(X, "X")
    B, M = G.shape[:2]
    K = X.shape[1]
    HW = X[0, 0].numel()
    assert G[0, 0].numel() == HW and X.shape[0] == B
    lib = _lib.load()
    ns = lib.ph_map_x_map_t_wide_nsplit(B, M, K, HW)
    part = torch.empty((B, ns, M, K), dtype=torch.float32, device=X.device)
    Bo = 1 if sum_batch else B
    if out is None:
        out = torch.empty((M, K) if sum_batch else (B, M, K), dtype=torch.float32, device=X.device)
    assert out.is_contiguous() and out.numel() == Bo * M * K and out.dtype == torch.float32
    rsp = None
    if rowsum is not None:
        assert rowsum.is_contiguous() and rowsum.numel() == Bo * M and rowsum.dtype == torch.float32
        rsp = torch.empty((B, ns, M), dtype=torch.float32, device=X.device)
    _lib.check(lib.ph_map_x_map_t_wide(_lib.ptr(G), _lib.ptr(X), _lib.ptr(part), _lib.ptr(out), B, M, K, HW, ns, _lib.ptr(rsp),
                                       _lib.ptr(rowsum), int(sum_batch), _lib.stream_ptr()), "ph_map_x_map_t_wide")
    return out


def nearest_up_add(fine, coarse):
    """in place: fine += F.interpolate(coarse, size=fine.shape[2:], mode='nearest'); both fp32 contiguous [B, C, h, w] on the GPU"""
    (B, Cn, H, W), (Hc, Wc) = fine.shape, coarse.shape[2:]
    assert fine.is_contiguous() and coarse.is_contiguous() and fine.dtype == coarse.dtype == torch.float32 and coarse.shape[:2] == (B, Cn)
    _lib.check(_lib.load().ph_nearest_up_add(_lib.ptr(fine), _lib.ptr(coarse), B * Cn, H, W, Hc, Wc, _lib.stream_ptr()), "ph_nearest_up_add")
    return fine


def nearest_up_add_bwd(g_fine, g_coarse, accumulate=True):
    """the transpose of `nearest_up_add`: g_coarse (+)= the sum of its up to four fine pixels, gathered in a fixed order"""
    (B, Cn, H, W), (Hc, Wc) = g_fine.shape, g_coarse.shape[2:]
    assert g_fine.is_contiguous() and g_coarse.is_contiguous() and g_fine.dtype == g_coarse.dtype == torch.float32
    assert g_coarse.shape[:2] == (B, Cn)
    _lib.check(_lib.load().ph_nearest_up_add_bwd(_lib.ptr(g_fine), _lib.ptr(g_coarse), B * Cn, H, W, Hc, Wc, int(accumulate),
                                                 _lib.stream_ptr()), "ph_nearest_up_add_bwd")
    return g_coarse


def nchw_bias_add(y, bias):
    """in place: y[b, c] += bias[c]"""
    B, Cn = y.shape[:2]
    assert y.is_contiguous() and y.dtype == torch.float32 and bias.is_contiguous() and bias.dtype == torch.float32 and bias.numel() == Cn
    _lib.check(_lib.load().ph_nchw_bias_add(_lib.ptr(y), _lib.ptr(bias), B, Cn, y[0, 0].numel(), _lib.stream_ptr()), "ph_nchw_bias_add")
    return y


def nchw_channel_sums(g):
    """[C]: sum over images and pixels of g [B, C, *spatial], accumulated in fp64 in a fixed order"""
    g = _gpu32(g, "g")
    B, Cn = g.shape[:2]
    HW = g[0, 0].numel()
    lib = _lib.load()
    part = torch.empty((Cn, B, lib.ph_nchw_channel_sums_nsplit(HW)), dtype=torch.float64, device=g.device)
    out = torch.empty((Cn,), dtype=torch.float32, device=g.device)
    _lib.check(lib.ph_nchw_channel_sums(_lib.ptr(g), _lib.ptr(part), _lib.ptr(out), B, Cn, HW, _lib.stream_ptr()), "ph_nchw_channel_sums")
    return out


class _Lateral(torch.autograd.Function):
    """F.conv2d(X, W [M, K, 1, 1], bias) (fpn.py:158-161): `ph_rows_x_map_ex` with the bias in its epilogue; backward: the input
    gradient is the same product on W^T (only where the stage asks for one), the weight and bias gradients ONE wide map x map^T
    pass over (dL/dY, X) summed over the batch"""

    @staticmethod
    def forward(ctx, X, W, bias):
        X, Wd, bd = _gpu32(X, "X"), _param32(W, "lateral conv weight"), _param32(bias, "lateral conv bias")
        B = X.shape[0]
        Y = rows_x_map(Wd.flatten(1)[None], X, bias=bd[None].expand(B, -1))
        ctx.save_for_backward(X, Wd)
        return Y

    @staticmethod
    def backward(ctx, gY):
        X, W = ctx.saved_tensors
        gY = _gpu32(gY, "grad")
        gX = gW = gb = None
        if ctx.needs_input_grad[0]:
            gX = rows_x_map(W.flatten(1).t()[None], gY)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            gb = torch.empty((W.shape[0],), dtype=torch.float32, device=X.device)
            gW = map_x_mapT_wide(gY, X, rowsum=gb, sum_batch=True).view(W.shape)
        return gX, gW, gb


class _NearestUpAdd(torch.autograd.Function):
    """the top-down pathway (fpn.py:164-175) on the four lateral maps, in place: level i - 1 += nearest(level i), from the coarsest
    down.  Backward runs the other way, from level 0 up: each coarse level's own gradient takes the gather of the (finished) finer
    one's, so the four results are the gradients of the four laterals and nothing is added outside the kernel."""

    @staticmethod
    def forward(ctx, *lat):
        for i in range(len(lat) - 1, 0, -1):
            nearest_up_add(lat[i - 1], lat[i])
        ctx.mark_dirty(*lat[:-1])
        return lat

    @staticmethod
    def backward(ctx, *gs):
        gs = [_gpu32(g, "grad") for g in gs]
        out = [gs[0]]
        for i in range(1, len(gs)):
            out.append(nearest_up_add_bwd(out[i - 1], gs[i].clone(), accumulate=True))
        return tuple(out)


class _Conv3x3Bias(torch.autograd.Function):
    """an FPN output convolution (fpn.py:177-179): `_Conv3x3` at stride 1 with the bias added in place behind it; the bias gradient
    is the channel sums of dL/dY"""

    @staticmethod
    def forward(ctx, X, W, bias):
        bd = _param32(bias, "output conv bias")
        return nchw_bias_add(_Conv3x3.forward(ctx, X, _param32(W, "output conv weight"), 1), bd)

    @staticmethod
    def backward(ctx, gY):
        gX, gW, _ = _Conv3x3.backward(ctx, gY)
        return gX, gW, (nchw_channel_sums(gY) if ctx.needs_input_grad[2] else None)


def fpn_forward_train(fpn, stages):
    """fpn.FPN.forward (mmdet/models/necks/fpn.py:151-203) for the shipped structure, every operation a differentiable libpolyhead
    node: four lateral 1x1 convolutions with bias, the nearest top-down add, four 3x3 output convolutions with bias.  fp32 NCHW,
    products on hi + lo bf16 MFMA like the neck's.  Gradients flow to the 16 parameters and to the stages that require one.
    -> the four levels, a tuple"""
    if len(stages) != len(fpn.lateral_convs):
        raise _lib.PolyheadError(f"fpn_forward_train: {len(fpn.lateral_convs)} stages, got {len(stages)}")
    for i, t in enumerate(stages):
        Lo._gpu(t, f"inputs[{i}]")
    for n, p in fpn.named_parameters():
        _param32(p, n)
    lat = [_Lateral.apply(stages[i].float(), m.conv.weight, m.conv.bias) for i, m in enumerate(fpn.lateral_convs)]
    lat = _NearestUpAdd.apply(*lat)
    return tuple(_Conv3x3Bias.apply(lat[i], m.conv.weight, m.conv.bias) for i, m in enumerate(fpn.fpn_convs))


# ---- the backbone in training: the image -> the stages, the stage gradients -> the gradients of the trained parameters -------------
def _resnet_train_state(backbone, img):
    """the refusals of the device training path, then (plan, forward pack, transposed packs, image as the plan takes it)"""
    def no(arg, why):
        raise NotImplementedError(f"resnet_forward_train: {arg}: the device training path covers the shipped backbone ({why})")
    if backbone.frozen_stages < 1:
        no("frozen_stages", "frozen_stages >= 1: the stem and layer1 have no backward")
    if not backbone.norm_eval:
        no("norm_eval", "norm_eval=True: BatchNorm in training mode is not built")
    if backbone.precision != "bf16":
        no("precision", "grade 'bf16': fp16 would need loss scaling, which does not exist here")
    if img.requires_grad:
        no("img", "an input image that requires grad: no gradient is returned for the image")
    if any(m.training for m in backbone.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)):
        no("norm_eval", "every BatchNorm in eval mode (ResNet.train() leaves them there)")
    E._require_gpu(img, "img")
    if img.dim() != 4 or img.shape[1] != 3:
        raise _lib.PolyheadError("resnet_forward_train: img must be [B, 3, H, W]")
    eps = {m.eps for m in backbone.modules() if isinstance(m, torch.nn.BatchNorm2d)}
    if len(eps) != 1:
        raise _lib.PolyheadError("resnet_forward_train: ph_resnet_cfg carries one BatchNorm eps; this module's norms have several")
    dev, (B, _, H, W) = img.device, img.shape
    st = backbone.__dict__.setdefault("_train_state", dict(packs={}, plans={}))
    with torch.cuda.device(dev):
        key = (str(dev), backbone._versions())
        if key not in st["packs"]:
            st["packs"].clear()
            cfg = E.native_resnet_cfg(B, H, W, backbone.depth, "bf16", torch.float32, torch.float32, (0, 1, 2, 3), eps.pop())
            pack = E.native_resnet_pack(backbone, cfg, dev)
            st["packs"][key] = (pack, E.native_resnet_pack_bwd(pack))
        pack, wt = st["packs"][key]
        pkey = (B, H, W, str(dev), tuple(backbone.out_indices), backbone.frozen_stages, tuple(map(tuple, backbone.block_table())))
        plan = st["plans"].get(pkey)
        if plan is None:
            if len(st["plans"]) >= 2:                    # a training plan keeps every activation of its size
                st["plans"].clear()
            plan = st["plans"][pkey] = E.ResNetTrainPlan(B, H, W, backbone.block_table(), backbone.out_indices, backbone.frozen_stages, dev)
    return plan, pack.pk, wt, img.contiguous() if img.dtype in (torch.float32, torch.bfloat16) else img.contiguous().float()


def _resnet_trained(backbone):
    """[(key, conv, bn)] of the trained convolutions in the plan's order, key = (stage, block, name)"""
    out = []
    for si in range(backbone.frozen_stages, 4):
        for j, m in enumerate(getattr(backbone, backbone.res_layers[si])):
            out += [((si, j, "conv1"), m.conv1, m.bn1), ((si, j, "conv2"), m.conv2, m.bn2), ((si, j, "conv3"), m.conv3, m.bn3)]
            if m.downsample is not None:
                out.append(((si, j, "downsample"), m.downsample[0], m.downsample[1]))
    return out


class _ResNetStages(torch.autograd.Function):
    """resnet.ResNet's forward on engine.ResNetTrainPlan; backward: the stage gradients through the plan's backward.  The parameters
    are inputs for the graph's sake only (the forward reads the packs): per trained convolution its weight, its norm's weight and bias"""

    @staticmethod
    def forward(ctx, backbone, img, *params):
        plan, pk, wt, xin = _resnet_train_state(backbone, img)
        with torch.cuda.device(img.device):
            outs = plan.forward(xin, pk)
        ctx.backbone, ctx.plan, ctx.wt, ctx.generation = backbone, plan, wt, plan.generation
        return tuple(o.clone() for o in outs)

    @staticmethod
    def backward(ctx, *gs):
        backbone, plan = ctx.backbone, ctx.plan
        if plan.generation != ctx.generation:
            raise _lib.PolyheadError("resnet_forward_train: the plan ran another forward before this backward; its activations are gone")
        grads = {si: g.float().contiguous() for si, g in zip(backbone.out_indices, gs) if g is not None and si >= plan.first_trained}
        trained = _resnet_trained(backbone)
        f32 = lambda t: _param32(t.detach(), "backbone parameter")
        params = {key: (f32(c.weight), f32(bn.weight), f32(bn.running_mean), f32(bn.running_var), bn.eps,
                        bn.weight.requires_grad or bn.bias.requires_grad) for key, c, bn in trained}
        with torch.cuda.device(plan.device):
            out = plan.backward(grads, ctx.wt, params)
        res = []
        for i, (key, c, bn) in enumerate(trained):
            dw, dg, db = out[key]
            need = ctx.needs_input_grad[2 + 3 * i:5 + 3 * i]
            res += [dw.clone() if need[0] else None, dg.clone() if need[1] else None, db.clone() if need[2] else None]
        return (None, None) + tuple(res)


def resnet_forward_train(backbone, img):
    """resnet.ResNet.forward (mmdet/models/backbones/resnet.py:631-646) for training the stages behind the frozen ones on the device:
    the forward is the inference path's launch sequence with every activation kept (engine.ResNetTrainPlan; the folded weights are
    re-packed on the device whenever a parameter's or a running statistic's version changed), the backward takes the gradients of the
    stages -- a missing one is zeros, those of the frozen stages are ignored -- to the gradients of every trained conv.weight,
    bn.weight and bn.bias (csrc/ph_resnet_train.hip).  Scope: depth 50 / 101 / 152, frozen_stages >= 1, norm_eval=True, grade bf16, an
    image that does not require grad; anything else raises NotImplementedError naming the argument.  Returns the stages of
    out_indices as fp32 NCHW."""
    params = [p for _, c, bn in _resnet_trained(backbone) for p in (c.weight, bn.weight, bn.bias)]
    return _ResNetStages.apply(backbone, img, *params)


# ---- the video side: RoI features of the key frame and the track head's losses -------------------------------------------------
class _RoIExtract(torch.autograd.Function):
    """SingleRoIExtractor + RoIAlign(7, sampling_ratio 2, aligned) of one image (track_head.roi_extract, fp32 output); backward:
    `ph_roi_align_fpn_bwd`, a gather that writes every level's gradient in full"""

    @staticmethod
    def forward(ctx, rois, strides, finest_scale, *feats):
        from .track_head import roi_extract
        feats = [_gpu32(f, "FPN level") for f in feats]
        rois = _gpu32(rois, "rois")
        _, f32 = roi_extract(feats, rois, _lib.PH_PREC_BF16, strides, float(finest_scale), want_f32=True)
        ctx.shapes, ctx.strides, ctx.finest = [tuple(f.shape) for f in feats], tuple(strides), float(finest_scale)
        ctx.save_for_backward(rois)
        return f32

    @staticmethod
    def backward(ctx, g):
        rois, = ctx.saved_tensors
        g = _gpu32(g, "grad")
        L = len(ctx.shapes)
        outs = [torch.empty(s, dtype=torch.float32, device=g.device) for s in ctx.shapes]
        ptrs = (C.c_void_p * L)(*[o.data_ptr() for o in outs])
        hw = (C.c_int32 * (2 * L))(*[v for s in ctx.shapes for v in s[-2:]])
        sc = (C.c_float * L)(*[1.0 / s for s in ctx.strides[:L]])
        _lib.check(_lib.load().ph_roi_align_fpn_bwd(_lib.ptr(g), hw, sc, L, _lib.ptr(rois), rois.shape[0], ctx.finest, ptrs, _lib.stream_ptr()),
                   "ph_roi_align_fpn_bwd")
        return (None, None, None) + tuple(o if need else None for o, need in zip(outs, ctx.needs_input_grad[3:]))


def track_forward_train(track_head, feats, ref_feats, rois, ref_rois, key_gt_inds, ref_gt_inds, gt_match_indices, strides=(4, 8, 16, 32),
                        finest_scale=56):
    """The track branch of PolyphonicVideo.forward_train (polyphonic_former_video.py:245-319) after the boxes: per image i the RoI
    features of the key frame (feats[i]: its FPN levels [1, 256, H_l, W_l], gradients flow) and of the reference frame (ref_feats[i],
    from the no-grad pass: no gradient), the track head in its training form on all of them, `track_loss`.  rois[i] / ref_rois[i]:
    [n, 5] (0, x1, y1, x2, y2) -- the caller computes the boxes from its masks; key_gt_inds[i] / ref_gt_inds[i]: the RoIs'
    pos_assigned_gt_inds; gt_match_indices[i]: per key ground truth its index among the reference frame's or -1.
    -> {'loss_track', 'loss_track_aux'} attached to the graph."""
    from .track_head import roi_extract
    B = len(feats)
    if not (B == len(ref_feats) == len(rois) == len(ref_rois) == len(key_gt_inds) == len(ref_gt_inds) == len(gt_match_indices)) or B == 0:
        raise ValueError("track_forward_train: one entry per image in every list")
    with torch.enable_grad():
        key_x = [_RoIExtract.apply(rois[i], tuple(strides), finest_scale, *feats[i]) for i in range(B)]
        with torch.no_grad():
            ref_x = [roi_extract([f.detach() for f in ref_feats[i]], ref_rois[i], _lib.PH_PREC_BF16, strides, float(finest_scale), want_f32=True)[1]
                     for i in range(B)]
        nk = sum(t.shape[0] for t in key_x)
        emb = track_head.forward_train(torch.cat(key_x + ref_x))          # GroupNorm is per RoI: one pass for both frames
        ks = [types.SimpleNamespace(pos_assigned_gt_inds=torch.as_tensor(t)) for t in key_gt_inds]
        rs = [types.SimpleNamespace(pos_assigned_gt_inds=torch.as_tensor(t)) for t in ref_gt_inds]
        return track_head.track_loss(emb[:nk], emb[nk:], [torch.as_tensor(t) for t in gt_match_indices], ks, rs)


def gt_match_indices(gt_ids, ref_ids):
    """polyphonic_former_video.py:246-251 for one image: per key-frame ground truth the FIRST index of its instance id among the
    reference frame's ids, or -1 (`ref_ids.index(i) if i in ref_ids else -1`).  Integer torch on the ids' device -- a minimum over a
    masked index, not an argmax on ties --, nothing is downloaded.  -> int64 [len(gt_ids)]"""
    g = gt_ids.reshape(-1).long()
    r = ref_ids.reshape(-1).long().to(g.device)
    R = r.numel()
    if R == 0 or g.numel() == 0:
        return torch.full((g.numel(),), -1, dtype=torch.long, device=g.device)
    idx = torch.arange(R, device=g.device)[None].expand(g.numel(), R)
    first = torch.where(g[:, None] == r[None, :], idx, torch.full_like(idx, R)).min(dim=1).values
    return torch.where(first < R, first, torch.full_like(first, -1))


def _track_assign_ok(assigner):
    """what the batched assignment covers (`losses._assign_cost`): one-to-one mask Hungarian matching on class / mask / dice costs,
    no weighted depth cost"""
    from .assigner import _MaskAssignerBase
    return isinstance(assigner, _MaskAssignerBase) and assigner.topk == 1 and (assigner.depth_cost is None or assigner.depth_cost.weight == 0)


def _fast_assign_ok(assigner, sampler):
    """the descriptor path covers the shipped training configuration (polyphonic_former.py:170-192): an assigner the batched
    assignment covers, and the pseudo sampler"""
    from .assigner import MaskPseudoSampler
    return _track_assign_ok(assigner) and isinstance(sampler, MaskPseudoSampler)


def track_sample(assigner, mask_preds, cls_scores, gt, num_proposals, num_thing_classes, device_assign=False):
    """polyphonic_former_video.py:256-280 for the B images of one frame set: the track assigner (MaskHungarianAssigner: class, mask and
    dice costs over ALL pixels, no valid map, no depth cost) on the detached final-stage scaled_mask_preds[:, :Np] and
    cls_scores[:, :Np, :n_thing] against the UN-hardened thing masks at the assign resolution (`gt`: a soft `losses.StepGT`).  Pseudo
    sampling is the identity on the assignment, so what comes back is the assignment itself: `match` int32 [B, max(Gmax, 1)] on the
    device, the prediction row of every ground truth or -1 -- the form `track_head.gt_mask_rois` takes
    (`losses.assign_match`: solved on the host, or with device_assign by `ph_assign_solve`, whose status words are appended to
    gt.status_words)."""
    if not _track_assign_ok(assigner):
        raise NotImplementedError("track_sample: one-to-one Hungarian matching on class / mask / dice costs (the shipped track_train_cfg)")
    Np, nt = int(num_proposals), int(num_thing_classes)
    pred = _gpu32(mask_preds, "scaled_mask_preds")[:, :Np]
    cls = None if cls_scores is None else cls_scores.detach()[:, :Np, :nt].float()
    if pred.shape[0] != gt.B or pred.shape[1] != Np:
        raise ValueError("track_sample: mask_preds must hold num_proposals rows for every image of the ground truth")
    return Lo.assign_match(assigner, pred, cls, gt.all_pixels(), device_assign)


def video_track_branch(track_head, track_assigner, x, x_ref, key_last, ref_last, gt, ref_gt, gt_ids, ref_ids, pad_hw, num_proposals,
                       num_thing_classes, device_assign=False, strides=(4, 8, 16, 32), finest_scale=56):
    """The tracking part of PolyphonicVideo.forward_train (polyphonic_former_video.py:245-319) in one function: `gt_match_indices`, the
    two `track_sample`s, ONE `gt_mask_rois` call for all key and reference frames, `track_forward_train`.
    x / x_ref: the FPN levels [B, 256, H_l, W_l] of the key (gradients flow) and reference frames; key_last / ref_last: the final stage's
    (object_feats, cls_score, mask_preds, scaled_mask_preds) of `roi_forward_train` / `simple_test_mask_preds`; gt / ref_gt: soft
    `losses.StepGT` of the two frames' thing masks; gt_ids / ref_ids: per image the instance ids; pad_hw: the padded image size.
    With device_assign nothing here waits for the host.  -> {'loss_track', 'loss_track_aux'} attached to the graph."""
    from .track_head import gt_mask_rois
    B, Np = gt.B, int(num_proposals)
    if ref_gt.B != B or len(gt_ids) != B or len(ref_ids) != B:
        raise ValueError("video_track_branch: one reference frame, id list and ground truth per key image")
    gmi = [gt_match_indices(gt_ids[i], ref_ids[i]) for i in range(B)]
    mk = track_sample(track_assigner, key_last[3], key_last[1], gt, Np, num_thing_classes, device_assign)
    mr = track_sample(track_assigner, ref_last[3], ref_last[1], ref_gt, Np, num_thing_classes, device_assign)
    n = [min(g, Np) for g in gt.G + ref_gt.G]
    rois, pos_gt, _ = gt_mask_rois(list(gt.masks) + list(ref_gt.masks), [mk[i] for i in range(B)] + [mr[i] for i in range(B)], n, pad_hw,
                                   num_proposals=Np)
    feats = [[lv[i:i + 1] for lv in x] for i in range(B)]
    ref_feats = [[lv[i:i + 1] for lv in x_ref] for i in range(B)]
    return track_forward_train(track_head, feats, ref_feats, rois[:B], rois[B:], pos_gt[:B], pos_gt[B:], gmi, strides, finest_scale)


# ---- the two heads' training forwards (ONE implementation: the API methods and TrainStep both call these) --------------------
def parse_losses(losses):
    """mmdet BaseDetector._parse_losses (base.py:188-199): the objective is the sum of the entries with 'loss' in the key"""
    return sum(v.mean() for k, v in losses.items() if "loss" in k and torch.is_tensor(v))


def _attach(values, total):
    """values: {name: detached scalar}, total: the differentiable objective these values add up to (their 'loss' entries,
    already weighted).  Returns the dict the reference's forward_train returns, with every 'loss' entry carrying an equal
    share of `total`'s graph, so that what mmdet forms from it -- `sum(the 'loss' entries)`, base.py:188-199 -- has exactly
    the gradient of the objective, through ONE autograd node per head and stage.  (The loss kernels return
    d(sum of a head's losses) / d(prediction), not one gradient per entry: only the SUM of the entries is differentiable
    in a meaningful way, which is all the reference's runner ever differentiates.)"""
    keys = [k for k in values if "loss" in k]
    share = (total - total.detach()) / max(len(keys), 1)
    return {k: (v + share if "loss" in k else v) for k, v in values.items()}


def check_stage_topology(head):
    """the assumptions stage_forward hard-codes (the shipped configuration, configs/_base_/models/polyphonic_former.py:111-165);
    the constructors reject everything else, this guards modules altered after construction"""
    bad = []
    if len(head.cls_fcs) != 3 or len(head.mask_fcs) != 3 or len(head.depth_regs) != 2: bad.append("num_cls_fcs / num_mask_fcs != 1")
    if head.dropout != 0.0: bad.append("dropout")
    if head.conv_kernel_size != 1 or head.mask_transform_stride != 1 or head.feat_gather_stride != 1: bad.append("kernel size / strides")
    if head.hard_mask_thr != 0.5: bad.append("hard_mask_thr")
    if not head.with_ffn or len(head.ffn.layers) != 3 or len(head.ffn.layers[0]) != 3: bad.append("FFN layout")   # (Linear, act, Dropout), Linear, Dropout
    if bad:
        raise NotImplementedError("training forward: unsupported KernelUpdateHead topology: " + ", ".join(bad))


def check_rpn_topology(head):
    bad = []
    if len(head.loc_convs) != 1 or len(head.seg_convs) != 1 or len(head.depth_convs) != 1: bad.append("num_*_convs != 1")
    if head.conv_kernel_size != 1 or not head.use_binary or not head.proposal_feats_with_obj: bad.append("kernel size / use_binary")
    if head.feat_downsample_stride > 1 and head.feat_refine: bad.append("feat_refine")
    if head.feat_downsample_stride not in (1, 2): bad.append("feat_downsample_stride")
    if bad:
        raise NotImplementedError("training forward: unsupported KernelHead topology: " + ", ".join(bad))


def _valid_pixels(gt_masks_i, gt_sem_seg_i):
    """1.0 where any instance or stuff mask of the image is set (kernel_head.py:415, kernel_update.py:238:
    `torch.cat((gt_masks, gt_sem_seg)).sum(0).bool()`), without materialising the concatenation"""
    v = None
    for t in (gt_masks_i, gt_sem_seg_i):
        if t.shape[0]:
            a = t.ne(0).any(dim=0)
            v = a if v is None else (v | a)
    if v is None:
        return torch.zeros(gt_masks_i.shape[1:], dtype=torch.float32, device=gt_masks_i.device)
    return v.float()


def _step_gt(cache, hard, gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth):
    if cache is None:
        cache = {}
    if hard not in cache:
        cache[hard] = Lo.StepGT(gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth, hard)
    return cache[hard]


def rpn_forward_train(h, feats, img_metas, gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth, want_grads=False, gt_cache=None,
                      device_assign=False):
    """KernelHead.forward_train, kernel_head.py:349-454, on the three post-neck maps (gradients flow into `feats` when they
    require them).  Returns (losses, r): `losses` = the reference's dict with the 'loss' entries attached to the graph
    (`_attach`), `depth_dense` logged only (base.py:198 leaves it out of the objective); r = the differentiable training-
    mode decode (no stuff rows).  want_grads: losses['_grads'] = d(sum of the 'loss' entries) / d(scaled mask, seg and
    direct depth predictions).  device_assign: the assignment and the target tables on the device (`losses.assign_desc_device`), no
    host round trip; the host path where the kernels' limits do not hold."""
    check_rpn_topology(h)
    if h.assigner is None:
        raise ValueError("forward_train needs train_cfg (assigner / sampler)")
    r = rpn_forward(h, feats)
    up = (lambda t: upsample2x(t)) if h.feat_downsample_stride == 2 else (lambda t: t)
    smask, sseg, sdep0 = up(r["mask_preds"]), up(r["seg_preds"]), up(r["depth_pred"])         # :364-398
    N = h.num_proposals + h.num_stuff_classes
    if _fast_assign_ok(h.assigner, h.sampler):
        # round 5: batched assignment (one pixel pass + one D2H for all images), targets as pointer tables, ONE loss call
        gt = _step_gt(gt_cache, bool(h.hard_target), gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth)
        desc = Lo.assign_desc_device(h, gt, h.assigner, smask.detach(), None, h.num_proposals, h.train_cfg, roi=False) if device_assign else None
        if desc is None:
            assigns = Lo.assign_batch(h.assigner, smask.detach(), None, gt)
            desc = Lo.build_desc(h, gt, assigns, h.num_proposals, h.train_cfg, roi=False)
        loss_fn = lambda mp, sp, dp: Lo.fused_losses(h, desc, mp, None, dp, sp, with_grads=True)
    else:
        if h.hard_target:                 # local to the rpn side, as in the reference (kernel_head.py:400-403); StepGT hardens its own
            gt_masks = [m.bool().float() for m in gt_masks]
        sdep = sdep0.detach().expand(-1, N, -1, -1)
        srs = []
        for i in range(len(img_metas)):                                                       # :411-426
            valid = _valid_pixels(gt_masks[i], gt_sem_seg[i])
            ar = h.assigner.assign(smask[i].detach(), None, gt_masks[i], gt_labels[i], img_metas[i], depth_pred=sdep[i],
                                   gt_depth=gt_depth[i], gt_valid=valid)
            sr = h.sampler.sample(ar, smask[i].detach(), gt_masks[i], depth=sdep[i])
            sr.valid_mask = valid
            srs.append(sr)
        targets = h.get_targets(srs, gt_masks, h.train_cfg, True, gt_sem_seg=gt_sem_seg, gt_sem_cls=gt_sem_cls, gt_depth=gt_depth)
        loss_fn = lambda mp, sp, dp: Lo.rpn_losses(h, mp, sp, dp.expand(-1, N, -1, -1), *targets, with_grads=True)
    kept = {}

    def fn(mp, sp, dp):
        ls, g = loss_fn(mp, sp, dp)
        kept.update(mask_pred=g["mask_pred"], seg_preds=g["seg_preds"], depth_pred=g["depth_pred"])
        return ls, (g["mask_pred"], g["seg_preds"], g["depth_pred"])

    values = {}
    total = _Objective.apply(fn, values, smask, sseg, sdep0)
    losses = _attach(values, total)
    if gt_depth is not None:
        losses["depth_dense"] = Lo.dense_depth_loss(h, sdep0.detach(), gt_depth)              # :438-442, logged only
    if want_grads:
        losses["_grads"] = kept
    return losses, r


def rpn_outputs(h, r):
    """what KernelHead.forward_train hands to the roi head besides the losses (kernel_head.py:444-454): the stuff rows
    appended when cat_stuff_mask, all tensors still on the graph"""
    B = r["x"].shape[0]
    nt, L = h.num_thing_classes, h.num_classes
    mask_preds, k, q = r["mask_preds"], r["proposal"], r["depth_proposal"]
    if h.cat_stuff_mask:
        mask_preds = torch.cat([mask_preds, r["seg_preds"][:, nt:L]], dim=1)
        stuff = _lib.named_params(h)["conv_seg.weight"][nt:L].flatten(1)
        k = torch.cat([k, stuff[None].expand(B, -1, -1)], dim=1)
    N = k.shape[1]
    return k, mask_preds, q.expand(B, N, -1)


def roi_forward_train(ih, x, dfe, k, mask_preds, q, depth_pred, img_metas, gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth,
                      want_grads=False, gt_cache=None, device_assign=False):
    """KernelUpdateIterHead.forward_train, kernel_update.py:159-280.  x, dfe [B, C, H, W]; k / q [B, N, C] kernels and depth
    kernels; mask_preds [B, N, H, W]; depth_pred [B, 1, H, W].  Every stage: forward in training form, the Hungarian
    assignment on the previous stage's detached predictions and the stage's losses on the assigned targets as one autograd node.
    Where the targets come from is the one thing that differs between configurations: descriptors into the step's ground truth
    (`_DescTargets`, the shipped configuration) or per-image sampling and materialised targets (`_ListTargets`).  Returns (losses,
    last): losses = {s{stage}_{name}} weighted and attached (`_attach`), last = the final stage's (object_feats, cls_score,
    mask_preds, scaled_mask_preds)."""
    if ih.post_assign:
        raise NotImplementedError                       # as the reference (:222-223)
    if not ih.mask_assigner:
        raise ValueError("forward_train needs train_cfg (assigner / sampler per stage)")
    up = ih.mask_head[0].mask_upsample_stride
    if up not in (1, 2):
        raise NotImplementedError("libpolyhead: mask_upsample_stride must be 1 or 2")
    scale = (lambda t: upsample2x(t)) if up == 2 else (lambda t: t)
    prev_mask = scale(mask_preds.detach()).detach()                                           # :179-191
    if all(_fast_assign_ok(a, sm) for a, sm in zip(ih.mask_assigner, ih.mask_sampler)):
        gt = _step_gt(gt_cache, bool(ih.hard_target), gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth)
        targets = _DescTargets(ih, gt, device_assign)
    else:
        targets = _ListTargets(ih, scale, depth_pred, k.shape[1], img_metas, gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth)
    total, m, values, grads, prev_cls = 0.0, mask_preds, {}, [], None                         # :193-196
    cls = smask = None
    for s in range(ih.num_stages):
        head = ih.mask_head[s]
        check_stage_topology(head)
        cls, m, k, depth, q = stage_forward(head, x, dfe, k, m, q)
        smask, sdepth = scale(m), scale(depth)                                                 # training: every stage (:131)
        loss_fn = targets.stage(s, head, prev_mask, prev_cls, smask, sdepth)
        kept = {}

        def fn(cs, mp, dp, loss_fn=loss_fn, kept=kept):
            ls, g = loss_fn(cs, mp, dp)
            kept.update(g)
            return ls, (g["cls_score"], g["mask_pred"], g["depth_pred"])

        box = {}
        w = ih.stage_loss_weights[s]
        obj = _Objective.apply(fn, box, cls, smask, sdepth)
        total = total + (obj if w == 1 else w * obj)
        for key, v in box.items():
            values[f"s{s}_{key}"] = v if w == 1 else v * w
        grads.append(kept)
        prev_mask, prev_cls = smask.detach(), cls.detach()                                     # :273-276
    losses = _attach(values, total)
    if want_grads:
        losses["_grads"] = grads
    return losses, (k, cls, m, smask)


class _DescTargets:
    """where `roi_forward_train`'s stages take their targets from on the shipped configuration (`_fast_assign_ok`): per stage one
    batched assignment (`ph_match_sums` over all images + one D2H + the host Hungarian solves), one pointer-table upload and ONE loss
    call (`ph_train_losses`).  No sampler gathers, no materialised targets: every target row is a row of the step's ground truth
    (`losses.StepGT`).  The previous stage's depth predictions only feed the DepthCost, whose weight is 0 here, so they are not
    formed.  device_assign: assignment and tables by `ph_assign_desc` on the device instead (no D2H, no host solve, no upload); a
    stage the kernels do not cover takes the host path."""

    def __init__(self, ih, gt, device_assign):
        self.ih, self.gt, self.device_assign = ih, gt, device_assign
        self.assigns = self.ddesc = None

    def stage(self, s, head, prev_mask, prev_cls, smask, sdepth):
        """-> the stage's `fn(cls, mask, depth) -> (losses, grads dict)`; prev_*: the previous stage's detached predictions"""
        ih, gt = self.ih, self.gt
        Np, nt, cfg = ih.num_proposals, ih.num_thing_classes, ih.train_cfg[s]
        if s < ih.assign_stages:
            c = None if prev_cls is None else prev_cls[:, :Np, :nt]
            self.ddesc = Lo.assign_desc_device(head, gt, ih.mask_assigner[s], prev_mask[:, :Np], c, Np, cfg, roi=True) if self.device_assign else None
            if self.ddesc is None:
                self.assigns = Lo.assign_batch(ih.mask_assigner[s], prev_mask[:, :Np], c, gt)  # :231-251
        elif self.ddesc is not None:                                                           # the last assignment again, other weights
            self.ddesc = Lo.assign_desc_device(head, gt, None, prev_mask[:, :Np], None, Np, cfg, roi=True, prev=self.ddesc)
        desc = self.ddesc if self.ddesc is not None else Lo.build_desc(head, gt, self.assigns, Np, cfg, roi=True)
        return lambda cs, mp, dp: Lo.fused_losses(head, desc, mp, cs, dp, None, with_grads=True)


class _ListTargets:
    """the same for every other configuration (topk > 1, a weighted DepthCost, another sampler): per image `assign` and `sample`, the
    head's `get_targets`, `losses.stage_losses` on the materialised targets.  prev_depth: the scaled direct depth prediction expanded
    to the N rows ([B, N, 2H, 2W]), then every stage's own -- only this path's DepthCost reads it."""

    def __init__(self, ih, scale, depth_pred, N, img_metas, gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth):
        if ih.hard_target:
            gt_masks = [m.bool().float() for m in gt_masks]
        self.ih, self.img_metas, self.assign = ih, img_metas, []
        self.prev_depth = scale(depth_pred.detach().expand(-1, N, -1, -1).contiguous()).detach()
        self.gt = (gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth)
        # the pixels some ground-truth mask covers (:238): the same for every stage -- evaluated once per image instead of once per
        # image and stage (a 24 MB concatenation + reduction each at the assign stride of cfg2)
        self.valids = [_valid_pixels(gt_masks[i], gt_sem_seg[i]) for i in range(len(gt_masks))]

    def stage(self, s, head, prev_mask, prev_cls, smask, sdepth):
        ih = self.ih
        gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth = self.gt
        Np, nt = ih.num_proposals, ih.num_thing_classes
        srs = []
        if s < ih.assign_stages:
            self.assign = []
        for i, valid in enumerate(self.valids):
            if s < ih.assign_stages:
                c = None if prev_cls is None else prev_cls[i][:Np, :nt]
                self.assign.append(ih.mask_assigner[s].assign(prev_mask[i][:Np], c, gt_masks[i], gt_labels[i], self.img_metas[i],
                                                              depth_pred=self.prev_depth[i][:Np], gt_depth=gt_depth[i], gt_valid=valid))
            sr = ih.mask_sampler[s].sample(self.assign[i], smask[i].detach(), gt_masks[i], depth=sdepth[i].detach())
            sr.valid_mask = valid
            srs.append(sr)
        targets = head.get_targets(srs, gt_masks, gt_labels, ih.train_cfg[s], True, gt_sem_seg=gt_sem_seg, gt_sem_cls=gt_sem_cls, gt_depth=gt_depth)
        self.prev_depth = sdepth.detach()                                                      # :273-276
        return lambda cs, mp, dp: Lo.stage_losses(head, cs, mp, dp, *targets, with_grads=True)


# ---- the step ------------------------------------------------------------------------------------------------------------------
def _heads_forward_train(rpn, roi, feats, img_metas, gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth, device_assign, gt_cache=None):
    """the two heads on the three post-neck maps, what both steps run: -> (the 24 losses attached to the graph, the final stage's
    (object_feats, cls_score, mask_preds, scaled_mask_preds), the step's ground-truth cache).  gt_cache: the cache pre-filled
    (`_prepared_cache`), so that no `losses.StepGT` is derived from the lists."""
    gt_cache = {} if gt_cache is None else gt_cache         # the step's ground truth (losses.StepGT), shared by the two heads
    rpn_losses, r = rpn_forward_train(rpn, feats, img_metas, gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth,
                                      gt_cache=gt_cache, device_assign=device_assign)
    k, mask_preds, q = rpn_outputs(rpn, r)
    losses, last = roi_forward_train(roi, r["x"], r["dfe"], k, mask_preds, q, r["depth_pred"], img_metas, gt_masks, gt_labels,
                                     gt_sem_seg, gt_sem_cls, gt_depth, gt_cache=gt_cache, device_assign=device_assign)
    losses.update(rpn_losses)                               # polyphonic_former.py:126
    return losses, last, gt_cache


def _prepared_cache(prepared, hards):
    """the ground-truth cache of a step whose ground truth `gt.prepare_gt` left on the device: one `losses.StepGT` per `hard_target`
    value the step asks for, views of the prepared buffers"""
    return {bool(h): prepared.step_gt(bool(h)) for h in set(bool(h) for h in hards)}


def _prepared_lists(prepared):
    """(gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth) as `forward_backward` takes them, views of the prepared buffers"""
    return prepared.gt_masks, prepared.gt_labels, prepared.gt_sem_seg, prepared.gt_sem_cls, prepared.gt_depth


class _StepBase:
    """what the two training steps share: the checks of the two heads, the bucketed gradient all-reduce over `parameters()`, the
    leaves, the objective / backward tail, the device solves' status words.  A subclass sets the modules it trains (`_trained`, in
    parameter order) before it calls this constructor, and runs its forward through `_step`."""

    def __init__(self, rpn_head, roi_head, bucket_bytes, group, device_assign):
        self.rpn, self.roi = rpn_head, roi_head
        # the Hungarian assignments and target tables on the device (csrc/ph_assign.hip): the step's forward waits for the host nowhere
        # after its ground truth is built; off by default
        self.device_assign = bool(device_assign)
        self._status = []
        if rpn_head.assigner is None or not roi_head.mask_assigner:
            raise ValueError(f"{type(self).__name__} needs heads built with train_cfg (assigner / sampler)")
        check_rpn_topology(rpn_head)
        for h in roi_head.mask_head:
            check_stage_topology(h)
        # data parallel: one process per GPU, gradients averaged by bucketed all-reduces (RCCL over xGMI) that start while
        # backward is still running (dist.GradBuckets); on one rank nothing is sent
        from .dist import GradBuckets
        self.group = group
        self.buckets = GradBuckets(self.parameters(), bucket_bytes=bucket_bytes, group=group)

    def close(self):
        self.buckets.remove()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def parameters(self):
        """every parameter of the trained modules once (by identity), module by module; the rpn head's `localization_fpn.*` are the
        neck's: left out where the step does not train the neck, listed with the neck where it does"""
        out, seen = [], set()
        for m in self._trained:
            for n, p in _lib.named_params(m).items():
                if m is getattr(self, "backbone", None) and not p.requires_grad:        # its frozen stages: no gradient, no bucket
                    continue
                if id(p) not in seen and not (m is self.rpn and n.startswith("localization_fpn.")):
                    seen.add(id(p))
                    out.append(p)
        return out

    def optimizer(self, **kw):
        """an `optim.AdamWStep` over `parameters()`: gradient clipping + AdamW in one launch-only call behind `forward_backward`
        (kw: lr, betas, eps, weight_decay, max_norm, skip_nonfinite)"""
        from .optim import AdamWStep
        return AdamWStep(self.parameters(), **kw)

    def assign_status(self):
        """the status words of the last step's device solves, downloaded now (a synchronising copy, when the caller chooses to):
        int64 [solves, B], 0 = solved; _lib.PH_ASSIGN_ENONFINITE: the image's costs were not finite and it got the trivial matching.
        Empty without `device_assign` or where every solve took the host path.  The video step's two track solves add a row each."""
        if not self._status:
            return torch.zeros((0, 0), dtype=torch.int64)
        return torch.stack(self._status).cpu()

    @staticmethod
    def _leaves(maps, name, requires_grad=True):
        """the step's own fp32 contiguous copies or views of its input maps, on the GPU; leaves of the graph where they get a gradient"""
        return [_gpu32(f, name).requires_grad_(requires_grad) for f in maps]

    def _step(self, leaves, forward, backward):
        """forward() -> (losses attached to the graph, the `losses.StepGT`s the step used); the objective, backward with the bucketed
        all-reduce -> (losses, objective, gradients of `leaves`), all detached"""
        with torch.enable_grad(), Lo.reduce_group(self.group):
            losses, gts = forward()
            self._status = [w for g in gts for w in g.status_words]
            total = parse_losses(losses)
            if backward:
                self.buckets.start()
                total.backward()
                self.buckets.finish()
        return {k_: v.detach() for k_, v in losses.items()}, total.detach(), [f.grad for f in leaves]


class TrainStep(_StepBase):
    """rpn_head: KernelHead, roi_head: KernelUpdateIterHead, both built with train_cfg.  `forward_backward` evaluates one
    step on the three post-neck maps and leaves `.grad` on every parameter of the two heads (accumulating, like autograd; averaged over the ranks
    when torch.distributed runs with more than one) and returns (losses, objective, gradients of the three maps).  The
    same two functions back the reference-named API methods (`KernelHead.forward_train`,
    `KernelUpdateIterHead.forward_train`), whose loss dicts mmdet's `_parse_losses` + `backward()` consume unchanged; this
    class adds the bucketed gradient all-reduce.  Use as a context manager (or call `close()`) to take the gradient hooks
    off the parameters again."""

    def __init__(self, rpn_head, roi_head, bucket_bytes=32 << 20, group=None, device_assign=False):
        self._trained = (rpn_head, roi_head)
        super().__init__(rpn_head, roi_head, bucket_bytes, group, device_assign)

    def forward_backward(self, feats, img_metas, gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth, backward=True):
        return self._forward_backward(feats, img_metas, (gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth), None, backward)

    def forward_backward_prepared(self, feats, img_metas, gt, backward=True):
        """`forward_backward` on ground truth `gt.prepare_gt` left on the device (gt: a `gt.PreparedGT`): the step's `losses.StepGT`s
        are views of the prepared buffers, nothing is derived from the mask lists and nothing is read back"""
        cache = _prepared_cache(gt, (self.rpn.hard_target, self.roi.hard_target))
        return self._forward_backward(feats, img_metas, _prepared_lists(gt), cache, backward)

    def _forward_backward(self, feats, img_metas, lists, gt_cache, backward):
        feats = self._leaves(feats, "the post-neck maps")

        def forward():
            losses, _, cache = _heads_forward_train(self.rpn, self.roi, feats, img_metas, *lists, self.device_assign, gt_cache=gt_cache)
            return losses, cache.values()

        return self._step(feats, forward, backward)


class VideoTrainStep(_StepBase):
    """PolyphonicVideo.forward_train after extract_feat (polyphonic_former_video.py:185-325) as one step: the neck in training form on
    the key frame's FPN levels and in eval form on the reference frame's, the two heads on the key frame exactly as `TrainStep` runs
    them, the reference frame through `simple_test_rpn` + `simple_test_mask_preds` in eval mode under no_grad, the track branch
    (`video_track_branch`), the objective, ONE backward with bucketed gradient all-reduce over the parameters of neck, both heads and
    the track head.  track_train_cfg: dict(assigner=...) as the model config has it (MaskHungarianAssigner, FocalLossCost 2, DiceCost 4,
    MaskCost 1) or a built assigner.  `rpn_head.localization_fpn` is None (the neck is this step's) or the same neck.
    fpn (a `fpn.FPN`, optional): the step starts one module earlier -- x / x_ref are the BACKBONE STAGES of the two frames, the key
    frame's go through `fpn_forward_train`, the reference frame's through the FPN's eval plan under no_grad, the FPN's 16 parameters
    are the first of `parameters()`, and the returned gradients are those of the key frame's stages (what the backbone's backward
    takes).  Without it nothing changes.
    backbone (a `resnet.ResNet`, optional, needs `fpn`): the step starts at the images -- x / x_ref are the image tensors [B, 3, H, W] of
    the two frames, the key frames go through `resnet_forward_train` (its scope: frozen_stages >= 1, norm_eval=True, grade bf16), the
    reference frames through the backbone's inference plan under no_grad, the backbone's trained parameters are the first of
    `parameters()`, and no input gradient is returned.  Without it nothing changes."""

    def __init__(self, neck, rpn_head, roi_head, track_head, track_train_cfg, bucket_bytes=32 << 20, group=None, device_assign=False,
                 strides=(4, 8, 16, 32), finest_scale=56, fpn=None, backbone=None):
        from .assigner import build_assigner
        if backbone is not None and fpn is None:
            raise ValueError("VideoTrainStep: backbone needs fpn (the backbone's stages feed the FPN)")
        self.neck, self.track_head, self.fpn, self.backbone = neck, track_head, fpn, backbone
        self._trained = tuple(m for m in (backbone, fpn) if m is not None) + (neck, rpn_head, roi_head, track_head)
        self.strides, self.finest_scale = tuple(strides), finest_scale
        if rpn_head.localization_fpn is not None and rpn_head.localization_fpn is not neck:
            raise ValueError("VideoTrainStep: rpn_head.localization_fpn must be None or the step's neck")
        a = track_train_cfg.get("assigner") if isinstance(track_train_cfg, dict) else getattr(track_train_cfg, "assigner", track_train_cfg)
        self.track_assigner = build_assigner(dict(a)) if isinstance(a, dict) else a
        if not _track_assign_ok(self.track_assigner):
            raise NotImplementedError("VideoTrainStep: track_train_cfg.assigner must be a one-to-one mask Hungarian assigner without depth cost")
        super().__init__(rpn_head, roi_head, bucket_bytes, group, device_assign)

    def _reference_frame(self, x_ref, ref_metas, levels_out=None):
        """:186-191, 207-243 for the reference frame: (FPN,) neck, rpn head and roi head in eval mode under no_grad, at the grade the
        module API runs; every module's `training` flag is put back.  With an FPN x_ref are the frame's backbone stages and
        `levels_out` (a list) receives its FPN levels: the eval plan's buffers, valid until that plan runs again; with a backbone
        x_ref is the frames' image tensor"""
        tops = [t for t in (self.backbone, self.fpn, self.neck, self.rpn, self.roi) if t is not None]
        mods = [m for top in tops for m in top.modules()]
        flags = [m.training for m in mods]
        try:
            for top in tops:
                top.eval()
            with torch.no_grad():
                if self.backbone is not None:
                    x_ref = list(self.backbone(x_ref))                              # the inference plan: no gradient is asked for
                if self.fpn is not None:
                    x_ref = list(self.fpn(x_ref))
                    if levels_out is not None:
                        levels_out[:] = x_ref
                src = x_ref if self.rpn.localization_fpn is not None else self.neck(x_ref)
                (pf, xf, mp, cs, _, df, dp, dpr, _) = self.rpn.simple_test_rpn(src, ref_metas)
                return self.roi.simple_test_mask_preds(xf, pf, mp, cs, ref_metas, depth_preds=dpr, depth_feats=df, depth_proposal=dp, imgs_whwh=None)
        finally:
            for m, f in zip(mods, flags):
                m.training = f

    def forward_backward(self, x, x_ref, img_metas, gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth, gt_instance_ids, ref_gt_masks,
                         ref_gt_labels, ref_gt_instance_ids, pad_hw, backward=True, ref_img_metas=None):
        """x / x_ref: the FPN levels of the key and the reference frames; the ground truth as the reference has it at :185 (things and
        stuff split, at the assign resolution).  -> (losses: the 24 image losses + loss_track + loss_track_aux, objective, gradients of
        the key frame's FPN levels: neck path + RoIAlign path).  The reference frame's levels get no gradient.  With the step's `fpn`:
        x / x_ref are the backbone stages and the gradients returned are those of the key frame's stages; with its `backbone` they
        are the image tensors and the list of gradients is empty."""
        return self._forward_backward(x, x_ref, img_metas, (gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth, gt_instance_ids),
                                      (ref_gt_masks, ref_gt_labels, ref_gt_instance_ids), pad_hw, backward, ref_img_metas)

    def forward_backward_prepared(self, x, x_ref, img_metas, gt, ref_gt, pad_hw, backward=True, ref_img_metas=None):
        """`forward_backward` on ground truth `gt.prepare_gt` left on the device: gt / ref_gt are the `gt.PreparedGT` of the key and
        the reference frames (both prepared with gt_instance_ids).  Every `losses.StepGT` of the step is a view of the prepared
        buffers; the reference frames' holds their things alone, as `forward_backward` builds it."""
        if gt.gt_instance_ids is None or ref_gt.gt_instance_ids is None:
            raise ValueError("VideoTrainStep.forward_backward_prepared: prepare both frames' ground truth with gt_instance_ids")
        cache = _prepared_cache(gt, (self.rpn.hard_target, self.roi.hard_target, False))
        return self._forward_backward(x, x_ref, img_metas, _prepared_lists(gt) + (gt.gt_instance_ids,),
                                      (ref_gt.gt_masks, ref_gt.gt_labels, ref_gt.gt_instance_ids), pad_hw, backward, ref_img_metas,
                                      gt_cache=cache, ref_gt=ref_gt.step_gt(False, with_stuff=False))

    def _forward_backward(self, x, x_ref, img_metas, key, ref, pad_hw, backward, ref_img_metas, gt_cache=None, ref_gt=None):
        """key: (gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth, gt_instance_ids), ref: (ref_gt_masks, ref_gt_labels,
        ref_gt_instance_ids); gt_cache / ref_gt: the key frames' cache and the reference frames' `losses.StepGT` where they are
        prepared, else derived from the lists where the step first needs them"""
        lists, gt_instance_ids = key[:5], key[5]
        ref_gt_masks, ref_gt_labels, ref_gt_instance_ids = ref
        what = "the FPN levels" if self.fpn is None else "the backbone stages"
        if self.backbone is not None:
            img, x, x_ref = _gpu32(x, "the key frames' images"), [], _gpu32(x_ref, "the reference frames' images")
        else:
            x = self._leaves(x, what)
            x_ref = self._leaves(x_ref, what, requires_grad=False)

        def forward():
            lv, lv_ref = x, x_ref
            if self.fpn is not None:
                lv, lv_ref = fpn_forward_train(self.fpn, x if self.backbone is None else resnet_forward_train(self.backbone, img)), []
            feats = neck_forward_train(self.neck, lv)                                                  # :185
            losses, last, cache = _heads_forward_train(self.rpn, self.roi, feats, img_metas, *lists, self.device_assign, gt_cache=gt_cache)
            ref_last = self._reference_frame(x_ref, ref_img_metas if ref_img_metas is not None else img_metas,
                                             levels_out=None if self.fpn is None else lv_ref)
            gt = _step_gt(cache, False, *lists)                                                        # the soft masks (:259)
            rgt = ref_gt if ref_gt is not None else Lo.StepGT(ref_gt_masks, ref_gt_labels, None, None, None, False)
            losses.update(video_track_branch(self.track_head, self.track_assigner, lv, lv_ref, last, ref_last, gt, rgt, gt_instance_ids,
                                             ref_gt_instance_ids, pad_hw, self.roi.num_proposals, self.roi.num_thing_classes,
                                             self.device_assign, self.strides, self.finest_scale))
            return losses, list(cache.values()) + [rgt]

        return self._step(x, forward, backward)
