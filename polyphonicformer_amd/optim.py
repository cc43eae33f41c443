"""The optimizer step of the training path: gradient clipping by the global L2 norm + AdamW over every parameter in ONE launch-only
call (csrc/ph_optim.hip; include/polyhead.h `ph_optim_step`).

What mmcv's OptimizerHook + `torch.optim.AdamW` do after `loss.backward()` for the schedule every shipped config trains with
(`AdamW(lr=2e-4, weight_decay=0.05)` behind `grad_clip=dict(max_norm=1, norm_type=2)`):

    clip_grad_norm_(params, max_norm, 2)  ->  AdamW.step()                     [-> zero_grad()]

as at most three launches that leave every `.grad` as backward produced it (the clip coefficient is applied on the fly), skip a step
whose gradient norm is not finite without a host read (a key / reference pair without a positive gives NaN gradients),
and bump `Parameter._version`, which is what the packed inference weights follow (`_lib.param_versions`).  The LR policy, the runner
and its hooks stay outside: `param_groups[i]['lr']` may be written between steps as mmcv's LR hook does, or `step(lr_factor=...)`
takes the schedule's factor, from the host or from a device scalar.

ONE step counter.  torch keeps a step per tensor and starts it at the tensor's first gradient; here the count is global (one bias
correction per call, on the device).  The two agree unless a parameter first receives a gradient at a later step than the others:
torch then corrects that tensor's moments as at step 1, this module as at the global count.  `state_dict()` writes the global count
into every tensor's state; `load_state_dict()` refuses a state whose per-tensor steps differ."""
import ctypes as C

import torch

from . import _lib

CHUNK = _lib.PH_OPTIM_CHUNK


def plan_items(numels, aligned):
    """the work items of a table, a pure function of the tensors' sizes and alignments (csrc/ph_optim.hip computes the same):
    numels[i] elements in chunks of CHUNK, numbered tensor by tensor; aligned[i]: p, g, m, v of tensor i are all 16-byte aligned.
    -> (item count, first_item column, per tensor "vec" | "scalar" | None for a tensor without elements).  A vector tensor moves
    its last n % 4 elements as scalars."""
    first, kinds, items = [], [], 0
    for n, al in zip(numels, aligned):
        if n < 0:
            raise ValueError("negative numel")
        first.append(items)
        items += (n + CHUNK - 1) // CHUNK
        kinds.append(None if n == 0 else "vec" if al else "scalar")
    return items, first, kinds


def all_aligned(*ptrs):
    """the vector rule of one tensor: p, g, m, v all 16-byte aligned (an item starts a multiple of 16 KB into each)"""
    return all(q % 16 == 0 for q in ptrs)


def item_tensor(first, item):
    """the tensor of work item `item`: the LAST entry of the first_item column not above it (the kernels' search)"""
    lo, hi = 0, len(first)
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if first[mid] <= item:
            lo = mid
        else:
            hi = mid
    return lo


def _pad4(n):
    return (n + 3) // 4 * 4


class AdamWStep:
    """AdamWStep(params_or_groups, lr, betas, eps, weight_decay, max_norm=None, skip_nonfinite=True)

    params_or_groups: an iterable of parameters, or of dicts as `torch.optim` takes them (`params`, optionally `lr`, `weight_decay`).
    Parameters are fp32 and contiguous; `step()` and `zero_grad()` need them on the GPU (`train._param32`'s rule: the kernels read raw
    pointers), the state exchange works wherever they live.  max_norm: clip_grad_norm_'s (None: no clipping).  skip_nonfinite: a
    call whose gradient norm is NaN or inf changes nothing (p, m, v and the step count keep their bits) and counts as skipped."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None, skip_nonfinite=True,
                 amsgrad=False, maximize=False):
        if amsgrad or maximize:
            raise NotImplementedError("AdamWStep: amsgrad / maximize are not implemented")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"AdamWStep: betas must lie in [0, 1): {betas}")
        if not eps > 0.0:
            raise ValueError(f"AdamWStep: eps must be positive: {eps}")
        self.defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.max_norm = None if max_norm is None else float(max_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.max_blocks = 0                                  # test aid: workgroups per launch at most (the results do not depend on it)
        params = list(params)
        if not params:
            raise ValueError("AdamWStep: no parameters")
        groups = params if isinstance(params[0], dict) else [dict(params=params)]
        self.param_groups, self.params, seen = [], [], set()
        for g in groups:
            g = dict(g)
            if g.get("amsgrad") or g.get("maximize"):
                raise NotImplementedError("AdamWStep: amsgrad / maximize are not implemented")
            ps = g["params"]
            g["params"] = [ps] if isinstance(ps, torch.Tensor) else list(ps)
            g.setdefault("lr", lr)
            g.setdefault("weight_decay", weight_decay)
            for p in g["params"]:
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise _lib.PolyheadError(f"AdamWStep: fp32 contiguous parameters only ({p.dtype}, contiguous={p.is_contiguous()})")
                if id(p) in seen:
                    raise ValueError("AdamWStep: a parameter appears in more than one group")
                seen.add(id(p))
                self.params.append(p)
            self.param_groups.append(g)
        dev = self.params[0].device
        if any(p.device != dev for p in self.params):
            raise ValueError("AdamWStep: all parameters must live on one device")
        self.device = dev
        # m and v: two zeroed arenas, every tensor's slice starts 16 bytes aligned
        numels = [p.numel() for p in self.params]
        self._offsets, total = [], 0
        for n in numels:
            self._offsets.append(total)
            total += _pad4(n)
        self._m = torch.zeros(max(total, 4), dtype=torch.float32, device=dev)
        self._v = torch.zeros(max(total, 4), dtype=torch.float32, device=dev)
        self.exp_avg = [self._m[o:o + n].view(p.shape) for o, n, p in zip(self._offsets, numels, self.params)]
        self.exp_avg_sq = [self._v[o:o + n].view(p.shape) for o, n, p in zip(self._offsets, numels, self.params)]
        # the state record (ph_optim_state) and the device views of its two floats, for logging without a read-back
        self._state = torch.zeros(C.sizeof(_lib.OptimState) // 8, dtype=torch.int64, device=dev)
        f = self._state.view(torch.float32)
        self.grad_norm = f[_lib.OptimState.grad_norm.offset // 4]
        self.clip_coef = f[_lib.OptimState.clip_coef.offset // 4]
        # the table: the host copy the library checks, the device copy the kernels read, and what the device copy was built from
        nt = len(self.params)
        self._table = (_lib.OptimTensor * nt)()
        self._table_dev = None
        self._key = None
        self._workspace = None
        # Two pinned staging images, used in turn, each with the event of its last upload: an image is rewritten only after the
        # copy that last read it has completed.  That copy is two uploads back, so the wait is a formality -- `Event.query()` says so
        # without blocking, and `Event.synchronize()` is reached only where it does not.
        self._images, self._events, self._turn = [None, None], [None, None], 0

    # ---- the table -------------------------------------------------------------------------------------------------------------
    def _table_key(self):
        ptrs = []
        for p in self.params:
            g = p.grad
            ptrs.append(p.data_ptr())
            ptrs.append(0 if g is None else g.data_ptr())
        return ptrs, [(g["lr"], g["weight_decay"]) for g in self.param_groups]

    def _sync_table(self):
        """re-uploads the table where a parameter, a gradient or a group value moved since the device copy was made; no
        synchronisation (see the staging images above)"""
        key = self._table_key()
        if key == self._key:
            return
        if self.device.type != "cuda":
            raise _lib.PolyheadError("AdamWStep: the parameters must live on the GPU: libpolyhead has no CPU path")
        if torch.cuda.is_current_stream_capturing():
            raise _lib.PolyheadError("AdamWStep: the table changed during a graph capture; run one eager step() or zero_grad() first "
                                     "and keep parameters, gradients and group values in place")
        ptrs, _ = key
        items, i = 0, 0
        for g in self.param_groups:
            for p in g["params"]:
                e, grad = self._table[i], p.grad
                if grad is not None and (grad.dtype != torch.float32 or not grad.is_contiguous() or grad.device != p.device or
                                         grad.numel() != p.numel()):
                    raise _lib.PolyheadError(f"AdamWStep: fp32 contiguous gradients of the parameter's size only (parameter {i})")
                n = p.numel()
                e.p, e.g = ptrs[2 * i] or None, ptrs[2 * i + 1] or None
                e.m, e.v = self.exp_avg[i].data_ptr() or None, self.exp_avg_sq[i].data_ptr() or None
                e.n, e.lr, e.weight_decay, e.first_item = n, float(g["lr"]), float(g["weight_decay"]), items
                items += (n + CHUNK - 1) // CHUNK
                i += 1
        nbytes = C.sizeof(self._table)
        if self._table_dev is None:
            self._table_dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            need = _lib.load().ph_optim_workspace_bytes(self._table, len(self.params))
            if need == 0:
                _lib.check(_lib.PH_EINVAL, "ph_optim_workspace_bytes")
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._images = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(2)]
        t = self._turn
        if self._events[t] is not None and not self._events[t].query():
            self._events[t].synchronize()
        C.memmove(self._images[t].data_ptr(), C.addressof(self._table), nbytes)
        self._table_dev.copy_(self._images[t], non_blocking=True)
        ev = self._events[t] or torch.cuda.Event()
        ev.record()
        self._events[t], self._turn, self._key = ev, 1 - t, key

    def _bump_versions(self):
        """what an in-place torch update would do: `_lib.param_versions` (the cache key of the packed inference weights) sees it"""
        torch._C._increment_version([p for p in self.params if p.grad is not None])

    # ---- the calls -------------------------------------------------------------------------------------------------------------
    def step(self, lr_factor=1.0, zero_grad=False):
        """one optimizer step, launches only.  lr_factor: a float, or a 1-element fp32 device tensor the kernel reads (a captured graph
        follows a schedule through it).  zero_grad: zeros are stored over every gradient the step has read, in place.  A parameter whose
        `.grad` is None is untouched.  Under a graph capture the version bump happens once, at capture: call `mark_updated()` after
        replays where packed weights have to follow."""
        self._sync_table()
        flags = (_lib.PH_OPTIM_SKIP_NONFINITE if self.skip_nonfinite else 0) | (_lib.PH_OPTIM_ZERO_GRADS if zero_grad else 0)
        cfg = _lib.OptimCfg(self.betas[0], self.betas[1], self.eps, self.max_norm if self.max_norm is not None else 0.0, flags,
                            self.max_blocks)
        if isinstance(lr_factor, torch.Tensor):
            if lr_factor.dtype != torch.float32 or lr_factor.numel() != 1 or lr_factor.device != self.device:
                raise _lib.PolyheadError("AdamWStep.step: a device lr_factor is one fp32 element on the parameters' device")
            host, dev = 1.0, _lib.ptr(lr_factor)
        else:
            host, dev = float(lr_factor), None
        _lib.check(_lib.load().ph_optim_step(C.byref(cfg), self._table, _lib.ptr(self._table_dev), len(self.params), host, dev,
                                             _lib.ptr(self._state), _lib.ptr(self._workspace), self._workspace.numel(), _lib.stream_ptr()),
                   "ph_optim_step")
        self._bump_versions()

    mark_updated = _bump_versions

    def zero_grad(self):
        """zeros over every gradient, one launch, in place: the gradients keep their addresses, so the table and a captured graph stay
        valid (torch's `zero_grad(set_to_none=False)`)"""
        self._sync_table()
        _lib.check(_lib.load().ph_optim_zero_grads(self._table, _lib.ptr(self._table_dev), len(self.params), self.max_blocks, _lib.stream_ptr()),
                   "ph_optim_zero_grads")
        torch._C._increment_version([p.grad for p in self.params if p.grad is not None])

    def _record(self):
        return _lib.OptimState.from_buffer_copy(self._state.cpu().numpy().tobytes())

    def info(self):
        """the state record, downloaded now -- the ONE synchronising call: steps applied, calls skipped, and of the last call its
        status (_lib.PH_OPTIM_OK / PH_OPTIM_ENONFINITE), gradient norm before clipping (-1 where no norm was asked for) and coefficient"""
        r = self._record()
        return dict(step=r.step, skipped=r.skipped, status=r.status, grad_norm=r.grad_norm, clip_coef=r.clip_coef)

    # ---- the state, in torch.optim.AdamW's layout ---------------------------------------------------------------------------------
    def state_dict(self):
        """`torch.optim.AdamW.state_dict()`'s layout: state[i] = {step, exp_avg, exp_avg_sq} for parameter i in group order, and
        param_groups with `params` as indices.  Every tensor gets the ONE global step; before the first step the state is empty, as
        torch's.  Synchronises (it reads the step count)."""
        step = self._record().step
        state = {}
        if step > 0:
            for i in range(len(self.params)):
                state[i] = dict(step=torch.tensor(float(step)), exp_avg=self.exp_avg[i].clone(), exp_avg_sq=self.exp_avg_sq[i].clone())
        groups, k = [], 0
        for g in self.param_groups:
            d = dict(lr=g["lr"], betas=self.betas, eps=self.eps, weight_decay=g["weight_decay"], amsgrad=False, maximize=False, foreach=None,
                     capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
            d.update({k_: v for k_, v in g.items() if k_ not in d and k_ != "params"})
            d["params"] = list(range(k, k + len(g["params"])))
            k += len(g["params"])
            groups.append(d)
        return dict(state=state, param_groups=groups)

    def load_state_dict(self, sd):
        """takes what `state_dict()` or a `torch.optim.AdamW` over the same parameters exported (mmcv stores the latter in a
        checkpoint): moments, the step count, and each group's lr / weight_decay.  The per-tensor steps must be equal (ValueError); a
        tensor without state starts from zero moments."""
        groups, state = sd["param_groups"], sd["state"]
        if len(groups) != len(self.param_groups) or any(len(a["params"]) != len(b["params"]) for a, b in zip(groups, self.param_groups)):
            raise ValueError("AdamWStep.load_state_dict: the groups do not match this optimizer's")
        for g in groups:
            if g.get("amsgrad") or g.get("maximize"):
                raise NotImplementedError("AdamWStep: amsgrad / maximize are not implemented")
            if tuple(g.get("betas", self.betas)) != self.betas or g.get("eps", self.eps) != self.eps:
                raise ValueError("AdamWStep.load_state_dict: betas / eps differ from this optimizer's")
        ids = [i for g in groups for i in g["params"]]
        steps = {float(state[i]["step"]) for i in ids if i in state}
        if len(steps) > 1:
            raise ValueError(f"AdamWStep.load_state_dict: the tensors' step counts differ ({sorted(steps)}); this optimizer keeps ONE")
        step = steps.pop() if steps else 0.0
        if step != int(step) or step < 0:
            raise ValueError(f"AdamWStep.load_state_dict: step {step} is not a count")
        for k, i in enumerate(ids):
            s = state.get(i)
            for dst, name in ((self.exp_avg[k], "exp_avg"), (self.exp_avg_sq[k], "exp_avg_sq")):
                if s is None:
                    dst.zero_()
                else:
                    if s[name].shape != dst.shape:
                        raise ValueError(f"AdamWStep.load_state_dict: {name} of parameter {k} has shape {tuple(s[name].shape)}")
                    dst.copy_(s[name])
        for g, mine in zip(groups, self.param_groups):
            mine["lr"], mine["weight_decay"] = g["lr"], g["weight_decay"]
        r = _lib.OptimState(step=int(step))
        r.grad_norm, r.clip_coef = -1.0, 1.0
        self._state.copy_(torch.frombuffer(bytearray(bytes(r)), dtype=torch.int64))
