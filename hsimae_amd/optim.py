"""Fused AdamW for `hsimae_amd.HSIMAE`.

The reference builds `torch.optim.AdamW` over two name-filtered parameter groups (Model_Pretraining.py:80-86) and
steps it once per iteration (:102).  With fwd+bwd at ~30 ms, 535 per-tensor updates are pure launch overhead; here
the whole flat parameter buffer is updated by ONE kernel (`hsimae_adamw_step`) with torch's AdamW arithmetic, and
the model is told to refresh its packed bf16 weight images.  `param_groups` is kept (one dict per reference group,
sharing `lr`) so LR schedulers that write `group['lr']` keep working.

`max_grad_norm` / `skip_nonfinite` (both off by default, and then nothing below changes) put the size of the update under control
without a host wait: `hsimae_grad_norm` forms the global 2-norm of every gradient that takes part in the step, the clip
coefficient and the decision to skip a non-finite step in device memory, and the step reads them there.

`layer_decay` / `freeze` (both off by default) and `param_groups` whose values differ are honoured by `hsimae_adamw_step_groups`: the
id byte the kernel already reads per element indexes a table of {lr, weight_decay} pairs that travels in the launch, so the step
stays one launch however many groups there are, and composes with the clipping above.

`FusedLAMB` (below) is the large-batch variant: the same buffers, ids, table and control block, with Adam's update scaled per parameter
tensor by |w| / |update| (`hsimae_lamb_step`, csrc/lamb.hip).

`ema_decay` (off by default) keeps an exponential moving average of the weights next to them: one `hsimae_ema_update` over the flat
buffer behind the step's own launches, which reads the same control block, so a skipped step leaves the average alone and the
step still waits for nothing.  `ema_state_dict()` reads the average, `swap_ema()` evaluates with it."""
from __future__ import annotations

import contextlib
import re
from collections import OrderedDict

import numpy as np
import torch

from . import _lib

_BLOCK = re.compile(r"^(blocks_1|blocks_2|blocks)\.(\d+)\.")


def layer_ids(model, depth=None, s_depth=None):
    """{parameter name: layer id} for layer-wise learning-rate decay, the MAE / BEiT convention on this model's names:
    `patch_embed.*` and `pos_embed` 0; `blocks_1.i.*` and `blocks_2.i.*` 1 + i (the two axis stacks run side by side and share a
    depth); `blocks.j.*` 1 + s_depth + j; everything else (`norm`, `cls_head`, the decoder, `mask_token`) depth + 1.
    `model`: an HSIMAE / DualViT / HSIViT, or an iterable of names with `depth` and `s_depth` given."""
    if hasattr(model, "named_parameters"):
        names = [n for n, _ in model.named_parameters()]
        depth = model.depth if depth is None else depth
        s_depth = model.s_depth if s_depth is None else s_depth
    else:
        names = list(model)
    if depth is None or s_depth is None:
        raise ValueError("layer_ids: a list of names needs depth and s_depth")
    depth, s_depth = int(depth), int(s_depth)
    out = {}
    for n in names:
        blk = _BLOCK.match(n)
        if n == "pos_embed" or n.startswith("patch_embed."):
            out[n] = 0
        elif blk:
            out[n] = 1 + int(blk.group(2)) + (s_depth if blk.group(1) == "blocks" else 0)
        else:
            out[n] = depth + 1
        if out[n] > depth + 1:
            raise ValueError(f"layer_ids: {n} lies behind depth {depth} (s_depth {s_depth})")
    return out


def weights_state_dict(model, flat, outside=()):
    """`model.state_dict()` with every parameter of the flat buffer read from `flat` (a tensor laid out like `model._flat`) and
    every parameter of `outside` [(parameter, tensor)] from its tensor: the same keys, dtypes and shapes, fresh tensors."""
    held = {id(p): flat[o:o + s] for p, o, s in zip(model._params_cache, model._offs, model._sizes)}
    held.update({id(p): t for p, t in outside})
    by_name = dict(model.named_parameters())
    out = OrderedDict()
    for k, v in model.state_dict().items():
        p = by_name.get(k)
        t = held.get(id(p)) if p is not None else None
        out[k] = v.detach().clone() if t is None else t.to(v.device).reshape(v.shape).to(v.dtype).clone()
    return out


class FusedAdamW:
    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, no_decay=("bias", "norm"), strict=True,
                 max_grad_norm=None, skip_nonfinite=False, layer_decay=None, freeze=(), ema_decay=None, ema_warmup=True):
        """max_grad_norm: clip the global gradient 2-norm to it, with torch.nn.utils.clip_grad_norm_'s coefficient
        min(1, max_norm / (norm + 1e-6)); `float("inf")` only measures.  skip_nonfinite: a step whose norm is Inf or NaN
        changes nothing (no parameter, no moment, no weight decay, no advance of the bias-correction count).

        The clip is applied INSIDE the step: `.grad` is not modified, the update is computed from g * coef.  A parameter
        that is masked out of the step (no `.grad`) is left out of the norm, as torch leaves out a `.grad` that is None.
        `step()` waits for nothing and copies nothing to the host; `grad_norm`, `clip_coef` and `skipped_steps` are 0-d device
        tensors (views of the control block), and reading them from the host is the caller's wait.

        Data parallel: the reducer's all-reduce has completed on the stream before `step()` reads the gradients; the norm kernel
        is launched on the same stream, sees the reduced gradients, and so every rank takes the same decision.

        layer_decay: a float in (0, 1]; a parameter of layer id i (`layer_ids`) is stepped with lr * layer_decay ** (depth + 1 - i):
        the head and the final norm at the full rate, the embedding at the smallest.  `param_groups` then holds one dict per distinct
        (lr_scale, decays or not) pair, top layer first, each with its own `lr`, `weight_decay` and `lr_scale`; schedulers keep
        writing `lr`, and `lr_scale` is applied at the step (as MAE's adjust_learning_rate does).
        freeze: name prefixes; a matching parameter is left out for good, exactly as one with requires_grad=False is: no update, no
        weight decay, its moments stay zero, and it is not part of the gradient norm.  `freeze` only selects what the optimizer
        steps: it does NOT shorten the backward pass, the frozen layers' gradients are still computed.
        Whatever is written into `param_groups` (by hand or by a scheduler with per-group values) is honoured at the next step.

        ema_decay: a float in [0, 1); `self.ema` then holds an fp32 moving average of the flat parameter buffer (and one tensor per
        live parameter outside it), started from the weights as they are before this optimizer's first step (what timm's ModelEma
        copies) and moved by every APPLIED step: ema += (1 - d) * (p - ema), d = min(ema_decay, (1 + t) / (10 + t)) with
        ema_warmup (TensorFlow's num_updates rule; t counts applied steps), d = ema_decay without.  A frozen parameter stays bit-equal
        to its average.  The average never feeds back into the step.  Like timm's it is fp32: at ema_decay = 0.9999 an increment
        below half an ulp of the average is lost."""
        self.model = model
        if ema_decay is not None:
            if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float, np.floating, np.integer)) or not 0.0 <= float(ema_decay) < 1.0:
                raise ValueError(f"ema_decay must be a float in [0, 1) (or None), got {ema_decay!r}")
            ema_decay = float(ema_decay)
        self.ema_decay, self.ema_warmup = ema_decay, bool(ema_warmup)
        self.ema = None
        self._swapped = False
        self.layer_decay = None if layer_decay is None else float(layer_decay)
        if self.layer_decay is not None and not 0.0 < self.layer_decay <= 1.0:
            raise ValueError(f"layer_decay must lie in (0, 1] (or be None), got {layer_decay}")
        self.freeze = (freeze,) if isinstance(freeze, str) else tuple(freeze)
        self._grouped = self.layer_decay is not None or bool(self.freeze)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        if self.max_grad_norm is not None and not self.max_grad_norm > 0:
            raise ValueError(f"max_grad_norm must be greater than 0 (or None), got {max_grad_norm}")
        self.skip_nonfinite = bool(skip_nonfinite)
        self._clip = self.max_grad_norm is not None or self.skip_nonfinite
        self._ctl = self._partials = None
        self._skipped_loaded = None
        self.strict = bool(strict)                   # see _sync_grads
        self._mask_cache = {}
        self.defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        # One entry per distinct (lr_scale, decays or not) pair, the two at scale 1 first: they keep the ids 0 / 1 ("decay / no decay"
        # as hsimae_adamw_step knows them).  Id 2 stays "frozen or absent", so the third entry takes id 3.
        if self.layer_decay is not None:
            lids, top = layer_ids(model), int(model.depth) + 1
            scale_of = lambda n: self.layer_decay ** (top - lids[n])            # noqa: E731
        else:
            scale_of = lambda n: 1.0                                            # noqa: E731
        # Parameters that do not live in the model's flat buffer (DualViT's cls_head) are stepped by a stock
        # torch.optim.AdamW with their group's hyper-parameters, read from param_groups at each step.  (Not in the clipped mode.)
        self._in_flat = in_flat = {id(p) for p in model._plist()} if hasattr(model, "_plist") else None
        members = {(1.0, False): [], (1.0, True): []}
        flat_keys, outside = [], []
        for n, p in model.named_parameters():
            key = (scale_of(n), any(k in n for k in no_decay))
            frozen = not p.requires_grad or any(n.startswith(f) for f in self.freeze)
            if in_flat is not None and id(p) not in in_flat:
                if not frozen:
                    members.setdefault(key, []).append(p)
                    outside.append((p, key))
                continue
            if frozen or n == "mask_token":                     # mask_token never receives a gradient
                flat_keys.append(None)
            else:
                members.setdefault(key, []).append(p)
                flat_keys.append(key)
        keys = sorted(members, key=lambda k: (-k[0], k[1]))
        self._gids = [k if k < 2 else k + 1 for k in range(len(keys))]          # table index of each param_group
        self._ngroups = self._gids[-1] + 1
        if self._ngroups > _lib.ADAMW_MAX_GROUPS:
            raise ValueError(f"FusedAdamW: {len(keys)} parameter groups need {self._ngroups} table entries, "
                             f"hsimae_adamw_step_groups takes {_lib.ADAMW_MAX_GROUPS}")
        gid_of = dict(zip(keys, self._gids))
        self._groups_of = [2 if k is None else gid_of[k] for k in flat_keys]
        self.param_groups = []
        for scale, is_nd in keys:
            g = dict(params=members[(scale, is_nd)], lr=lr, weight_decay=0.0 if is_nd else weight_decay, betas=tuple(betas), eps=eps)
            if self.layer_decay is not None:
                g["lr_scale"] = scale
            self.param_groups.append(g)
        self._extra = None
        # In the clipped mode the optimizer steps the outside parameters itself (its own moments, the grouped step with their
        # group's id for every element): a host-side optimizer could not honour a skip decided on the device.
        outside.sort(key=lambda pk: gid_of[pk[1]])                # decayed before not, as the stock optimizer's state lists them
        self._outside = [(p, gid_of[k]) for p, k in outside] if self._clip else []
        self._ema_params = [p for p, _ in outside] if self.ema_decay is not None else []      # in both modes
        self._ema_out = [None] * len(self._ema_params)
        self._out_m = [None] * len(self._outside)
        self._out_v = [None] * len(self._outside)
        if len(self._outside) > _lib.CLIP_MAX_SEGS - 1:
            raise NotImplementedError(f"FusedAdamW(max_grad_norm / skip_nonfinite): {len(self._outside)} parameters outside the flat "
                                      f"buffer, one hsimae_grad_norm call takes {_lib.CLIP_MAX_SEGS - 1}")
        if outside and not self._clip:
            self._extra_of = sorted({keys.index(k) for _, k in outside})        # which param_group each extra group follows
            groups = [dict(params=[p for p, k in outside if keys.index(k) == i], weight_decay=self.param_groups[i]["weight_decay"])
                      for i in self._extra_of]
            self._extra = torch.optim.AdamW(groups, lr=lr, betas=tuple(betas), eps=eps)
        self.step_count = 0
        self._flat_id = None
        self.exp_avg = self.exp_avg_sq = self._group = None

    def _bind(self):
        m = self.model
        if m._flat is None:
            raise RuntimeError("FusedAdamW: run a forward pass on the GPU first (the flat parameter buffer does not exist yet)")
        if self._flat_id != m._flat.data_ptr():
            flat = m._flat
            if self.exp_avg is None or self.exp_avg.numel() != flat.numel():
                self.exp_avg = torch.zeros_like(flat)
                self.exp_avg_sq = torch.zeros_like(flat)
            else:
                self.exp_avg, self.exp_avg_sq = self.exp_avg.to(flat.device), self.exp_avg_sq.to(flat.device)
            grp = torch.empty(flat.numel(), dtype=torch.uint8)
            for off, size, gid in zip(m._offs, m._sizes, self._groups_of):
                grp[off:off + size] = gid
            self._group_host = grp
            self._group = grp.to(flat.device)
            self._mask_cache = {}
            if self.ema_decay is not None:              # first bind: the weights before the first step; later: the average moves along
                self.ema = flat.clone() if self.ema is None or self.ema.numel() != flat.numel() else self.ema.to(flat.device)
                for k, p in enumerate(self._ema_params):
                    self._need_fp32(p)
                    e = self._ema_out[k]
                    self._ema_out[k] = p.detach().reshape(-1).clone() if e is None or e.numel() != p.numel() else e.to(p.device)
            self._flat_id = flat.data_ptr()

    def _need_fp32(self, p):
        if not p.is_contiguous() or p.dtype != torch.float32:
            raise RuntimeError(f"{type(self).__name__}: a parameter outside the flat buffer must be a contiguous fp32 tensor")

    def zero_grad(self, set_to_none: bool = True):
        zg = getattr(self.model, "zero_grad", None)
        if zg is not None:
            zg(set_to_none=set_to_none)              # HSIMAE.zero_grad also records that no gradient is at home any more
            return
        for p in self.model.parameters():
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def _sync_grads(self):
        """`.grad` is the contract, the flat gradient buffer only its usual home.  A parameter whose `.grad` is None (cleared
        by zero_grad and not touched by this step's backward — e.g. the encoder after a decoder-only backward) is SKIPPED like
        torch.optim.AdamW skips it: it is masked out of this step (group id 2: no update, no weight decay, moments kept), so a
        stale range of the flat buffer is never applied.  A `.grad` that is some other tensor (assigned or accumulated by the
        caller) is copied into its flat view first.  Returns the group-id tensor to use for this step.

        Cost: the model keeps track of which of its two parameter ranges (encoder, decoder) had their `.grad` attached by a
        backward since the last `zero_grad` (`HSIMAE._grads_home`).  When both were — every step of the reference's loop —
        the default (`strict=True`) compares every `.grad` with its flat view (532 attribute reads, ~50 us of host time that
        overlaps the device's backward) and the step is ONE launch: a `.grad` set to None or replaced by another tensor after
        the backward (clipping by assignment, masking, a hook) is seen, exactly as `torch.optim.AdamW` would see it.
        `strict=False` is the opt-in fast path for loops that never touch `.grad` between backward and step: four identity
        comparisons (first / last parameter of each range); a middle parameter's replaced `.grad` is then NOT noticed.  Only when
        something is missing or foreign is the per-parameter walk done, and its mask is built on the host and uploaded once
        (cached per pattern) — no per-parameter device writes."""
        m = self.model
        params, views = m._params_cache, m._grad_views
        home = getattr(m, "_grads_home", None)
        if home is not None and home[0] and home[1]:
            if self.strict:
                if all(params[i].grad is views[i] for i in m._trainable):
                    return self._group
            else:
                probe = (m._enc_idx[0], m._enc_idx[-1], m._dec_idx[0], m._dec_idx[-1])
                if all(params[i].grad is views[i] for i in probe):
                    return self._group
        missing, foreign = [], []
        for i in m._trainable:
            g = params[i].grad
            if g is None:
                missing.append(i)
            elif g is not views[i] and (g.data_ptr() != views[i].data_ptr() or g.shape != views[i].shape):
                foreign.append(i)
        for i in foreign:
            views[i].copy_(params[i].grad.to(views[i].dtype).reshape(views[i].shape))
        if not missing:
            return self._group
        key = tuple(missing)
        grp = self._mask_cache.get(key)
        if grp is None:
            host = self._group_host.clone()
            hv = host.numpy()
            for i in missing:
                hv[m._offs[i]: m._offs[i] + m._sizes[i]] = 2
            grp = host.to(self._group.device)             # one upload per pattern
            if len(self._mask_cache) >= 4:
                self._mask_cache.pop(next(iter(self._mask_cache)))
            self._mask_cache[key] = grp
        return grp

    def _defaults_agree(self):
        """The two default groups still describe ONE learning rate and weight decay (what hsimae_adamw_step takes)."""
        if self._grouped or len(self.param_groups) != 2:
            return False
        g0, g1 = self.param_groups
        return (g1["lr"] == g0["lr"] and g1["weight_decay"] == 0 and g0.get("lr_scale", 1.0) == 1.0 and g1.get("lr_scale", 1.0) == 1.0)

    @staticmethod
    def _effective_lr(g):
        return float(g["lr"]) * float(g.get("lr_scale", 1.0))      # fp64; rounded once to fp32 where it enters the table

    def lr_range(self):
        """(smallest, largest) effective learning rate over the groups that hold parameters; host values, no device read."""
        lrs = [self._effective_lr(g) for g in self.param_groups if g["params"]] or [self._effective_lr(self.param_groups[0])]
        return min(lrs), max(lrs)

    def _table(self):
        """param_groups as hsimae_adamw_step_groups takes them: entry id = {lr * lr_scale, weight_decay}; id 2 is the hole."""
        table = (_lib.AdamWGroup * self._ngroups)()
        for g, gid in zip(self.param_groups, self._gids):
            table[gid] = _lib.AdamWGroup(self._effective_lr(g), float(g["weight_decay"]))
        return table

    @torch.no_grad()
    def step(self):
        self._refuse_inside_swap("step()")
        self._bind()
        m, g0 = self.model, self.param_groups[0]
        self.step_count += 1
        stream = torch.cuda.current_stream(m._flat.device).cuda_stream
        hp = (float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"]), stream)
        group = self._sync_grads()
        live = self._grad_norm(group, hp) if self._clip else []     # the control block decides the size of this step
        table = self._table() if self._clip or not self._defaults_agree() else None
        self._step_flat(group, table, hp)
        self._step_outside(live, table, hp)
        m._packed_version = -1                    # packed bf16 images are stale now
        self._ema_update(stream)

    def _ctl_ptr(self):
        return None if self._ctl is None else self._ctl.data_ptr()       # there is one in the clipped mode only

    def _adamw_groups(self, p, g, m, v, ids, gid, n, table, hp):
        """One hsimae_adamw_step_groups over n elements: `ids` holds an id per element, or is None and `gid` is the id of all."""
        b1, b2, eps, stream = hp
        _lib.check(_lib.load().hsimae_adamw_step_groups(
            p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None if ids is None else ids.data_ptr(), gid, n, table,
            self._ngroups, b1, b2, eps, self.step_count, self._ctl_ptr(), stream), "hsimae_adamw_step_groups")

    def _step_flat(self, group, table, hp):
        m = self.model
        flat, grad = m._flat, m._flat_grad
        if table is not None:
            self._adamw_groups(flat, grad, self.exp_avg, self.exp_avg_sq, group, 0, flat.numel(), table, hp)
            return
        g0, (b1, b2, eps, stream) = self.param_groups[0], hp       # one lr, one weight decay, no control block
        _lib.check(_lib.load().hsimae_adamw_step(
            flat.data_ptr(), grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), group.data_ptr(), flat.numel(),
            float(g0["lr"]), b1, b2, eps, float(g0["weight_decay"]), self.step_count, stream), "hsimae_adamw_step")

    def _step_outside(self, live, table, hp):
        for k, p, g, gid in live:                  # the clipped mode: the grouped step with the parameter's id for every element
            self._adamw_groups(p, g, self._out_m[k], self._out_v[k], None, gid, p.numel(), table, hp)
        if self._extra is not None:                # the unclipped mode: the stock optimizer
            for ge, gi in zip(self._extra.param_groups, self._extra_of):
                ge["lr"] = self._effective_lr(self.param_groups[gi])
                ge["weight_decay"] = self.param_groups[gi]["weight_decay"]
            self._extra.step()

    # ------------------------------------------------------------------ moving average of the weights (off by default)
    def _ema_pairs(self):
        return [(self.ema, self.model._flat)] + list(zip(self._ema_out, self._ema_params))

    def _ema_update(self, stream):
        """One hsimae_ema_update over the flat buffer and one per live parameter outside it, behind the step's launches.  With a
        control block the kernel takes the skip decision and the count of applied steps from it; without one no step is skipped."""
        if self.ema_decay is None:
            return
        for e, p in self._ema_pairs():
            _lib.check(_lib.load().hsimae_ema_update(e.data_ptr(), p.data_ptr(), e.numel(), self.ema_decay, int(self.ema_warmup),
                                                     self.step_count, self._ctl_ptr(), stream), "hsimae_ema_update")

    def _need_ema(self, what):
        if self.ema_decay is None:
            raise RuntimeError(f"{type(self).__name__} was built without ema_decay: there is no average for {what}")

    def _refuse_inside_swap(self, what):
        if self._swapped:
            raise RuntimeError(f"{type(self).__name__}: {what} inside swap_ema(): the model holds the averaged weights")

    def _exchange(self):
        m = self.model
        stream = torch.cuda.current_stream(m._flat.device).cuda_stream
        for e, p in self._ema_pairs():
            _lib.check(_lib.load().hsimae_ema_swap(p.data_ptr(), e.data_ptr(), e.numel(), stream), "hsimae_ema_swap")
        m._packed_version = -1                    # the packed bf16 images are stale now ...
        if hasattr(m, "_head_pack"):
            m._head_pack = None                   # ... and so is DualViT's packed head: a kernel write does not advance Parameter._version

    @contextlib.contextmanager
    def swap_ema(self):
        """`with opt.swap_ema():` the model holds the averaged weights (and `self.ema` the raw ones); on exit they are exchanged
        back, bit for bit.  Two launches of hsimae_ema_swap per buffer in all, no copy.  It cannot be nested, and step() refuses to
        run inside it."""
        self._need_ema("swap_ema()")
        self._refuse_inside_swap("swap_ema()")
        self._bind()
        self._exchange()
        self._swapped = True
        try:
            yield self
        finally:
            self._exchange()
            self._swapped = False

    def ema_state_dict(self):
        """The averaged weights under `model.state_dict()`'s keys, dtypes and shapes (fresh tensors); entries that are not
        parameters, and parameters the optimizer does not step, are the model's own.  Loads wherever the model's state_dict does."""
        self._need_ema("ema_state_dict()")
        self._bind()
        if self._swapped:                          # the model holds the average right now
            return OrderedDict((k, v.detach().clone()) for k, v in self.model.state_dict().items())
        return weights_state_dict(self.model, self.ema, list(zip(self._ema_params, self._ema_out)))

    # ------------------------------------------------------------------ gradient norm / clipping / skip (off by default)
    def _ensure_ctl(self, device=None):
        if self._ctl is None:
            if not self._clip:
                raise AttributeError("FusedAdamW was built without max_grad_norm / skip_nonfinite: there is no gradient norm")
            device = device if device is not None else next(self.model.parameters()).device
            if torch.device(device).type != "cuda":
                raise RuntimeError("FusedAdamW: the model is not on the GPU (hsimae_amd has no CPU fallback)")
            f = _lib.ClipCtl
            self._ctl = torch.zeros(_lib.C.sizeof(f), dtype=torch.uint8, device=device)     # skipped = 0, norm_max = 0
            self._partials = torch.empty(_lib.CLIP_GRID, dtype=torch.float64, device=device)

            def field(fd, dtype):
                return self._ctl[fd.offset: fd.offset + fd.size].view(dtype)[0]
            self._views = dict(norm=field(f.norm, torch.float32), coef=field(f.coef, torch.float32),
                               skipped=field(f.skipped, torch.int64), norm_max=field(f.norm_max, torch.float32))
            if self._skipped_loaded is not None:
                self._views["skipped"].copy_(torch.as_tensor(self._skipped_loaded, dtype=torch.int64))
                self._skipped_loaded = None
        return self._views

    @property
    def grad_norm(self):
        """Global 2-norm of the last step's gradients, before clipping (0-d fp32 device tensor)."""
        return self._ensure_ctl()["norm"]

    @property
    def clip_coef(self):
        """What the last step multiplied the gradients by (0-d fp32 device tensor)."""
        return self._ensure_ctl()["coef"]

    @property
    def skipped_steps(self):
        """Number of steps skipped for a non-finite norm so far (0-d int64 device tensor)."""
        return self._ensure_ctl()["skipped"]

    @property
    def grad_norm_max(self):
        """Largest finite `grad_norm` since `reset_grad_norm_max()` (0-d fp32 device tensor; the loops log it per epoch)."""
        return self._ensure_ctl()["norm_max"]

    def reset_grad_norm_max(self):
        self._ensure_ctl()["norm_max"].zero_()

    def _grad_norm(self, group, hp):
        """hsimae_grad_norm over the flat gradient buffer and the `.grad` of the live parameters outside it; fills the control block.
        Returns those parameters as [(index into _outside, parameter, contiguous fp32 gradient, group id)], their moments in place."""
        m, (b1, b2, _, stream) = self.model, hp
        flat = m._flat
        self._ensure_ctl(flat.device)
        segs = (_lib.GradSeg * _lib.CLIP_MAX_SEGS)()
        segs[0] = _lib.GradSeg(m._flat_grad.data_ptr(), group.data_ptr(), flat.numel())
        live = []
        for k, (p, gid) in enumerate(self._outside):
            g = p.grad
            if g is None:                              # as torch: not in the norm, not stepped
                continue
            if g.dtype != torch.float32 or not g.is_contiguous():
                g = g.float().contiguous()
            self._need_fp32(p)
            if self._out_m[k] is None or self._out_m[k].device != p.device:
                z = torch.zeros(p.numel(), dtype=torch.float32, device=p.device)
                self._out_m[k] = z if self._out_m[k] is None else self._out_m[k].to(p.device)
                self._out_v[k] = z.clone() if self._out_v[k] is None else self._out_v[k].to(p.device)
            live.append((k, p, g, gid))
            segs[len(live)] = _lib.GradSeg(g.data_ptr(), None, g.numel())
        max_norm = float("inf") if self.max_grad_norm is None else self.max_grad_norm
        _lib.check(_lib.load().hsimae_grad_norm(segs, 1 + len(live), max_norm, int(self.skip_nonfinite), self.step_count, b1, b2,
                                                self._partials.data_ptr(), self._ctl.data_ptr(), stream), "hsimae_grad_norm")
        return live

    def state_dict(self):
        sd = {"step": self.step_count, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq,
              "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups],
              "extra": self._extra.state_dict() if self._extra is not None else None}
        if self._clip:
            sd["skipped"] = (self._views["skipped"].clone() if self._ctl is not None
                             else torch.as_tensor(self._skipped_loaded or 0, dtype=torch.int64))
            sd["outside_exp_avg"], sd["outside_exp_avg_sq"] = list(self._out_m), list(self._out_v)
        if self.ema_decay is not None:
            self._refuse_inside_swap("state_dict()")
            sd["ema"], sd["outside_ema"], sd["ema_decay"] = self.ema, list(self._ema_out), self.ema_decay
        return sd

    _KIND = "adamw"                                  # what state_dict()["optimizer"] names; a checkpoint without the key is AdamW's

    def load_state_dict(self, sd):
        kind = sd.get("optimizer", "adamw")
        if kind != self._KIND:
            raise ValueError(f"checkpoint was written by the {kind} optimizer, this one is {self._KIND}: its moments mean something else")
        if len(sd["param_groups"]) != len(self.param_groups):
            raise ValueError(f"checkpoint carries {len(sd['param_groups'])} parameter groups, this optimizer has {len(self.param_groups)} "
                             "(built with another layer_decay / freeze, or for another depth)")
        self.step_count = int(sd["step"])
        self.exp_avg, self.exp_avg_sq = sd["exp_avg"], sd["exp_avg_sq"]
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update(s)
        if self._extra is not None and sd.get("extra") is not None:
            self._extra.load_state_dict(sd["extra"])
        if self._clip:
            self._load_clip_state(sd)
        if self.ema_decay is not None:            # a checkpoint without an average: it starts from the loaded weights at the next bind
            self._refuse_inside_swap("load_state_dict()")
            self.ema = sd.get("ema")
            oe = sd.get("outside_ema")
            if oe is not None and len(oe) != len(self._ema_params):
                raise ValueError(f"checkpoint carries averages for {len(oe)} outside parameters, the model has {len(self._ema_params)}")
            self._ema_out = [None] * len(self._ema_params) if oe is None or self.ema is None else [None if t is None else t.reshape(-1) for t in oe]
        self._flat_id = None

    def _load_clip_state(self, sd):
        """`skipped` and the outside parameters' moments.  A checkpoint written without the feature has neither: skipped = 0, and
        the moments are taken from the stock optimizer's state it carries for those parameters (same order: decayed, then not)."""
        sk = sd.get("skipped", 0)
        if self._ctl is not None:
            self._views["skipped"].copy_(torch.as_tensor(sk, dtype=torch.int64))
        else:
            self._skipped_loaded = sk.clone() if torch.is_tensor(sk) else int(sk)
        n = len(self._outside)
        if sd.get("outside_exp_avg") is not None:
            om, ov = list(sd["outside_exp_avg"]), list(sd["outside_exp_avg_sq"])
            if len(om) != n or len(ov) != n:
                raise ValueError(f"checkpoint carries moments for {len(om)} outside parameters, the model has {n}")
            self._out_m = [None if t is None else t.reshape(-1) for t in om]
            self._out_v = [None if t is None else t.reshape(-1) for t in ov]
        elif sd.get("extra") is not None:
            state = sd["extra"].get("state", {})
            for k in range(n):
                st = state.get(k)
                if st is not None and "exp_avg" in st:
                    self._out_m[k] = st["exp_avg"].detach().float().reshape(-1).clone()
                    self._out_v[k] = st["exp_avg_sq"].detach().float().reshape(-1).clone()


# ---------------------------------------------------------------------------------------------------------------------- LAMB
def lamb_tensor_table(offs, sizes):
    """The tensor table of hsimae_lamb_step for tensors at `offs` with `sizes` floats: (rows, nchunks).  rows is a numpy record
    array laid out as hsimae_lamb_tensor {off, n, chunk0, reserved}; chunk0 is the prefix sum of ceil(size / HSIMAE_LAMB_CHUNK)."""
    offs, sizes = np.asarray(offs, dtype=np.int64), np.asarray(sizes, dtype=np.int64)
    per = (sizes + _lib.LAMB_CHUNK - 1) // _lib.LAMB_CHUNK
    ends = np.cumsum(per)
    nchunks = int(ends[-1]) if len(ends) else 0
    if nchunks >= 2 ** 31:
        raise ValueError(f"{nchunks} chunks do not fit hsimae_lamb_tensor.chunk0")
    rows = np.zeros(len(offs), dtype=np.dtype([("off", "<i8"), ("n", "<i8"), ("chunk0", "<i4"), ("reserved", "<i4")]))
    assert rows.dtype.itemsize == _lib.C.sizeof(_lib.LambTensor)
    rows["off"], rows["n"], rows["chunk0"] = offs, sizes, ends - per
    return rows, nchunks


class FusedLAMB(FusedAdamW):
    """LAMB (You et al., "Large Batch Optimization for Deep Learning", 2020; apex FusedLAMB, timm Lamb) on FusedAdamW's buffers:
    Adam's update u = m_hat / (sqrt(v_hat) + eps) + weight_decay * p, applied as p -= lr * r * u with one trust ratio
    r = |p| / |u| per parameter tensor (1 where either norm is 0).  With every r = 1 it is AdamW's step.

    max_grad_norm: as FusedAdamW's (the clip happens inside the step); None only measures the norm.  The gradient norm is always
    formed: the step reads the clip coefficient, the skip decision and the bias corrections from the device-side control block.
    trust_clip: an upper bound on r (timm's trust_clip=True is trust_clip=1.0); None: no bound.
    always_adapt: False leaves tensors whose weight decay is 0 (biases, norms) at r = 1, as timm does.
    layer_decay / freeze / param_groups / skip_nonfinite / strict / ema_decay / ema_warmup: FusedAdamW's.

    step() is hsimae_grad_norm (two launches) and hsimae_lamb_step (three) over the flat buffer, then one hsimae_lamb_step per
    live parameter outside it (DualViT's head); no ATen op, no host wait.  `trust_ratios` holds the last applied step's ratios."""
    _KIND = "lamb"

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, no_decay=("bias", "norm"), strict=True,
                 max_grad_norm=1.0, skip_nonfinite=False, layer_decay=None, freeze=(), trust_clip=None, always_adapt=False,
                 ema_decay=None, ema_warmup=True):
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError(f"max_grad_norm must be greater than 0 (or None), got {max_grad_norm}")
        # the parent in its clipped mode (it owns the outside parameters' moments and the control block); inf only measures
        super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, no_decay=no_decay, strict=strict,
                         max_grad_norm=float("inf") if max_grad_norm is None else max_grad_norm, skip_nonfinite=skip_nonfinite,
                         layer_decay=layer_decay, freeze=freeze, ema_decay=ema_decay, ema_warmup=ema_warmup)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.trust_clip = None if trust_clip is None else float(trust_clip)
        if self.trust_clip is not None and not self.trust_clip > 0:
            raise ValueError(f"trust_clip must be greater than 0 (or None), got {trust_clip}")
        self.always_adapt = bool(always_adapt)
        self.trust_ratio_names = [n for n, p in model.named_parameters() if self._in_flat is None or id(p) in self._in_flat]
        self._lamb_id = None
        self._tensors = self._lamb_partials = self._ratios = self._bad = None
        self._out_tab = [None] * len(self._outside)                # per outside parameter: (table, nchunks, partials)
        self._out_ratios = None

    def _bind(self):
        super()._bind()
        flat = self.model._flat
        if self._lamb_id != flat.data_ptr():
            rows, self._nchunks = lamb_tensor_table(self.model._offs, self.model._sizes)
            self._tensors = torch.from_numpy(rows.view(np.uint8).copy()).to(flat.device)      # one upload
            self._ntensors = len(rows)
            self._lamb_partials = torch.zeros(2 * self._nchunks, dtype=torch.float64, device=flat.device)
            if self._ratios is None or self._ratios.numel() != self._ntensors:
                self._ratios = torch.ones(self._ntensors, dtype=torch.float32, device=flat.device)
            else:
                self._ratios = self._ratios.to(flat.device)
            if self._bad is None:
                self._bad = torch.zeros((), dtype=torch.int32, device=flat.device)
            else:
                self._bad = self._bad.to(flat.device)
            if self._out_ratios is None:
                self._out_ratios = torch.ones(len(self._outside), dtype=torch.float32, device=flat.device)
            self._lamb_id = flat.data_ptr()

    @property
    def trust_ratios(self):
        """One fp32 trust ratio per tensor of the flat buffer (`trust_ratio_names` order), as the last applied step used them; 1 for
        a tensor that is frozen or not adapted (device tensor; reading it from the host is the caller's wait)."""
        self._bind()
        return self._ratios

    @property
    def trust_ratios_outside(self):
        """The ratios of the parameters outside the flat buffer (DualViT's cls_head.weight, cls_head.bias), in that order."""
        self._bind()
        return self._out_ratios

    @property
    def table_error(self):
        """0-d int32 device tensor: not 0 once a step has met an inconsistent tensor table (hsimae_lamb_step's `bad`)."""
        self._bind()
        return self._bad

    def adapted(self):
        """Host list of bool per flat tensor: does the step form a trust ratio for it (live, and decayed or always_adapt)."""
        wd = {gid: float(g["weight_decay"]) for g, gid in zip(self.param_groups, self._gids)}
        return [gid != 2 and (self.always_adapt or wd[gid] != 0.0) for gid in self._groups_of]

    def trust_ratio_range(self):
        """(smallest, largest) trust ratio among the adapted tensors of the flat buffer, a 2-element fp64 device tensor (not part of
        step(): the loops call it once per epoch, in their one device read)."""
        r = self.trust_ratios
        sel = torch.tensor(self.adapted(), dtype=torch.bool, device=r.device)
        r = r[sel].double()
        return torch.stack([r.min(), r.max()]) if r.numel() else torch.ones(2, dtype=torch.float64, device=self._ratios.device)

    def _grad_norm(self, group, hp):
        live = super()._grad_norm(group, hp)
        for k, p, g, gid in live:                                  # a one-tensor table per live parameter outside the flat buffer
            if self._out_tab[k] is None or self._out_tab[k][0].device != p.device:
                rows, nch = lamb_tensor_table([0], [p.numel()])
                self._out_tab[k] = (torch.from_numpy(rows.view(np.uint8).copy()).to(p.device), nch,
                                    torch.zeros(2 * nch, dtype=torch.float64, device=p.device))
        return live

    def _lamb(self, p, g, m, v, ids, gid, n, tensors, ntensors, nchunks, partials, ratios_ptr, table, hp):
        """One hsimae_lamb_step over n elements in `ntensors` tensors: `ids` holds an id per element, or is None and `gid` is the id
        of all."""
        b1, b2, eps, stream = hp
        _lib.check(_lib.load().hsimae_lamb_step(
            p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None if ids is None else ids.data_ptr(), gid, n, tensors.data_ptr(),
            ntensors, nchunks, table, self._ngroups, b1, b2, eps, (self.trust_clip or 0.0), int(self.always_adapt), partials.data_ptr(),
            ratios_ptr, self._bad.data_ptr(), self._ctl_ptr(), stream), "hsimae_lamb_step")

    def _step_flat(self, group, table, hp):
        m = self.model
        self._lamb(m._flat, m._flat_grad, self.exp_avg, self.exp_avg_sq, group, 0, m._flat.numel(), self._tensors, self._ntensors,
                   self._nchunks, self._lamb_partials, self._ratios.data_ptr(), table, hp)

    def _step_outside(self, live, table, hp):
        for k, p, g, gid in live:
            tab, nch, part = self._out_tab[k]
            self._lamb(p, g, self._out_m[k], self._out_v[k], None, gid, p.numel(), tab, 1, nch, part,
                       self._out_ratios.data_ptr() + 4 * k, table, hp)

    def state_dict(self):
        sd = super().state_dict()
        sd["optimizer"] = "lamb"                  # the trust ratios are not state: every step forms them anew
        return sd
