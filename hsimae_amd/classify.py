"""The supervised half of fine-tuning on the device (csrc/cls.hip): `ClassLoss` and `ScoreMeter`.

  ClassLoss(ignore_index=0)(logits, targets) -> loss   torch.nn.CrossEntropyLoss(reduction="mean", ignore_index=...) as one
      launch pair (hsimae_cls_loss): the loss, its gradient and the argmax of every row come out of the same pass over the
      logits; the backward is the saved gradient times the incoming scalar, read from device memory (hsimae_cls_grad_scale).
  ScoreMeter(num_class, device)   the confusion counts of (label, prediction) accumulated on the device (hsimae_confusion /
      hsimae_confusion_map) and OA / AA / kappa / per-class recall from them (hsimae_scores): what `finetune_train.scores`
      computes on the host from the two label vectors.

Nothing here waits for the host except ScoreMeter.compute() and ClassLoss.check(), one small copy each.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_CLASSES = 1024


def _need_cuda(t, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a torch tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise RuntimeError(f"hsimae_amd runs on MI355X only (no CPU fallback): {what} is on {t.device}")


def _labels(t, what, device):
    """int64, contiguous, on `device`: a tensor is used as it is when it already is all that (numpy arrays are uploaded)."""
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(t)))
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError(f"{what} must hold integer labels, got {t.dtype}")
    return t.detach().to(device=device, dtype=torch.int64).contiguous()


class _ClassLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, owner, need_grad):
        dev = logits.device
        N, Cc = int(logits.shape[0]), int(logits.shape[1])
        z = logits.detach()
        if z.stride(1) != 1 or z.stride(0) < Cc:          # the head's padded view out[:, :num_class] passes as it is
            z = z.contiguous()
        with torch.cuda.device(dev):
            lib = _lib.load()
            stream = torch.cuda.current_stream(dev).cuda_stream
            loss = torch.empty((), dtype=torch.float32, device=dev)
            pred = torch.empty(N, dtype=torch.int64, device=dev)
            n_valid = torch.empty((), dtype=torch.int64, device=dev)
            dl = torch.empty(N, Cc, dtype=torch.float32, device=dev) if need_grad else None
            p = _lib.ClsParams(logits=z.data_ptr(), ld=z.stride(0) if N > 1 else max(z.stride(0), Cc), targets=targets.data_ptr(), N=N,
                               C=Cc, ignore_index=owner.ignore_index, first=owner.first, loss=loss.data_ptr(),
                               n_valid=n_valid.data_ptr(), dlogits=_lib.ptr(dl), ldd=Cc, pred=pred.data_ptr(),
                               bad=owner._bad_flag(dev).data_ptr(), workspace=owner._workspace(dev, N).data_ptr())
            _lib.check(lib.hsimae_cls_loss(C.byref(p), stream), "hsimae_cls_loss")
        owner.last_pred, owner.last_n_valid = pred, n_valid
        ctx.dl = dl
        return loss

    @staticmethod
    def backward(ctx, g):
        dl = ctx.dl
        if dl is None:
            raise RuntimeError("ClassLoss: the forward ran without autograd, there is no gradient to return")
        dev = dl.device
        g = g.detach().to(device=dev, dtype=torch.float32)
        out = torch.empty_like(dl)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().hsimae_cls_grad_scale(dl.data_ptr(), g.data_ptr(), out.data_ptr(), dl.numel(),
                                                         torch.cuda.current_stream(dev).cuda_stream), "hsimae_cls_grad_scale")
        return out, None, None, None


class ClassLoss:
    """`torch.nn.CrossEntropyLoss(reduction="mean", ignore_index=ignore_index)` for fp32 logits [N, C] on the GPU (2 <= C <= 1024),
    also the strided view `out[:, :num_class]` DualViT's head returns (read in place, the pad columns are never read).
    After a call: `last_pred` = first + argmax(logits[:, first:], 1) (int64 [N], device) and `last_n_valid` (int64 scalar, device).
    A target that is neither `ignore_index` nor a class counts as ignored and raises a flag on the device, which `check()` reads."""

    def __init__(self, ignore_index=0, first=0):
        self.ignore_index, self.first = int(ignore_index), int(first)
        self.last_pred = self.last_n_valid = None
        self._bad, self._ws = {}, {}

    def _bad_flag(self, dev):
        if dev not in self._bad:
            self._bad[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
        return self._bad[dev]

    def _workspace(self, dev, N):
        nbytes = _lib.load().hsimae_cls_workspace_bytes(N)
        if nbytes < 0:
            _lib.check(int(nbytes), "hsimae_cls_workspace_bytes")
        ws = self._ws.get(dev)
        if ws is None or ws.numel() * 8 < nbytes:
            ws = self._ws[dev] = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        return ws

    def __call__(self, logits, targets):
        _need_cuda(logits, "logits")
        _need_cuda(targets, "targets")
        if logits.dtype != torch.float32:
            raise TypeError(f"logits must be float32, got {logits.dtype}")
        if logits.dim() != 2 or targets.dim() != 1 or targets.shape[0] != logits.shape[0]:
            raise ValueError(f"logits must be [N, C] and targets [N], got {tuple(logits.shape)} and {tuple(targets.shape)}")
        if not 2 <= logits.shape[1] <= MAX_CLASSES:
            raise ValueError(f"between 2 and {MAX_CLASSES} classes are served, got {logits.shape[1]}")
        if not 0 <= self.first < logits.shape[1]:
            raise ValueError(f"first={self.first} is not one of the {logits.shape[1]} classes")
        targets = _labels(targets, "targets", logits.device)
        need_grad = torch.is_grad_enabled() and logits.requires_grad
        return _ClassLossFn.apply(logits, targets, self, need_grad)

    def check(self):
        """Raise if a target seen since the last check() was out of range (one small copy from each device used)."""
        for dev, flag in self._bad.items():
            if int(flag.item()):
                flag.zero_()
                raise RuntimeError(f"ClassLoss: a target on {dev} was neither ignore_index={self.ignore_index} nor a class index")


class ScoreMeter:
    """Confusion counts of (label, prediction) over the labeled samples (label != 0), kept on the device, and the reference's
    scores from them.  update / update_map launch and return; compute() is the one place that waits."""

    def __init__(self, num_class, device="cuda:0"):
        self.num_class = int(num_class)
        if not 2 <= self.num_class <= MAX_CLASSES:
            raise ValueError(f"between 2 and {MAX_CLASSES} classes (label 0 included) are served, got {num_class}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("hsimae_amd runs on MI355X only (no CPU fallback): ScoreMeter needs a GPU")
        self._nout = 3 + 2 * (self.num_class - 1)
        self.cm = torch.zeros(self.num_class, self.num_class, dtype=torch.int64, device=self.device)
        self._out = torch.zeros(self._nout + 1, dtype=torch.float64, device=self.device)    # the scores | the `bad` flag's 8 bytes

    def _bad_ptr(self):
        return self._out.data_ptr() + 8 * self._nout

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def reset(self):
        self.cm.zero_()
        self._out.zero_()

    def update(self, gt, pred):
        gt, pred = _labels(gt, "gt", self.device).reshape(-1), _labels(pred, "pred", self.device).reshape(-1)
        if gt.numel() != pred.numel():
            raise ValueError(f"gt has {gt.numel()} entries, pred {pred.numel()}")
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().hsimae_confusion(gt.data_ptr(), pred.data_ptr(), gt.numel(), self.num_class, self.cm.data_ptr(),
                                                    self._bad_ptr(), self._stream()), "hsimae_confusion")

    def update_map(self, gt_map, pred_map, mask_map=None):
        """Counts (gt_map, masked map) and returns the masked map (device, int64, shaped like pred_map):
        pred_map where mask_map != 0, else 0; mask_map defaults to gt_map."""
        pred = _labels(pred_map, "pred_map", self.device)
        gt = _labels(gt_map, "gt_map", self.device).reshape(-1)
        mask = None if mask_map is None else _labels(mask_map, "mask_map", self.device).reshape(-1)
        if gt.numel() != pred.numel() or (mask is not None and mask.numel() != pred.numel()):
            raise ValueError(f"the maps differ in size: gt {gt.numel()}, pred {pred.numel()}" +
                             ("" if mask is None else f", mask {mask.numel()}"))
        masked = torch.empty_like(pred)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().hsimae_confusion_map(gt.data_ptr(), _lib.ptr(mask), pred.data_ptr(), masked.data_ptr(), pred.numel(),
                                                        self.num_class, self.cm.data_ptr(), self._bad_ptr(), self._stream()),
                       "hsimae_confusion_map")
        return masked

    def compute(self):
        """-> (oa, aa, kappa, ca) as `finetune_train.scores` returns them; one device-to-host copy."""
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().hsimae_scores(self.cm.data_ptr(), self.num_class, self._out.data_ptr(), self._stream()), "hsimae_scores")
        host = self._out.cpu().numpy()
        if int(host[self._nout:].view(np.int32)[0]):
            raise RuntimeError(f"ScoreMeter: a label or a prediction was outside [0, {self.num_class})")
        k = self.num_class - 1
        ca = host[3:3 + k][host[3 + k:3 + 2 * k] != 0.0].copy()
        return float(host[0]), float(host[1]), float(host[2]), ca
