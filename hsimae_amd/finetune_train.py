"""The reference's fine-tuning entry point (Model_Finetuning.py:66-240 `dual_branch_finetuning`) on the MI355X-native
parts: same signature, same order of operations, hyper-parameters and RNG consumption per step.

  model      : hsimae_amd.DualViT (row N3), optionally initialised from a pretraining checkpoint by key (:84-96)
  data       : labeled / unlabeled / validation cubes resident in HBM (`HSIdataset` below, the reference's :26-63 with the
               same two python-`random` flip draws per training sample), batched by hsimae_amd.data.DeviceLoader
  step       : loss = lamda * loss_rec + CrossEntropy(ignore_index=0)(class_pred, y)             (:150-160)
               the cross-entropy, its gradient and the predictions are one launch pair (hsimae_amd.ClassLoss); the losses of
               an epoch are summed on the device and read once, at its end
  optimizer  : hsimae_amd.FusedAdamW (default betas), CosineLRScheduler stepped per EPOCH with
               t_initial=epochs, lr_min=lr/100, warmup_t=ceil(0.1 epochs), warmup_lr_init=lr/100  (:103-106, 236)
  metrics    : OA / AA / kappa on the labeled pixels (gt != 0, classes shifted by one)             (:171-178, 206-215)
               counted and computed on the device (hsimae_amd.ScoreMeter); `scores` below is the same arithmetic on the host
Not carried over: the matplotlib figure (:131-137, 222-233, 240-241).  The reference's defaults dim=144 / dec_dim=72 (widths that
are not multiples of the kernels' 32-deep k-step) run zero-padded to 160 / 96 inside the library.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import random

import numpy as np
import torch

from . import _lib
from .checkpoint import load_matching
from .classify import ClassLoss, ScoreMeter
from .colormap import save_label_png
from .data import DeviceLoader
from .finetune import DualViT, HSIViT, scene_views
from .optim import FusedAdamW, FusedLAMB, weights_state_dict
from .pretrain import seed_everything
from .scene_data import SceneCubes, device_scene, unlabeled_pixels
from .scene_pass import as_scene
from .sched import CosineLRScheduler
from .segment import spatial_labels, spatial_step_of


class HSIdataset:
    """Model_Finetuning.py:26-63: a list of [h, w, Bands] cubes (+ labels); training samples are flipped along w then h
    with probability 0.5 each (python `random`, horizontal draw first); items come out as [1, Bands, h, w] fp32."""

    def __init__(self, data_list, gt=None, train=False, device="cuda:0"):
        self.device = torch.device(device)
        arr = np.ascontiguousarray(np.stack([np.asarray(d, dtype=np.float32) for d in data_list]))
        self._x = torch.from_numpy(arr).to(self.device)                         # [n, h, w, Bands]
        self.gt = None if gt is None else np.asarray(gt)
        self._y = None if gt is None else torch.from_numpy(self.gt.astype(np.int64)).to(self.device)
        self.train = train

    def __len__(self):
        return self._x.shape[0]

    def batch(self, indices):
        idx = torch.as_tensor(np.asarray(indices, dtype=np.int64)).to(self.device)
        x = self._x[idx]
        if self.train:
            fh = np.zeros(len(indices), dtype=bool); fv = np.zeros(len(indices), dtype=bool)
            for i in range(len(indices)):
                fh[i] = random.random() < 0.5                                   # np.flip(data, 1): along w
                fv[i] = random.random() < 0.5                                   # np.flip(data, 0): along h
            fh_t, fv_t = torch.from_numpy(fh).to(self.device), torch.from_numpy(fv).to(self.device)
            x = torch.where(fh_t.view(-1, 1, 1, 1), x.flip(2), x)
            x = torch.where(fv_t.view(-1, 1, 1, 1), x.flip(1), x)
        x = x.permute(0, 3, 1, 2).unsqueeze(1)                                  # [n, 1, Bands, h, w] (band-fastest view)
        return x if self._y is None else (x, self._y[idx])


def spilt_dataset(data, label, training_ratio=0.8):
    """Utils/Preprocessing.py:276-300: per-class split after one np.random.permutation; the first
    (1 - ratio) * count samples of each class (in shuffled order) go to validation."""
    label = np.asarray(label)
    shuffled = np.random.permutation(np.arange(label.shape[0]))
    n_classes = len(np.unique(label))
    assert n_classes == label.max()
    val_quota = np.array([np.sum(label == c + 1) for c in range(n_classes)]) * (1 - training_ratio)
    seen = np.zeros(n_classes)
    tr, va = [], []
    for i in shuffled:
        c = label[i] - 1
        seen[c] += 1
        (va if seen[c] <= val_quota[c] else tr).append(i)
    if training_ratio == 1:
        va = tr[:int(len(tr) * 0.2)]
    return [data[i] for i in tr], label[tr], [data[i] for i in va], label[va]


def scores(gt, pred):
    """(OA, AA, kappa, per-class recall) over gt != 0 with classes shifted by one (Model_Finetuning.py:171-178):
    sklearn's accuracy_score / recall_score(average=None) / cohen_kappa_score restated on the confusion matrix."""
    gt, pred = np.asarray(gt).astype(np.int64), np.asarray(pred).astype(np.int64)
    keep = gt != 0
    g, p = gt[keep] - 1, pred[keep] - 1
    labels = np.unique(np.concatenate([g, p]))
    lut = {v: i for i, v in enumerate(labels)}
    cm = np.zeros((len(labels), len(labels)), dtype=np.float64)
    for a, b in zip(g, p):
        cm[lut[a], lut[b]] += 1
    n = cm.sum()
    oa = np.trace(cm) / n
    present = cm.sum(1) > 0
    ca = np.diag(cm)[present] / cm.sum(1)[present]                             # recall of the classes present in gt
    pe = float((cm.sum(0) * cm.sum(1)).sum()) / (n * n)
    kappa = (oa - pe) / (1 - pe) if pe < 1 else 0.0
    return float(oa), float(ca.mean()), float(kappa), ca


def val_score(oa, aa, kappa):
    """The reference's per-epoch `val_aa` (Model_Finetuning.py: the mean of OA, AA and kappa; it only plots it)."""
    return (oa + aa + kappa) / 3


def best_epoch(scores):
    """Index of the epoch `keep_best` keeps: the reference's Utils/Early_Stop.py rule with delta = 0, i.e. an epoch whose score is
    >= the best so far replaces it, so among equal scores the LAST wins.  A NaN never replaces a number; the first epoch is always
    taken.  None for an empty list."""
    best = at = None
    for i, s in enumerate(scores):
        if best is None or best != best or s >= best:
            best, at = s, i
    return at


def dual_branch_finetuning(data_list, labeled_index, unlabeled_data, gt, save_dir, model_name, pretrained=None,
                           lr=1e-3, wd=5e-3, depth=12, dim=144, dec_depth=2, dec_dim=72, s_depth=6,
                           epochs=100, mask_ratio=0.5, lamda=5, batch_size=32, device="cuda:0", log=print,
                           max_grad_norm=None, skip_nonfinite=False, layer_decay=None, freeze=(), optimizer="adamw",
                           ema_decay=None, ema_warmup=True, keep_best=False):
    """`max_grad_norm` / `skip_nonfinite` go to FusedAdamW; when either is set every epoch logs the largest gradient norm it saw and
    the number of steps skipped so far, both read in the epoch's one wait for its losses.  `layer_decay` / `freeze` go to FusedAdamW
    too (layer-wise learning-rate decay, name prefixes left out of the step); with `layer_decay` every epoch also logs the smallest
    and largest effective learning rate it stepped with, from the host's param_groups.  `optimizer`: "adamw" (the default) or
    "lamb": FusedLAMB with the same arguments and max_grad_norm 1.0 where it was left None; every epoch then also logs the smallest
    and largest trust ratio among the adapted tensors, in the same wait.

    `ema_decay` / `ema_warmup` go to the optimizer: it keeps a moving average of the weights on the device, every epoch's
    validation runs on the AVERAGED weights (inside `swap_ema()`, and its log line says so), and next to `model_name`, which stays
    the raw last-epoch weights, `<stem>_ema.pkl` is written with the same keys.  `keep_best`: the epoch whose validation
    `val_score` is the best so far (`best_epoch`'s rule; on the weights that were validated, the averaged ones with `ema_decay`)
    is copied device to device at the epoch's existing wait, and `<stem>_best.pkl` is written at the end.  The return value is
    unchanged: the last epoch's scores.  Whether either helps OA / AA / kappa on a real scene has not been measured."""
    device = torch.device(device)
    h, w, c = data_list[0].shape

    def datasets():
        data_arr = [data_list[i] for i in labeled_index]
        tr_x, tr_y, va_x, va_y = spilt_dataset(data_arr, gt, training_ratio=0.5)
        return (HSIdataset(tr_x, tr_y, train=True, device=device), HSIdataset(unlabeled_data, train=True, device=device),
                HSIdataset(va_x, va_y, device=device))

    return _finetune(datasets, h, c, gt, save_dir, model_name, pretrained, lr, wd, depth, dim, dec_depth, dec_dim, s_depth, epochs,
                     mask_ratio, lamda, batch_size, device, log, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite,
                     layer_decay=layer_decay, freeze=freeze, optimizer=optimizer, ema_decay=ema_decay, ema_warmup=ema_warmup,
                     keep_best=keep_best)


def dual_branch_finetuning_scene(scene, labeled_index, gt, save_dir, model_name, pretrained=None,
                                 lr=1e-3, wd=5e-3, depth=12, dim=144, dec_depth=2, dec_dim=72, s_depth=6,
                                 epochs=100, mask_ratio=0.5, lamda=5, batch_size=32, device="cuda:0", log=print,
                                 max_grad_norm=None, skip_nonfinite=False, layer_decay=None, freeze=(), optimizer="adamw",
                                 ema_decay=None, ema_warmup=True, keep_best=False):
    """`dual_branch_finetuning` from the scene itself: `scene` is the processed [H, W, C] `HSI_data` (get_scene_set_dual's third
    result; a device tensor is used in place), `labeled_index` the labeled pixels r * W + c and `gt` their labels.  The same
    loop, with `data_list[i]` = the padded window of pixel i and `unlabeled_data` = the scene's non-overlapping 9 x 9 tiles,
    both cut per batch on the device (scene_data.SceneCubes): no `data_cubes` is ever built.  Same np.random / torch /
    python-random consumption, same return value."""
    device = torch.device(device)
    scene = device_scene(scene, device)                                         # uploaded once, shared by the three sets
    H, W, c = (int(v) for v in scene.shape)
    device = scene.device
    sets = []

    def datasets():
        tr_i, tr_y, va_i, va_y = spilt_dataset(list(labeled_index), gt, training_ratio=0.5)
        sets.extend([SceneCubes(scene, tr_i, tr_y, train=True), SceneCubes(scene, unlabeled_pixels(H, W), train=True),
                     SceneCubes(scene, va_i, va_y)])
        return tuple(sets)

    def check():
        for ds in sets:
            ds.check()

    return _finetune(datasets, 9, c, gt, save_dir, model_name, pretrained, lr, wd, depth, dim, dec_depth, dec_dim, s_depth, epochs,
                     mask_ratio, lamda, batch_size, device, log, check, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite,
                     layer_decay=layer_decay, freeze=freeze, optimizer=optimizer, ema_decay=ema_decay, ema_warmup=ema_warmup,
                     keep_best=keep_best)


def _finetune(datasets, h, c, gt, save_dir, model_name, pretrained, lr, wd, depth, dim, dec_depth, dec_dim, s_depth, epochs, mask_ratio,
              lamda, batch_size, device, log, check_data=None, max_grad_norm=None, skip_nonfinite=False, layer_decay=None, freeze=(), optimizer="adamw",
              ema_decay=None, ema_warmup=True, keep_best=False):
    """The loop of Model_Finetuning.py:66-240.  `datasets()` -> (labeled, unlabeled, validation), called where the reference
    splits the labeled set (after the model's initialisation draws); `check_data()` once per epoch, with the loss's check."""
    n_class = int(np.max(gt) + 1)
    model = DualViT(img_size=h, patch_size=3, in_chans=1, bands=c, b_patch_size=8, num_class=n_class,
                    embed_dim=dim, depth=depth, num_heads=dim // 16, s_depth=s_depth,
                    decoder_embed_dim=dec_dim, decoder_depth=dec_depth, decoder_num_heads=dec_dim // 8,
                    norm_pix_loss=True, trunc_init=True, drop_path=0.2).to(device)
    save_path = os.path.join(save_dir, model_name.replace(".pkl", ""))
    os.makedirs(save_path, exist_ok=True)
    if pretrained:
        load_matching(model, pretrained, device, match_shapes=False).train()

    if optimizer not in ("adamw", "lamb"):
        raise ValueError(f'optimizer must be "adamw" or "lamb", got {optimizer!r}')
    lamb = optimizer == "lamb"
    if lamb:
        optimizer = FusedLAMB(model, lr=lr, weight_decay=wd, max_grad_norm=1.0 if max_grad_norm is None else max_grad_norm,
                              skip_nonfinite=skip_nonfinite, layer_decay=layer_decay, freeze=freeze, ema_decay=ema_decay,
                              ema_warmup=ema_warmup)
    else:
        optimizer = FusedAdamW(model, lr=lr, weight_decay=wd, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite,
                               layer_decay=layer_decay, freeze=freeze, ema_decay=ema_decay, ema_warmup=ema_warmup)
    clipped = max_grad_norm is not None or skip_nonfinite or lamb
    scheduler = CosineLRScheduler(optimizer, t_initial=epochs, lr_min=lr * 0.01, warmup_t=int(np.ceil(0.1 * epochs)),
                                  warmup_lr_init=lr * 0.01)
    criterion = ClassLoss(ignore_index=0)
    meter = ScoreMeter(n_class, device)

    train_ds, unl_ds, val_ds = datasets()
    train_dl = DeviceLoader(train_ds, batch_size=batch_size, shuffle=True)
    unl_bs = int(np.ceil(len(unl_ds) / len(train_dl)) / 2)
    unl_dl = DeviceLoader(unl_ds, batch_size=unl_bs, shuffle=True)
    val_dl = DeviceLoader(val_ds, batch_size=512, shuffle=False)
    log(f"train {len(train_ds)} labeled / {len(unl_ds)} unlabeled cubes, {len(train_dl)} iterations per epoch")

    epoch_loss_list, val_loss_list, val_value = [], [], None
    ema = ema_decay is not None
    head = [p for n, p in model.named_parameters() if n.startswith("cls_head.")]
    val_scores, best_flat, best_head = [], None, None
    for epoch in range(epochs):
        model.train()
        seed_everything(42 + epoch); labeled_iter = iter(train_dl)              # `stable(loader, 42 + epoch)` twice
        seed_everything(42 + epoch); unlabeled_iter = iter(unl_dl)
        train_loss = torch.zeros((), dtype=torch.float64, device=device)         # summed on the device, read once per epoch
        lr_lo, lr_hi = optimizer.lr_range()                                     # the scheduler writes once per epoch
        for _ in range(len(train_dl)):
            x, y = next(labeled_iter)
            x_u = next(unlabeled_iter)
            loss_rec, _, _, outputs = model(x, x_u, mask_ratio=mask_ratio)
            loss = lamda * loss_rec + criterion(outputs, y)
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            train_loss += loss.detach()

        model.eval()
        with torch.no_grad(), (optimizer.swap_ema() if ema else contextlib.nullcontext()):
            seed_everything(42 + epoch)
            val_loss = torch.zeros((), dtype=torch.float64, device=device)
            meter.reset()
            for x, y in val_dl:
                outputs = model(x, mask_ratio=mask_ratio)
                val_loss += criterion(outputs, y)
                meter.update(y, criterion.last_pred)
            val_value = list(meter.compute())
            if ema or keep_best:
                val_scores.append(val_score(*val_value[:3]))
                log(f"epoch {epoch}: validated on the {'EMA' if ema else 'raw'} weights: OA {val_value[0]:.6f}, AA {val_value[1]:.6f}, "
                    f"kappa {val_value[2]:.6f}, val_aa {val_scores[-1]:.6f}")
            if keep_best and best_epoch(val_scores) == epoch:                   # the weights just validated, device to device
                if best_flat is None:
                    best_flat, best_head = torch.empty_like(model._flat), [torch.empty_like(p) for p in head]
                best_flat.copy_(model._flat)
                for b, p in zip(best_head, head):
                    b.copy_(p)
        if clipped:                                                             # the same wait also brings the norm and the count
            read = torch.stack([train_loss, val_loss, optimizer.grad_norm_max.double(), optimizer.skipped_steps.double()])
            if lamb:
                read = torch.cat([read, optimizer.trust_ratio_range()])
            vals = read.tolist()                                                # the epoch's one wait
            tr, va, norm_max, skipped = vals[:4]
            optimizer.reset_grad_norm_max()
            log(f"epoch {epoch}: train loss {tr / len(train_dl):.6f}, largest gradient norm {norm_max:.6g}, "
                f"{int(skipped)} steps skipped so far" + (f", trust ratio {vals[4]:.6g} .. {vals[5]:.6g}" if lamb else ""))
        else:
            tr, va = torch.stack([train_loss, val_loss]).tolist()               # the epoch's one wait for its losses
        if layer_decay is not None:
            log(f"epoch {epoch}: learning rate {lr_lo:.6g} .. {lr_hi:.6g} over {len(optimizer.param_groups)} groups")
        criterion.check()
        if check_data is not None:
            check_data()
        epoch_loss_list.append(tr / len(train_dl))
        val_loss_list.append(va / len(val_dl))
        scheduler.step(epoch)

    torch.save(model.state_dict(), os.path.join(save_dir, model_name))
    stem = os.path.join(save_dir, os.path.splitext(model_name)[0])
    if ema:
        torch.save(optimizer.ema_state_dict(), stem + "_ema.pkl")
    if keep_best and best_flat is not None:
        at = best_epoch(val_scores)
        torch.save(weights_state_dict(model, best_flat, list(zip(head, best_head))), stem + "_best.pkl")
        log(f"best epoch {at}: val_aa {val_scores[at]:.6f} on the {'EMA' if ema else 'raw'} weights -> {stem}_best.pkl")
    return val_value, epoch_loss_list, val_loss_list


def eval_vit(img_size, bands, n_class, dim, depth, s_depth, device):
    """The evaluation model of the five wrappers below: the reference's HSIViT (Model_Finetuning.py:250-255) at these widths."""
    return HSIViT(img_size=img_size, patch_size=3, in_chans=1, bands=bands, b_patch_size=8, num_class=n_class, embed_dim=dim,
                  depth=depth, num_heads=dim // 16, s_depth=s_depth, sep_pos_embed=True, use_learnable_pos_emb=False).to(device)


def test_model(data_cubes, test_gt, gt, save_dir, model_name, depth=12, dim=96, s_depth=6, device="cuda:0", save_images=False):
    """Model_Finetuning.test_model (:243-300): every cube of the scene through HSIViT loaded key-filtered from the
    fine-tuned checkpoint, class = 1 + argmax over logits[:, 1:], scores on the labeled test pixels.
    -> (oa, aa, kappa, per-class recall, prediction map shaped like `gt`).  save_images=True also writes the reference's two
    colour-map PNGs (:282-285, 299-300; `_save_maps`)."""
    device = torch.device(device)
    h, w, c = data_cubes[0].shape
    n_class = int(np.max(gt) + 1)
    model = load_matching(eval_vit(h, c, n_class, dim, depth, s_depth, device), os.path.join(save_dir, model_name), device,
                          match_shapes=False)
    dataset = HSIdataset(data_cubes, device=device)
    lib = _lib.load()
    n_total = len(dataset)
    pred = torch.zeros(n_total, dtype=torch.int64, device=device)
    with torch.no_grad(), torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        k0 = 0
        for x in DeviceLoader(dataset, batch_size=256, shuffle=False):
            logits = model(x)
            # label = 1 + argmax(logits[:, 1:]) written in place into the device-resident map, as predict_scene does
            sp = _lib.SceneParams(H=1, W=n_total, C=c, p0=k0, N=int(logits.shape[0]))
            _lib.check(lib.hsimae_class_argmax(C.byref(sp), logits.data_ptr(), logits.stride(0), n_class, 1, pred.data_ptr(), stream),
                       "hsimae_class_argmax")
            k0 += int(logits.shape[0])
    return _score_and_save(pred.view(np.asarray(gt).shape), test_gt, gt, n_class, device, save_dir, model_name, save_images)


def _scene_scores(pred, test_gt, gt, n_class, device, want_masked=False):
    """Model_Finetuning.py:285-290 on the device: the prediction map zeroed where `gt` is 0, counted against `test_gt`.
    want_masked=True: -> (scores, that zeroed map)."""
    meter = ScoreMeter(n_class, device)
    masked = meter.update_map(np.asarray(test_gt).reshape(-1), pred.reshape(-1), mask_map=np.asarray(gt).reshape(-1))
    return (meter.compute(), masked) if want_masked else meter.compute()


def _save_maps(save_dir, model_name, oa, pred, masked):
    """The reference's two pictures (:267-269, 282-285, 299-300) in <save_dir>/<stem>/: <stem>_all_oa_<OA %>.png from the whole
    prediction map and <stem>_oa_<OA %>.png from the map zeroed where the scene has no label."""
    save_path = os.path.join(save_dir, model_name.replace(".pkl", ""))
    os.makedirs(save_path, exist_ok=True)
    tag = str(np.around(oa * 100, 2))
    save_label_png(os.path.join(save_path, model_name.replace(".pkl", "_all_oa_" + tag + ".png")), pred)
    save_label_png(os.path.join(save_path, model_name.replace(".pkl", "_oa_" + tag + ".png")), masked)


def _score_and_save(pred, test_gt, gt, n_class, device, save_dir, model_name, save_images):
    """What test_model and test_model_scene end with: the scores of the device-resident map `pred`, the pictures if asked for."""
    shape = np.asarray(gt).shape
    (oa, aa, kappa, ca), masked = _scene_scores(pred, test_gt, gt, n_class, device, want_masked=True)
    if save_images:
        _save_maps(save_dir, model_name, oa, pred.view(shape), masked.view(shape))
    return oa, aa, kappa, ca, pred.cpu().numpy().reshape(shape)


def test_model_scene(scene, test_gt, gt, save_dir, model_name, depth=12, dim=96, s_depth=6, device="cuda:0", batch_size=8192,
                     views=(0,), save_images=False, smooth=None):
    """`test_model` from the scene itself: `scene` is the [H, W, C] `HSI_data` the reference cuts `data_cubes` from
    (Utils/Preprocessing.py:189-213, after GWPCA / norm), fp32 or fp64.  The same model, loaded the same way; the windows are
    cut on the device (HSIViT.predict_scene, at most `batch_size` pixels per chunk) instead of being built on the host.
    `views` other than (0,): the label of the class probabilities averaged over these flips of every window
    (HSIViT.classify_scene; "flips" = all four).  save_images=True also writes the reference's two colour-map PNGs.
    `smooth`: None (the default) changes nothing; an EdgeFilter (True: the default one) filters the class-probability maps with
    the scene's first principal component as the guide before the argmax (smooth.EdgeFilter, smooth.scene_guide); a Superpixels
    segments the scene's first three principal components and lets every superpixel decide by its mean class probabilities
    (segment.Superpixels, segment.segment_vote).  The map after that step is what is scored, pictured and returned.
    -> (oa, aa, kappa, per-class recall, prediction map shaped like `gt`), as test_model returns them."""
    device = torch.device(device)
    views = scene_views(views)
    if len(scene.shape) != 3:
        raise ValueError(f"scene must be [H, W, C], got shape {tuple(scene.shape)}")
    c = int(scene.shape[2])
    n_class = int(np.max(gt) + 1)
    model = load_matching(eval_vit(9, c, n_class, dim, depth, s_depth, device), os.path.join(save_dir, model_name), device,
                          match_shapes=False)
    filt = spatial_step_of(smooth)
    if filt is not None:
        scene = as_scene(scene).to(device)                 # uploaded once: the classification and the guide share it
        res = model.classify_scene(scene, batch_size=batch_size, views=views, return_probs=True, on_device=True)
        pred = spatial_labels(filt, res, scene)
    elif views != (0,) or save_images:
        pred = model.classify_scene(scene, batch_size=batch_size, views=views, on_device=True).labels
    else:
        pred = model.predict_scene(scene, batch_size=batch_size, on_device=True)
    return _score_and_save(pred, test_gt, gt, n_class, device, save_dir, model_name, save_images)


def knn_eval_scene(scene, train_index, train_labels, test_gt, gt, pretrained, depth=12, dim=96, s_depth=6, k=20, temperature=0.07,
                   bank_flips=(0,), device="cuda:0", batch_size=8192, save_dir=None, model_name=None, save_images=False, smooth=None):
    """The evaluation of a checkpoint that needs no fine-tuning: a weighted k-NN classifier on the frozen encoder's pooled features
    (Wu et al. 2018; DINO's knn_classifier), over the whole scene.  Inputs are what get_scene_set_dual returns: `scene` the
    processed [H, W, C] `HSI_data`, `train_index` / `train_labels` the labelled pixels that form the bank, `test_gt` / `gt` as in
    test_model_scene.  `pretrained`: the path of a state dict, loaded key-filtered as dual_branch_finetuning loads it: a
    pretraining checkpoint (HSIMAE) and a fine-tuned one (DualViT) both work, the classification head is never used.
    `k`, `temperature`, `bank_flips`: HSIViT.knn_scene's.  save_images=True writes test_model_scene's two pictures into
    <save_dir>/<stem of model_name>/ (model_name defaults to the checkpoint's file name).  `smooth`: test_model_scene's, applied to
    the vote's class probabilities.
    -> (oa, aa, kappa, per-class recall, prediction map shaped like `gt`), scored as test_model_scene scores."""
    device = torch.device(device)
    bank_flips = scene_views(bank_flips)
    filt = spatial_step_of(smooth)
    if len(scene.shape) != 3:
        raise ValueError(f"scene must be [H, W, C], got shape {tuple(scene.shape)}")
    if save_images and save_dir is None:
        raise ValueError("save_images=True needs save_dir")
    c = int(scene.shape[2])
    n_class = int(np.max(gt) + 1)
    model = load_matching(eval_vit(9, c, n_class, dim, depth, s_depth, device), pretrained, device, match_shapes=True)
    if filt is not None:
        scene = as_scene(scene).to(device)                 # uploaded once: the classification and the guide share it
    res = model.knn_scene(scene, train_index, train_labels, k=k, temperature=temperature, bank_flips=bank_flips,
                          batch_size=batch_size, return_probs=filt is not None, on_device=True)
    pred = res.labels if filt is None else spatial_labels(filt, res, scene)
    name = os.path.basename(str(pretrained)) if model_name is None else model_name
    return _score_and_save(pred, test_gt, gt, n_class, device, save_dir, name, save_images)


def svm_eval_scene(scene, train_index, train_labels, test_gt, gt, pretrained=None, features="spectra", search=True, C=1.0,
                   gamma="scale", depth=12, dim=96, s_depth=6, bank_flips=(0,), device="cuda:0", batch_size=8192, save_dir=None,
                   model_name=None, save_images=False, smooth=None):
    """The baseline the reference reports next to its deep models (Compared_Methods/svm_rbf.py): an RBF-kernel support-vector
    machine, over the whole scene, on the device (HSIViT.svm_scene, svm.RBFSVM).  Inputs as knn_eval_scene's: `scene` the
    processed [H, W, C] `HSI_data`, `train_index` / `train_labels` the labelled pixels the machine is fitted on (at most 8192),
    `test_gt` / `gt` as in test_model_scene.  features="spectra" (the reference's baseline: centre-pixel spectra, no encoder;
    `pretrained` may be None: a model is then built for the band count only and never run) or "encoder" (the frozen encoder's
    pooled features: `pretrained` is the path of a state dict, loaded as knn_eval_scene loads it).  search=True runs the
    reference's two-stage grid search over C and gamma (RBFSVM.fit_reference; it draws its splits from numpy's global
    generator); search=False fits once at `C`, `gamma`.  None of these defaults is tuned on a real scene.  save_images=True
    writes test_model_scene's two pictures into <save_dir>/<stem of model_name>/ (model_name defaults to the checkpoint's
    file name, or "svm_rbf.pkl").  `smooth`: test_model_scene's (None, True, an EdgeFilter or a Superpixels), applied to the
    machine's vote shares.
    -> (oa, aa, kappa, per-class recall, prediction map shaped like `gt`), scored as test_model_scene scores."""
    device = torch.device(device)
    filt = spatial_step_of(smooth)
    if len(scene.shape) != 3:
        raise ValueError(f"scene must be [H, W, C], got shape {tuple(scene.shape)}")
    if save_images and save_dir is None:
        raise ValueError("save_images=True needs save_dir")
    if features == "encoder" and pretrained is None:
        raise ValueError('features="encoder" needs a pretrained checkpoint')
    c = int(scene.shape[2])
    n_class = int(np.max(gt) + 1)
    model = eval_vit(9, c + (-c) % 8, n_class, dim, depth, s_depth, device)          # (spectra: any band count; never run)
    if pretrained is not None:
        model = load_matching(model, pretrained, device, match_shapes=True)
    if filt is not None:
        scene = as_scene(scene).to(device)                 # uploaded once: the classification and the guide share it
    res = model.svm_scene(scene, train_index, train_labels, features=features, C=C, gamma=gamma, search=search,
                          bank_flips=bank_flips, batch_size=batch_size, return_probs=filt is not None, on_device=True)
    model.last_svm.check()
    pred = res.labels if filt is None else spatial_labels(filt, res, scene)
    name = model_name or (os.path.basename(str(pretrained)) if pretrained is not None else "svm_rbf.pkl")
    return _score_and_save(pred, test_gt, gt, n_class, device, save_dir, name, save_images)


def linear_probe_scene(scene, train_index, train_labels, test_gt, gt, pretrained, depth=12, dim=96, s_depth=6, bank_flips=(0,),
                       views=(0,), device="cuda:0", batch_size=8192, save_dir=None, model_name=None, save_images=False,
                       smooth=None, **probe_kwargs):
    """The evaluation masked-autoencoder work reports first: a linear classifier on the frozen encoder's pooled features, trained
    on the device on the cached features of the labelled pixels (HSIViT.probe_scene, probe.LinearProbe), over the whole scene.
    Inputs as knn_eval_scene's: `scene` the processed [H, W, C] `HSI_data`, `train_index` / `train_labels` the labelled pixels the
    probe is fitted on, `test_gt` / `gt` as in test_model_scene; `pretrained` the path of a state dict, loaded key-filtered as
    knn_eval_scene loads it (a pretraining and a fine-tuned checkpoint both work; a fine-tuned head is replaced by the probe).
    `bank_flips`, `views`, `probe_kwargs` (max_iter, lr, weight_decay, ..): probe_scene's.  The defaults are not tuned on a real scene.
    With `save_dir` the probed model's state dict (HSIViT's own, as dual_branch_finetuning saves it: encoder as loaded, head = the probe) is
    written as <save_dir>/<stem of model_name>_probe.pkl, which test_model_scene and the reference's test_model load;
    model_name defaults to the checkpoint's file name.  save_images=True also writes test_model_scene's two pictures.
    `smooth`: test_model_scene's, applied to the probe's class probabilities.
    -> (oa, aa, kappa, per-class recall, prediction map shaped like `gt`), scored as test_model_scene scores."""
    device = torch.device(device)
    bank_flips, views = scene_views(bank_flips), scene_views(views)
    filt = spatial_step_of(smooth)
    if len(scene.shape) != 3:
        raise ValueError(f"scene must be [H, W, C], got shape {tuple(scene.shape)}")
    if save_images and save_dir is None:
        raise ValueError("save_images=True needs save_dir")
    c = int(scene.shape[2])
    n_class = int(np.max(gt) + 1)
    model = load_matching(eval_vit(9, c, n_class, dim, depth, s_depth, device), pretrained, device, match_shapes=True)
    if filt is not None:
        scene = as_scene(scene).to(device)                 # uploaded once: the classification and the guide share it
    res = model.probe_scene(scene, train_index, train_labels, bank_flips=bank_flips, views=views, batch_size=batch_size,
                            return_probs=filt is not None, on_device=True, **probe_kwargs)
    pred = res.labels if filt is None else spatial_labels(filt, res, scene)
    model.last_probe.check()
    name = os.path.basename(str(pretrained)) if model_name is None else model_name
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        stem = name[:-4] if name.endswith(".pkl") else name
        torch.save(model.state_dict(), os.path.join(save_dir, stem + "_probe.pkl"))
    return _score_and_save(pred, test_gt, gt, n_class, device, save_dir, name, save_images)


def cluster_eval_scene(scene, gt, pretrained, n_clusters=None, depth=12, dim=96, s_depth=6, features="encoder", metric=None, flip=0,
                       max_iter=20, n_init=1, generator=None, init="random", fit_pixels=None, device="cuda:0", batch_size=8192,
                       save_dir=None, model_name=None, save_images=False):
    """The evaluation of a checkpoint that needs no label to produce its map: k-means on the frozen encoder's pooled features over
    the whole scene (HSIViT.cluster_scene), scored against `gt` the way the unsupervised HSI literature scores a clustering.
    `pretrained`: the path of a state dict, loaded as knn_eval_scene loads it (a pretraining and a fine-tuned checkpoint both
    work); it may be None with features="spectra", the classical baseline of k-means on the spectra themselves, which runs no
    encoder.  `n_clusters` defaults to the number of real classes in `gt` (distinct labels other than 0).  `features`, `metric`,
    `flip`, `max_iter`, `n_init`, `generator`, `init`, `fit_pixels`: cluster_scene's.
    The contingency counts of (gt, cluster) over the labelled pixels are taken on the device (ScoreMeter with max(clusters,
    classes) + 1 labels); from that small table, on the host in fp64 (hsimae_amd.cluster): the one-to-one matching of clusters to
    classes that maximises the matched pixels (Hungarian), clusters left unmatched mapped to their majority class, then
    `scores` on the mapped map, and purity, NMI (arithmetic-mean normalisation) and ARI of the raw partition.
    save_images=True writes test_model_scene's two pictures from the mapped map into <save_dir>/<stem of model_name>/, which
    needs every class label inside the colour palette: otherwise ValueError, before anything is clustered.
    -> (oa, aa, kappa, per-class recall, nmi, ari, purity, mapped prediction map, raw cluster map), both maps int64 shaped like gt."""
    from .cluster import ari, cluster_mapping, nmi, purity
    from .colormap import PALETTE
    device = torch.device(device)
    if len(scene.shape) != 3:
        raise ValueError(f"scene must be [H, W, C], got shape {tuple(scene.shape)}")
    if features not in ("encoder", "spectra"):
        raise ValueError(f'features must be "encoder" or "spectra", got {features!r}')
    if pretrained is None and features == "encoder":
        raise ValueError('features="encoder" needs a pretrained checkpoint')
    gt = np.asarray(gt)
    if gt.shape != tuple(scene.shape[:2]) or gt.dtype.kind not in "iu" or gt.min() < 0:
        raise ValueError(f"gt must be a map of non-negative integer labels shaped {tuple(scene.shape[:2])}")
    classes = np.unique(gt[gt != 0])
    if not classes.size:
        raise ValueError("gt holds no labelled pixel")
    n_class = int(classes.max()) + 1
    K = int(classes.size if n_clusters is None else n_clusters)
    if save_images:
        if save_dir is None:
            raise ValueError("save_images=True needs save_dir")
        if n_class > PALETTE.shape[0]:
            raise ValueError(f"save_images=True: label {n_class - 1} is outside the palette's {PALETTE.shape[0]} colours")
    c = int(scene.shape[2])
    bands = c if features == "encoder" else 32                 # (the spectra path never runs the encoder)
    model = eval_vit(9, bands, n_class, dim, depth, s_depth, device).eval()
    if pretrained is not None and features == "encoder":
        load_matching(model, pretrained, device, match_shapes=True)
    raw = model.cluster_scene(scene, K, fit_pixels=fit_pixels, features=features, metric=metric, flip=flip, max_iter=max_iter,
                              n_init=n_init, generator=generator, batch_size=batch_size, on_device=True, init=init).labels
    meter = ScoreMeter(max(K, n_class - 1) + 1, device)
    meter.update(gt.reshape(-1), raw.reshape(-1))              # rows: gt, columns: cluster; gt = 0 is not counted
    table = meter.cm.cpu().numpy().astype(np.float64)[1:n_class, 1:K + 1]
    present = np.flatnonzero(table.sum(1) > 0)                 # classes 1 + present
    lut = np.zeros(K + 1, np.int64)
    lut[1:] = 1 + present[cluster_mapping(table[present])]
    raw = raw.cpu().numpy().reshape(gt.shape)
    mapped = lut[raw]
    oa, aa, kappa, ca = scores(gt.reshape(-1), mapped.reshape(-1))
    if save_images:
        name = os.path.basename(str(pretrained)) if model_name is None else model_name
        _save_maps(save_dir, name, oa, mapped, np.where(gt == 0, 0, mapped))
    return oa, aa, kappa, ca, nmi(table), ari(table), purity(table), mapped, raw
