"""Row N3: the dual-branch fine-tuning model (`Models.DualViT`, Models.py:637-993) on the MI355X-native
kernels — inference AND the fine-tuning step (Model_Finetuning.py:150-156).

  class_pred = cls_head(AGG(norm(encoder(imgs))))                      (forward_encoder :869-894, head :962-970)
  with imgs_u: the masked-autoencoder path on concat(imgs, imgs_u)      (forward :975-993) — the pretraining hot path
  training mode: DropPath (stochastic depth, Models.py:235-263) on both residual branches of every encoder block,
  rate linspace(0, drop_path, depth)[i] (:687), one Bernoulli factor per sequence of the block's input.

Same constructor keywords, same parameter names / order / init stream as the reference (the head is registered
between `norm` and `decoder_embed`), so checkpoints load both ways.  Everything on the encoder / decoder runs through
the HIP library: `hsimae_encode` (+ `hsimae_encode_backward`) = the masked schedule with the full token grid and
identity order, `hsimae_forward` / `hsimae_backward` for the reconstruction branch, DropPath as per-row factor vectors
(`hsimae_io.drop_scale`), `hsimae_agg_pool` + `hsimae_gemm` for the head's forward.  The head's backward (an
[N, T*D] x [classes, T*D] product) is three torch matmuls on the device.
RNG: DropPath factors are drawn from torch's generator of the input's device in the reference's order (classification
pass, then grid / masking noise, then reconstruction pass); `drop_factors=` replaces the draws (parity tests).
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .model import HSIMAE
from .scene_pass import ScenePass, as_scene, gpu_of, largest_chunk, pixel_indices, to_host

# what DualViT.classify_scene returns
SceneClassification = collections.namedtuple("SceneClassification", ["labels", "confidence", "margin", "probs"])


def scene_views(views):
    """classify_scene's `views` as a tuple of distinct flip codes in 0 .. 3 (bit 0: along w, bit 1: along h); "flips" is all four."""
    if isinstance(views, str):
        if views != "flips":
            raise ValueError(f'views must be "flips" or a tuple of flip codes 0 .. 3, got {views!r}')
        return (0, 1, 2, 3)
    try:
        out = tuple(views)
    except TypeError:
        raise ValueError(f'views must be "flips" or a tuple of flip codes 0 .. 3, got {views!r}') from None
    if not out or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 3 for v in out):
        raise ValueError(f"views must be a non-empty tuple of flip codes 0 .. 3, got {views!r}")
    if len(set(out)) != len(out):
        raise ValueError(f"views repeats a flip code: {views!r}")
    return tuple(int(v) for v in out)


def scene_array(scene, bands, batch_size):
    """The checks every whole-scene entry point that runs the encoder makes of its `scene` and `batch_size` (DualViT._scene_args,
    reconstruct_scene): scene_pass.as_scene, and bands the model can take -> (scene tensor, H, W, bands)."""
    s = as_scene(scene)
    H, W, Cb = (int(v) for v in s.shape)
    if Cb % 8:
        raise ValueError(f"scene has {Cb} bands: the band count must be a multiple of 8 (b_patch_size)")
    if Cb != bands:
        raise ValueError(f"scene has {Cb} bands, the model was built for bands={bands}")
    if int(batch_size) < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    return s, H, W, Cb


class _FineTuneStep(torch.autograd.Function):
    """DualViT.forward in training as one autograd node: encoder / decoder parameter gradients are written by the kernels
    into the model's flat gradient buffer; the head's two parameters are ordinary autograd inputs."""

    @staticmethod
    def forward(ctx, anchor, head_w, head_b, model, imgs, imgs_u, ratio, noise, grid, drop_factors):
        out = model._train_forward(imgs, imgs_u, ratio, noise, grid, drop_factors)
        ctx.model, ctx.saved = model, out["saved"]
        if imgs_u is None:
            return out["class_pred"]
        ctx.mark_non_differentiable(out["pred_rec"], out["mask"])
        return out["loss_rec"], out["pred_rec"], out["mask"], out["class_pred"]

    @staticmethod
    def backward(ctx, *gs):
        g_loss, g_cls = (None, gs[0]) if len(gs) == 1 else (gs[0], gs[3])
        gw, gb = ctx.model._train_backward(ctx.saved, g_loss, g_cls)
        return None, gw, gb, None, None, None, None, None, None, None


class DualViT(HSIMAE):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=1024, depth=24, s_depth=6, num_heads=16,
                 mlp_ratio=4.0, norm_layer=nn.LayerNorm, bands=32, b_patch_size=8, num_class=100, no_qkv_bias=False,
                 trunc_init=False, drop_path=0., decoder_embed_dim=512, decoder_depth=8, decoder_num_heads=16,
                 norm_pix_loss=False, **kwargs):
        super().__init__(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim, depth=depth,
                         num_heads=num_heads, decoder_embed_dim=decoder_embed_dim, decoder_depth=decoder_depth,
                         decoder_num_heads=decoder_num_heads, mlp_ratio=mlp_ratio, norm_layer=norm_layer,
                         norm_pix_loss=norm_pix_loss, bands=bands, b_patch_size=b_patch_size, no_qkv_bias=no_qkv_bias,
                         trunc_init=trunc_init, s_depth=s_depth, _num_class=num_class)
        self.drop_path = drop_path            # stochastic depth: active in training mode only (Models.py:244)
        self.num_class = num_class
        self._head_pack = None

    # ------------------------------------------------------------------ unmasked encoder (Models.py:869-894)
    def forward_encoder(self, x):
        """-> latent [N, T*9, D]: every token kept, natural order (the masked schedule with the full grid)."""
        T, L = self.input_size[0], self.input_size[1] ** 2
        N = x.shape[0]
        n1 = torch.arange(T, dtype=torch.float32).expand(N, T)          # increasing noise => ids_keep = identity
        n2 = torch.arange(L, dtype=torch.float32).expand(N, L)
        with torch.no_grad():
            _, _, _, st = self._run_forward(x, 0.0, (n1, n2), (T, L), want_latent=True, encoder_only=True)
        return st["latent"]

    def forward_mask_encoder(self, x, mask_ratio, noise=None, grid=None):
        """DualViT's name for the masked encoder (Models.py:896-921) = HSIMAE.forward_encoder; inference only."""
        return HSIMAE.forward_encoder(self, x, mask_ratio, noise, grid)

    def _packed_head(self, dev):
        w = self.cls_head.weight
        key = (w._version, self.cls_head.bias._version, dev)
        if self._head_pack is None or self._head_pack[0] != key:
            nc, k = w.shape
            npad = (nc + 15) // 16 * 16
            kp = (k + 31) // 32 * 32                          # K extent of the image: whole MFMA k-steps (T * D need not be one)
            img = torch.zeros(npad * kp, dtype=torch.bfloat16, device=dev)
            src = w.detach().to(device=dev, dtype=torch.float32).contiguous()
            desc = (_lib.PackDesc * 1)(_lib.PackDesc(src=src.data_ptr(), rows=nc, cols=k, transpose=0, n_off=0, k_off=0,
                                                     KS=kp // 32, dst=img.data_ptr()))
            table = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8).clone().to(dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(_lib.load().hsimae_pack_matrix(table.data_ptr(), 1, src.numel(), stream), "hsimae_pack_matrix")
            bias = torch.zeros(npad, dtype=torch.float32, device=dev)      # padded: the F32 epilogue stores whole octets
            bias[:nc] = self.cls_head.bias.detach().to(device=dev, dtype=torch.float32)
            self._head_pack = (key, img, bias, npad, (src, table))
        return self._head_pack[1], self._head_pack[2], self._head_pack[3]

    def head(self, x, type="AGG"):
        """(class_pred [N, num_class], pooled [N, T*D]); 'AGG' only (the reference's default and only caller)."""
        if type != "AGG":
            raise NotImplementedError("only the 'AGG' head is built")
        N = x.shape[0]
        T, L, D = self.input_size[0], self.input_size[1] ** 2, self.dim
        lib = _lib.load()
        dev = x.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        x = x.contiguous()
        pooled = torch.empty(N, T * D, dtype=torch.float32, device=dev)
        _lib.check(lib.hsimae_agg_pool(x.data_ptr(), pooled.data_ptr(), N, T, L, D, stream), "hsimae_agg_pool")
        img, bias, npad = self._packed_head(dev)
        out = torch.empty(N, npad, dtype=torch.float32, device=dev)
        k, kp = T * D, (T * D + 31) // 32 * 32
        a = pooled
        if kp != k:                                           # zero-padded operand rows (whole k-steps)
            a = torch.zeros(N, kp, dtype=torch.float32, device=dev)
            a[:, :k] = pooled
        p = _lib.GemmParams(A=a.data_ptr(), lda=kp, M=N, N=npad, K=kp, n_valid=npad, W=img.data_ptr(),
                            bias=bias.data_ptr(), out=out.data_ptr(), ldo=npad)
        _lib.check(lib.hsimae_gemm(C.byref(p), _lib.A_F32, _lib.E_F32, stream), "hsimae_gemm")
        return out[:, :self.num_class], pooled

    # ------------------------------------------------------------------ whole-scene inference (Model_Finetuning.py:243-300)
    # hsimae_encode's arena takes ~4 MB per window at Base width (~8 MB at Large): the default chunk is the largest one whose
    # arena fits this budget, and never more than `batch_size` pixels
    SCENE_WORKSPACE_BUDGET = 8 << 30

    def _scene_chunk(self, batch_size):
        grid = (self.input_size[0], self.input_size[1] ** 2)      # the unmasked encoder keeps the full token grid
        return largest_chunk(_lib.load(), self._config(), [grid], batch_size, self.SCENE_WORKSPACE_BUDGET)

    def _scene_pass(self, scene, pixels, batch_size, by_p0=False):
        """The argument checks the entry points share (scene, batch_size, pixels; the device last) and the ScenePass over `pixels`;
        over all pixels (None): the index list arange(H * W), or with by_p0 no list (hsimae_scene_windows' range from p0)."""
        s, H, W, _ = scene_array(scene, self.patch_embed.bands, batch_size)
        pix = None if pixels is None else pixel_indices(pixels, H * W)
        if pix is None and not by_p0:
            pix = torch.arange(H * W, dtype=torch.int64, device=gpu_of(self))
        return ScenePass(self, s, pix, self._scene_chunk(batch_size))

    def predict_scene(self, scene, pixels=None, batch_size=8192, return_logits=False, on_device=False):
        """Per-pixel classification map of a whole scene (what `test_model` computes from `data_cubes`, :268-283), from the
        scene itself: `scene` [H, W, C] fp32 / fp64 (numpy or tensor; the `HSI_data` of get_data_set_dual after GWPCA / norm)
        is uploaded once; per chunk of pixels, on the current stream: the symmetric-padded 9 x 9 windows (hsimae_scene_windows),
        the unmasked encoder (hsimae_encode), the AGG head, and label = 1 + argmax(logits[:, 1:]) written in place into a
        device-resident map (hsimae_class_argmax).  The host waits once, for the final copy.
        Evaluates as in eval mode (no DropPath), without autograd.  `pixels`: row-major pixel indices r * W + c to classify
        (default: all); the map is 0 elsewhere.  `batch_size` caps the pixels per chunk; the chunk is also kept small enough
        for the encoder's workspace to fit SCENE_WORKSPACE_BUDGET bytes.
        -> int64 [H, W] map (CPU), and with return_logits=True also fp32 [n, num_class] logits (CPU) in pixel order.
        on_device=True: both stay on the model's device and nothing waits for the host."""
        sp = self._scene_pass(scene, pixels, batch_size, by_p0=True)
        lib, H, W, dev = _lib.load(), sp.H, sp.W, sp.dev
        with torch.no_grad(), torch.cuda.device(dev):
            labels = torch.zeros(H * W, dtype=torch.int64, device=dev)
            logits_all = torch.empty(sp.n_total, self.num_class, dtype=torch.float32, device=dev) if return_logits else None
            for k0, n in sp.chunks():
                wp = sp.window_params(k0, n)
                _lib.check(lib.hsimae_scene_windows(C.byref(wp), sp.stream), "hsimae_scene_windows")
                st = sp.encode(n)
                logits, _ = self.head(st["latent"])
                st.release()
                _lib.check(lib.hsimae_class_argmax(C.byref(wp), logits.data_ptr(), logits.stride(0), self.num_class, 1,
                                                   labels.data_ptr(), sp.stream), "hsimae_class_argmax")
                if logits_all is not None:
                    logits_all[k0:k0 + n].copy_(logits)
            out, logits_all = to_host([labels.view(H, W), logits_all], on_device)
        return (out, logits_all) if return_logits else out

    def classify_scene(self, scene, pixels=None, batch_size=8192, views=(0,), return_probs=False, on_device=False):
        """predict_scene with what a classifier's user asks for next: the class probabilities behind every label, averaged over
        `views` of the pixel's window, and per pixel the winning probability and its margin over the runner-up.
        `views`: distinct flip codes 0 .. 3 (bit 0 flips the window along w, bit 1 along h: hsimae_scene_batch's, the flips
        fine-tuning draws); "flips" = (0, 1, 2, 3).  Per chunk and view, on the current stream: the flipped windows
        (hsimae_scene_batch), the unmasked encoder, the AGG head, and hsimae_class_prob: softmax over the real classes 1 ..
        num_class - 1 (class 0 is "unlabelled": probability 0), summed over the views in a chunk-local buffer; the last view
        writes mean, label = argmax of the mean (of the logits with one view: predict_scene's label bit for bit), confidence =
        mean[label] and margin = mean[label] - the largest other mean into device-resident maps.
        `scene`, `pixels`, `batch_size`, eval / no-grad behaviour: as predict_scene.  Pixels not asked for get label 0,
        confidence 0 and margin 0.
        -> SceneClassification(labels int64 [H, W], confidence fp32 [H, W], margin fp32 [H, W], probs fp32 [n, num_class] in pixel
        order with return_probs=True, else None), on the CPU after one wait for the copies; on_device=True: all stay on the
        model's device and nothing waits for the host."""
        views = scene_views(views)
        sp = self._scene_pass(scene, pixels, batch_size)
        lib, nc, H, W, dev = _lib.load(), self.num_class, sp.H, sp.W, sp.dev
        with torch.no_grad(), torch.cuda.device(dev):
            labels, conf, margin, probs = self._scene_maps(sp, return_probs)
            acc = torch.empty(sp.chunk, nc, dtype=torch.float32, device=dev)   # the views' sum of one chunk (view 0 overwrites it)
            flips = [torch.full((sp.chunk,), v, dtype=torch.uint8, device=dev) for v in views]
            for k0, n in sp.chunks():
                for vi, fl in enumerate(flips):
                    sp.cut(k0, n, fl)
                    st = sp.encode(n)
                    logits, _ = self.head(st["latent"])
                    st.release()
                    cp = _lib.ClassProbParams(logits=logits.data_ptr(), ld=logits.stride(0), N=n, C=nc, first=1, view=vi,
                                              n_views=len(views), acc=acc.data_ptr(), lda=nc, H=H, W=W,
                                              pixels=sp.items.data_ptr() + 8 * k0, label_map=labels.data_ptr(),
                                              conf_map=conf.data_ptr(), margin_map=margin.data_ptr(),
                                              probs=None if probs is None else probs.data_ptr() + 4 * nc * k0, ldp=nc)
                    _lib.check(lib.hsimae_class_prob(C.byref(cp), sp.stream), "hsimae_class_prob")
            out = to_host([labels.view(H, W), conf.view(H, W), margin.view(H, W), probs], on_device)
            if not on_device and int(sp.bad.item()):      # (the indices were checked on the host: this cannot happen)
                raise RuntimeError("classify_scene: a pixel index was outside the scene")
        return SceneClassification(*out)

    def _scene_maps(self, sp, want_probs):
        """The device-resident results classify_scene and knn_scene fill: labels, confidence and margin per pixel of the scene (0
        where not asked for), and with want_probs the [n, num_class] probabilities in pixel order."""
        n_px, dev = sp.H * sp.W, sp.dev
        return (torch.zeros(n_px, dtype=torch.int64, device=dev), torch.zeros(n_px, dtype=torch.float32, device=dev),
                torch.zeros(n_px, dtype=torch.float32, device=dev),
                torch.empty(sp.n_total, self.num_class, dtype=torch.float32, device=dev) if want_probs else None)

    # ------------------------------------------------------------------ features of a scene, and their k-NN evaluation
    def scene_features(self, scene, pixels=None, batch_size=8192, flip=0, on_device=True):
        """The pooled encoder features of a scene's pixels: what `head()` feeds the classification layer, fp32 [n, T * D], rows in
        pixel order (row-major over the scene, or the order of `pixels`).  Per chunk, on the current stream: the windows flipped
        by the constant code `flip` in 0 .. 3 (hsimae_scene_batch, classify_scene's path), the unmasked encoder, and
        hsimae_agg_pool written straight into the chunk's rows of the result.  The head GEMM is not run: a checkpoint from
        pretraining has no trained `cls_head`.  `scene`, `pixels`, `batch_size`, eval / no-grad behaviour: as predict_scene.
        on_device=True (the default): the result stays on the model's device and nothing waits for the host."""
        (flip,) = scene_views((flip,))
        sp = self._scene_pass(scene, pixels, batch_size)
        with torch.no_grad(), torch.cuda.device(sp.dev):
            feats = torch.empty(sp.n_total, sp.T * self.dim, dtype=torch.float32, device=sp.dev)
            flips = torch.full((sp.chunk,), flip, dtype=torch.uint8, device=sp.dev)
            for k0, n in sp.chunks():
                sp.cut(k0, n, flips)
                sp.pooled_into(feats[k0:k0 + n], n)
        return to_host([feats], on_device)[0]

    KNN_GROUP_ROWS = 32768

    def knn_scene(self, scene, bank_pixels, bank_labels, pixels=None, k=20, temperature=0.07, bank_flips=(0,), batch_size=8192,
                  return_probs=False, on_device=False):
        """classify_scene without a trained head: every pixel gets the weighted vote of the `k` labelled pixels whose pooled
        encoder features are most similar to its own (knn.KNNClassifier; cosine similarity, weights exp(sim / temperature), DINO's
        defaults).  The bank is `scene_features` of `bank_pixels` under each flip code of `bank_flips` ("flips" = all four),
        concatenated as rows, with `bank_labels` (one per bank pixel, in [1, num_class)) repeated per code.  Per chunk of query
        pixels: the features (as scene_features, flip 0, in the same chunks); per group of whole chunks (up to KNN_GROUP_ROWS
        rows): hsimae_row_normalize, hsimae_knn_topk, and hsimae_knn_vote into device-resident maps.  `scene`, `pixels`, `batch_size`, eval / no-grad behaviour: as predict_scene.
        -> SceneClassification like classify_scene's (probs fp32 [n, num_class] with return_probs=True), on the CPU after one
        wait for the copies; on_device=True: all stay on the model's device and nothing waits for the host after the bank's
        labels were checked.  The fitted classifier of the last call stays reachable as `self.last_knn` (its bank: `.bank`)."""
        from .knn import KNNClassifier
        bank_flips = scene_views(bank_flips)
        sp = self._scene_pass(scene, pixels, batch_size)   # its device scene is the one the bank's passes use too
        H, W, n_total, dev = sp.H, sp.W, sp.n_total, sp.dev
        with torch.no_grad(), torch.cuda.device(dev):
            y = torch.as_tensor(np.asarray(bank_labels) if not isinstance(bank_labels, torch.Tensor) else bank_labels)
            if y.dim() != 1 or y.dtype.is_floating_point or y.dtype == torch.bool:
                raise ValueError("bank_labels must be a 1-D array of integer labels")
            bank = [self.scene_features(sp.scene, bank_pixels, batch_size, flip=f, on_device=True) for f in bank_flips]
            if bank[0].shape[0] != y.numel():
                raise ValueError(f"{y.numel()} labels for {bank[0].shape[0]} bank pixels")
            knn = KNNClassifier(k=k, temperature=temperature, num_class=self.num_class, first=1)
            knn.fit(bank[0] if len(bank) == 1 else torch.cat(bank), y.to(dev).repeat(len(bank_flips)))
            del bank
            self.last_knn = knn                            # the fitted classifier of the last call (its bank: knn.bank)
            labels, conf, margin, probs = self._scene_maps(sp, return_probs)
            # the k-NN launches want more rows than one encoder chunk has (2,095 at Base: 33 workgroups of hsimae_knn_topk on 256
            # CUs): the features of whole chunks are collected up to KNN_GROUP_ROWS rows, then searched and voted on together
            group = max(1, self.KNN_GROUP_ROWS // sp.chunk) * sp.chunk
            feats = torch.empty(min(group, n_total), sp.T * self.dim, dtype=torch.float32, device=dev)
            flips = torch.zeros(sp.chunk, dtype=torch.uint8, device=dev)
            for g0 in range(0, n_total, group):
                gn = min(group, n_total - g0)
                for k0, n in sp.chunks(g0, g0 + gn):
                    sp.cut(k0, n, flips)
                    sp.pooled_into(feats[k0 - g0:k0 - g0 + n], n)
                knn.predict_into(feats[:gn], H, W, sp.items[g0:g0 + gn], labels, conf, margin, None if probs is None else probs[g0:g0 + gn])
            out = to_host([labels.view(H, W), conf.view(H, W), margin.view(H, W), probs], on_device)
            if not on_device:
                knn.check()
        return SceneClassification(*out)

    # ------------------------------------------------------------------ an RBF support-vector machine on features or spectra
    def svm_scene(self, scene, bank_pixels, bank_labels, pixels=None, features="encoder", C=1.0, gamma="scale", search=False,
                  bank_flips=(0,), batch_size=8192, return_probs=False, on_device=False):
        """knn_scene with an RBF-kernel support-vector machine in place of the vote (svm.RBFSVM: sklearn's SVC(kernel='rbf'),
        one-vs-one): the baseline hyperspectral papers report next to their deep models, and the non-linear counterpart of the
        linear probe.  features="encoder": the bank is built as knn_scene builds it (`scene_features` of `bank_pixels` under
        each flip code of `bank_flips`, `bank_labels` in [1, num_class) repeated per code) and the queries go through the
        encoder in knn_scene's chunks and groups of KNN_GROUP_ROWS rows.  features="spectra": cluster_scene's rows, the scene's
        own [H * W, C] as fp32 (C zero-padded to the next multiple of 4), with no encoder pass (`bank_flips` is ignored): the
        reference's Compared_Methods/svm_rbf.py on centre-pixel spectra.  `C`, `gamma`: RBFSVM's (gamma="scale" reads one
        number from the device).  search=True: RBFSVM.fit_reference, the reference's two-stage grid search (it draws its
        splits from numpy's global generator and refits on a training half; `C` and `gamma` are then ignored).  At most 8192
        bank rows and 32 classes.  The defaults are not tuned on a real scene.
        -> SceneClassification like classify_scene's; confidence, margin and probs are SHARES OF THE PAIRWISE VOTES, not Platt
        probabilities.  On the CPU after one wait for the copies; on_device=True: all stay on the model's device, and with
        features="spectra", a float `gamma` and search=False nothing waits for the host (the pixel lists are checked on the host
        and uploaded from pinned memory; the encoder path uploads its lists as knn_scene does).  The fitted
        model of the last call stays reachable as `self.last_svm`."""
        from .svm import RBFSVM
        if features not in ("encoder", "spectra"):
            raise ValueError(f'features must be "encoder" or "spectra", got {features!r}')
        bank_flips = scene_views(bank_flips) if features == "encoder" else (0,)
        y = torch.as_tensor(np.asarray(bank_labels) if not isinstance(bank_labels, torch.Tensor) else bank_labels)
        if y.dim() != 1 or y.dtype.is_floating_point or y.dtype == torch.bool:
            raise ValueError("bank_labels must be a 1-D array of integer labels")
        svm = RBFSVM(self.num_class, first=1, C=C, gamma=gamma)
        dev = gpu_of(self)

        def up(t):                                         # a host list to the device without a wait (pinned, asynchronous)
            return t if t.is_cuda else t.contiguous().pin_memory().to(dev, non_blocking=True)
        if features == "encoder":
            sp = self._scene_pass(scene, pixels, batch_size)
            H, W, n_total = sp.H, sp.W, sp.n_total
        else:
            s = as_scene(scene)
            H, W, Cb = (int(v) for v in s.shape)
            pix = None if pixels is None else pixel_indices(pixels, H * W)
            bank_pix = pixel_indices(bank_pixels, H * W, "bank_pixels", allow_empty=False)
            n_total = H * W if pix is None else pix.numel()
        with torch.no_grad(), torch.cuda.device(dev):
            if features == "encoder":
                bank = [self.scene_features(sp.scene, bank_pixels, batch_size, flip=f, on_device=True) for f in bank_flips]
                bank = bank[0] if len(bank) == 1 else torch.cat(bank)
            else:
                rows = (s if s.is_cuda else up(s)).reshape(H * W, Cb).to(torch.float32)
                if Cb % 4:
                    rows = torch.nn.functional.pad(rows, (0, 4 - Cb % 4))
                bank = rows[up(bank_pix)]
            if bank.shape[0] != y.numel() * len(bank_flips):
                raise ValueError(f"{y.numel()} labels for {bank.shape[0] // len(bank_flips)} bank pixels")
            yb = up(y).repeat(len(bank_flips))
            if search:
                svm.fit_reference(bank, yb)
            else:
                svm.fit(bank, yb)
            del bank
            self.last_svm = svm
            n_px = H * W
            labels = torch.zeros(n_px, dtype=torch.int64, device=dev)
            conf = torch.zeros(n_px, dtype=torch.float32, device=dev)
            margin = torch.zeros(n_px, dtype=torch.float32, device=dev)
            probs = torch.empty(n_total, self.num_class, dtype=torch.float32, device=dev) if return_probs else None
            if features == "spectra":
                pix_d = None if pix is None else up(pix)
                svm.predict_into(rows if pix is None else rows[pix_d], H, W, pix_d, labels, conf, margin, probs)
            else:
                group = max(1, self.KNN_GROUP_ROWS // sp.chunk) * sp.chunk
                feats = torch.empty(min(group, n_total), sp.T * self.dim, dtype=torch.float32, device=dev)
                flips = torch.zeros(sp.chunk, dtype=torch.uint8, device=dev)
                for g0 in range(0, n_total, group):
                    gn = min(group, n_total - g0)
                    for k0, n in sp.chunks(g0, g0 + gn):
                        sp.cut(k0, n, flips)
                        sp.pooled_into(feats[k0 - g0:k0 - g0 + n], n)
                    svm.predict_into(feats[:gn], H, W, sp.items[g0:g0 + gn], labels, conf, margin,
                                     None if probs is None else probs[g0:g0 + gn])
            out = to_host([labels.view(H, W), conf.view(H, W), margin.view(H, W), probs], on_device)
            if not on_device:
                svm.check()
        return SceneClassification(*out)

    # ------------------------------------------------------------------ a linear probe on the frozen encoder
    def probe_scene(self, scene, bank_pixels, bank_labels, pixels=None, bank_flips=(0,), views=(0,), batch_size=8192,
                    return_probs=False, on_device=False, **probe_kwargs):
        """classify_scene with a head trained here, on the frozen encoder: a linear probe (probe.LinearProbe: per-column
        standardised features, full-batch AdamW on the device) fitted on the pooled features of the labelled pixels.  The bank is
        built as knn_scene builds it: `scene_features` of `bank_pixels` under each flip code of `bank_flips` ("flips" = all four),
        concatenated as rows, `bank_labels` (one per bank pixel, in [1, num_class)) repeated per code.  The encoder runs once over
        the bank; no step of the fit touches it.  `probe_kwargs`: LinearProbe's (max_iter, lr, weight_decay, betas, eps,
        schedule, bn_eps).
        THIS OVERWRITES THE MODEL'S HEAD: the probe folded back to the raw features (LinearProbe.head) is copied into
        `cls_head.weight` / `.bias`, so every entry point that serves a trained head (classify_scene, predict_scene, the colour maps,
        state_dict) serves the probe from then on.  num_class <= 64.
        -> classify_scene(scene, pixels, views=views)'s SceneClassification with that head; `scene`, `pixels`, `batch_size`,
        `return_probs`, `on_device`: as classify_scene.  With on_device=True nothing waits for the host.  The fitted probe of the last
        call stays reachable as `self.last_probe` (`.loss_history`, `.grad_norm`, `.check()`)."""
        from .probe import LinearProbe
        bank_flips = scene_views(bank_flips)
        probe = LinearProbe(self.num_class, first=1, **probe_kwargs)
        s = scene_array(scene, self.patch_embed.bands, batch_size)[0]
        dev = gpu_of(self)
        with torch.no_grad(), torch.cuda.device(dev):
            s = s.to(dev).contiguous()                     # uploaded once: the bank's passes and the classification share it
            y = torch.as_tensor(np.asarray(bank_labels) if not isinstance(bank_labels, torch.Tensor) else bank_labels)
            if y.dim() != 1 or y.dtype.is_floating_point or y.dtype == torch.bool:
                raise ValueError("bank_labels must be a 1-D array of integer labels")
            bank = [self.scene_features(s, bank_pixels, batch_size, flip=f, on_device=True) for f in bank_flips]
            if bank[0].shape[0] != y.numel():
                raise ValueError(f"{y.numel()} labels for {bank[0].shape[0]} bank pixels")
            probe.fit(bank[0] if len(bank) == 1 else torch.cat(bank), y.to(dev).repeat(len(bank_flips)))
            del bank
            weight, bias = probe.head()
            self.cls_head.weight.copy_(weight)             # (in-place: the version counters move, so _packed_head repacks)
            self.cls_head.bias.copy_(bias)
            self.last_probe = probe
        out = self.classify_scene(s, pixels, batch_size=batch_size, views=views, return_probs=return_probs, on_device=on_device)
        if not on_device:
            probe.check()
        return out

    # ------------------------------------------------------------------ a land-cover map without labels
    def cluster_scene(self, scene, n_clusters, pixels=None, fit_pixels=None, features="encoder", metric=None, flip=0, max_iter=20,
                      n_init=1, generator=None, batch_size=8192, on_device=False, init="random"):
        """k-means (cluster.KMeans: hsimae_kmeans_assign / hsimae_kmeans_update) on the features of a scene's pixels: the
        segmentation a pretrained encoder gives without any label.
        features="encoder": `scene_features` (flip code `flip`), default metric "cosine"; features="spectra": the scene's own
        [H * W, C] rows as fp32 (C zero-padded to the next multiple of 4), default metric "euclidean": the classical baseline,
        with no encoder pass.  `fit_pixels` (pixel indices r * W + c, default: `pixels`) are the rows the centroids are fitted
        on; every one of `pixels` (default: all) is then labelled.  The features of the fitted pixels stay resident across the
        rounds (Base, 610 x 340 x 32 at T * D = 512 columns: 425 MB); with `fit_pixels` given (a grid, say), the other pixels are
        labelled chunk by chunk through KMeans.predict_into, so a large scene never holds all its features.
        `init`: "random" (KMeans': distinct fitted rows from torch.randperm on `generator`), a 1-D integer array of n_clusters
        pixel indices whose features seed the centroids, or a float tensor [n_clusters, D] of seed centroids in feature space.
        `max_iter`, `n_init`: KMeans'.  `scene`, `batch_size`, eval / no-grad behaviour: as predict_scene.
        -> SceneClustering(labels int64 [H, W] in 1 .. n_clusters, 0 where not asked; score fp32 [H, W]; margin fp32 [H, W] (best
        - second best score); centroids fp32 [n_clusters, D]; counts int64 [n_clusters] over the fitted pixels; inertia; n_iter),
        on the CPU after one wait for the copies; on_device=True: all stay on the model's device and, with n_init = 1, nothing
        waits for the host.  The fitted object of the last call stays reachable as `self.last_kmeans`."""
        from .cluster import KMeans, SceneClustering
        if features not in ("encoder", "spectra"):
            raise ValueError(f'features must be "encoder" or "spectra", got {features!r}')
        (flip,) = scene_views((flip,))
        metric = metric or ("cosine" if features == "encoder" else "euclidean")
        # the scene's own rows need no band count the encoder can take: it is not run
        s = scene_array(scene, self.patch_embed.bands, batch_size)[0] if features == "encoder" else as_scene(scene)
        H, W, Cb = (int(v) for v in s.shape)
        seeds = init if not isinstance(init, str) and torch.as_tensor(init).dim() == 1 else None     # pixels that seed the centroids
        pix, fit_pix, seed_pix = (None if p is None else pixel_indices(p, H * W, what, allow_empty=False)
                                  for p, what in ((pixels, "pixels"), (fit_pixels, "fit_pixels"), (seeds, "init")))
        n_total = H * W if pix is None else pix.numel()
        if seed_pix is not None and seed_pix.numel() != int(n_clusters):
            raise ValueError(f"init names {seed_pix.numel()} seed pixels for {n_clusters} clusters")
        dev = gpu_of(self)
        with torch.no_grad(), torch.cuda.device(dev):
            s = s.to(dev).contiguous()
            if features == "spectra":
                rows = s.reshape(H * W, Cb).to(torch.float32)
                if Cb % 4:
                    rows = torch.nn.functional.pad(rows, (0, 4 - Cb % 4))

                def feats(p):
                    return rows if p is None else rows[p.to(dev)]
            else:
                def feats(p):
                    return self.scene_features(s, p, batch_size, flip=flip, on_device=True)
            if seed_pix is not None:
                init = feats(seed_pix)
            elif not isinstance(init, str):
                init = torch.as_tensor(init).to(device=dev, dtype=torch.float32)
            km = KMeans(n_clusters, metric=metric, max_iter=max_iter, n_init=n_init, init=init, generator=generator, first=1)
            labels = torch.zeros(H * W, dtype=torch.int64, device=dev)
            score = torch.zeros(H * W, dtype=torch.float32, device=dev)
            margin = torch.zeros(H * W, dtype=torch.float32, device=dev)
            if fit_pix is None:                            # fit on the asked pixels: their features are held once
                f = feats(pix)
                km.fit(f)
                km.predict_into(f, H, W, None if pix is None else pix.to(dev), labels, score, margin)
                del f
            else:
                km.fit(feats(fit_pix))
                items = torch.arange(H * W, dtype=torch.int64) if pix is None else pix
                group = self.KNN_GROUP_ROWS
                for g0 in range(0, n_total, group):
                    part = items[g0:g0 + group]
                    km.predict_into(feats(part), H, W, part.to(dev), labels, score, margin)
            self.last_kmeans = km
            out = to_host([labels.view(H, W), score.view(H, W), margin.view(H, W), km.centroids, km.counts, km.inertia_, km.n_iter_],
                          on_device)
        return SceneClustering(*out)

    # ------------------------------------------------------------------ stochastic depth (Models.py:235-263, 687-731)
    def drop_rates(self):
        """DropPath probability of every encoder block in execution order (blocks_1, blocks_2, blocks)."""
        dpr = [x.item() for x in torch.linspace(0, self.drop_path, self.depth)]
        out = []
        if self.s_depth > 0:
            out += dpr[:self.s_depth] + dpr[:self.s_depth]
        if self.s_depth < 12:
            out += dpr[self.s_depth:self.depth]
        return out

    def draw_drop_factors(self, N, len_t, len_l, device):
        """Per-sequence factors (0 or 1/keep) of one encoder pass, drawn in the reference's order: attention then MLP of
        every block; a block with rate 0 holds nn.Identity and draws nothing (Models.py:298)."""
        s, nf = self.s_depth, (self.depth - self.s_depth if self.s_depth < 12 else 0)
        nseq = ([N * len_t] * s + [N * len_l] * s if s > 0 else []) + [N] * nf
        out = []
        for p, n in zip(self.drop_rates(), nseq):
            if p == 0.0:
                out.append((None, None))
                continue
            keep = 1 - p
            pair = []
            for _ in range(2):
                m = torch.empty(n, 1, 1, device=device).bernoulli_(keep)
                if keep > 0.0:
                    m.div_(keep)
                pair.append(m.reshape(-1))
            out.append(tuple(pair))
        return out

    def _row_scales(self, factors, N, len_t, len_l, device):
        """[n_blocks, 2, N*K] fp32 per-row factors for hsimae_io.drop_scale, rows in the kernels' (n, t, l) order:
        a spatial block's sequence is (n, t) ('b (t l) c -> (b t) l c'), a spectral block's (n, l), a fusion block's n."""
        if factors is None or all(a is None and b is None for a, b in factors):
            return None
        s = self.s_depth
        rows = torch.ones(len(factors), 2, N, len_t, len_l, dtype=torch.float32, device=device)
        for e, pair in enumerate(factors):
            for j, m in enumerate(pair):
                if m is None:
                    continue
                m = m.to(device=device, dtype=torch.float32)
                if s > 0 and e < s:
                    rows[e, j] = m.view(N, len_t, 1)
                elif s > 0 and e < 2 * s:
                    rows[e, j] = m.view(N, 1, len_l)
                else:
                    rows[e, j] = m.view(N, 1, 1)
        return rows.reshape(len(factors), 2, N * len_t * len_l).contiguous()

    # ------------------------------------------------------------------ training step
    def _train_forward(self, imgs, imgs_u, mask_ratio, noise, grid, drop_factors):
        dev = imgs.device
        T, L = self.input_size[0], self.input_size[1] ** 2
        N = imgs.shape[0]
        use_drop = self.training and self.drop_path > 0.0
        f_cls = f_rec = None
        if drop_factors is not None:
            f_cls, f_rec = drop_factors
        elif use_drop:
            f_cls = self.draw_drop_factors(N, T, L, dev)              # forward_encoder's draws come first (Models.py:976)
        n1 = torch.arange(T, dtype=torch.float32).expand(N, T)
        n2 = torch.arange(L, dtype=torch.float32).expand(N, L)
        _, _, _, st_cls = self._run_forward(imgs, 0.0, (n1, n2), (T, L), want_latent=True, encoder_only=True,
                                            drop_scale=self._row_scales(f_cls, N, T, L, dev))
        class_pred, pooled = self.head(st_cls["latent"])
        saved = {"cls": st_cls, "pooled": pooled, "N": N, "rec": None}
        out = {"class_pred": class_pred, "saved": saved}
        if imgs_u is not None:
            imgs_all = torch.concat([imgs, imgs_u], dim=0)
            Na = imgs_all.shape[0]
            # RNG order of forward_mask_encoder: grid (python random), noise_1, noise_2, then the blocks' DropPaths
            len_t, len_l = grid if grid is not None else self.get_dim_patches(T, L, mask_ratio)
            if noise is None:
                noise = (torch.rand(Na, T, device=dev), torch.rand(Na, L, device=dev))
            if drop_factors is None and use_drop:
                f_rec = self.draw_drop_factors(Na, int(len_t), int(len_l), dev)
            loss_rec, pred_rec, mask, st_rec = self._run_forward(
                imgs_all, mask_ratio, noise, (int(len_t), int(len_l)), want_latent=False,
                drop_scale=self._row_scales(f_rec, Na, int(len_t), int(len_l), dev))
            saved["rec"] = st_rec
            out.update(loss_rec=loss_rec, pred_rec=pred_rec, mask=mask)
        return out

    def _train_backward(self, saved, g_loss, g_cls):
        lib, cfg = _lib.load(), self._config()
        dev = self._flat.device
        gw = gb = None
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            scratch = self._flat_scratch
            scratch.zero_()                                   # weight grads are accumulated with atomics
            nocb = _lib.BUCKET_CB(0)
            det = self._det_buffer(dev)
            for st in (saved["rec"], saved["cls"]):
                if st is not None:
                    st["io"].det_acc = det
            if saved["rec"] is not None and g_loss is not None:
                saved["rec"].check_alive()
                saved["rec"]["_done"] = True
                _lib.check(lib.hsimae_backward(C.byref(cfg), C.byref(saved["rec"]["io"]), scratch.data_ptr(), nocb, None, stream),
                           "hsimae_backward")
                scratch.mul_(g_loss)                          # chain rule with d/d(loss_rec) (lamda in the reference's loop)
            if g_cls is not None:
                # head (Models.py:962-970): class_pred = pooled W^T + b, pooled[n, t*D + c] = mean_l latent[n, t, l, c]
                N, T, L, D = saved["N"], self.input_size[0], self.input_size[1] ** 2, self.dim
                g_cls = g_cls.to(torch.float32).contiguous()
                w = self.cls_head.weight.detach().contiguous()
                gw, gb = torch.empty_like(w), torch.empty(w.shape[0], dtype=torch.float32, device=dev)
                dlat = torch.empty(N, T, L, D, dtype=torch.float32, device=dev)
                _lib.check(lib.hsimae_head_bwd(g_cls.data_ptr(), saved["pooled"].data_ptr(), w.data_ptr(), gw.data_ptr(), gb.data_ptr(),
                                               dlat.data_ptr(), N, w.shape[0], T, L, D, stream), "hsimae_head_bwd")
                saved["cls"].check_alive()
                saved["cls"]["_done"] = True
                _lib.check(lib.hsimae_encode_backward(C.byref(cfg), C.byref(saved["cls"]["io"]), dlat.data_ptr(),
                                                      scratch.data_ptr(), nocb, None, stream), "hsimae_encode_backward")
        self._apply_grads(scratch, 1.0)
        for st in (saved["rec"], saved["cls"]):
            if st is not None:
                st.release()
        return gw, gb

    def forward(self, imgs, imgs_u=None, mask_ratio=0.75, noise=None, grid=None, drop_factors=None):
        """-> class_pred, or (loss_rec, pred_rec, mask, class_pred) with imgs_u (Models.py:975-991).
        `noise`, `grid` as in HSIMAE.forward; `drop_factors=(classification pass, reconstruction pass)`, each a list of
        (attn, mlp) per-sequence factor vectors per encoder block (None entries = no DropPath), replaces the draws."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            if imgs.is_cuda:
                self._ensure_flat(imgs.device)
            if self._reducer is not None:
                raise NotImplementedError("data-parallel fine-tuning is not built (pretraining only)")
            anchor = self._anchor if self._anchor is not None else torch.zeros((), requires_grad=True)
            return _FineTuneStep.apply(anchor, self.cls_head.weight, self.cls_head.bias, self, imgs, imgs_u, mask_ratio,
                                       noise, grid, drop_factors)
        with torch.no_grad():
            out = self._train_forward(imgs, imgs_u, mask_ratio, noise, grid, drop_factors)
        if imgs_u is None:
            return out["class_pred"]
        return out["loss_rec"], out["pred_rec"], out["mask"], out["class_pred"]


class HSIViT(DualViT):
    """The encoder-only classifier the reference evaluates fine-tuned checkpoints with (`Models.HSIViT`, Models.py:996-1167;
    `Model_Finetuning.test_model` :243-300): `forward(imgs) -> class logits`, 385-entry state_dict (encoder + `cls_head`),
    loaded key-filtered from a DualViT checkpoint.  Inference only.  The kernels' parameter layout always has a decoder, so a
    minimal one exists behind the scenes; it is not part of the module tree (state_dict / named_parameters do not list it).
    (Its random initialisation differs from the reference's stream: the class exists to load checkpoints.)"""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4.0,
                 norm_layer=nn.LayerNorm, bands=16, b_patch_size=4, num_class=100, no_qkv_bias=False, trunc_init=False,
                 drop_rate=0., drop_path=0., s_depth=6, **kwargs):
        super().__init__(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim, depth=depth,
                         s_depth=s_depth, num_heads=num_heads, mlp_ratio=mlp_ratio, norm_layer=norm_layer, bands=bands,
                         b_patch_size=b_patch_size, num_class=num_class, no_qkv_bias=no_qkv_bias, trunc_init=trunc_init,
                         drop_path=drop_path, decoder_embed_dim=32, decoder_depth=1, decoder_num_heads=4, norm_pix_loss=False)
        self._config()                                                  # cached while the decoder is still visible
        full = [p for n, p in self.named_parameters() if not n.startswith("cls_head.")]
        object.__setattr__(self, "_full_params", full)                  # flat-buffer order, decoder included
        hidden = {}
        for name in ("mask_token", "decoder_pos_embed"):
            hidden[name] = self._parameters.pop(name)
        for name in ("decoder_embed", "decoder_blocks", "decoder_norm", "decoder_pred"):
            hidden[name] = self._modules.pop(name)
        object.__setattr__(self, "_hidden_decoder", hidden)             # keeps them alive, outside the module tree

    def _plist(self):
        return self._full_params

    def _apply(self, fn, *a, **k):                                       # .to(device) must move the hidden decoder too
        out = super()._apply(fn, *a, **k)
        for v in self._hidden_decoder.values():
            if isinstance(v, nn.Module):
                v._apply(fn)
            else:
                v.data = fn(v.data)
        return out

    def forward(self, imgs):
        if self.training and torch.is_grad_enabled():
            raise NotImplementedError("hsimae_amd.HSIViT is the evaluation model (inference only); fine-tune with DualViT")
        with torch.no_grad():
            latent = self.forward_encoder(imgs)
            pred, _ = self.head(latent)
        return pred
