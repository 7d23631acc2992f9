"""csrc/kmeans.hip on the GPU: hsimae_kmeans_assign and hsimae_kmeans_update against the fp64 restatement and its derived bounds
and checks (tests/kmeans_ref.py), every call made twice and compared bit for bit; KMeans on Gaussian clusters; cluster_scene
against KMeans run by hand on scene_features; cluster_eval_scene's scores, pictures and checkpoints."""
import contextlib
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kmeans_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 8
FILL = -7


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def guarded(n, dtype, fill=FILL):
    """(whole buffer, the n elements in its middle): GUARD elements of `fill` on either side must survive a call."""
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def intact(whole, fill=FILL):
    w = whole.cpu()
    return bool((w[:GUARD] == fill).all() and (w[-GUARD:] == fill).all())


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ assign
def run_assign(x, c, bias, D, first, H, W, p0=0, pixels=None, score=True, margin=True, changed=True, prev=None):
    """x [N, ldx], c [K, ldc] device fp32 -> dict of (whole, inner): label (prefilled with `prev` or FILL), score, margin, changed."""
    from hsimae_amd import _lib
    N, K = x.shape[0], c.shape[0]
    out = {"label": guarded(H * W, torch.int64), "score": guarded(H * W, torch.float32) if score else None,
           "margin": guarded(H * W, torch.float32) if margin else None,
           "changed": guarded(_lib.KMEANS_GRID, torch.int32) if changed else None}
    if prev is not None:
        out["label"][1].copy_(prev)
    ptr = {key: (None if v is None else v[1].data_ptr()) for key, v in out.items()}
    p = _lib.KmeansAssignParams(x=x.data_ptr(), ldx=x.shape[1], c=c.data_ptr(), ldc=c.shape[1], bias=_lib.ptr(bias), N=N, K=K, D=D,
                                first=first, H=H, W=W, p0=p0, pixels=_lib.ptr(pixels), labels=ptr["label"], score=ptr["score"],
                                margin=ptr["margin"], changed=ptr["changed"])
    _lib.check(_lib.load().hsimae_kmeans_assign(C.byref(p), stream()), "hsimae_kmeans_assign")
    return out


def same_bits(a, b):
    return all((a[key] is None and b[key] is None) or torch.equal(bits(a[key][0]), bits(b[key][0])) for key in a)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "x".join(map(str, c)))
def test_assign_passes_every_check_on_every_row(case):
    N, K, D = case
    first = 1
    big = N > 10000
    for exact, with_bias in ((False, True), (True, True), (False, False), (True, False)):
        x, c, b = R.assign_case(N, K, D, D + 4, D + 8, exact=exact, bias=with_bias, spherical=not with_bias)
        s64, beta = R.scores_ref(x, c, b, D)
        xd, cd, bd = cuda(x), cuda(c), cuda(b)
        for name, H, W, p0, pixels in R.pixel_forms(N)[:1 if big and (exact or not with_bias) else 3]:
            pix, inside = R.rows_at(H, W, p0, pixels, N)
            prev = torch.randint(0, K + 2, (H * W,), device="cuda")
            out = run_assign(xd, cd, bd, D, first, H, W, p0, cuda(pixels), prev=prev)
            assert all(intact(out[key][0]) for key in out), (case, name)
            lm, sm, mm = (out[key][1].cpu().numpy() for key in ("label", "score", "margin"))
            written = np.zeros(H * W, bool)
            written[pix[inside]] = True
            pv = prev.cpu().numpy()
            assert np.array_equal(lm[~written], pv[~written]) and np.all(sm[~written] == FILL) and np.all(mm[~written] == FILL)
            rows = np.flatnonzero(inside)
            w = R.check_assign(lm[pix[rows]], sm[pix[rows]], mm[pix[rows]], s64[rows], beta[rows], first, exact=exact)
            print(f"{case} exact {exact} bias {with_bias} {name}: {w}")
            assert w["ok"] and w["b_worst"] <= 1.0 and w["c_worst"] <= 1.0, w
            ch = out["changed"][1].cpu().numpy()
            assert int(ch.sum()) == int((lm[pix[rows]] != pv[pix[rows]]).sum())          # the host's recount
            assert np.all(ch[(N + 63) // 64:] == 0)
            again = run_assign(xd, cd, bd, D, first, H, W, p0, cuda(pixels), prev=prev)
            assert same_bits(again, out), (case, name)                                   # bit for bit


def test_assign_optional_outputs_may_be_absent_in_every_combination():
    N, K, D = 130, 65, 36
    x, c, b = R.assign_case(N, K, D, D, D)
    xd, cd, bd = cuda(x), cuda(c), cuda(b)
    full = run_assign(xd, cd, bd, D, 3, 10, 13)
    for score in (False, True):
        for margin in (False, True):
            for changed in (False, True):
                out = run_assign(xd, cd, bd, D, 3, 10, 13, score=score, margin=margin, changed=changed)
                for key in out:
                    if out[key] is not None:
                        assert torch.equal(bits(out[key][0]), bits(full[key][0])), (key, score, margin, changed)
    assert int(full["label"][1].min()) >= 3 and int(full["label"][1].max()) < 3 + K


def test_assign_never_gives_a_row_to_a_nan_centroid_while_a_number_is_there():
    D = 36
    for K, row in ((130, 0), (130, 64), (130, 129), (2, 1), (65, 64)):
        x, c, b = R.assign_case(63, K, D, D, D, nan_row=row)
        out = run_assign(cuda(x), cuda(c), cuda(b), D, 1, 1, 63)
        lm, sm, mm = (out[key][1].cpu().numpy() for key in ("label", "score", "margin"))
        assert not (lm == 1 + row).any() and not np.isnan(sm).any() and (np.isnan(mm).any() == (K == 2)), (K, row)
        s64, beta = R.scores_ref(x, c, b, D)
        assert R.check_assign(lm, sm, mm, s64, beta, 1)["ok"]
    x, c, b = R.assign_case(5, 3, D, D, D)
    c[:] = np.nan                                                                        # nothing but NaN: the lowest index
    out = run_assign(cuda(x), cuda(c), cuda(b), D, 1, 1, 5)
    assert (out["label"][1] == 1).all() and torch.isnan(out["score"][1]).all()


def test_refusals_write_nothing():
    from hsimae_amd import _lib
    for what, got, want in R.refusals(_lib.load(), _lib):
        assert got == want, (what, got, want)
    x = torch.ones(8, 8, device="cuda")
    lw, lab = guarded(8, torch.int64)
    p = _lib.KmeansAssignParams(x=x.data_ptr(), ldx=8, c=x.data_ptr(), ldc=8, N=8, K=1025, D=8, first=1, H=1, W=8, labels=lab.data_ptr())
    assert _lib.load().hsimae_kmeans_assign(C.byref(p), stream()) == -2
    p.K, p.N = 8, 0
    assert _lib.load().hsimae_kmeans_assign(C.byref(p), stream()) == 0
    torch.cuda.synchronize()
    assert (lw == FILL).all()


# ------------------------------------------------------------------ update
def run_update(x, labels, c, bias, D, first, normalize, changed=None, state=None):
    """c [K, ldc] and bias [K] are updated in place (clones of the caller's) -> dict of tensors; counts / sums / state guarded."""
    from hsimae_amd import _lib
    N, K = x.shape[0], c.shape[0]
    c, bias = c.clone(), (None if bias is None else bias.clone())
    out = {"c": c, "bias": bias, "counts": guarded(K, torch.int64), "sums": guarded(K * D, torch.float64),
           "state": guarded(_lib.KMEANS_STATE, torch.float64), "scratch": guarded(K * ((D + 63) // 64) + 1, torch.float64)}
    out["state"][1].copy_(torch.zeros(_lib.KMEANS_STATE) if state is None else state)
    p = _lib.KmeansUpdateParams(x=x.data_ptr(), ldx=x.shape[1], labels=labels.data_ptr(), N=N, K=K, D=D, first=first,
                                normalize=int(normalize), c=c.data_ptr(), ldc=c.shape[1], bias=_lib.ptr(bias),
                                counts=out["counts"][1].data_ptr(), sums=out["sums"][1].data_ptr(), changed=_lib.ptr(changed),
                                scratch=out["scratch"][1].data_ptr(), state=out["state"][1].data_ptr())
    _lib.check(_lib.load().hsimae_kmeans_update(C.byref(p), stream()), "hsimae_kmeans_update")
    return out


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "x".join(map(str, c)))
def test_update_from_the_devices_own_labels(case):
    N, K, D = case
    first = 1
    for normalize in (False, True):
        x, c, b = R.assign_case(N, K, D, D + 4, D + 8, seed=1, bias=not normalize, spherical=normalize)
        xd, cd, bd = cuda(x), cuda(c), cuda(b)
        a = run_assign(xd, cd, bd, D, first, 1, N, score=False, margin=False)
        labels = a["label"][1].clone()
        lab = labels.cpu().numpy()
        empty_planted = None
        if K > 1 and N > 1:                                                              # plant an empty cluster, and bad labels
            empty_planted = int(lab[0] - first)
            other = first + (empty_planted + 1) % K
            lab = np.where(lab == first + empty_planted, other, lab)
            if N >= 5:
                lab[1], lab[N - 1] = first - 1, first + K
            labels = cuda(lab)
        ref = R.update_ref(x, lab, c, K, D, first, normalize)
        state0 = torch.tensor([9.0, 9.0, 3.0, 9.0, 9.0, 9.0, 9.0, 9.0], dtype=torch.float64)
        out = run_update(xd, labels, cd, bd, D, first, normalize, changed=a["changed"][1], state=state0)
        for key in ("counts", "sums", "state", "scratch"):
            assert intact(out[key][0]), key
        assert np.array_equal(out["counts"][1].cpu().numpy(), ref["counts"])             # exact
        sums = out["sums"][1].view(K, D).cpu().numpy()
        assert np.array_equal(sums.view(np.int64), ref["sums"].view(np.int64))           # the ascending chain, bit for bit
        got_c = out["c"].cpu().numpy()
        assert np.isnan(got_c[:, D:]).all()                                              # the pad was not touched
        wc = R.ratio(got_c[:, :D], ref["c"], ref["c_bound"])
        m = ref["member"]
        assert np.array_equal(got_c[~m, :D].view(np.int32), c[~m, :D].view(np.int32))    # an empty cluster keeps its bits
        wb = 0.0
        if not normalize:
            b64, bb = R.bias_ref(got_c, D)
            gb = out["bias"].cpu().numpy()
            wb = R.ratio(gb[m], b64[m], bb[m])
            assert np.array_equal(gb[~m].view(np.int32), b[~m].view(np.int32))
        else:
            norms = np.sqrt((got_c[m, :D].astype(np.float64) ** 2).sum(1))
            assert np.all(np.abs(norms - 1) <= 2 * 2.0 ** -23), float(np.abs(norms - 1).max())
        st = out["state"][1].cpu().numpy()
        rel = abs(st[0] - ref["inertia"]) / max(ref["inertia"], 1e-300)
        print(f"{case} normalize {normalize}: err / bound c {wc:.3f} bias {wb:.3f}; inertia rel {rel:.3g}; empty {ref['empty']} bad {ref['bad']}")
        assert wc <= 1.0 and wb <= 1.0 and rel <= 1e-12
        changed = int(a["changed"][1].sum())
        assert st[1] == changed and st[2] == 3 + (changed > 0) and st[3] == ref["empty"] and st[4] == ref["bad"] and np.all(st[5:] == 0)
        if empty_planted is not None:
            assert not m[empty_planted] and ref["empty"] >= 1
        if N >= 5 and K > 1:
            assert ref["bad"] == 2
        again = run_update(xd, labels, cd, bd, D, first, normalize, changed=a["changed"][1], state=state0)
        for key in ("counts", "sums", "state"):
            assert torch.equal(bits(again[key][0]), bits(out[key][0])), key
        assert torch.equal(bits(again["c"]), bits(out["c"])) and (bd is None or torch.equal(bits(again["bias"]), bits(out["bias"])))
        nochange = run_update(xd, labels, cd, bd, D, first, normalize, changed=None, state=state0)
        assert float(nochange["state"][1][1]) == 0 and float(nochange["state"][1][2]) == 3


def test_update_adds_the_member_rows_in_ascending_order():
    """Rows of very different magnitude: the fp64 sums round, and only the ascending chain gives these bits."""
    N, K, D = 300, 3, 68
    x, c, b = R.assign_case(N, K, D, D, D, seed=3)
    x = R.wide_rows(x)
    lab = 1 + np.random.RandomState(1).randint(0, K, N).astype(np.int64)
    out = run_update(cuda(x), cuda(lab), cuda(c), cuda(b), D, 1, False)
    sums = out["sums"][1].view(K, D).cpu().numpy()
    up, down = (R.emulate_update(x, lab, c, b, K, D, 1, False, fault=f)[2] for f in (None, "descending"))
    assert not np.array_equal(up.view(np.int64), down.view(np.int64))
    assert np.array_equal(sums.view(np.int64), up.view(np.int64))
    ref = R.update_ref(x, lab, c, K, D, 1, False)
    assert R.ratio(out["c"].cpu().numpy(), ref["c"], ref["c_bound"]) <= 1.0


# ------------------------------------------------------------------ KMeans
def test_kmeans_recovers_the_planted_clusters_and_is_idempotent_at_the_fixed_point():
    from hsimae_amd import KMeans
    bank, by, qs, qy = R.clusters()                          # 7 classes, D = 32, N = 1000
    seeds = R.class_seeds(bank, by, 7)
    qd, sd = cuda(qs), cuda(seeds)
    for metric in ("euclidean", "cosine"):
        ref = R.fit_ref(qs, seeds, metric, 20)
        assert ref["n_iter"] == 2 and np.array_equal(ref["labels"], qy)
        runs = {}
        for it in (5, 20):
            km = KMeans(7, metric=metric, max_iter=it, init=sd).fit(qd)
            assert all(t.is_cuda for t in (km.centroids, km.counts, km.labels_, km.inertia_, km.n_iter_, km.empty_))
            assert km.labels_.dtype == torch.int64 and km.inertia_.dtype == torch.float64 and km.inertia_.dim() == 0
            assert np.array_equal(km.labels_.cpu().numpy(), qy)
            assert int(km.n_iter_) == 2 and int(km.empty_) == 0
            rel = abs(float(km.inertia_) - ref["inertia"]) / ref["inertia"]
            print(f"{metric} max_iter {it}: inertia {float(km.inertia_):.6f} (fp64 {ref['inertia']:.6f}, rel {rel:.3g})")
            assert rel <= 1e-6
            assert np.array_equal(km.counts.cpu().numpy(), np.bincount(qy - 1, minlength=7))
            runs[it] = km
        assert torch.equal(bits(runs[5].centroids), bits(runs[20].centroids)) and torch.equal(runs[5].labels_, runs[20].labels_)
        assert torch.equal(bits(runs[5].inertia_.view(1)), bits(runs[20].inertia_.view(1)))
        km = runs[20]
        labels, score, margin = km.predict(qd)
        assert torch.equal(labels, km.labels_) and float(margin.min()) > 0 and torch.equal(km.fit_predict(qd), labels)
        lab = torch.zeros(1000, dtype=torch.int64, device="cuda")
        perm = torch.randperm(1000, generator=torch.Generator().manual_seed(3)).cuda()
        km.predict_into(qd, 20, 50, perm, lab)
        assert torch.equal(lab[perm], labels)


def test_kmeans_random_seeding_is_reproducible_and_restarts_never_lose():
    from hsimae_amd import KMeans
    _, _, qs, _ = R.clusters()
    qd = cuda(qs)
    for metric in ("euclidean", "cosine"):
        a = KMeans(7, metric=metric, generator=torch.Generator().manual_seed(11)).fit(qd)
        b = KMeans(7, metric=metric, generator=torch.Generator().manual_seed(11)).fit(qd)
        assert torch.equal(bits(a.centroids), bits(b.centroids)) and torch.equal(a.labels_, b.labels_)
        g = torch.Generator().manual_seed(5)
        singles = [float(KMeans(7, metric=metric, generator=g).fit(qd).inertia_) for _ in range(3)]
        best = KMeans(7, metric=metric, n_init=3, generator=torch.Generator().manual_seed(5)).fit(qd)
        print(f"{metric}: single runs {singles}, n_init=3 {float(best.inertia_)}")
        assert all(float(best.inertia_) <= s for s in singles) and float(best.inertia_) == min(singles)
        assert int(best.labels_.min()) >= 1 and int(best.labels_.max()) <= 7


# ------------------------------------------------------------------ cluster_scene, cluster_eval_scene
def tiny_hsivit(num_class=7, seed=0):
    """tests/test_gpu_knn.py's tiny model, built here: same shape, same seeds."""
    from hsimae_amd import HSIViT
    torch.manual_seed(seed)
    m = quiet(HSIViT, img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, num_class=num_class, embed_dim=32, depth=3,
              num_heads=2, s_depth=2, trunc_init=True)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            elif "norm" in n and n.endswith("weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
    return m.cuda().eval()


def scene_23x19(seed=5, dtype=np.float64):
    return np.random.default_rng(seed).standard_normal((23, 19, 32)).astype(dtype)


def test_cluster_scene_is_kmeans_on_scene_features():
    from hsimae_amd import KMeans, SceneClustering
    m = tiny_hsivit(seed=2)
    scene = scene_23x19(seed=6)
    K, bs = 5, 256
    res = m.cluster_scene(scene, K, generator=torch.Generator().manual_seed(7), batch_size=bs, max_iter=10)
    assert isinstance(res, SceneClustering) and not res.labels.is_cuda and tuple(res.labels.shape) == (23, 19)
    f = m.scene_features(scene, batch_size=bs)
    km = KMeans(K, metric="cosine", max_iter=10, generator=torch.Generator().manual_seed(7)).fit(f)
    labels, score, margin = km.predict(f)
    assert torch.equal(res.labels.reshape(-1), labels.cpu()) and torch.equal(bits(res.score.reshape(-1)), bits(score.cpu()))
    assert torch.equal(bits(res.margin.reshape(-1)), bits(margin.cpu())) and torch.equal(bits(res.centroids), bits(km.centroids.cpu()))
    assert torch.equal(res.counts, km.counts.cpu()) and float(res.inertia) == float(km.inertia_) and int(res.n_iter) == int(km.n_iter_)
    assert torch.equal(bits(m.last_kmeans.centroids), bits(km.centroids)) and int(res.labels.min()) >= 1 and int(res.labels.max()) <= K
    # fitted on a grid, a subset labelled, the rest 0
    rng = np.random.default_rng(3)
    grid = np.arange(0, 437, 3)
    sub = rng.permutation(437)[:300]
    part = m.cluster_scene(scene, K, pixels=sub, fit_pixels=grid, generator=torch.Generator().manual_seed(7), batch_size=bs, max_iter=10)
    km2 = KMeans(K, metric="cosine", max_iter=10, generator=torch.Generator().manual_seed(7)).fit(m.scene_features(scene, grid, bs))
    want = km2.predict(m.scene_features(scene, sub, bs))[0].cpu()
    asked = np.zeros(437, bool)
    asked[sub] = True
    got = part.labels.reshape(-1)
    assert torch.equal(got[torch.from_numpy(sub)], want) and (got[~asked] == 0).all() and (part.score.reshape(-1)[~asked] == 0).all()
    assert int(part.counts.sum()) == len(grid)
    # the spectra themselves
    spec = m.cluster_scene(scene, K, features="spectra", generator=torch.Generator().manual_seed(9), max_iter=10)
    rows = torch.from_numpy(scene).cuda().reshape(437, 32).float()
    km3 = KMeans(K, metric="euclidean", max_iter=10, generator=torch.Generator().manual_seed(9)).fit(rows)
    assert torch.equal(spec.labels.reshape(-1), km3.labels_.cpu()) and torch.equal(bits(spec.centroids), bits(km3.centroids.cpu()))
    odd = m.cluster_scene(scene[:, :, :30], 3, features="spectra", generator=torch.Generator().manual_seed(9), max_iter=5)   # 30 -> 32
    assert tuple(odd.centroids.shape) == (3, 32) and (odd.centroids[:, 30:] == 0).all() and int(odd.labels.min()) >= 1
    dev = m.cluster_scene(torch.from_numpy(scene).cuda(), K, generator=torch.Generator().manual_seed(7), batch_size=bs, max_iter=10,
                          on_device=True)
    assert all(t.is_cuda for t in dev) and torch.equal(dev.labels.cpu(), res.labels)
    for bad in (dict(features="pca"), dict(metric="manhattan"), dict(flip=4)):
        with pytest.raises(ValueError):
            m.cluster_scene(scene, K, **bad)


def planted_scene(seed=21):
    """A 23 x 19 label map of 4 blocks (a border of 0 = unlabelled) and spectra = class mean + small noise."""
    rng = np.random.default_rng(seed)
    gt = np.zeros((23, 19), np.int64)
    truth = np.zeros((23, 19), np.int64)
    truth[:12, :10], truth[:12, 10:], truth[12:, :10], truth[12:, 10:] = 3, 1, 4, 2
    gt[1:-1, 1:-1] = truth[1:-1, 1:-1]
    means = 2.0 * rng.standard_normal((5, 32))
    scene = means[truth] + 0.05 * rng.standard_normal((23, 19, 32))
    return scene, gt, truth


def test_cluster_eval_scene_scores_a_planted_scene_after_matching(tmp_path):
    from hsimae_amd import cluster_eval_scene, label_to_colormap
    import prob_ref
    scene, gt, truth = planted_scene()
    seeds = np.array([int(np.flatnonzero(truth.reshape(-1) == k)[5]) for k in (2, 4, 1, 3)])     # cluster ids: a permutation
    out = quiet(cluster_eval_scene, scene, gt, None, features="spectra", init=seeds, max_iter=5, depth=3, dim=32, s_depth=2, save_dir=str(tmp_path),
                model_name="spectra.pkl", save_images=True)
    oa, aa, kappa, ca, nmi, ari, purity, mapped, raw = out
    assert np.array_equal(mapped, truth) and not np.array_equal(raw, truth)
    assert np.array_equal(raw, np.array([0, 3, 1, 4, 2])[truth])
    assert oa == 1.0 and aa == 1.0 and kappa == 1.0 and np.all(ca == 1.0)
    assert abs(nmi - 1) <= 1e-12 and abs(ari - 1) <= 1e-12 and purity == 1.0
    whole = prob_ref.decode_png(open(os.path.join(tmp_path, "spectra", "spectra_all_oa_100.0.png"), "rb").read())
    assert np.array_equal(whole, label_to_colormap(mapped))
    masked = prob_ref.decode_png(open(os.path.join(tmp_path, "spectra", "spectra_oa_100.0.png"), "rb").read())
    assert np.array_equal(masked, label_to_colormap(np.where(gt == 0, 0, mapped)))
    big = gt.copy()
    big[2, 2] = 25                                                                       # outside the palette: before clustering
    with pytest.raises(ValueError, match="palette"):
        cluster_eval_scene(scene, big, None, features="spectra", depth=3, dim=32, s_depth=2, save_dir=str(tmp_path), save_images=True)
    with pytest.raises(ValueError):
        cluster_eval_scene(scene, gt, None)                                              # the encoder needs a checkpoint


def test_cluster_eval_scene_loads_both_kinds_of_checkpoint_and_scores_its_mapped_map(tmp_path):
    from hsimae_amd import HSIMAE, DualViT, cluster_eval_scene
    from hsimae_amd.finetune_train import scores
    kw = dict(img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, embed_dim=32, depth=3, num_heads=2, s_depth=2,
              trunc_init=True, decoder_embed_dim=32, decoder_depth=1, decoder_num_heads=4, norm_pix_loss=True)
    torch.manual_seed(4)
    d = quiet(DualViT, num_class=6, **kw)
    torch.manual_seed(5)
    mae = quiet(HSIMAE, **kw)
    torch.save(d.state_dict(), os.path.join(tmp_path, "ft.pkl"))
    torch.save(mae.state_dict(), os.path.join(tmp_path, "mae.pkl"))
    rng = np.random.default_rng(13)
    scene = scene_23x19(seed=14)
    gt = rng.integers(0, 6, size=(23, 19))
    gt.reshape(-1)[:6] = np.arange(6)
    raws = {}
    for name in ("ft.pkl", "mae.pkl"):
        for K in (None, 8):                                                              # as many clusters as classes; more
            out = quiet(cluster_eval_scene, scene, gt, os.path.join(tmp_path, name), n_clusters=K, depth=3, dim=32, s_depth=2,
                        batch_size=256, max_iter=8, generator=torch.Generator().manual_seed(1))
            oa, aa, kappa, ca, nmi, ari, purity, mapped, raw = out
            assert mapped.shape == gt.shape and raw.min() >= 1 and raw.max() <= (K or 5) and mapped.min() >= 1 and mapped.max() <= 5
            want = scores(gt.reshape(-1), mapped.reshape(-1))
            assert abs(oa - want[0]) <= 1e-12 and abs(aa - want[1]) <= 1e-12 and abs(kappa - want[2]) <= 1e-12
            assert np.allclose(ca, want[3], rtol=0, atol=1e-12)
            assert 0 <= nmi <= 1 and -1 <= ari <= 1 and oa <= purity <= 1
            lut = {}
            for r, mp in zip(raw.reshape(-1), mapped.reshape(-1)):                       # the mapped map is a relabelling of the raw one
                assert lut.setdefault(int(r), int(mp)) == int(mp)
            if K is None:
                assert len(set(lut.values())) == len(lut)                                # one to one
                raws[name] = raw
    assert not np.array_equal(raws["ft.pkl"], raws["mae.pkl"])                           # two encoders, two maps
