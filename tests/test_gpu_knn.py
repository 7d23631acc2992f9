"""csrc/knn.hip on the GPU: hsimae_row_normalize, hsimae_knn_topk and hsimae_knn_vote against the fp64 restatement and its
derived bounds and checks (tests/knn_ref.py); KNNClassifier on Gaussian clusters under the predict rule; DualViT.scene_features
against head(forward_encoder(windows)); knn_scene against the three calls composed by hand; knn_eval_scene's scores, pictures
and checkpoints."""
import contextlib
import ctypes as C
import io
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_ref as R  # noqa: E402

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
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ normalise
def run_norm(x, D, ldo=None, norms=True, in_place=False):
    """x device fp32 [N, ld] -> (out whole, out [N, ldo], norms whole, norms [N] or None)."""
    from hsimae_amd import _lib
    N, ld = x.shape
    ldo = ld if in_place else (ldo or D + 1)
    ow, o = (None, x.view(-1)) if in_place else guarded(N * ldo, torch.float32)
    nw, n = guarded(N, torch.float32) if norms else (None, None)
    p = _lib.RowNormalizeParams(x=x.data_ptr(), ld=ld, N=N, D=D, out=o.data_ptr(), ldo=ldo, norms=_lib.ptr(n))
    _lib.check(_lib.load().hsimae_row_normalize(C.byref(p), stream()), "hsimae_row_normalize")
    return ow, o.view(N, ldo), nw, n


@pytest.mark.parametrize("D", [1, 4, 63, 64, 65, 1536])
def test_row_normalize_lies_inside_the_bound_of_the_restatement(D):
    for N in (1, 5, 257):
        x = R.normalize_case(N, D, D + 3)
        ref, bound, n64, nb = R.normalize_ref(x, D)
        xd = torch.from_numpy(x).cuda()
        ow, o, nw, n = run_norm(xd, D)
        got = o.cpu().numpy()
        w, wn = R.ratio(got[:, :D], ref, bound), R.ratio(n.cpu().numpy(), n64, nb)
        print(f"N {N} D {D}: err / bound: out {w:.3f}, norms {wn:.3f}")
        assert w <= 1.0 and wn <= 1.0
        assert intact(ow) and intact(nw) and np.all(got[:, D:] == FILL)
        if N >= 5:
            assert np.all(got[0, :D] == 0) and n64[1] < 1e-12 and np.isfinite(got[2, :D]).all()
        ow2, o2, _, none = run_norm(xd, D, norms=False)
        assert none is None and torch.equal(bits(ow2), bits(ow))                         # bit-identical, norms absent
        inp = xd.clone()
        run_norm(inp, D, in_place=True)
        assert torch.equal(bits(inp[:, :D]), bits(o[:, :D])) and torch.isnan(inp[:, D:]).all()      # the pad was not touched


# ------------------------------------------------------------------ top-k
def run_topk(q, b, D, k):
    """q [Q, ldq], b [M, ldb] device fp32 -> (idx whole, idx [Q, k], sim whole, sim [Q, k])."""
    from hsimae_amd import _lib
    Q, M = q.shape[0], b.shape[0]
    iw, i = guarded(Q * k, torch.int32)
    sw, s = guarded(Q * k, torch.float32)
    p = _lib.KnnTopkParams(q=q.data_ptr(), ldq=q.shape[1], bank=b.data_ptr(), ldb=b.shape[1], Q=Q, M=M, D=D, k=k,
                           idx=i.data_ptr(), sim=s.data_ptr())
    _lib.check(_lib.load().hsimae_knn_topk(C.byref(p), stream()), "hsimae_knn_topk")
    return iw, i.view(Q, k), sw, s.view(Q, k)


PAST_THE_GRID = 2048 * 64 + 1                              # one query tile more than the grid holds workgroups
TOPK_CASES = [(1, 1, 4, 1), (1, 2, 8, 1), (63, 63, 36, 2), (63, 64, 8, 20), (65, 65, 36, 64), (65, 64, 512, 64), (65, 21, 4, 20),
              (130, 20, 8, 20), (130, 257, 512, 20), (130, 1000, 1536, 64), (5, 1000, 36, 1), (63, 3, 1536, 2),
              (PAST_THE_GRID, 65, 4, 2)]


@pytest.mark.parametrize("case", TOPK_CASES, ids=lambda c: "x".join(map(str, c)))
def test_topk_passes_every_check_on_every_row(case):
    Q, M, D, k = case
    for exact in (False, True):
        q, b = R.topk_case(Q, M, D, D + 4, D + 8, exact=exact)
        qd, bd = torch.from_numpy(q).cuda(), torch.from_numpy(b).cuda()
        iw, idx, sw, sim = run_topk(qd, bd, D, k)
        w = R.check_topk(idx.cpu().numpy(), sim.cpu().numpy(), q, b, D, k, exact=exact)
        print(f"{case} exact {exact}: {w}")
        assert w["ok"] and w["b_worst"] <= 1.0, w
        assert intact(iw) and intact(sw)
        iw2, _, sw2, _ = run_topk(qd, bd, D, k)
        assert torch.equal(iw2, iw) and torch.equal(bits(sw2), bits(sw))


def test_topk_returns_a_nan_row_only_when_the_numbers_run_out():
    D, k = 36, 20
    for M, row in ((257, 0), (257, 100), (257, 256), (65, 64), (21, 7)):
        q, b = R.topk_case(63, M, D, D, D, nan_row=row)
        _, idx, _, sim = run_topk(torch.from_numpy(q).cuda(), torch.from_numpy(b).cuda(), D, k)
        idx, sim = idx.cpu().numpy(), sim.cpu().numpy()
        assert not (idx == row).any() and not np.isnan(sim).any(), (M, row)
        assert R.check_topk(idx, sim, q, b, D, k)["ok"]
    q, b = R.topk_case(63, k, D, D, D, nan_row=5)                                       # M = k: the NaN row comes last
    _, idx, _, sim = run_topk(torch.from_numpy(q).cuda(), torch.from_numpy(b).cuda(), D, k)
    idx, sim = idx.cpu().numpy(), sim.cpu().numpy()
    assert np.all(idx[:, -1] == 5) and np.isnan(sim[:, -1]).all() and not np.isnan(sim[:, :-1]).any()
    assert R.check_topk(idx, sim, q, b, D, k)["ok"]


# ------------------------------------------------------------------ vote
def run_vote(idx, sim, labels, Cc, first, T, H, W, p0=0, pixels=None, ldp=None, conf=True, margin=True, probs=True):
    """-> dict of (whole, inner) buffers: label, conf, margin, probs (or None), and `bad` (int32 [1])."""
    from hsimae_amd import _lib
    Q, k = idx.shape
    ldp = ldp or Cc + 5
    out = {"label": guarded(H * W, torch.int64), "conf": guarded(H * W, torch.float32) if conf else None,
           "margin": guarded(H * W, torch.float32) if margin else None, "probs": guarded(Q * ldp, torch.float32) if probs else None}
    ptr = {key: (None if v is None else v[1].data_ptr()) for key, v in out.items()}
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = _lib.KnnVoteParams(idx=idx.data_ptr(), sim=sim.data_ptr(), Q=Q, k=k, M=labels.shape[0], bank_labels=labels.data_ptr(), C=Cc,
                           first=first, inv_temperature=1.0 / T, H=H, W=W, p0=p0, pixels=_lib.ptr(pixels), label_map=ptr["label"],
                           conf_map=ptr["conf"], margin_map=ptr["margin"], probs=ptr["probs"], ldp=ldp, bad=bad.data_ptr())
    _lib.check(_lib.load().hsimae_knn_vote(C.byref(p), stream()), "hsimae_knn_vote")
    out["ldp"], out["bad"] = ldp, bad
    return out


def vote_in_row_order(out, row_of, ref, Q, Cc):
    """The maps read back per row -> (p, label, conf, margin); a row whose pixel lies outside the map takes the restatement's
    values.  Also checks that nothing else in the maps was written and that the guards survived."""
    for key in ("label", "conf", "margin", "probs"):
        assert out[key] is None or intact(out[key][0]), key
    pr = out["probs"][1].view(Q, out["ldp"]).cpu().numpy()
    assert np.all(pr[:, Cc:] == FILL)
    label, conf, margin = ref["label"].copy(), ref["conf"].copy(), ref["margin"].copy()
    lm, cm, mm = (out[key][1].cpu().numpy() for key in ("label", "conf", "margin"))
    assert np.all(lm[row_of < 0] == FILL) and np.all(cm[row_of < 0] == FILL) and np.all(mm[row_of < 0] == FILL)
    pix = np.flatnonzero(row_of >= 0)
    assert np.all(lm[pix] != FILL)
    label[row_of[pix]], conf[row_of[pix]], margin[row_of[pix]] = lm[pix], cm[pix], mm[pix]
    return pr[:, :Cc], label, conf, margin


@pytest.mark.parametrize("shape", R.VOTE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_vote_lies_inside_the_bound_of_the_restatement(shape):
    Q, Cc, ld = shape
    forms = R.pixel_forms(Q)
    for first, k, T in itertools.product((0, 1), R.KS, R.TEMPS):
        idx, sim, labels = R.vote_case(Q, Cc, first, k, T)
        ref = R.vote_ref(idx, sim, labels, Cc, first, R.inv_t32(T))
        dev = [torch.from_numpy(a).cuda() for a in (idx, sim, labels)]
        for name, H, W, p0, pixels in forms:
            pix_d = None if pixels is None else torch.from_numpy(pixels).cuda()
            out = run_vote(*dev, Cc, first, T, H, W, p0, pix_d, ldp=ld)
            got = vote_in_row_order(out, R.rows_of_pixels(H, W, p0, pixels, Q), ref, Q, Cc)
            w = R.vote_worst(got, ref, first)
            print(f"{shape} first {first} k {k} T {T} {name}: err / bound: p {w['p']:.3f}, conf {w['conf']:.3f}, "
                  f"margin {w['margin']:.3f}; labels wrong {w['wrong']}, share left open {w['open']:.5f}")
            assert w["zeros"] and w["wrong"] == 0 and w["p"] <= 1.0 and w["conf"] <= 1.0 and w["margin"] <= 1.0
            assert w["open"] <= 0.01 and int(out["bad"].item()) == 0
        again = run_vote(*dev, Cc, first, T, H, W, p0, pix_d, ldp=ld)
        for key in ("label", "conf", "margin", "probs"):                                 # bit for bit
            assert torch.equal(bits(again[key][0]), bits(out[key][0])), key


def test_vote_planted_ties_go_to_the_lower_class():
    for idx, sim, labels, Cc, first, want in R.tie_cases():
        out = run_vote(*[torch.from_numpy(a).cuda() for a in (idx, sim, labels)], Cc, first, 0.07, 1, 1)
        assert int(out["label"][1].item()) == want and float(out["conf"][1].item()) == 0.5 and float(out["margin"][1].item()) == 0.0


def test_vote_optional_outputs_may_be_absent_in_every_combination():
    Q, Cc, first, k, T = 65, 33, 1, 20, 0.07
    dev = [torch.from_numpy(a).cuda() for a in R.vote_case(Q, Cc, first, k, T)]
    full = run_vote(*dev, Cc, first, T, 5, 15, 3)
    for conf, margin, probs in itertools.product((False, True), repeat=3):
        out = run_vote(*dev, Cc, first, T, 5, 15, 3, conf=conf, margin=margin, probs=probs)
        for key in ("label", "conf", "margin", "probs"):
            if out[key] is not None:
                assert torch.equal(out[key][0], full[key][0]), (key, conf, margin, probs)


def test_vote_flags_a_bad_bank_label_and_zeroes_its_row():
    Q, Cc, first, k, T = 65, 9, 1, 20, 0.07
    idx, sim, labels = R.vote_case(Q, Cc, first, k, T, M=300)
    labels[idx[7, 3]] = 0                                   # below first
    labels[idx[11, 0]] = Cc                                 # past the classes
    idx[20, 5] = 300                                        # a neighbour outside the bank
    ref = R.vote_ref(idx, sim, labels, Cc, first, R.inv_t32(T))
    assert ref["bad"][[7, 11, 20]].all()
    out = run_vote(*[torch.from_numpy(a).cuda() for a in (idx, sim, labels)], Cc, first, T, 1, Q)
    got = vote_in_row_order(out, np.arange(Q), ref, Q, Cc)
    w = R.vote_worst(got, ref, first)
    assert int(out["bad"].item()) == 1 and w["all"] <= 1.0, w
    rows = np.flatnonzero(ref["bad"])
    assert np.all(got[1][rows] == 0) and np.all(got[2][rows] == 0) and np.all(got[3][rows] == 0) and np.all(got[0][rows] == 0)


def test_refusals_write_nothing():
    from hsimae_amd import _lib
    for what, got, want in R.refusals(_lib.load(), _lib):
        assert got == want, (what, got, want)
    iw, i = guarded(64, torch.int32)
    sw, s = guarded(64, torch.float32)
    x = torch.ones(8, 8, device="cuda")
    p = _lib.KnnTopkParams(q=x.data_ptr(), ldq=8, bank=x.data_ptr(), ldb=8, Q=8, M=8, D=8, k=9, idx=i.data_ptr(), sim=s.data_ptr())
    assert _lib.load().hsimae_knn_topk(C.byref(p), stream()) == -1                      # k > M
    p.k, p.Q = 8, 0
    assert _lib.load().hsimae_knn_topk(C.byref(p), stream()) == 0                       # nothing to do
    torch.cuda.synchronize()
    assert (iw == FILL).all() and (sw == FILL).all()


# ------------------------------------------------------------------ the classifier
def test_classifier_on_gaussian_clusters_under_the_predict_rule():
    from hsimae_amd import KNNClassifier
    bank, by, qs, qy = R.clusters()                          # 7 classes, D = 32, M = 140, Q = 1000
    k, T = 20, 0.07
    knn = KNNClassifier(k=k, temperature=T).fit(torch.from_numpy(bank).cuda(), torch.from_numpy(by))
    assert knn.num_class == 8 and knn.bank.is_cuda and knn.labels.is_cuda
    qd = torch.from_numpy(qs).cuda()
    labels, conf, margin, probs = knn.predict(qd, return_probs=True)
    assert all(t.is_cuda for t in (labels, conf, margin, probs))
    qn = run_norm(qd, 32, ldo=32)[1]
    ref = R.predict_ref(qn.cpu().numpy(), knn.bank.cpu().numpy(), by, k, 8, 1, R.inv_t32(T))
    idx, sim = knn.neighbours(qd)
    assert R.check_topk(idx.cpu().numpy(), sim.cpu().numpy(), qn.cpu().numpy(), knn.bank.cpu().numpy(), 32, k)["ok"]
    lab = labels.cpu().numpy()
    share = float((~ref["decided"]).sum()) / len(lab)
    acc = float((lab == qy).mean())
    rows = ref["decided"]                                    # there the neighbour set is determined: the bounds must hold
    w = R.vote_worst((probs.cpu().numpy()[rows], lab[rows], conf.cpu().numpy()[rows], margin.cpu().numpy()[rows]),
                     {key: v[rows] for key, v in ref.items()}, 1)
    print(f"share left open {share:.4f}, accuracy {acc:.3f}, err / bound p {w['p']:.3f} conf {w['conf']:.3f} margin {w['margin']:.3f}")
    assert np.array_equal(lab[ref["decided"]], ref["label"][ref["decided"]]) and share <= 0.02
    assert np.array_equal(np.sort(idx.cpu().numpy()[rows], 1), np.sort(ref["idx"][rows], 1))
    assert w["wrong"] == 0 and w["p"] <= 1.0 and w["conf"] <= 1.0 and w["margin"] <= 1.0
    assert probs.cpu().numpy()[:, 0].max() == 0 and np.allclose(probs.cpu().numpy().sum(1), 1, atol=1e-5)
    three = knn.predict(qd)
    assert len(three) == 3 and torch.equal(three[0], labels) and torch.equal(bits(three[1]), bits(conf))
    knn.check()
    with pytest.raises(ValueError):
        KNNClassifier(k=20).fit(torch.from_numpy(bank).cuda(), torch.from_numpy(by - 1))          # label 0 is below first
    with pytest.raises(ValueError):
        KNNClassifier(k=20, num_class=7).fit(torch.from_numpy(bank).cuda(), torch.from_numpy(by))   # label 7 is past num_class


# ------------------------------------------------------------------ scene_features, knn_scene, knn_eval_scene
def tiny_hsivit(num_class=7, seed=0):
    """tests/test_gpu_prob.py's tiny model, built here: same shape, same seeds."""
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


def pooled_of_windows(m, scene, pix, flip, bs):
    """head(forward_encoder(SceneCubes.gather(...)))[1] in chunks of `bs` -> fp32 [n, T * D] (device)."""
    from hsimae_amd import SceneCubes
    cubes = SceneCubes(scene)
    rows = [m.head(m.forward_encoder(cubes.gather(pix[k0:k0 + bs], np.full(len(pix[k0:k0 + bs]), flip, np.uint8))))[1]
            for k0 in range(0, len(pix), bs)]
    cubes.check()
    return torch.cat(rows)


def test_scene_features_are_the_pooled_features_of_the_windows():
    m = tiny_hsivit()
    scene = scene_23x19()
    pix = np.arange(23 * 19)
    want = pooled_of_windows(m, scene, pix, 0, 256)
    f = m.scene_features(scene, batch_size=256)
    assert f.is_cuda and f.dtype == torch.float32 and tuple(f.shape) == (437, 4 * 32)
    assert torch.equal(bits(f), bits(want))                                              # the same chunk shape: bit for bit
    host = m.scene_features(scene, batch_size=256, on_device=False)
    assert not host.is_cuda and torch.equal(host, f.cpu())
    other = m.scene_features(scene, batch_size=100).double()
    rms = float(((other - want.double()) ** 2).mean().sqrt() / (want.double() ** 2).mean().sqrt())
    print(f"chunks of 100 against chunks of 256: RMS-relative {rms:.3g}")
    assert rms <= 1e-3
    for flip in (1, 2, 3):
        g = m.scene_features(scene, batch_size=256, flip=flip)
        assert torch.equal(bits(g), bits(pooled_of_windows(m, scene, pix, flip, 256))) and not torch.equal(g, f)
    sub = np.array([436, 0, 18, 19, 200, 5, 418])
    assert torch.equal(bits(m.scene_features(scene, pixels=sub, batch_size=256)), bits(pooled_of_windows(m, scene, sub, 0, 256)))
    for bad in (4, -1, 1.0, True):
        with pytest.raises(ValueError):
            m.scene_features(scene, flip=bad)
    was = m.training
    m.train()
    assert torch.equal(bits(m.scene_features(scene, batch_size=256)), bits(f)) and m.training       # eval behaviour, mode untouched
    m.train(was)


def test_scene_features_of_an_fp32_scene_smaller_than_the_pad():
    m = tiny_hsivit(seed=4)
    scene = np.random.default_rng(9).standard_normal((3, 5, 32)).astype(np.float32)
    for flip in (0, 3):
        f = m.scene_features(scene, flip=flip)
        assert torch.equal(bits(f), bits(pooled_of_windows(m, scene, np.arange(15), flip, 15)))


def test_knn_scene_is_the_three_calls_on_scene_features():
    from hsimae_amd.finetune import SceneClassification
    m = tiny_hsivit(seed=2)
    scene = scene_23x19(seed=6)
    rng = np.random.default_rng(3)
    bank_pix = rng.choice(437, 60, replace=False)
    bank_y = rng.integers(1, 7, 60)
    bank_y[:6] = np.arange(1, 7)
    sub = rng.permutation(437)[:300]
    k, T, bs = 5, 0.07, 256
    res = m.knn_scene(scene, bank_pix, bank_y, pixels=sub, k=k, temperature=T, batch_size=bs, return_probs=True)
    assert isinstance(res, SceneClassification) and not res.labels.is_cuda and tuple(res.labels.shape) == (23, 19)
    # by hand: the features, then the three C-ABI calls
    fb, fq = m.scene_features(scene, bank_pix, bs), m.scene_features(scene, sub, bs)
    bn, qn = run_norm(fb, 128, ldo=128)[1], run_norm(fq, 128, ldo=128)[1]
    assert torch.equal(bits(m.last_knn.bank), bits(bn))
    _, idx, _, sim = run_topk(qn, bn, 128, k)
    out = run_vote(idx, sim, torch.from_numpy(bank_y).cuda(), 7, 1, T, 23, 19, 0, torch.from_numpy(sub).cuda(), ldp=7)
    lm, cm, mm = (out[key][1].cpu() for key in ("label", "conf", "margin"))
    asked = np.zeros(437, bool)
    asked[sub] = True
    for got, want in ((res.labels, lm), (res.confidence, cm), (res.margin, mm)):
        got = got.reshape(-1)
        assert torch.equal(got[asked], want[asked]) and (got[~asked] == 0).all() and (want[~asked] == FILL).all()
    assert torch.equal(res.probs, out["probs"][1].view(300, 7).cpu())
    assert res.labels.reshape(-1)[asked].min() >= 1 and int(out["bad"].item()) == 0
    # everything on the device, all pixels, no probabilities
    dev = m.knn_scene(torch.from_numpy(scene).cuda(), bank_pix, bank_y, k=k, temperature=T, batch_size=bs, on_device=True)
    assert dev.probs is None and all(t.is_cuda for t in dev[:3]) and int(dev.labels.min()) >= 1 and float(dev.confidence.min()) > 0
    # the four flip views of the bank
    m.knn_scene(scene, bank_pix, bank_y, pixels=sub[:10], k=k, bank_flips="flips", batch_size=bs)
    four = m.last_knn
    assert tuple(four.bank.shape) == (240, 128) and torch.equal(bits(four.bank[:60]), bits(bn))
    assert not torch.equal(four.bank[60:120], bn) and torch.equal(four.labels.cpu(), torch.from_numpy(bank_y).repeat(4))
    with pytest.raises(ValueError):
        m.knn_scene(scene, bank_pix, bank_y[:-1], k=k)
    with pytest.raises(ValueError):
        m.knn_scene(scene, bank_pix, bank_y, k=k, bank_flips="all")


def test_knn_eval_scene_scores_its_own_map_and_loads_both_kinds_of_checkpoint(tmp_path):
    from hsimae_amd import HSIMAE, DualViT, HSIViT, knn_eval_scene, label_to_colormap
    from hsimae_amd.finetune_train import scores
    import prob_ref
    kw = dict(img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, embed_dim=32, depth=3, num_heads=2, s_depth=2,
              trunc_init=True, decoder_embed_dim=32, decoder_depth=1, decoder_num_heads=4, norm_pix_loss=True)
    torch.manual_seed(4)
    d = quiet(DualViT, num_class=6, **kw)
    torch.manual_seed(5)
    mae = quiet(HSIMAE, **kw)
    torch.save(d.state_dict(), os.path.join(tmp_path, "ft.pkl"))
    torch.save(mae.state_dict(), os.path.join(tmp_path, "mae.pkl"))
    assert "cls_head.weight" not in mae.state_dict() and "cls_head.weight" in d.state_dict()
    rng = np.random.default_rng(13)
    scene = scene_23x19(seed=14)
    gt = rng.integers(0, 6, size=(23, 19))
    gt.reshape(-1)[:6] = np.arange(6)
    flat = gt.reshape(-1)
    train_index = np.flatnonzero((flat != 0) & (rng.random(437) < 0.3))
    train_labels = flat[train_index]
    test_gt = gt.copy()
    test_gt.reshape(-1)[train_index] = 0
    args = dict(depth=3, dim=32, s_depth=2, k=5, batch_size=256)
    maps, out_of = {}, {}
    for name in ("ft.pkl", "mae.pkl"):
        out = quiet(knn_eval_scene, scene, train_index, train_labels, test_gt, gt, os.path.join(tmp_path, name), save_dir=str(tmp_path),
                    save_images=True, **args)
        oa, aa, kappa, ca, pred = out
        assert pred.shape == gt.shape and pred.dtype == np.int64 and pred.min() >= 1 and pred.max() <= 5
        want = scores(test_gt.reshape(-1), np.where(gt == 0, 0, pred).reshape(-1))
        assert abs(oa - want[0]) <= 1e-12 and abs(aa - want[1]) <= 1e-12 and abs(kappa - want[2]) <= 1e-12
        assert np.allclose(ca, want[3], rtol=0, atol=1e-12)
        stem = name.replace(".pkl", "")
        tag = str(np.around(oa * 100, 2))
        assert sorted(os.listdir(os.path.join(tmp_path, stem))) == sorted([f"{stem}_all_oa_{tag}.png", f"{stem}_oa_{tag}.png"])
        whole = prob_ref.decode_png(open(os.path.join(tmp_path, stem, f"{stem}_all_oa_{tag}.png"), "rb").read())
        assert np.array_equal(whole, label_to_colormap(pred))
        maps[name], out_of[name] = pred, out
    assert not np.array_equal(maps["ft.pkl"], maps["mae.pkl"])                           # two encoders, two maps
    # the fine-tuned checkpoint: the map of an HSIViT loaded the same way
    v = quiet(HSIViT, img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, num_class=6, embed_dim=32, depth=3,
              num_heads=2, s_depth=2, sep_pos_embed=True, use_learnable_pos_emb=False).cuda()
    sd = v.state_dict()
    sd.update({key: t for key, t in torch.load(os.path.join(tmp_path, "ft.pkl"), map_location="cuda").items() if key in sd})
    v.load_state_dict(sd)
    v.eval()
    assert np.array_equal(v.knn_scene(scene, train_index, train_labels, k=5, batch_size=256).labels.numpy(), maps["ft.pkl"])
    plain = quiet(knn_eval_scene, scene, train_index, train_labels, test_gt, gt, os.path.join(tmp_path, "ft.pkl"), **args)
    assert np.array_equal(plain[4], maps["ft.pkl"]) and plain[:3] == out_of["ft.pkl"][:3] and sorted(os.listdir(tmp_path / "ft")) != []
