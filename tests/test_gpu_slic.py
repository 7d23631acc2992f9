"""csrc/slic.hip on the GPU: hsimae_slic and hsimae_segment_vote against the fp64 restatement and its derived bounds
(tests/slic_ref.py) over the whole case list through the C ABI with guarded buffers, twice bit for bit; the optional outputs; the
refusals; rounds = r against r calls; the planted scene; and the Python layer: Superpixels.fit, segment_classification and the
`smooth=` argument of the three evaluation entry points.

Every step is checked from the device's own inputs to that step (the centres a round started from, the labels the device itself
chose), so a pixel the bounds leave open cannot cascade into the next check.

Measured on MI355X over CASES and VOTE_CASES: worst err / bound 0.972 (the winning distance, 130 x 130 at size 2, the assign after
one round; 0.853 at the start, 33 x 70 at size 32); every new centre and every segment vector equals the restatement bit for bit
(err / bound 0); no label wrong; largest share left open 0 outside the exact-input cases (there 11.1 % of the pixels tie exactly and
the labels equal the first argmin)."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import slic_ref as R  # noqa: E402
import smooth_ref  # noqa: E402
from test_gpu_smooth import quiet, same, scene_23x19, tiny_dualvit  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 8
FILL = -7                                                  # what the outputs hold before a call


def guarded(n, dtype, fill=FILL):
    """(whole buffer, the n elements in its middle): GUARD elements of `fill` on either side must survive a call."""
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def guards_intact(out):
    for k, v in out.items():
        if v is not None:
            whole = v[0].cpu()
            assert (whole[:GUARD] == FILL).all() and (whole[-GUARD:] == FILL).all(), k


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    for k in a:
        if a[k] is not None:
            assert torch.equal(bits(a[k][0]), bits(b[k][0])), k


def run_slic(c, dev, w, init, rounds, start=None, counts=True, dist=True, tmp=True):
    """One call on the current stream -> dict of (whole, inner) buffers: centres, tmp, counts, labels, dist (or None)."""
    from hsimae_amd import _lib
    H, W, S, G = c[:4]
    ny, nx = R.grid(H, W, S)
    K = ny * nx
    out = {"centres": guarded(K * 8, torch.float32), "tmp": guarded(K * 8, torch.float32) if tmp else None,
           "counts": guarded(K, torch.int32) if counts else None, "labels": guarded(H * W, torch.int32),
           "dist": guarded(H * W, torch.float32) if dist else None}
    if start is not None:
        out["centres"][1].copy_(torch.from_numpy(start).reshape(-1))
    ptr = {k: (None if v is None else v[1].data_ptr()) for k, v in out.items()}
    p = _lib.SlicParams(guide=dev["guide"].data_ptr(), guide_scale=dev["scale"].data_ptr(), G=G, H=H, W=W, size=S, w=w, init=init,
                        rounds=rounds, centres=ptr["centres"], centres_tmp=ptr["tmp"], counts=ptr["counts"], labels=ptr["labels"],
                        dist=ptr["dist"])
    _lib.check(_lib.load().hsimae_slic(C.byref(p), torch.cuda.current_stream().cuda_stream), "hsimae_slic")
    return out


def host(out, key, shape):
    return out[key][1].cpu().numpy().reshape(shape)


def upload(case):
    return {"guide": torch.from_numpy(case["guide"]).cuda(), "scale": torch.from_numpy(case["scale"]).cuda()}


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_slic_lies_inside_the_bounds_of_the_restatement(c):
    H, W, S, G, variant = c
    case = R.make_case(*c)
    guide, scale, w, start = case["guide"], case["scale"], case["w"], case["start"]
    K = start.shape[0]
    dev = upload(case)
    # the grid centres
    placed = run_slic(c, dev, w, 1, 0, tmp=False)
    guards_intact(placed)
    assert np.array_equal(host(placed, "centres", (K, 8)).view(np.int32), R.init_centres(guide, scale, S).view(np.int32))
    # one assign from the start
    first = run_slic(c, dev, w, 0, 0, start, tmp=False)
    guards_intact(first)
    assert np.array_equal(host(first, "centres", (K, 8)).view(np.int32), start.view(np.int32))          # no round: no centre moves
    lab = host(first, "labels", (H, W))
    a = R.check_assign(guide, scale, start, w, S, lab, host(first, "dist", (H, W)), host(first, "counts", K), exact=case["exact"])
    # one round from the start: the new centres are the means over the labels the device itself chose, then the next assign
    nxt = run_slic(c, dev, w, 0, 1, start)
    guards_intact(nxt)
    new = host(nxt, "centres", (K, 8))
    u = R.check_update(guide, scale, lab, start, new)
    b = R.check_assign(guide, scale, new, w, S, host(nxt, "labels", (H, W)), host(nxt, "dist", (H, W)), host(nxt, "counts", K))
    print(f"{R.case_id(c)}: start: dist err / bound {a['dist']:.3f}, wrong {a['wrong']}, open {a['open']:.5f}; update err / bound "
          f"{u['ratio']:.3f} (bit-equal {u['bits']}, {u['empty']} empty); next: dist {b['dist']:.3f}, wrong {b['wrong']}, open {b['open']:.5f}")
    assert a["wrong"] == 0 and a["counts"] and a["first"] and a["dist"] <= 1.0
    assert u["kept"] and u["ratio"] <= 1.0
    assert b["wrong"] == 0 and b["counts"] and b["dist"] <= 1.0
    if case["exact"]:
        assert u["bits"]                                   # exact inputs: labels equal the first argmin (a["first"]), centres bit for bit
    else:
        assert a["open"] <= 0.02 and b["open"] <= 0.02
    if variant == "empty":
        assert u["empty"] >= 1
    same_bits(first, run_slic(c, dev, w, 0, 0, start, tmp=False))
    same_bits(nxt, run_slic(c, dev, w, 0, 1, start))


def test_optional_outputs_of_slic_may_be_absent_in_every_combination():
    c = (17, 33, 4, 4, "")
    case = R.make_case(*c)
    dev = upload(case)
    full = run_slic(c, dev, case["w"], 1, 2)
    for counts, dist in itertools.product((False, True), repeat=2):
        out = run_slic(c, dev, case["w"], 1, 2, counts=counts, dist=dist)
        guards_intact(out)
        same_bits(out, full)


@pytest.mark.parametrize("c,r", [((23, 19, 3, 3, ""), 3), ((130, 130, 2, 1, ""), 2), ((48, 40, 8, 1, "planted"), 4)], ids=["23x19-S3-r3", "130x130-S2-r2", "planted-r4"])
def test_a_fit_of_r_rounds_equals_r_calls_of_one_round(c, r):
    H, W, S, G, _ = c
    case = R.make_case(*c)
    dev = upload(case)
    whole = run_slic(c, dev, case["w"], 1, r)
    step = run_slic(c, dev, case["w"], 1, 0)
    for _ in range(r):
        K = case["start"].shape[0]
        step = run_slic(c, dev, case["w"], 0, 1, host(step, "centres", (K, 8)))
    for k in ("centres", "counts", "labels", "dist"):
        assert torch.equal(bits(whole[k][1]), bits(step[k][1])), k
    assert int(whole["counts"][1].sum()) == H * W


def test_every_refusal_returns_its_code_and_writes_nothing():
    from hsimae_amd import _lib
    lib = _lib.load()
    for what, got, want in R.refusals(lib, _lib):
        assert got == want, (what, got, want)
    c = (9, 17, 8, 1, "")
    case = R.make_case(*c)
    dev = upload(case)
    stream = torch.cuda.current_stream().cuda_stream
    out = {k: guarded(256, torch.int32 if k in ("counts", "labels") else torch.float32) for k in ("centres", "tmp", "counts", "labels", "dist")}
    p = _lib.SlicParams(guide=dev["guide"].data_ptr(), guide_scale=dev["scale"].data_ptr(), G=1, H=9, W=17, size=33, w=case["w"], init=1,
                        rounds=1, centres=out["centres"][1].data_ptr(), centres_tmp=out["tmp"][1].data_ptr(),
                        counts=out["counts"][1].data_ptr(), labels=out["labels"][1].data_ptr(), dist=out["dist"][1].data_ptr())
    assert lib.hsimae_slic(C.byref(p), stream) == -1                                                 # size 33
    p.size, p.centres_tmp = 8, out["centres"][1].data_ptr()
    assert lib.hsimae_slic(C.byref(p), stream) == -1                                                 # the two buffers are one
    p.centres_tmp = None
    assert lib.hsimae_slic(C.byref(p), stream) == -4                                                 # a round needs the second buffer
    vout = {k: guarded(256, {"label": torch.int64, "count": torch.int32}.get(k, torch.float32)) for k in ("label", "conf", "margin", "probs", "count")}
    probs = torch.rand(153, 8, device="cuda")
    seg = torch.zeros(153, dtype=torch.int32, device="cuda")
    v = _lib.SegmentVoteParams(probs=probs.data_ptr(), ldp=8, n=153, C=8, first=1, labels=seg.data_ptr(), H=9, W=17, size=8, mode=2, fill=0,
                               out_probs=vout["probs"][1].data_ptr(), ldo=8, seg_count=vout["count"][1].data_ptr(),
                               label_map=vout["label"][1].data_ptr(), conf_map=vout["conf"][1].data_ptr(), margin_map=vout["margin"][1].data_ptr())
    assert lib.hsimae_segment_vote(C.byref(v), stream) == -1                                         # mode 2
    v.mode, v.out_probs = 0, probs.data_ptr()
    assert lib.hsimae_segment_vote(C.byref(v), stream) == -1                                         # in place
    torch.cuda.synchronize()
    for k, (whole, _) in list(out.items()) + list(vout.items()):
        assert (whole == FILL).all(), k


# ------------------------------------------------------------------ the vote
def run_vote(c, case, dev, out_probs=True, seg_count=True, conf=True, margin=True):
    from hsimae_amd import _lib
    H, W, S, Cc, first, form, mode, fill = c
    K = int(np.prod(R.grid(H, W, S)))
    out = {"label": guarded(H * W, torch.int64), "conf": guarded(H * W, torch.float32) if conf else None,
           "margin": guarded(H * W, torch.float32) if margin else None, "probs": guarded(K * case["ldo"], torch.float32) if out_probs else None,
           "count": guarded(K, torch.int32) if seg_count else None}
    ptr = {k: (None if v is None else v[1].data_ptr()) for k, v in out.items()}
    p = _lib.SegmentVoteParams(probs=dev["probs"].data_ptr(), ldp=case["ldp"], n=case["n"], C=Cc, first=first, row_of=_lib.ptr(dev["row_of"]),
                               labels=dev["label"].data_ptr(), H=H, W=W, size=S, mode=mode, fill=fill, out_probs=ptr["probs"],
                               ldo=case["ldo"], seg_count=ptr["count"], label_map=ptr["label"], conf_map=ptr["conf"], margin_map=ptr["margin"])
    _lib.check(_lib.load().hsimae_segment_vote(C.byref(p), torch.cuda.current_stream().cuda_stream), "hsimae_segment_vote")
    return out


def upload_vote(case):
    return {k: (None if case[k] is None else torch.from_numpy(np.ascontiguousarray(case[k])).cuda()) for k in ("probs", "row_of", "label")}


@pytest.mark.parametrize("c", R.VOTE_CASES, ids=R.vote_id)
def test_segment_vote_lies_inside_the_bounds_of_the_restatement(c):
    H, W, S, Cc, first, form, mode, fill = c
    case = R.make_vote_case(*c)
    ref = R.vote_ref(case["probs"], case["n"], Cc, first, case["row_of"], case["label"], S, mode, fill)
    dev = upload_vote(case)
    out = run_vote(c, case, dev)
    guards_intact(out)
    K = ref["cnt"].size
    vec = host(out, "probs", (K, case["ldo"]))
    got = R.check_vote(ref, first, Cc, vec, host(out, "count", K), host(out, "label", H * W), host(out, "conf", H * W),
                       host(out, "margin", H * W), FILL)
    bit_equal = np.array_equal(vec[ref["live"]][:, first:Cc].view(np.int32), ref["vec"][ref["live"]][:, first:].view(np.int32))
    print(f"{R.vote_id(c)}: vector err / bound {got['vec']:.3f} (bit-equal {bit_equal}); {int(ref['live'].sum())} of {K} segments live, "
          f"{int(ref['written'].sum())} of {H * W} pixels written")
    assert got["count"] and got["self"] and got["untouched"] and got["zeros"] and got["vec"] <= 1.0
    same_bits(out, run_vote(c, case, dev))


def test_optional_outputs_of_the_vote_may_be_absent_in_every_combination():
    c = (23, 19, 3, 18, 1, "subset", 0, 1)
    case = R.make_vote_case(*c)
    dev = upload_vote(case)
    full = run_vote(c, case, dev)
    for flags in itertools.product((False, True), repeat=4):
        out = run_vote(c, case, dev, *flags)
        guards_intact(out)
        same_bits(out, full)


# ------------------------------------------------------------------ the Python layer
def planted_on_device(seed=0):
    s = smooth_ref.planted_scene(seed)
    return s, torch.from_numpy(s["probs"]).cuda(), (torch.from_numpy(s["guide"]).cuda(), torch.from_numpy(s["scale"]).cuda())


def test_the_planted_scene_is_repaired_on_the_device_and_fit_never_waits():
    from hsimae_amd import Superpixels, segment_classification
    from hsimae_amd.finetune import SceneClassification
    s, probs, guide = planted_on_device()
    H, W = s["H"], s["W"]
    raw = 1 + probs[:, 1:].argmax(1)
    assert R.oa(raw.cpu().numpy(), s["truth"]) < 0.8
    res = SceneClassification(raw.view(H, W), torch.zeros(H, W, device="cuda"), torch.zeros(H, W, device="cuda"), probs)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        segs = Superpixels(8, 0.1, 10).fit(guide, H, W)
        mean = segment_classification(res, segs, mode="mean", on_device=True)
        vote = segment_classification(res, segs, mode="vote", return_probs=True, on_device=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert segs.check() is segs and segs.grid == (6, 5) and tuple(segs.centres.shape) == (30, 3) and int(segs.counts.min()) > 0
    assert segs.labels.dtype == torch.int32 and R.purity(segs.labels.cpu().numpy(), s["truth"]) == 1.0
    assert R.oa(mean.labels.cpu().numpy(), s["truth"]) == 1.0 and R.oa(vote.labels.cpu().numpy(), s["truth"]) == 1.0
    want, _, cnt = R.fit_ref(s["guide"], s["scale"], 8, 0.1, 10)
    print(f"planted scene on the device: OA raw {R.oa(raw.cpu().numpy(), s['truth']):.4f}, mean 1.0, vote 1.0; labels equal the "
          f"restatement's: {np.array_equal(want, segs.labels.cpu().numpy())}")
    # return_probs: the segment vector of each input row
    seg = segs.labels.reshape(-1).cpu().numpy()
    pv = vote.probs.cpu().numpy()
    assert pv.shape == (H * W, 6) and all((pv[seg == k] == pv[seg == k][0]).all() for k in range(30))
    assert torch.equal(vote.confidence.reshape(-1), vote.probs.gather(1, vote.labels.reshape(-1, 1)).reshape(-1))


def test_segment_classification_is_the_lib_call_by_hand_and_leaves_its_input_alone():
    from hsimae_amd import _lib, scene_segments, segment_classification
    m = tiny_dualvit().cuda().eval()
    scene = torch.from_numpy(scene_23x19()).cuda()
    H, W = 23, 19
    segs = scene_segments(scene, size=4, compactness=0.2, max_iter=3, channels=2).check()
    assert segs.grid == (6, 5) and tuple(segs.centres.shape) == (30, 4)
    for pix, mode, fill in ((None, "mean", False), (torch.tensor([436, 0, 18, 19, 200, 5, 418, 201, 219, 181]), "vote", True),
                            (torch.arange(0, H * W, 2), "mean", True)):
        res = m.classify_scene(scene, pixels=pix, batch_size=256, return_probs=True, on_device=True)
        before = [None if t is None else t.clone() for t in res]
        got = segment_classification(res, segs, pixels=pix, mode=mode, fill=fill, return_probs=True, on_device=True)
        assert all(t.is_cuda for t in got) and same(res, before)                   # the input result is not modified
        n = res.probs.shape[0]
        row_of = None
        if pix is not None:
            row_of = torch.full((H * W,), -1, dtype=torch.int32, device="cuda")
            row_of[pix.cuda()] = torch.arange(n, dtype=torch.int32, device="cuda")
        lab, conf, margin = torch.zeros(H * W, dtype=torch.int64, device="cuda"), torch.zeros(H * W, device="cuda"), torch.zeros(H * W, device="cuda")
        vec = torch.zeros(30, 6, device="cuda")
        p = _lib.SegmentVoteParams(probs=res.probs.data_ptr(), ldp=6, n=n, C=6, first=1, row_of=_lib.ptr(row_of), labels=segs.labels.data_ptr(),
                                   H=H, W=W, size=4, mode={"mean": 0, "vote": 1}[mode], fill=int(fill), out_probs=vec.data_ptr(), ldo=6,
                                   label_map=lab.data_ptr(), conf_map=conf.data_ptr(), margin_map=margin.data_ptr())
        _lib.check(_lib.load().hsimae_segment_vote(C.byref(p), torch.cuda.current_stream().cuda_stream), "hsimae_segment_vote")
        of_row = segs.labels.reshape(-1).long() if pix is None else segs.labels.reshape(-1).long()[pix.cuda()]
        assert same(got, (lab.view(H, W), conf.view(H, W), margin.view(H, W), vec[of_row]))
        # against the restatement, from the device's own inputs
        ref = R.vote_ref(res.probs.cpu().numpy(), n, 6, 1, None if row_of is None else row_of.cpu().numpy(), segs.labels.cpu().numpy(), 4,
                         p.mode, int(fill))
        vec_h = np.where(ref["live"][:, None], vec.cpu().numpy(), np.float32(0))
        chk = R.check_vote(ref, 1, 6, vec_h, None, lab.cpu().numpy(), conf.cpu().numpy(), margin.cpu().numpy(), 0)
        assert chk["all"] <= 1.0, chk
        if fill:                                                                   # every pixel of every segment that has a classified pixel
            live = torch.from_numpy(ref["live"]).cuda()[segs.labels.reshape(-1).long()]
            assert torch.equal(got.labels.reshape(-1) > 0, live) and (pix.numel() < H * W and int(live.sum()) > n)
        host = segment_classification(res, segs, pixels=pix, mode=mode, fill=fill)
        assert host.probs is None and not host.labels.is_cuda and torch.equal(host.labels, got.labels.cpu())
    with pytest.raises(ValueError, match="return_probs=True"):
        segment_classification(m.classify_scene(scene, batch_size=256, on_device=True), segs)


def test_the_evaluation_entry_points_take_superpixels_for_smooth(tmp_path):
    """test_model_scene, knn_eval_scene and linear_probe_scene with smooth=Superpixels(size=4): the scores returned are the scores
    of the map returned, the map differs from the unsmoothed one, and smooth=None is the call without it, bit for bit."""
    from hsimae_amd import Superpixels, knn_eval_scene, linear_probe_scene, test_model_scene
    from hsimae_amd.finetune_train import scores
    d = tiny_dualvit()
    ckpt = os.path.join(tmp_path, "ft.pkl")
    torch.save(d.state_dict(), ckpt)
    rng = np.random.default_rng(13)
    scene = scene_23x19()
    gt = rng.integers(0, 6, size=(23, 19))
    gt.reshape(-1)[:6] = np.arange(6)
    flat = gt.reshape(-1)
    train_index = np.flatnonzero((flat != 0) & (rng.random(437) < 0.3))
    train_labels = flat[train_index]
    test_gt = gt.copy()
    test_gt.reshape(-1)[train_index] = 0
    kw = dict(depth=3, dim=32, s_depth=2, batch_size=256)
    sp = Superpixels(size=4)
    calls = ((test_model_scene, (scene, test_gt, gt, str(tmp_path), "ft.pkl"), {}),
             (knn_eval_scene, (scene, train_index, train_labels, test_gt, gt, ckpt), dict(k=5)),
             (linear_probe_scene, (scene, train_index, train_labels, test_gt, gt, ckpt), dict(max_iter=10)))
    for fn, args, extra in calls:
        base = quiet(fn, *args, **kw, **extra)
        none = quiet(fn, *args, smooth=None, **kw, **extra)
        assert base[:3] == none[:3] and np.array_equal(base[3], none[3]) and np.array_equal(base[4], none[4])
        out = quiet(fn, *args, smooth=sp, **kw, **extra)
        assert out[4].shape == gt.shape and out[4].min() >= 1 and not np.array_equal(out[4], base[4])
        want = scores(test_gt.reshape(-1), np.where(gt == 0, 0, out[4]).reshape(-1))
        assert max(abs(a - b) for a, b in zip(out[:3], want[:3])) <= 1e-12 and np.abs(out[3] - want[3]).max() <= 1e-12
    with pytest.raises(TypeError):
        test_model_scene(scene, test_gt, gt, str(tmp_path), "ft.pkl", smooth="superpixels", **kw)
