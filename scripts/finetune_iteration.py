"""Fine-tuning iteration at the reference's defaults: the parent's loop body (torch CrossEntropyLoss, argmax, loss.item())
against this tree's (ClassLoss, device sums), alternating, on the same model; epoch-end metric; test_model_scene tail.
--prep: the data side instead, on a synthetic 610 x 340 x 32 fp64 scene: host time and peak host bytes of building data_cubes +
data_cubes_2 + the three HSIdataset uploads against get_scene_set_dual(GWPCA=False) + three SceneCubes, and the batch assembly
time per iteration of both at the reference's batch sizes (-> profiles/finetune_prep.json)."""
import contextlib, io, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.getcwd())
from hsimae_amd import DualViT, ClassLoss, ScoreMeter, FusedAdamW
from hsimae_amd.finetune_train import scores

PROFILE = "--profile" in sys.argv
dev = torch.device("cuda:0")


def prep():
    import random
    import tracemalloc
    from hsimae_amd import DeviceLoader, SceneCubes, get_scene_set_dual, unlabeled_pixels
    from hsimae_amd.finetune_train import HSIdataset, spilt_dataset
    from hsimae_amd.scene_data import split_labeled, tile_origins
    H, W, Cb, n_class = 610, 340, 32, 10
    rng = np.random.default_rng(0)
    raw = rng.standard_normal((H, W, Cb))
    gt = rng.integers(0, n_class, (H, W)); gt.reshape(-1)[:n_class] = np.arange(n_class)
    res = {"scene": [H, W, Cb], "scene_bytes": raw.nbytes}
    torch.zeros(1, device=dev); torch.cuda.synchronize()

    def measured(fn):
        tracemalloc.start(); torch.cuda.synchronize(); t = time.perf_counter()
        out = fn(); torch.cuda.synchronize(); dt = time.perf_counter() - t
        peak = tracemalloc.get_traced_memory()[1]; tracemalloc.stop()
        return out, dt, peak

    def old_prep():                                                 # Utils/Preprocessing.py:205-213 + Model_Finetuning.py:111-115
        cubes2 = np.array([raw[r:r + 9, c:c + 9] for r in tile_origins(H) for c in tile_origins(W)])
        pad = np.pad(raw, ((4, 4), (4, 4), (0, 0)), "symmetric")
        cubes = np.array([pad[r:r + 9, c:c + 9] for r in range(H) for c in range(W)])
        np.random.seed(1); idx, lab, _ = split_labeled(gt, num=40)
        np.random.seed(2); tr_x, tr_y, va_x, va_y = spilt_dataset([cubes[i] for i in idx], lab, training_ratio=0.5)
        return HSIdataset(tr_x, tr_y, train=True, device=dev), HSIdataset(cubes2, train=True, device=dev), HSIdataset(va_x, va_y, device=dev)

    def new_prep():
        np.random.seed(1); idx, lab, scene, _, _ = get_scene_set_dual(raw, gt, num=40, GWPCA=False, device=dev)
        np.random.seed(2); tr_i, tr_y, va_i, va_y = spilt_dataset(list(idx), lab, training_ratio=0.5)
        return SceneCubes(scene, tr_i, tr_y, train=True), SceneCubes(scene, unlabeled_pixels(H, W), train=True), SceneCubes(scene, va_i, va_y)

    sets = {}
    for name, fn in (("new", new_prep), ("old", old_prep)):
        sets[name], res[f"prep_{name}_s"], res[f"prep_{name}_peak_host_bytes"] = measured(fn)
        print(f"prep {name}: {res[f'prep_{name}_s']:.3f} s, peak host {res[f'prep_{name}_peak_host_bytes'] / 1e6:.1f} MB, "
              f"{len(sets[name][0])} / {len(sets[name][1])} / {len(sets[name][2])} items")

    def epoch(ds3):                                                 # the loop's data path, Model_Finetuning.py:119-122, 144-149
        train_dl = DeviceLoader(ds3[0], batch_size=32, shuffle=True)
        unl_dl = DeviceLoader(ds3[1], batch_size=int(np.ceil(len(ds3[1]) / len(train_dl)) / 2), shuffle=True)
        a, b = iter(train_dl), iter(unl_dl)
        for _ in range(len(train_dl)):
            next(a); next(b)
        return len(train_dl)

    for name in ("old", "new"):
        torch.manual_seed(0); epoch(sets[name]); torch.cuda.synchronize()
        times = []
        for rep in range(5):
            t = time.perf_counter(); n = epoch(sets[name]); torch.cuda.synchronize()
            times.append((time.perf_counter() - t) / n * 1e3)
        res[f"batch_{name}_ms"] = times
        print(f"batch assembly, ms / iteration (labeled 32 + unlabeled), {name}:", ["%.3f" % v for v in times])
    random.seed(3)
    xo = sets["old"][0].batch(list(range(32)))
    random.seed(3)
    xn = sets["new"][0].batch(list(range(32)))
    res["first_batch_equal"] = bool(torch.equal(xo[0], xn[0]) and torch.equal(xo[1], xn[1]))
    print("first labeled batch equal:", res["first_batch_equal"])
    os.makedirs("profiles", exist_ok=True)
    json.dump(res, open("profiles/finetune_prep.json", "w"), indent=1)


if "--prep" in sys.argv:
    prep(); sys.exit(0)

torch.manual_seed(0); np.random.seed(0)
n_class, bands, B = 10, 32, 32
with contextlib.redirect_stdout(io.StringIO()):
    model = DualViT(img_size=9, patch_size=3, in_chans=1, bands=bands, b_patch_size=8, num_class=n_class, embed_dim=144, depth=12,
                    num_heads=9, s_depth=6, decoder_embed_dim=72, decoder_depth=2, decoder_num_heads=9, norm_pix_loss=True,
                    trunc_init=True, drop_path=0.2).to(dev)
opt = FusedAdamW(model, lr=1e-3, weight_decay=5e-3)
nb = 8
xs = [torch.rand(B, 1, bands, 9, 9, device=dev) for _ in range(nb)]
xus = [torch.rand(2 * B, 1, bands, 9, 9, device=dev) for _ in range(nb)]
ys = [torch.randint(0, n_class, (B,), device=dev) for _ in range(nb)]
ce = torch.nn.CrossEntropyLoss(reduction="mean", ignore_index=0)
cl = ClassLoss(ignore_index=0)
model.train()

def old_iters(n):
    train_loss, preds, gts = 0.0, [], []
    for i in range(n):
        x, xu, y = xs[i % nb], xus[i % nb], ys[i % nb]
        loss_rec, _, _, out = model(x, xu, mask_ratio=0.5)
        loss = 5 * loss_rec + ce(out, y)
        preds.append(out.detach().argmax(1)); gts.append(y)
        opt.zero_grad(); loss.backward(); opt.step()
        train_loss += loss.item()
    return train_loss

def new_iters(n):
    train_loss = torch.zeros((), dtype=torch.float64, device=dev)
    for i in range(n):
        x, xu, y = xs[i % nb], xus[i % nb], ys[i % nb]
        loss_rec, _, _, out = model(x, xu, mask_ratio=0.5)
        loss = 5 * loss_rec + cl(out, y)
        opt.zero_grad(); loss.backward(); opt.step()
        train_loss += loss.detach()
    return float(train_loss)

def timed(fn, n):
    torch.cuda.synchronize(); t = time.perf_counter(); fn(n); torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3

if PROFILE:
    new_iters(3); torch.cuda.synchronize()
    print("profiled 3 iterations of the new loop body"); sys.exit(0)

old_iters(5); new_iters(5)
res = {"old_ms": [], "new_ms": []}
N_IT = 40
for rep in range(6):
    res["old_ms"].append(timed(old_iters, N_IT)); res["new_ms"].append(timed(new_iters, N_IT))
print("ms / iteration, old:", ["%.3f" % v for v in res["old_ms"]]); print("ms / iteration, new:", ["%.3f" % v for v in res["new_ms"]])

# same seeded inputs: the two losses agree
torch.manual_seed(1); model.eval()
with torch.no_grad():
    out = model(xs[0], mask_ratio=0.5)
    a, b = ce(out, ys[0]).item(), cl(out, ys[0]).item()
print(f"loss on the same logits: torch {a:.7f}  ClassLoss {b:.7f}")
res["loss_torch"], res["loss_classloss"] = a, b

# epoch-end metric: 20 validation batches of 512
gts = [torch.randint(0, n_class, (512,), device=dev) for _ in range(20)]
prs = [torch.where(torch.rand(512, device=dev) < 0.7, g, torch.randint(0, n_class, (512,), device=dev)) for g in gts]
def old_metric():
    return scores(torch.cat(gts).cpu().numpy(), torch.cat(prs).cpu().numpy())
meter = ScoreMeter(n_class, dev)
def new_metric():
    meter.reset()
    for g, p in zip(gts, prs): meter.update(g, p)
    return meter.compute()
def wall(fn, reps):
    fn(); torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps): r = fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t) / reps * 1e3, r
res["metric_old_ms"], ro = wall(old_metric, 10); res["metric_new_ms"], rn = wall(new_metric, 10)
print(f"epoch-end metric over 10240 samples: host scores() {res['metric_old_ms']:.2f} ms, ScoreMeter (20 updates + compute) {res['metric_new_ms']:.3f} ms; OA {ro[0]:.6f} / {rn[0]:.6f}")

# test_model_scene from the end of predict_scene to its return, 610 x 340
H, W = 610, 340
gt = np.random.randint(0, n_class, (H, W)); test_gt = np.where(np.random.rand(H, W) < 0.8, gt, 0)
pred_dev = torch.randint(1, n_class, (H, W), device=dev)
def old_tail():
    pred = pred_dev.cpu().numpy().reshape(gt.shape)
    pred_all = pred.copy(); pred[gt == 0] = 0
    return scores(test_gt.reshape(-1), pred.reshape(-1))
def new_tail():
    m = ScoreMeter(n_class, dev)
    m.update_map(test_gt.reshape(-1), pred_dev.reshape(-1), mask_map=gt.reshape(-1))
    r = m.compute(); pred_all = pred_dev.cpu().numpy().reshape(gt.shape)
    return r
res["tail_old_ms"], ro = wall(old_tail, 3); res["tail_new_ms"], rn = wall(new_tail, 10)
print(f"test_model_scene tail 610 x 340: host {res['tail_old_ms']:.1f} ms, device {res['tail_new_ms']:.2f} ms; OA {ro[0]:.9f} / {rn[0]:.9f} kappa {ro[2]:.9f} / {rn[2]:.9f}")
os.makedirs("profiles", exist_ok=True)
json.dump(res, open("profiles/finetune_iteration.json", "w"), indent=1)
