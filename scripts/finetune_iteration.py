"""Fine-tuning iteration at the reference's defaults: the parent's loop body (torch CrossEntropyLoss, argmax, loss.item())
against this tree's (ClassLoss, device sums), alternating, on the same model; epoch-end metric; test_model_scene tail."""
import contextlib, io, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.getcwd())
from hsimae_amd import DualViT, ClassLoss, ScoreMeter, FusedAdamW
from hsimae_amd.finetune_train import scores

PROFILE = "--profile" in sys.argv
dev = torch.device("cuda:0")
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
