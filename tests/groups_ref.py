"""fp64 restatement and error bound for the grouped AdamW step of csrc/clip.hip (hsimae_adamw_step_groups; tests/test_gpu_groups.py,
tests/test_groups_bound_cpu.py), and the test side's own restatement of the layer table FusedAdamW(layer_decay=) builds.

A plain module, not a conftest, in the idiom of clip_ref.py.  Nothing here is measured:

  step    clip_ref.adamw_ctl_ref (elem_ref.adamw_ref fed g * coef, with its slack for the multiply and the two bias corrections)
          is applied once per table entry, to the elements that carry that entry's id, with that entry's fp32 lr and weight decay,
          and the results are merged by id.  The bound of an element is therefore clip_ref's step bound evaluated with the
          element's own lr and weight decay.  An entry whose weight decay is 0 does not decay (hsimae_adamw_step's id 1).
  frozen  id 2 and every id >= ngroups pass through untouched, whatever the table holds at 2: reference = input, bound 0.
"""
import re

import torch

import clip_ref as R
from clip_ref import Out, f32, gen, skew, adamw_inputs, ADAMW_HP, STEP_N  # noqa: F401  (re-exported for the two test files)

MAX_GROUPS = 64                   # HSIMAE_ADAMW_MAX_GROUPS
N_STRIDE = 4 * 256 * 2048 + 4 * 37 + 3      # one full pass of the capped grid (2048 workgroups of float4), a partial one, a tail of 3


def live_mask(ids, ngroups):
    return (ids != 2) & (ids < ngroups)


def adamw_groups_ref(p, g, m, v, ids, table, coef, apply_, t, b1, b2, eps):
    """hsimae_adamw_step_groups.  table: [(lr, weight_decay)] of length ngroups (entry 2 is never looked at); coef: the fp32
    coefficient the step reads (1.0 without a control block); t: the step of the bias corrections.  p, g, m, v: fp32 tensors, or
    fp64 ones when a trajectory is carried in fp64."""
    ngroups = len(table)
    ref = {k: a.double().clone() for k, a in (("p", p), ("m", m), ("v", v))}
    term = {k: torch.zeros_like(a) for k, a in ref.items()}
    if apply_:
        for k, (lr, wd) in enumerate(table):
            if k == 2:
                continue
            idx = torch.nonzero(ids == k).reshape(-1)
            if idx.numel() == 0:
                continue
            kind = torch.full((idx.numel(),), 0 if f32(wd) != 0.0 else 1, dtype=torch.uint8)
            one = R.adamw_ctl_ref(p[idx], g[idx], m[idx], v[idx], kind, coef, 1, t, lr, b1, b2, eps, wd)
            for name in "pmv":
                ref[name][idx] = one[name].ref
                term[name][idx] = one[name].term
    assert not bool(term["p"][~live_mask(ids, ngroups)].any())
    return {k: Out(ref[k], "C_ADAM", term[k]) for k in "pmv"}


def table_for(ngroups, base_lr=1e-3, decay=0.75, wd=0.05):
    """lr falls geometrically with the id, every other entry decays; entry 2 holds values no step may use."""
    t = [(base_lr * decay ** k, wd if k % 2 == 0 else 0.0) for k in range(ngroups)]
    if ngroups > 2:
        t[2] = (-1.0, float("nan"))
    return t


def ids_for(n, ngroups, seed):
    """Ids drawn per element over the table (most float4 mix groups), with runs of one id, runs of id 2 (all-frozen float4), and
    ids >= ngroups planted (ngroups itself, 255 and a value in between)."""
    g_ = gen(seed)
    ids = torch.randint(0, ngroups, (n,), generator=g_, dtype=torch.uint8)
    beyond = [v for v in (ngroups, (ngroups + 255) // 2, 255)]
    if n >= 64:
        ids[8:24] = ngroups - 1
        ids[24:40] = 2
        ids[40:44] = 0
        ids[44:48] = torch.tensor([beyond[0], beyond[1], beyond[2], beyond[0]], dtype=torch.uint8)
        where = torch.randperm(n, generator=g_)[: max(3, n // 16)]
        for j, w in enumerate(where.tolist()):
            ids[w] = (2, beyond[0], beyond[2])[j % 3]
        ids[n - 3:] = torch.tensor([0, 2, ngroups - 1], dtype=torch.uint8)     # the tail behind the float4 body
    else:
        plant = [0, 2, beyond[0], ngroups - 1, 255]
        for j in range(n):
            ids[j] = plant[j % len(plant)]
    return ids


def step_inputs(n, ngroups, seed):
    """elem_ref.adamw_inputs with ids over the table and NaN gradients under every element the step must not touch."""
    inp = adamw_inputs(max(n, 64), seed)
    inp = {k: a[:n].clone() for k, a in inp.items() if k != "group"}
    inp["g"] = torch.where(inp["g"].isnan(), torch.full_like(inp["g"], 0.02), inp["g"])
    inp["ids"] = ids_for(n, ngroups, seed + 100)
    inp["g"][~live_mask(inp["ids"], ngroups)] = float("nan")
    return inp


# ------------------------------------------------------------------------------------------------ the layer table, restated
def layer_of(name, depth, s_depth):
    """patch_embed.*, pos_embed: 0;  blocks_1.i / blocks_2.i: 1 + i;  blocks.j: 1 + s_depth + j;  everything else: depth + 1."""
    if name == "pos_embed" or name.startswith("patch_embed."):
        return 0
    for stack, base in (("blocks_1", 1), ("blocks_2", 1), ("blocks", 1 + s_depth)):
        hit = re.match(r"^" + stack + r"\.(\d+)\.", name)
        if hit:
            return base + int(hit.group(1))
    return depth + 1


def layer_table(names, depth, s_depth, layer_decay, lr, wd, no_decay=("bias", "norm"), frozen=()):
    """names -> (ids {name: table id, 2 for a frozen name}, table [(lr * scale, wd)], scales [scale per table id]).  Top layer
    first: ids 0 / 1 are decay / no decay at scale 1, the hole at 2, the next layer takes 3 / 4, and so on."""
    keys = {(1.0, False), (1.0, True)}
    key_of = {}
    for n in names:
        if n == "mask_token" or any(n.startswith(f) for f in frozen):
            continue
        scale = 1.0 if layer_decay is None else layer_decay ** (depth + 1 - layer_of(n, depth, s_depth))
        key_of[n] = (scale, any(k in n for k in no_decay))
        keys.add(key_of[n])
    order = sorted(keys, key=lambda k: (-k[0], k[1]))
    gid = {k: (i if i < 2 else i + 1) for i, k in enumerate(order)}
    ngroups = max(gid.values()) + 1
    table, scales = [(0.0, 0.0)] * ngroups, [0.0] * ngroups
    for (scale, nd), i in gid.items():
        table[i], scales[i] = (lr * scale, 0.0 if nd else wd), scale
    return {n: gid[key_of[n]] if n in key_of else 2 for n in names}, table, scales
