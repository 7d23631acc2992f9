"""The grouped AdamW step without a GPU: the fp64 restatement (tests/groups_ref.py) against torch.optim.AdamW in fp64 with one
torch group per table entry, the bound against planted faults, `hsimae_amd.optim.layer_ids` over the manifest's name lists, and
the groups FusedAdamW(layer_decay=, freeze=) builds on a CPU model object."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import groups_ref as G  # noqa: E402

N = G.STEP_N


@pytest.fixture(autouse=True)
def rng_state_left_as_found():
    """Tests that run after this file and draw from the global generators without seeding find them as they would have without it."""
    import random
    saved = random.getstate(), np.random.get_state(), torch.get_rng_state()
    yield
    random.setstate(saved[0])
    np.random.set_state(saved[1])
    torch.set_rng_state(saved[2])


def clean_inputs(ngroups, seed=5, n=N):
    """step_inputs with finite gradients under the untouched lanes too (a fault that steps them shows as a number)."""
    inp = G.step_inputs(n, ngroups, seed)
    inp["g"][~G.live_mask(inp["ids"], ngroups)] = 0.75
    return inp


# ------------------------------------------------------------------------------------------------ against torch, fp64
@pytest.mark.parametrize("ngroups", [1, 3, 29, 64])
def test_restatement_equals_torch_adamw_with_one_group_per_entry_in_fp64(ngroups):
    """Three steps, the learning rates changed between them.  Every value the restatement rounds to fp32 is exact there: the
    table's lr and weight decay are rounded before torch sees them, b1 = 1/2, b2 = 3/4, eps = 2^-20, and torch's step count is
    held at 1 (both bias corrections are exactly 2), so 1e-12 of each array's magnitude can be asked.  The moments and the
    parameters carry over from step to step in fp64 on both sides."""
    b1, b2, eps = 0.5, 0.75, 2.0 ** -20
    inp = G.step_inputs(N, ngroups, 7)
    ids = inp["ids"]
    idx = {k: torch.nonzero(ids == k).reshape(-1) for k in range(ngroups) if k != 2}
    idx = {k: i for k, i in idx.items() if i.numel()}
    assert len(idx) == ngroups - (1 if ngroups > 2 else 0), "an entry without elements"
    params = {k: torch.nn.Parameter(inp["p"][i].double()) for k, i in idx.items()}
    opt = torch.optim.AdamW([dict(params=[params[k]], lr=1.0, weight_decay=0.0) for k in idx], lr=1.0, betas=(b1, b2), eps=eps)
    for k, i in idx.items():                                   # moments that are not zero
        opt.state[params[k]] = dict(step=torch.tensor(0.0), exp_avg=inp["m"][i].double().clone(), exp_avg_sq=inp["v"][i].double().clone())
    state = {k: inp[k].double() for k in "pmv"}
    for step, base in enumerate((1e-3, 3.3e-4, 2.5e-3)):
        table = [(G.f32(lr), G.f32(wd) if wd == wd else wd) for lr, wd in G.table_for(ngroups, base_lr=base)]
        for grp, k in zip(opt.param_groups, idx):
            grp["lr"], grp["weight_decay"] = table[k]
            params[k].grad = inp["g"][idx[k]].double()
            opt.state[params[k]]["step"] = torch.tensor(0.0)
        opt.step()
        ref = G.adamw_groups_ref(state["p"], inp["g"], state["m"], state["v"], ids, table, 1.0, 1, 1, b1, b2, eps)
        for k, i in idx.items():
            st = opt.state[params[k]]
            for name, got in (("p", params[k].detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
                want = ref[name].ref[i]
                err = float((got - want).abs().max())
                assert err <= 1e-12 * float(want.abs().max()), (ngroups, step, k, name, err)
        dead = ~G.live_mask(ids, ngroups)
        for name in "pmv":
            assert torch.equal(ref[name].ref[dead], state[name][dead]) and not bool(ref[name].bound()[dead].any())
        state = {name: ref[name].ref for name in "pmv"}


# ------------------------------------------------------------------------------------------------ fp32 emulation and faults
NG = 9                                                         # the faults' table: ids 0, 1, 3 .. 8 live, 2 the hole
LR, SCALES = 1e-3, [0.75 ** (k // 2) for k in range(NG)]       # (lr, lr_scale) per entry, as param_groups hold them


def build_table(fault=None):
    """The table as FusedAdamW forms it: lr * lr_scale in fp64, rounded once to fp32; every other entry decays."""
    t = []
    for k, s in enumerate(SCALES):
        eff = LR * s * s if fault == "scale_twice" else LR if fault == "scale_not_applied" else LR * s
        t.append((G.f32(eff), G.f32(0.05) if k % 2 == 0 else 0.0))
    if fault == "neighbours_swapped":
        t[5], t[6] = t[6], t[5]
    t[2] = (G.f32(7e-4), G.f32(0.05))                          # finite, so that a step that uses it shows as a number
    return t


def emulate(inp, table, coef, t, hp, fault=None):
    """The kernel as it computes, in fp32, element by element through a gathered table."""
    f = np.float32
    ids = inp["ids"].long()
    ng = len(table)
    live = G.live_mask(inp["ids"], ng)
    look = ids.clamp(max=ng - 1)
    if fault == "frozen_updated":
        live = live | (inp["ids"] == 2)
        look = torch.where(inp["ids"] == 2, torch.zeros_like(look), look)
    if fault == "table2_used":
        live = live | (inp["ids"] == 2)
    if fault == "beyond_uses_last":
        live = live | (inp["ids"] >= ng)
    lr = torch.tensor([f(a) for a, _ in table])[look]
    wd = torch.tensor([f(b) for _, b in table])[look]
    if fault == "group0_lr":
        lr = torch.full_like(lr, float(f(table[0][0])))
    if fault == "decay_on_wd0":
        wd = torch.full_like(wd, float(f(table[0][1])))
    b1, b2, eps = f(hp["b1"]), f(hp["b2"]), f(hp["eps"])
    i1, i2 = (G.f32(a) for a in G.R.bias_corrections(t, hp["b1"], hp["b2"]))
    p, m, v = inp["p"], inp["m"], inp["v"]
    gc = torch.where(live, inp["g"], torch.zeros_like(inp["g"])) * float(f(coef))
    x = torch.where(wd != 0, p * (1.0 - lr * wd), p)
    mn = m + (gc - m) * float(f(1) - b1)
    vn = v * float(b2) + gc * gc * float(f(1) - b2)
    den = torch.sqrt(vn) * i2 + float(eps)
    pn = x - lr * i1 * (mn / den)
    return dict(p=torch.where(live, pn, p), m=torch.where(live, mn, m), v=torch.where(live, vn, v))


def judge(got, inp, table, coef, t, hp):
    ref = G.adamw_groups_ref(inp["p"], inp["g"], inp["m"], inp["v"], inp["ids"], table, coef, 1, t, hp["b1"], hp["b2"], hp["eps"])
    return max(ref[k].ratio(got[k]) for k in "pmv")


@pytest.mark.parametrize("coef", [1.0, 0.3])
@pytest.mark.parametrize("ngroups", [1, 3, 29, 64])
def test_fp32_emulation_stays_within_the_bound(ngroups, coef):
    hp = G.ADAMW_HP
    inp = clean_inputs(ngroups)
    table = [(G.f32(a), G.f32(b)) for a, b in G.table_for(ngroups)]
    if ngroups > 2:
        table[2] = (G.f32(7e-4), G.f32(0.05))
    for t in (1, 2, 1000):
        w = judge(emulate(inp, table, G.f32(coef), t, hp), inp, table, G.f32(coef), t, hp)
        print(f"ngroups {ngroups} coef {coef} t {t}: worst err / bound {w:.3f}")
        assert w <= 1.0


FAULTS = ["group0_lr", "decay_on_wd0", "scale_twice", "scale_not_applied", "frozen_updated", "table2_used", "beyond_uses_last",
          "neighbours_swapped"]


@pytest.mark.parametrize("fault", FAULTS)
def test_bound_rejects_planted_faults(fault):
    hp = G.ADAMW_HP
    inp = clean_inputs(NG)
    assert all(bool((inp["ids"] == k).any()) for k in range(NG)) and bool((inp["ids"] >= NG).any())
    good = build_table()
    assert judge(emulate(inp, good, 1.0, 2, hp), inp, good, 1.0, 2, hp) <= 1.0       # the harness itself is clean on this very input
    in_table = fault in ("scale_twice", "scale_not_applied", "neighbours_swapped")
    got = emulate(inp, build_table(fault) if in_table else good, 1.0, 2, hp, None if in_table else fault)
    w = judge(got, inp, good, 1.0, 2, hp)
    print(f"{fault}: worst err / bound = {w:.3g}")
    assert w > 10.0, w


# ------------------------------------------------------------------------------------------------ layer ids
def manifest():
    with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as fh:
        return json.load(fh)


def depths_of(names):
    s_depth = 1 + max(int(n.split(".")[1]) for n in names if n.startswith("blocks_1."))
    rest = [int(n.split(".")[1]) for n in names if n.startswith("blocks.")]
    return s_depth + (1 + max(rest) if rest else 0), s_depth


@pytest.mark.parametrize("key", ["C2_base96", "HSIMAE_base32", "DualViT_base32", "HSIViT_base32"])
def test_layer_ids_over_the_manifests_name_lists(key):
    from hsimae_amd.optim import layer_ids
    names = [row[0] for row in manifest()[key]]
    depth, s_depth = depths_of(names)
    if key == "C2_base96":
        assert (depth, s_depth) == (12, 9) and names == manifest()["named_parameters_C2"]
    ids = layer_ids(names, depth=depth, s_depth=s_depth)
    assert list(ids) == names and all(isinstance(v, int) and 0 <= v <= depth + 1 for v in ids.values())
    for n, i in ids.items():
        hit = re.match(r"^(blocks_1|blocks_2|blocks)\.(\d+)\.", n)
        if n == "pos_embed" or n.startswith("patch_embed."):
            assert i == 0, n
        elif hit and hit.group(1) == "blocks":
            assert i == 1 + s_depth + int(hit.group(2)), n
        elif hit:
            assert i == 1 + int(hit.group(2)), n
        else:
            assert i == depth + 1, n
            assert n.split(".")[0] in ("norm", "cls_head", "mask_token", "decoder_pos_embed", "decoder_embed", "decoder_blocks",
                                       "decoder_norm", "decoder_pred"), n
        assert i == G.layer_of(n, depth, s_depth)
    for n in names:                                            # the two axis stacks share a depth
        if n.startswith("blocks_1."):
            assert ids[n] == ids["blocks_2." + n[len("blocks_1."):]]
    assert max(ids.values()) == depth + 1 == ids["norm.weight"] and min(ids.values()) == 0
    assert sorted(set(ids.values())) == list(range(depth + 2)), "a layer without a parameter"
    if "cls_head.weight" in ids:
        assert ids["cls_head.weight"] == ids["cls_head.bias"] == depth + 1
    assert 0.75 ** (depth + 1 - ids["norm.weight"]) == 1.0      # the scale of the top id is exactly 1
    with pytest.raises(ValueError):
        layer_ids(names)                                       # a bare list of names carries no depth


# ------------------------------------------------------------------------------------------------ group construction
def cpu_model(kind="HSIMAE", depth=4, s_depth=2, dim=64):
    import contextlib
    import io
    from hsimae_amd import HSIMAE, DualViT
    kw = dict(img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, embed_dim=dim, depth=depth, s_depth=s_depth,
              num_heads=4, decoder_embed_dim=32, decoder_depth=1, decoder_num_heads=4, norm_pix_loss=True, trunc_init=True)
    with contextlib.redirect_stdout(io.StringIO()):
        return HSIMAE(**kw) if kind == "HSIMAE" else DualViT(num_class=4, drop_path=0.0, **kw)


@pytest.mark.parametrize("kind", ["HSIMAE", "DualViT"])
def test_groups_of_a_layer_decay_optimizer(kind):
    from hsimae_amd import FusedAdamW
    from hsimae_amd.optim import layer_ids
    m = cpu_model(kind)
    depth = 4
    opt = FusedAdamW(m, lr=2e-3, weight_decay=5e-3, layer_decay=0.75)
    lids = layer_ids(m)
    assert max(lids.values()) == depth + 1
    groups = opt.param_groups
    assert len(groups) == 2 * (depth + 2)                      # layers 0 .. depth + 1, each with and without decay
    for j, g in enumerate(groups):
        assert {"params", "lr", "weight_decay", "lr_scale", "betas", "eps"} <= set(g)
        assert g["lr_scale"] == 0.75 ** (j // 2) and g["lr"] == 2e-3
        assert g["weight_decay"] == (5e-3 if j % 2 == 0 else 0.0) and g["params"]
    assert groups[0]["lr_scale"] == groups[1]["lr_scale"] == 1.0
    assert opt._gids == [0, 1] + list(range(3, 2 * (depth + 2) + 1)) and 2 not in opt._gids and opt._ngroups == 2 * (depth + 2) + 1
    # every parameter that is stepped lies in exactly one group, and in the one its name asks for
    name_of = {id(p): n for n, p in m.named_parameters()}
    seen = [id(p) for g in groups for p in g["params"]]
    assert len(seen) == len(set(seen))
    assert set(seen) == {id(p) for n, p in m.named_parameters() if n != "mask_token" and p.requires_grad}
    for g in groups:
        for p in g["params"]:
            n = name_of[id(p)]
            assert g["lr_scale"] == 0.75 ** (depth + 1 - lids[n]), n
            assert (g["weight_decay"] == 0.0) == any(k in n for k in ("bias", "norm")), n
    # the ids the flat buffer is stepped with are the test's own restatement of the table
    flat_names = [n for n, _ in m.named_parameters() if not n.startswith("cls_head.")]
    fixed = tuple(n for n, p in m.named_parameters() if not p.requires_grad)      # the sin-cos position tables
    assert set(fixed) <= {"pos_embed", "decoder_pos_embed"}
    want, table, _ = G.layer_table([n for n, _ in m.named_parameters()], depth, 2, 0.75, 2e-3, 5e-3, frozen=fixed)
    assert opt._groups_of == [want[n] for n in flat_names]
    got = opt._table()
    assert len(got) == len(table) == opt._ngroups
    for k, (lr, wd) in enumerate(table):
        if k != 2:
            assert (got[k].lr, got[k].weight_decay) == (G.f32(lr), G.f32(wd)), k
    assert opt.lr_range() == (2e-3 * 0.75 ** (depth + 1), 2e-3)
    if kind == "DualViT":                                      # the head is stepped with ids 0 / 1 at scale 1
        head = {id(m.cls_head.weight): 0, id(m.cls_head.bias): 1}
        assert id(m.cls_head.weight) in {id(p) for p in groups[0]["params"]} and id(m.cls_head.bias) in {id(p) for p in groups[1]["params"]}
        clipped = FusedAdamW(m, lr=2e-3, layer_decay=0.75, max_grad_norm=1.0)
        assert [(id(p), gid) for p, gid in clipped._outside] == list(head.items())


def test_freeze_removes_the_prefixes_from_every_group_and_the_default_is_the_two_dicts_it_was():
    from hsimae_amd import FusedAdamW
    m = cpu_model("DualViT")
    plain = FusedAdamW(m, lr=1e-3)
    assert len(plain.param_groups) == 2 and all(set(g) == {"params", "lr", "weight_decay", "betas", "eps"} for g in plain.param_groups)
    assert plain._gids == [0, 1] and plain._ngroups == 2 and set(plain._groups_of) == {0, 1, 2} and plain._defaults_agree()
    plain.param_groups[1]["lr"] = 3e-3
    assert not plain._defaults_agree()
    frozen = ("patch_embed", "blocks_1.0.", "blocks_2.0.")
    for kw in (dict(), dict(layer_decay=0.75)):
        opt = FusedAdamW(m, lr=1e-3, freeze=frozen, **kw)
        kept = {id(p) for g in opt.param_groups for p in g["params"]}
        flat_names = [n for n, _ in m.named_parameters() if not n.startswith("cls_head.")]
        for n, p in m.named_parameters():
            assert (id(p) in kept) == (not n.startswith(frozen) and n != "mask_token" and p.requires_grad), n
        for n, gid in zip(flat_names, opt._groups_of):
            assert (gid == 2) == (n.startswith(frozen) or n == "mask_token" or not dict(m.named_parameters())[n].requires_grad), n
        assert not opt._defaults_agree()                       # an optimizer built with freeze takes the grouped launch
    probe = FusedAdamW(m, lr=1e-3, freeze=tuple(n for n, _ in m.named_parameters() if not n.startswith("cls_head.")))
    assert [len(g["params"]) for g in probe.param_groups] == [1, 1] and set(probe._groups_of) == {2}
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="layer_decay"):
            FusedAdamW(m, layer_decay=bad)


def test_more_than_64_table_entries_raise():
    """depth 31: layers 0 .. 32 with and without decay are 66 groups; depth 30 gives 64 groups and, with the hole at 2, 65 entries:
    one too many as well.  depth 29 (62 groups, 63 entries) is taken."""
    from hsimae_amd import FusedAdamW
    for depth, ok in ((29, True), (30, False), (31, False)):
        m = cpu_model("HSIMAE", depth=depth, s_depth=2, dim=16)
        if ok:
            assert FusedAdamW(m, layer_decay=0.9)._ngroups == 63
        else:
            with pytest.raises(ValueError, match="table entries"):
                FusedAdamW(m, layer_decay=0.9)


def test_loading_a_checkpoint_with_another_group_count_raises():
    from hsimae_amd import FusedAdamW
    m = cpu_model("HSIMAE")
    two, many = FusedAdamW(m, lr=1e-3), FusedAdamW(m, lr=1e-3, layer_decay=0.75)
    with pytest.raises(ValueError, match=r"2 parameter groups.*12"):
        many.load_state_dict(two.state_dict())
    with pytest.raises(ValueError, match=r"12 parameter groups.*2"):
        two.load_state_dict(many.state_dict())
    sd = many.state_dict()
    assert [g["lr_scale"] for g in sd["param_groups"]] == [0.75 ** (j // 2) for j in range(12)]
    sd["param_groups"][3]["lr"] = 7e-4
    again = FusedAdamW(m, lr=1e-3, layer_decay=0.75)
    again.load_state_dict(sd)
    assert again.param_groups[3]["lr"] == 7e-4 and again.param_groups[3]["lr_scale"] == 0.75


def test_library_exports_the_grouped_step_and_refuses_before_any_launch():
    import ctypes as C
    from hsimae_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "hsimae_hip.h")).read()
    assert "hsimae_adamw_step_groups" in _lib.SYMBOLS and re.search(r"\bhsimae_adamw_step_groups\s*\(", hdr)
    assert int(re.search(r"#define HSIMAE_ADAMW_MAX_GROUPS (\d+)", hdr).group(1)) == _lib.ADAMW_MAX_GROUPS == G.MAX_GROUPS == 64
    assert C.sizeof(_lib.AdamWGroup) == 8 and C.sizeof(_lib.AdamWGroup * 64) == 512
    assert lib.hsimae_version() == _lib.ABI_VERSION == 108

    def tab(*pairs):
        return (_lib.AdamWGroup * max(len(pairs), 1))(*[_lib.AdamWGroup(a, b) for a, b in pairs])

    def st(p=1 << 20, g=1 << 21, m=1 << 22, v=1 << 23, group=None, gu=0, n=17, table=tab((1e-3, 0.05), (1e-3, 0.0)), ng=2, step=1,
           ctl=None):
        return lib.hsimae_adamw_step_groups(p, g, m, v, group, gu, n, table, ng, 0.9, 0.95, 1e-8, step, ctl, None)
    nan = float("nan")
    assert st(n=-1) == -1 and st(ng=0) == -1 and st(ng=65) == -1 and st(gu=-1) == -1 and st(gu=3) == -1 and st(step=0) == -1
    assert st(table=tab((-1e-3, 0.0), (1e-3, 0.0))) == -1 and st(table=tab((1e-3, -0.1), (1e-3, 0.0))) == -1
    assert st(table=tab((nan, 0.0), (1e-3, 0.0))) == -1 and st(table=tab((1e-3, 0.0), (1e-3, nan))) == -1
    assert st(p=None) == -4 and st(g=None) == -4 and st(m=None) == -4 and st(v=None) == -4 and st(table=None) == -4
    assert st(p=(1 << 20) + 2) == -3 and st(ctl=(1 << 24) + 4, step=0) == -3
    assert st(n=0) == 0 and st(n=0, table=None) == 0 and st(gu=2) == 0
    assert st(gu=2, table=tab((1e-3, 0.0), (1e-3, 0.0), (-1.0, nan)), ng=3) == 0      # table[2] is ignored
