"""Paired weight-gradient launches and the one decoder slab reduce of hsimae_backward (csrc/api.hip WgPair, csrc/plan.h
BlockPlan::wgrad_pair / DecPlan::reduce_once).

On the fused d = 128 path the weight gradients of two consecutive encoder blocks of a stack go out as one 14-task launch, the
first pair of fusion blocks takes decoder_embed's along (15 tasks), a stack with an odd number of blocks ends in a one-block
launch, and the fused decoder's blocks share one slab reduce.  HSIMAE_WGRAD_PAIR=0 / HSIMAE_DEC_REDUCE_ONCE=0 (read by the
forward, like every schedule switch) give one launch per block again.  No arithmetic differs between the two schedules, only
the order in which partial sums meet:

  * `deterministic` mode (fixed-point shadow sums: order-independent): every gradient tensor of the paired schedule is
    bit-identical to the unpaired one's.  Model: embed_dim 128, 8 heads, decoder 2 x 64, N = 6; bands 48 and 96 with every grid
    grid_candidates keeps (one and two); (s_depth, depth) = (2, 3), (3, 4), (3, 6): even and odd stacks with 1, 1 and 3 fusion blocks, so
    the left-over single block, the fusion pair and the folded decoder_embed task all run.  Once more in a child process with
    HSIMAE_TWO_STREAMS=0, where both axis stacks share the caller's stream and the spectral stack takes the second pair of
    operand sets.
  * default mode (float atomics): the paired launch as api.hip builds it, two blocks' tasks (+ decoder_embed's) in one
    hsimae_wgrad call at the planner's row split, against the same tasks as one launch per block, each within the bound
    tests/wgrad_ref.py derives for float-atomic commits (bound_dW / bound_db with the launch's own P and S, nothing added)
    and the two within the sum of their bounds.  The operands are needed for that bound, so this part runs at the launch
    level, on the problem builder of tests/test_gpu_wgrad.py.
  * the range callback: every element of the flat gradient buffer in exactly one report, offsets non-increasing per stack
    (and over the whole pass when no bucket stream is given).
  * a forward + backward in an arena of exactly hsimae_workspace_bytes (guard bytes behind it intact), refused in a smaller one."""
import contextlib
import ctypes as C
import io
import os
import subprocess
import sys

import pytest
import torch

from hsimae_amd import HSIMAE, _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_wgrad as TW  # noqa: E402
import wgrad_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 6
DEPTHS = [(2, 3), (3, 4), (3, 6)]
GRIDS = [(48, (2, 7)), (96, (3, 9)), (96, (9, 3))]          # every grid grid_candidates keeps at mask ratio 0.75: M = 84, 162, 162
UNPAIRED = {"HSIMAE_WGRAD_PAIR": "0", "HSIMAE_DEC_REDUCE_ONCE": "0"}


def make(bands, s_depth, depth, det):
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        m = HSIMAE(img_size=9, patch_size=3, in_chans=1, bands=bands, b_patch_size=8, embed_dim=128, depth=depth, num_heads=8,
                   s_depth=s_depth, decoder_embed_dim=64, decoder_depth=2, decoder_num_heads=8, norm_pix_loss=True, trunc_init=True)
    m = m.to(DEV)
    m.deterministic = det
    return m


def inputs(bands):
    g = torch.Generator().manual_seed(21)
    T = bands // 8
    x = torch.rand(N, 1, bands, 9, 9, generator=g).to(DEV)
    return x, (torch.rand(N, T, generator=g), torch.rand(N, 9, generator=g))


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def one_pass(m, x, noise, grid, **switches):
    m.zero_grad(set_to_none=True)
    with env(**switches):                 # the forward records the schedule; the backward follows the record
        loss = m(x, 0.75, noise=noise, grid=grid)[0]
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def det_case(bands, grid, s_depth, depth):
    m = make(bands, s_depth, depth, True)
    x, noise = inputs(bands)
    l0, g0 = one_pass(m, x, noise, grid)
    assert len(g0) > 50 and all(bool(torch.isfinite(v).all()) for v in g0.values())
    assert any(bool(v.abs().max() > 0) for k, v in g0.items() if k.startswith("decoder_embed"))
    for sw in ({"HSIMAE_WGRAD_PAIR": "0"}, {"HSIMAE_DEC_REDUCE_ONCE": "0"}, UNPAIRED):
        l1, g1 = one_pass(m, x, noise, grid, **sw)
        assert l1 == l0 and g1.keys() == g0.keys()
        bad = [n for n in g0 if not torch.equal(g0[n], g1[n])]
        assert not bad, f"{sw}: {len(bad)} gradients differ from the paired schedule's, e.g. {bad[:4]}"


@pytest.mark.parametrize("s_depth,depth", DEPTHS)
@pytest.mark.parametrize("bands,grid", GRIDS)
def test_deterministic_gradients_are_bit_identical(bands, grid, s_depth, depth):
    assert grid in HSIMAE.grid_candidates(bands // 8, 9, 0.75)
    det_case(bands, grid, s_depth, depth)


def test_the_grids_are_all_that_are_kept():
    assert sorted(GRIDS) == sorted((b, g) for b in (48, 96) for g in HSIMAE.grid_candidates(b // 8, 9, 0.75))


def test_deterministic_gradients_on_one_stream():
    """HSIMAE_TWO_STREAMS is read once per process: a child runs the odd and the even stack with both stacks on the caller's stream."""
    code = ("import sys; sys.path.insert(0, %r); import test_gpu_wgrad_pairing as T\n"
            "from hsimae_amd import _lib\n"
            "assert _lib.load().hsimae_two_streams_active() == 0\n"
            "T.det_case(48, (2, 7), 2, 3); T.det_case(96, (9, 3), 3, 6); print('one-stream ok')\n" % os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HSIMAE_TWO_STREAMS="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "one-stream ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------------------------------------ default mode, launch level
def pair_case(M, fold):
    """Two d = 128 blocks' tasks as block_bwd deposits them (planes where M allows) and, with `fold`, decoder_embed's."""
    planar = M % 32 == 0
    b = TW.block("x", M, 128, 344, 1, planar=planar)
    ops, tasks = {}, []
    for k in (0, 1):
        ops.update({f"{n}{k}": v for n, v in b.ops.items()})
        tasks += [t._replace(dO=f"{t.dO}{k}", A=f"{t.A}{k}") for t in b.tasks]
    if fold:
        ops.update(dyb=(TW.BF, [(0, 64)], 0), lat=(TW.BF, [(0, 128)], 0))
        tasks.append(TW.Task("dyb", 0, 64, "lat", 0, 128))
    t128 = R.tiles([(t.N, t.K) for t in tasks], 128)
    assert t128 == 26 + int(fold)
    return TW.Case(f"pair-{M}-{int(fold)}", M, R.plan_msplit(t128, M), ops, tasks, False, M + 48 if planar else 0), planar


def launch_some(pr, idx, msplit, planar, flat):
    """TW.launch for the tasks `idx` of the problem at another row split, accumulating into `flat`."""
    sub = TW.Problem.__new__(TW.Problem)
    sub.__dict__.update(pr.__dict__)
    sub.c = pr.c._replace(tasks=[pr.c.tasks[i] for i in idx], msplit=msplit)
    sub.dW_off, sub.db_off, sub.flat0 = [pr.dW_off[i] for i in idx], [pr.db_off[i] for i in idx], flat
    res = TW.launch(sub, planar=planar)
    assert res.rc == 0
    return res.flat, TW.rule(sub.c)


@pytest.mark.parametrize("M,fold", [(333, False), (333, True), (2752, True), (2752, False)])
def test_paired_launch_against_one_launch_per_block(M, fold):
    """M = 333: ragged last chunk, row-major operands, 6 slices (the contiguous-parts workgroup map); M = 2752 = 86 x 32: planes,
    16 slices (whole XCD groups, dma3) against 32 per block."""
    c, planar = pair_case(M, fold)
    pr = TW.Problem(c)
    n = len(c.tasks)
    paired = TW.launch(pr, planar=planar)
    wW, wb = TW.check(pr, paired, tag="/paired")                          # within the bound of its own (path, P, S)
    groups = [list(range(0, 7)), list(range(7, 14))] + ([[14]] if fold else [])
    flat, rules = pr.flat0, {}
    for idx in groups:
        ms = R.plan_msplit(R.tiles([(c.tasks[i].N, c.tasks[i].K) for i in idx], 128), M)
        flat, rl = launch_some(pr, idx, ms, planar, flat)
        rules.update({i: rl for i in idx})
    assert torch.equal(TW.bits(flat)[~pr.valid], TW.bits(pr.flat0)[~pr.valid])
    path2, P2, S2 = TW.rule(c)
    if M == 2752:
        assert (path2, P2) == ("dma3", 16) and rules[0][:2] == ("dma3", 32)
    worst = 0.0
    a, b = paired.flat.double(), flat.double()
    for i, t in enumerate(c.tasks):
        dW64, db64, absW, absb, dW0, db0 = pr.ref[i]
        path1, P1, S1 = rules[i]
        b1, b2 = R.bound_dW(path1, P1, S1, absW, dW0), R.bound_dW(path2, P2, S2, absW, dW0)
        one = pr.dW_view(b, i)[:t.N, :t.K]
        two = pr.dW_view(a, i)[:t.N, :t.K]
        assert R.ratio(one, dW64, b1) <= 1.0
        worst = max(worst, R.ratio(two, one, b1 + b2))
        if t.bias:
            o = pr.db_off[i]
            c1, c2 = R.bound_db(path1, P1, S1, M, absb, db0), R.bound_db(path2, P2, S2, M, absb, db0)
            assert R.ratio(b[o:o + t.N], db64, c1) <= 1.0
            worst = max(worst, R.ratio(a[o:o + t.N], b[o:o + t.N], c1 + c2))
    print(f"RATIO pair-vs-single M={M} fold={fold}: {worst:.4f} (paired vs fp64: dW {wW:.4f} db {wb:.4f})")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ ranges and the arena
def raw_pass(m, bands, grid, cb, bucket, arena=None, nbytes=None):
    """hsimae_forward + hsimae_backward through the C ABI on the model's buffers; arena: (aligned pointer) instead of the pool's."""
    x, noise = inputs(bands)
    _, _, _, st = m._run_forward(x, 0.75, noise, grid, want_latent=False)
    lib, cfg, io_ = _lib.load(), m._config(), st["io"]
    stream = torch.cuda.current_stream().cuda_stream
    if arena is not None:
        io_.workspace, io_.workspace_bytes = arena, nbytes
        rc = lib.hsimae_forward(C.byref(cfg), C.byref(io_), stream)
        if rc:
            st.release()
            return rc, None
    scratch = torch.zeros_like(m._flat)
    io_.det_acc = None
    io_.bucket_stream = bucket
    rc = lib.hsimae_backward(C.byref(cfg), C.byref(io_), scratch.data_ptr(), cb, None, stream)
    torch.cuda.synchronize()
    st.release()
    return rc, scratch


@pytest.mark.parametrize("with_bucket", [False, True])
@pytest.mark.parametrize("s_depth,depth", DEPTHS)
def test_ranges_tile_the_gradient_buffer(s_depth, depth, with_bucket):
    m = make(48, s_depth, depth, False)
    grid = HSIMAE.grid_candidates(6, 9, 0.75)[0]
    got = []
    cb = _lib.BUCKET_CB(lambda stage, off, n, user: got.append((stage, off, n)))
    side = torch.cuda.Stream(device=DEV) if with_bucket else None
    rc, _ = raw_pass(m, 48, grid, cb, side.cuda_stream if side else None)
    assert rc == 0
    total = m._flat.numel()
    assert [s for s, _, _ in got] == list(range(len(got))) and all(n > 0 for _, _, n in got)
    spans = sorted((off, off + n) for _, off, n in got)
    assert spans[0][0] == 0 and spans[-1][1] == total, (spans[0], spans[-1], total)
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])), "a gap or an element reported twice"
    assert len(got) == 2 + 2 + 1 + depth - s_depth + 2 * s_depth          # pred / norm, 2 decoder blocks, norm | embed, blocks, patch_embed
    names = [n for n, _ in m.named_parameters() if not n.startswith("cls_head.")]          # (the flat buffer's order: HSIMAE._plist)
    first = {k: m._offs[names.index(k)] for k in ("blocks_1.0.norm1.weight", "blocks_2.0.norm1.weight", "blocks.0.norm1.weight")}
    assert first["blocks_1.0.norm1.weight"] < first["blocks_2.0.norm1.weight"] < first["blocks.0.norm1.weight"]
    lo2, hi2 = first["blocks_2.0.norm1.weight"], first["blocks.0.norm1.weight"]
    spectral = [off for _, off, _ in got if lo2 <= off < hi2]
    rest = [off for _, off, _ in got if not lo2 <= off < hi2]
    assert len(spectral) == s_depth
    assert spectral == sorted(spectral, reverse=True) and rest == sorted(rest, reverse=True), "a stack's ranges out of back-to-front order"
    if not with_bucket:
        offs = [off for _, off, _ in got]
        assert offs == sorted(offs, reverse=True)


def test_exact_arena():
    m = make(96, 3, 6, False)
    grid = HSIMAE.grid_candidates(12, 9, 0.75)[1]
    lib, cfg = _lib.load(), m._config()
    nbytes = lib.hsimae_workspace_bytes(C.byref(cfg), N, grid[0], grid[1])
    assert nbytes > 0 and nbytes % 256 == 0
    GUARD = 1 << 20
    buf = torch.zeros(nbytes + 256 + GUARD, dtype=torch.uint8, device=DEV)
    base = (buf.data_ptr() + 255) // 256 * 256
    lead = base - buf.data_ptr()
    buf[lead + nbytes:] = 0xA5
    none = _lib.BUCKET_CB(0)
    rc_ref, ref = raw_pass(m, 96, grid, none, None)
    rc, got = raw_pass(m, 96, grid, none, None, arena=base, nbytes=nbytes)
    assert rc_ref == 0 and rc == 0
    assert bool((buf[lead + nbytes:] == 0xA5).all()), "the pass wrote behind hsimae_workspace_bytes"
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    # the same pass in the pool's arena: two roundings of float-atomic sums, compared loosely here (the bounds are tested above)
    assert float((got.double() - ref.double()).norm() / ref.double().norm()) < 1e-3
    rc_small, _ = raw_pass(m, 96, grid, none, None, arena=base, nbytes=nbytes - 256)
    assert rc_small == -1                                                 # HSIMAE_EDIMS: the carve does not fit
