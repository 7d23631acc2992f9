"""hsimae_wgrad, launch path by launch path, against a float64 reference (tests/wgrad_ref.py) on a real MI355X.

hs_wgrad (csrc/wgrad.hip) picks one of five launch paths from the operands' types, alignment and sizes and from msplit: the
register-staged wgrad_kernel (`reg`), the LDS-DMA kernel on 128 x 128 tiles with a 6- or a 3-stage ring (`dma6`, `dma3`), the
same on 256 x 256 tiles committing with atomics (`big`) or through the slab and wgrad_slab_reduce_kernel (`big_slab`).
wgrad_ref.expected restates that rule; the first test proves that the cases below reach every path.

One helper builds every case.  Operand buffers are wider than their matrices and every padding column, every row past M and
every spare row / column of a planar operand holds NaN: the kernels may fetch padding, but nothing of it may reach a
committed element.  dW lives in a buffer with ldw = K + 8 and 3 guard rows, db between 8 guard floats on either side; guards
hold a finite sentinel (NaN cannot be a canary under atomicAdd) and must be bit-identical afterwards.  dW0 / db0 are random:
the contract is accumulate.  Every element is compared under the derived bound of wgrad_ref (never max-over-max); the worst
err / bound per case is printed ("RATIO ...", run with -s).

Worst err / bound seen on MI355X per path over two runs (float atomics: the order of the commits varies).  The bound is not
adjusted to them; the fp32 emulation of tests/test_wgrad_bound_cpu.py sits at the same 0.01 - 0.2:

    path       dW       db        at
    reg        0.200    0.193     M = 1 (one product per element); 0.16 / 0.009 at M = 45
    dma6       0.171    0.076     M = 45, msplit 3; planar operands 0.096 / 0.039
    dma3       0.034    0.019     the d = 128 block at M = 333, msplit 24 (dW), at M = 2733, msplit 17 (db)
    big        0.105    0.028     M = 200, P = 7; planar operands 0.082 / 0.028
    big_slab   0.076    0.028     M = 256, P = 8
    det        0.084    0.016     the d = 128 block at M = 333 with det_base / det_acc
"""
import ctypes as C
import functools
import os
import sys
from collections import namedtuple

import pytest
import torch

from hsimae_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, EDIMS, EUNSUP, ENULL = 0, -1, -2, -4
SENT = -7777.25                        # guard value of the output buffer
SLAB_SENT = 0x7FC12345                 # a NaN with a payload no kernel produces: "this float of the slab was never written"
SLAB_FLOATS = (64 + 1) * (1 << 20) // 4
BF, F32 = torch.bfloat16, torch.float32
RS = [0.0, 1.0, 1.0 / 0.9, 1.0 / 0.7, 1.3]       # DropPath factors: 0, 1 and non-powers of two

# one linear of a launch: dO = columns [doff, doff + N) of operand `dO`, A = columns [aoff, aoff + K) of operand `A`
Task = namedtuple("Task", "dO doff N A aoff K bias rs pd pa", defaults=(True, False, False, False))
# ops: name -> (dtype, [(first column, columns) of every valid range], elements the buffer starts past a 16-byte boundary)
Case = namedtuple("Case", "name M msplit ops tasks slab plane_rows", defaults=(False, 0))


def rup(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ the cases
def single(name, M, N, K, msplit, f32=False, slab=False, rs=False, lead=0):
    return Case(name, M, msplit, {"dO": (F32 if f32 else BF, [(0, N)], lead), "A": (BF, [(0, K)], 0)},
                [Task("dO", 0, N, "A", 0, K, True, rs)], slab)


def block(name, M, d, h, msplit, slab=False, planar=False):
    """One transformer block's seven linears as block_bwd (csrc/api.hip) builds them: q | k | v column slices of one dqkv slab
    over one A, w1 | w3 slices of one dh13 slab, w2 with K = h; the projection without a bias gradient (want_bias false)."""
    hp = rup(h, 64) if planar else rup(h, 32)
    ops = {"dqkv": (BF, [(0, d), (d, d), (2 * d, d)], 0), "u": (BF, [(0, d)], 0), "g1b": (BF, [(0, d)], 0), "o": (BF, [(0, d)], 0),
           "dh13": (BF, [(0, h), (hp, h)], 0), "u2": (BF, [(0, d)], 0), "g0b": (BF, [(0, d)], 0), "g": (BF, [(0, h)], 0)}
    tasks = [Task("dqkv", 0, d, "u", 0, d), Task("dqkv", d, d, "u", 0, d), Task("dqkv", 2 * d, d, "u", 0, d),
             Task("g1b", 0, d, "o", 0, d, False),
             Task("dh13", 0, h, "u2", 0, d, pd=planar), Task("dh13", hp, h, "u2", 0, d, pd=planar),
             Task("g0b", 0, d, "g", 0, h, pa=planar)]
    return Case(name, M, msplit, ops, tasks, slab, M + 48 if planar else 0)


def mlp3(name, M, d, h, msplit, slab=False):
    """w1 | w3 | w2 with dh1 | dh3 and g as 64-column planes of M + 48 rows (hsimae_backward's layout)."""
    b = block(name, M, d, h, msplit, slab, planar=True)
    return b._replace(ops={k: v for k, v in b.ops.items() if k in ("dh13", "u2", "g0b", "g")}, tasks=b.tasks[4:])


MIXED = Case("reg-mixed", 333, 2, {"dO": (F32, [(0, 72)], 0), "A": (BF, [(0, 64)], 0), "dOb": (BF, [(0, 136)], 0), "Ab": (BF, [(0, 72)], 0)},
             [Task("dO", 0, 72, "A", 0, 64), Task("dOb", 0, 136, "Ab", 0, 72)])
PLAN_MS = R.plan_msplit(13, 2733)                # the split hsimae_backward passes for the d = 128 block at M = 2733: 32

CASES = [
    # reg: one ragged 64-row chunk, M below one chunk with more slices than chunks, M = 1, DropPath factors, a bf16 dO 8 bytes off
    single("reg-45", 45, 72, 64, 3, f32=True),
    single("reg-333", 333, 136, 72, 2, f32=True),
    single("reg-1", 1, 128, 128, 1, f32=True),
    single("reg-rowscale", 333, 136, 72, 2, f32=True, rs=True),
    single("reg-unaligned", 333, 136, 72, 2, lead=4),
    MIXED,
    # dma6: nch <= 1 per slice and an empty slice; 3 x 2 ragged tiles, 20 chunks through the 6-stage ring; the msplit % 8 == 0 map
    single("dma6-45", 45, 72, 64, 3),
    single("dma6-610", 610, 344, 136, 1),
    single("dma6-1000", 1000, 128, 128, 8),
    block("dma6-block", 333, 128, 344, 3),
    # dma3: grid 16 * 17 = 272 (contiguous parts, 6 chunks through 3 stages), 13 * 24 = 312 (XCD groups), the planner's own split
    block("dma3-block-ms17", 2733, 128, 344, 17),
    block("dma3-block-ms24", 2733, 128, 344, 24),
    block("dma3-block-plan", 2733, 128, 344, PLAN_MS),
    block("dma3-block-short", 333, 128, 344, 24),        # one chunk per slice (fewer than the ring prefetches), 13 empty slices
    # big: P = 7 < 8 (a given slab is ignored); 2 x 2 ragged tiles; 3 k-tiles; the d = 256 block: 13 tiles, P = 19, 7 chunks per slice
    single("big-200", 200, 256, 256, 8, slab=True),
    single("big-333", 333, 344, 264, 8),
    single("big-1500", 1500, 256, 696, 8),
    block("big-block", 3685, 256, 680, 8),
    block("big-block-s3", 1800, 256, 680, 8),            # 3 chunks per slice: exactly what the 4-stage ring prefetches
    # big_slab: P = 8, 12, 11 (msplit % 4 = 3: the reduce's tail loop; ragged tiles in its index map), the block with P = 19
    single("slab-256", 256, 256, 256, 8, slab=True),
    single("slab-357", 357, 256, 256, 8, slab=True),
    single("slab-325", 325, 344, 264, 8, slab=True),
    block("slab-block", 3685, 256, 680, 8, slab=True),
    block("slab-block-empty", 640, 256, 680, 8, slab=True),      # 20 chunks over 19 slices: 2 each, 9 slices write zero tiles
]
PLANAR = [mlp3("planar-128", 320, 128, 344, 3), mlp3("planar-256", 320, 256, 680, 8), mlp3("planar-256-slab", 320, 256, 680, 8, slab=True)]
BY_NAME = {c.name: c for c in CASES + PLANAR}
PATH_OF = {"slab": "big_slab"}


def esize(dtype):
    return 4 if dtype == F32 else 2


def rule(c):
    """(path, P, S) wgrad_ref.expected gives for the case."""
    tasks = [(t.N, t.K, int(c.ops[t.dO][0] == F32)) for t in c.tasks]
    aligned = all(c.ops[k][2] == 0 for t in c.tasks for k in (t.dO, t.A)) and \
        all(t.doff * esize(c.ops[t.dO][0]) % 16 == 0 and t.aoff * 2 % 16 == 0 for t in c.tasks)
    return R.expected(tasks, c.M, c.msplit, c.slab, aligned)


def test_cases_reach_every_path():
    reached = {rule(c)[0] for c in CASES}
    assert reached == {"reg", "dma6", "dma3", "big", "big_slab"}, reached
    for c in CASES:                                       # every case runs on the path its name says
        head = c.name.split("-")[0]
        assert rule(c)[0] == PATH_OF.get(head, head), (c.name, rule(c))
    assert [rule(c)[0] for c in PLANAR] == ["dma6", "big", "big_slab"]
    # both workgroup maps of the 128-tile kernels, the reduce's tail loop, the short last XCD part
    assert rule(BY_NAME["dma3-block-ms17"])[1] % 8 and rule(BY_NAME["dma3-block-ms24"])[1] % 8 == 0 and PLAN_MS == 32
    assert rule(BY_NAME["slab-325"])[1] % 4 == 3 and rule(BY_NAME["slab-block"])[1:] == (19, 7) and rule(BY_NAME["big-200"])[1] == 7


# ------------------------------------------------------------------------------------------------ plumbing
def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.view(torch.int32)


class Operand:
    """Values [M, W] with NaN outside the valid column ranges; the row-major buffer [M + 2, ld] (ld > W, NaN in the pad columns
    and in the 2 rows past M, optionally starting `lead` elements past the allocation's 16-byte boundary) and, on demand, the
    planar image [W64 / 64][R][64] with NaN in the spare rows and spare columns."""

    def __init__(self, M, dtype, segs, lead, seed):
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.M, self.dtype, self.f32 = M, dtype, dtype == F32
        self.W = max(o + n for o, n in segs)
        self.ld = rup(self.W, 32) + 32
        vals = torch.full((M, self.W), float("nan"), device=DEV)
        for o, n in segs:
            vals[:, o:o + n] = torch.randn(M, n, device=DEV, generator=g) * 0.5 + 0.05
        self.raw = torch.full((lead + (M + 2) * self.ld,), float("nan"), dtype=dtype, device=DEV)
        self.rows = self.raw[lead:].view(M + 2, self.ld)
        self.rows[:M, :self.W] = vals.to(dtype)
        self._planar = {}

    def ptr(self, off):
        return self.rows.data_ptr() + off * esize(self.dtype)

    def values(self, off, n):
        return self.rows[:self.M, off:off + n]

    def planar(self, R_):
        if R_ not in self._planar:
            W64 = rup(self.W, 64)
            img = torch.full((W64 // 64, R_, 64), float("nan"), dtype=self.dtype, device=DEV)
            wide = torch.full((self.M, W64), float("nan"), dtype=self.dtype, device=DEV)
            wide[:, :self.W] = self.rows[:self.M, :self.W]
            img[:, :self.M, :] = wide.view(self.M, W64 // 64, 64).permute(1, 0, 2)
            self._planar[R_] = img
        return self._planar[R_]

    def with_value(self, m, col, v):
        """A copy with one element replaced (NaN / Inf containment)."""
        o = object.__new__(Operand)
        o.__dict__.update(self.__dict__)
        o.raw = self.raw.clone()
        o.rows = o.raw[self.raw.numel() - (self.M + 2) * self.ld:].view(self.M + 2, self.ld)
        o.rows[m, col] = v
        o._planar = {}
        return o


class Problem:
    """Operands, initial outputs and the float64 reference of one case; built once, shared, never modified."""

    def __init__(self, c):
        self.c = c
        self.ops = {k: Operand(c.M, dt, segs, lead, seed=1000 + 7 * i) for i, (k, (dt, segs, lead)) in enumerate(sorted(c.ops.items()))}
        g = torch.Generator(device=DEV).manual_seed(5)
        self.rs = torch.tensor(RS, device=DEV)[torch.arange(c.M, device=DEV) % len(RS)].contiguous()
        off, self.dW_off, self.db_off = 8, [], []
        for t in c.tasks:
            self.dW_off.append(off)
            off += (t.N + 3) * (t.K + 8)
            self.db_off.append(off + 8)
            off += t.N + 16
        flat = torch.full((off + 8,), SENT, device=DEV)
        self.valid = torch.zeros(off + 8, dtype=torch.bool, device=DEV)
        self.ref = []
        for i, t in enumerate(c.tasks):
            dW0 = torch.randn(t.N, t.K, device=DEV, generator=g)
            self.dW_view(flat, i)[:t.N, :t.K] = dW0
            self.dW_view(self.valid, i)[:t.N, :t.K] = True
            db0 = None
            if t.bias:
                db0 = torch.randn(t.N, device=DEV, generator=g)
                flat[self.db_off[i]:self.db_off[i] + t.N] = db0
                self.valid[self.db_off[i]:self.db_off[i] + t.N] = True
            dW64, db64, absW, absb = R.ref64(self.ops[t.dO].values(t.doff, t.N), self.ops[t.A].values(t.aoff, t.K), t.N, t.K, dW0, db0,
                                             self.rs if t.rs else None)
            assert bool(torch.isfinite(dW64).all() and torch.isfinite(db64).all())
            self.ref.append((dW64, db64, absW, absb, dW0, db0))
        self.flat0 = flat

    def dW_view(self, flat, i):
        t = self.c.tasks[i]
        return flat[self.dW_off[i]:self.dW_off[i] + (t.N + 3) * (t.K + 8)].view(t.N + 3, t.K + 8)


@functools.lru_cache(maxsize=None)
def problem(name):
    return Problem(BY_NAME[name])


@functools.lru_cache(maxsize=None)
def _slab():
    return torch.empty(SLAB_FLOATS, dtype=torch.int32, device=DEV)


def fresh_slab():
    """64 MiB + 1 MiB of SLAB_SENT."""
    s = _slab()
    s.fill_(SLAB_SENT)
    return s


@functools.lru_cache(maxsize=None)
def slab_reserved():
    """Bytes of slab hsimae_workspace_bytes reserves for a stream that can run a 256 x 256-tile launch (d = 256): 64 MiB."""
    from hsimae_amd import swiglu_hidden
    cfg = _lib.Config(bands=96, embed_dim=256, depth=12, s_depth=9, num_heads=16, dec_dim=64, dec_depth=8, dec_heads=8,
                      hidden=swiglu_hidden(256, 4.0), dec_hidden=swiglu_hidden(64, 4.0), norm_pix_loss=1)
    n = _lib.load().hsimae_wgrad_slab_bytes(C.byref(cfg), 1)
    assert n == 64 << 20
    return n


Result = namedtuple("Result", "rc flat acc slab")


def launch(pr, det=False, planar=False, override=None, rs=None):
    """One hsimae_wgrad call of the case on a fresh copy of its outputs.  override: operands replaced for this call; rs: other
    row factors; planar: the tasks marked pd / pa pass their operand as planes."""
    c = pr.c
    rs = pr.rs if rs is None else rs
    lib = _lib.load()
    ops = dict(pr.ops, **(override or {}))
    flat = pr.flat0.clone()
    acc = torch.zeros(flat.numel(), dtype=torch.int64, device=DEV) if det else None
    sl = fresh_slab() if c.slab else None
    wp = _lib.WgradParams()
    Rr = c.plane_rows
    aligned = True
    for i, t in enumerate(c.tasks):
        d, a = ops[t.dO], ops[t.A]
        if planar and t.pd:
            dptr, ldo, dpr = d.planar(Rr).data_ptr() + 2 * t.doff * Rr, rup(t.N, 64), Rr
        else:
            dptr, ldo, dpr = d.ptr(t.doff), d.ld, 0
        if planar and t.pa:
            aptr, lda, apr = a.planar(Rr).data_ptr() + 2 * t.aoff * Rr, rup(t.K, 64), Rr
        else:
            aptr, lda, apr = a.ptr(t.aoff), a.ld, 0
        aligned = aligned and (dptr | aptr) & 15 == 0
        wp.t[i] = _lib.WgradTask(dO=dptr, dO_f32=int(d.f32), ldo=ldo, A=aptr, lda=lda, N=t.N, K=t.K,
                                 dW=flat.data_ptr() + 4 * pr.dW_off[i], ldw=t.K + 8,
                                 db=flat.data_ptr() + 4 * pr.db_off[i] if t.bias else None,
                                 dO_rowscale=rs.data_ptr() if t.rs else None, dO_plane_rows=dpr, A_plane_rows=apr)
    assert aligned == (rule(c)[0] != "reg" or any(pr.ops[t.dO].f32 for t in c.tasks)), "the buffers' alignment is not the case's"
    wp.ntasks, wp.M, wp.msplit = len(c.tasks), c.M, c.msplit
    if det:
        wp.det_base, wp.det_acc = flat.data_ptr(), acc.data_ptr()
    if sl is not None:
        wp.slab = sl.data_ptr()
    rc = lib.hsimae_wgrad(C.byref(wp), stream())
    torch.cuda.synchronize()
    return Result(rc, flat, acc, sl)


def check(pr, res, det=False, poisoned=None, tag=""):
    """Every committed element within the bound, every other float of the output buffer bit-intact; the slab written exactly
    where the rule says.  poisoned = (task, n): row n of that task's dW and its db[n] are expected non-finite and left out."""
    c = pr.c
    path, P, S = rule(c)
    assert res.rc == OK, f"hsimae_wgrad returned {res.rc}"
    out = res.flat.double()
    if det:
        out = out + res.acc.double() * R.DET_ULP               # what the library's conversion pass does
        assert bool((res.acc[~pr.valid] == 0).all()), "det_acc written outside the tasks' ranges"
    assert torch.equal(bits(res.flat)[~pr.valid], bits(pr.flat0)[~pr.valid]), "a guard / pad element of dW or db was written"
    slab_dW = path == "big_slab"                             # dW through the slab: fp32 adds, also under det
    worst_W = worst_b = 0.0
    for i, t in enumerate(c.tasks):
        dW64, db64, absW, absb, dW0, db0 = pr.ref[i]
        dW = pr.dW_view(out, i)[:t.N, :t.K]
        keep = torch.ones(t.N, dtype=torch.bool, device=DEV)
        if poisoned is not None and poisoned[0] == i:
            keep[poisoned[1]] = False
        bW = R.bound_dW(path, P, S, absW, dW0, det and not slab_dW)
        worst_W = max(worst_W, R.ratio(dW[keep], dW64[keep], bW[keep]))
        if det:
            fW, aW = pr.dW_view(res.flat, i)[:t.N, :t.K][keep], pr.dW_view(res.acc, i)[:t.N, :t.K][keep]
            if slab_dW:
                assert bool((aW == 0).all()), "slab + det: dW belongs in fp32"
            else:
                assert torch.equal(fW, dW0[keep]), "det: dW belongs in the fixed-point shadow"
        if t.bias:
            o = pr.db_off[i]
            bb = R.bound_db(path, P, S, c.M, absb, db0, det)
            worst_b = max(worst_b, R.ratio(out[o:o + t.N][keep], db64[keep], bb[keep]))
            if det:
                assert torch.equal(res.flat[o:o + t.N][keep], db0[keep]), "det: db belongs in the fixed-point shadow"
    print(f"RATIO {c.name + tag:<28s} {path:<8s} P={P:<3d} S={S:<3d} dW={worst_W:.4f} db={worst_b:.4f}")
    assert worst_W <= 1.0 and worst_b <= 1.0, (c.name, worst_W, worst_b)
    if res.slab is not None:
        n = P * R.tiles([(t.N, t.K) for t in c.tasks], 256) * 128 * 512 if slab_dW else 0
        assert 4 * n <= slab_reserved()
        assert bool((res.slab[:n] != SLAB_SENT).all()), "the slab path did not write all of its partial tiles"
        assert bool((res.slab[n:] == SLAB_SENT).all()), "the slab was written past P * tiles * 128 * 512 floats"
        if slab_dW and all(t.N % 256 == 0 and t.K % 256 == 0 for t in c.tasks):
            # whole tiles only: every partial sum is a number.  (A ragged tile's partial rows / columns past N / K are sums over
            # the NaN padding; they sit in the slab and are never added into dW, which the ratios above prove.)
            assert bool(torch.isfinite(res.slab[:n].view(torch.float32)).all())
    return worst_W, worst_b


def dW_mask(pr):
    """True on the committed elements of every task's dW (not db: the bias sums always meet through atomics)."""
    m = torch.zeros_like(pr.valid)
    for i, t in enumerate(pr.c.tasks):
        pr.dW_view(m, i)[:t.N, :t.K] = True
    return m


# ------------------------------------------------------------------------------------------------ the matrix
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_wgrad_path(name):
    pr = problem(name)
    res = launch(pr)
    check(pr, res)
    if rule(pr.c)[0] == "big_slab":                          # no float atomics on dW: the same bits again
        again = launch(pr)
        assert torch.equal(bits(res.flat)[dW_mask(pr)], bits(again.flat)[dW_mask(pr)])


def test_row_factor_zero_drops_the_row():
    """dO_rowscale 0 on every row: dW and db keep exactly what they held (0 * dO is 0, not skipped arithmetic gone wrong)."""
    pr = problem("reg-rowscale")
    res = launch(pr, rs=torch.zeros_like(pr.rs))
    assert res.rc == OK and torch.equal(bits(res.flat), bits(pr.flat0))


@pytest.mark.parametrize("name", [c.name for c in PLANAR])
def test_planar_operands(name):
    """dh1 | dh3 and g as 64-column planes of M + 48 rows: the same dW / db as the row-major launch, both within the bound."""
    pr = problem(name)
    rows = launch(pr)
    planes = launch(pr, planar=True)
    check(pr, rows, tag="/rows")
    check(pr, planes, tag="/planes")
    path, P, S = rule(pr.c)
    for i, t in enumerate(pr.c.tasks):
        dW64, db64, absW, absb, dW0, db0 = pr.ref[i]
        a, b = pr.dW_view(rows.flat, i)[:t.N, :t.K], pr.dW_view(planes.flat, i)[:t.N, :t.K]
        assert R.ratio(a, b.double(), 2 * R.bound_dW(path, P, S, absW, dW0)) <= 1
    if path == "big_slab":
        assert torch.equal(bits(rows.flat)[dW_mask(pr)], bits(planes.flat)[dW_mask(pr)])      # same products, same fixed order


# ------------------------------------------------------------------------------------------------ deterministic commits
DET = ["reg-333", "dma6-block", "big-333", "slab-block"]
POISON = ["reg-333", "dma6-610", "big-333", "slab-325"]


@pytest.mark.parametrize("name", DET)
def test_deterministic_commits(name):
    """det_base / det_acc: within the bound plus the fixed-point term, bit-identical on a second run, nothing outside the tasks'
    ranges; with the slab, dW arrives in fp32 and db in the shadow (what block_bwd passes)."""
    pr = problem(name)
    first = launch(pr, det=True)
    check(pr, first, det=True, tag="/det")
    second = launch(pr, det=True)
    assert torch.equal(bits(first.flat), bits(second.flat)) and torch.equal(first.acc, second.acc)


def poison_site(pr):
    t = pr.c.tasks[0]
    return pr.c.M // 2 + 1, t.N - 3            # a row in the middle, a column of the last (ragged) n-tile


@pytest.mark.parametrize("name", POISON)
def test_deterministic_commits_keep_a_non_finite_addend(name):
    """One +inf in dO[m, n]: row n of dW and db[n] come out NaN (hs_gadd poisons the fp32 slot; through the slab the fp32 sum is
    +-inf or NaN by itself), every other element is still within the bound."""
    pr = problem(name)
    m, n = poison_site(pr)
    res = launch(pr, det=True, override={"dO": pr.ops["dO"].with_value(m, n, float("inf"))})
    check(pr, res, det=True, poisoned=(0, n), tag="/det+inf")
    t = pr.c.tasks[0]
    out = res.flat.double() + res.acc.double() * R.DET_ULP
    row = pr.dW_view(out, 0)[n, :t.K]
    if rule(pr.c)[0] == "big_slab":
        assert bool((~torch.isfinite(row)).all())
    else:
        assert bool(row.isnan().all())
    assert bool(out[pr.db_off[0] + n].isnan())


@pytest.mark.parametrize("name", ["dma6-610", "big-333"])
def test_nan_stays_in_its_row(name):
    """One NaN in a valid dO[m, n], float atomics: exactly row n of dW and db[n] are NaN."""
    pr = problem(name)
    m, n = poison_site(pr)
    res = launch(pr, override={"dO": pr.ops["dO"].with_value(m, n, float("nan"))})
    check(pr, res, poisoned=(0, n), tag="/nan")
    t = pr.c.tasks[0]
    assert bool(pr.dW_view(res.flat, 0)[n, :t.K].isnan().all()) and bool(res.flat[pr.db_off[0] + n].isnan())


# ------------------------------------------------------------------------------------------------ the planner's row split
def test_planner_msplit_is_covered():
    """hsimae_wgrad_msplit for the block batches above: the range test_plan_asan_cpu.py asserts, whole XCD groups from 8 up, and
    the value the case dma3-block-plan runs with."""
    lib = _lib.load()
    for tiles, M in ((13, 333), (13, 2733), (52, 3685)):
        ms = lib.hsimae_wgrad_msplit(tiles, M)
        assert 1 <= ms <= max(1, (M + 63) // 64), (tiles, M, ms)
        assert ms < 8 or ms % 8 == 0, (tiles, M, ms)
        assert ms == R.plan_msplit(tiles, M), (tiles, M, ms)
    c = BY_NAME["dma3-block-plan"]
    assert R.tiles([(t.N, t.K) for t in c.tasks], 128) == 13 and c.msplit == lib.hsimae_wgrad_msplit(13, c.M)
    assert R.tiles([(t.N, t.K) for t in BY_NAME["big-block"].tasks], 128) == 52


# ------------------------------------------------------------------------------------------------ refusals and no-ops
def _refusal_params(M=64):
    """A valid one-task launch (64 rows, 128 x 128, bf16) over buffers large enough for every variation below."""
    dO = torch.zeros(4 + 66 * 256, device=DEV)                  # fp32: also large enough read as bf16
    A = torch.zeros(66 * 256, dtype=BF, device=DEV)
    out = torch.full((131 * 136 + 160,), SENT, device=DEV)
    rs = torch.ones(M, device=DEV)
    wp = _lib.WgradParams()
    wp.t[0] = _lib.WgradTask(dO=dO.data_ptr(), dO_f32=0, ldo=128, A=A.data_ptr(), lda=128, N=128, K=128, dW=out.data_ptr() + 32,
                             ldw=136, db=out.data_ptr() + 4 * (131 * 136 + 16))
    wp.ntasks, wp.M, wp.msplit = 1, M, 2
    return wp, (dO, A, out, rs)


def _set(**kw):
    def f(wp, bufs):
        for k, v in kw.items():
            if k in ("ntasks", "M", "msplit"):
                setattr(wp, k, v)
            else:
                setattr(wp.t[0], k, v)
    return f


def _bump_dO(wp, bufs):
    wp.t[0].dO = bufs[0].data_ptr() + 8


def _rowscale(wp, bufs):
    wp.t[0].dO_rowscale = bufs[3].data_ptr()


REFUSALS = [
    ("ntasks-17", _set(ntasks=17), EDIMS),
    ("msplit-0", _set(msplit=0), EDIMS),
    ("ldo%8", _set(ldo=132), EDIMS),
    ("lda%8", _set(lda=132), EDIMS),
    ("planar-f32-dO", _set(dO_plane_rows=64, dO_f32=1), EDIMS),
    ("planar-dO-M%32", _set(dO_plane_rows=64, M=40), EDIMS),
    ("planar-A-M%32", _set(A_plane_rows=64, M=40), EDIMS),
    ("planar-dO-rows<M", _set(dO_plane_rows=32), EDIMS),
    ("planar-A-rows<M", _set(A_plane_rows=32), EDIMS),
    ("planar-dO-ld%64", _set(dO_plane_rows=64, ldo=160), EDIMS),
    ("planar-A-ld%64", _set(A_plane_rows=64, lda=160), EDIMS),
    ("planar-misaligned", lambda wp, b: (_set(dO_plane_rows=64)(wp, b), _bump_dO(wp, b)), EUNSUP),
    ("rowscale-bf16-dO", _rowscale, EUNSUP),
    ("rowscale-bf16-dO-misaligned", lambda wp, b: (_rowscale(wp, b), _bump_dO(wp, b)), EUNSUP),
    ("ntasks-0", _set(ntasks=0), OK),
    ("M-0", _set(M=0), OK),
]


@pytest.mark.parametrize("rid,change,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_and_no_ops(rid, change, code):
    wp, bufs = _refusal_params()
    change(wp, bufs)
    rc = _lib.load().hsimae_wgrad(C.byref(wp), stream())
    torch.cuda.synchronize()
    assert rc == code, f"{rid}: hsimae_wgrad returned {rc}, expected {code}"
    assert bool((bufs[2] == SENT).all()), f"{rid}: an output was written"


def test_null_params():
    assert _lib.load().hsimae_wgrad(None, stream()) == ENULL
