"""fp64 restatement and a derived error bound for csrc/ema.hip (tests/test_gpu_ema.py, tests/test_ema_bound_cpu.py): the moving
average of the weights that follows the optimizer step, and the exchange of weights and averages.

A plain module, not a conftest, in the manner of clip_ref.py.  The restatement is written from the formula in float64:

    t = step - skipped;   d = min(decay, (1 + t) / (10 + t)) with warm-up, decay without;   ema' = ema + (1 - d) (p - ema)

and nothing moves on a step that is not applied.  An output is accepted when |y - y64| <= err, and err is DERIVED from the sequence
include/hsimae_hip.h states (s = p - ema, one fp32 rounding; a = (float)(1 - d); ema' = fmaf(a, s, ema), one fp32 rounding); no
measured constant enters it.  With U = 2^-24 (half an ulp, relative), e the average the device holds and err its distance from the
restatement before the step:

  subtraction   |s - (p - e)| <= U |p - e|, and |p - e| <= |p - ema64| + err; it reaches the result times a
  a             1 - d and the quotient are fp64 (three roundings, 2^-53 each), then one fp32 rounding: |a32 - a| <= (U + 4 2^-53) a,
                which reaches the result times |p - e|
  fma           one rounding of the result: U |ema'|, and |ema'| <= |ema64'| + err'; where the result is denormal the rounding is
                absolute, at most half the smallest denormal, 2^-150 (an fp32 subtraction is exact there)
  propagated    the step maps an error of e to |1 - a| of it (p is an input: it carries none)

so  err' (1 - U) = |1 - a| err + (2 U + 4 2^-53) a (|p - ema64| + err) + U |ema64'| + 2^-150, summed over the steps taken.
An element whose p equals its average bit for bit is outside the bound's business: it must keep its bits (`kept`)."""
import numpy as np

U = 2.0 ** -24
E53 = 2.0 ** -53
TINY = 2.0 ** -150
GRID = 2048                                   # HSIMAE_EMA_MAX_GRID: workgroups of 256 threads, one float4 per thread and pass
N_TWICE = 4 * (GRID * 256 + 256 + 37) + 3     # the float4 loop runs twice for part of the grid, then a tail of 3
SMALL_N = [0, 1, 3, 4, 5, 7, 8, 255, 256, 257]


def f32bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def decay_at(decay, warmup, t):
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


class Average:
    """The restatement's state: `ref` (fp64), `err` (the bound so far, per element) and the count of skipped steps."""

    def __init__(self, ema0, skipped=0):
        self.ref = np.asarray(ema0, dtype=np.float32).astype(np.float64)
        self.err = np.zeros_like(self.ref)
        self.skipped = int(skipped)

    def step(self, p, decay, warmup, step, apply_=True):
        """One hsimae_ema_update at optimizer step `step`.  apply_ False: the step is skipped; it is counted and nothing moves."""
        if not apply_:
            self.skipped += 1
            return self
        t = step - self.skipped
        a = 1.0 - decay_at(decay, warmup, t)
        p = np.asarray(p, dtype=np.float32).astype(np.float64)
        new = self.ref + a * (p - self.ref)
        err = abs(1.0 - a) * self.err + (2 * U + 4 * E53) * a * (np.abs(p - self.ref) + self.err) + U * np.abs(new) + TINY
        self.ref, self.err = new, err / (1.0 - U)
        return self

    def ratio(self, got):
        """Worst |got - ref| / err; inf for a value that is not finite or is off where the bound is 0."""
        got = np.asarray(got, dtype=np.float32).astype(np.float64).reshape(self.ref.shape)
        if got.size == 0:
            return 0.0
        if not np.isfinite(got).all():
            return float("inf")
        d = np.abs(got - self.ref)
        if ((self.err <= 0) & (d > 0)).any():
            return float("inf")
        return float(np.max(np.where(d > 0, d / np.maximum(self.err, 1e-300), 0.0)))


def kept(before, p, after):
    """Every element whose p equals its average bit for bit has kept its bits (-0.0, denormals and NaN payloads included)."""
    b, q, a = f32bits(before), f32bits(p), f32bits(after)
    same = b == q
    return bool(np.array_equal(a[same], b[same]))


def swapped(a0, b0, a1, b1):
    """(a1, b1) is (b0, a0), bit for bit."""
    return bool(np.array_equal(f32bits(a1), f32bits(b0)) and np.array_equal(f32bits(b1), f32bits(a0)))


def inputs(n, seed, equal_every=5):
    """(ema, p) fp32: values of mixed sign and magnitude around 0.05, p a few per cent away from its average, and every
    `equal_every`-th element equal to it bit for bit."""
    rng = np.random.default_rng(seed)
    ema = (0.05 * rng.standard_normal(n) * np.exp(rng.standard_normal(n))).astype(np.float32)
    p = (ema.astype(np.float64) * (1.0 + 0.05 * rng.standard_normal(n)) + 1e-3 * rng.standard_normal(n)).astype(np.float32)
    if equal_every:
        p[::equal_every] = ema[::equal_every]
    return ema, p
