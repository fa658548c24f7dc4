"""rt_grad_sqnorm and rt_clip_adam_step (csrc/optim.hip) against numpy fp64,
called through the C ABI on synthetic slabs, and FusedTrainStep's Adam moments
against the oracle.

The Adam reference takes the hyperparameters as the ABI carries them
(``float(np.float32(x))``: the kernel is Adam with beta2 = float32(0.999)
throughout) and the fp32 arrays widened; the tolerance is per element and counts
the fp32 roundings of each expression of the kernel's chain (``adam_ref``), so
it holds whichever ``a + b*c`` the compiler contracts. There is no allowance for
outliers. ``test_bound_self_test_cpu`` checks the bound without a GPU against two
numpy-fp32 emulations of the chain and against emulations with a fault planted.
"""
import functools
import math

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

E = 2.0 ** -23
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
GUARD = 64          # elements allocated past n, which no launch may touch
F32 = np.float32


def hp(x):
    """A hyperparameter as the C ABI carries it."""
    return float(np.float32(x))


# ---------------------------------------------------------------------------
# fp64 references
# ---------------------------------------------------------------------------
def clip_coef(sumsq, max_norm):
    """clip_grad_norm_'s factor, fp64, from fp64 per-tensor sums: the norm is
    rounded to fp32 as the kernel holds it; a NaN norm gives NaN (torch.clamp
    keeps it), an infinite one gives 0."""
    with np.errstate(over="ignore", invalid="ignore"):
        total = float(np.float32(np.sqrt(np.sum(np.asarray(sumsq, dtype=np.float64)))))
        c = hp(max_norm) / (total + 1e-6)
    return 1.0 if c > 1.0 else c


def adam_ref(p, g, m, v, coef, step, lr=LR, wd=0.0, b1=B1, b2=B2, eps=EPS, bound=True):
    """One clip + Adam step in fp64 and its per-element fp32 rounding bound.
    Returns ((p1, m1, v1), (tp, tm, tv)); the bound is None when not asked for."""
    p, g, m, v = (np.asarray(x).astype(np.float64) for x in (p, g, m, v))
    lr, wd, b1, b2, eps = hp(lr), hp(wd), hp(b1), hp(b2), hp(eps)
    step = int(step)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        gv = g * coef + wd * p
        m1 = m + (1 - b1) * (gv - m)
        v1 = b2 * v + (1 - b2) * gv * gv
        rbc2 = math.sqrt(1 - b2 ** step)
        den = np.sqrt(v1) / rbc2 + eps
        ss = lr / (1 - b1 ** step)
        upd = ss * m1 / den
        p1 = p - upd
        if not bound:
            return (p1, m1, v1), None
        tg = 8 * E * np.abs(g) * coef + 4 * E * np.abs(wd * p)   # 8: the three fp32 roundings inside the kernel's coef
        tm = (1 - b1) * tg + 4 * E * (np.abs(m) + np.abs(gv))
        tv = (1 - b2) * (2 * np.abs(gv) * tg + tg * tg) + 4 * E * v1
        ts = np.where(v1 == 0, np.sqrt(tv), np.minimum(tv / (2 * np.sqrt(v1)), np.sqrt(tv)))
        td = ts / rbc2 + 4 * E * den
        tp = 2 * E * np.abs(p) + ss * (tm / den + np.abs(m1) * td / (den * den)) + 4 * E * np.abs(upd)
    return (p1, m1, v1), (tp, tm, tv)


def bound_ratios(got, ref, tol):
    """max |got - ref| / tol per array (p, m, v) where the reference is finite;
    NaN positions must agree exactly. An element with tol == 0 must be exact."""
    out = []
    for name, a, r, t in zip("pmv", got, ref, tol):
        a = np.asarray(a).astype(np.float64)
        nan = np.isnan(r)
        assert np.array_equal(np.isnan(a), nan), f"{name}: NaN positions differ"
        err = np.abs(a - r)[~nan]
        t = t[~nan]
        exact = t == 0
        assert not np.any(err[exact] != 0), f"{name}: inexact where the bound is zero"
        out.append(float(np.max(err[~exact] / t[~exact])) if np.any(~exact) else 0.0)
    return out


def assert_within_bound(got, ref, tol, what):
    ratios = bound_ratios(got, ref, tol)
    print(f"optim-bound {what}: err/tol p={ratios[0]:.3f} m={ratios[1]:.3f} v={ratios[2]:.3f}")
    assert max(ratios) <= 1.0, (what, ratios)
    return ratios


# ---------------------------------------------------------------------------
# numpy-fp32 emulations of the kernel's chain (the bound's self-test)
# ---------------------------------------------------------------------------
def _fma(a, b, c):
    # the fp32 product is exact in fp64; one fp64 and one fp32 rounding of the sum
    return (a.astype(np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F32)


def adam_emulated(p, g, m, v, sumsq, max_norm, step, lr=LR, wd=0.0, b1=B1, b2=B2, eps=EPS, fused=False, fault=None):
    """clip_adam_kernel's arithmetic in numpy fp32, op by op (``fused``: with the
    contractions the compiler may make). ``fault`` plants one error."""
    lr, wd, b1, b2, eps, max_norm = (F32(x) for x in (lr, wd, b1, b2, eps, max_norm))
    one = F32(1)
    total = F32(np.sqrt(np.sum(np.asarray(sumsq, dtype=np.float64))))
    coef = max_norm / (total + F32(1e-6))
    coef = one if coef > one else coef
    if fault == "coef":
        coef = F32(coef * F32(1 + 1e-4))
    st = step - 1 if fault == "step" else step
    step_size = F32(float(lr) / (1.0 - float(b1) ** st))
    bc2 = 1.0 - float(b2) ** st
    bc2s = F32(bc2 if fault == "bc2" else math.sqrt(bc2))
    w1, w2 = one - b1, one - b2
    if fault == "swap":
        w1, w2 = w2, w1
    gv = g * coef
    if wd != 0 and fault != "wd":
        gv = _fma(p, wd, gv) if fused else gv + wd * p
    if fused:
        mv = _fma(gv - m, w1, m)
        vv = _fma(w2 * gv, gv, v * b2)
    else:
        mv = m + w1 * (gv - m)
        vv = v * b2 + w2 * gv * gv
    denom = np.sqrt(vv + eps) / bc2s if fault == "eps" else np.sqrt(vv) / bc2s + eps
    q = mv / denom
    pn = _fma(q, -step_size, p) if fused else p - step_size * q
    return pn.astype(F32), mv.astype(F32), vv.astype(F32)


# ---------------------------------------------------------------------------
# synthetic state
# ---------------------------------------------------------------------------
N_MAX = 3 * 262144 + 5
SIZES = [1, 255, 256, 257, 262144, 262145, 262144 + 257, N_MAX]


def draw_grads(rng, n):
    return (rng.standard_normal(n) * np.exp(rng.uniform(-14.0, 1.0, n))).astype(F32)


def shape_grads(g, p, wd, coef, phase=2):
    """The test step's gradients: every third element zero, every seventh
    cancelling the weight decay term to 1e-6 of itself (gv ~ 0)."""
    g = g.copy()
    n = g.size
    idx = np.arange(3, n, 7)
    sign = np.where(idx % 2 == 0, 1.0, -1.0)
    if coef > 0 and math.isfinite(coef):
        g[idx] = (-hp(wd) * p[idx].astype(np.float64) * (1 + 1e-6 * sign) / coef).astype(F32)
    g[phase % 3::3] = 0
    return g


@functools.lru_cache(maxsize=None)
def _states():
    """(fresh, warm) states of N_MAX elements, computed once and read-only:
    fresh is m = v = 0 before step 1; warm is 30 reference steps (fp64 chain,
    state rounded to fp32 after every step) before step 31. Smaller cases take
    a prefix: the update is element-wise."""
    rng = np.random.default_rng(20240531)
    p0 = (0.1 * rng.standard_normal(N_MAX)).astype(F32)
    zeros = np.zeros(N_MAX, dtype=F32)
    p, m, v = p0, zeros, zeros
    for step in range(1, 31):
        g = draw_grads(rng, N_MAX)
        if step % 2:
            g[2::3] = 0
        (p, m, v), _ = adam_ref(p, g, m, v, 1.0, step, wd=1e-5, bound=False)
        p, m, v = (x.astype(F32) for x in (p, m, v))
    g_test = draw_grads(rng, N_MAX)
    out = {"fresh": (p0, zeros, zeros, 1), "warm": (p, m, v, 31), "g": g_test}
    for k in ("fresh", "warm"):
        for a in out[k][:3]:
            a.setflags(write=False)
    g_test.setflags(write=False)
    return out


def state(kind, n):
    s = _states()
    p, m, v, step = s[kind]
    return p[:n], m[:n], v[:n], step, s["g"][:n]


def split_sumsq(total, n_tensors):
    """``total`` (a power of two) spread over 1, 64, 65 or 130 slots so that
    every partial sum is exact in fp64: the order of the sum cannot matter."""
    if n_tensors == 1:
        s = [total]
    elif n_tensors == 64:
        s = [total / 64] * 64
    elif n_tensors == 65:
        s = [total / 64] * 63 + [total / 128] * 2
    else:
        assert n_tensors == 130
        s = [total / 128] * 126 + [total / 256] * 4
    s = np.array(s, dtype=np.float64)
    assert s.size == n_tensors and float(np.sum(s)) == total and float(np.sum(s[::-1])) == total
    return s


def clip_sumsq(kind, max_norm):
    """Total Σg² for a clip case (powers of two times max_norm²)."""
    return {"clipped": 128.0 * max_norm * max_norm,    # norm 11.3·max_norm: coef 0.088
            "below": 0.25 * max_norm * max_norm,       # norm max_norm / 2: coef clamps to 1
            "zero": 0.0}[kind]                         # coef = max_norm / 1e-6: clamps to 1


# ---------------------------------------------------------------------------
# the bound, without a GPU
# ---------------------------------------------------------------------------
# planted faults and the least share of elements (p, m or v) each must push out of
# the bound at a warm state. At wd = 0, 1/7 of the elements never see a gradient
# and a third have none in the tested step, where a wrong clip factor cannot show;
# eps inside the root shows only where exp_avg_sq is small.
FAULTS = [("step", 0.8), ("bc2", 0.8), ("swap", 0.8), ("eps", 0.25), ("coef", 0.2), ("wd", 0.5)]


@pytest.mark.parametrize("wd", [0.0, 1e-5, 1e-2])
def test_bound_self_test_cpu(wd):
    """31 steps of the two fp32 emulations, each step checked against the fp64
    reference taken from the emulation's own previous state: the bound holds
    with room. At the warm state (step 31) each planted fault leaves it."""
    n = 20000
    rng = np.random.default_rng(7)
    worst = [0.0, 0.0, 0.0]
    for fused in (False, True):
        p = (0.1 * rng.standard_normal(n)).astype(F32)
        m = np.zeros(n, dtype=F32)
        v = np.zeros(n, dtype=F32)
        for step in range(1, 32):
            max_norm = (1.0, 0.25)[step % 2]
            sumsq = split_sumsq(clip_sumsq(("clipped", "below", "zero")[step % 3], max_norm), (1, 65, 130)[step % 3])
            coef = clip_coef(sumsq, max_norm)
            g = shape_grads(draw_grads(rng, n), p, wd, coef, phase=step)
            if step % 3 == 2:
                g[:] = 0
            ref, tol = adam_ref(p, g, m, v, coef, step, wd=wd)
            got = adam_emulated(p, g, m, v, sumsq, max_norm, step, wd=wd, fused=fused)
            worst = [max(a, b) for a, b in zip(worst, bound_ratios(got, ref, tol))]
            if step == 31:
                for fault, least in FAULTS:
                    if fault == "wd" and wd != 1e-2:
                        continue
                    bad = adam_emulated(p, g, m, v, sumsq, max_norm, step, wd=wd, fused=fused, fault=fault)
                    outside = np.zeros(n, dtype=bool)
                    for b, r, t in zip(bad, ref, tol):
                        outside |= np.abs(b.astype(np.float64) - r) > t
                    print(f"optim-bound fault {fault} wd={wd} fused={fused}: {outside.mean():.3f} outside")
                    assert outside.mean() >= least, (fault, outside.mean())
            p, m, v = got
    print(f"optim-bound emulation wd={wd}: err/tol p={worst[0]:.3f} m={worst[1]:.3f} v={worst[2]:.3f}")
    assert max(worst) <= 0.5, worst       # a correct chain keeps 2x room or more


def test_clip_coef_and_split_helpers_cpu():
    assert clip_coef([0.0], 1.0) == 1.0 and clip_coef([0.01], 1.0) == 1.0
    assert abs(clip_coef([100.0], 1.0) - 0.1) < 1e-7
    assert math.isnan(clip_coef([1.0, float("nan")], 1.0)) and clip_coef([1.0, float("inf")], 1.0) == 0.0
    for t in (1, 64, 65, 130):
        split_sumsq(128.0, t)


# ---------------------------------------------------------------------------
# GPU plumbing
# ---------------------------------------------------------------------------
def _guarded(a, dev, fill):
    """``a`` on the device with GUARD extra elements holding a pattern."""
    full = np.concatenate([a, (fill + np.arange(GUARD)).astype(a.dtype)])
    return torch.from_numpy(full).to(dev)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


class Slabs:
    """p, g, m, v of n elements (+ guards) on the device."""

    def __init__(self, dev, p, g, m, v):
        self.n = p.size
        self.host = [np.ascontiguousarray(x, dtype=F32) for x in (p, g, m, v)]
        self.t = [_guarded(x, dev, f) for x, f in zip(self.host, (1234.5, -77.25, 3.0e4, 0.0625))]

    def step(self, sumsq, max_norm, step, lr=LR, wd=0.0, lr_dev=None, step_dev=None, zero_buf=None, zero_words=0,
             n_tensors=None):
        from rtrec_amd import native
        p, g, m, v = self.t
        n_tensors = sumsq.numel() if n_tensors is None else n_tensors
        native.call("rt_clip_adam_step", native.ptr(p), native.ptr(g), native.ptr(m), native.ptr(v), self.n,
                    native.ptr(sumsq), n_tensors, max_norm, lr, native.ptr(lr_dev), B1, B2, EPS, wd, step,
                    native.ptr(step_dev), native.ptr(zero_buf), zero_words, native.stream_of(p))
        torch.cuda.synchronize()

    def read(self):
        """(p, m, v) after a step; asserts the consumed-gradient contract and the guards."""
        out = [x.cpu().numpy() for x in self.t]
        for x, f in zip(out, (1234.5, -77.25, 3.0e4, 0.0625)):
            assert np.array_equal(_bits(x[self.n:]), _bits((f + np.arange(GUARD)).astype(F32))), "guard overwritten"
        g = out[1][:self.n]
        assert not g.any() and not np.signbit(g).any(), "the gradients are not all +0 after the step"
        return out[0][:self.n], out[2][:self.n], out[3][:self.n]


def run_case(dev, p, g, m, v, step, sumsq, max_norm, wd, what, **kw):
    """One launch from (p, g, m, v) checked against the fp64 reference."""
    s = Slabs(dev, p, g, m, v)
    s.step(torch.from_numpy(np.asarray(sumsq, dtype=np.float64)).to(dev), max_norm, step, wd=wd, **kw)
    got = s.read()
    ref, tol = adam_ref(p, g, m, v, clip_coef(sumsq, max_norm), step, wd=wd)
    assert_within_bound(got, ref, tol, what)
    return got


# ---------------------------------------------------------------------------
# rt_grad_sqnorm
# ---------------------------------------------------------------------------
def _layout(sizes):
    starts = np.concatenate([[0], np.cumsum([(s + 3) // 4 * 4 for s in sizes])]).astype(np.int64)
    return starts       # starts[t + 1] is the next tensor's start: the zero padding is summed


def _sumsq_ref(g, starts):
    return np.array([math.fsum((g[lo:hi].astype(np.float64) ** 2).tolist())
                     for lo, hi in zip(starts[:-1], starts[1:])])


@gpu
@pytest.mark.parametrize("layout", ["blocks", "many"])
def test_grad_sqnorm(device, layout):
    """``blocks``: tensors around one chunk (1,024), around the 64 blocks of a
    tensor's grid row (65,536) and past them (a second trip), one empty.
    ``many``: 130 tensors of 1 to 40 elements. Products of fp32 values are
    exact in fp64 and the sums are fp64, hence rtol 1e-12."""
    from rtrec_amd import native
    rng = np.random.default_rng(11)
    if layout == "blocks":
        sizes = [0, 1, 255, 1023, 1024, 1025, 65536, 65537, 200003]
    else:
        sizes = [int(s) for s in rng.integers(1, 41, 130)]
        sizes[:2] = [1, 40]
    starts = _layout(sizes)
    g = np.zeros(starts[-1], dtype=F32)
    for lo, s in zip(starts, sizes):
        g[lo:lo + s] = (rng.standard_normal(s) * np.exp(rng.uniform(-30.0, 30.0, s))).astype(F32)
    if layout == "blocks":   # fp32 squares of these are inf: only fp64 squares give the sum
        lo = int(starts[5])
        g[lo + np.array([0, 511, 1024])] = np.array([3e19, -1e20, 7e19], dtype=F32)
        with np.errstate(over="ignore"):
            assert np.isinf(g[lo] * g[lo])
    ref = _sumsq_ref(g, starts)
    prefill = np.where(ref > 0, ref * (0.25 + 0.01 * np.arange(len(sizes))), 3.75)
    dg = torch.from_numpy(g).to(device)
    offsets = torch.from_numpy(starts).to(device)
    sumsq = torch.from_numpy(prefill).to(device)
    step = torch.full((1,), 5, dtype=torch.int32, device=device)
    seed = torch.full((1,), 2 ** 40 + 9, dtype=torch.int64, device=device)
    native.call("rt_grad_sqnorm", native.ptr(dg), native.ptr(offsets), len(sizes), native.ptr(sumsq),
                native.ptr(step), native.ptr(seed), native.stream_of(dg))
    torch.cuda.synchronize()
    got = sumsq.cpu().numpy()
    np.testing.assert_allclose(got, prefill + ref, rtol=1e-12, atol=0.0)
    empty = [t for t, s in enumerate(sizes) if s == 0]
    assert np.array_equal(_bits(got[empty]), _bits(prefill[empty]))
    assert int(step.item()) == 6 and int(seed.item()) == 2 ** 40 + 10
    # NULL counters: the same sums once more, the counters stay
    native.call("rt_grad_sqnorm", native.ptr(dg), native.ptr(offsets), len(sizes), native.ptr(sumsq), None, None,
                native.stream_of(dg))
    torch.cuda.synchronize()
    np.testing.assert_allclose(sumsq.cpu().numpy(), prefill + 2 * ref, rtol=1e-12, atol=0.0)
    assert np.array_equal(_bits(sumsq.cpu().numpy()[empty]), _bits(prefill[empty]))
    assert int(step.item()) == 6 and int(seed.item()) == 2 ** 40 + 10
    assert np.array_equal(_bits(dg.cpu().numpy()), _bits(g))


# ---------------------------------------------------------------------------
# rt_clip_adam_step: one step
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("wd", [0.0, 1e-5])
@pytest.mark.parametrize("kind", ["fresh", "warm"])
@pytest.mark.parametrize("n", SIZES)
def test_adam_one_step(device, n, kind, wd):
    """Sizes around one block (256), the grid's 1,024 blocks (262,144) and up to
    three grid-stride trips with a ragged tail; scalars for step and lr."""
    p, m, v, step, g0 = state(kind, n)
    for max_norm in (1.0, 0.25):
        for clip in ("clipped", "below", "zero"):
            sumsq = split_sumsq(clip_sumsq(clip, max_norm), 1)
            g = np.zeros(n, dtype=F32) if clip == "zero" else shape_grads(g0, p, wd, clip_coef(sumsq, max_norm))
            run_case(device, p, g, m, v, step, sumsq, max_norm, wd, f"n={n} {kind} wd={wd} {clip} max_norm={max_norm}")


@gpu
@pytest.mark.parametrize("max_norm", [1.0, 0.25])
@pytest.mark.parametrize("clip", ["clipped", "below", "zero"])
def test_adam_sumsq_spread_over_tensors(device, clip, max_norm):
    """The same total over 1, 64, 65 and 130 per-tensor slots (wave 0's strided
    loop and its wave_sum): each within the bound, and — the totals being exact
    in any order — bit-equal to one another."""
    n, wd = 1025, 1e-5
    p, m, v, step, g0 = state("warm", n)
    total = clip_sumsq(clip, max_norm)
    g = np.zeros(n, dtype=F32) if clip == "zero" else shape_grads(g0, p, wd, clip_coef([total], max_norm))
    got = [run_case(device, p, g, m, v, step, split_sumsq(total, t), max_norm, wd, f"{clip} over {t} tensors")
           for t in (1, 64, 65, 130)]
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert np.array_equal(_bits(a), _bits(b))


@gpu
@pytest.mark.parametrize("target", [1.0, 0.37, 0.096, 1e-3])
def test_clip_factor_is_visible_in_first_moment(device, target):
    """From m = v = 0 at step 1 without weight decay, m1 = (1-b1)·g·coef: the
    ratio reads the kernel's clip factor (three fp32 roundings in coef, two in
    the moment: 8E covers them)."""
    n = 4099
    p, m, v, step, g0 = state("fresh", n)
    sumsq = np.array([0.5 if target == 1.0 else (1.0 / target) ** 2])
    coef = clip_coef(sumsq, 1.0)
    assert abs(coef - target) <= 1e-3 * target
    got = run_case(device, p, g0, m, v, 1, sumsq, 1.0, 0.0, f"coef={target}")
    ok = np.abs(g0) * target > 1e-30          # normal numbers all the way
    assert ok.sum() > n // 2
    read = got[1][ok].astype(np.float64) / ((1 - hp(B1)) * g0[ok].astype(np.float64))
    assert np.max(np.abs(read / coef - 1)) <= 8 * E, (coef, np.max(np.abs(read / coef - 1)))


@gpu
def test_device_step_and_lr_take_precedence(device):
    n, wd = 1025, 1e-5
    p, m, v, _, g0 = state("warm", n)
    sumsq = split_sumsq(clip_sumsq("clipped", 1.0), 1)
    coef = clip_coef(sumsq, 1.0)
    g = shape_grads(g0, p, wd, coef)
    dsumsq = torch.from_numpy(sumsq).to(device)
    lr_dev = torch.tensor([3e-4], dtype=torch.float32, device=device)
    step_dev = torch.tensor([7], dtype=torch.int32, device=device)
    cases = [("lr_dev", dict(lr=1.0, lr_dev=lr_dev, step=7), 3e-4, 7),
             ("step_dev", dict(lr=LR, step_dev=step_dev, step=1), LR, 7),
             ("both", dict(lr=1.0, lr_dev=lr_dev, step_dev=step_dev, step=1), 3e-4, 7),
             ("scalars", dict(lr=3e-4, step=7), 3e-4, 7),
             ("scalars, step 1", dict(lr=LR, step=1), LR, 1)]
    for what, kw, lr_used, step_used in cases:
        s = Slabs(device, p, g, m, v)
        s.step(dsumsq, 1.0, kw.pop("step"), wd=wd, **kw)
        ref, tol = adam_ref(p, g, m, v, coef, step_used, lr=lr_used, wd=wd)
        assert_within_bound(s.read(), ref, tol, f"precedence: {what}")
    assert int(step_dev.item()) == 7 and float(lr_dev.item()) == float(np.float32(3e-4))   # read, never written


@gpu
@pytest.mark.parametrize("n,zero_words", [(300, 5000), (262145, 3), (300, 0)])
def test_zero_buf(device, n, zero_words):
    """zero_buf[0, zero_words) comes back zero, whether longer than the grid's
    first trip or shorter than one block; the words past it are untouched.
    zero_words == 0 is run with a NULL buffer."""
    wd = 1e-5
    p, m, v, step, g0 = state("warm", n)
    sumsq = split_sumsq(clip_sumsq("clipped", 1.0), 1)
    g = shape_grads(g0, p, wd, clip_coef(sumsq, 1.0))
    fill = np.arange(1, zero_words + GUARD + 1, dtype=np.float64) * -1.5
    zbuf = torch.from_numpy(fill).to(device) if zero_words else None
    run_case(device, p, g, m, v, step, sumsq, 1.0, wd, f"zero_buf n={n} words={zero_words}", zero_buf=zbuf,
             zero_words=zero_words)
    if zero_words:
        z = zbuf.cpu().numpy()
        assert not _bits(z[:zero_words]).any()
        assert np.array_equal(_bits(z[zero_words:]), _bits(fill[zero_words:]))


@gpu
def test_norm_then_adam_counter_chain(device):
    """Three rounds of rt_grad_sqnorm (which bumps the step and seed counters)
    and rt_clip_adam_step (which reads the step counter; its scalar step stays
    1, as FusedTrainStep passes it) over a slab of 130 small tensors. Each
    round's state lies within the bound of the fp64 step taken from the
    kernels' own previous state."""
    from rtrec_amd import native
    rng = np.random.default_rng(23)
    sizes = [int(s) for s in rng.integers(1, 41, 130)]
    starts = _layout(sizes)
    n, wd, max_norm = int(starts[-1]), 1e-5, 1.0
    used = np.zeros(n, dtype=bool)
    for lo, s in zip(starts, sizes):
        used[lo:lo + s] = True
    p0 = np.where(used, 0.1 * rng.standard_normal(n), 0).astype(F32)
    zeros = np.zeros(n, dtype=F32)
    s = Slabs(device, p0, zeros, zeros, zeros)
    offsets = torch.from_numpy(starts).to(device)
    sumsq = torch.zeros(len(sizes), dtype=torch.float64, device=device)
    step_dev = torch.zeros(1, dtype=torch.int32, device=device)
    seed_dev = torch.full((1,), 41, dtype=torch.int64, device=device)
    p, m, v = p0, zeros, zeros
    for rnd in (1, 2, 3):
        g = np.where(used, 40.0 * rng.standard_normal(n) * np.exp(rng.uniform(-14.0, 1.0, n)), 0).astype(F32)
        s.t[1][:n].copy_(torch.from_numpy(g))
        sumsq.zero_()       # the step's first forward launch in FusedTrainStep
        native.call("rt_grad_sqnorm", native.ptr(s.t[1]), native.ptr(offsets), len(sizes), native.ptr(sumsq),
                    native.ptr(step_dev), native.ptr(seed_dev), native.stream_of(sumsq))
        s.step(sumsq, max_norm, 1, wd=wd, step_dev=step_dev)
        ref_sumsq = _sumsq_ref(g, starts)
        np.testing.assert_allclose(sumsq.cpu().numpy(), ref_sumsq, rtol=1e-12, atol=0.0)
        coef = clip_coef(ref_sumsq, max_norm)
        assert coef < 0.5    # the rounds are clipped ones
        ref, tol = adam_ref(p, g, m, v, coef, rnd, wd=wd)
        p, m, v = s.read()
        assert_within_bound((p, m, v), ref, tol, f"chain round {rnd}")
        assert int(step_dev.item()) == rnd and int(seed_dev.item()) == 41 + rnd
    assert int(step_dev.item()) == 3


@gpu
@pytest.mark.parametrize("wd", [0.0, 1e-5])
def test_non_finite_norm_propagates(device, wd):
    """clip_grad_norm_ clamps with torch.clamp(max=1), which keeps NaN: a NaN
    norm poisons every parameter and moment (the run fails loudly). An infinite
    norm gives coef = 0: finite gradients drop out (gv = wd·p), an infinite one
    becomes inf·0 = NaN, alone."""
    n = 262145 + 300
    p, m, v, step, g0 = state("warm", n)
    g = shape_grads(g0, p, wd, 1.0)
    # a NaN in one tensor's sum
    sumsq = split_sumsq(128.0, 65)
    sumsq[37] = float("nan")
    s = Slabs(device, p, g, m, v)
    s.step(torch.from_numpy(sumsq).to(device), 1.0, step, wd=wd)
    for name, a in zip("pmv", s.read()):          # read() also checks g == 0 and the guards
        assert np.isnan(a).all(), name
    # sums reaching inf
    sumsq = split_sumsq(128.0, 65)
    sumsq[64] = float("inf")
    assert clip_coef(sumsq, 1.0) == 0.0
    g = g.copy()
    hot = np.array([0, 255, 256, 262144, n - 1])
    g[hot] = np.array([np.inf, -np.inf, np.inf, -np.inf, np.inf], dtype=F32)
    got = run_case(device, p, g, m, v, step, sumsq, 1.0, wd, f"inf norm wd={wd}")   # NaN positions compared exactly
    want = np.zeros(n, dtype=bool)
    want[hot] = True
    for name, a in zip("pmv", got):
        assert np.array_equal(np.isnan(a), want), name


# ---------------------------------------------------------------------------
# FusedTrainStep: the Adam moments against the oracle
# ---------------------------------------------------------------------------
def _moment_close(got, ref, scale, msg):
    np.testing.assert_allclose(got, ref, rtol=1e-3, atol=1e-4 * np.abs(ref).max() + 1e-7 * scale, err_msg=msg)


@gpu
@pytest.mark.parametrize("max_norm,wd", [(1.0, 0.0), (0.25, 0.0), (100.0, 0.0), (1.0, 1e-2)])
def test_fused_train_step_moments(device, max_norm, wd):
    """Two steps; after each, every exp_avg / exp_avg_sq / step of
    optimizer_state_dict() against oracle.train_step's, at the project's bar for
    parameter gradients (rtol 1e-3, atol 1e-4·max|ref| + 1e-7) carried through
    the linear map from gradient to moment. The oracle's gradient norm is ~10:
    max_norm 1 and 0.25 clip by 10x and 40x, 100 does not clip."""
    from oracle import two_tower as orc
    from rtrec_amd.models.two_tower import ItemTower, TwoTowerModel, UserTower
    from rtrec_amd.training.fused_step import FusedTrainStep
    torch.manual_seed(5)
    model = TwoTowerModel(UserTower(10, 32, [64, 32], dropout_rate=0.0),
                          ItemTower(15, 32, [64, 32], dropout_rate=0.0, use_content_embedding=False),
                          temperature=0.05)
    us = {k: v.detach().clone() for k, v in model.user_tower.state_dict().items()}
    its = {k: v.detach().clone() for k, v in model.item_tower.state_dict().items()}
    biases = {"user_bias": model.user_bias.detach().clone(), "item_bias": model.item_bias.detach().clone()}
    names = orc.param_names(us, its)
    assert names == [k for k, _ in model.named_parameters()]   # state[i] is parameter i of model.parameters()
    model.to(device)
    step = FusedTrainStep(model, lr=1e-3, weight_decay=wd, max_norm=max_norm)
    assert len(names) == len(step.slab.params)
    gen = torch.Generator().manual_seed(9)
    opt = {}
    b1, b2 = hp(B1), hp(B2)
    for k in (1, 2):
        u = torch.randn(64, 10, generator=gen)
        p = torch.randn(64, 15, generator=gen)
        n = torch.randn(64, 4, 15, generator=gen)
        r = orc.train_step(us, its, biases, opt, u, p, n, temperature=0.05, lr=1e-3, weight_decay=wd,
                           max_norm=max_norm)
        norm = r["grad_norm"]
        assert norm > 2 * max_norm or norm < max_norm / 2, (norm, max_norm)   # clearly clipped, or clearly not
        step(u.to(device), p.to(device), n.to(device))
        torch.cuda.synchronize()
        s = (1 - b1) * min(1.0, max_norm / norm)
        got = step.optimizer_state_dict()["state"]
        assert len(got) == len(names)
        for i, name in enumerate(names):
            want = opt[name]
            assert int(got[i]["step"]) == k == want["step"], name
            assert got[i]["exp_avg"].shape == want["exp_avg"].shape, name
            _moment_close(got[i]["exp_avg"].cpu().numpy(), want["exp_avg"].numpy(), s, f"step {k} exp_avg {name}")
            _moment_close(np.sqrt(got[i]["exp_avg_sq"].cpu().numpy()), np.sqrt(want["exp_avg_sq"].numpy()),
                          s * math.sqrt(1 - b2) / (1 - b1), f"step {k} sqrt(exp_avg_sq) {name}")
