"""Forward plus backward of small tower chains through rtrec_amd.models.fused
against a float64 evaluation of the same modules, at the shapes that pick each
build of the dz kernel `linear_bwd_dz_kernel<TPWK, WPL, KS, FE>` (CASES names
the instance every dz launch of a case reaches). A launch of two dA tiles per
wave (k = 256) with at most 256 row blocks is split over k and runs the
one-tile KS instance, so the two-tile instances need more than 256 row blocks:
m = 8224 rows. The bars are those of tests/test_gpu_model.py for tower
gradients: outputs 1e-4 relative + 2e-6, the input gradient 1e-3 relative +
1e-5, every parameter gradient 1e-3 relative + 1e-4 of its own largest entry.
One test function walks all cases and reports every case that fails."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

K0 = 24


def _seq(hidden, n, p):
    mods, k = [], K0
    for h in hidden:
        mods += [nn.Linear(k, h), nn.ReLU(), nn.BatchNorm1d(h), nn.Dropout(p)]
        k = h
    mods.append(nn.Linear(k, n))
    seq = nn.Sequential(*mods)
    with torch.no_grad():
        for mod in seq:
            if isinstance(mod, nn.BatchNorm1d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.5, 0.5)
    return seq.train()


def _masks(blocks, x, seg_split, seed_base, device):
    """The dropout masks of the chain's hidden blocks, read back from the
    forward: the blocks up to i followed by an identity Linear, run with the
    same per-layer seeds (BN shifts every kept value away from 0)."""
    from rtrec_amd.models.fused import Block, chain_forward
    masks = []
    for i, b in enumerate(blocks[:-1]):
        h = b.linear.out_features
        eye = nn.Linear(h, h).to(device)
        with torch.no_grad():
            eye.weight.copy_(torch.eye(h))
            eye.bias.zero_()
        probe = list(blocks[:i + 1]) + [Block(eye)]
        out = chain_forward(probe, x, normalize=False, seg_split=seg_split, seed_base=seed_base).out
        masks.append((out != 0).cpu())
    return masks


def _reference(ref, x, r, seg_split, masks, p):
    """float64 autograd of the same chain (``ref``: its float64 copy): each BN
    segment is its own batch."""
    xr = x.cpu().double().requires_grad_(True)
    segs = [(0, seg_split), (seg_split, x.shape[0])] if seg_split else [(0, x.shape[0])]
    outs = []
    for lo, hi in segs:
        h, li = xr[lo:hi], 0
        for mod in ref:
            if isinstance(mod, nn.Dropout):
                if p > 0:
                    h = h * masks[li][lo:hi].double() / (1.0 - p)
                li += 1
            else:
                h = mod(h)
        outs.append(F.normalize(h, dim=1))
    y = torch.cat(outs)
    (y * r.cpu().double()).sum().backward()
    return y.detach(), xr.grad, [q.grad for q in ref.parameters()]


# name, m, seg_split, hidden widths, out width, dropout p, want_dsrc.
# The first Linear has no dA (its dz is computed by the dW launch) unless dsrc is
# asked for; the instances below are those of the other layers, last layer first.
CASES = (
    # <1,false,false,0>: a partial last row block keeps the all-paths instance
    ("partial-row-block", 101, 0, (128,), 128, 0.0, False),
    # <1,false,false,1>, two BatchNorm segments
    ("two-bn-segments", 128, 32, (128,), 128, 0.0, False),
    # <1,false,false,0>: n = 16 has pad columns, so no fast F.normalize phase A
    ("n16-pad-columns", 128, 0, (128,), 16, 0.0, False),
    # <1,false,true,0>: k = 256 on 4 row blocks is split over k
    ("k256-ksplit", 128, 0, (256,), 128, 0.0, False),
    # <1,false,false,1>, then <1,false,true,0>
    ("c2-widths-ksplit", 128, 0, (256, 128), 128, 0.2, False),
    # <1,false,false,1>, then <1,false,false,0> for the first Linear (dsrc, no Wᵀ)
    ("dsrc", 128, 0, (128,), 128, 0.0, True),
    # <2,false,false,1>: k = 256 into F.normalize, 257 row blocks
    ("two-tiles-normalize", 8224, 0, (256,), 128, 0.0, False),
    ("two-tiles-normalize-dropout", 8224, 0, (256,), 128, 0.2, False),
    # <1,false,false,1>, then <2,false,false,2>: k = 256 into BatchNorm (the C2 dz2 launch)
    ("two-tiles-batchnorm", 8224, 0, (256, 128), 128, 0.0, False),
    ("two-tiles-batchnorm-dropout", 8224, 0, (256, 128), 128, 0.2, False),
    # the same with dsrc: the first Linear's dz launch joins (<1,false,false,0>)
    ("two-tiles-batchnorm-dropout-dsrc", 8224, 0, (256, 128), 128, 0.2, True),
)


def test_chain_forward_backward_vs_float64(device):
    failed = []
    for case in CASES:
        try:
            _run_case(device, *case)
        except AssertionError as e:
            failed.append(f"{case[0]}: {e}")
    assert not failed, "\n".join(failed)


def _run_case(device, what, m, seg_split, hidden, n, p, want_dsrc):
    from rtrec_amd.models.fused import ParamSlab, blocks_from_sequential, chain_backward, chain_forward
    torch.manual_seed(100 * m + 10 * len(hidden) + n + int(10 * p))
    seq = _seq(hidden, n, p)
    ref = copy.deepcopy(seq).double().train()
    x = torch.randn(m, K0)
    r = torch.randn(m, n)
    seq.to(device)
    slab = ParamSlab(seq).ensure()
    blocks = blocks_from_sequential(seq)
    xd, rd = x.to(device), r.to(device)
    seed_base = 1234
    masks = _masks(blocks, xd, seg_split, seed_base, device) if p > 0 else None
    if masks is not None:
        for mk in masks:  # a real mask, not all-kept
            assert abs(mk.float().mean().item() - (1 - p)) < 0.02, what
    y_ref, dx_ref, grads_ref = _reference(ref, x, r, seg_split, masks, p)

    ctx = chain_forward(blocks, xd, seg_split=seg_split, seed_base=seed_base)
    slab.grad.zero_()
    dx = chain_backward(blocks, ctx, rd, slab, want_dsrc=want_dsrc)
    torch.cuda.synchronize()
    np.testing.assert_allclose(ctx.out.cpu().numpy(), y_ref.numpy(), rtol=1e-4, atol=2e-6, err_msg=what)
    if want_dsrc:
        np.testing.assert_allclose(dx.cpu().numpy(), dx_ref.numpy(), rtol=1e-3, atol=1e-5, err_msg=what)
    else:
        assert dx is None, what
    names = [k for k, _ in seq.named_parameters()]
    for name, q, want in zip(names, seq.parameters(), grads_ref):
        want = want.numpy()
        np.testing.assert_allclose(q.grad.cpu().numpy(), want, rtol=1e-3, atol=1e-4 * np.abs(want).max() + 1e-7,
                                   err_msg=f"{what} {name}")
