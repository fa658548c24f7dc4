"""Fused loss on the fp32 path at the shapes where its wave / span geometry
changes: both launches take 256-row spans; launch 1 runs them as two 32-row
tiles per wave on 4 waves, launch 2 as one tile per wave on 8 waves (D <= 128)
or two tiles per wave on 4 (D = 256). Reference: the loss formulas of
tests/test_gpu_loss_dtypes.py in float64 (torch autograd); the bars are that
file's (loss 1e-4 relative, every gradient 1e-4 of its own largest entry; the
bias gradients, which that file does not check, get the same gradient bar).
One test function walks all shapes and reports every shape that fails."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TAU = 0.05


def _inputs(b, nx, d, n_neg):
    g = torch.Generator().manual_seed(1000 * b + 10 * nx + d + n_neg)
    u = F.normalize(torch.randn(b, d, generator=g), dim=1)
    p = F.normalize(torch.randn(nx, d, generator=g), dim=1)
    q = F.normalize(torch.randn(b * n_neg, d, generator=g), dim=1) if n_neg else None
    return u, p, q


def _close_grad(got, ref, what):
    ref = ref.numpy()
    np.testing.assert_allclose(got.cpu().numpy().astype(np.float64).reshape(ref.shape), ref, rtol=0,
                               atol=1e-4 * float(np.abs(ref).max()), err_msg=what)


def _square(device, b, d, n_neg):
    from oracle import two_tower as orc
    from rtrec_amd import kernels
    what = f"b={b} d={d} n_neg={n_neg}"
    u, p, q = _inputs(b, b, d, n_neg)
    ub, ib = torch.tensor([0.1]), torch.tensor([-0.05])
    uu, pp = u.double().requires_grad_(), p.double().requires_grad_()
    qq = q.double().requires_grad_() if q is not None else None
    ubd, ibd = ub.double().requires_grad_(), ib.double().requires_grad_()
    ib_loss = orc.in_batch_negative_loss(uu, pp, TAU)
    if q is not None:
        ex = orc.contrastive_loss(uu, pp, qq, TAU, ubd, ibd)
        total = 0.7 * ex + 0.3 * ib_loss
    else:
        total = ib_loss
    total.backward()
    qd = q.to(device) if q is not None else None
    loss, du, dp, dq, dub, dib = kernels.twotower_loss(u.to(device), p.to(device), qd, TAU, ub.to(device),
                                                       ib.to(device))
    loss_only = kernels.twotower_loss(u.to(device), p.to(device), qd, TAU, ub.to(device), ib.to(device),
                                      grad=False)[0]
    torch.cuda.synchronize()
    np.testing.assert_allclose(loss[0].item(), total.item(), rtol=1e-4, err_msg=what)
    np.testing.assert_allclose(loss[2].item(), ib_loss.item(), rtol=1e-4, err_msg=what)
    _close_grad(du, uu.grad, what + " du")
    _close_grad(dp, pp.grad, what + " dp")
    if q is not None:
        np.testing.assert_allclose(loss[1].item(), ex.item(), rtol=1e-4, err_msg=what)
        _close_grad(dq, qq.grad, what + " dq")
        _close_grad(dub, ubd.grad, what + " d user_bias")
        _close_grad(dib, ibd.grad, what + " d item_bias")
    # the loss-only call runs the same launch 1 and the same scalar reduction
    # (fp64 atomics, one per 32 users): equal up to their order
    np.testing.assert_allclose(loss_only.cpu().numpy(), loss.cpu().numpy(), rtol=1e-12, err_msg=what)


def _rect(device, b, nx, off, d):
    """b local users against nx items, label of user i = item off + i (the
    rectangular entry has no explicit-negative term)."""
    from rtrec_amd import kernels
    what = f"b={b} nx={nx} off={off} d={d}"
    u, p, _ = _inputs(b, nx, d, 0)
    uu, pp = u.double().requires_grad_(), p.double().requires_grad_()
    ref = F.cross_entropy(uu @ pp.t() / TAU, off + torch.arange(b))
    ref.backward()
    loss, du, dp = kernels.inbatch_loss(u.to(device), p.to(device), TAU, label_offset=off)
    loss_only = kernels.inbatch_loss(u.to(device), p.to(device), TAU, label_offset=off, grad=False)[0]
    torch.cuda.synchronize()
    np.testing.assert_allclose(loss[0].item(), ref.item(), rtol=1e-4, err_msg=what)
    _close_grad(du, uu.grad, what + " du")
    _close_grad(dp, pp.grad, what + " dp")
    np.testing.assert_allclose(loss_only.cpu().numpy(), loss.cpu().numpy(), rtol=1e-12, err_msg=what)


def test_loss_fp32_vs_float64_at_wave_and_span_edges(device):
    failed = []

    def case(fn, *shape):
        try:
            fn(device, *shape)
        except AssertionError as e:
            failed.append(str(e))

    # (b, d, n_neg): seven idle waves; a partial span with fewer tiles than
    # waves; five tiles (launch 1: a wave with a second tile), no explicit term;
    # a full 256-row span plus one tile; rows not a multiple of 32; the 4-wave
    # path (d = 256)
    for b, d, n_neg in ((32, 128, 16), (96, 128, 3), (160, 64, 0), (288, 128, 16), (40, 128, 16), (64, 256, 16)):
        case(_square, b, d, n_neg)
    # (b, nx, off, d): nx != b with a label offset, the data-parallel shard case.
    # It runs without explicit negatives (n_neg = 0): the only entry point with
    # nx != b, rt_inbatch_loss_fwd_bwd, has no explicit term.
    case(_rect, 64, 192, 64, 128)
    assert not failed, "\n".join(failed)
    # the workspace both launches share: part is [ceil(b / 256)][b] float2, then
    # three [b] float vectors, + 256 B, whatever wave count launch 2 runs with
    from rtrec_amd import native
    ws = native.lib().rt_twotower_loss_workspace_bytes
    for b in (32, 256, 257, 288, 1024):
        for d in (64, 128, 256):
            assert ws(b, d) == -(-b // 256) * b * 8 + 3 * b * 4 + 256, (b, d)
