"""Fragment-ordered weight images: a training chain stores the
fp32 values of its weights in the order the lanes of the forward and dz
k-loops read them (rt_linear_fwd_args.w_frag / next_w_frag / wt_frag_out,
rt_linear_bwd_args.wt_frag), written once per chain by a side task. Operand
values and MFMA order are those of the loads from W / Wᵀ, so the tower
outputs must be bit-identical with the images on and off, and a train step
equal up to the fp32 atomics of its last dW launch (the criteria of
tests/test_gpu_wplanes.py). Each test function walks its cases and reports
every case that fails."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from rtrec_amd.models import fused

pytestmark = pytest.mark.gpu

SEED_BASE = 4321
P_DROP = 0.2
# (hidden widths, embedding width): the C2 widths; n = 96 leaves the fourth
# column tile off and n = 100 has zero-padded image rows and a partial tile;
# k = 40 pads to 64 and n = 256 takes the two-tile forward instance
WIDTHS = (((256, 128), 128), ((64, 96), 100), ((40, 256), 64))
# (rows, seg_split) of an item batch. A merged positives + negatives chain needs
# its first segment to be a multiple of 32 rows, so 3 positives + 30 negatives
# run as the trainer's unmerged path runs them: two tower calls, each its own
# BatchNorm batch (3 rows; 30 rows). 33 rows as one batch span a partial second
# row block; 70 rows with a 32-row first segment are two BatchNorm segments in
# one chain with a partial last row block.
ITEM_BATCHES = ((3, 0), (30, 0), (33, 0), (70, 32))


@pytest.fixture
def frag_switch():
    keep = (fused.W_FRAG_FWD, fused.W_FRAG_DZ)
    yield
    fused.W_FRAG_FWD, fused.W_FRAG_DZ = keep


def _set(fwd, dz):
    fused.W_FRAG_FWD, fused.W_FRAG_DZ = fwd, dz


def _model(device, hidden, emb, dropout=P_DROP, seed=3):
    from rtrec_amd.training.utils import create_two_tower_model_for_training
    torch.manual_seed(seed)
    cfg = {"embedding_dim": emb, "hidden_layers": list(hidden), "dropout_rate": dropout, "temperature": 0.05}
    m = create_two_tower_model_for_training(3, 20, cfg)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm1d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.5, 0.5)
    return m.to(device)


def _masks(blocks, x, seg_split, device):
    """The dropout masks of the chain's hidden blocks, read back from the
    forward (tests/test_gpu_dz_fast_paths.py): the blocks up to i followed by an
    identity Linear, run with the same per-layer seeds."""
    masks = []
    for i, b in enumerate(blocks[:-1]):
        h = b.linear.out_features
        eye = nn.Linear(h, h).to(device).train()
        with torch.no_grad():
            eye.weight.copy_(torch.eye(h))
            eye.bias.zero_()
        probe = list(blocks[:i + 1]) + [fused.Block(eye)]
        out = fused.chain_forward(probe, x, normalize=False, seg_split=seg_split, seed_base=SEED_BASE).out
        masks.append((out != 0).cpu())
    return masks


def _forward64(seq, x, seg_split, masks):
    """float64 evaluation of the chain; each BatchNorm segment is its own batch."""
    ref = copy.deepcopy(seq).cpu().double()
    ref.train(seq.training)
    xr = x.cpu().double()
    segs = [(0, seg_split), (seg_split, x.shape[0])] if seg_split else [(0, x.shape[0])]
    outs = []
    with torch.no_grad():
        for lo, hi in segs:
            h, li = xr[lo:hi], 0
            for mod in ref:
                if isinstance(mod, nn.Dropout):
                    if masks is not None:
                        h = h * masks[li][lo:hi].double() / (1.0 - P_DROP)
                    li += 1
                else:
                    h = mod(h)
            outs.append(F.normalize(h, dim=1))
    return torch.cat(outs)


def _chain_out(seq, x, seg_split):
    blocks = fused.blocks_from_sequential(seq)
    out = fused.chain_forward(blocks, x, seg_split=seg_split, seed_base=SEED_BASE).out
    torch.cuda.synchronize()
    return out


def _forward_case(device, hidden, emb, rows, seg_split, training):
    what = f"hidden={hidden} emb={emb} rows={rows} seg={seg_split} {'train' if training else 'eval'}"
    m = _model(device, hidden, emb)
    g = torch.Generator(device=device).manual_seed(rows + 7 * emb)
    for seq, k0 in ((m.item_tower.mlp, 20), (m.user_tower.mlp, 3)):
        x = torch.randn(rows, k0, device=device, generator=g)
        seq.train(training)
        state = copy.deepcopy(seq.state_dict())  # the running statistics move with every training forward
        outs = {}
        for on in (False, True):
            seq.load_state_dict(state)
            _set(on, on)
            outs[on] = _chain_out(seq, x, seg_split)
        assert torch.equal(outs[False], outs[True]), f"{what} k0={k0}: image on != off"
        seq.load_state_dict(state)
        masks = _masks(fused.blocks_from_sequential(seq), x, seg_split, device) if training else None
        seq.load_state_dict(state)
        ref = _forward64(seq, x, seg_split, masks)
        # the bar tests/test_gpu_model.py holds tower outputs to
        np.testing.assert_allclose(outs[True].cpu().numpy(), ref.numpy(), rtol=1e-4, atol=2e-6,
                                   err_msg=f"{what} k0={k0}")


def test_forward_image_on_off_bit_identical(device, frag_switch):
    failed = []
    for hidden, emb in WIDTHS:
        for rows, seg in ITEM_BATCHES:
            for training in (True, False):
                if not training and seg:
                    continue  # eval BatchNorm has no batches to separate
                try:
                    _forward_case(device, hidden, emb, rows, seg, training)
                except AssertionError as e:
                    failed.append(str(e)[:600])
    assert not failed, "\n".join(failed)


def test_stale_image_is_rewritten(device, frag_switch):
    """The images are written by every chain, never cached: after an in-place
    weight update the next training forward reads the new weights."""
    failed = []
    for hidden, emb in WIDTHS:
        m = _model(device, hidden, emb)
        seq = m.item_tower.mlp.train()
        g = torch.Generator(device=device).manual_seed(11)
        x = torch.randn(70, 20, device=device, generator=g)
        _set(True, True)
        first = _chain_out(seq, x, 0)
        with torch.no_grad():
            for mod in seq:
                if isinstance(mod, nn.Linear):
                    mod.weight.mul_(1.5)
        state = copy.deepcopy(seq.state_dict())
        on = _chain_out(seq, x, 0)
        seq.load_state_dict(state)
        _set(False, False)
        off = _chain_out(seq, x, 0)
        if not torch.equal(on, off):
            failed.append(f"hidden={hidden} emb={emb}: forward after weight.mul_ differs from the image-off forward")
        if torch.equal(on, first):
            failed.append(f"hidden={hidden} emb={emb}: the weight update did not change the output")
    assert not failed, "\n".join(failed)


def _grads(device, m0, b, n_neg, sides, legacy):
    """Loss and every parameter gradient of one fused step's forward + backward."""
    from rtrec_amd.training.fused_step import FusedTrainStep
    g = torch.Generator(device=device).manual_seed(2)
    ut = torch.randn(600, 3, device=device, generator=g)
    mt = torch.randn(3416, 20, device=device, generator=g)
    u = torch.randint(0, 600, (b,), device=device, generator=g)
    pn = torch.randint(0, 3416, (b * (n_neg + 1),), device=device, generator=g)
    p, n = pn[:b], pn[b:].view(b, n_neg)
    old = os.environ.get("RTREC_DW_LEGACY")
    if legacy:
        os.environ["RTREC_DW_LEGACY"] = "1"
    try:
        _set(*sides)
        m = copy.deepcopy(m0)
        st = FusedTrainStep(m, dropout_seed=77)
        m.train()
        st._ensure_clean()
        st._grads(ut, mt, mt, u, p, n)
        torch.cuda.synchronize()
        return float(st.loss_buf[0].item()), [st.slab.grad[o:e].clone() for o, e in st.slab.bounds]
    finally:
        if legacy:
            if old is None:
                del os.environ["RTREC_DW_LEGACY"]
            else:
                os.environ["RTREC_DW_LEGACY"] = old


def _tower_grads(device, m0, sides, legacy, rows=96, seg_split=32):
    """Forward + backward of both towers' chains with a fixed output gradient,
    for embedding widths the fused loss does not take (it needs D % 8 == 0):
    (0.0, every parameter gradient of the item tower, then of the user tower)."""
    old = os.environ.get("RTREC_DW_LEGACY")
    if legacy:
        os.environ["RTREC_DW_LEGACY"] = "1"
    try:
        _set(*sides)
        m = copy.deepcopy(m0)
        grads = []
        g = torch.Generator(device=device).manual_seed(9)
        for seq, k0 in ((m.item_tower.mlp, 20), (m.user_tower.mlp, 3)):
            seq.train()
            x = torch.randn(rows, k0, device=device, generator=g)
            blocks = fused.blocks_from_sequential(seq)
            dout = torch.randn(rows, blocks[-1].linear.out_features, device=device, generator=g)
            slab = fused.ParamSlab(seq).ensure()
            slab.grad.zero_()
            ctx = fused.chain_forward(blocks, x, seg_split=seg_split, seed_base=SEED_BASE)
            fused.chain_backward(blocks, ctx, dout, slab)
            torch.cuda.synchronize()
            grads += [q.grad.detach().clone().reshape(-1) for q in seq.parameters()]
        return 0.0, grads
    finally:
        if legacy:
            if old is None:
                del os.environ["RTREC_DW_LEGACY"]
            else:
                os.environ["RTREC_DW_LEGACY"] = old


def _step(device, m0, emb, b, n_neg, sides, legacy):
    if emb % 8:
        return _tower_grads(device, m0, sides, legacy)
    return _grads(device, m0, b, n_neg, sides, legacy)


def _same_step(a, b, what):
    la, lb = a[0], b[0]
    assert abs(la - lb) <= 1e-12 * abs(la) + 1e-300, f"{what}: loss {la} vs {lb}"
    for i, (ga, gb) in enumerate(zip(a[1], b[1])):
        tol = 1e-5 * float(ga.abs().max()) + 1e-30
        err = float((ga - gb).abs().max())
        assert err <= tol, f"{what}: gradient tensor {i} differs by {err} > {tol}"


def test_train_step_image_on_off(device, frag_switch):
    """FusedTrainStep._grads with the images on (both sides, and each side
    alone) against off: the loss within 1e-12 relative, every gradient within
    1e-5 of its tensor's max; the same in the per-layer backward order
    (RTREC_DW_LEGACY=1). B = 514 with 16 negatives gives the negatives' item
    chain 8,224 rows (B is no multiple of 32, so positives and negatives run as
    chains of their own): the smallest launch that reaches the two-tile dz
    instances (tests/test_gpu_dz_fast_paths.py: at most 256 row blocks are
    split over k). The fused loss takes D % 8 == 0 only, so the [64, 96] / 100
    towers cannot go through _grads (with or without the images): they run
    chain forward + backward with a fixed output gradient (two BatchNorm
    segments, 96 rows), and [64, 96] / 104 — n = 104 also has zero-padded image
    rows and a partial tile, and a dz image with pad columns — takes the step."""
    failed = []
    cases = [((256, 128), 128, 64, 4, False), ((64, 96), 100, 64, 4, False), ((64, 96), 104, 64, 4, False),
             ((256, 128), 128, 64, 4, True), ((64, 96), 100, 64, 4, True), ((64, 96), 104, 64, 4, True),
             ((256, 128), 128, 514, 16, False)]
    for hidden, emb, b, n_neg, legacy in cases:
        what = f"hidden={hidden} emb={emb} B={b} N={n_neg} legacy={legacy}"
        m0 = _model(device, hidden, emb)
        off = _step(device, m0, emb, b, n_neg, (False, False), legacy)
        for sides in ((True, True), (True, False), (False, True)):
            try:
                _same_step(off, _step(device, m0, emb, b, n_neg, sides, legacy), f"{what} sides={sides}")
            except AssertionError as e:
                failed.append(str(e)[:400])
    assert not failed, "\n".join(failed)


def test_shapes_without_an_image_fall_back(device, frag_switch):
    """k = 50 on layer 2 (k % 8 != 0: no forward image) and n = 50 on layer 1's
    dz; an embedding width with n % 8 != 0 (no dz image for the last Linear):
    with the switch on they run the loads from W / Wᵀ and match the switch-off
    result exactly. (Gradients: dA of those layers is bit-identical, the dW sums
    add with atomics, so the step criteria apply.)"""
    failed = []
    for hidden, emb in (((50, 128), 128), ((64, 128), 100)):
        what = f"hidden={hidden} emb={emb}"
        m = _model(device, hidden, emb)
        g = torch.Generator(device=device).manual_seed(5)
        for seq, k0 in ((m.item_tower.mlp, 20), (m.user_tower.mlp, 3)):
            seq.train()
            x = torch.randn(70, k0, device=device, generator=g)
            state = copy.deepcopy(seq.state_dict())
            outs = {}
            for on in (False, True):
                seq.load_state_dict(state)
                _set(on, on)
                outs[on] = _chain_out(seq, x, 32)
            if not torch.equal(outs[False], outs[True]):
                failed.append(f"{what} k0={k0}: forward differs")
        m0 = _model(device, hidden, emb)
        try:
            _same_step(_step(device, m0, emb, 64, 4, (False, False), False),
                       _step(device, m0, emb, 64, 4, (True, True), False), what)
        except AssertionError as e:
            failed.append(str(e)[:400])
    # which Linears get an image is the host entry's answer
    from rtrec_amd import native
    wb = native.lib().rt_linear_w_frag_bytes
    assert wb(128, 50, 0) == 0 and wb(50, 20, 1) == 0 and wb(100, 128, 1) == 0
    assert wb(128, 64, 0) > 0 and wb(128, 64, 1) > 0
    assert not failed, "\n".join(failed)


TAU = 0.05


def _loss_case(device, b, n_neg, d, dtype):
    """rt_twotower_loss_fwd_bwd against the float64 formulas of
    tests/test_gpu_loss_waves.py, at that file's bars: loss 1e-4 relative, every
    gradient 1e-4 of its own largest entry. 16-bit inputs are rounded first, so
    the reference sees the values the kernel widens."""
    from oracle import two_tower as orc
    from rtrec_amd import kernels
    what = f"b={b} n_neg={n_neg} d={d} {dtype}"
    g = torch.Generator().manual_seed(1000 * b + 10 * n_neg + d)
    u = F.normalize(torch.randn(b, d, generator=g), dim=1).to(dtype)
    p = F.normalize(torch.randn(b, d, generator=g), dim=1).to(dtype)
    q = F.normalize(torch.randn(b * n_neg, d, generator=g), dim=1).to(dtype) if n_neg else None
    ub, ib = torch.tensor([0.1]), torch.tensor([-0.05])
    uu, pp = u.double().requires_grad_(), p.double().requires_grad_()
    qq = q.double().requires_grad_() if q is not None else None
    ubd, ibd = ub.double().requires_grad_(), ib.double().requires_grad_()
    ib_loss = orc.in_batch_negative_loss(uu, pp, TAU)
    total = 0.7 * orc.contrastive_loss(uu, pp, qq, TAU, ubd, ibd) + 0.3 * ib_loss if q is not None else ib_loss
    total.backward()
    qd = q.to(device) if q is not None else None
    loss, du, dp, dq, dub, dib = kernels.twotower_loss(u.to(device), p.to(device), qd, TAU, ub.to(device),
                                                       ib.to(device))
    torch.cuda.synchronize()
    np.testing.assert_allclose(loss[0].item(), total.item(), rtol=1e-4, err_msg=what)

    def close(got, ref, name):
        ref = ref.numpy()
        np.testing.assert_allclose(got.float().cpu().numpy().astype(np.float64).reshape(ref.shape), ref, rtol=0,
                                   atol=1e-4 * float(np.abs(ref).max()), err_msg=f"{what} {name}")
    close(du, uu.grad, "du")
    close(dp, pp.grad, "dp")
    if q is not None:
        close(dq, qq.grad, "dq")
        close(dub, ubd.grad, "d user_bias")
        close(dib, ibd.grad, "d item_bias")


def test_loss_fixed_tile_vs_float64(device):
    """The loss launches' fixed 32 x D tile: a batch below one tile with D = 32,
    two spans with partial tiles at D = 128, the 4-wave form at D = 256."""
    failed = []
    for b, n_neg, d in ((33, 3, 32), (257, 16, 128), (64, 0, 256)):
        for dtype in (torch.float32, torch.bfloat16):
            try:
                _loss_case(device, b, n_neg, d, dtype)
            except AssertionError as e:
                failed.append(str(e)[:400])
    assert not failed, "\n".join(failed)
