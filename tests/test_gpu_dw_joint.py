"""The joint backward order: every dz launch of a tower (pair), then ONE dW
launch for all of its Linears (rt_linear_bwd_dw_f32_joint), whose row-split
tiles are either added with atomics or stored and folded by the norm launch
(rt_grad_sqnorm_fold).

Parameter gradients are checked against torch autograd on the same modules and
against the per-layer order (RTREC_DW_LEGACY=1), both under the bar
tests/test_gpu_model.py uses for tower parameter gradients: rtol 1e-3,
atol 1e-4·max|ref| + 1e-7. With dropout on, autograd cannot draw the kernels'
masks, so those cases compare the two orders over ONE forward (same masks)."""
import contextlib
import copy
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _close(got, ref, msg):
    got, ref = got.detach().cpu().numpy(), ref.detach().cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-3, atol=1e-4 * np.abs(ref).max() + 1e-7, err_msg=msg)


@contextlib.contextmanager
def _legacy_order():
    old = os.environ.get("RTREC_DW_LEGACY")
    os.environ["RTREC_DW_LEGACY"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["RTREC_DW_LEGACY"]
        else:
            os.environ["RTREC_DW_LEGACY"] = old


def _mlp(widths, dropout, device, seed):
    from rtrec_amd.models.two_tower import _build_mlp
    torch.manual_seed(seed)
    return _build_mlp(widths[0], list(widths[1:-1]), widths[-1], dropout, "relu").to(device).train()


def _autograd(seq, segments, dout):
    """Parameter grads of Σ normalize(seq(x))·dout, one seq call per BN batch."""
    seq.zero_grad(set_to_none=True)
    out = torch.cat([F.normalize(seq(x), dim=1) for x in segments])
    (out * dout).sum().backward()
    grads = [p.grad.detach().clone() for p in seq.parameters()]
    seq.zero_grad(set_to_none=True)
    return grads


class _Chain:
    """One tower chain: module, fused forward context, upstream gradient."""

    def __init__(self, seq, src, ids, seg_split, seed):
        from rtrec_amd.models.fused import blocks_from_sequential, chain_forward
        self.seq, self.src, self.ids, self.seg = seq, src, ids, seg_split
        self.blocks = blocks_from_sequential(seq)
        self.ctx = chain_forward(self.blocks, src, ids, True, None, None, seg_split, seed_base=seed)
        g = torch.Generator().manual_seed(seed)
        self.dout = torch.randn(self.ctx.out.shape, generator=g).to(src.device)

    def segments(self):
        x = self.src if self.ids is None else self.src[self.ids]
        return [x[:self.seg], x[self.seg:]] if self.seg else [x]

    def bwd(self, slab):
        return (self.blocks, self.ctx, self.dout, slab, False, None, None, True)


def _grads_of(slab, seqs):
    torch.cuda.synchronize()
    out = [slab.grad_of(p).detach().clone() for s in seqs for p in s.parameters()]
    slab.grad.zero_()
    return out


def _fold(slab, sink):
    """What FusedTrainStep._fold_norm does with the sink's descriptors."""
    from rtrec_amd import native
    assert sink.folds, "the joint launch stored no split tiles"
    sumsq = torch.zeros(len(slab.params), dtype=torch.float64, device=slab.grad.device)
    arr = (native.GradFold * len(sink.folds))(*sink.folds)
    native.call("rt_grad_sqnorm_fold", native.ptr(slab.grad), native.ptr(slab.tensor_offsets()), len(slab.params),
                native.ptr(sumsq), None, None, arr, len(sink.folds), native.stream_of(slab.grad))
    torch.cuda.synchronize()
    ref = torch.stack([(slab.grad_of(p).double() ** 2).sum() for p in slab.params])
    torch.testing.assert_close(sumsq, ref, rtol=1e-12, atol=0.0)


def _pair_orders(chains, slab):
    """Gradients of one forward under the three orders: per-layer, joint with
    atomics, joint with stored tiles + fold."""
    from rtrec_amd.models.fused import FoldSink, chain_backward_pair
    seqs = [c.seq for c in chains]
    slab.grad.zero_()
    with _legacy_order():
        chain_backward_pair(chains[0].bwd(slab), chains[1].bwd(slab))
    legacy = _grads_of(slab, seqs)
    chain_backward_pair(chains[0].bwd(slab), chains[1].bwd(slab))
    atomic = _grads_of(slab, seqs)
    sink = FoldSink(slab)
    chain_backward_pair(chains[0].bwd(slab), chains[1].bwd(slab), fold_sink=sink)
    _fold(slab, sink)
    fold = _grads_of(slab, seqs)
    return legacy, atomic, fold


def _pair(device, user_w, item_w, dropout):
    """The C2 pair at minimum batch: B = 32, N = 2 — item rows 96 as BN batches
    32 / 64, user rows 32, both gathered through ids."""
    from rtrec_amd.models.fused import ParamSlab
    g = torch.Generator().manual_seed(3)
    both = nn.ModuleDict({"item": _mlp(item_w, dropout, device, 1), "user": _mlp(user_w, dropout, device, 2)})
    slab = ParamSlab(both).ensure()
    itab = torch.rand(80, item_w[0], generator=g).to(device)
    utab = torch.randn(50, user_w[0], generator=g).to(device)
    iids = torch.randint(0, 80, (96,), generator=g).to(device)
    uids = torch.randint(0, 50, (32,), generator=g).to(device)
    chains = [_Chain(both["item"], itab, iids, 32, 11), _Chain(both["user"], utab, uids, 0, 12)]
    return both, slab, chains


@pytest.mark.parametrize("dropout", [0.0, 0.2])
def test_c2_pair_min_batch(device, dropout):
    """Both tile families in one launch (128x32 fused-dz first layers, 64x64
    for the rest), two BN segments, gathered first layers."""
    both, slab, chains = _pair(device, [3, 256, 128, 128], [20, 256, 128, 128], dropout)
    legacy, atomic, fold = _pair_orders(chains, slab)
    names = [f"{t}.{n}" for t in ("item", "user") for n, _ in both[t].named_parameters()]
    for n, l, a, f in zip(names, legacy, atomic, fold):
        _close(a, l, f"atomic vs per-layer: {n}")
        _close(f, l, f"fold vs per-layer: {n}")
    if dropout == 0.0:
        ref = _autograd(both["item"], chains[0].segments(), chains[0].dout) + \
            _autograd(both["user"], chains[1].segments(), chains[1].dout)
        for n, r, a, f in zip(names, ref, atomic, fold):
            _close(a, r, f"atomic vs autograd: {n}")
            _close(f, r, f"fold vs autograd: {n}")


def test_depth_mismatch_takes_per_layer_path(device):
    """User tower of 2 Linears, item tower of 3: no pairing, the per-layer order."""
    from rtrec_amd.models.fused import FoldSink, chain_backward_pair
    both, slab, chains = _pair(device, [3, 64, 32], [20, 64, 48, 32], 0.0)
    slab.grad.zero_()
    sink = FoldSink(slab)
    chain_backward_pair(chains[0].bwd(slab), chains[1].bwd(slab), fold_sink=sink)
    assert not sink.folds  # nothing left for a fold: the gradients are complete
    got = _grads_of(slab, [c.seq for c in chains])
    ref = _autograd(both["item"], chains[0].segments(), chains[0].dout) + \
        _autograd(both["user"], chains[1].segments(), chains[1].dout)
    for i, (r, a) in enumerate(zip(ref, got)):
        _close(a, r, f"param {i}")


def _single(device, widths, m, with_ids):
    from rtrec_amd.models.fused import ParamSlab, chain_backward
    g = torch.Generator().manual_seed(m)
    seq = _mlp(widths, 0.0, device, 4)
    slab = ParamSlab(seq).ensure()
    if with_ids:
        src = torch.randn(300, widths[0], generator=g).to(device)
        ids = torch.randint(0, 300, (m,), generator=g).to(device)
    else:
        src, ids = torch.randn(m, widths[0], generator=g).to(device), None
    ch = _Chain(seq, src, ids, 0, 21)
    slab.grad.zero_()
    with _legacy_order():
        chain_backward(ch.blocks, ch.ctx, ch.dout, slab)
    legacy = _grads_of(slab, [seq])
    chain_backward(ch.blocks, ch.ctx, ch.dout, slab)
    joint = _grads_of(slab, [seq])
    ref = _autograd(seq, ch.segments(), ch.dout)
    for (n, _), r, l, j in zip(seq.named_parameters(), ref, legacy, joint):
        _close(j, l, f"joint vs per-layer: {n}")
        _close(j, r, f"joint vs autograd: {n}")


@pytest.mark.parametrize("m", [5, 70])
@pytest.mark.parametrize("widths", [[10, 72, 40, 24], [10, 50, 40, 24]])
def test_odd_single_chain(device, m, widths):
    """Below and across one 32-row chunk; width 50 takes the sets the joint
    kernel has no instantiation for (scalar staging loads, a recomputed input,
    an unfused first-layer dz) through their own launches."""
    _single(device, widths, m, False)


def test_id_chain_many_splits(device):
    """4,100 gathered rows: 65 row splits of the first layer, the last of 4 rows."""
    _single(device, [10, 72, 40, 24], 4100, True)


@pytest.mark.parametrize("words", [16, 20])
@pytest.mark.parametrize("splits", [1, 9, 65])
def test_grad_sqnorm_fold_synthetic(device, splits, words):
    from rtrec_amd import native
    rng = np.random.default_rng(splits * 100 + words)
    sizes = [12, words, 7, words]            # tensors 1 and 3 are described, 0 and 2 are not
    offs = np.concatenate([[0], np.cumsum([(s + 3) // 4 * 4 for s in sizes])]).astype(np.int64)
    bounds = [(int(offs[i]), int(offs[i]) + sizes[i]) for i in range(4)]
    g0 = np.zeros(offs[-1], dtype=np.float32)
    for lo, hi in bounds:
        g0[lo:hi] = rng.standard_normal(hi - lo).astype(np.float32)
    parts = [rng.standard_normal((splits, words)).astype(np.float32) for _ in range(2)]
    want = g0.copy()
    for p, t in zip(parts, (1, 3)):
        acc = p[0].copy()
        for s in range(1, splits):
            acc = (acc + p[s]).astype(np.float32)   # ascending split order, fp32
        lo = bounds[t][0]
        want[lo:lo + words] = (g0[lo:lo + words] + acc).astype(np.float32)
    grads = torch.from_numpy(g0).to(device)
    dparts = [torch.from_numpy(p).to(device) for p in parts]
    offsets = torch.tensor([b[0] for b in bounds] + [bounds[-1][1]], dtype=torch.int64, device=device)
    sumsq = torch.zeros(4, dtype=torch.float64, device=device)
    step = torch.full((1,), 5, dtype=torch.int32, device=device)
    seed = torch.full((1,), 9, dtype=torch.int64, device=device)
    folds = (native.GradFold * 2)(native.GradFold(dparts[0].data_ptr(), bounds[1][0], words, splits, 1),
                                  native.GradFold(dparts[1].data_ptr(), bounds[3][0], words, splits, 3))
    native.call("rt_grad_sqnorm_fold", native.ptr(grads), native.ptr(offsets), 4, native.ptr(sumsq),
                native.ptr(step), native.ptr(seed), folds, 2, native.stream_of(grads))
    torch.cuda.synchronize()
    got = grads.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))   # bit-equal, undescribed tensors untouched
    ref = np.array([np.sum(want[lo:hi].astype(np.float64) ** 2) for lo, hi in bounds])
    np.testing.assert_allclose(sumsq.cpu().numpy(), ref, rtol=1e-12, atol=0.0)
    assert int(step.item()) == 6 and int(seed.item()) == 10


# ---------------------------------------------------------------------------
# FusedTrainStep
# ---------------------------------------------------------------------------
def _step_setup(device, batch=64, n_batches=3, seed=4):
    from rtrec_amd.data.movielens import build_batches, feature_tables, synthetic_movielens
    from rtrec_amd.training.utils import create_two_tower_model_for_training
    data = synthetic_movielens(n_users=300, n_movies=400, n_ratings=12000, seed=seed)
    uf, mf = feature_tables(data)
    bu, bp, bn = build_batches(data.train_interactions, data.num_movies, batch, 4, n_batches, seed=9)
    ut, mt = torch.from_numpy(uf).to(device), torch.from_numpy(mf).to(device)
    batches = [tuple(torch.from_numpy(x[i]).to(device) for x in (bu, bp, bn)) for i in range(n_batches)]
    torch.manual_seed(0)
    model = create_two_tower_model_for_training(3, 20, {"embedding_dim": 64, "hidden_layers": [128, 64],
                                                        "dropout_rate": 0.0, "temperature": 0.05}).to(device)
    return ut, mt, batches, model


@pytest.mark.parametrize("disturb", [False, True])
def test_replay_matches_eager(device, disturb):
    """3 steps from one state, eager vs captured and replayed (the loss bar of
    tests/test_gpu_graph.py). ``disturb``: a second FusedTrainStep with a four
    times larger batch runs between the replays; the split tiles belong to each
    step object, so it cannot move or overwrite the captured step's."""
    from rtrec_amd.training.fused_step import FusedTrainStep
    ut, mt, batches, m1 = _step_setup(device)
    m2 = copy.deepcopy(m1)
    eager = FusedTrainStep(m1)
    ref = [eager(ut, mt, mt, user_ids=b[0], pos_ids=b[1], neg_ids=b[2]).clone() for b in batches]
    g = FusedTrainStep(m2)
    st = tuple(t.clone() for t in batches[0])
    g.capture(ut, mt, mt, user_ids=st[0], pos_ids=st[1], neg_ids=st[2], warmup=1)
    assert g._fold.buf is not None  # the single-process step stores and folds its split tiles
    if disturb:
        ut2, mt2, big, m3 = _step_setup(device, batch=256, n_batches=1, seed=5)
        other = FusedTrainStep(m3)
    got = []
    for b in batches:
        for dst, src in zip(st, b):
            dst.copy_(src)
        got.append(g.replay().clone())
        if disturb:
            other(ut2, mt2, mt2, user_ids=big[0][0], pos_ids=big[0][1], neg_ids=big[0][2])
    torch.cuda.synchronize()
    for a, c in zip(ref, got):
        torch.testing.assert_close(c, a, rtol=1e-6, atol=1e-7)


def _step_grads(step, ut, mt, b):
    step._ensure_clean()
    step._grads(ut, mt, mt, b[0], b[1], b[2])
    step._allreduce()
    step._fold_norm()
    torch.cuda.synchronize()
    grads = step.slab.grad.detach().clone()
    step._adam()
    step._clean = True
    return grads


def test_process_group_step_adds_with_atomics(device):
    """With a (one-rank) process group the all-reduce sits between gradients and
    norm: no tiles are stored. Its gradients, the single-process step's (stored
    tiles folded by the norm launch) and the per-layer order's agree."""
    import socket

    import torch.distributed as dist

    from rtrec_amd.training.fused_step import FusedTrainStep
    ut, mt, batches, m1 = _step_setup(device, n_batches=1)
    m2, m3 = copy.deepcopy(m1), copy.deepcopy(m1)
    with _legacy_order():
        ref = _step_grads(FusedTrainStep(m1), ut, mt, batches[0])
    single = FusedTrainStep(m2)
    got_fold = _step_grads(single, ut, mt, batches[0])
    assert single._fold.buf is not None
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        dp = FusedTrainStep(m3, process_group=dist.group.WORLD)
        got_atomic = _step_grads(dp, ut, mt, batches[0])
        assert dp._fold.buf is None and not dp._fold.folds
    finally:
        dist.destroy_process_group()
    for i, (lo, hi) in enumerate(single.slab.bounds):
        _close(got_fold[lo:hi], ref[lo:hi], f"fold vs per-layer: tensor {i}")
        _close(got_atomic[lo:hi], ref[lo:hi], f"atomic vs per-layer: tensor {i}")
