"""rt_tower_infer_f32 alone (one launch: the whole eval-mode tower for 1..8
rows) against ``oracle.tower_forward(train=False)`` on the module's
``state_dict``, with BatchNorm running statistics, gamma, beta and the Linear
biases randomised.

Bars (the project's own): outputs within 1e-4 * max|ref| of the oracle
(DESIGN.md §3), and on 512 rows of the 256 -> [256, 128] -> 128 tower the bar of
``test_tower_forward_is_fp32_class``. Row independence is exact: a row's bits
depend neither on m nor on its slot."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

# (input k0, hidden, emb): the smallest shapes that reach every code path
SHAPES = {
    "c2_user": (3, [256, 128], 128),        # the C2 user tower; dword path, k < 4
    "service": (10, [512, 256, 128], 128),  # service default; the 512 maximum
    "odd": (50, [50, 130], 24),             # k % 4 != 0 inside; n no multiple of the wave count; column tails
    "max": (512, [512], 512),               # both maxima
    "single": (8, [], 16),                  # a single Linear, no BN
}
TABLE_ROWS = 100


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import native
    native.lib()
    return native


def _module(k0, hidden, emb, act="relu", seed=0):
    from rtrec_amd.models.two_tower import UserTower
    torch.manual_seed(seed)
    t = UserTower(k0, emb, list(hidden), dropout_rate=0.0, activation=act)
    with torch.no_grad():
        for mod in t.mlp:
            if isinstance(mod, nn.BatchNorm1d):
                mod.running_mean.uniform_(-0.5, 0.5)
                mod.running_var.uniform_(0.5, 2.0)
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.5, 0.5)
            elif isinstance(mod, nn.Linear):
                mod.bias.uniform_(-0.1, 0.1)
    return t.eval()


class Case:
    """A tower's state (CPU for the oracle, device for the kernel), a 100-row
    table of inputs and the oracle's output for every table row, computed once."""

    def __init__(self, nat, k0, hidden, emb, act="relu", seed=0, rows=TABLE_ROWS):
        from oracle import two_tower as orc
        self.nat, self.act, self.n_hidden, self.emb, self.k0 = nat, act, len(hidden), emb, k0
        mod = _module(k0, hidden, emb, act, seed)
        self.module = mod
        self.state = {k: v.clone() for k, v in mod.state_dict().items()}
        self.dev = {k: v.cuda().contiguous() for k, v in self.state.items() if v.dtype == torch.float32}
        g = torch.Generator().manual_seed(seed + 100)
        self.table = torch.randn(rows, k0, generator=g)
        self.table_dev = self.table.cuda()
        with torch.no_grad():
            self.ref = orc.tower_forward(self.state, self.table, train=False, activation=act).numpy()
        self.ref.setflags(write=False)

    def args(self, m, src, src_rows, ids, out, norms=None, normalize=1):
        nat = self.nat
        a = nat.TowerInferArgs()
        a.src, a.src_rows, a.ld_src, a.ids = nat.ptr(src), src_rows, self.k0, nat.ptr(ids)
        a.m, a.n_layers, a.normalize = m, self.n_hidden + 1, normalize
        a.out, a.norms_out = nat.ptr(out), nat.ptr(norms)
        for l in range(self.n_hidden + 1):
            L, w = a.layers[l], self.dev[f"mlp.{4 * l}.weight"]
            L.w, L.bias, L.k, L.n = nat.ptr(w), nat.ptr(self.dev[f"mlp.{4 * l}.bias"]), w.shape[1], w.shape[0]
            L.act = nat.ACTS["none"]
            if l < self.n_hidden:
                bn = f"mlp.{4 * l + 2}"
                L.act = nat.ACTS[self.act]
                L.bn_gamma, L.bn_beta = nat.ptr(self.dev[f"{bn}.weight"]), nat.ptr(self.dev[f"{bn}.bias"])
                L.bn_mean, L.bn_var = nat.ptr(self.dev[f"{bn}.running_mean"]), nat.ptr(self.dev[f"{bn}.running_var"])
                L.bn_eps = 1e-5
        return a

    def by_ids(self, ids, normalize=1, want_norms=False, out_rows=None):
        """Rows ``ids`` of the table through the fused gather: (rc, out, norms)."""
        m = len(ids)
        ids_dev = torch.tensor(ids, dtype=torch.int64, device="cuda")
        out = torch.full((out_rows or m, self.emb), 7.5, dtype=torch.float32, device="cuda")
        norms = torch.full((8,), -1.0, dtype=torch.float32, device="cuda") if want_norms else None
        a = self.args(m, self.table_dev, self.table_dev.shape[0], ids_dev, out, norms, normalize)
        rc = self.nat.lib().rt_tower_infer_f32(ctypes.byref(a), self.nat.stream_of(out))
        torch.cuda.synchronize()
        return rc, out.cpu().numpy(), (norms.cpu().numpy() if want_norms else None)

    def by_rows(self, x_dev, m):
        """The first m rows of ``x_dev`` without ids."""
        out = torch.empty((m, self.emb), dtype=torch.float32, device="cuda")
        a = self.args(m, x_dev, x_dev.shape[0], None, out)
        rc = self.nat.lib().rt_tower_infer_f32(ctypes.byref(a), self.nat.stream_of(out))
        torch.cuda.synchronize()
        return rc, out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(nat, name, act="relu"):
    return Case(nat, *SHAPES[name], act=act)


def _close(got, ref):
    tol = 1e-4 * np.abs(ref).max()
    err = np.abs(got - ref).max()
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("m", range(1, 9))
@pytest.mark.parametrize("name", list(SHAPES))
def test_matches_oracle(nat, name, m):
    c = _case(nat, name)
    ids = [(17 * i + 3 * m) % TABLE_ROWS for i in range(m)]
    rc, out, _ = c.by_ids(ids)          # through ids into the 100-row table
    assert rc == 0
    _close(out, c.ref[ids])
    rc, out2 = c.by_rows(c.table_dev[ids].contiguous(), m)   # the same rows without ids: the same bits
    assert rc == 0
    assert np.array_equal(out, out2)


@pytest.mark.parametrize("act", ["relu", "gelu", "leaky_relu", "tanh", "sigmoid"])
def test_activations(nat, act):
    c = _case(nat, "odd", act)
    ids = [5, 99, 0, 42, 7]
    rc, out, _ = c.by_ids(ids)
    assert rc == 0
    _close(out, c.ref[ids])


@pytest.mark.parametrize("name", ["odd", "service"])
def test_normalize_flag_and_norms_out(nat, name):
    c = _case(nat, name)
    ids = [1, 2, 3]
    _, unit, none = c.by_ids(ids)
    assert none is None
    _close(unit, c.ref[ids])
    _, unit_n, norms1 = c.by_ids(ids, want_norms=True)
    _, raw, norms0 = c.by_ids(ids, normalize=0, want_norms=True)
    _, raw_only, _ = c.by_ids(ids, normalize=0)
    assert np.array_equal(unit_n, unit) and np.array_equal(raw_only, raw)   # norms_out changes nothing else
    assert np.array_equal(norms0, norms1) and np.all(norms0[3:] == -1.0)     # [m] written, no more
    ref_norm = np.linalg.norm(raw.astype(np.float64), axis=1)
    assert np.abs(norms0[:3] - ref_norm).max() <= 1e-6 * ref_norm.max()
    _close(raw / np.maximum(norms0[:3, None], 1e-12), c.ref[ids])          # the raw rows are the oracle's, unnormalised
    assert np.abs(np.linalg.norm(unit.astype(np.float64), axis=1) - 1).max() < 1e-6


def test_fp32_class_bar_on_512_rows(nat):
    """The bar of test_tower_forward_is_fp32_class on 512 rows of the
    256 -> [256, 128] -> 128 tower, as 64 calls of 8: max error against the
    float64 module <= 4 x torch-CPU-fp32's max error + 1e-7, and < 2e-6."""
    c = Case(nat, 256, [256, 128], 128, seed=7, rows=512)
    x = c.table
    ref_mlp = copy.deepcopy(c.module.mlp).double()
    with torch.no_grad():
        z64 = ref_mlp(x.double())
        ref = z64 / z64.norm(dim=1, keepdim=True)
        z32 = copy.deepcopy(c.module.mlp)(x)
        cpu32 = z32 / z32.norm(dim=1, keepdim=True)
    out = torch.empty((512, 128), dtype=torch.float32, device="cuda")
    for i in range(64):
        a = c.args(8, c.table_dev[8 * i:], 8, None, out[8 * i:])
        assert nat.lib().rt_tower_infer_f32(ctypes.byref(a), nat.stream_of(out)) == 0
    got = out.cpu().double()
    err_dev = (got - ref).abs().max().item()
    err_cpu = (cpu32.double() - ref).abs().max().item()
    print(f"err_dev {err_dev:.3e} err_cpu {err_cpu:.3e}")
    assert err_dev <= 4 * err_cpu + 1e-7, (err_dev, err_cpu)
    assert err_dev < 2e-6, err_dev


@pytest.mark.parametrize("name", list(SHAPES))
def test_row_independence_is_exact(nat, name):
    """Every row of an m = 8 call is bit-equal to that row computed alone with
    m = 1, and to that row in another slot of calls with other m."""
    c = _case(nat, name)
    ids = [11, 3, 97, 50, 0, 64, 29, 8]
    _, full, _ = c.by_ids(ids)
    for slot, i in enumerate(ids):
        _, alone, _ = c.by_ids([i])
        assert np.array_equal(alone[0], full[slot]), (name, slot)
    rev = ids[::-1]
    _, out, _ = c.by_ids(rev)
    assert np.array_equal(out, full[::-1])
    for m in (2, 3, 4, 5, 7):                       # every instantiation, rows shifted by one slot
        sub = (ids[1:] + ids[:1])[:m]
        _, out, _ = c.by_ids(sub)
        assert np.array_equal(out, full[[ids.index(i) for i in sub]]), (name, m)


def test_rows_past_m_are_not_written(nat):
    c = _case(nat, "odd")
    rc, out, _ = c.by_ids([4, 5, 6], out_rows=8)
    assert rc == 0
    _close(out[:3], c.ref[[4, 5, 6]])
    assert np.all(out[3:] == 7.5)


def test_bad_ids_read_a_zero_row(nat):
    c = _case(nat, "c2_user")
    zero = torch.zeros((1, c.k0), dtype=torch.float32, device="cuda")
    rc, want = c.by_rows(zero, 1)
    assert rc == 0
    rc, out, _ = c.by_ids([7, TABLE_ROWS, -1, 9])
    assert rc == 0
    assert np.array_equal(out[1], want[0]) and np.array_equal(out[2], want[0])
    _close(out[[0, 3]], c.ref[[7, 9]])


def test_zero_last_layer_gives_zeros_not_nan(nat):
    c = Case(nat, 8, [16], 16, seed=3)
    last = f"mlp.{4 * c.n_hidden}"
    c.dev[f"{last}.weight"].zero_()
    c.dev[f"{last}.bias"].zero_()
    rc, out, norms = c.by_ids([0, 1], want_norms=True)
    assert rc == 0
    assert np.all(out == 0.0) and np.all(norms[:2] == 0.0)
