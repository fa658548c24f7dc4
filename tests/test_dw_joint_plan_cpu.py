"""Host-only checks of the joint dW launch's row plan
(rt_linear_bwd_dw_joint_splits: no GPU work, pointers are never dereferenced)."""
import ctypes

import pytest

from conftest import PKG

PTR = 4096  # any 16-B aligned non-null value


@pytest.fixture(scope="module")
def native():
    import subprocess

    from rtrec_amd import native as nat
    if not (PKG / "lib" / "librtrec_hip.so").exists():
        subprocess.run(["make", "-s", "-j8", "-C", str(PKG)], check=True)
    nat.lib()
    return nat


def _set(native, m, k, n, first, last=False):
    a = native.LinearBwdArgs()
    a.m, a.k, a.n = m, k, n
    a.w = a.dw = a.dz_ws = a.src = a.dbias = PTR
    a.ld_src = k
    if last:
        a.grad_mode = 0
        a.dout = a.l2_out = a.norms = PTR
    else:
        a.grad_mode = 1
        a.g = a.z = a.g_stats = a.save_mean = a.save_invstd = a.bn_gamma = PTR
    if first:        # gathered first Linear, dz fused into its dW blocks
        a.fuse_dz = 1
        a.ids = PTR
        a.src_rows = 100
    else:            # staged input rows, a dz launch of its own
        a.prev_mode = 1
        a.prev_mean = a.prev_invstd = a.prev_gamma = a.prev_beta = PTR
        a.g_prev = a.a_in = PTR
    return a


def _pair(native, mi, mu):
    """The C2 towers 3/20 -> 256 -> 128 -> 128, last layer first, item then user."""
    return [_set(native, mi, 128, 128, False, True), _set(native, mu, 128, 128, False, True),
            _set(native, mi, 256, 128, False), _set(native, mu, 256, 128, False),
            _set(native, mi, 20, 256, True), _set(native, mu, 3, 256, True)]


def _splits(native, sets):
    arr = (native.LinearBwdArgs * len(sets))(*sets)
    out = (ctypes.c_int64 * len(sets))()
    rc = native.lib().rt_linear_bwd_dw_joint_splits(arr, len(sets), out)
    return rc, list(out)


def test_c2_plan_fits_two_blocks_per_cu(native):
    sets = _pair(native, 17408, 1024)
    rc, sp = _splits(native, sets)
    assert rc == 0
    tiles = [((a.n + 63) // 64) * ((a.k + 63) // 64) if a.k > 32 else (a.n + 127) // 128 for a in sets]
    assert sum(t * s for t, s in zip(tiles, sp)) <= 512
    # one rows-per-split for the 64x64 sets (a tower's layers 2 and 3 split alike), every row covered
    assert sp[0] == sp[2] and sp[1] == sp[3]
    assert all(s >= 1 for s in sp)
    # the first-layer sets' gather ids fit their LDS stage (<= 2,048 rows per split)
    assert sp[4] * 2048 >= 17408


def test_small_batches_get_whole_chunks(native):
    rc, sp = _splits(native, _pair(native, 96, 32))
    assert rc == 0 and sp == [3, 1, 3, 1, 3, 1]   # 32-row chunks


def test_argument_errors(native):
    L = native.lib()
    sets = _pair(native, 96, 32)
    out = (ctypes.c_int64 * 8)()
    assert L.rt_linear_bwd_dw_joint_splits(None, 1, out) == -1
    seven = (native.LinearBwdArgs * 7)(*(sets + sets[:1]))
    assert L.rt_linear_bwd_dw_joint_splits(seven, 7, out) == -1
    assert L.rt_linear_bwd_dw_f32_joint(seven, 7, None) == -1
    bad = _pair(native, 96, 32)
    bad[0].fold_src = bad[0].fold_dst = PTR     # a fold inside the dW launch: nothing follows to run it
    bad[0].fold_words, bad[0].fold_splits, bad[0].fold_in = 16, 2, 1
    assert _splits(native, bad)[0] == -1
    assert L.rt_grad_sqnorm_fold(None, None, 0, None, None, None, None, 9, None) == -1
