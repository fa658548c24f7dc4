"""rt_grad_sqnorm / rt_clip_adam_step at the C-ABI boundary, without a GPU:
every argument error comes back as RT_ERR_INVALID before any device work (the
pointers are dummies that are never dereferenced), empty calls are RT_OK
without a launch, and the ctypes signatures carry the header's arguments."""
import ctypes
import re
import subprocess

import pytest

from conftest import PKG, REPO

RT_OK, RT_ERR_INVALID = 0, -1
P, G, M, V, SUMSQ, OFFS, ZBUF, DEV = (ctypes.c_void_p(a) for a in
                                      (0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000,
                                       0x70000000, 0x80000000))


@pytest.fixture(scope="module")
def native():
    from rtrec_amd import native as nat
    if not (PKG / "lib" / "librtrec_hip.so").exists():
        subprocess.run(["make", "-s", "-j8", "-C", str(PKG)], check=True)
    nat.lib()
    return nat


def test_grad_sqnorm_argument_errors(native):
    L = native.lib()

    def sqnorm(grads=G, offsets=OFFS, n_tensors=3, sumsq=SUMSQ, step=None, seed=None):
        return L.rt_grad_sqnorm(grads, offsets, n_tensors, sumsq, step, seed, None)

    assert sqnorm(n_tensors=-1) == RT_ERR_INVALID
    assert sqnorm(grads=None) == RT_ERR_INVALID
    assert sqnorm(offsets=None) == RT_ERR_INVALID
    assert sqnorm(sumsq=None) == RT_ERR_INVALID
    assert sqnorm(step=DEV, seed=DEV, sumsq=None) == RT_ERR_INVALID      # counters do not rescue a bad call
    # nothing to do: RT_OK without a launch, every pointer null
    assert sqnorm(grads=None, offsets=None, n_tensors=0, sumsq=None) == RT_OK
    assert sqnorm(n_tensors=0) == RT_OK
    with pytest.raises(native.RTError):
        native.call("rt_grad_sqnorm", None, OFFS, 3, SUMSQ, None, None, None)


def _adam(L, p=P, g=G, m=M, v=V, n=0, sumsq=SUMSQ, n_tensors=1, max_norm=1.0, lr=1e-3, lr_dev=None, b1=0.9,
          b2=0.999, eps=1e-8, wd=1e-5, step=1, step_dev=None, zero_buf=None, zero_words=0):
    """n defaults to 0: a call that passes the argument check returns before any launch."""
    return L.rt_clip_adam_step(p, g, m, v, n, sumsq, n_tensors, max_norm, lr, lr_dev, b1, b2, eps, wd, step,
                               step_dev, zero_buf, zero_words, None)


def test_clip_adam_argument_errors(native):
    L = native.lib()
    assert _adam(L) == RT_OK                                             # n == 0
    assert _adam(L, n=-1) == RT_ERR_INVALID
    for name in ("p", "g", "m", "v", "sumsq"):
        assert _adam(L, **{name: None}) == RT_ERR_INVALID, name
        assert _adam(L, n=1000, **{name: None}) == RT_ERR_INVALID, name
    for n_tensors in (0, -1):
        assert _adam(L, n_tensors=n_tensors) == RT_ERR_INVALID, n_tensors
    for step in (0, -1):
        assert _adam(L, step=step) == RT_ERR_INVALID, step               # no device counter: step >= 1
        assert _adam(L, step=step, step_dev=DEV) == RT_OK, step          # the device counter takes precedence
    assert _adam(L, zero_buf=ZBUF, zero_words=-1) == RT_ERR_INVALID
    assert _adam(L, zero_words=-1) == RT_ERR_INVALID
    assert _adam(L, zero_buf=None, zero_words=8) == RT_ERR_INVALID
    # accepted: a buffer with nothing to zero, a device learning rate, nothing at all to zero
    assert _adam(L, zero_buf=ZBUF, zero_words=0) == RT_OK
    assert _adam(L, zero_buf=ZBUF, zero_words=5000, lr_dev=DEV, step_dev=DEV) == RT_OK
    with pytest.raises(native.RTError):
        native.call("rt_clip_adam_step", P, G, M, V, 0, SUMSQ, 0, 1.0, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 1, None,
                    None, 0, None)


def test_ctypes_signatures_match_header(native):
    """Argument for argument: pointers as void*, the element counts as int64,
    the hyperparameters as float (the kernel's arithmetic depends on that)."""
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "rtrec_hip.h").read_text(), flags=re.S)
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    for name in ("rt_grad_sqnorm", "rt_clip_adam_step"):
        m = re.search(r"^\s*int\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.M | re.S)
        assert m, name
        want = []
        for param in m.group(1).split(","):
            words = param.replace("*", " * ").split()
            want.append(ctypes.c_void_p if "*" in words else kinds[[w for w in words if w != "const"][0]])
        res, args = native.SIGNATURES[name]
        assert res is ctypes.c_int
        assert len(args) == len(want), (name, len(args), len(want))
        assert list(args) == want, name
