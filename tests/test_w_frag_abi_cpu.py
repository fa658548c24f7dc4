"""Fragment-ordered weight images, the parts that need no GPU: the header
structs and the ctypes mirror agree on the new fields, the host entry
rt_linear_w_frag_bytes returns the image sizes, validate_fwd / validate_bwd
refuse an image pointer on a shape the image does not cover (m = 0: validated,
nothing launched, pointers never dereferenced), and the index arithmetic of
csrc/w_frag.h is a bijection onto the padded matrix (tests/w_frag_layout_main.cpp,
a stand-alone program built with g++)."""
import ctypes
import re
import subprocess

import pytest

from conftest import PKG, REPO

HEADER = REPO / "include" / "rtrec_hip.h"


@pytest.fixture(scope="module")
def native():
    from rtrec_amd import native as nat
    if not (PKG / "lib" / "librtrec_hip.so").exists():
        subprocess.run(["make", "-s", "-j8", "-C", str(PKG)], check=True)
    nat.lib()
    return nat


def _struct_fields(name):
    """Field names of a header struct, in declaration order."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", text, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        for part in decl.split(","):
            m = re.search(r"(\w+)\s*(?:\[[^\]]*\])?\s*$", part.strip())
            if m and part.strip():
                names.append(m.group(1))
    return names


def test_header_and_ctypes_agree_on_the_image_fields(native):
    fwd = _struct_fields("rt_linear_fwd_args")
    bwd = _struct_fields("rt_linear_bwd_args")
    assert fwd == [f for f, _ in native.LinearFwdArgs._fields_]
    assert bwd == [f for f, _ in native.LinearBwdArgs._fields_]
    assert fwd[-3:] == ["w_frag", "next_w_frag", "wt_frag_out"]
    assert bwd[-1] == "wt_frag"
    for cls, names in ((native.LinearFwdArgs, fwd[-3:]), (native.LinearBwdArgs, bwd[-1:])):
        for f in names:
            assert getattr(cls, f).size == ctypes.sizeof(ctypes.c_void_p)
    assert "rt_linear_w_frag_bytes" in native.SIGNATURES


def _ceil(a, b):
    return -(-a // b)


def test_image_sizes(native):
    wb = native.lib().rt_linear_w_frag_bytes
    for n, k in ((128, 256), (128, 128), (96, 64), (100, 96), (256, 40), (64, 256), (8, 8), (256, 256)):
        # forward: float4 [T][S][4][64], T = ceil(n/32), S = pad(k)/32
        assert wb(n, k, 0) == _ceil(n, 32) * _ceil(k, 32) * 4 * 64 * 16, (n, k)
        assert wb(n, k, 0) == 32 * _ceil(n, 32) * 32 * _ceil(k, 32) * 4
    for n, k in ((128, 256), (128, 128), (96, 64), (104, 96), (256, 40), (64, 250), (8, 3)):
        # dz: float4 [KT][NS][2][64], KT = ceil(k/32), NS = pad(n)/16
        assert wb(n, k, 1) == _ceil(k, 32) * (32 * _ceil(n, 32) // 16) * 2 * 64 * 16, (n, k)
    # whole tiles: n · pad(k) · 4 bytes
    assert wb(128, 256, 0) == 128 * 256 * 4 and wb(128, 256, 1) == 128 * 256 * 4
    assert wb(128, 40, 0) == 128 * 64 * 4
    # shapes without an image
    assert wb(128, 50, 0) == 0 and wb(128, 20, 0) == 0 and wb(512, 64, 0) == 0
    assert wb(50, 64, 1) == 0 and wb(100, 64, 1) == 0 and wb(128, 512, 1) == 0
    assert wb(0, 64, 0) == 0 and wb(64, 0, 1) == 0 and wb(-8, 64, 0) == 0


P = 4096  # a 16-byte aligned dummy address (m = 0: never dereferenced)


def _fwd(native, n, k, **kw):
    a = native.LinearFwdArgs()
    a.m, a.k, a.n, a.ld_src = 0, k, n, k
    a.src, a.w = P, P
    for f, v in kw.items():
        setattr(a, f, v)
    return native.lib().rt_linear_fwd_f32(ctypes.byref(a), None)


def _bwd(native, n, k, **kw):
    a = native.LinearBwdArgs()
    a.m, a.k, a.n, a.ld_src = 0, k, n, k
    a.w = a.dw = a.dz_ws = a.src = a.g = a.z = a.g_prev = P
    a.grad_mode = 3
    for f, v in kw.items():
        setattr(a, f, v)
    return native.lib().rt_linear_bwd_dz_f32(ctypes.byref(a), None)


def test_validate_refuses_images_on_uncovered_shapes(native):
    assert _fwd(native, 128, 256) == 0
    assert _fwd(native, 128, 256, w_frag=P) == 0
    assert _fwd(native, 256, 40, w_frag=P) == 0
    assert _fwd(native, 128, 50, w_frag=P) == -1          # k % 8 != 0
    assert _fwd(native, 128, 20, w_frag=P) == -1
    assert _fwd(native, 384, 64, w_frag=P) == -1          # n > 256: no image instance
    assert _fwd(native, 128, 256, w_frag=P + 4) == -1     # misaligned image
    assert _fwd(native, 128, 256, w_frag=P, w=P + 4) == -1
    # side tasks
    assert _fwd(native, 128, 20, next_w=P, next_w_frag=P, next_n=128, next_k=256) == 0
    assert _fwd(native, 128, 20, next_w=P, next_w_frag=P, next_n=128, next_k=50) == -1
    assert _fwd(native, 128, 20, next_w_frag=P, next_n=128, next_k=256) == -1   # no source weight
    assert _fwd(native, 128, 20, next_w=P, next_w_frag=P + 8, next_n=128, next_k=256) == -1
    assert _fwd(native, 128, 256, wt_frag_out=P) == 0
    assert _fwd(native, 100, 256, wt_frag_out=P) == -1    # n % 8 != 0
    assert _fwd(native, 128, 256, wt_frag_out=P + 4) == -1
    # backward
    assert _bwd(native, 128, 256) == 0
    assert _bwd(native, 128, 256, wt_frag=P) == 0
    assert _bwd(native, 96, 64, wt_frag=P) == 0
    assert _bwd(native, 100, 64, wt_frag=P) == -1         # n % 8 != 0
    assert _bwd(native, 50, 64, wt_frag=P) == -1
    assert _bwd(native, 128, 512, wt_frag=P) == -1        # k > 256: the four-tile instance reads no image
    assert _bwd(native, 128, 256, wt_frag=P + 4) == -1


def test_layout_is_a_bijection(tmp_path):
    exe = tmp_path / "w_frag_layout_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-I", str(PKG / "csrc"),
                    str(REPO / "tests" / "w_frag_layout_main.cpp"), "-o", str(exe)], check=True)
    shapes = [(96, 40), (100, 128), (128, 256), (256, 64)]
    run = subprocess.run([str(exe)] + [f"{n}:{k}" for n, k in shapes], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == len(shapes)
    for (n, k), ln in zip(shapes, lines):
        f = ln.split()
        assert f[-1] == "ok" and int(f[0]) == n and int(f[1]) == k
        assert int(f[2]) * 4 == 32 * _ceil(n, 32) * 32 * _ceil(k, 32)
        assert int(f[3]) * 4 == 32 * _ceil(k, 32) * 32 * _ceil(n, 32)
