"""The v4 top-K sample planner (csrc/topk_sample_plan.h) as host code of its
own: a stand-alone program (tests/topk_plan_main.cpp) built with g++ under
ASan + UBSan and run as a child process, nothing preloaded and nothing loaded
into Python. Its (stride, rank, sampled, total) per shape are compared with a
model written here from scipy's binomial tail; the program itself asks the
memoised planner twice from each of two threads and fails on any disagreement
or sanitizer report."""
import subprocess

import numpy as np
import pytest
from scipy.stats import binom

from conftest import PKG, REPO

NT = 128          # rows per scan stage
MAX_STRIDE = 64   # RT_TOPK_V4_MAX_STRIDE
APPEND_CAP = 500  # RT_TOPK_V4_APPEND_CAP
KS = (1, 10, 33, 64, 100, 128)


def _split_rows(nx, ways):
    """rows per split of nx rows cut `ways` ways, in whole stages (as plan_v4)"""
    tiles = -(-nx // NT)
    return -(-tiles // ways) * NT


def _shapes():
    cut = [(125_000, _split_rows(125_000, 16)),       # the C4 shard, 16 splits
           (1_000_000, _split_rows(1_000_000, 16)),
           (1_000_000, _split_rows(1_000_000, 2)),
           (65_536, _split_rows(65_536, 16)),
           (65_536, 65_536),
           (1_249, 1_280),                            # one split of 10 stages, the last one ragged
           (3 * 40 * NT + 100, 40 * NT)]              # the last split is a single (ragged) stage
    whole = [(nx, nx) for nx, _ in cut] + [(ips, ips) for _, ips in cut]
    return list(dict.fromkeys(cut + whole))


def _model_stages(nx, ips, stride):
    """every split samples its own stages 0, stride, 2 stride, ..."""
    nst, sps = -(-nx // NT), -(-ips // NT)
    sampled = sum(len(range(0, min(sps, nst - s0), stride)) for s0 in range(0, nst, sps))
    return sampled, nst


def _model_plan(k, nx, ips):
    for stride in range(MAX_STRIDE, 1, -1):
        sampled, nst = _model_stages(nx, ips, stride)
        if sampled < 4:
            continue
        f = sampled / nst
        sf = binom.sf(np.arange(32), k, f)  # sf[r - 1] = P(Bin(k, f) >= r)
        rank = next((r for r in range(1, 33) if r > k or sf[r - 1] <= 1e-6), 0)
        if rank > 0 and rank / f <= APPEND_CAP:
            return stride, rank
    return 0, 0


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("topk_plan") / "topk_plan_main"
    # the sanitizer runtimes linked statically: a dynamic ASan runtime refuses to
    # start when the environment preloads any other library ahead of it
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-pthread", "-I", str(PKG / "csrc"),
                    str(REPO / "tests" / "topk_plan_main.cpp"), "-o", str(exe)], check=True)
    return exe


def test_plan_matches_binomial_model_under_sanitizers(plan_exe):
    grid = [(k, nx, ips) for k in KS for nx, ips in _shapes()]
    run = subprocess.run([str(plan_exe)] + [f"{k}:{nx}:{ips}" for k, nx, ips in grid], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    assert not run.stderr, run.stderr[-4000:]  # a sanitizer report goes to stderr
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == len(grid)
    planned = 0
    for (k, nx, ips), ln in zip(grid, lines):
        stride, rank = _model_plan(k, nx, ips)
        want = (k, nx, ips, stride, rank) + _model_stages(nx, ips, stride or 1)
        assert tuple(int(x) for x in ln.split()) == want, (ln, want)
        planned += stride > 0
    assert planned > len(grid) // 2  # the grid exercises the search, not only "no stride fits"
