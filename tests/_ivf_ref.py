"""Numpy restatement of the IVF-Flat index for the IVF tests: the clustered
corpus generator, Lloyd's steps in fp64, and the "probed-lists search" that
defines what rt_ivf_topk and HipIVFFlatIndex must return. No Faiss, nothing
from the reference: an IVF search IS the Flat search (oracle/flatip.c)
restricted to the rows of the probed lists, so the expected scores and ids
are the oracle's own bits."""
import functools

import numpy as np

from oracle import flat_ip as orc


def unit_rows(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def clustered_corpus(n=8192, d=32, n_centres=64, n_queries=256, seed=0):
    """(rows [n, d], queries [n_queries, d]) fp32, unit norm: ``n_centres``
    unit-norm Gaussian centres, row = centre + 0.7 N(0, I) / sqrt(d)
    renormalised, query = a corpus row + 0.05 noise, renormalised."""
    rng = np.random.default_rng(seed)
    centres = unit_rows(rng.standard_normal((n_centres, d)))
    which = rng.integers(0, n_centres, n)
    rows = unit_rows(centres[which] + 0.7 * rng.standard_normal((n, d)) / np.sqrt(d))
    pick = rng.choice(n, n_queries, replace=False)
    queries = unit_rows(rows[pick] + 0.05 * rng.standard_normal((n_queries, d)))
    rows, queries = rows.astype(np.float32), queries.astype(np.float32)
    rows.setflags(write=False)
    queries.setflags(write=False)
    return rows, queries


def initial_positions(n, nlist, seed):
    """The rows HipIVFFlatIndex starts its centroids from: the first nlist entries
    of the seeded CPU permutation of the n positions."""
    import torch
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:nlist].numpy()


def assign(rows, centroids):
    """Nearest centroid by inner product in fp64, the lowest centroid id winning ties."""
    return np.argmax(rows.astype(np.float64) @ centroids.astype(np.float64).T, axis=1)


def lloyd(rows, init_positions, iters=10, normalize=True):
    """fp64 k-means: assign, mean (renormalised for the cosine metric); an empty
    list keeps its centroid. Returns (centroids fp64, final assignment)."""
    x = rows.astype(np.float64)
    c = x[np.asarray(init_positions)].copy()
    for _ in range(iters):
        a = assign(x, c)
        for l in range(c.shape[0]):
            m = a == l
            if m.any():
                v = x[m].mean(axis=0)
                if normalize:
                    nv = np.linalg.norm(v)
                    v = v / nv if nv > 0 else v
                c[l] = v
    return c, assign(x, c)


def bitmap_of_excluded(mask):
    """uint32 [nq, ceil(n / 32)] from a bool [nq, n] mask: bit j of row q = item j skipped."""
    nq, n = mask.shape
    words = (n + 31) // 32
    padded = np.zeros((nq, words * 32), dtype=bool)
    padded[:, :n] = mask
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view(np.uint32)


def probed_lists_search(queries, rows, assignment, probes, k, exclude_bits=None, dtype_code=None):
    """Flat search of ``queries`` over ``rows`` (both as the oracle takes them,
    original order) restricted to the rows whose list is in the query's probe
    row (``probes`` [nq, nprobe], -1 / out-of-range entries name no list),
    OR-ed with the call's own ``exclude_bits``."""
    assignment = np.asarray(assignment)
    mask = np.ones((len(probes), len(assignment)), dtype=bool)
    for q, pr in enumerate(np.asarray(probes)):
        mask[q] = ~np.isin(assignment, pr)
    bits = bitmap_of_excluded(mask)
    if exclude_bits is not None:
        bits = bits | np.ascontiguousarray(exclude_bits).view(np.uint32)
    return orc.flat_ip_search(queries, rows, k, exclude_bits=bits, dtype_code=dtype_code, nthreads=16)


def coarse_probes(queries_f32, centroids_f32, nprobe):
    """Top-nprobe lists per query: the Flat oracle over the centroids."""
    return orc.flat_ip_search(np.ascontiguousarray(queries_f32, dtype=np.float32),
                              np.ascontiguousarray(centroids_f32, dtype=np.float32), nprobe, nthreads=16)[1]


def ivf_search(queries, rows, centroids, assignment, nprobe, k, exclude_bits=None):
    """The whole fp32 IVF search of the reference model."""
    probes = coarse_probes(queries, centroids, nprobe)
    return probed_lists_search(np.ascontiguousarray(queries), np.ascontiguousarray(rows), assignment, probes, k,
                               exclude_bits=exclude_bits)


def recall_at_k(got_ids, want_ids):
    """Mean over queries of |got ∩ want| / |want| (ids < 0 are pads)."""
    tot = 0.0
    for g, w in zip(got_ids, want_ids):
        w = set(int(i) for i in w if i >= 0)
        tot += len(w & set(int(i) for i in g if i >= 0)) / max(len(w), 1)
    return tot / len(want_ids)
