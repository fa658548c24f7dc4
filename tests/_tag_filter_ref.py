"""Numpy restatement of the category filter for the tag-filter tests: the
eligibility rule, the shared fixture (tags and masks over
``_ivf_ref.clustered_corpus()``), and the filter as the exclusion bitmap of the
ineligible items — so the expected results are the existing oracles' own
(``oracle.flat_ip.flat_ip_search(..., exclude_bits=...)``,
``_ivf_ref.probed_lists_search(..., exclude_bits=...)``)."""
import functools

import numpy as np

import _ivf_ref as ref

NLIST, SEED = 64, 1234


def eligible(tags, any_of, none_of):
    """bool [nq, n]: item p is eligible for query q iff
    ``(any_of[q] == 0 or tags[p] & any_of[q]) and not tags[p] & none_of[q]``."""
    tags = np.asarray(tags, dtype=np.uint64)[None, :]
    any_of = np.asarray(any_of, dtype=np.uint64).reshape(-1, 1)
    none_of = np.asarray(none_of, dtype=np.uint64).reshape(-1, 1)
    zero = np.uint64(0)
    return ((any_of == zero) | ((tags & any_of) != zero)) & ((tags & none_of) == zero)


def filter_bits(tags, any_of, none_of, other=None):
    """uint32 [nq, ceil(n / 32)]: bit p of row q set for every INELIGIBLE p, OR-ed
    onto ``other`` (another exclusion bitmap of the same shape)."""
    bits = ref.bitmap_of_excluded(~eligible(tags, any_of, none_of))
    if other is not None:
        bits = bits | np.ascontiguousarray(other).view(np.uint32)
    return bits


def fixture_tags(n):
    """Tags of position p: bits p % 7 and 7 + p % 5; 0 where p % 11 == 0; bit 63
    added where p % 1601 == 3."""
    p = np.arange(n, dtype=np.uint64)
    one = np.uint64(1)
    t = (one << (p % np.uint64(7))) | (one << (np.uint64(7) + p % np.uint64(5)))
    t[p % np.uint64(11) == 0] = 0
    t[p % np.uint64(1601) == 3] |= one << np.uint64(63)
    return t


def fixture_masks(nq):
    """Masks of query q: any_of = 1 << (q % 7), none_of = 1 << (7 + q % 5)."""
    q = np.arange(nq, dtype=np.uint64)
    one = np.uint64(1)
    return one << (q % np.uint64(7)), one << (np.uint64(7) + q % np.uint64(5))


@functools.lru_cache(maxsize=None)
def ivf_fixture():
    """The shared IVF fixture: corpus, queries, the fp64 Lloyd lists (nlist 64,
    seed 1234), tags and masks. Read-only arrays."""
    rows, queries = ref.clustered_corpus()
    cent, assignment = ref.lloyd(rows, ref.initial_positions(len(rows), NLIST, SEED))
    cent = cent.astype(np.float32)
    tags = fixture_tags(len(rows))
    any_of, none_of = fixture_masks(len(queries))
    for a in (cent, assignment, tags, any_of, none_of):
        a.setflags(write=False)
    return dict(rows=rows, queries=queries, centroids=cent, assignment=assignment, tags=tags, any_of=any_of,
                none_of=none_of)


@functools.lru_cache(maxsize=None)
def fixture_probes(nprobe):
    f = ivf_fixture()
    p = ref.coarse_probes(f["queries"], f["centroids"], nprobe)
    p.setflags(write=False)
    return p


def eligible_in_probed(nprobe):
    """int [nq]: eligible rows among the probed lists, per query of the fixture."""
    f = ivf_fixture()
    ok = eligible(f["tags"], f["any_of"], f["none_of"])
    probes = fixture_probes(nprobe)
    return np.array([int((ok[q] & np.isin(f["assignment"], probes[q])).sum()) for q in range(len(probes))])


def as_i64(a):
    """uint64 words as the int64 tensor-friendly view of the same bits."""
    return np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)
