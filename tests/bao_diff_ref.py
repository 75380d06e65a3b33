"""The outboard diff restated in plain Python / numpy (include/b3wit.h "outboard diff").  Nothing here calls the library.

The definition read aloud.  G = max(g_a, g_b); a unit is 2^G chunks, the last one of a file possibly ragged.  A unit's CV is STORED as
the file's root where the unit is the whole file, else as the left or right half of the node over the unit's parent subtree; the
outboard of group_log g <= G is the full outboard's pre-order with every node over at most 2^g chunks left out
(bao_groups_ref.filter_full_outboard), so it holds that node.  Unit u of b is SAME iff it exists in a, covers the same chunks in both,
is the whole file in both or in neither, and the two stored CVs are equal; a chunk's bit is its unit's verdict.

  same_chunks()      over the spans of bao_groups_ref.node_spans: any sizes the recursion walks in reasonable time
  places_np()        where every unit's CV is stored, for large chunk counts: the walk down from the root for all units at once (numpy);
                     it needs only the positions, not the hashes
  same_chunks_np()   the definition over places_np, for files of more than 2^G chunks on both sides
  truth()            what the BYTES say: a unit is same iff both files have it with the same extent and every chunk of it has the same
                     bytes (and it is the whole file in both or in neither) - equal to the definition unless BLAKE3 collides"""
import functools

import numpy as np

import bao_groups_ref as GR
import bao_ref as R

CHUNK = R.CHUNK


def unit_span(n, G, u):
    """(first chunk, chunk count) of unit u of a file of n chunks"""
    first = u << G
    return first, min(1 << G, n - first)


@functools.lru_cache(maxsize=None)
def _halves(n, g):
    """{(first chunk, chunk count) of a child: (index of its parent's node in the outboard of group_log g, 0 left / 1 right)}"""
    out = {}
    kept = [(first, m) for first, m in GR.node_spans(n) if m > (1 << g)]
    for i, (first, m) in enumerate(kept):
        k = R._split(m)
        out[(first, k)] = (i, 0)
        out[(first + k, m - k)] = (i, 1)
    return out


def stored_cv(ob, root, n, g, G, u):
    """the 32 bytes stored for unit u (of 2^G chunks) of a file of n chunks whose outboard of group_log g <= G is `ob`, root: 32 bytes"""
    span = unit_span(n, G, u)
    if span == (0, n):
        return bytes(root)
    i, side = _halves(n, g)[span]
    at = 8 + 64 * i + 32 * side
    return bytes(ob[at:at + 32])


def same_chunks(ob_a, len_a, root_a, g_a, ob_b, len_b, root_b, g_b):
    """-> a bool per chunk of b"""
    na, nb, G = R.num_chunks(len_a), R.num_chunks(len_b), max(g_a, g_b)
    out = np.zeros(nb, bool)
    for u in range(GR.num_groups(nb, G)):
        first, m = unit_span(nb, G, u)
        if first >= na or unit_span(na, G, u) != (first, m):
            continue
        if (na <= 1 << G) != (nb <= 1 << G):
            continue
        if stored_cv(ob_a, root_a, na, g_a, G, u) == stored_cv(ob_b, root_b, nb, g_b, G, u):
            out[first:first + m] = True
    return out


def _left_of(cnt):
    """the largest power of two strictly below each cnt >= 2 (int64 array)"""
    k = cnt - 1
    for s in (1, 2, 4, 8, 16, 32):
        k |= k >> s
    return (k + 1) >> 1


def places_np(n, g, G):
    """byte offset, in the outboard of group_log g <= G of a file of n > 2^G chunks, of the stored CV of every unit of 2^G chunks"""
    assert n > 1 << G and g <= G
    total, t = GR.num_groups(n, g), G - g
    a = np.arange(GR.num_groups(n, G), dtype=np.int64) << t
    size = np.minimum(1 << t, total - a)
    p, lo, cnt = np.zeros_like(a), np.zeros_like(a), np.full_like(a, total)
    out = np.full_like(a, -1)
    live = np.ones(a.size, bool)
    while live.any():
        k = _left_of(np.where(live, cnt, 2))
        left = a < lo + k
        clo, ccnt = np.where(left, lo, lo + k), np.where(left, k, cnt - k)
        hit = live & (clo == a) & (ccnt == size)
        out[hit] = 8 + 64 * p[hit] + 32 * (~left[hit])
        live &= ~hit
        p = np.where(live, np.where(left, p + 1, p + k), p)
        lo, cnt = np.where(live, clo, lo), np.where(live, ccnt, cnt)
        assert (cnt[live] > size[live]).all()
    return out


def same_chunks_np(ob_a, na, g_a, ob_b, nb, g_b):
    """same_chunks for outboards as numpy uint8 arrays and files of na, nb > 2^G chunks (no unit is a whole file) -> a bool per chunk of b"""
    G = max(g_a, g_b)
    pa, pb = places_np(na, g_a, G), places_np(nb, g_b, G)
    u = np.arange(pb.size, dtype=np.int64)
    first = u << G
    ok = (first < na) & (np.minimum(first + (1 << G), na) == np.minimum(first + (1 << G), nb))
    u = u[ok]
    cols = np.arange(32, dtype=np.int64)
    eq = (ob_a[pa[u][:, None] + cols] == ob_b[pb[u][:, None] + cols]).all(axis=1)
    unit_same = np.zeros(pb.size, bool)
    unit_same[u] = eq
    return np.repeat(unit_same, 1 << G)[:nb]


def truth(data_a, data_b, G):
    """what the bytes say, for units of 2^G chunks -> a bool per chunk of b"""
    na, nb = R.num_chunks(len(data_a)), R.num_chunks(len(data_b))
    a, b = np.frombuffer(bytes(data_a), dtype=np.uint8), np.frombuffer(bytes(data_b), dtype=np.uint8)
    eq = np.zeros(nb, bool)
    for c in range(min(na, nb)):
        ra, rb = R.chunk_range(len(data_a), c), R.chunk_range(len(data_b), c)
        eq[c] = ra == rb and bool((a[ra[0]:ra[1]] == b[rb[0]:rb[1]]).all())
    out = np.zeros(nb, bool)
    for u in range(GR.num_groups(nb, G)):
        first, m = unit_span(nb, G, u)
        if first < na and unit_span(na, G, u) == (first, m) and (na <= 1 << G) == (nb <= 1 << G) and eq[first:first + m].all():
            out[first:first + m] = True
    return out
