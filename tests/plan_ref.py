"""The chained-mode planner restated in numpy: every step record of every chunk path of a preimage, from two rules only —
BLAKE3's tree ("the left subtree takes the largest power of two below the chunk count", BLAKE3 specification 2.4-2.6) and
the reference driver's way of walking a path (the PathNode at height g gives its RIGHT half where bit g of the chunk
index is clear, else its LEFT half: rust_fold/src/blake3_hash.rs:58-84, as tests/bao_ref.py::siblings_for reads it).  The record
layouts are those of include/b3wit.h (b3w_chain_plan_leaves_device / b3w_chain_plan_parents_device).  No segment, spine or row
arithmetic: the tree is a plain recursion, a path is "follow the parent pointers", rows follow chunk order because the records
are laid down chunk by chunk.  Test infrastructure: the checker of csrc/b3w_plan.hip and csrc/b3w_chain.cpp."""
import sys
from types import SimpleNamespace

import numpy as np

import blake3_ref as B

_IV = np.array(B.IV, dtype=np.uint32)


def path_len(chunk, n_chunks):
    """parents above `chunk` in the tree over n_chunks chunks (a direct walk from the root)"""
    p = 0
    while n_chunks > 1:
        k = 1 << ((n_chunks - 1).bit_length() - 1)          # the largest power of two below n_chunks
        if chunk < k:
            n_chunks = k
        else:
            chunk, n_chunks = chunk - k, n_chunks - k
        p += 1
    return p


def _tree_shape(n):
    """BLAKE3's tree over chunks 0 .. n - 1 as arrays over node ids: leaves are 0 .. n - 1, the root is the last node.
    -> left, right (children; -1 for leaves), up (parent; -1 for the root), rank (0 for leaves, else 1 + the larger child rank)"""
    left, right, rank = [-1] * n, [-1] * n, [0] * n

    def build(lo, m):
        if m == 1:
            return lo
        k = 1 << ((m - 1).bit_length() - 1)
        a, b = build(lo, k), build(lo + k, m - k)
        left.append(a)
        right.append(b)
        rank.append(1 + max(rank[a], rank[b]))
        return len(left) - 1

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 200))
    try:
        root = build(0, n)
    finally:
        sys.setrecursionlimit(limit)
    assert root == len(left) - 1
    left, right, rank = np.array(left, dtype=np.int64), np.array(right, dtype=np.int64), np.array(rank, dtype=np.int64)
    up = np.full(left.size, -1, dtype=np.int64)
    inner = np.nonzero(left >= 0)[0]
    up[left[inner]] = inner
    up[right[inner]] = inner
    return left, right, up, rank


def _leaves(data, first_chunk, plen):
    """leaf records [n, 16, 32] (rows past a chunk's last block stay zero), blocks per chunk [n], chunk CVs [n, 8]"""
    n = plen.size
    padded = np.zeros(n * 1024, dtype=np.uint8)
    padded[:data.size] = data
    words = padded.view("<u4").reshape(n, 16, 16)
    idx = np.arange(n, dtype=np.uint64) + np.uint64(first_chunk)
    t0, t1 = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32)
    nbytes = np.full(n, 1024, dtype=np.int64)
    nbytes[-1] = data.size - (n - 1) * 1024                   # only the last chunk of the preimage may be short
    n_blocks = np.maximum((nbytes + 63) // 64, 1)
    recs = np.zeros((n, 16, 32), dtype=np.uint32)
    cv = np.tile(_IV, (n, 1))
    for j in range(int(n_blocks.max())):
        on = n_blocks > j
        bb = np.clip(nbytes - 64 * j, 0, 64).astype(np.uint32)
        last = n_blocks - 1 == j
        d = ((B.CHUNK_START if j == 0 else 0) + B.CHUNK_END * last + B.ROOT * (last & (plen == 0))).astype(np.uint32)
        r = recs[:, j, :]
        r[on, 0], r[on, 1] = n_blocks[on], j
        r[on, 2:10] = cv[on]
        r[on, 10], r[on, 11] = t0[on], t1[on]
        r[on, 12], r[on, 13], r[on, 14] = plen[on] + 1, plen[on] + 1, plen[on]
        r[on, 15:31] = words[on, j, :]
        r[on, 31] = bb[on]
        cv[on] = B._compress_np(cv[on], words[on, j, :], t0[on], t1[on], bb[on], d[on])
    return recs, n_blocks.astype(np.uint32), cv


def plan(data, first_chunk=0, preimage_len=None, parents_of=None):
    """data: uint8 array.  With preimage_len None it is the whole preimage (first_chunk must be 0): leaf records, chunk CVs, the tree,
    the root and the parent records.  With preimage_len given, data holds the bytes from first_chunk * 1024 to the end of a chunk
    range of a preimage that long (the last local chunk short only if it is the preimage's last): leaf records and chunk CVs only.
    parents_of: the chunks whose parent records are wanted (default: all).

    -> leaf [n, 16, 32], n_blocks [n], cvs [n, 8], root [8], parents [rows, 32] (the selected chunks in order, each bottom up),
       parent_first [len(selected) + 1] (rows of chunk i: parent_first[i] .. parent_first[i + 1]), final [len(selected), 8] (the
       running value after a chunk's last step), plen [n] (path lengths of the n chunks), records_of(lo, hi) (the record rows of the
       chunk range [lo, hi) the way the planner and the driver lay them down: leaf rows, then parent rows)"""
    data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    whole = preimage_len is None
    total = data.size if whole else int(preimage_len)
    assert total > 0 and data.size > 0 and (not whole or first_chunk == 0)
    n_total = (total + 1023) // 1024
    n = (data.size + 1023) // 1024
    assert first_chunk + n <= n_total and (data.size % 1024 == 0 or first_chunk * 1024 + data.size == total)
    out = SimpleNamespace(n_chunks=n_total, first_chunk=first_chunk)
    if not whole:
        out.plen = np.array([path_len(first_chunk + i, n_total) for i in range(n)], dtype=np.int64)
        out.leaf, out.n_blocks, out.cvs = _leaves(data, first_chunk, out.plen)
        return out

    left, right, up, rank = _tree_shape(n)
    # path lengths: the number of parent pointers between a leaf and the root
    cur, plen = np.arange(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    paths = []                                                # paths[g][c] = the node at height g of chunk c's path (-1: above the root)
    while True:
        cur = np.where(cur >= 0, up[np.maximum(cur, 0)], -1)
        if (cur < 0).all():
            break
        paths.append(cur)
        plen += cur >= 0
    out.plen = plen
    out.leaf, out.n_blocks, out.cvs = _leaves(data, 0, plen)

    # node CVs, rank by rank (a node's children have smaller ranks)
    cv = np.zeros((left.size, 8), dtype=np.uint32)
    cv[:n] = out.cvs
    root_id = left.size - 1
    for r in range(1, int(rank.max()) + 1):
        ids = np.nonzero(rank == r)[0]
        d = np.where(ids == root_id, B.PARENT | B.ROOT, B.PARENT).astype(np.uint32)
        cv[ids] = B._compress_np(np.tile(_IV, (ids.size, 1)), np.concatenate([cv[left[ids]], cv[right[ids]]], axis=1), 0, 0, 64, d)
    out.root = cv[root_id].copy()

    sel = np.arange(n, dtype=np.int64) if parents_of is None else np.asarray(list(parents_of), dtype=np.int64)
    spl = plen[sel]
    first = np.concatenate([[0], np.cumsum(spl)]).astype(np.int64)
    par = np.zeros((int(first[-1]), 32), dtype=np.uint32)
    h = out.cvs[sel].copy()
    chunk = sel.astype(np.uint64)
    for g in range(len(paths)):
        on = spl > g
        if not on.any():
            break
        node = paths[g][sel[on]]
        clear = ((chunk[on] >> np.uint64(g)) & np.uint64(1)) == 0
        sib = np.where(clear[:, None], cv[right[node]], cv[left[node]])
        depth = spl[on] - 1 - g
        rows = first[:-1][on] + g
        par[rows, 0] = par[rows, 1] = out.n_blocks[sel[on]]
        par[rows, 2:10] = h[on]
        par[rows, 10] = (chunk[on] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        par[rows, 11] = (chunk[on] >> np.uint64(32)).astype(np.uint32)
        par[rows, 12] = par[rows, 13] = spl[on] + 1
        par[rows, 14] = depth
        par[rows, 15:23] = sib
        par[rows, 31] = 64
        m = np.where(clear[:, None], np.concatenate([h[on], sib], axis=1), np.concatenate([sib, h[on]], axis=1))
        d = np.where(depth == 0, B.PARENT | B.ROOT, B.PARENT).astype(np.uint32)
        h[on] = B._compress_np(np.tile(_IV, (int(on.sum()), 1)), m, 0, 0, 64, d)
    out.parents, out.parent_first, out.final, out.parents_of = par, first, h, sel

    def records_of(lo, hi):
        assert parents_of is None and 0 <= lo <= hi <= n
        used = np.arange(16)[None, :] < out.n_blocks[lo:hi, None]
        return np.concatenate([out.leaf[lo:hi][used], par[first[lo]:first[hi]]])
    out.records_of = records_of
    return out
