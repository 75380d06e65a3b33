"""Bao outboards over chunk groups, restated in plain Python on bao_ref / blake3_ref.  Test infrastructure.

  G = 2^g chunks to a group; n_groups = ceil(n_chunks / G)
  group outboard = 8-byte little-endian content length, then the parent nodes of BLAKE3's tree shape over the GROUPS in pre-order
                   (64 bytes each: left child CV, right child CV); a leaf of that tree is the CV of BLAKE3's tree over the group's own
                   chunks (chunk counters first + i; ROOT only where the group is the whole file)
  a chunk's path = its group's path in the tree over groups (stored), then the path of chunk c - first inside the tree over the
                   group's min(G, n_chunks - first) chunks (recomputed from the group's bytes), first = c // G * G

The layout is pinned to this construction, not to another implementation's files."""
import functools
import struct

import bao_ref as R
import blake3_ref as B

CHUNK = R.CHUNK


def num_groups(n_chunks, g):
    return (n_chunks + (1 << g) - 1) >> g


def _parent(left, right, root):
    return B.compress(B.IV, left + right, 0, 64, B.PARENT | (B.ROOT if root else 0))[:8]


def _chunks_tree(cvs, first, m, root, nodes=None, want=None):
    """CV of BLAKE3's tree over the chunk CVs cvs[first : first + m] (a list of 8-word lists; a one-chunk tree is its chunk's CV as
    given).  nodes / want: appends the 64-byte nodes on the path of chunk index `want`, root first."""
    if m == 1:
        return cvs[first]
    k = R._split(m)
    left = _chunks_tree(cvs, first, k, False, nodes if want is not None and want < first + k else None, want)
    right = _chunks_tree(cvs, first + k, m - k, False, nodes if want is not None and want >= first + k else None, want)
    if nodes is not None:
        nodes.insert(0, R._cv_bytes(left) + R._cv_bytes(right))       # (the recursion returns bottom up: every node goes in front of the deeper ones)
    return _parent(left, right, root)


@functools.lru_cache(maxsize=None)
def _chunk_cv(chunk_bytes, counter, root):
    return B.chunk_cv(chunk_bytes, counter, root)


def _group_cvs(data, length, first, gn, sole_chunk):
    """the chunk CVs of the group's gn chunks from `data` = the group's bytes (chunk i of the group at 1024 i; bytes past the file's
    end ignored)"""
    out = []
    for i in range(gn):
        a, b = R.chunk_range(length, first + i)
        out.append(list(_chunk_cv(bytes(data[i * CHUNK:i * CHUNK + (b - a)]), first + i, bool(sole_chunk))))
    return out


def group_outboard(data, g):
    """-> (group outboard bytes, root words), from a walk over the groups"""
    data = bytes(data)
    n, G = R.num_chunks(len(data)), 1 << g
    ng = num_groups(n, g)
    nodes = []

    def leaf(group, root):
        first = group * G
        gn = min(G, n - first)
        cvs = _group_cvs(data[first * CHUNK:(first + gn) * CHUNK], len(data), first, gn, root and gn == 1)
        return _chunks_tree(cvs, 0, gn, root)

    def walk(first, m, root):
        if m == 1:
            return leaf(first, root)
        k = R._split(m)
        slot = len(nodes)
        nodes.append(None)
        left = walk(first, k, False)
        right = walk(first + k, m - k, False)
        nodes[slot] = R._cv_bytes(left) + R._cv_bytes(right)
        return _parent(left, right, root)
    root = walk(0, ng, True)
    return struct.pack("<Q", len(data)) + b"".join(nodes), root


def group_outboard_size(length, g):
    return 8 + 64 * (num_groups(R.num_chunks(length), g) - 1)


def group_path_nodes(chunk, n_chunks, g):
    """indices in the group outboard of the stored part of the chunk's path, root first"""
    assert 0 <= chunk < n_chunks
    return R.path_nodes(chunk >> g, num_groups(n_chunks, g))


def node_spans(n):
    """(first chunk, chunk count) of every parent node of the full outboard of n chunks, in pre-order"""
    out = []

    def walk(first, m):
        if m == 1:
            return
        k = R._split(m)
        out.append((first, m))
        walk(first, k)
        walk(first + k, m - k)
    walk(0, n)
    return out


def filter_full_outboard(ob, g):
    """the full outboard with every node over at most 2^g chunks left out"""
    length = struct.unpack("<Q", ob[:8])[0]
    spans = node_spans(R.num_chunks(length))
    return ob[:8] + b"".join(ob[8 + 64 * i:8 + 64 * i + 64] for i, (_, m) in enumerate(spans) if m > (1 << g))


def slice_from_group(ob_g, group_bytes, chunk, g):
    """the chunk's ordinary bao slice (header, path nodes root first, the chunk's bytes) rebuilt from the group outboard and the
    bytes of the chunk's group alone"""
    length = struct.unpack("<Q", ob_g[:8])[0]
    n, G = R.num_chunks(length), 1 << g
    first = chunk // G * G
    gn = min(G, n - first)
    upper = [ob_g[8 + 64 * i:8 + 64 * i + 64] for i in group_path_nodes(chunk, n, g)]
    cvs = _group_cvs(group_bytes, length, first, gn, n == 1)
    lower = []
    _chunks_tree(cvs, 0, gn, n <= G, lower, chunk - first)
    a, b = R.chunk_range(length, chunk)
    at = (chunk - first) * CHUNK
    return ob_g[:8] + b"".join(upper) + b"".join(lower) + bytes(group_bytes[at:at + (b - a)])


def group_bytes(data, chunk, g):
    """what a provider reads for a challenge of `chunk`: its group's bytes, zero-padded to 1024 << g"""
    first = (chunk >> g << g) * CHUNK
    part = bytes(data[first:first + (CHUNK << g)])
    return part + bytes((CHUNK << g) - len(part))


def group_outboard_np(data, g):
    """group_outboard for a large file (numpy uint8 array of at least one whole group and 2 KiB): the chunk CVs and the complete
    groups' trees vectorised with numpy (blake3_ref.chunk_cvs_np), the tree over the groups walked as above"""
    import numpy as np
    length, G = data.size, 1 << g
    n = R.num_chunks(length)
    whole = length // CHUNK
    assert whole >= 2 and n > G
    cvs = B.chunk_cvs_np(data[:whole * CHUNK])
    if whole < n:
        cvs = np.concatenate([cvs, np.array([B.chunk_cv(data[whole * CHUNK:].tobytes(), whole, False)], dtype=np.uint32)])
    full = n // G
    lvl = cvs[:full * G]
    for _ in range(g):                                                    # a complete group: pairs level by level
        lvl = B._compress_np(np.tile(np.array(B.IV, dtype=np.uint32), (lvl.shape[0] // 2, 1)), lvl.reshape(-1, 16), 0, 0, 64, B.PARENT)
    leaves = [[int(x) for x in row] for row in lvl]
    if full * G < n:                                                      # the short last group
        leaves.append(_chunks_tree([[int(x) for x in row] for row in cvs[full * G:]], 0, n - full * G, False))
    nodes = []

    def walk(first, m, root):
        if m == 1:
            return leaves[first]
        k = R._split(m)
        slot = len(nodes)
        nodes.append(None)
        left = walk(first, k, False)
        right = walk(first + k, m - k, False)
        nodes[slot] = R._cv_bytes(left) + R._cv_bytes(right)
        return _parent(left, right, root)
    root = walk(0, len(leaves), True)
    return struct.pack("<Q", length) + b"".join(nodes), root
