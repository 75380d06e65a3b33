"""Bao's slice of a RANGE of chunks restated in plain Python on blake3_ref, from the definition and not from the C code: the recursive
encoder from the data alone, the sequential top-down decoder, and the projection of a range slice onto one of its chunks (which is
that chunk's one-chunk slice, bao_ref.slice_chunk).  Test infrastructure.

  slice of chunks [a, a + k) = the 8-byte little-endian length, then the tree in pre-order restricted to the range: a parent node whose
  span meets the range gives its 64 bytes, then its left subtree if that meets the range, then its right one; a chunk of the range
  gives its bytes."""
import struct

import blake3_ref as B
from bao_ref import CHUNK, _cv_bytes, _split, num_chunks

_SUBTREE = {}
_HASHED = {}                                             # the decoder's hashes by what was hashed: tampered slices differ in one part


def _chunk_cv(body, counter, root):
    k = (body, counter, root)
    if k not in _HASHED:
        _HASHED[k] = B.chunk_cv(body, counter, root)
    return _HASHED[k]


def _node_cv(node, root):
    k = (node, root)
    if k not in _HASHED:
        _HASHED[k] = B.compress(B.IV, list(struct.unpack("<16I", node)), 0, 64, B.PARENT | (B.ROOT if root else 0))[:8]
    return _HASHED[k]


def _subtree_cv(data, key, first, m, root):
    """CV words of the subtree over chunks [first, first + m) (cached per file: `key` names the data)"""
    k = (key, first, m, root)
    if k not in _SUBTREE:
        if m == 1:
            _SUBTREE[k] = B.chunk_cv(data[first * CHUNK:(first + 1) * CHUNK], first, root)
        else:
            s = _split(m)
            left, right = _subtree_cv(data, key, first, s, False), _subtree_cv(data, key, first + s, m - s, False)
            _SUBTREE[k] = B.compress(B.IV, left + right, 0, 64, B.PARENT | (B.ROOT if root else 0))[:8]
    return _SUBTREE[k]


def seed(data, key):
    """the CVs of the file's whole chunks in one vectorised pass (blake3_ref.chunk_cvs_np) into the cache: the files of a thousand chunks"""
    import numpy as np
    whole = len(data) // CHUNK
    if whole >= 2 and (key, 0, 1, False) not in _SUBTREE:
        cvs = B.chunk_cvs_np(np.frombuffer(bytes(data[:whole * CHUNK]), dtype=np.uint8))
        for c in range(whole):
            _SUBTREE[(key, c, 1, False)] = [int(x) for x in cvs[c]]


def encode(data, a, k, key=None):
    """the slice of chunks [a, a + k) from the data alone -> (slice bytes, places): places maps ("chunk", c) and ("node", lo, size) to
    the offset of that part within the slice"""
    data = bytes(data)
    key = key if key is not None else hash(data)
    n = num_chunks(len(data))
    assert k >= 1 and 0 <= a and a + k <= n
    out, places = [struct.pack("<Q", len(data))], {}
    at = [8]

    def walk(lo, m):
        if m == 1:
            places[("chunk", lo)] = at[0]
            body = data[lo * CHUNK:(lo + 1) * CHUNK]
            out.append(body)
            at[0] += len(body)
            return
        s = _split(m)
        places[("node", lo, m)] = at[0]
        out.append(_cv_bytes(_subtree_cv(data, key, lo, s, False)) + _cv_bytes(_subtree_cv(data, key, lo + s, m - s, False)))
        at[0] += 64
        if a < lo + s:
            walk(lo, s)
        if a + k > lo + s:
            walk(lo + s, m - s)
    walk(0, n)
    return b"".join(out), places


def union_nodes(n, a, c):
    """U(a, c) read aloud: the parent nodes whose span meets [a, c]"""
    def walk(lo, m):
        if m == 1 or lo > c or lo + m <= a:
            return 0
        s = _split(m)
        return 1 + walk(lo, s) + walk(lo + s, m - s)
    return walk(0, n)


def path_spans(c, n):
    """(lo, size) of the nodes on chunk c's path, root first"""
    out, lo, m = [], 0, n
    while m > 1:
        out.append((lo, m))
        s = _split(m)
        if c < lo + s:
            m = s
        else:
            lo, m = lo + s, m - s
    return out


def decode(sl, length, a, k, root_words):
    """the sequential decoder: reads the slice front to back -> (status per chunk of the range, {chunk: bytes} of those of status 0).
    3 the header is not the length, 2 a node on the chunk's path (or the root) fails, 1 the chunk's bytes fail."""
    n = num_chunks(length)
    hdr = struct.unpack("<Q", sl[:8])[0] != length
    status, got = {}, {}
    at = [8]

    def walk(lo, m, want, bad, root):
        if m == 1:
            size = min(length, (lo + 1) * CHUNK) - lo * CHUNK
            body = sl[at[0]:at[0] + size]
            at[0] += size
            st = 3 if hdr else 2 if bad else 1 if _chunk_cv(body, lo, root) != want else 0
            status[lo] = st
            if st == 0:
                got[lo] = body
            return
        words = list(struct.unpack("<16I", sl[at[0]:at[0] + 64]))
        at[0] += 64
        bad = bad or _node_cv(sl[at[0] - 64:at[0]], root) != want
        s = _split(m)
        if a < lo + s:
            walk(lo, s, words[:8], bad, False)
        if a + k > lo + s:
            walk(lo + s, m - s, words[8:], bad, False)
    walk(0, n, list(root_words), False, True)
    assert at[0] == len(sl)
    return [status[c] for c in range(a, a + k)], got


def project(sl, places, length, c):
    """the projection of a range slice onto its chunk c: the header, the nodes of c's path found in the slice root first, c's bytes"""
    n = num_chunks(length)
    size = min(length, (c + 1) * CHUNK) - c * CHUNK
    at = places[("chunk", c)]
    return sl[:8] + b"".join(sl[places[("node", lo, m)]:places[("node", lo, m)] + 64] for lo, m in path_spans(c, n)) + sl[at:at + size]
