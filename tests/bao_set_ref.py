"""Bao's slice of a SET of chunks (the union S of one file's ascending, disjoint runs) restated in plain Python on blake3_ref and
bao_range_ref's caches, from the definition and not from the C code: the recursive encoder from the data alone with the places of its
parts, the sequential top-down decoder, and the projection of a set slice onto one of its chunks (bao_range_ref.project over the set
slice's places: that chunk's one-chunk slice).  Test infrastructure.

  set slice = the 8-byte little-endian length, then the tree in pre-order restricted to S: a parent node whose span meets S gives its 64
  bytes, then its left subtree if that meets S, then its right one; a chunk of S gives its bytes."""
import bisect
import struct

import bao_range_ref as RR
from bao_ref import CHUNK, _cv_bytes, _split, num_chunks


def chunks_of(runs):
    """the chunks of the runs [(first, count), ...], ascending"""
    return [c for a, k in runs for c in range(a, a + k)]


def _meets(wanted, lo, hi):
    """does the sorted chunk list meet [lo, hi)?"""
    i = bisect.bisect_left(wanted, lo)
    return i < len(wanted) and wanted[i] < hi


def encode(data, runs, key=None):
    """the set slice of the runs from the data alone -> (slice bytes, places): places maps ("chunk", c) and ("node", lo, size) to the
    offset of that part within the slice"""
    data = bytes(data)
    key = key if key is not None else hash(data)
    n = num_chunks(len(data))
    wanted = chunks_of(runs)
    assert wanted and wanted == sorted(set(wanted)) and 0 <= wanted[0] and wanted[-1] < n
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
        out.append(_cv_bytes(RR._subtree_cv(data, key, lo, s, False)) + _cv_bytes(RR._subtree_cv(data, key, lo + s, m - s, False)))
        at[0] += 64
        if _meets(wanted, lo, lo + s):
            walk(lo, s)
        if _meets(wanted, lo + s, lo + m):
            walk(lo + s, m - s)
    walk(0, n)
    return b"".join(out), places


def union_nodes(n, wanted, c):
    """U_S(c) read aloud: the parent nodes whose span meets S n [0, c]"""
    upto = wanted[:bisect.bisect_right(wanted, c)]

    def walk(lo, m):
        if m == 1 or not _meets(upto, lo, lo + m):
            return 0
        s = _split(m)
        return 1 + walk(lo, s) + walk(lo + s, m - s)
    return walk(0, n)


def decode(sl, length, runs, root_words):
    """the sequential decoder: reads the slice front to back -> (status per wanted chunk ascending, {chunk: bytes} of those of status 0).
    3 the header is not the length, 2 a node on the chunk's path (or the root) fails, 1 the chunk's bytes fail."""
    n = num_chunks(length)
    wanted = chunks_of(runs)
    hdr = struct.unpack("<Q", sl[:8])[0] != length
    status, got = {}, {}
    at = [8]

    def walk(lo, m, want, bad, root):
        if m == 1:
            size = min(length, (lo + 1) * CHUNK) - lo * CHUNK
            body = sl[at[0]:at[0] + size]
            at[0] += size
            st = 3 if hdr else 2 if bad else 1 if RR._chunk_cv(body, lo, root) != want else 0
            status[lo] = st
            if st == 0:
                got[lo] = body
            return
        words = list(struct.unpack("<16I", sl[at[0]:at[0] + 64]))
        at[0] += 64
        bad = bad or RR._node_cv(sl[at[0] - 64:at[0]], root) != want
        s = _split(m)
        if _meets(wanted, lo, lo + s):
            walk(lo, s, words[:8], bad, False)
        if _meets(wanted, lo + s, lo + m):
            walk(lo + s, m - s, words[8:], bad, False)
    walk(0, n, list(root_words), False, True)
    assert at[0] == len(sl)
    return [status[c] for c in wanted], got


def project(sl, places, length, c):
    """the projection of a set slice onto its chunk c: that chunk's one-chunk slice"""
    return RR.project(sl, places, length, c)
