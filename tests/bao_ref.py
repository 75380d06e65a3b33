"""Bao (0.12, 1 KiB chunks) restated in plain Python from the bao specification, on top of blake3_ref: the combined tree's
outboard, the slice of one chunk and the top-down slice decoder.  Test infrastructure.

  outboard = 8-byte little-endian content length, then every parent node of BLAKE3's tree in pre-order (64 bytes each: left child
             CV, right child CV); an input of at most one chunk has the header alone
  slice    = the header, the parent nodes on the chunk's path root first, the chunk's bytes"""
import struct

import blake3_ref as B

CHUNK = 1024


def num_chunks(length):
    return max(1, (length + CHUNK - 1) // CHUNK)


def _split(m):
    """left subtree size of a node over m chunks: the largest power of two strictly below m"""
    k = 1
    while k * 2 < m:
        k *= 2
    return k


def _cv_bytes(words):
    return struct.pack("<8I", *words)


def outboard(data):
    """-> (outboard bytes, root words)"""
    data = bytes(data)
    nodes = []

    def walk(first, m, root):                  # returns the subtree's CV words; appends its parent nodes in pre-order
        if m == 1:
            return B.chunk_cv(data[first * CHUNK:(first + 1) * CHUNK], first, root)
        k = _split(m)
        slot = len(nodes)
        nodes.append(None)
        left = walk(first, k, False)
        right = walk(first + k, m - k, False)
        nodes[slot] = _cv_bytes(left) + _cv_bytes(right)
        return B.compress(B.IV, left + right, 0, 64, B.PARENT | (B.ROOT if root else 0))[:8]
    root = walk(0, num_chunks(len(data)), True)
    return struct.pack("<Q", len(data)) + b"".join(nodes), root


def path_nodes(chunk, n):
    """pre-order indices of chunk's path nodes, root first"""
    assert 0 <= chunk < n
    out, p, m = [], 0, n
    while m > 1:
        k = _split(m)
        out.append(p)
        if chunk < k:
            p, m = p + 1, k
        else:
            p, chunk, m = p + k, chunk - k, m - k
    return out


def chunk_range(length, chunk):
    return chunk * CHUNK, min(length, chunk * CHUNK + CHUNK)


def slice_chunk(ob, data, chunk):
    length = struct.unpack("<Q", ob[:8])[0]
    a, b = chunk_range(length, chunk)
    return ob[:8] + b"".join(ob[8 + 64 * i:8 + 64 * i + 64] for i in path_nodes(chunk, num_chunks(length))) + bytes(data[a:b])


class DecodeError(Exception):
    pass


def decode_slice(sl, chunk, root_words):
    """bao's decoder for the slice of one chunk: verifies top down against the root, returns the chunk's bytes"""
    length = struct.unpack("<Q", sl[:8])[0]
    n = num_chunks(length)
    if chunk >= n:
        raise DecodeError("chunk out of range")
    a, b = chunk_range(length, chunk)
    want, flags, pos, c, m = list(root_words), B.PARENT | B.ROOT, 8, chunk, n
    while m > 1:
        node = sl[pos:pos + 64]
        words = list(struct.unpack("<16I", node))
        if B.compress(B.IV, words, 0, 64, flags)[:8] != want:
            raise DecodeError("parent node mismatch")
        k = _split(m)
        if c < k:
            want, m = words[:8], k
        else:
            want, c, m = words[8:], c - k, m - k
        flags, pos = B.PARENT, pos + 64
    body = sl[pos:]
    if len(body) != b - a:
        raise DecodeError("chunk length")
    if B.chunk_cv(body, chunk, n == 1) != want:
        raise DecodeError("chunk mismatch")
    return body


def siblings_for(sl, chunk, chunk_len):
    """the sibling CVs the reference's hash_with_path reads from a slice (rust_fold/src/blake3_hash.rs:58-84): parent_cvs =
    slice[8 .. len - chunk_len]; node i (root first) gives its RIGHT half where bit par_len - i - 1 of the chunk index is clear,
    else its LEFT half.  Returned bottom up (height 0 first), the order the parent steps consume them."""
    parent = sl[8:len(sl) - chunk_len]
    par_len = len(parent) // 64
    out = []
    for i in range(par_len):
        words = list(struct.unpack("<16I", parent[64 * i:64 * i + 64]))
        bit = (chunk >> (par_len - i - 1)) & 1
        out.append(words[8:] if bit == 0 else words[:8])
    return out[::-1]
