"""Bao slices without a GPU: the library's host calls for slices (b3w_bao_slice_size, b3w_bao_slice_batch_layout,
b3w_bao_slice_decode) against the plain-Python restatement (tests/bao_ref.py): sizes and the packed layout for every chunk, the
host decoder on every slice the restatement makes and on every tampered one, and the slices of the reference-made incomplete-tree
transcript against the transcript's roots."""
import ctypes
import gzip
import json
import os
import struct

import numpy as np
import pytest

import b3w_testlib as T
import bao_ref as R
from test_bao_cpu import LENGTHS, _data, _flip

BAD = 100
_CACHE = {}


def _made(length):
    """-> (data, outboard, root words) of the test file of this length"""
    if length not in _CACHE:
        data = _data(length)
        _CACHE[length] = (data,) + R.outboard(data)
    return _CACHE[length]


def _path_lens(n):
    """path length of every chunk of a tree over n chunks (the walk of bao_ref.path_nodes, all chunks at once)"""
    c = np.arange(n, dtype=np.int64)
    m = np.full(n, n, dtype=np.int64)
    P = np.zeros(n, dtype=np.int64)
    while (m > 1).any():
        live = m > 1
        k = np.where(live, 1 << (np.ceil(np.log2(np.maximum(m, 2))).astype(np.int64) - 1), 1)      # largest power of two strictly below m
        assert ((k < m) | ~live).all() and ((2 * k >= m) | ~live).all()
        left = c < k
        P += live
        c = np.where(live & ~left, c - k, c)
        m = np.where(live, np.where(left, k, m - k), m)
    return P


def _decode(L, sl, length, chunk, root, slice_len=None):
    rw = np.array(root, dtype=np.uint32)
    out = ctypes.create_string_buffer(1024)
    cnt, st = ctypes.c_uint32(12345), ctypes.c_int32(-1)
    rc = L.b3w_bao_slice_decode(sl, len(sl) if slice_len is None else slice_len, length, chunk, rw.ctypes.data, out, ctypes.byref(cnt), ctypes.byref(st))
    return rc, st.value, out.raw[:cnt.value] if rc == 0 else b""


def _ref_accepts(sl, chunk, root, length):
    """the restatement's decoder as a caller who knows the file's length uses it.  bao's decoder takes the length FROM the header
    and authenticates it only through the tree's shape, so on its own it accepts e.g. chunk 0 of a 3 072-byte file under a header
    of 3 073 (the same path); the library's decoder is given the length and reports such a header as status 3, so the
    restatement's verdict is held together with the header comparison."""
    if len(sl) < 8 or struct.unpack("<Q", sl[:8])[0] != length:
        return False
    try:
        R.decode_slice(sl, chunk, root)
        return True
    except (R.DecodeError, struct.error):
        return False


def test_abi_is_1_4():
    assert T.pkg().lib().b3w_abi_version() == (1 << 16) | 4


def test_sizes_and_layout_equal_the_restatement():
    m = T.pkg()
    L = m.lib()
    lens, files, chunks, want = [], [], [], []
    for f, length in enumerate(LENGTHS):
        data, ob, _ = _made(length)
        n = R.num_chunks(length)
        assert list(_path_lens(n)) == [len(R.path_nodes(c, n)) for c in range(n)]
        lens.append(length)
        for c in range(n):
            size = len(R.slice_chunk(ob, data, c))
            assert L.b3w_bao_slice_size(length, c) == size == m.bao.slice_size(length, c), (length, c)
            files.append(f)
            chunks.append(c)
            want.append(size)
        assert L.b3w_bao_slice_size(length, n) == 0 and L.b3w_bao_slice_size(length, n + 7) == 0
    big = (1 << 30) + 5                                                    # sizes only
    n = R.num_chunks(big)
    P = _path_lens(n)
    assert int(P[0]) == 21 and int(P[n - 1]) == 1
    lens.append(big)
    for c in range(n):
        size = 8 + 64 * int(P[c]) + (1024 if c < n - 1 else 5)
        assert L.b3w_bao_slice_size(big, c) == size, c
    files += [len(LENGTHS)] * n
    chunks += list(range(n))
    want += [8 + 64 * int(p) + 1024 for p in P[:-1]] + [8 + 64 + 5]
    # the packed layout: in sample order, every start a multiple of 8, no entry reaches into the next
    order = np.random.default_rng(5).permutation(len(files))
    fi, ch, want = np.array(files, dtype=np.uint32)[order], np.array(chunks, dtype=np.uint64)[order], np.array(want, dtype=np.uint64)[order]
    ln = np.array(lens, dtype=np.uint64)
    sf = np.zeros(fi.size + 1, dtype=np.uint64)
    total = L.b3w_bao_slice_batch_layout(ln.ctypes.data, ln.size, fi.ctypes.data, ch.ctypes.data, fi.size, sf.ctypes.data)
    assert total == int(sf[-1]) and (sf % 8 == 0).all()
    assert (sf[:-1] + want <= sf[1:]).all()
    assert (sf[1:] - (sf[:-1] + want) < 16).all()                          # (and no more padding than an alignment needs)
    assert list(m.bao.slice_layout(ln, fi, ch)) == list(sf)
    none = np.zeros(1, dtype=np.uint64)
    assert L.b3w_bao_slice_batch_layout(ln.ctypes.data, ln.size, None, None, 0, none.ctypes.data) == int(none[0])
    # bad indices
    f1, c1 = np.array([ln.size], dtype=np.uint32), np.array([0], dtype=np.uint64)
    assert L.b3w_bao_slice_batch_layout(ln.ctypes.data, ln.size, f1.ctypes.data, c1.ctypes.data, 1, sf.ctypes.data) == -BAD
    f1, c1 = np.array([LENGTHS.index(1024)], dtype=np.uint32), np.array([1], dtype=np.uint64)
    assert L.b3w_bao_slice_batch_layout(ln.ctypes.data, ln.size, f1.ctypes.data, c1.ctypes.data, 1, sf.ctypes.data) == -BAD
    with pytest.raises(m.B3WError):
        m.bao.slice_layout(ln, [0], [1])
    with pytest.raises(m.B3WError):
        m.bao.slice_size(1024, 1)


@pytest.mark.parametrize("length", LENGTHS)
def test_host_decoder_on_every_slice_and_every_tampering(length):
    m = T.pkg()
    L = m.lib()
    data, ob, root = _made(length)
    n = R.num_chunks(length)
    wrong_root = list(root)
    wrong_root[3] ^= 0x10000

    def both(sl, c, rt, want_status):
        rc, st, body = _decode(L, sl, length, c, rt)
        assert rc == 0 and st == want_status, (length, c, st, want_status)
        assert _ref_accepts(sl, c, rt, length) == (want_status == 0), (length, c, want_status)
        return body
    for c in range(n):
        sl = R.slice_chunk(ob, data, c)
        a, b = R.chunk_range(length, c)
        P = len(R.path_nodes(c, n))
        assert both(sl, c, root, 0) == data[a:b]
        assert m.bao.decode_slice(sl, length, c, root) == (0, data[a:b])
        if b > a:                                             # a byte of the chunk
            assert both(_flip(sl, 8 + 64 * P + (c * 7) % (b - a)), c, root, 1) == b""
        for i in range(P):                                    # a byte of every node on the path, in either half
            both(_flip(sl, 8 + 64 * i + (c + 13 * i) % 32), c, root, 2)
            both(_flip(sl, 8 + 64 * i + 32 + (c + 5 * i) % 32), c, root, 2)
        both(_flip(sl, c % 8), c, root, 3)                     # a header that is not the length
        both(sl, c, wrong_root, 2 if P else 1)                # one chunk: its ROOT-flagged output is what meets the root
        if P and b > a:                                       # precedence: header, then a node, then the bytes
            worst = _flip(_flip(_flip(sl, 0), 8 + 64 * (P - 1) + 40), 8 + 64 * P)
            both(worst, c, root, 3)
            both(_flip(_flip(sl, 8 + 64 * (P - 1) + 40), 8 + 64 * P), c, root, 2)
        # a slice one byte short or long is refused
        assert _decode(L, sl, length, c, root, slice_len=len(sl) - 1)[0] == BAD
        assert _decode(L, sl + b"\0", length, c, root)[0] == BAD
        assert not _ref_accepts(sl[:-1], c, root, length) and not _ref_accepts(sl + b"\0", c, root, length)
    assert _decode(L, R.slice_chunk(ob, data, 0), length, n, root)[0] == BAD          # no such chunk


def test_the_reference_transcripts_slices_decode():
    """the slices test_slices_give_the_sibling_cvs_of_the_reference_transcript builds, through the host decoder against the roots the
    reference-made transcript records"""
    L = T.pkg().lib()
    doc = json.load(gzip.open(os.path.join(T.GOLD, "incomplete_trees.nova_vesta.json.gz"), "rt"))
    W = T.workloads()
    checked = 0
    for tree in doc["trees"]:
        n = tree["n_chunks"]
        data = W.lcg_preimage(n * 1024, seed=1).tobytes()
        ob, _ = R.outboard(data)
        for leaf in tree["leaves"]:
            c = leaf["leaf"]
            sl = R.slice_chunk(ob, data, c)
            rc, st, body = _decode(L, sl, n * 1024, c, tree["root"])
            assert rc == 0 and st == 0 and body == data[c * 1024:c * 1024 + 1024], (n, c, rc, st)
            checked += 1
    assert checked > 100
