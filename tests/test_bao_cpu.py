"""Bao outboards and slices without a GPU: the plain-Python restatement (tests/bao_ref.py) checks itself against BLAKE3 and
against the reference-made incomplete-tree transcript, and the library's host helpers (b3w_bao_outboard_size,
b3w_bao_path_nodes, b3w_bao_slice, b3w_sample_rows) must equal it."""
import ctypes
import gzip
import json
import os
import struct

import numpy as np
import pytest

import b3w_testlib as T
import bao_ref as R
import blake3_ref as B

LENGTHS = [0, 1, 1023, 1024, 1025] + [n * 1024 for n in range(2, 41)] + [17 * 1024 + 300, 33 * 1024 - 1]


def _data(length, seed=7):
    return np.random.default_rng(seed + length).integers(0, 256, length, dtype=np.uint8).tobytes()


def _flip(b, i):
    b = bytearray(b)
    b[i] ^= 0x01
    return bytes(b)


@pytest.mark.parametrize("length", LENGTHS)
def test_restatement_decodes_every_chunk_and_catches_a_flipped_byte(length):
    data = _data(length)
    ob, root = R.outboard(data)
    assert root == B.hash_words(data)
    n = R.num_chunks(length)
    assert len(ob) == 8 + 64 * (n - 1) and struct.unpack("<Q", ob[:8])[0] == length
    for c in range(n):
        sl = R.slice_chunk(ob, data, c)
        a, b = R.chunk_range(length, c)
        assert R.decode_slice(sl, c, root) == data[a:b]
        P = len(R.path_nodes(c, n))
        if b > a:                                             # a byte of the chunk
            with pytest.raises(R.DecodeError):
                R.decode_slice(_flip(sl, 8 + 64 * P + (c * 7) % (b - a)), c, root)
        for i in range(P):                                    # a byte of every node on the path, either half
            with pytest.raises(R.DecodeError):
                R.decode_slice(_flip(sl, 8 + 64 * i + (c + 13 * i) % 64), c, root)


def test_slices_give_the_sibling_cvs_of_the_reference_transcript():
    """hash_with_path's parsing of the restated slices (directions from bit par_len - i - 1, the other half) gives word for word
    the sibling CVs (record words 15..22) of every parent step the reference WASM was driven through"""
    doc = json.load(gzip.open(os.path.join(T.GOLD, "incomplete_trees.nova_vesta.json.gz"), "rt"))
    W = T.workloads()
    checked = 0
    for tree in doc["trees"]:
        n = tree["n_chunks"]
        data = W.lcg_preimage(n * 1024, seed=1).tobytes()
        ob, root = R.outboard(data)
        assert root == tree["root"]
        for leaf in tree["leaves"]:
            c = leaf["leaf"]
            sl = R.slice_chunk(ob, data, c)
            sib = R.siblings_for(sl, c, 1024)
            assert len(sib) == leaf["path_len"]
            for g, stp in enumerate(leaf["steps"][1:]):
                assert stp["record"][15:23] == sib[g], (n, c, g)
                checked += 1
    assert checked > 500


def _path_nodes(L, c, n):
    out = (ctypes.c_uint64 * 64)()
    cnt = ctypes.c_uint32()
    rc = L.b3w_bao_path_nodes(c, n, out, ctypes.byref(cnt))
    return rc, list(out[:cnt.value])


def test_host_helpers_equal_the_restatement():
    L = T.pkg().lib()
    for length in LENGTHS + [(1 << 30) + 5]:
        n = R.num_chunks(length)
        assert L.b3w_bao_outboard_size(length) == 8 + 64 * (n - 1)
    for n in list(range(1, 70)) + [255, 256, 257, 1000]:
        for c in range(n):
            rc, idx = _path_nodes(L, c, n)
            assert rc == 0 and idx == R.path_nodes(c, n), (n, c)
            assert len(idx) == L.b3w_chain_path_len(c, n)
    for length in [0, 1, 1023, 1024, 1025, 3 * 1024 + 5, 37 * 1024, 100 * 1024 + 77]:
        data = _data(length)
        ob, _ = R.outboard(data)
        for c in range(R.num_chunks(length)):
            a, b = R.chunk_range(length, c)
            want = R.slice_chunk(ob, data, c)
            ln = ctypes.c_uint64()
            assert L.b3w_bao_slice(ob, length, c, data[a:b], None, ctypes.byref(ln)) == 0 and ln.value == len(want)
            out = ctypes.create_string_buffer(len(want))
            assert L.b3w_bao_slice(ob, length, c, data[a:b], out, ctypes.byref(ln)) == 0
            assert out.raw == want, (length, c)


def test_sample_rows_is_sample_major_with_duplicates():
    L = T.pkg().lib()
    for length in [1, 1024, 5 * 1024 + 1, 37 * 1024, 100 * 1024 + 77]:
        n = R.num_chunks(length)
        chunks = np.array([n - 1, 0, n // 2, n - 1, 0], dtype=np.uint64)
        rf = np.zeros(len(chunks) + 1, dtype=np.uint64)
        total = L.b3w_sample_rows(length, chunks.ctypes.data, len(chunks), rf.ctypes.data)
        row, want = 0, []
        for c in chunks:
            a, b = R.chunk_range(length, int(c))
            want.append(row)
            row += max(1, (b - a + 63) // 64) + len(R.path_nodes(int(c), n))
        assert total == row and list(rf) == want + [row], length


def test_argument_errors():
    L = T.pkg().lib()
    bad = -T.pkg().B3W_E_BAD_ARGUMENT
    chunks = np.array([0, 5], dtype=np.uint64)
    rf = np.zeros(3, dtype=np.uint64)
    assert L.b3w_sample_rows(5 * 1024, chunks.ctypes.data, 2, rf.ctypes.data) == bad         # chunk 5 of 5
    assert L.b3w_sample_rows(5 * 1024 + 1, chunks.ctypes.data, 2, rf.ctypes.data) > 0
    assert _path_nodes(L, 3, 3)[0] == 100 and _path_nodes(L, 0, 0)[0] == 100
    data = _data(3000)
    ob, _ = R.outboard(data)
    ln = ctypes.c_uint64()
    assert L.b3w_bao_slice(ob, 3000, 3, b"", None, ctypes.byref(ln)) == 100                   # no chunk 3
    assert L.b3w_bao_slice(ob, 3001, 0, data[:1024], None, ctypes.byref(ln)) == 100           # the header says 3000
    assert L.b3w_bao_slice(ob, 3000, 0, None, ctypes.create_string_buffer(8 + 128 + 1024), ctypes.byref(ln)) == 100
