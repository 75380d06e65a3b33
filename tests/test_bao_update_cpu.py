"""Outboards updated in place after writes, without a GPU: the plain-Python restatement (tests/bao_update_ref.py) and the library's
host call (b3w_bao_outboard_update, bao.update_host) against the full recompute (bao_groups_ref.group_outboard) of the file as it is
after the writes, every byte; sparseness shown by poison (the nodes with no dirty unit below them are never written); a changed chunk
that the list misses is what b3w_bao_verify finds, at exactly its unit; b3w_bao_update_scratch_bytes against counts made here; the
names, the ABI number and the refusals that need no device; bao.chunk_ranges."""
import ctypes
import os
import re

import numpy as np
import pytest

import b3w_testlib as T
import bao_groups_ref as GR
import bao_ref as R
import bao_update_ref as U
import test_bao_cpu as C

GS = (0, 1, 4, 6)
NAMES = {"b3w_bao_outboard_update_batch_device": 17, "b3w_bao_update_scratch_bytes": 5, "b3w_bao_outboard_update": 8}
_MADE = {}


def _made(length, g):
    """-> (data A, its group outboard of g, its root words)"""
    if (length, g) not in _MADE:
        data = C._data(length)
        _MADE[(length, g)] = (data,) + GR.group_outboard(data, g)
    return _MADE[(length, g)]


def _written(data, chunks):
    """the file after a write into each of these chunks (a flipped byte at a place that depends on the chunk alone)"""
    out = bytearray(data)
    for c in chunks:
        a, b = R.chunk_range(len(data), c)
        if b > a:
            out[a + (c * 7) % (b - a)] ^= 0x01
    return bytes(out)


def _dirty_sets(n):
    """name -> the chunks written: first, last, middle, a run across the top power-of-two split, every other chunk, all, none"""
    k = R._split(n) if n > 1 else 0
    sets = {"first": [0], "last": [n - 1], "middle": [n // 2], "across the split": list(range(max(0, k - 2), min(n, k + 2))),
            "every other": list(range(0, n, 2)), "all": list(range(n)), "none": []}
    return sets


def _ranges(chunks):
    """runs of consecutive chunks as (first, count) pairs"""
    out = []
    for c in chunks:
        if out and out[-1][0] + out[-1][1] == c:
            out[-1][1] += 1
        else:
            out.append([c, 1])
    return [tuple(x) for x in out]


def _host(L, data, ob, root, ranges, g):
    """b3w_bao_outboard_update in place on copies -> (outboard bytes, root words)"""
    buf = np.frombuffer(bytes(ob), dtype=np.uint8).copy()
    rw = np.array(root, dtype=np.uint32)
    fc = np.array([a for a, _ in ranges], dtype=np.uint64)
    nc = np.array([c for _, c in ranges], dtype=np.uint64)
    assert L.b3w_bao_outboard_update(data, len(data), buf.ctypes.data, g, fc.ctypes.data, nc.ctypes.data, len(ranges), rw.ctypes.data) == 0
    return buf.tobytes(), [int(x) for x in rw]


def test_the_names_are_declared_exported_and_bound():
    m = T.pkg()
    L = m.lib()
    hdr = open(os.path.join(T.ROOT, "include", "b3wit.h")).read()
    declared = set(re.findall(r"\b(b3w_[a-z0-9_]+)\s*\(", hdr))
    for name, n_args in NAMES.items():
        assert name in declared and name in m.EXPORTED_SYMBOLS, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_args, name
    assert L.b3w_bao_outboard_update_batch_device.restype is ctypes.c_int32 and L.b3w_bao_update_scratch_bytes.restype is ctypes.c_uint64
    assert L.b3w_abi_version() == (1 << 16) + 4                                # new names only: the number stays
    for name in ("outboard_update_batch", "update_host", "chunk_ranges"):
        assert callable(getattr(m.bao, name)), name


@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("length", C.LENGTHS)
def test_updates_equal_the_full_recompute_and_write_nothing_else(length, g):
    m = T.pkg()
    L = m.lib()
    data, ob, root = _made(length, g)
    n = R.num_chunks(length)
    nu = GR.num_groups(n, g)
    for name, chunks in _dirty_sets(n).items():
        now = _written(data, chunks)
        ranges = _ranges(chunks)
        want_ob, want_root = GR.group_outboard(now, g) if chunks else (ob, root)
        assert (want_root != root) == (now != data), (length, g, name)         # (a file of no bytes has nothing to flip)
        units = U.dirty_units(ranges, n, g)
        assert units == sorted({c >> g for c in chunks})
        # every byte, by the restatement and by the library
        assert U.update(now, ob, root, ranges, g) == (want_ob, want_root), (length, g, name)
        assert _host(L, now, ob, root, ranges, g) == (want_ob, want_root), (length, g, name)
        got_ob, got_root = m.bao.update_host(now, ob, root, [a for a, _ in ranges], [c for _, c in ranges], g)
        assert (got_ob, list(got_root)) == (want_ob, want_root), (length, g, name)
        # sparseness by poison: the nodes with no dirty unit below them stay as they were, the others are the recompute's
        bad_ob, keep = U.poison(ob, nu, units)
        for got, _ in (U.update(now, bad_ob, root, ranges, g), _host(L, now, bad_ob, root, ranges, g)):
            assert got[:8] == ob[:8]
            for i in range(nu - 1):
                node = got[8 + 64 * i:8 + 64 * i + 64]
                assert node == (want_ob[8 + 64 * i:8 + 64 * i + 64] if i in keep else b"\xEE" * 64), (length, g, name, i)
        # ... and with every changed byte listed many times over, out of order: the same
        if chunks:
            messy = [(c, 1) for c in reversed(chunks)] + ranges + [(chunks[0], min(3, n - chunks[0])), (chunks[-1], 0)]
            assert _host(L, now, ob, root, messy, g) == (want_ob, want_root) == U.update(now, ob, root, messy, g), (length, g, name)


@pytest.mark.parametrize("g", GS)
def test_a_missed_chunk_is_what_verification_finds_at_exactly_its_unit(g):
    L = T.pkg().lib()
    seen = 0
    for length in C.LENGTHS + [70 * 1024, 130 * 1024 + 5]:                 # (the last two: files of more than one group of 64)
        data, ob, root = _made(length, g)
        n = R.num_chunks(length)
        nu = GR.num_groups(n, g)
        if nu < 2:
            continue                                                       # (one unit: a listed chunk rehashes all there is)
        listed, missed = 0, n - 1
        now = _written(data, [listed, missed])
        for got_ob, got_root in (U.update(now, ob, root, [(listed, 1)], g), _host(L, now, ob, root, [(listed, 1)], g)):
            st = np.full(nu, 0xEE, dtype=np.uint8)
            rw = np.array(got_root, dtype=np.uint32)
            fs, fb = ctypes.c_int32(-1), ctypes.c_uint64(0)
            assert L.b3w_bao_verify(now, length, got_ob, g, rw.ctypes.data, st.ctypes.data, ctypes.byref(fs), ctypes.byref(fb)) == 0
            want = [0] * nu
            want[missed >> g] = 1
            assert list(st) == want and (fs.value, fb.value) == (1, missed >> g), (length, g)
        seen += 1
    assert seen >= 2


def _scratch(L, lens, files, firsts, counts):
    ln, fi = np.array(lens, dtype=np.uint64), np.array(files, dtype=np.uint32)
    fc, nc = np.array(firsts, dtype=np.uint64), np.array(counts, dtype=np.uint64)
    return L.b3w_bao_update_scratch_bytes(ln.ctypes.data, fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, fi.size)


def test_scratch_sizes_equal_counts_made_here():
    L = T.pkg().lib()
    K = 1024
    #       0     1        2          3             4                5                  6 (1 026 tiles)
    lens = [0, 5 * K, 64 * K, 65 * K + 3, (1 << 20) + 1, 2051 * K - 300, (1 << 30) + (1 << 20) + 5]
    cases = [
        ([0, 1, 2, 3], [0, 2, 0, 7], [1, 3, 64, 50]),                          # files of one tile: none
        ([4], [0], [1]), ([4], [1024], [1]), ([4], [1023], [2]), ([4, 4, 4], [5, 5, 1000], [1, 1, 30]),
        ([5, 5, 5], [2050, 0, 1020], [1, 1, 11]),                              # three tiles, out of order
        ([5, 5, 5, 5], [100, 90, 100, 1500], [2000, 20, 2000, 1]),             # overlapping and duplicated
        ([6], [0], [1]), ([6, 6, 6, 6], [0, 1023 * K, 1024 * K, 1025 * K], [1, 1, 1, 1]),
        ([6, 5, 6, 1, 4], [1024 * K - 1, 2047, 1024 * K - 1, 0, 1000], [2, 2, 2, 5, 25]),
        ([6], [0], [1025 * K + 1025]),                                          # all of it: 1 026 tiles and 2 spans
        ([5, 6], [3, 3], [0, 0]),                                               # empty ranges
    ]
    want = [0, 1, 1, 2, 2, 3, 3, 1 + 1, 4 + 2, (2 + 2) + 2 + 0 + 2, 1026 + 2, 0]
    for (files, firsts, counts), w in zip(cases, want):
        assert U.scratch_items(lens, files, firsts, counts) == w, (files, firsts, counts)
        assert _scratch(L, lens, files, firsts, counts) == 32 * w, (files, firsts, counts)
    assert L.b3w_bao_update_scratch_bytes(None, None, None, None, 0) == 0
    one = (ctypes.c_uint64 * 1)(5 << 20)
    assert L.b3w_bao_update_scratch_bytes(one, None, one, one, 1) == 0 and L.b3w_bao_update_scratch_bytes(None, one, one, one, 1) == 0


def test_refusals_that_need_no_device():
    m = T.pkg()
    L = m.lib()
    bad = m.B3W_E_BAD_ARGUMENT
    one = (ctypes.c_uint64 * 1)(0)
    assert L.b3w_bao_outboard_update_batch_device(None, None, 0, None, None, 0, 0, None, None, None, None, None, None, 0, None, 0, None) == bad
    assert L.b3w_bao_outboard_update_batch_device(None, one, 8, one, one, 1, 0, one, one, one, one, one, one, 1, None, 0, None) == bad
    assert one[0] == 0
    data, ob, root = _made(5 * 1024, 1)
    buf = np.frombuffer(ob, dtype=np.uint8).copy()
    rw = np.array(root, dtype=np.uint32)
    fc, nc = np.array([1, 4], dtype=np.uint64), np.array([2, 1], dtype=np.uint64)

    def call(d=data, o=buf.ctypes.data, g=1, a=fc.ctypes.data, c=nc.ctypes.data, k=2, r=rw.ctypes.data):
        return L.b3w_bao_outboard_update(d, len(data), o, g, a, c, k, r)
    assert call(d=None) == bad and call(o=None) == bad and call(r=None) == bad and call(a=None) == bad and call(c=None) == bad and call(g=7) == bad
    for first, count in ((5, 1), (4, 2), (0, 6), (6, 0), (1 << 63, 1 << 63)):  # past the file's 5 chunks
        fc[1], nc[1] = first, count
        assert call() == bad, (first, count)
    assert buf.tobytes() == ob and list(rw) == list(root)                      # a refused call writes nothing
    fc[1], nc[1] = 5, 0                                                        # an empty range at the end is dropped
    assert call() == 0 and call(a=None, c=None, k=0) == 0
    assert buf.tobytes() == ob and list(rw) == list(root)                      # (the file is as it was: the same bytes again)
    # a file of no bytes has one chunk
    e_ob, e_root = GR.group_outboard(b"", 0)
    e_buf, e_rw = np.frombuffer(e_ob, dtype=np.uint8).copy(), np.zeros(8, dtype=np.uint32)
    z, o1 = np.array([0], dtype=np.uint64), np.array([1], dtype=np.uint64)
    assert L.b3w_bao_outboard_update(None, 0, e_buf.ctypes.data, 0, z.ctypes.data, o1.ctypes.data, 1, e_rw.ctypes.data) == 0 and list(e_rw) == e_root
    assert L.b3w_bao_outboard_update(None, 0, e_buf.ctypes.data, 0, o1.ctypes.data, o1.ctypes.data, 1, e_rw.ctypes.data) == bad
    # the Python calls, before they touch a device
    for g in (-1, 7):
        with pytest.raises(m.B3WError, match="group_log"):
            m.bao.update_host(data, ob, root, [0], [1], g)
        with pytest.raises(m.B3WError, match="group_log"):
            m.bao.outboard_update_batch(None, None, [0], [10], None, None, [0], [0], [1], group_log=g)
    with pytest.raises(m.B3WError, match="size"):
        m.bao.update_host(data, ob + bytes(64), root, [0], [1], 1)
    with pytest.raises(m.B3WError, match="2 first chunks and 1 chunk counts"):
        m.bao.update_host(data, ob, root, [0, 1], [1], 1)
    with pytest.raises(m.B3WError):
        m.bao.update_host(data, ob, root, [5], [1], 1)


def test_chunk_ranges():
    m = T.pkg()

    def cr(off, cnt):
        a, b = m.bao.chunk_ranges(off, cnt)
        assert a.dtype == np.uint64 and b.dtype == np.uint64
        return list(zip(a.tolist(), b.tolist()))
    assert cr([0], [1]) == [(0, 1)] and cr([1023], [1]) == [(0, 1)] and cr([1023], [2]) == [(0, 2)] and cr([1024], [1024]) == [(1, 1)]
    assert cr([1024], [1025]) == [(1, 2)] and cr([0], [4096]) == [(0, 4)] and cr([4095], [4096]) == [(3, 5)]
    assert cr([5000, 0, 7, 5000], [10, 0, 0, 10]) == [(4, 1), (4, 1)]          # writes of no bytes are dropped, the order and repeats stay
    assert cr([], []) == [] and cr(2048, 1) == [(2, 1)]
    assert cr([(1 << 40) + 1023], [2]) == [(1 << 30, 2)]
    with pytest.raises(m.B3WError):
        m.bao.chunk_ranges([0, 1], [1])
    with pytest.raises(m.B3WError):
        m.bao.chunk_ranges([-1], [1])
    with pytest.raises(m.B3WError):
        m.bao.chunk_ranges([0], [-1])
