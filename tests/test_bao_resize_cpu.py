"""Outboards of files after appends and truncations, without a GPU: the library's host call (b3w_bao_outboard_resize, bao.resize_host)
against a yardstick it does not touch (tests/bao_resize_ref.py: b3w_bao_outboard_update with every chunk dirty, itself shown equal to the
plain-Python restatement), every byte, on every transition; that the kept tiles' bytes are never read and their nodes moved, not
recomputed, by poison; b3w_bao_resize_kept_tiles and b3w_bao_resize_scratch_bytes against counts made here; the names, the ABI number
and the refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import b3w_testlib as T
import bao_groups_ref as GR
import bao_resize_ref as RR

K, M, GS = RR.K, RR.M, RR.GS
NAMES = {"b3w_bao_resize_kept_tiles": 2, "b3w_bao_resize_scratch_bytes": 3, "b3w_bao_outboard_resize_batch_device": 18, "b3w_bao_outboard_resize": 7}


def _host(L, file_bytes, old_ob, old_len, g):
    """b3w_bao_outboard_resize -> (outboard bytes, root words)"""
    out = np.full(GR.group_outboard_size(len(file_bytes), g), 0xA5, dtype=np.uint8)
    rw = np.zeros(8, dtype=np.uint32)
    assert L.b3w_bao_outboard_resize(file_bytes, len(file_bytes), old_ob, old_len, g, out.ctypes.data, rw.ctypes.data) == 0
    return out.tobytes(), [int(x) for x in rw]


def test_the_names_are_declared_exported_and_bound():
    m = T.pkg()
    L = m.lib()
    hdr = open(os.path.join(T.ROOT, "include", "b3wit.h")).read()
    declared = set(re.findall(r"\b(b3w_[a-z0-9_]+)\s*\(", hdr))
    for name, n_args in NAMES.items():
        assert name in declared and name in m.EXPORTED_SYMBOLS, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_args, name
    assert L.b3w_bao_outboard_resize_batch_device.restype is ctypes.c_int32 and L.b3w_bao_outboard_resize.restype is ctypes.c_int32
    assert L.b3w_bao_resize_kept_tiles.restype is ctypes.c_uint64 and L.b3w_bao_resize_scratch_bytes.restype is ctypes.c_uint64
    assert L.b3w_abi_version() == (1 << 16) + 4                                # new names only: the number stays
    for name in ("resize_kept_tiles", "outboard_resize_batch", "resize_host"):
        assert callable(getattr(m.bao, name)), name


def test_kept_tiles():
    m = T.pkg()
    L = m.lib()
    for (old, new), want in (((0, 0), 0), ((M - 1, 5 * M), 0), ((M, M), 1), ((3 * M + 5, 2 * M), 2), ((2 * M, 3 * M + 5), 2)):
        assert L.b3w_bao_resize_kept_tiles(old, new) == want == m.bao.resize_kept_tiles(old, new) == RR.kept_tiles(old, new), (old, new)


def test_scratch_sizes_equal_counts_made_here():
    L = T.pkg().lib()
    #       0    1      2       3          4              5                 6 (1 026 tiles)       7 (exactly 1 024)
    lens = [0, 5 * K, 64 * K, M, M + 1, 2051 * K - 300, (1 << 30) + (1 << 20) + 5, 1 << 30]
    want_slots = [0, 0, 0, 0, 2, 3, 1026 + 2, 1024]
    assert [RR.scratch_slots(x) for x in lens] == want_slots
    ln = np.array(lens, dtype=np.uint64)
    for files in ([0], [3], [4], [5], [6], [7], [0, 1, 2, 3], [6, 4, 5, 1], [4, 4], [6, 5, 6, 0], list(range(8))):
        fi = np.array(files, dtype=np.uint32)
        assert L.b3w_bao_resize_scratch_bytes(ln.ctypes.data, fi.ctypes.data, fi.size) == 32 * sum(want_slots[f] for f in files), files
    fi = np.array([6], dtype=np.uint32)
    assert L.b3w_bao_resize_scratch_bytes(None, None, 0) == 0 and L.b3w_bao_resize_scratch_bytes(ln.ctypes.data, fi.ctypes.data, 0) == 0
    assert L.b3w_bao_resize_scratch_bytes(None, fi.ctypes.data, 1) == 0 and L.b3w_bao_resize_scratch_bytes(ln.ctypes.data, None, 1) == 0


def test_the_yardstick_equals_the_restatement():
    """once: the all-dirty update walk against bao_groups_ref at one length above 2 MiB and at the small lengths it serves"""
    big = 2 * M + 5 * K
    arr = RR.stream()[:big]
    for g in (0, 4):
        assert RR.all_dirty(arr.tobytes(), g) == GR.group_outboard_np(arr, g), g
    for length in (41 * K, 64 * K, 65 * K):
        for g in GS:
            assert RR.all_dirty(RR.data(length), g) == GR.group_outboard(RR.data(length), g), (length, g)


@pytest.mark.parametrize("g", GS)
def test_every_transition_equals_the_yardstick(g):
    m = T.pkg()
    L = m.lib()
    for old, new in RR.TRANSITIONS:
        old_ob, _ = RR.yardstick(old, g)
        want = RR.yardstick(new, g)
        assert _host(L, RR.data(new), old_ob, old, g) == want, (old, new, g)
        got_ob, got_root = m.bao.resize_host(RR.data(new), old_ob, old, g)
        assert (got_ob, [int(x) for x in got_root]) == want, (old, new, g)


@pytest.mark.parametrize("g", GS)
def test_kept_tiles_are_not_read_and_their_nodes_are_moved(g):
    L = T.pkg().lib()
    seen = 0
    for old, new in RR.TRANSITIONS:
        kept = RR.kept_tiles(old, new)
        if not kept:
            continue
        seen += 1
        old_ob, _ = RR.yardstick(old, g)
        want_ob, want_root = RR.yardstick(new, g)                              # (made from the true bytes, before the poison)
        before = bytes(bytearray(old_ob))
        poisoned = b"\xEE" * (kept * M) + RR.data(new)[kept * M:]
        assert _host(L, poisoned, old_ob, old, g) == (want_ob, want_root), (old, new, g)
        assert old_ob == before                                                # the old outboard is only read
        # (a file that is now whole kept tiles, as M + 1 -> M or 9M + 3K -> 4M, was all poison: no byte of it is read)
        # a flipped byte in a node of a kept block that is not the block's first: the same byte at the node's new place, nothing else
        for tile in sorted({0, kept - 1}):
            p_old, p_new = L.b3w_bao_stream_open_block_pos(old, g, tile), L.b3w_bao_stream_open_block_pos(new, g, tile)
            nodes = (1024 >> g) - 1
            for node in sorted({1, nodes - 1}):
                at_old, at_new = 8 + 64 * (p_old + node) + 13, 8 + 64 * (p_new + node) + 13
                bent = bytearray(old_ob)
                bent[at_old] ^= 0x40
                got_ob, got_root = _host(L, RR.data(new), bytes(bent), old, g)
                expect = bytearray(want_ob)
                expect[at_new] ^= 0x40
                assert got_ob == bytes(expect) and got_root == want_root, (old, new, g, tile, node)
    assert seen >= 8


def test_refusals_that_need_no_device():
    m = T.pkg()
    L = m.lib()
    bad = m.B3W_E_BAD_ARGUMENT
    g, old, new = 1, M + 1, 2 * M + 5 * K
    old_ob, _ = RR.yardstick(old, g)
    file_bytes = RR.data(new)
    out = np.full(GR.group_outboard_size(new, g), 0xA5, dtype=np.uint8)
    rw = np.full(8, 0xA5A5A5A5, dtype=np.uint32)
    src = np.frombuffer(old_ob, dtype=np.uint8).copy()

    def call(d=file_bytes, n=new, o=src.ctypes.data, ol=old, gl=g, w=out.ctypes.data, r=rw.ctypes.data):
        return L.b3w_bao_outboard_resize(d, n, o, ol, gl, w, r)
    assert call(d=None) == bad and call(o=None) == bad and call(w=None) == bad and call(r=None) == bad and call(gl=7) == bad
    assert call(n=(1 << 40) + 1) == bad and call(ol=(1 << 40) + 1) == bad      # more than 2^30 chunks
    assert call(w=src.ctypes.data) == bad and call(w=src.ctypes.data + src.size - 8) == bad and call(o=out.ctypes.data + 64) == bad   # overlaps
    assert (out == 0xA5).all() and (rw == 0xA5A5A5A5).all() and src.tobytes() == old_ob      # a refused call writes nothing
    assert call() == 0 and (out.tobytes(), [int(x) for x in rw]) == RR.yardstick(new, g)
    # no byte is needed for a truncation to whole tiles: a null file is taken
    want = RR.yardstick(M, g)
    out1 = np.zeros(GR.group_outboard_size(M, g), dtype=np.uint8)
    assert L.b3w_bao_outboard_resize(None, M, src.ctypes.data, old, g, out1.ctypes.data, rw.ctypes.data) == 0
    assert (out1.tobytes(), [int(x) for x in rw]) == want
    # the Python calls, before they touch a device
    for gl in (-1, 7):
        with pytest.raises(m.B3WError, match="group_log"):
            m.bao.resize_host(file_bytes, old_ob, old, gl)
        with pytest.raises(m.B3WError, match="group_log"):
            m.bao.outboard_resize_batch(None, None, [0], [10], [20], None, [0], None, [0], None, [0], group_log=gl)
    with pytest.raises(m.B3WError, match="size"):
        m.bao.resize_host(file_bytes, old_ob + bytes(64), old, g)
    with pytest.raises(m.B3WError, match="size"):
        m.bao.resize_host(file_bytes, old_ob, old, 0)
    with pytest.raises(m.B3WError, match="negative"):
        m.bao.resize_host(file_bytes, old_ob, -1, g)
    with pytest.raises(m.B3WError, match="negative"):
        m.bao.resize_kept_tiles(-1, 5)
    with pytest.raises(m.B3WError, match="2 offsets, 1 old and 2 new"):
        m.bao.outboard_resize_batch(None, None, [0, 0], [10], [20, 20], None, [0, 0], None, [0, 0], None, [0])
    with pytest.raises(m.B3WError, match="outboard places"):
        m.bao.outboard_resize_batch(None, None, [0, 0], [10, 10], [20, 20], None, [0], None, [0, 0], None, [0])
    with pytest.raises(m.B3WError, match="file index 2"):
        m.bao.outboard_resize_batch(None, None, [0, 0], [10, 10], [20, 20], None, [0, 0], None, [0, 0], None, [0, 2])
    with pytest.raises(m.B3WError, match="listed twice"):
        m.bao.outboard_resize_batch(None, None, [0, 0], [10, 10], [20, 20], None, [0, 0], None, [0, 0], None, [1, 0, 1])
    assert m.bao.outboard_resize_batch(None, None, [0], [10], [20], None, [0], None, [0], None, []) is None     # nothing listed: nothing done
    # the device call's refusals that come before a context is used
    one = (ctypes.c_uint64 * 1)(0)
    assert L.b3w_bao_outboard_resize_batch_device(None, None, 0, None, None, None, 0, 0, None, None, None, None, None, None, 0, None, 0, None) == bad
    assert L.b3w_bao_outboard_resize_batch_device(None, one, 8, one, one, one, 1, 0, one, one, one, one, one, one, 1, None, 0, None) == bad
    assert one[0] == 0
