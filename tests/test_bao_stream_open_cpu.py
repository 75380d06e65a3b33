"""Host-only parts of the open-length outboard sessions (b3w_bao_stream_open_*, bao.StreamOutboardOpen / outboard_stream_open): the
names are declared, exported and bound; the staging size; b3w_bao_stream_open_block_pos held against the path calls, which is the
contiguity the design rests on (a full tile's stored nodes are one run of the file's pre-order outboard, in the order they have in a
file of that one tile); null handles are refused; the helper refuses bad arguments before it makes anything on a device."""
import ctypes
import os
import re

import pytest

import b3w_testlib as T

MIB = 1 << 20
NONE = (1 << 64) - 1
NAMES = ("b3w_bao_stream_open_staging_bytes", "b3w_bao_stream_open_scratch_bytes", "b3w_bao_stream_open_block_pos",
         "b3w_bao_stream_open_begin", "b3w_bao_stream_open_finish")
LENGTHS = (2 * MIB, 3 * MIB, 3 * MIB + 5, 5 * MIB + 5, 1025 * MIB + 1)


def test_the_names_are_declared_exported_and_bound():
    m = T.pkg()
    L = m.lib()
    hdr = open(os.path.join(T.ROOT, "include", "b3wit.h")).read()
    declared = set(re.findall(r"\b(b3w_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in m.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert re.search(r"#define\s+B3W_BAO_STREAM_OPEN\s+2\b", hdr)
    assert m.bao.STREAM_OPEN == 2
    for name in ("StreamOutboardOpen", "outboard_stream_open"):
        assert callable(getattr(m.bao, name)), name
    assert L.b3w_abi_version() == (1 << 16) + 4                                # new names only: the number stays


def test_the_staging_is_a_block_per_whole_mib_of_capacity_and_a_fixed_pad():
    m = T.pkg()
    L = m.lib()
    hdr = open(os.path.join(T.ROOT, "include", "b3wit.h")).read()
    pad = int(re.search(r"#define\s+B3W_BAO_STREAM_OPEN_STAGING_PAD\s+(\d+)", hdr).group(1))
    assert pad == m.bao.OPEN_STAGING_PAD and pad % 16 == 0

    def blocks(capacity, g):
        return L.b3w_bao_stream_open_staging_bytes(capacity, g) - pad
    assert blocks(0, 0) == 0 and blocks(MIB - 1, 0) == 0
    assert blocks(MIB, 0) == 65472
    assert blocks(3 * MIB + 5, 4) == 3 * 63 * 64
    for g in range(7):
        assert blocks(7 * MIB, g) == 7 * ((1024 >> g) - 1) * 64
    assert L.b3w_bao_stream_open_staging_bytes(3 * MIB, 7) == 0                # (exactly: no pad either)
    # the scratch: a slot per tile, the tail's included, and per 1 024 of them; never nothing
    assert L.b3w_bao_stream_open_scratch_bytes(0) == 64
    assert L.b3w_bao_stream_open_scratch_bytes(3 * MIB + 5) == (4 + 1) * 32
    assert L.b3w_bao_stream_open_scratch_bytes(1025 * MIB) == (1025 + 2) * 32
    for n in (1, MIB, 5 * MIB + 5, 1025 * MIB + 1):                           # enough for a known-length session of any length up to it
        assert L.b3w_bao_stream_open_scratch_bytes(n) >= L.b3w_bao_stream_scratch_bytes(n, m.bao.STREAM_OUTBOARD)


@pytest.mark.parametrize("g", [0, 4, 6])
@pytest.mark.parametrize("length", LENGTHS)
def test_block_pos_is_where_the_tiles_nodes_start_and_they_are_one_run(length, g):
    m = T.pkg()
    L = m.lib()
    n = m.bao.num_chunks(length)
    inside = 10 - g                                                            # stored nodes of a chunk's path at or below its tile's root
    full = length // MIB
    tiles = sorted(set(list(range(min(full, 4))) + list(range(max(0, full - 3), full))))
    assert tiles
    for t in tiles:
        pos = L.b3w_bao_stream_open_block_pos(length, g, t)
        path = m.bao.group_path_nodes(1024 * t, n, g) if g else m.bao.path_nodes(1024 * t, n)
        assert pos == path[len(path) - inside], (t, pos, path)                 # the path node that covers exactly the tile
        for j in (0, 1, 63, 64, 511, 512, 1023):
            path = m.bao.group_path_nodes(1024 * t + j, n, g) if g else m.bao.path_nodes(1024 * t + j, n)
            local = m.bao.group_path_nodes(j, 1024, g) if g else m.bao.path_nodes(j, 1024)
            assert len(local) == inside and local[0] == 0
            assert path[len(path) - inside:] == [pos + k for k in local], (t, j)
    # the block ends inside the outboard: its last node is below the node count
    last = L.b3w_bao_stream_open_block_pos(length, g, full - 1) + (1024 >> g) - 1
    assert 8 + 64 * last <= m.bao.group_outboard_size(length, g)
    # not a full tile of this file: the ragged last tile (or the tile behind the end), a tile past the end; no such group_log
    assert L.b3w_bao_stream_open_block_pos(length, g, full) == NONE
    assert L.b3w_bao_stream_open_block_pos(length, g, full + 7) == NONE
    assert L.b3w_bao_stream_open_block_pos(length, 7, 0) == NONE


def test_a_file_of_one_tile_is_its_own_block_and_shorter_files_have_none():
    L = T.pkg().lib()
    for g in range(7):
        assert L.b3w_bao_stream_open_block_pos(MIB, g, 0) == 0
        assert L.b3w_bao_stream_open_block_pos(MIB - 1, g, 0) == NONE
        assert L.b3w_bao_stream_open_block_pos(0, g, 0) == NONE


def test_null_handles_are_refused_by_every_entry_point():
    m = T.pkg()
    L = m.lib()
    h = ctypes.c_void_p()
    buf = (ctypes.c_uint8 * 64)()
    n = ctypes.c_uint64(7)
    assert L.b3w_bao_stream_open_begin(None, MIB, 0, buf, 1 << 20, buf, 1 << 20, ctypes.byref(h)) == m.B3W_E_BAD_ARGUMENT
    assert not h.value
    assert L.b3w_bao_stream_open_begin(None, MIB, 0, buf, 1 << 20, buf, 1 << 20, None) == m.B3W_E_BAD_ARGUMENT
    assert L.b3w_bao_stream_open_finish(None, None, 0, buf, 64, buf, None, ctypes.byref(n)) == m.B3W_E_BAD_ARGUMENT
    assert n.value == 7
    assert L.b3w_bao_stream_open_finish(None, buf, 5, buf, 64, buf, None, None) == m.B3W_E_BAD_ARGUMENT
    assert L.b3w_bao_stream_push(None, 0, buf, MIB, None) == m.B3W_E_BAD_ARGUMENT
    L.b3w_bao_stream_free(None)


def test_the_python_calls_refuse_bad_arguments_before_touching_a_device():
    m = T.pkg()
    src = b"\0" * 10
    for window in (0, -MIB, MIB - 1, MIB + 1024, 3 * MIB // 2):
        with pytest.raises(m.B3WError, match="1 MiB"):
            m.bao.outboard_stream_open(None, src, MIB, window)
    with pytest.raises(m.B3WError, match="ring"):
        m.bao.outboard_stream_open(None, src, MIB, MIB, ring=0)
    for g in (-1, 7):
        with pytest.raises(m.B3WError, match="group_log"):
            m.bao.outboard_stream_open(None, src, MIB, MIB, group_log=g)
        with pytest.raises(m.B3WError, match="group_log"):
            m.bao.StreamOutboardOpen(None, MIB, group_log=g)
    with pytest.raises(m.B3WError, match="capacity"):
        m.bao.outboard_stream_open(None, src, -1, MIB)
    with pytest.raises(m.B3WError, match="capacity"):
        m.bao.StreamOutboardOpen(None, -1)
    with pytest.raises(m.B3WError, match="capacity"):                          # a buffer is taken whole: its size is known at once
        m.bao.outboard_stream_open(None, src, 9, MIB)
