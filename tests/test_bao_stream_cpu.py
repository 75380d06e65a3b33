"""Host-only parts of the stream sessions (b3w_bao_stream_*, bao.windows): the scratch a session needs is the batch calls' for the
one length, at every class boundary of the kernels; the windows the helpers push cover a file exactly once; the header's new names
are exported and bound."""
import ctypes
import os
import re

import numpy as np
import pytest

import b3w_testlib as T

K = 1024
TILE = 1 << 20
NAMES = ("b3w_bao_stream_scratch_bytes", "b3w_bao_stream_outboard_begin", "b3w_bao_stream_verify_begin", "b3w_bao_stream_push",
         "b3w_bao_stream_finish", "b3w_bao_stream_free")
# around 64 chunks (the small kernel's files), one tile (1 024 chunks), 1 024 tiles (the second storey), and the longest file taken
LENS = [0, 1, K - 1, K, K + 1, 63 * K, 64 * K - 1, 64 * K, 64 * K + 1, 65 * K, TILE - 1, TILE, TILE + 1, 2 * TILE, 2049 * K + 3,
        1023 * TILE, 1024 * TILE - 1, 1024 * TILE, 1024 * TILE + 1, 1025 * TILE, 1026 * TILE + 5, 2048 * TILE + 1, (1 << 40) - 1, 1 << 40]


def test_scratch_bytes_are_the_batch_calls_for_one_file():
    m = T.pkg()
    L = m.lib()
    for ln in LENS:
        one = np.array([ln], dtype=np.uint64)
        assert L.b3w_bao_stream_scratch_bytes(ln, m.bao.STREAM_OUTBOARD) == L.b3w_bao_batch_scratch_bytes(one.ctypes.data, 1), ln
        assert L.b3w_bao_stream_scratch_bytes(ln, m.bao.STREAM_VERIFY) == L.b3w_bao_verify_scratch_bytes(one.ctypes.data, 1), ln
        assert m.bao.stream_scratch_bytes(ln, m.bao.STREAM_VERIFY) == L.b3w_bao_stream_scratch_bytes(ln, 1)
    # what the figures are: 32 bytes a tile and a group of 1 024 tiles; 36 an entry, rounded up to 16; nothing below the classes
    assert L.b3w_bao_stream_scratch_bytes(64 * K, 0) == 0 and L.b3w_bao_stream_scratch_bytes(64 * K + 1, 0) == 32
    assert L.b3w_bao_stream_scratch_bytes(TILE, 1) == 0 and L.b3w_bao_stream_scratch_bytes(TILE + 1, 1) == (2 * 36 + 15) // 16 * 16
    assert L.b3w_bao_stream_scratch_bytes(1026 * TILE + 5, 0) == (1027 + 2) * 32
    assert L.b3w_bao_stream_scratch_bytes(1026 * TILE + 5, 1) == ((1027 + 2) * 36 + 15) // 16 * 16
    assert L.b3w_bao_stream_scratch_bytes(TILE + 1, 2) == 0                       # no such kind


@pytest.mark.parametrize("window", [TILE, 2 * TILE, 5 * TILE, 256 * TILE])
def test_windows_cover_the_file_exactly_once(window):
    m = T.pkg()
    for ln in [0, 1, K, TILE - 1, TILE, TILE + 1, 2049 * K + 3, 3 * TILE, 5 * TILE + 5, 10 * TILE, 257 * TILE + 77, 1026 * TILE + 5]:
        w = m.bao.windows(ln, window)
        assert len(w) == (ln + window - 1) // window
        at = 0
        for off, nb in w:
            assert off == at and nb > 0 and off % TILE == 0                      # in order, none empty, from a tile's first byte
            assert nb % TILE == 0 or off + nb == ln                              # whole tiles, or the file's end
            assert nb <= window
            at += nb
        assert at == ln
        assert all(nb == window for _, nb in w[:-1])


def test_windows_refuses_sizes_that_are_not_whole_tiles():
    m = T.pkg()
    for bad in (0, -TILE, TILE - 1, TILE + K, 3 * TILE // 2):
        with pytest.raises(m.B3WError):
            m.bao.windows(10 * TILE, bad)


def test_the_new_names_are_declared_exported_and_bound():
    m = T.pkg()
    L = m.lib()
    hdr = open(os.path.join(T.ROOT, "include", "b3wit.h")).read()
    declared = set(re.findall(r"\b(b3w_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in m.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert "B3W_BAO_STREAM_OUTBOARD 0" in hdr and re.search(r"B3W_BAO_STREAM_VERIFY\s+1", hdr)
    assert (m.bao.STREAM_OUTBOARD, m.bao.STREAM_VERIFY) == (0, 1)


def test_null_sessions_are_refused_on_the_host():
    m = T.pkg()
    L = m.lib()
    assert L.b3w_bao_stream_push(None, 0, None, TILE, None) == m.B3W_E_BAD_ARGUMENT
    assert L.b3w_bao_stream_finish(None, None) == m.B3W_E_BAD_ARGUMENT
    L.b3w_bao_stream_free(None)
    h = ctypes.c_void_p()
    assert L.b3w_bao_stream_outboard_begin(None, TILE, 0, None, None, None, 0, ctypes.byref(h)) == m.B3W_E_BAD_ARGUMENT and not h
