"""Host-only parts of finishing many open-length sessions at once (b3w_bao_stream_open_finish_many, bao.open_finish_many /
outboard_stream_open_many): the name is declared, exported and bound, the ABI number stays; a null context is refused; the Python
helper refuses bad arguments before it touches a device (its context here is None)."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

import b3w_testlib as T

MIB = 1 << 20
NAME = "b3w_bao_stream_open_finish_many"


def test_the_name_is_declared_exported_and_bound():
    m = T.pkg()
    L = m.lib()
    hdr = open(os.path.join(T.ROOT, "include", "b3wit.h")).read()
    declared = set(re.findall(r"\b(b3w_[a-z0-9_]+)\s*\(", hdr))
    assert NAME in declared and NAME in m.EXPORTED_SYMBOLS
    fn = getattr(L, NAME)
    assert fn.argtypes is not None and len(fn.argtypes) == 10 and fn.restype is ctypes.c_int32
    assert L.b3w_abi_version() == (1 << 16) + 4                                # new names only: the number stays
    for name in ("open_finish_many", "outboard_stream_open_many"):
        assert callable(getattr(m.bao, name)), name


def test_a_null_context_is_refused():
    m = T.pkg()
    L = m.lib()
    one = (ctypes.c_uint64 * 1)(0)
    lens = (ctypes.c_uint64 * 1)(7)
    assert L.b3w_bao_stream_open_finish_many(None, one, one, one, one, one, one, 1, None, lens) == m.B3W_E_BAD_ARGUMENT
    assert L.b3w_bao_stream_open_finish_many(None, None, None, None, None, None, None, 0, None, None) == m.B3W_E_BAD_ARGUMENT
    assert lens[0] == 7


def test_the_python_calls_refuse_bad_arguments_before_touching_a_device():
    m = T.pkg()
    many = m.bao.outboard_stream_open_many
    src = [b"\0" * 10, io.BytesIO(b"\0" * 10)]
    caps = [MIB, MIB]
    for lanes in (0, -1):
        with pytest.raises(m.B3WError, match="lanes"):
            many(None, src, caps, MIB, lanes=lanes)
    for ring in (0, -2):
        with pytest.raises(m.B3WError, match="ring"):
            many(None, src, caps, MIB, ring=ring)
    for window in (0, -MIB, MIB - 1, MIB + 1024, 3 * MIB // 2):
        with pytest.raises(m.B3WError, match="1 MiB"):
            many(None, src, caps, window)
    for g in (-1, 7):
        with pytest.raises(m.B3WError, match="group_log"):
            many(None, src, caps, MIB, group_log=g)
    with pytest.raises(m.B3WError, match="2 sources and 1 capacities"):
        many(None, src, caps[:1], MIB)
    with pytest.raises(m.B3WError, match="2 sources and 3 capacities"):
        many(None, src, caps + [MIB], MIB)
    with pytest.raises(m.B3WError, match="capacity -1 of source 1 is negative"):
        many(None, src, [MIB, -1], MIB)
    with pytest.raises(m.B3WError, match="source 0 holds 10 bytes, more than its capacity"):   # a buffer is taken whole: its size is known at once
        many(None, src, [9, MIB], MIB)
    with pytest.raises(m.B3WError, match="source 1 holds 12 bytes"):
        many(None, [b"", np.zeros(3, dtype=np.uint32)], [0, 11], MIB)
    assert many(None, [], [], MIB) == []                                       # no file: nothing to make
    with pytest.raises(m.B3WError, match="2 sessions and 1 tails"):
        m.bao.open_finish_many([None, None], [None])
    assert m.bao.open_finish_many([]) == []
