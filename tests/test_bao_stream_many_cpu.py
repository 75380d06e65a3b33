"""Host-only parts of the calls that push and finish many stream sessions at once (b3w_bao_stream_push_many / _finish_many,
bao.push_many / finish_many / outboard_stream_many / verify_stream_many): the names are declared, exported and bound; a null context
is refused before anything is touched; the helpers refuse their bad arguments before they make anything on a device.  (n = 0 with a
context, and null arrays and sessions with one, need a context and so a device: tests/test_gpu_bao_stream_many.py.)"""
import os
import re

import numpy as np
import pytest

import b3w_testlib as T

TILE = 1 << 20
NAMES = ("b3w_bao_stream_push_many", "b3w_bao_stream_finish_many")


def test_the_two_names_are_declared_exported_and_bound():
    m = T.pkg()
    L = m.lib()
    hdr = open(os.path.join(T.ROOT, "include", "b3wit.h")).read()
    declared = set(re.findall(r"\b(b3w_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in m.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert L.b3w_abi_version() == (1 << 16) + 4                                # new names only: the number stays


def test_a_null_context_is_refused_whatever_else_is_given():
    m = T.pkg()
    L = m.lib()
    one = np.zeros(1, dtype=np.uint64)
    assert L.b3w_bao_stream_push_many(None, None, None, None, None, 0, None) == m.B3W_E_BAD_ARGUMENT
    assert L.b3w_bao_stream_push_many(None, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, None) == m.B3W_E_BAD_ARGUMENT
    assert L.b3w_bao_stream_finish_many(None, None, 0, None) == m.B3W_E_BAD_ARGUMENT
    assert L.b3w_bao_stream_finish_many(None, one.ctypes.data, 1, None) == m.B3W_E_BAD_ARGUMENT


def test_the_python_calls_exist_and_take_nothing_as_nothing():
    m = T.pkg()
    for name in ("push_many", "finish_many", "outboard_stream_many", "verify_stream_many"):
        assert callable(getattr(m.bao, name)), name
    m.bao.push_many([], [], [])                                                # no session: no context is asked for
    assert m.bao.finish_many([]) == []
    with pytest.raises(m.B3WError):
        m.bao.push_many([], [0], [])


@pytest.mark.parametrize("helper", ["outboard_stream_many", "verify_stream_many"])
def test_the_helpers_refuse_bad_arguments_before_touching_a_device(helper):
    m = T.pkg()
    src = [b"\0" * 10, b"\0" * 20]

    def call(sources, lengths, window_bytes, lanes, ring=2, g=0):                # (no context, no outboards: a refusal needs neither)
        if helper == "outboard_stream_many":
            return m.bao.outboard_stream_many(None, sources, lengths, window_bytes, g, lanes, ring)
        return m.bao.verify_stream_many(None, sources, lengths, None, None, window_bytes, g, lanes, ring)
    for lanes in (0, -1):
        with pytest.raises(m.B3WError, match="lanes"):
            call(src, [10, 20], TILE, lanes)
    for window in (0, -TILE, TILE - 1, TILE + 1024, 3 * TILE // 2):
        with pytest.raises(m.B3WError, match="1 MiB"):
            call(src, [10, 20], window, 2)
    with pytest.raises(m.B3WError, match="lengths"):
        call(src, [10], TILE, 2)
    with pytest.raises(m.B3WError, match="ring"):
        call(src, [10, 20], TILE, 2, ring=0)
    with pytest.raises(m.B3WError, match="group_log"):
        call(src, [10, 20], TILE, 2, g=7)


def test_the_helpers_defaults_are_whole_tiles_and_at_least_a_lane():
    m = T.pkg()
    assert m.bao.DEFAULT_MANY_WINDOW_BYTES % TILE == 0 and m.bao.DEFAULT_MANY_WINDOW_BYTES > 0 and m.bao.DEFAULT_MANY_LANES >= 1
