"""Bao outboards over chunk groups without a GPU: the format (where BLAKE3's tree splits, the pre-order places in group units, a
chunk's path as stored part + recomputed part) for every chunk count 1 ... 699 and g = 0 ... 6 against the tree shape of
tests/bao_ref.py; the restatement (tests/bao_groups_ref.py) against the full outboard filtered by node span and against bao's
decoder; and the library's host helpers (b3w_bao_group_outboard_size, b3w_bao_group_batch_layout, b3w_bao_group_path_nodes)
against the restatement and, at g = 0, against the calls for full outboards."""
import ctypes

import numpy as np
import pytest

import b3w_testlib as T
import bao_groups_ref as GR
import bao_ref as R
import blake3_ref as B
import test_bao_cpu as C

GS = range(7)
LENGTHS = sorted(set(C.LENGTHS) | {k * (1 << g) * 1024 + d for g in GS for k in (1, 2, 3) for d in (-1, 0, 1)})


def _preorder_pos(total, a, size):
    """the device function preorder_pos of csrc/b3w_bao.hip: the pre-order place of the node over [a, a + size) of a tree over total"""
    p, lo, cnt = 0, 0, total
    while cnt > 1 and not (lo == a and cnt == size):
        k = R._split(cnt)
        if a < lo + k:
            p, cnt = p + 1, k
        else:
            p, lo, cnt = p + k, lo + k, cnt - k
    assert lo == a and cnt == size
    return p


def _span_path(c, n):
    """(first chunk, chunk count) of the nodes on chunk c's path in a tree over n chunks, root first"""
    out, lo, m = [], 0, n
    while m > 1:
        out.append((lo, m))
        k = R._split(m)
        if c < lo + k:
            m = k
        else:
            lo, m = lo + k, m - k
    return out


@pytest.mark.parametrize("g", GS)
def test_the_format_for_every_chunk_count(g):
    G = 1 << g
    for n in range(1, 700):
        ng = GR.num_groups(n, g)
        spans = GR.node_spans(n)
        big = [(a, m) for a, m in spans if m > G]
        # every node over more than G chunks splits at a multiple of G, so those nodes are the tree over the groups, in its pre-order
        assert all(a % G == 0 and (a + R._split(m)) % G == 0 for a, m in big)
        assert [(a // G, (m + G - 1) // G) for a, m in big] == GR.node_spans(ng), n
        assert len(big) == ng - 1 and GR.group_outboard_size(n * 1024, g) == 8 + 64 * len(big)
        # their places: the device function in group units
        for i, (a, m) in enumerate(big):
            assert _preorder_pos(ng, a // G, (m + G - 1) // G) == i, (n, a, m)
        # a chunk's path: the group's path among the groups, then the path inside a tree over the group's own chunks
        for c in {0, n - 1, n // 2, (n - 1) // G * G, max(0, (n - 1) // G * G - 1), min(n - 1, G), min(n - 1, R._split(n) if n > 1 else 0),
                  max(0, (R._split(n) if n > 1 else 1) - 1)}:
            first = c // G * G
            gn = min(G, n - first)
            upper = [(a * G, min(m * G, n - a * G)) for a, m in _span_path(c // G, ng)]
            lower = [(first + a, m) for a, m in _span_path(c - first, gn)]
            assert upper + lower == _span_path(c, n), (n, c)
            assert [spans.index(x) for x in upper] == [R.path_nodes(c, n)[i] for i in range(len(upper))]
            assert [big.index(x) for x in upper] == GR.group_path_nodes(c, n, g), (n, c)


def test_every_chunk_of_small_trees_has_the_composed_path():
    for g in GS:
        G = 1 << g
        for n in range(1, 200):
            ng = GR.num_groups(n, g)
            for c in range(n):
                first = c // G * G
                assert len(_span_path(c, n)) == len(_span_path(c // G, ng)) + len(_span_path(c - first, min(G, n - first))), (g, n, c)


@pytest.mark.parametrize("length", LENGTHS)
def test_restatement_against_the_full_outboard_and_the_decoder(length):
    data = C._data(length)
    ob, root = R.outboard(data)
    assert root == B.hash_words(data)
    n = R.num_chunks(length)
    for g in GS:
        ob_g, root_g = GR.group_outboard(data, g)
        assert root_g == root, g
        assert ob_g == GR.filter_full_outboard(ob, g), g
        assert len(ob_g) == GR.group_outboard_size(length, g)
        if g == 0:
            assert ob_g == ob
        for c in range(n):
            sl = GR.slice_from_group(ob_g, GR.group_bytes(data, c, g), c, g)
            assert sl == R.slice_chunk(ob, data, c), (g, c)
            a, b = R.chunk_range(length, c)
            assert R.decode_slice(sl, c, root) == data[a:b], (g, c)


def _group_path_nodes(L, c, n, g):
    out = (ctypes.c_uint64 * 64)()
    cnt = ctypes.c_uint32()
    rc = L.b3w_bao_group_path_nodes(c, n, g, out, ctypes.byref(cnt))
    return rc, list(out[:cnt.value])


def test_host_helpers_equal_the_restatement():
    m = T.pkg()
    L = m.lib()
    assert m.bao.MAX_GROUP_LOG == 6
    lens = np.array(LENGTHS + [(1 << 30) + 5, 1 << 30], dtype=np.uint64)
    for g in GS:
        for length in lens:
            assert L.b3w_bao_group_outboard_size(int(length), g) == GR.group_outboard_size(int(length), g) == m.bao.group_outboard_size(int(length), g)
        assert L.b3w_bao_group_outboard_size(1 << 30, 4) == 4194248 and L.b3w_bao_outboard_size(1 << 30) == 67108808
        ob_first = np.zeros(lens.size + 1, dtype=np.uint64)
        total = L.b3w_bao_group_batch_layout(lens.ctypes.data, lens.size, g, ob_first.ctypes.data)
        want = np.concatenate([[0], np.cumsum([GR.group_outboard_size(int(x), g) for x in lens])])
        assert list(ob_first) == list(want) and total == int(want[-1]) and (ob_first % 8 == 0).all()
        assert list(m.bao.group_batch_layout(lens, g)) == list(want)
        for n in list(range(1, 140)) + [255, 256, 257, 699, 1000, 4097]:
            for c in range(n) if n < 140 else sorted({0, n - 1, n // 2, (n - 1) >> g << g, 1 << g, 64, 65, 127, 128}):
                if c >= n:
                    continue
                rc, idx = _group_path_nodes(L, c, n, g)
                assert rc == 0 and idx == GR.group_path_nodes(c, n, g) == m.bao.group_path_nodes(c, n, g), (g, n, c)


def test_group_log_zero_is_the_full_outboard():
    L = T.pkg().lib()
    lens = np.array(LENGTHS + [(1 << 30) + 5], dtype=np.uint64)
    for length in lens:
        assert L.b3w_bao_group_outboard_size(int(length), 0) == L.b3w_bao_outboard_size(int(length))
    a, b = np.zeros(lens.size + 1, dtype=np.uint64), np.zeros(lens.size + 1, dtype=np.uint64)
    assert L.b3w_bao_group_batch_layout(lens.ctypes.data, lens.size, 0, a.ctypes.data) == L.b3w_bao_batch_layout(lens.ctypes.data, lens.size, b.ctypes.data)
    assert list(a) == list(b)
    for n in list(range(1, 70)) + [255, 256, 257, 1000]:
        for c in range(n):
            assert _group_path_nodes(L, c, n, 0) == C._path_nodes(L, c, n), (n, c)


def test_argument_errors():
    m = T.pkg()
    L = m.lib()
    bad = m.B3W_E_BAD_ARGUMENT
    lens = np.array([5000, 70000], dtype=np.uint64)
    ob_first = np.zeros(3, dtype=np.uint64)
    out = (ctypes.c_uint64 * 64)()
    cnt = ctypes.c_uint32()
    # a group_log above B3W_BAO_MAX_GROUP_LOG
    assert L.b3w_bao_group_outboard_size(5000, 7) == 0
    assert L.b3w_bao_group_batch_layout(lens.ctypes.data, 2, 7, ob_first.ctypes.data) == 0
    assert _group_path_nodes(L, 0, 5, 7)[0] == bad
    for call in (m.bao.group_outboard_size, m.bao.group_batch_layout):
        with pytest.raises(m.B3WError):
            call(5000, 7)
    with pytest.raises(m.B3WError):
        m.bao.group_path_nodes(0, 5, 7)
    # a chunk at or past the count, no chunks
    assert _group_path_nodes(L, 5, 5, 2)[0] == bad and _group_path_nodes(L, 6, 5, 2)[0] == bad and _group_path_nodes(L, 0, 0, 2)[0] == bad
    assert _group_path_nodes(L, 4, 5, 2) == (0, [0])
    # null pointers
    assert L.b3w_bao_group_path_nodes(0, 5, 2, None, ctypes.byref(cnt)) == bad
    assert L.b3w_bao_group_path_nodes(0, 5, 2, out, None) == bad
    assert L.b3w_bao_group_batch_layout(lens.ctypes.data, 2, 2, None) == 0
    assert L.b3w_bao_group_batch_layout(None, 2, 2, ob_first.ctypes.data) == 0
    assert L.b3w_bao_group_outboard_batch_device(None, None, None, None, 0, 2, None, None, None, 0, None) == bad
    assert L.b3w_sample_plan_group_batch_device(None, None, 0, 2, None, None, None, None, 0, None, None, None, None) == bad
