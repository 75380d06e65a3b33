"""Bao outboards of a batch of files without a GPU: the host helpers of the batch calls (b3w_bao_batch_layout,
b3w_bao_batch_scratch_bytes, b3w_sample_rows_batch) against the plain-Python restatement (tests/bao_ref.py) and against the
single-file helpers, their argument errors, and the tile scheme the device kernels follow restated in Python: tiles are subtrees,
the tree over the tile CVs is BLAKE3's shape again, and merging in place with the odd item waiting gives BLAKE3's tree with every
node at its pre-order place."""
import numpy as np
import pytest

import b3w_testlib as T
import bao_ref as R
from test_bao_cpu import LENGTHS

ORDERS = [LENGTHS + [(1 << 30) + 5, 0],
          [0, (1 << 30) + 5] + LENGTHS[::-1],
          [LENGTHS[(7 * i) % len(LENGTHS)] for i in range(len(LENGTHS))] + [0, 0, (1 << 30) + 5, 1]]


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


@pytest.mark.parametrize("order", range(len(ORDERS)))
def test_layout_is_the_outboard_sizes_summed(order):
    L = T.pkg().lib()
    lens = _u64(ORDERS[order])
    ob_first = np.full(lens.size + 1, 0xFFFFFFFF, dtype=np.uint64)
    total = L.b3w_bao_batch_layout(lens.ctypes.data, lens.size, ob_first.ctypes.data)
    want = [0]
    for ln in ORDERS[order]:
        want.append(want[-1] + 8 + 64 * (R.num_chunks(ln) - 1))
    assert list(ob_first) == want and total == want[-1]
    assert all(int(x) % 8 == 0 for x in ob_first)
    for f, ln in enumerate(ORDERS[order]):
        assert int(ob_first[f + 1] - ob_first[f]) == L.b3w_bao_outboard_size(ln)


@pytest.mark.parametrize("order", range(len(ORDERS)))
def test_scratch_is_within_what_the_single_file_calls_need_together(order):
    L = T.pkg().lib()
    lens = _u64(ORDERS[order])
    need = L.b3w_bao_batch_scratch_bytes(lens.ctypes.data, lens.size)
    bound = sum((2 * R.num_chunks(ln) + 64) * 32 for ln in ORDERS[order])
    tiles = sum((R.num_chunks(ln) + 1023) // 1024 for ln in ORDERS[order])
    print(f"scratch {need} B for {tiles} tiles; the single-file calls together {bound} B")
    assert 0 < need <= bound
    assert need <= 32 * tiles + 32 * len(ORDERS[order])          # one CV per tile, and one per group of 1 024 tiles
    small = _u64([0, 1, 1024, 64 * 1024])                         # files of at most 64 chunks need none
    assert L.b3w_bao_batch_scratch_bytes(small.ctypes.data, small.size) == 0


def test_sample_rows_batch_equals_the_single_file_rows():
    L = T.pkg().lib()
    lens = [1, 1024, 5 * 1024 + 1, 37 * 1024, 100 * 1024 + 77, 0, (1 << 20) + 1]
    rng = np.random.default_rng(4)
    files, chunks = [], []
    for f, ln in enumerate(lens):                                 # the last chunk of every file, a duplicate of it, the first, a few more
        n = R.num_chunks(ln)
        for c in [n - 1, n - 1, 0] + list(rng.integers(0, n, 3)):
            files.append(f)
            chunks.append(int(c))
    perm = rng.permutation(len(files))                           # interleaved over the files
    files = np.ascontiguousarray(np.array(files)[perm], dtype=np.uint32)
    chunks = _u64(np.array(chunks)[perm])
    ln64 = _u64(lens)
    rf = np.zeros(files.size + 1, dtype=np.uint64)
    total = L.b3w_sample_rows_batch(ln64.ctypes.data, ln64.size, files.ctypes.data, chunks.ctypes.data, files.size, rf.ctypes.data)
    row = 0
    for s in range(files.size):
        one = np.zeros(2, dtype=np.uint64)
        c = _u64([chunks[s]])
        k = L.b3w_sample_rows(lens[files[s]], c.ctypes.data, 1, one.ctypes.data)
        a, b = R.chunk_range(lens[files[s]], int(chunks[s]))
        assert k == max(1, (b - a + 63) // 64) + len(R.path_nodes(int(chunks[s]), R.num_chunks(lens[files[s]])))
        assert int(rf[s]) == row
        row += k
    assert total == row and int(rf[-1]) == row


def test_argument_errors():
    m = T.pkg()
    L = m.lib()
    bad = m.B3W_E_BAD_ARGUMENT
    lens = _u64([5 * 1024, 3000])
    rf = np.zeros(3, dtype=np.uint64)

    def rows(files, chunks, n_files=2):
        f, c = np.ascontiguousarray(files, dtype=np.uint32), _u64(chunks)
        return L.b3w_sample_rows_batch(lens.ctypes.data, n_files, f.ctypes.data, c.ctypes.data, f.size, rf.ctypes.data)
    assert rows([0, 1], [4, 2]) > 0
    assert rows([0, 2], [4, 0]) == -bad                           # file index = n_files
    assert rows([0, 1], [5, 0]) == -bad                           # chunk index = chunk count (5 of 5)
    assert rows([0, 1], [0, 3]) == -bad                           # (3 of 3)
    assert rows([0], [0], n_files=0) == -bad                      # no files: every file index is out of range
    assert rows([], [], n_files=0) == 0 and rf[0] == 0            # no files, no samples: nothing
    one = np.full(1, 7, dtype=np.uint64)
    assert L.b3w_bao_batch_layout(None, 0, one.ctypes.data) == 0 and one[0] == 0
    assert L.b3w_bao_batch_scratch_bytes(lens.ctypes.data, 0) == 0
    # without a context nothing can be asked of the device
    assert L.b3w_bao_outboard_batch_device(None, None, None, None, 0, None, None, None, 0, None) == bad
    assert L.b3w_sample_plan_batch_device(None, None, 0, None, None, None, None, 0, None, None, None, None) == bad


# ---- the tile scheme, restated ----------------------------------------------------------------------------------------
def _reference_tree(n):
    """BLAKE3's tree over n chunks by recursion: its parent nodes (left CV, right CV) in pre-order, and its root"""
    nodes = []

    def walk(first, m):
        if m == 1:
            return ("chunk", first)
        k = R._split(m)
        slot = len(nodes)
        nodes.append(None)
        left = walk(first, k)
        right = walk(first + k, m - k)
        nodes[slot] = (left, right)
        return ("parent", left, right)
    return nodes, walk(0, n)


def _preorder_pos(total, a, size):
    """position, relative to the root of a tree over `total` chunks, of its node over chunks [a, a + size)"""
    p, lo, cnt = 0, 0, total
    while cnt > 1 and not (lo == a and cnt == size):
        k = R._split(cnt)
        if a < lo + k:
            p, cnt = p + 1, k
        else:
            p, lo, cnt = p + k, lo + k, cnt - k
    assert (lo, cnt) == (a, size), "not a subtree"
    return p


def _merge_in_place(cv, cnt, unit, total, out, base):
    """cv[i]: the CV of item i (unit chunks each, the last maybe fewer) of a tree over `total` chunks whose root sits at `base`"""
    lvl = 0
    while (1 << lvl) < cnt:
        j = 0
        while ((2 * j) << lvl) + (1 << lvl) < cnt:
            i0 = (2 * j) << lvl
            i1 = i0 + (1 << lvl)
            a = i0 * unit
            size = min((i0 + (2 << lvl)) * unit, total) - a
            p = base + _preorder_pos(total, a, size)
            assert p not in out
            out[p] = (cv[i0], cv[i1])
            cv[i0] = ("parent", cv[i0], cv[i1])
            j += 1
        lvl += 1
    return cv[0]


def _tiled_tree(n, tile):
    """storey by storey: groups of `tile` items merge in place; the groups' CVs are the next storey's items"""
    out = {}
    items, unit = [("chunk", i) for i in range(n)], 1
    while True:
        span = unit * tile
        groups = []
        for g in range((n + span - 1) // span):
            a = g * span
            tot = min(span, n - a)
            cnt = (tot + unit - 1) // unit
            base = _preorder_pos(n, a, tot) if tot > 1 else 0
            groups.append(_merge_in_place(items[g * tile:g * tile + cnt], cnt, unit, tot, out, base))
        if len(groups) == 1:
            return out, groups[0]
        items, unit = groups, span


@pytest.mark.parametrize("tile", [2, 4, 8])
def test_tiles_merged_in_place_are_blake3s_tree(tile):
    for n in list(range(1, 70)) + [100, 127, 128, 129, 255, 256, 257, 300, 1000]:
        nodes, root = _reference_tree(n)
        out, got_root = _tiled_tree(n, tile)
        assert got_root == root, n
        assert sorted(out) == list(range(n - 1)) and all(out[i] == nodes[i] for i in range(n - 1)), n
