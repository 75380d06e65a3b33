"""The numpy restatement of the chain planner (tests/plan_ref.py) held against what is independent of it (no GPU needed): the
reference WASM's transcript of incomplete trees (tests/golden/incomplete_trees.nova_vesta.json.gz), the pure-Python BLAKE3 of
tests/blake3_ref.py, and the library's host-side index functions."""
import gzip
import json
import os

import numpy as np
import pytest

import b3w_testlib as T
import blake3_ref as B
import plan_ref as R


def test_restatement_equals_the_reference_wasm_transcript():
    """all eight trees, every leaf: the last leaf record, every parent record, final_h and the root, word for word"""
    W = T.workloads()
    doc = json.load(gzip.open(os.path.join(T.GOLD, "incomplete_trees.nova_vesta.json.gz"), "rt"))
    assert [t["n_chunks"] for t in doc["trees"]] == [2, 3, 5, 6, 7, 8, 11, 100]
    seen = 0
    for tree in doc["trees"]:
        n = tree["n_chunks"]
        ref = R.plan(W.lcg_preimage(n * 1024, seed=1))
        assert ref.root.tolist() == tree["root"], n
        assert len(tree["leaves"]) == n
        for leaf in tree["leaves"]:
            c = leaf["leaf"]
            assert ref.plen[c] == leaf["path_len"], (n, c)
            steps = leaf["steps"]                             # the last leaf block, then the parent steps
            assert len(steps) == 1 + ref.plen[c]
            assert ref.leaf[c, ref.n_blocks[c] - 1].tolist() == steps[0]["record"], (n, c)
            rows = ref.parents[ref.parent_first[c]:ref.parent_first[c + 1]]
            for g, stp in enumerate(steps[1:]):
                assert rows[g].tolist() == stp["record"], (n, c, g)
            assert ref.final[c].tolist() == leaf["final_h"], (n, c)
            assert (ref.final[c].tolist() == tree["root"]) == leaf["ends_in_root"], (n, c)
            seen += 1
    assert seen == 142


@pytest.mark.parametrize("nbytes", [1, 1023, 1024, 1025, 5 * 1024 + 1, 1025 * 1024 + 5])
def test_root_is_blake3_of_the_preimage(nbytes):
    data = np.random.default_rng(nbytes).integers(0, 256, nbytes, dtype=np.uint8)
    ref = R.plan(data)
    assert ref.root.tolist() == B.hash_words(data.tobytes())
    assert ref.n_chunks == (nbytes + 1023) // 1024 and ref.n_blocks[-1] == ((nbytes - 1) % 1024) // 64 + 1
    assert ref.cvs[-1].tolist() == B.chunk_cv(data.tobytes()[(ref.n_chunks - 1) * 1024:], ref.n_chunks - 1, ref.n_chunks == 1)
    if ref.n_chunks == 1:
        assert ref.parents.shape[0] == 0 and np.array_equal(ref.final[0], ref.root)


@pytest.mark.parametrize("n", [1025, 2050, 3071])
def test_final_is_the_root_exactly_where_the_library_says_provable_and_rows_agree(n):
    L = T.pkg().lib()
    data = np.random.default_rng(n).integers(0, 256, n * 1024 - 77, dtype=np.uint8)
    ref = R.plan(data)
    ends = (ref.final == ref.root[None, :]).all(axis=1)
    provable = np.array([L.b3w_chain_path_provable(c, n) for c in range(n)], dtype=bool)
    assert np.array_equal(ends, provable) and provable[:1024].all() and not provable[-1]
    assert ref.parent_first.tolist() == [L.b3w_chain_parent_row(c, n) for c in range(n + 1)]
    assert ref.plen.tolist() == [L.b3w_chain_path_len(c, n) for c in range(n)] == [R.path_len(c, n) for c in range(n)]


def test_selected_chunks_and_chunk_ranges_give_the_same_rows():
    """parents_of and the (first_chunk, preimage_len) form are views of the same plan"""
    data = np.random.default_rng(9).integers(0, 256, 11 * 1024 + 70, dtype=np.uint8)
    ref = R.plan(data)
    some = R.plan(data, parents_of=[0, 7, 11])
    for i, c in enumerate([0, 7, 11]):
        assert np.array_equal(some.parents[some.parent_first[i]:some.parent_first[i + 1]], ref.parents[ref.parent_first[c]:ref.parent_first[c + 1]])
        assert np.array_equal(some.final[i], ref.final[c])
    part = R.plan(data[3 * 1024:], first_chunk=3, preimage_len=data.size)
    assert np.array_equal(part.leaf, ref.leaf[3:]) and np.array_equal(part.cvs, ref.cvs[3:]) and np.array_equal(part.n_blocks, ref.n_blocks[3:])
    mid = R.plan(data[3 * 1024:6 * 1024], first_chunk=3, preimage_len=data.size)
    assert np.array_equal(mid.leaf, ref.leaf[3:6]) and np.array_equal(mid.cvs, ref.cvs[3:6])
    rows = ref.records_of(3, 12)
    assert rows.shape[0] == 8 * 16 + 2 + ref.parent_first[12] - ref.parent_first[3]
    assert np.array_equal(rows[8 * 16 + 1], ref.leaf[11, 1]) and np.array_equal(rows[8 * 16 + 2], ref.parents[ref.parent_first[3]])
