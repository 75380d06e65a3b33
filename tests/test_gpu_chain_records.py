"""Chained pass: EVERY step record of large, ragged and sharded trees against the numpy restatement of the planner
(tests/plan_ref.py, itself pinned to the reference WASM's transcript by tests/test_plan_ref_cpu.py).

The shapes are the smallest that open a branch of csrc/b3w_plan.hip / csrc/b3w_chain.cpp which no record was ever held against:
the tree kernel with levels merged by earlier launches (more than 1 024 chunks: carries that wait in HBM beside carries that wait
in LDS), the fused tree + path plan on incomplete trees and chunk sub-ranges, the one-thread-per-chunk leaf kernel and both
leaf kernels' byte paths on unaligned sources, the driver's ragged slices and one-step batches, and chunk indices across 2^32."""
import ctypes
import functools

import numpy as np
import pytest

import b3w_testlib as T
import plan_ref as R
import ref_models as RM

pytestmark = pytest.mark.gpu


# ---- shared, read-only expectations ---------------------------------------------------------------------------------------------
def _freeze(ref):
    for v in vars(ref).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _case(n_chunks, last_bytes):
    """seeded random preimage of n_chunks chunks whose last chunk has last_bytes bytes, and its restated plan"""
    nbytes = (n_chunks - 1) * 1024 + last_bytes
    data = np.random.default_rng(n_chunks * 2048 + last_bytes).integers(0, 256, nbytes, dtype=np.uint8)
    data.setflags(write=False)
    return data, _freeze(R.plan(data))


def _same(got, want, what):
    """whole-array equality; on failure the first differing (chunk, row, word)"""
    got, want = np.asarray(got).view(np.uint32), np.asarray(want).view(np.uint32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    g2, w2 = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    row, word = (int(x[0]) for x in np.nonzero(g2 != w2))
    chunk = int(w2[row, 10]) | (int(w2[row, 11]) << 32) if w2.shape[1] == 32 else row
    raise AssertionError(f"{what}: first difference at chunk {chunk}, row {row}, word {word}: got {g2[row, word]:#x}, want {w2[row, word]:#x}; "
                         f"{int((g2 != w2).any(axis=1).sum())} of {g2.shape[0]} rows differ")


@pytest.fixture(scope="module")
def ctx():
    c = T.pkg().Context("nova_vesta", 0)
    yield c
    c.close()


def _dev():
    import torch
    return torch.device("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint32)


# ---- the planner alone ----------------------------------------------------------------------------------------------------------
TREES = [(1024, 1024),     # l0 = 0 at its upper edge, complete tree
         (1025, 5),        # l0 = 1: one carry waiting in HBM, none in LDS; a one-block last chunk
         (2047, 1024),     # l0 = 1: the HBM carry plus a carry at every LDS level (11 segments)
         (2049, 64),       # l0 = 1 with level 1 of exactly 1 024 nodes
         (2050, 65),       # l0 = 2: level 0 even, the carry of level 1 in HBM only
         (3071, 700),      # l0 = 2: carries at both HBM levels and at the LDS levels
         (6145, 64)]       # l0 = 3: one HBM carry and one LDS carry far apart (segments 4 096, 2 048, 1)


@pytest.mark.parametrize("n_chunks,last_bytes", TREES, ids=[f"{n}x{b}" for n, b in TREES])
def test_every_record_of_trees_merged_over_several_launches(ctx, n_chunks, last_bytes):
    import torch
    data, ref = _case(n_chunks, last_bytes)
    plan = T.pkg().ChainPlanner(ctx).plan(torch.from_numpy(data.copy()).to(_dev()))
    torch.cuda.synchronize()
    n_leaf = int(ref.n_blocks.sum())
    assert (plan["n_chunks"], plan["n_leaf_steps"], plan["n_parent_steps"]) == (n_chunks, n_leaf, int(ref.parent_first[-1]))
    want = ref.records_of(0, n_chunks)
    got = _host(plan["records"])
    _same(_host(plan["root"]), ref.root, "root")
    _same(_host(plan["chunk_cvs"]), ref.cvs, "chunk CVs")
    _same(got[:n_leaf], want[:n_leaf], "leaf records")
    _same(got[n_leaf:], want[n_leaf:], "parent records")


SPLITS = [(3071, 700, (0, 1000, 2048, 3071)), (6145, 64, (0, 4096, 6144, 6145))]


@pytest.mark.parametrize("n_chunks,last_bytes,cuts", SPLITS, ids=["3071", "6145"])
def test_chunk_sub_ranges_get_their_rows_of_the_same_plan(ctx, n_chunks, last_bytes, cuts):
    import torch
    data, ref = _case(n_chunks, last_bytes)
    d_pre = torch.from_numpy(data.copy()).to(_dev())
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        plan = T.pkg().ChainPlanner(ctx).plan(d_pre, first_chunk=lo, n_chunks_local=hi - lo)
        torch.cuda.synchronize()
        n_leaf = int(ref.n_blocks[lo:hi].sum())
        assert (plan["n_leaf_steps"], plan["n_parent_steps"]) == (n_leaf, int(ref.parent_first[hi] - ref.parent_first[lo])), (lo, hi)
        want, got = ref.records_of(lo, hi), _host(plan["records"])
        _same(got[:n_leaf], want[:n_leaf], f"leaf records of chunks [{lo}, {hi})")
        _same(got[n_leaf:], want[n_leaf:], f"parent records of chunks [{lo}, {hi})")
        _same(_host(plan["root"]), ref.root, "root")


def _at_offset(data, offset):
    """the preimage in device memory, starting `offset` bytes past a 256-byte boundary (a slice of a larger tensor)"""
    import torch
    big = torch.zeros(data.size + 512, dtype=torch.uint8, device=_dev())
    skip = (-big.data_ptr()) % 256 + offset
    view = big[skip:skip + data.size]
    view.copy_(torch.from_numpy(data.copy()))
    assert view.data_ptr() % 256 == offset and view.is_contiguous()
    return view


@pytest.mark.parametrize("offset", [0, 1, 4])
def test_quad_leaf_kernel_reads_an_unaligned_source(ctx, offset):
    import torch
    data, ref = _case(38, 333)
    plan = T.pkg().ChainPlanner(ctx).plan(_at_offset(data, offset))
    torch.cuda.synchronize()
    n_leaf = int(ref.n_blocks.sum())
    _same(_host(plan["records"])[:n_leaf], ref.records_of(0, 38)[:n_leaf], "leaf records")
    _same(_host(plan["chunk_cvs"]), ref.cvs, "chunk CVs")
    _same(_host(plan["root"]), ref.root, "root")
    _same(_host(plan["records"])[n_leaf:], ref.parents, "parent records")


BIG = 65537                                                   # more than 65 536 chunks in one call: one thread per chunk


@functools.lru_cache(maxsize=None)
def _big_case():
    nbytes = (BIG - 1) * 1024 + 77
    data = np.random.default_rng(BIG).integers(0, 256, nbytes, dtype=np.uint8)
    data.setflags(write=False)
    return data, _freeze(R.plan(data, parents_of=[0, BIG - 2, BIG - 1]))


def test_one_thread_per_chunk_leaf_kernel_and_the_tree_above_it(ctx):
    """65 537 chunks, a 77-byte last chunk: every leaf record and chunk CV of ONE b3w_chain_plan_leaves_device call at source
    offsets 0 (words, and bytes for the short block), 1 (bytes) and 4 (words); the same preimage in two calls (65 536 + 1 chunks:
    the four-lanes-per-chunk kernel) gives identical arrays; the tree (six levels merged by launches of their own, the carry of
    level 0 waiting in HBM) ends in the restatement's root; parent records of chunks 0, 65 535 and 65 536."""
    import torch
    L = T.pkg().lib()
    data, ref = _big_case()
    dev, n, ln = _dev(), BIG, data.size
    levels = torch.zeros((2 * n + 64) * 8, dtype=torch.int32, device=dev)
    root = torch.zeros(8, dtype=torch.int32, device=dev)
    first = None
    for offset in (0, 1, 4):
        d_pre = _at_offset(data, offset)
        recs = torch.zeros((n * 16, 32), dtype=torch.int32, device=dev)
        levels.zero_()
        assert L.b3w_chain_plan_leaves_device(ctx.handle, d_pre.data_ptr(), ln, 0, n, recs.data_ptr(), levels.data_ptr(), None) == 0
        torch.cuda.synchronize()
        got = _host(recs).reshape(n, 16, 32)
        _same(got, ref.leaf, f"leaf records, source offset {offset}")
        _same(_host(levels[:n * 8]).reshape(n, 8), ref.cvs, f"chunk CVs, source offset {offset}")
        if offset == 0:
            first = got
    d_pre = _at_offset(data, 0)
    recs2 = torch.zeros((n * 16, 32), dtype=torch.int32, device=dev)
    cvs2 = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    assert L.b3w_chain_plan_leaves_device(ctx.handle, d_pre.data_ptr(), ln, 0, n - 1, recs2.data_ptr(), cvs2.data_ptr(), None) == 0
    assert L.b3w_chain_plan_leaves_device(ctx.handle, d_pre.data_ptr() + (n - 1) * 1024, ln, n - 1, 1, recs2[(n - 1) * 16:].data_ptr(),
                                          cvs2[n - 1:].data_ptr(), None) == 0
    torch.cuda.synchronize()
    _same(_host(recs2).reshape(n, 16, 32), first, "leaf records of two calls against one call")
    _same(_host(cvs2), ref.cvs, "chunk CVs of two calls")
    # the tree over the CVs of the last one-call plan, and three paths through it
    assert L.b3w_chain_tree_device(ctx.handle, levels.data_ptr(), n, root.data_ptr(), None) == 0
    par = torch.zeros((int(ref.parent_first[-1]), 32), dtype=torch.int32, device=dev)
    assert L.b3w_chain_plan_parents_device(ctx.handle, levels.data_ptr(), n, ln, 0, 1, par.data_ptr(), None) == 0
    assert L.b3w_chain_plan_parents_device(ctx.handle, levels.data_ptr(), n, ln, n - 2, 2, par[int(ref.parent_first[1]):].data_ptr(), None) == 0
    torch.cuda.synchronize()
    _same(_host(root), ref.root, "root")
    assert ref.plen[[0, n - 2, n - 1]].tolist() == [17, 17, 1]
    _same(_host(par), ref.parents, "parent records of chunks 0, 65 535, 65 536")


def test_chunk_indices_across_two_to_the_32(ctx):
    """five chunks from 2^32 - 2 on, of a preimage of 2^32 + 3 chunks whose last has 24 bytes: words 10 / 11 of the records, the
    high counter word of the compression (in every running value and chunk CV), the depths of a tree that large"""
    import torch
    L = T.pkg().lib()
    first, nl = (1 << 32) - 2, 5
    ln = ((1 << 32) + 3) * 1024 - 1000
    n = L.b3w_chain_num_chunks(ln)
    assert n == (1 << 32) + 3
    data = np.random.default_rng(32).integers(0, 256, nl * 1024 - 1000, dtype=np.uint8)
    ref = R.plan(data, first_chunk=first, preimage_len=ln)
    assert ref.plen.tolist() == [L.b3w_chain_path_len(first + i, n) for i in range(nl)] == [33, 33, 3, 3, 2]
    assert ref.n_blocks.tolist() == [16, 16, 16, 16, 1] and ref.leaf[4, 0, 31] == 24
    assert ref.leaf[:, 0, 10].tolist() == [0xFFFFFFFE, 0xFFFFFFFF, 0, 1, 2] and ref.leaf[:, 0, 11].tolist() == [0, 0, 1, 1, 1]
    d_pre = torch.zeros(nl * 1024, dtype=torch.uint8, device=_dev())
    d_pre[:data.size] = torch.from_numpy(data.copy())
    recs = torch.zeros((nl * 16, 32), dtype=torch.int32, device=_dev())
    cvs = torch.zeros((nl, 8), dtype=torch.int32, device=_dev())
    assert L.b3w_chain_plan_leaves_device(ctx.handle, d_pre.data_ptr(), ln, first, nl, recs.data_ptr(), cvs.data_ptr(), None) == 0
    torch.cuda.synchronize()
    _same(_host(recs).reshape(nl, 16, 32), ref.leaf, "leaf records")
    _same(_host(cvs), ref.cvs, "chunk CVs")


# ---- the streamed driver: witnesses go through the ring ---------------------------------------------------------------------------
def _drive(ctx, data, ref, first, nl, batch_steps, ring, all_cvs=None):
    """b3w_chain_create(first, nl) -> run_leaves (the whole host preimage) -> run_parents, with a consumer that notes every batch
    and clones a few bodies while they sit in the ring.  Checks everything the pass leaves behind against the restatement's rows of
    chunks [first, first + nl) and returns the consumer's calls."""
    import torch
    m = T.pkg()
    L = m.lib()
    dev = _dev()
    body = ctx.body_bytes
    want = ref.records_of(first, first + nl)
    n_leaf = int(ref.n_blocks[first:first + nl].sum())
    n_par = int(ref.parent_first[first + nl] - ref.parent_first[first])
    rows = n_leaf + n_par
    assert want.shape[0] == rows
    h = ctypes.c_void_p()
    assert L.b3w_chain_create(ctx.handle, data.size, first, nl, batch_steps, ring, 1, ctypes.byref(h)) == 0, ctx.last_error()
    try:
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        assert L.b3w_chain_info(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), None, None) == 0
        assert (a.value, b.value, c.value) == (n_leaf, n_par, ref.n_chunks)
        calls, clones, errors, slots = [], [], [], set()

        def consumer(user, d_bodies, pitch, first_step, count, stream):
            try:
                calls.append((first_step, count, d_bodies))
                assert pitch == body
                take = [first_step, first_step + count - 1] if count < batch_steps else []       # both ends of every short batch
                take += [r for r in (n_leaf - 1, n_leaf) if first_step <= r < first_step + count]   # either side of the leaf / parent border
                if d_bodies not in slots:                                                         # the first batch of every ring slot
                    slots.add(d_bodies)
                    take.append(first_step)
                view = m.chain._view(d_bodies, (count, body), "|u1", dev)
                for r in sorted(set(take)):
                    clones.append((r, d_bodies, view[r - first_step].clone()))
            except Exception as e:                            # (an exception cannot leave a ctypes callback)
                errors.append(repr(e))
        cb = m.chain._CONSUMER(consumer)
        assert L.b3w_chain_run_leaves(h, data.ctypes.data, cb, None, None) == 0, ctx.last_error()
        d_all = torch.from_numpy(all_cvs.view(np.int32).copy()).to(dev) if all_cvs is not None else None
        assert L.b3w_chain_run_parents(h, d_all.data_ptr() if d_all is not None else None, cb, None, None) == 0, ctx.last_error()
        pub, st, root = np.zeros((rows, 15), np.uint32), np.full(rows, -1, np.int32), np.zeros(8, np.uint32)
        assert L.b3w_chain_outputs(h, pub.ctypes.data, st.ctypes.data, root.ctypes.data, None) == 0
        recs = _host(m.chain._view(L.b3w_chain_records(h), (rows, 32), "<i4", dev))
        cvs = _host(m.chain._view(L.b3w_chain_local_cvs(h), (nl, 8), "<i4", dev))
        bodies = [(r, p, t.cpu().numpy()) for r, p, t in clones]
    finally:
        L.b3w_chain_destroy(h)
    assert not errors, errors
    _same(recs[:n_leaf], want[:n_leaf], "leaf records")
    _same(recs[n_leaf:], want[n_leaf:], "parent records")
    assert (st == 0).all(), np.nonzero(st)[0][:8]
    _same(root, ref.root, "root")
    _same(cvs, ref.cvs[first:first + nl], "local chunk CVs")
    _same(pub, RM._nova_public_np(want), "public outputs")
    # the last parent step of every path leaves the restatement's final running value, at depth 0
    cs = np.arange(first, first + nl)
    cs = cs[ref.plen[cs] > 0]
    last = n_leaf + ref.parent_first[cs + 1] - ref.parent_first[first] - 1
    _same(pub[last, 2:10], ref.final[cs], "h_out of the last parent steps")
    assert (pub[last, 11] == 0).all()
    # the consumer's batches: [0, rows) in order, cut at every slice end and at the leaf / parent border, never longer than batch_steps
    slice_chunks = min(8192, max(1024, nl // 8))
    borders = [int(ref.n_blocks[first:first + s].sum()) for s in range(slice_chunks, nl, slice_chunks)] + [n_leaf, rows]
    at = 0
    for f, k, _ in calls:
        assert f == at and 1 <= k <= batch_steps, (f, k, at)
        assert not any(f < e < f + k for e in borders), (f, k)
        at += k
    assert at == rows
    expect, lo = [], 0
    for e in borders:
        expect += [(s, min(batch_steps, e - s)) for s in range(lo, e, batch_steps)]
        lo = e
    assert [(f, k) for f, k, _ in calls] == expect
    # the ring: batch i lies in slot i mod ring
    ptrs = [p for _, _, p in calls]
    assert len(set(ptrs[:ring])) == min(ring, len(ptrs)) and all(ptrs[i] == ptrs[i - ring] for i in range(ring, len(ptrs)))
    # bodies cloned inside the consumer, byte for byte
    assert 0 < len(bodies) <= 64 and len({p for _, p, _ in bodies}) == min(ring, len(ptrs))
    bad, wantb = T.oracle_batch_u32("nova_vesta", want[[r for r, _, _ in bodies]])
    assert bad == 0
    for i, (r, _, got) in enumerate(bodies):
        assert np.array_equal(got, wantb[i]), f"body of step {r}"
    return calls


def test_driver_two_slices_the_second_a_single_step(ctx):
    """1 025 chunks, last chunk 5 bytes: slices of 1 024 + 1 chunks, the second one step in a batch of its own; the path kernel"""
    data, ref = _case(1025, 5)
    calls = _drive(ctx, data, ref, 0, 1025, 1000, 2)
    assert (16384, 1) in [(f, k) for f, k, _ in calls] and (16000, 384) in [(f, k) for f, k, _ in calls]


@pytest.mark.parametrize("n_chunks", [255, 256, 257])
def test_driver_fused_plan_around_its_threshold(ctx, n_chunks):
    """at most 256 chunks: the tree kernel plans the paths itself (255: an 8-segment tree; 256: complete); 257: the path kernel"""
    data, ref = _case(n_chunks, 100)
    _drive(ctx, data, ref, 0, n_chunks, 1024, 3)


def test_driver_nine_ragged_slices(ctx):
    """8 201 chunks, last chunk 129 bytes: slices of 1 025 chunks (no multiple of 1 024), the ninth of one chunk; the copy events go
    round three times"""
    data, ref = _case(8201, 129)
    calls = _drive(ctx, data, ref, 0, 8201, 4096, 2)
    assert [(f, k) for f, k, _ in calls if f >= 8 * 16400][:2] == [(8 * 16400, 3), (8 * 16400 + 3, 4096)]


@pytest.mark.parametrize("n_chunks,last_bytes,nranks", [(300, 100, 3), (300, 100, 7), (1025, 5, 2)], ids=["300over3", "300over7", "1025over2"])
def test_driver_shards_in_one_process(ctx, n_chunks, last_bytes, nranks):
    """every rank's share of a b3w_chain_shard split, one after the other, the other ranks' chunk CVs uploaded from the restatement:
    300 chunks (segments 256 | 32 | 8 | 4) through the fused plan with first_chunk > 0, 1 025 chunks through the path kernel"""
    L = T.pkg().lib()
    data, ref = _case(n_chunks, last_bytes)
    at = 0
    for r in range(nranks):
        first, nl = ctypes.c_uint64(), ctypes.c_uint32()
        L.b3w_chain_shard(n_chunks, r, nranks, ctypes.byref(first), ctypes.byref(nl))
        assert first.value == at and nl.value in (n_chunks // nranks, n_chunks // nranks + 1)
        _drive(ctx, data, ref, first.value, nl.value, 512, 2, all_cvs=ref.cvs)
        at += nl.value
    assert at == n_chunks
