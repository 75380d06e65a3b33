"""Bao outboards on the device and challenged chunk paths planned from an outboard (bao.py, b3w_bao_* / b3w_sample_*): the outboard
is byte-equal to the plain-Python restatement (tests/bao_ref.py), the sampled paths' records are the chain planner's rows for those
chunks word for word — the reference-made incomplete-tree transcript included — and every tampered input is caught."""
import gzip
import json
import os
import struct

import numpy as np
import pytest

import b3w_testlib as T
import bao_ref as R
import blake3_ref as B

pytestmark = pytest.mark.gpu


def _dev(data):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def _data(length, seed=11):
    return np.random.default_rng(seed + length).integers(0, 256, length, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("length", [0, 1, 1023, 1024, 1025, 3 * 1024 + 5, 37 * 1024, 1 << 20, 100 * 1024 + 77])
def test_device_outboard_equals_the_restatement(length):
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    data = _data(length)
    ob, root = m.bao.outboard(ctx, _dev(data) if length else data)
    want_ob, want_root = R.outboard(data)
    assert list(root) == want_root == B.hash_words(data)
    assert ob.cpu().numpy().tobytes() == want_ob
    ctx.close()


@pytest.mark.parametrize("quad", ["0", "1"])
def test_device_outboard_small_shapes_both_kernels(quad, monkeypatch):
    """the lane-per-chunk and the four-lanes-per-chunk chunk-CV kernels give the same outboard (B3W_BAO_QUAD switches)"""
    monkeypatch.setenv("B3W_BAO_QUAD", quad)
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    for length in [1, 1024, 5 * 1024 + 1, 64 * 1024, 65 * 1024 + 9]:
        data = _data(length, 3)
        ob, root = m.bao.outboard(ctx, _dev(data))
        want_ob, want_root = R.outboard(data)
        assert list(root) == want_root and ob.cpu().numpy().tobytes() == want_ob, length
    ctx.close()


def test_device_outboard_256_mib():
    """a complete tree of 256 Ki chunks: the pre-order outboard against numpy levels, the root against BLAKE3"""
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    rng = np.random.default_rng(256)
    data = rng.integers(0, 256, 256 << 20, dtype=np.uint8)
    ob, root = m.bao.outboard(ctx, _dev(data))
    cvs = B.chunk_cvs_np(data)
    levels = B.tree_levels_np(cvs)
    assert list(root) == [int(x) for x in levels[-1][0]]
    n = cvs.shape[0]
    got = ob.cpu().numpy()
    assert got.size == 8 + 64 * (n - 1) and struct.unpack("<Q", got[:8].tobytes())[0] == data.size
    nodes = got[8:].view("<u4").reshape(n - 1, 16)
    # pre-order of a complete tree: the node at level t, index i sits at (i << t) - popcount(i) + (levels - 1 - t) ... restated by
    # walking: node of chunks [a, a + 2^t) at depth d = L - t with r right turns = popcount(a >> t) has position d + a - r
    Lv = len(levels) - 1
    for t in range(1, Lv + 1):
        i = np.arange(levels[t].shape[0], dtype=np.int64)
        a = i << t
        pos = (Lv - t) + a - np.array([bin(x).count("1") for x in (i.tolist())], dtype=np.int64)
        kids = levels[t - 1].reshape(-1, 16)
        assert np.array_equal(nodes[pos], kids), t
    # and the restated path of a few chunks decodes
    for c in [0, 1, n // 3, n - 1]:
        sl = m.bao.slice_chunk(got, data.size, c, data[c * 1024:(c + 1) * 1024].tobytes())
        assert R.decode_slice(sl, c, list(root)) == data[c * 1024:(c + 1) * 1024].tobytes()
    ctx.close()


def _chain_rows(m, plan, chunks, n):
    """row indices of the chain planner's records for `chunks`, in b3w_sample_rows' order"""
    rows = m.ChainPlanner(None).parent_rows(n)
    n_leaf = plan["n_leaf_steps"]
    out = []
    for c in chunks:
        c = int(c)
        nb = int(plan["last_blocks"]) if c == n - 1 else 16
        row, pl, _ = rows[c]
        out += [c * 16 + j for j in range(nb)] + [n_leaf + row + j for j in range(pl)]
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize("length", [1, 700, 2048, 64 * 1024, 3 * 1024 + 5, 37 * 1024 + 64, 100 * 1024 + 77])
def test_sampled_records_equal_the_chain_planner(length):
    import torch
    m = T.pkg()
    ctx = m.Context("nova_bn254", 0)
    data = _data(length, 5)
    d_pre = _dev(data)
    n = m.bao.num_chunks(length)
    rng = np.random.default_rng(length)
    chunks = np.concatenate([rng.integers(0, n, 12), [n - 1, 0, n - 1]]).astype(np.uint64)       # duplicates, the last chunk
    ob, root = m.bao.outboard(ctx, d_pre)
    out = m.bao.plan_samples(ctx, ob, length, root, chunks, m.bao.chunk_bytes(data, chunks))
    assert (out["sample_status"] == 0).all()
    plan = m.ChainPlanner(ctx).plan(d_pre)
    idx = _chain_rows(m, plan, chunks, n)
    want = plan["records"][torch.from_numpy(idx).cuda()]
    got = out["records"]
    assert got.shape == want.shape and torch.equal(got, want)
    # the same witnesses: public outputs and statuses of both through the batch kernel
    res = []
    for recs in (got, want):
        k = recs.shape[0]
        d_b = torch.empty((k, ctx.body_bytes), dtype=torch.uint8, device="cuda")
        d_p = torch.zeros((k, 15), dtype=torch.int32, device="cuda")
        d_s = torch.full((k,), -1, dtype=torch.int32, device="cuda")
        ctx.run_device(recs.data_ptr(), k, d_b.data_ptr(), 0, d_p.data_ptr(), d_s.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        res.append((d_p.cpu().numpy().view(np.uint32), d_s.cpu().numpy()))
    assert np.array_equal(res[0][0], res[1][0]) and (res[0][1] == 0).all() and (res[1][1] == 0).all()
    pub = res[0][0]
    rf = out["row_first"]
    for s, c in enumerate(chunks):
        last = pub[int(rf[s + 1]) - 1]
        if out["provable"][s]:
            assert list(last[2:10]) == list(root), (s, c)
    ctx.close()


def test_reference_transcript_from_the_outboard_alone():
    """the incomplete-trees golden (the reference WASM driven along every path of 2 ... 100-chunk trees): the last leaf block and
    every parent step, planned from the outboard and the one chunk's bytes"""
    m = T.pkg()
    W = T.workloads()
    ctx = m.Context("nova_vesta", 0)
    doc = json.load(gzip.open(os.path.join(T.GOLD, "incomplete_trees.nova_vesta.json.gz"), "rt"))
    for tree in doc["trees"]:
        n = tree["n_chunks"]
        data = W.lcg_preimage(n * 1024, seed=1).tobytes()
        ob, root = m.bao.outboard(ctx, _dev(data))
        assert list(root) == tree["root"]
        chunks = np.array([leaf["leaf"] for leaf in tree["leaves"]], dtype=np.uint64)
        only = m.bao.chunk_bytes(data, chunks)                              # the planner sees these bytes and the outboard, no more
        out = m.bao.plan_samples(ctx, ob, n * 1024, root, chunks, only)
        assert (out["sample_status"] == 0).all()
        recs = out["records"].cpu().numpy().view(np.uint32)
        rf = out["row_first"]
        for s, leaf in enumerate(tree["leaves"]):
            steps = leaf["steps"]
            assert int(rf[s + 1] - rf[s]) == 16 + leaf["path_len"] and len(steps) == 1 + leaf["path_len"]
            assert bool(out["provable"][s]) == leaf["ends_in_root"]
            for k, stp in enumerate(steps):
                assert list(recs[int(rf[s]) + 15 + k]) == stp["record"], (n, leaf["leaf"], k)
    ctx.close()


def test_tampering_is_caught_per_sample():
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    length = 37 * 1024 + 500
    data = _data(length, 9)
    n = m.bao.num_chunks(length)
    ob, root = m.bao.outboard(ctx, _dev(data))
    chunks = np.array([0, 5, 17, n - 1, 5], dtype=np.uint64)
    good = m.bao.chunk_bytes(data, chunks)

    def status(ob_t, cb, rt=root):
        return list(m.bao.plan_samples(ctx, ob_t, length, rt, chunks, cb)["sample_status"])
    assert status(ob, good) == [0] * 5
    cb = good.clone()
    cb[2, 100] ^= 1                                                   # a byte of sample 2's chunk
    assert status(ob, cb) == [0, 0, 1, 0, 0]
    cb = good.clone()
    cb[3, 1023] ^= 1                                                  # past the file's end: ignored
    assert status(ob, cb) == [0] * 5
    path17 = m.bao.path_nodes(17, n)
    path5 = m.bao.path_nodes(5, n)
    node = path17[-1]                                                 # the lowest node of chunk 17's path (on no other sampled path?)
    others = set(path5) | set(m.bao.path_nodes(0, n)) | set(m.bao.path_nodes(n - 1, n))
    assert node not in others
    bad = ob.clone()
    bad[8 + 64 * node + 3] ^= 1
    assert status(bad, good) == [0, 0, 2, 0, 0]
    onpath = set(path17) | others
    free = next(i for i in range(n - 1) if i not in onpath)          # a node on no sampled path
    bad = ob.clone()
    bad[8 + 64 * free + 40] ^= 1
    assert status(bad, good) == [0] * 5
    wrong = root.copy()
    wrong[4] ^= 1
    assert status(ob, good, wrong) == [2] * 5
    bad = ob.clone()
    bad[0] ^= 1                                                       # the header
    assert status(bad, good) == [3] * 5
    with pytest.raises(m.B3WError):
        m.bao.plan_samples(ctx, ob, length, root, np.array([n], dtype=np.uint64), good[:1])
    comp = m.Context("compression", 0)
    with pytest.raises(m.B3WError):
        m.bao.plan_samples(comp, ob, length, root, chunks, good)
    comp.close()
    ctx.close()


def test_bodies_commitments_and_streaming():
    import torch
    import ec_ref as E
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    length = 11 * 1024 + 33
    data = _data(length, 2)
    d_pre = _dev(data)
    n = m.bao.num_chunks(length)
    chunks = np.array([3, 10, 7, 3], dtype=np.uint64)
    ob, root = m.bao.outboard(ctx, d_pre)
    cb = m.bao.chunk_bytes(d_pre, chunks)
    seen, sampled = [], {}

    def consumer(bodies, pitch, first_row, count):
        seen.append((first_row, count))
        for r in (first_row, first_row + count - 1):
            sampled[r] = bodies[r - first_row].cpu().numpy()
    r1cs = m.R1cs(ctx)
    out = m.bao.prove_samples(ctx, ob, length, root, chunks, cb, batch_steps=7, consumer=consumer, r1cs=r1cs)
    rows = out["records"].shape[0]
    assert sorted(seen) == [(r, min(7, rows - r)) for r in range(0, rows, 7)]
    assert (out["status"] == 0).all().item() and (out["violations"] == 0).all().item()
    recs = out["records"].cpu().numpy().view(np.uint32)
    idx = sorted(sampled)
    _, want = T.oracle_batch_u32("nova_vesta", recs[idx])
    for k, r in enumerate(idx):
        assert np.array_equal(sampled[r], want[k]), r
    # commitments from the records alone equal b3w_commit_records on the chain's rows for those chunks
    key = m.CommitKey(ctx, "pallas", E.points_to_bytes(E.random_points("pallas", ctx.witness_size)), window=12)
    res = m.bao.prove_samples(ctx, ob, length, root, chunks, cb, batch_steps=16, commit_key=key)
    plan = m.ChainPlanner(ctx).plan(d_pre)
    chain_recs = plan["records"].cpu().numpy().view(np.uint32)[_chain_rows(m, plan, chunks, n)]
    pts, _, st = key.commit_records(chain_recs)
    assert (st == 0).all() and (res["status"] == 0).all().item()
    assert np.array_equal(res["points"].cpu().numpy(), pts)
    key.close()
    r1cs.close()
    ctx.close()
