"""Bao slices on the device (bao.slices_batch / plan_samples_slices / prove_samples_slices, b3w_bao_slice_batch_device /
b3w_sample_plan_slices_device): every extracted slice is byte for byte the restatement's (tests/bao_ref.py::slice_chunk), from
full outboards and from group outboards alike (tests/bao_groups_ref.py::slice_from_group), and the records planned from slices
alone are word for word those the existing planner writes from the full outboards.  Tampering in a slice gives the status and the
records the existing planner gives for the same byte tampered in the outboard, the chunk's bytes or the root, stays with its
sample, and the host decoder (b3w_bao_slice_decode) agrees on every status."""
import gzip
import json
import os

import numpy as np
import pytest

import b3w_testlib as T
import bao_groups_ref as GR
import bao_ref as R
from test_gpu_bao_batch import _arena, _file
from test_gpu_bao_groups import _plan_shapes, _sample_chunks

pytestmark = pytest.mark.gpu

K = 1024
_WORLD = {}


def _world():
    """the arena of test_gpu_bao_groups' planning test (every shape of its outboard test plus files of exactly one group for g = 1, 4,
    6), and the restatement's full outboard of every file"""
    if not _WORLD:
        arena, offsets, lens = _plan_shapes()
        obs, cache = [], {}
        for f in range(len(lens)):
            data = _file(arena, offsets, lens, f)
            if data not in cache:
                cache[data] = R.outboard(data)[0]
            obs.append(cache[data])
        _WORLD.update(arena=arena, offsets=offsets, lens=lens, obs=obs)
    return _WORLD["arena"], _WORLD["offsets"], _WORLD["lens"], _WORLD["obs"]


def _want_slice(w, f, c):
    arena, offsets, lens, obs = w
    return R.slice_chunk(obs[f], _file(arena, offsets, lens, f), c)


def _listed_samples(m, lens, g, rng, dups=7):
    """chunk 0, the last chunk, both sides of the top three splits (and the chunks around the last group) of every file, a few drawn
    ones, some of them twice, shuffled"""
    files, chunks = [], []
    for f, ln in enumerate(lens):
        for c in _sample_chunks(m.bao.num_chunks(ln), g, rng):
            files.append(f)
            chunks.append(c)
    for k in rng.integers(0, len(files), dups):
        files.append(files[k])
        chunks.append(chunks[k])
    perm = rng.permutation(len(files))
    return np.array(files, dtype=np.uint32)[perm], np.array(chunks, dtype=np.uint64)[perm]


def _slices_of(m, out, lens, files, chunks):
    """-> the list of the samples' slices (bytes) of a slices_batch result"""
    host = out["slices"].cpu().numpy()
    sf = out["slice_first"]
    return [host[int(sf[s]):int(sf[s]) + m.bao.slice_size(int(lens[files[s]]), int(chunks[s]))].tobytes() for s in range(len(files))]


def test_extraction_from_full_outboards():
    import torch
    m = T.pkg()
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    w = _world()
    arena, offsets, lens, _ = w
    ln = np.array(lens, dtype=np.uint64)
    d_arena = torch.from_numpy(arena).cuda()
    full = m.bao.outboard_batch(ctx, d_arena, offsets, lens)
    rng = np.random.default_rng(41)
    files, chunks = _listed_samples(m, lens, 0, rng)
    n_of = np.array([m.bao.num_chunks(x) for x in lens])
    assert all(((files == f) & (chunks == 0)).any() and ((files == f) & (chunks == n_of[f] - 1)).any() for f in range(len(lens)))
    assert any(lens[f] == 0 for f in files) and len(set(zip(files.tolist(), chunks.tolist()))) < files.size            # the empty file; duplicates
    cb = m.bao.chunk_bytes_batch(arena, offsets, lens, files, chunks)
    sf = m.bao.slice_layout(ln, files, chunks)
    total, guard = int(sf[-1]), 4096
    d_slices = torch.full((total + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    s0 = torch.cuda.current_stream().cuda_stream
    # no samples: nothing is written
    assert L.b3w_bao_slice_batch_device(ctx.handle, ln.ctypes.data, ln.size, 0, full["outboards"].data_ptr(), None, None, 0, None, d_slices.data_ptr(), s0) == 0
    torch.cuda.synchronize()
    assert bool((d_slices == 0xA5).all().item())
    assert L.b3w_bao_slice_batch_device(ctx.handle, ln.ctypes.data, ln.size, 0, full["outboards"].data_ptr(), files.ctypes.data, chunks.ctypes.data, files.size,
                                        cb.data_ptr(), d_slices.data_ptr(), s0) == 0, ctx.last_error()
    torch.cuda.synchronize()
    host = d_slices.cpu().numpy()
    assert (host[total:] == 0xA5).all(), "the call wrote behind the slices"
    at = 0
    for s in range(files.size):                                   # every slice byte for byte the restatement's, the padding untouched
        a = int(sf[s])
        want = _want_slice(w, int(files[s]), int(chunks[s]))
        assert a % 8 == 0 and (host[at:a] == 0xA5).all(), s
        assert host[a:a + len(want)].tobytes() == want, (s, int(files[s]), int(chunks[s]))
        at = a + len(want)
    assert (host[at:total] == 0xA5).all()
    out = m.bao.slices_batch(ctx, full["outboards"], lens, files, chunks, cb)
    assert list(out["slice_first"]) == list(sf)
    assert _slices_of(m, out, lens, files, chunks) == [_want_slice(w, int(f), int(c)) for f, c in zip(files, chunks)]
    none = m.bao.slices_batch(ctx, full["outboards"], lens, [], [], cb[:0])
    assert none["slices"].numel() == int(none["slice_first"][-1]) and none["slice_first"].size == 1
    ctx.close()


@pytest.mark.parametrize("g", [1, 4, 6])
def test_extraction_from_group_outboards_forty_calls(g):
    """40 calls on freshly drawn samples, every byte of every call: a missing LDS wait showed as a wrong CV in some calls only"""
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    w = _world()
    arena, offsets, lens, _ = w
    d_arena = torch.from_numpy(arena).cuda()
    full = m.bao.outboard_batch(ctx, d_arena, offsets, lens)
    grp = m.bao.outboard_groups_batch(ctx, d_arena, offsets, lens, g)
    grp_host = grp["outboards"].cpu().numpy()
    ob_g = [grp_host[int(grp["ob_first"][f]):int(grp["ob_first"][f + 1])].tobytes() for f in range(len(lens))]
    rng = np.random.default_rng(500 + g)
    n_of = np.array([m.bao.num_chunks(x) for x in lens])
    compared = 0
    for call in range(40):
        if call == 0:
            files, chunks = _listed_samples(m, lens, g, rng)
            assert any(n_of[f] == (1 << g) for f in files) and any(lens[f] == 0 for f in files)
            assert any(n_of[f] % (1 << g) and c >= n_of[f] // (1 << g) * (1 << g) for f, c in zip(files, chunks))       # a short last group
        else:
            files = rng.integers(0, len(lens), 48).astype(np.uint32)
            chunks = np.array([rng.integers(0, n_of[f]) for f in files], dtype=np.uint64)
        cb = m.bao.chunk_bytes_batch(d_arena, offsets, lens, files, chunks)
        gb = m.bao.group_bytes_batch(d_arena, offsets, lens, files, chunks, g)
        got = m.bao.slices_batch(ctx, grp["outboards"], lens, files, chunks, gb, group_log=g)
        ref = m.bao.slices_batch(ctx, full["outboards"], lens, files, chunks, cb)
        assert list(got["slice_first"]) == list(ref["slice_first"])
        assert torch.equal(got["slices"], ref["slices"]), f"g = {g}, call {call}: the slices from the group outboards differ from those from the full outboards"
        mine = _slices_of(m, got, lens, files, chunks)
        gb_host = gb.cpu().numpy()
        for s in range(files.size):
            f, c = int(files[s]), int(chunks[s])
            assert mine[s] == GR.slice_from_group(ob_g[f], gb_host[s].tobytes(), c, g), (g, call, s, f, c)
            assert mine[s] == _want_slice(w, f, c), (g, call, s, f, c)
            compared += len(mine[s])
    print(f"g = {g}: 40 calls, {compared} slice bytes compared")
    ctx.close()


@pytest.mark.parametrize("lanes,chain", [(None, None), ("4", None), ("1", "1"), ("16", "1")])
def test_planned_records_equal_the_existing_planner(lanes, chain, monkeypatch):
    """the default route, and the measurement switches' routes (B3W_SLICE_PLAN_LANES, B3W_SLICE_PLAN_CHAIN): the same words"""
    import torch
    m = T.pkg()
    if lanes is not None:
        monkeypatch.setenv("B3W_SLICE_PLAN_LANES", lanes)
    if chain is not None:
        monkeypatch.setenv("B3W_SLICE_PLAN_CHAIN", chain)
    ctx = m.Context("nova_bn254", 0)
    arena, offsets, lens, _ = _world()
    d_arena = torch.from_numpy(arena).cuda()
    full = m.bao.outboard_batch(ctx, d_arena, offsets, lens)
    rng = np.random.default_rng(77)
    files, chunks = _listed_samples(m, lens, 4, rng)
    cb = m.bao.chunk_bytes_batch(arena, offsets, lens, files, chunks)
    sl = m.bao.slices_batch(ctx, full["outboards"], lens, files, chunks, cb)
    want = m.bao.plan_samples_batch(ctx, full["outboards"], lens, full["roots"], files, chunks, cb)
    got = m.bao.plan_samples_slices(ctx, lens, full["roots"], files, chunks, sl["slices"])
    assert (want["sample_status"] == 0).all()
    bad = np.nonzero(got["sample_status"])[0]
    assert bad.size == 0, [(int(files[s]), int(chunks[s]), int(got["sample_status"][s])) for s in bad[:10]]
    assert list(got["row_first"]) == list(want["row_first"]) and got["records"].shape == want["records"].shape
    assert list(got["provable"]) == list(want["provable"]) and got["provable"].any() and not got["provable"].all()
    if not torch.equal(got["records"], want["records"]):
        rf = want["row_first"]
        diff = [(int(files[s]), int(chunks[s])) for s in range(files.size)
                if not torch.equal(got["records"][int(rf[s]):int(rf[s + 1])], want["records"][int(rf[s]):int(rf[s + 1])])]
        raise AssertionError(f"the records of {len(diff)} of {files.size} samples differ, first (file, chunk): {diff[:10]}")
    print(f"{files.size} samples of {len(lens)} files, {got['records'].shape[0]} rows compared word for word")
    # from the slices of the group outboards too (they are the same bytes)
    grp = m.bao.outboard_groups_batch(ctx, d_arena, offsets, lens, 4)
    sl4 = m.bao.slices_batch(ctx, grp["outboards"], lens, files, chunks, m.bao.group_bytes_batch(d_arena, offsets, lens, files, chunks, 4), group_log=4)
    got4 = m.bao.plan_samples_slices(ctx, lens, grp["roots"], files, chunks, sl4["slices"])
    assert torch.equal(got4["records"], want["records"]) and (got4["sample_status"] == 0).all()
    comp = m.Context("compression", 0)
    with pytest.raises(m.B3WError):
        m.bao.plan_samples_slices(comp, lens, full["roots"], files, chunks, sl["slices"])
    comp.close()
    ctx.close()


def test_reference_transcript_from_slices():
    """the incomplete-trees golden (the reference WASM driven along every path of 2 ... 100-chunk trees) replayed through the slice
    planner: the last leaf block and every parent step, record for record; all trees one batch"""
    import torch
    m = T.pkg()
    W = T.workloads()
    ctx = m.Context("nova_vesta", 0)
    doc = json.load(gzip.open(os.path.join(T.GOLD, "incomplete_trees.nova_vesta.json.gz"), "rt"))
    lens = [tree["n_chunks"] * 1024 for tree in doc["trees"]]
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    arena = np.concatenate([np.frombuffer(W.lcg_preimage(ln, seed=1).tobytes(), dtype=np.uint8) for ln in lens])
    out = m.bao.outboard_batch(ctx, torch.from_numpy(arena).cuda(), offsets, lens)
    roots = out["roots"].cpu().numpy().view(np.uint32)
    files = np.array([f for f, tree in enumerate(doc["trees"]) for _ in tree["leaves"]], dtype=np.uint32)
    chunks = np.array([leaf["leaf"] for tree in doc["trees"] for leaf in tree["leaves"]], dtype=np.uint64)
    sl = m.bao.slices_batch(ctx, out["outboards"], lens, files, chunks, m.bao.chunk_bytes_batch(arena, offsets, lens, files, chunks))
    plan = m.bao.plan_samples_slices(ctx, lens, out["roots"], files, chunks, sl["slices"])          # the planner sees the slices and the roots, no more
    assert (plan["sample_status"] == 0).all()
    recs = plan["records"].cpu().numpy().view(np.uint32)
    rf = plan["row_first"]
    s = 0
    for f, tree in enumerate(doc["trees"]):
        assert list(roots[f]) == tree["root"]
        for leaf in tree["leaves"]:
            steps = leaf["steps"]
            assert int(rf[s + 1] - rf[s]) == 16 + leaf["path_len"] and len(steps) == 1 + leaf["path_len"]
            assert bool(plan["provable"][s]) == leaf["ends_in_root"]
            for k, stp in enumerate(steps):
                assert list(recs[int(rf[s]) + 15 + k]) == stp["record"], (tree["n_chunks"], leaf["leaf"], k)
            s += 1
    assert s == files.size
    ctx.close()


def test_tampered_slices_equal_the_tampered_outboard():
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    lens = [88 * K + 500, 48 * K, 33 * K + 1, 16 * K + 9, 700, 0, 5 * K]
    n = [m.bao.num_chunks(x) for x in lens]
    arena, offsets = _arena(lens, starts_odd=(1,), seed=9)
    ob = m.bao.outboard_batch(ctx, torch.from_numpy(arena).cuda(), offsets, lens)
    #                  0  1   2   3   4   5  6         7   8   9   10 11  12 13 14 15
    files = np.array([0, 1,  2,  0,  1,  2, 0,        1,  2,  1,  3, 3,  4, 5, 6, 6], dtype=np.uint32)
    chunks = np.array([0, 17, 32, 49, 47, 0, n[0] - 1, 16, 33, 15, 0, 16, 0, 0, 4, 2], dtype=np.uint64)
    N = files.size
    cb = m.bao.chunk_bytes_batch(arena, offsets, lens, files, chunks)
    obs, roots = ob["outboards"], ob["roots"]
    good = m.bao.slices_batch(ctx, obs, lens, files, chunks, cb)
    sf = good["slice_first"]
    rf = m.bao.sample_rows_batch(lens, files, chunks)
    P = [len(R.path_nodes(int(chunks[s]), n[files[s]])) for s in range(N)]
    nbytes = [R.chunk_range(lens[files[s]], int(chunks[s])) for s in range(N)]
    nbytes = [b - a for a, b in nbytes]
    size = [8 + 64 * P[s] + nbytes[s] for s in range(N)]
    host_roots = roots.cpu().numpy().view(np.uint32)

    def from_slices(slices_t=good["slices"], roots_t=roots):
        out = m.bao.plan_samples_slices(ctx, lens, roots_t, files, chunks, slices_t)
        return list(out["sample_status"]), out["records"]

    def from_outboards(obs_t=obs, cb_t=cb, roots_t=roots):
        out = m.bao.plan_samples_batch(ctx, obs_t, lens, roots_t, files, chunks, cb_t)
        return list(out["sample_status"]), out["records"]

    def rows(recs, s):
        return recs[int(rf[s]):int(rf[s + 1])]

    def host_status(slices_t, s, roots_np=host_roots):
        a = int(sf[s])
        sl = slices_t[a:a + size[s]].cpu().numpy().tobytes()
        return m.bao.decode_slice(sl, lens[files[s]], int(chunks[s]), roots_np[files[s]])[0]
    st0, recs0 = from_slices()
    stw, recsw = from_outboards()
    assert st0 == [0] * N == stw and torch.equal(recs0, recsw)
    assert [host_status(good["slices"], s) for s in range(N)] == [0] * N
    checked = 0

    def check(s, slices_t, want_status, obs_t=obs, cb_t=cb):
        """sample s's slice is tampered: its status and records are the existing planner's on the tampered outboard / bytes, every other
        sample is verified with unchanged records, and the host decoder says the same"""
        st, recs = from_slices(slices_t)
        stw, recsw = from_outboards(obs_t, cb_t)
        assert stw[s] == want_status and st[s] == want_status, (s, st[s], stw[s], want_status)
        assert torch.equal(rows(recs, s), rows(recsw, s)), s
        for o in range(N):
            if o != s:
                assert st[o] == 0 and torch.equal(rows(recs, o), rows(recs0, o)), (s, o)
        assert host_status(slices_t, s) == want_status, s
    for s in range(N):
        f, c, a = int(files[s]), int(chunks[s]), int(sf[s])
        path = R.path_nodes(c, n[f])
        ob_at = int(ob["ob_first"][f])
        if nbytes[s]:                                             # a byte of the chunk
            k = (s * 131) % nbytes[s]
            bad, bad_cb = good["slices"].clone(), cb.clone()
            bad[a + 8 + 64 * P[s] + k] ^= 1
            bad_cb[s, k] ^= 1
            check(s, bad, 1, cb_t=bad_cb)
            checked += 1
        for j in range(P[s]):                                     # every node, either half
            for half in (0, 1):
                x = 32 * half + (s + 7 * j) % 32
                bad, bad_ob = good["slices"].clone(), obs.clone()
                bad[a + 8 + 64 * j + x] ^= 1
                bad_ob[ob_at + 8 + 64 * path[j] + x] ^= 1
                check(s, bad, 2, obs_t=bad_ob)
                checked += 1
        bad, bad_ob = good["slices"].clone(), obs.clone()          # the header
        bad[a + s % 8] ^= 1
        bad_ob[ob_at + s % 8] ^= 1
        check(s, bad, 3, obs_t=bad_ob)
        checked += 1
    assert checked >= 140
    # the root on the device: the file's samples, no other; the same from both planners, and from the host decoder
    for f in range(len(lens)):
        wrong = roots.clone()
        wrong[f, f % 8] ^= 1
        st, recs = from_slices(roots_t=wrong)
        stw, recsw = from_outboards(roots_t=wrong)
        assert st == stw and st == [(2 if P[s] else 1) if files[s] == f else 0 for s in range(N)]
        assert torch.equal(recs, recsw) and torch.equal(recs, recs0)                              # (the records do not depend on the root)
        wrong_np = wrong.cpu().numpy().view(np.uint32)
        assert [host_status(good["slices"], s, wrong_np) for s in range(N)] == st
    # all at once, one kind a sample: every sample its own verdict
    bad, bad_ob, bad_cb = good["slices"].clone(), obs.clone(), cb.clone()
    bad[int(sf[3]) + 8 + 64 * P[3] + 9] ^= 1
    bad_cb[3, 9] ^= 1
    bad[int(sf[14]) + 8 + 3] ^= 1                                 # (chunk 4 of 5 hangs off the root: its one node)
    bad[int(sf[10])] ^= 1
    st, recs = from_slices(bad)
    assert st == [1 if s == 3 else 2 if s == 14 else 3 if s == 10 else 0 for s in range(N)]
    assert [host_status(bad, s) for s in range(N)] == st
    # what only slices allow: the valid slice of ANOTHER chunk of the same file, of the same path length and byte count, in a sample's place
    swaps = 0
    for s, other in ((1, 18), (5, 1), (7, 31), (9, 14), (15, 3), (0, 1)):
        f = int(files[s])
        assert other != int(chunks[s]) and len(R.path_nodes(other, n[f])) == P[s]
        extra = m.bao.slices_batch(ctx, obs, lens, [f], [other], m.bao.chunk_bytes_batch(arena, offsets, lens, [f], [other]))
        assert m.bao.slice_size(lens[f], other) == size[s]
        e0 = int(extra["slice_first"][0])
        assert m.bao.decode_slice(extra["slices"][e0:e0 + size[s]].cpu().numpy().tobytes(), lens[f], other, host_roots[f])[0] == 0
        bad = good["slices"].clone()
        bad[int(sf[s]):int(sf[s]) + size[s]] = extra["slices"][e0:e0 + size[s]]
        st, recs = from_slices(bad)
        want = host_status(bad, s)
        assert want != 0 and st == [want if o == s else 0 for o in range(N)], (s, other, want, st)
        for o in range(N):
            if o != s:
                assert torch.equal(rows(recs, o), rows(recs0, o)), (s, o)
        swaps += 1
    assert swaps == 6
    ctx.close()


def test_prove_samples_slices_equals_prove_samples_batch():
    import torch
    import ec_ref as E
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    lens = [43 * 1024 + 33, 16 * 1024, 700, 32 * 1024]
    arena, offsets = _arena(lens, seed=2)
    d_arena = torch.from_numpy(arena).cuda()
    full = m.bao.outboard_batch(ctx, d_arena, offsets, lens)
    files = np.array([0, 1, 0, 2, 1, 0, 3, 3], dtype=np.uint32)
    chunks = np.array([3, 4, 43, 0, 15, 32, 16, 0], dtype=np.uint64)
    cb = m.bao.chunk_bytes_batch(arena, offsets, lens, files, chunks)
    sl = m.bao.slices_batch(ctx, full["outboards"], lens, files, chunks, cb)["slices"]
    roots = full["roots"].cpu().numpy().view(np.uint32)
    key = m.CommitKey(ctx, "pallas", E.points_to_bytes(E.random_points("pallas", ctx.witness_size)), window=12)
    r1cs = m.R1cs(ctx)
    want = m.bao.prove_samples_batch(ctx, full["outboards"], lens, full["roots"], files, chunks, cb, batch_steps=16, commit_key=key)
    got = m.bao.prove_samples_slices(ctx, lens, full["roots"], files, chunks, sl, batch_steps=16, commit_key=key)
    want2 = m.bao.prove_samples_batch(ctx, full["outboards"], lens, full["roots"], files, chunks, cb, batch_steps=7, r1cs=r1cs)
    got2 = m.bao.prove_samples_slices(ctx, lens, full["roots"], files, chunks, sl, batch_steps=7, r1cs=r1cs)
    assert (got["sample_status"] == 0).all() and (got2["sample_status"] == 0).all()
    for a, b in ((got, want), (got2, want2)):
        assert torch.equal(a["records"], b["records"]) and list(a["row_first"]) == list(b["row_first"])
        assert torch.equal(a["public"], b["public"]) and torch.equal(a["status"], b["status"]) and (a["status"] == 0).all().item()
    assert torch.equal(got["points"], want["points"]) and got2["points"] is None
    assert torch.equal(got2["violations"], want2["violations"]) and (got2["violations"] == 0).all().item()
    pub = got2["public"].cpu().numpy().view(np.uint32)
    rf = got["row_first"]
    assert got["provable"].any()
    for s in range(files.size):
        if got["provable"][s]:
            assert list(pub[int(rf[s + 1]) - 1][2:10]) == list(roots[files[s]]), s
    key.close()
    r1cs.close()
    ctx.close()


def test_refusals_before_anything_is_written():
    import torch
    m = T.pkg()
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    lens = [5 * K, 1, 40 * K]
    arena, offsets = _arena(lens, seed=4)
    ln = np.array(lens, dtype=np.uint64)
    full = m.bao.outboard_batch(ctx, torch.from_numpy(arena).cuda(), offsets, lens)
    files, chunks = np.array([0, 2], dtype=np.uint32), np.array([4, 39], dtype=np.uint64)
    cb = m.bao.chunk_bytes_batch(arena, offsets, lens, files, chunks)
    d_slices = torch.full((8192,), 0xA5, dtype=torch.uint8, device="cuda")
    d_recs = torch.full((64, 32), -7, dtype=torch.int32, device="cuda")
    d_st = torch.full((2,), -1, dtype=torch.int32, device="cuda")

    def extract(g, fi, ch):
        fi, ch = np.array(fi, dtype=np.uint32), np.array(ch, dtype=np.uint64)
        return L.b3w_bao_slice_batch_device(ctx.handle, ln.ctypes.data, ln.size, g, full["outboards"].data_ptr(), fi.ctypes.data, ch.ctypes.data, fi.size,
                                            cb.data_ptr(), d_slices.data_ptr(), 0)

    def plan(fi, ch):
        fi, ch = np.array(fi, dtype=np.uint32), np.array(ch, dtype=np.uint64)
        return L.b3w_sample_plan_slices_device(ctx.handle, ln.ctypes.data, ln.size, full["roots"].data_ptr(), fi.ctypes.data, ch.ctypes.data, fi.size,
                                               d_slices.data_ptr(), d_recs.data_ptr(), d_st.data_ptr(), 0)
    assert extract(7, files, chunks) == m.B3W_E_BAD_ARGUMENT and "group_log" in ctx.last_error()
    assert extract(0, [0, 3], [4, 0]) == m.B3W_E_BAD_ARGUMENT and "file index" in ctx.last_error()
    assert extract(0, [0, 1], [5, 0]) == m.B3W_E_BAD_ARGUMENT and "chunk index" in ctx.last_error()
    assert extract(4, [0, 1], [0, 1]) == m.B3W_E_BAD_ARGUMENT
    assert plan([0, 3], [4, 0]) == m.B3W_E_BAD_ARGUMENT and "file index" in ctx.last_error()
    assert plan([0, 2], [4, 40]) == m.B3W_E_BAD_ARGUMENT and "chunk index" in ctx.last_error()
    assert L.b3w_bao_slice_batch_device(ctx.handle, ln.ctypes.data, ln.size, 0, full["outboards"].data_ptr(), files.ctypes.data, chunks.ctypes.data, 2,
                                        cb.data_ptr(), d_slices.data_ptr() + 8, 0) == m.B3W_E_BAD_ARGUMENT and "aligned" in ctx.last_error()
    torch.cuda.synchronize()
    assert bool((d_slices == 0xA5).all().item()) and bool((d_recs == -7).all().item()) and bool((d_st == -1).all().item())
    with pytest.raises(m.B3WError):
        m.bao.slices_batch(ctx, full["outboards"], lens, files, chunks, cb, group_log=7)
    with pytest.raises(m.B3WError):
        m.bao.slices_batch(ctx, full["outboards"], lens, [3], [0], cb)
    with pytest.raises(m.B3WError):
        m.bao.plan_samples_slices(ctx, lens, full["roots"], [1], [1], d_slices)
    assert extract(0, files, chunks) == 0 and plan(files, chunks) == 0          # and the same arguments, valid, go through
    torch.cuda.synchronize()
    assert d_st.tolist() == [0, 0]
    ctx.close()
