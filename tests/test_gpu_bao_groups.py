"""Bao outboards over chunk groups and challenged paths planned from them (bao.outboard_groups_batch / plan_samples_groups_batch /
prove_samples_groups_batch, b3w_bao_group_outboard_batch_device / b3w_sample_plan_group_batch_device): every group outboard is the
restatement's (tests/bao_groups_ref.py) and every root BLAKE3's, at g = 0 the bytes are the existing batch call's, and the records
planned from a group outboard plus the group's bytes are word for word those the existing planner writes from the full outboard
plus the chunk's bytes.  Tampering stays with the samples it hits: status 1 for a flipped byte anywhere in the sampled chunk's
GROUP, 2 for a stored node or the root, 3 for the header."""
import gzip
import json
import os

import numpy as np
import pytest

import b3w_testlib as T
import bao_groups_ref as GR
import bao_ref as R
import blake3_ref as B
from test_gpu_bao_batch import _arena, _file

pytestmark = pytest.mark.gpu

GS = [0, 1, 4, 6]
K = 1024
BASE = [0, 1, 1023, K, 1025, 3 * K + 5, 37 * K, 100 * K + 77, 1023 * K, 1 << 20, (1 << 20) + 1, 1025 * K, 2049 * K + 3, 3 << 20]


def _shapes():
    """the arena of test_every_shape_against_the_restatement: its lengths in its order, two odd starts, one file listed twice"""
    order = np.random.default_rng(3).permutation(len(BASE))
    lens = [BASE[i] for i in order]
    arena, offsets = _arena(lens, starts_odd=(2, 9))
    dup = lens.index(100 * K + 77)
    lens.append(lens[dup])
    offsets = np.append(offsets, offsets[dup])
    return arena, offsets, lens


def _check_groups_against_restatement(out, arena, offsets, lens, files, g):
    obs = out["outboards"].cpu().numpy()
    roots = out["roots"].cpu().numpy().view(np.uint32)
    cache = {}
    for f in files:
        data = _file(arena, offsets, lens, f)
        if data not in cache:
            cache[data] = GR.group_outboard(data, g)
        want_ob, want_root = cache[data]
        a, b = int(out["ob_first"][f]), int(out["ob_first"][f + 1])
        assert b - a == GR.group_outboard_size(len(data), g)
        assert obs[a:b].tobytes() == want_ob, (g, f, lens[f])
        assert list(roots[f]) == want_root, (g, f, lens[f])


_ROOTS = {}


@pytest.mark.parametrize("g", GS)
def test_every_shape_against_the_restatement(g):
    import torch
    m = T.pkg()
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    arena, offsets, lens = _shapes()
    assert int(offsets[2]) % 2 == 1 and int(offsets[9]) % 2 == 1
    ln = np.array(lens, dtype=np.uint64)
    d_arena = torch.from_numpy(arena).cuda()
    ob_first = m.bao.group_batch_layout(ln, g)
    total = int(ob_first[-1])
    guard = 4096
    d_obs = torch.full((total + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    d_roots = torch.zeros((len(lens), 8), dtype=torch.int32, device="cuda")
    need = L.b3w_bao_batch_scratch_bytes(ln.ctypes.data, ln.size)
    d_scratch = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    # a scratch one byte short and a group_log of 7 are refused before anything is written
    assert L.b3w_bao_group_outboard_batch_device(ctx.handle, d_arena.data_ptr(), offsets.ctypes.data, ln.ctypes.data, ln.size, g, d_obs.data_ptr(),
                                                 d_roots.data_ptr(), d_scratch.data_ptr(), need - 1, 0) == m.B3W_E_BAD_ARGUMENT
    assert "scratch" in ctx.last_error()
    assert L.b3w_bao_group_outboard_batch_device(ctx.handle, d_arena.data_ptr(), offsets.ctypes.data, ln.ctypes.data, ln.size, 7, d_obs.data_ptr(),
                                                 d_roots.data_ptr(), d_scratch.data_ptr(), need, 0) == m.B3W_E_BAD_ARGUMENT
    assert "group_log" in ctx.last_error()
    torch.cuda.synchronize()
    assert bool((d_obs == 0xA5).all().item())
    assert L.b3w_bao_group_outboard_batch_device(ctx.handle, d_arena.data_ptr(), offsets.ctypes.data, ln.ctypes.data, ln.size, g, d_obs.data_ptr(),
                                                 d_roots.data_ptr(), d_scratch.data_ptr(), need, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert bool((d_obs[total:] == 0xA5).all().item()), "the group call wrote behind the outboards"
    out = dict(outboards=d_obs[:total], ob_first=ob_first, roots=d_roots)
    _check_groups_against_restatement(out, arena, offsets, lens, range(len(lens)), g)
    for f in range(len(lens)):                                     # every root is BLAKE3 of the file (hashed once for all g)
        data = _file(arena, offsets, lens, f)
        if data not in _ROOTS:
            _ROOTS[data] = B.hash_words(data)
        assert list(d_roots[f].cpu().numpy().view(np.uint32)) == _ROOTS[data], f
    again = m.bao.outboard_groups_batch(ctx, d_arena, offsets, ln, g)
    assert torch.equal(again["outboards"], d_obs[:total]) and torch.equal(again["roots"], d_roots) and list(again["ob_first"]) == list(ob_first)
    if g == 0:                                                     # the full outboards: the existing call's bytes
        full = m.bao.outboard_batch(ctx, d_arena, offsets, ln)
        assert torch.equal(full["outboards"], d_obs[:total]) and torch.equal(full["roots"], d_roots) and list(full["ob_first"]) == list(ob_first)
    none = m.bao.outboard_groups_batch(ctx, d_arena, [], [], g)
    assert none["outboards"].numel() == 0 and none["roots"].shape == (0, 8) and list(none["ob_first"]) == [0]
    ctx.close()


def test_many_small_files_at_16_kib_groups():
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    g = 4
    rng = np.random.default_rng(2048)
    rng.integers(0, 8 * 1024 + 1, 2048)                            # (the lengths of the existing 100 000-file test: its generator's second draw)
    n_files = 100000
    lens = rng.integers(0, 32 * 1024 + 1, n_files).astype(np.uint64)
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    d_arena = torch.randint(0, 256, (int(lens.sum()),), dtype=torch.uint8, device="cuda", generator=gen)
    out = m.bao.outboard_groups_batch(ctx, d_arena, offsets, lens, g)
    full = m.bao.outboard_batch(ctx, d_arena, offsets, lens)
    torch.cuda.synchronize()
    size = np.diff(out["ob_first"]).astype(np.int64)
    assert ((size == 8) == (lens <= 16 * 1024)).all() and ((size == 72) == (lens > 16 * 1024)).all()
    assert int(out["ob_first"][-1]) == 8 * n_files + 64 * int((lens > 16 * 1024).sum())
    assert torch.equal(out["roots"], full["roots"])
    first = torch.from_numpy(out["ob_first"][:-1].astype(np.int64)).cuda()
    hdr = out["outboards"][first[:, None] + torch.arange(8, device="cuda")[None, :]].cpu().numpy()
    assert np.array_equal(hdr.copy().view("<u8").reshape(-1), lens), "a header is not its file's length"
    arena = d_arena.cpu().numpy()
    pick = [int(f) for f in rng.choice(n_files, 300, replace=False)]
    _check_groups_against_restatement(out, arena, offsets, [int(x) for x in lens], pick, g)
    ctx.close()


def test_a_file_of_1026_tiles():
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    g = 4
    gen = torch.Generator(device="cuda")
    gen.manual_seed(256)
    lens = [3000, (1 << 30) + (1 << 20) + 5, 1, 70 * 1024]
    offsets = np.array([0, 3008, 3008 + lens[1] + 3, 3008 + lens[1] + 16], dtype=np.uint64)
    d_arena = torch.randint(0, 256, (int(offsets[3]) + lens[3],), dtype=torch.uint8, device="cuda", generator=gen)
    out = m.bao.outboard_groups_batch(ctx, d_arena, offsets, lens, g)
    roots = out["roots"].cpu().numpy().view(np.uint32)
    big = d_arena[3008:3008 + lens[1]].cpu().numpy()
    want_ob, want_root = GR.group_outboard_np(big, g)
    a, b = int(out["ob_first"][1]), int(out["ob_first"][2])
    assert out["outboards"][a:b].cpu().numpy().tobytes() == want_ob and list(roots[1]) == want_root
    arena = {f: d_arena[int(offsets[f]):int(offsets[f]) + lens[f]].cpu().numpy().tobytes() for f in (0, 2, 3)}
    for f, data in arena.items():
        want_ob, want_root = GR.group_outboard(data, g)
        a, b = int(out["ob_first"][f]), int(out["ob_first"][f + 1])
        assert out["outboards"][a:b].cpu().numpy().tobytes() == want_ob and list(roots[f]) == want_root, f
    ctx.close()


# ---- planning ----------------------------------------------------------------------------------------------------------
def _sample_chunks(n, g, rng):
    """the chunks to challenge of a file of n chunks: chunk 0, the last chunk, the chunks around the start of the (maybe short) last
    group, both sides of every split of the tree's top three levels, a few random ones"""
    G = 1 << g
    out = {0, n - 1, (n - 1) // G * G, max(0, (n - 1) // G * G - 1), (n - 1) // G * G + (n - 1 - (n - 1) // G * G) // 2}

    def splits(lo, m, depth):
        if m > 1 and depth:
            k = R._split(m)
            out.update((lo + k - 1, lo + k))
            splits(lo, k, depth - 1)
            splits(lo + k, m - k, depth - 1)
    splits(0, n, 3)
    out.update(int(c) for c in rng.integers(0, n, 5))
    return sorted(out)


def _plan_shapes():
    """every shape of the outboard test, and files of exactly one group for g = 1, 4, 6 and one chunk more"""
    arena, offsets, lens = _shapes()
    extra = [2 * K, 16 * K, 64 * K, 16 * K + 1, 64 * K + 1, 2 * K - 1, 16 * K - 1, 64 * K - 1]
    arena2, offsets2 = _arena(extra, starts_odd=(1, 4), seed=11)
    return np.concatenate([arena, arena2]), np.concatenate([offsets, offsets2 + np.uint64(arena.size)]), lens + extra


@pytest.mark.parametrize("g", GS)
def test_planned_records_equal_the_existing_planner(g):
    import torch
    m = T.pkg()
    ctx = m.Context("nova_bn254", 0)
    arena, offsets, lens = _plan_shapes()
    d_arena = torch.from_numpy(arena).cuda()
    full = m.bao.outboard_batch(ctx, d_arena, offsets, lens)
    grp = m.bao.outboard_groups_batch(ctx, d_arena, offsets, lens, g)
    assert torch.equal(full["roots"], grp["roots"])
    rng = np.random.default_rng(100 + g)
    files, chunks = [], []
    for f, ln in enumerate(lens):
        for c in _sample_chunks(m.bao.num_chunks(ln), g, rng):
            files.append(f)
            chunks.append(c)
    perm = rng.permutation(len(files))
    files, chunks = np.array(files, dtype=np.uint32)[perm], np.array(chunks, dtype=np.uint64)[perm]
    n_of = np.array([m.bao.num_chunks(x) for x in lens])
    # the cases that must be there
    assert all(((files == f) & (chunks == 0)).any() and ((files == f) & (chunks == n_of[f] - 1)).any() for f in range(len(lens)))
    assert any(n_of[f] == 1 and lens[f] == 0 for f in files) and any(n_of[f] == 1 and lens[f] > 0 for f in files)
    assert any(n_of[f] == (1 << g) for f in files)                                            # a file of exactly one group
    assert g == 0 or any(n_of[f] % (1 << g) and c >= n_of[f] // (1 << g) * (1 << g) for f, c in zip(files, chunks))   # a short last group
    cb = m.bao.chunk_bytes_batch(arena, offsets, lens, files, chunks)
    gb = m.bao.group_bytes_batch(arena, offsets, lens, files, chunks, g)
    assert gb.shape == (files.size, 1024 << g)
    assert torch.equal(gb, m.bao.group_bytes_batch(d_arena, offsets, lens, files, chunks, g))
    for s in range(0, files.size, 37):                                                        # the restatement's reading of "the group's bytes"
        assert gb[s].cpu().numpy().tobytes() == GR.group_bytes(_file(arena, offsets, lens, files[s]), int(chunks[s]), g), s
    want = m.bao.plan_samples_batch(ctx, full["outboards"], lens, full["roots"], files, chunks, cb)
    got = m.bao.plan_samples_groups_batch(ctx, grp["outboards"], lens, grp["roots"], files, chunks, gb, g)
    assert (want["sample_status"] == 0).all()
    bad = np.nonzero(got["sample_status"])[0]
    assert bad.size == 0, [(int(files[s]), int(chunks[s]), int(got["sample_status"][s])) for s in bad[:10]]
    assert list(got["row_first"]) == list(want["row_first"]) and got["records"].shape == want["records"].shape
    assert list(got["provable"]) == list(want["provable"])
    if not torch.equal(got["records"], want["records"]):
        rf = want["row_first"]
        diff = [(int(files[s]), int(chunks[s])) for s in range(files.size)
                if not torch.equal(got["records"][int(rf[s]):int(rf[s + 1])], want["records"][int(rf[s]):int(rf[s + 1])])]
        raise AssertionError(f"g = {g}: the records of {len(diff)} of {files.size} samples differ, first (file, chunk): {diff[:10]}")
    print(f"g = {g}: {files.size} samples of {len(lens)} files, {got['records'].shape[0]} rows compared word for word")
    # argument errors, before anything is launched
    with pytest.raises(m.B3WError):
        m.bao.plan_samples_groups_batch(ctx, grp["outboards"], lens, grp["roots"], [len(lens)], [0], gb[:1], g)
    with pytest.raises(m.B3WError):
        m.bao.plan_samples_groups_batch(ctx, grp["outboards"], lens, grp["roots"], [lens.index(1)], [1], gb[:1], g)      # chunk 1 of 1
    ln64 = np.array(lens, dtype=np.uint64)
    f1, c1 = np.array([0], dtype=np.uint32), np.array([0], dtype=np.uint64)
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    assert m.lib().b3w_sample_plan_group_batch_device(ctx.handle, ln64.ctypes.data, ln64.size, 7, grp["outboards"].data_ptr(), grp["roots"].data_ptr(),
                                                       f1.ctypes.data, c1.ctypes.data, 1, gb.data_ptr(), got["records"].data_ptr(), st.data_ptr(), 0) == m.B3W_E_BAD_ARGUMENT
    assert "group_log" in ctx.last_error() and int(st.item()) == -1
    assert m.lib().b3w_sample_plan_group_batch_device(ctx.handle, ln64.ctypes.data, ln64.size, g, grp["outboards"].data_ptr(), grp["roots"].data_ptr(),
                                                       f1.ctypes.data, c1.ctypes.data, 0, None, None, None, 0) == 0              # no samples: nothing
    comp = m.Context("compression", 0)
    with pytest.raises(m.B3WError):
        m.bao.plan_samples_groups_batch(comp, grp["outboards"], lens, grp["roots"], files, chunks, gb, g)
    comp.close()
    ctx.close()


@pytest.mark.parametrize("g", GS)
def test_reference_transcript_from_the_group_outboard(g):
    """the incomplete-trees golden (the reference WASM driven along every path of 2 ... 100-chunk trees) replayed through the group
    planner: the last leaf block and every parent step, planned from the group outboards and the groups' bytes; all trees one batch"""
    import torch
    m = T.pkg()
    W = T.workloads()
    ctx = m.Context("nova_vesta", 0)
    doc = json.load(gzip.open(os.path.join(T.GOLD, "incomplete_trees.nova_vesta.json.gz"), "rt"))
    lens = [tree["n_chunks"] * 1024 for tree in doc["trees"]]
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    arena = np.concatenate([np.frombuffer(W.lcg_preimage(ln, seed=1).tobytes(), dtype=np.uint8) for ln in lens])
    out = m.bao.outboard_groups_batch(ctx, torch.from_numpy(arena).cuda(), offsets, lens, g)
    roots = out["roots"].cpu().numpy().view(np.uint32)
    files = np.array([f for f, tree in enumerate(doc["trees"]) for _ in tree["leaves"]], dtype=np.uint32)
    chunks = np.array([leaf["leaf"] for tree in doc["trees"] for leaf in tree["leaves"]], dtype=np.uint64)
    only = m.bao.group_bytes_batch(arena, offsets, lens, files, chunks, g)      # the planner sees these bytes and the group outboards, no more
    plan = m.bao.plan_samples_groups_batch(ctx, out["outboards"], lens, out["roots"], files, chunks, only, g)
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


@pytest.mark.parametrize("g", [1, 4, 6])
def test_tampering_stays_local(g):
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    G = 1 << g
    lens = [(5 * G + G // 2) * 1024 + 500, 3 * G * 1024, (2 * G + 1) * 1024 + 1, G * 1024 + 9, 700]
    n = [m.bao.num_chunks(x) for x in lens]
    arena, offsets = _arena(lens, starts_odd=(1,), seed=9)
    ob = m.bao.outboard_groups_batch(ctx, torch.from_numpy(arena).cuda(), offsets, lens, g)
    #                  0  1       2      3          4          5  6         7  8      9      10 11 12
    files = np.array([0, 1,      2,     0,         1,         2, 0,        1, 2,     1,     3, 3, 4], dtype=np.uint32)
    chunks = np.array([0, G + 1, 2 * G, 3 * G + 1, 3 * G - 1, 0, n[0] - 1, G, G + 1, G - 1, 0, G, 0], dtype=np.uint64)
    good = m.bao.group_bytes_batch(arena, offsets, lens, files, chunks, g)
    obs, roots = ob["outboards"], ob["roots"]
    N = files.size

    def plan(obs_t=obs, gb=good, roots_t=roots):
        out = m.bao.plan_samples_groups_batch(ctx, obs_t, lens, roots_t, files, chunks, gb, g)
        return list(out["sample_status"]), out["records"]

    def expect(**hit):
        return [hit.get(f"s{s}", 0) for s in range(N)]
    st0, recs0 = plan()
    assert st0 == [0] * N
    rf = m.bao.sample_rows_batch(lens, files, chunks)

    def untouched_equal(recs, touched):
        for s in range(N):
            if s not in touched:
                assert torch.equal(recs[int(rf[s]):int(rf[s + 1])], recs0[int(rf[s]):int(rf[s + 1])]), s
    # a flipped byte in ANOTHER chunk of sample 3's group (file 0, chunk 3 G + 1: the byte is in chunk 3 G): status 1 for that sample alone;
    # its own leaf records do not see the byte, its parent records may (the recomputed sibling)
    gb = good.clone()
    gb[3, 100] ^= 1
    st, recs = plan(gb=gb)
    assert st == expect(s3=1)
    untouched_equal(recs, {3})
    nb = 16
    assert torch.equal(recs[int(rf[3]):int(rf[3]) + nb], recs0[int(rf[3]):int(rf[3]) + nb])
    # samples 1 and 7 share a group of file 1 (chunks G + 1 and G) but each brings its own copy of the group's bytes: a byte flipped in
    # sample 7's copy, inside chunk G + 1, is sample 7's alone
    gb = good.clone()
    gb[7, 1024 + 5] ^= 1
    st, recs = plan(gb=gb)
    assert st == expect(s7=1)
    untouched_equal(recs, {7})
    # a flipped byte in the sampled chunk itself (sample 4: file 1, chunk 3 G - 1, the last of its group)
    gb = good.clone()
    gb[4, (G - 1) * 1024 + 17] ^= 1
    st, recs = plan(gb=gb)
    assert st == expect(s4=1)
    untouched_equal(recs, {4})
    cb1 = gb
    # a flipped stored node of file 1: 2 for exactly the samples whose group_path_nodes hold it
    mine = [s for s in range(N) if files[s] == 1]
    paths = {s: m.bao.group_path_nodes(int(chunks[s]), n[1], g) for s in mine}
    assert paths[4] == R.path_nodes((3 * G - 1) >> g, 3)
    node = paths[1][-1]
    hit = {s for s in mine if node in paths[s]}
    assert hit and hit != set(mine)
    bad = obs.clone()
    bad[int(ob["ob_first"][1]) + 8 + 64 * node + 3] ^= 1
    st, recs = plan(obs_t=bad)
    assert st == [2 if s in hit else 0 for s in range(N)]
    untouched_equal(recs, hit)
    # a flipped root word of file 2: its three samples, no other
    wrong = roots.clone()
    wrong[2, 4] ^= 1
    st, recs = plan(roots_t=wrong)
    assert st == expect(s2=2, s5=2, s8=2)
    untouched_equal(recs, set())                                  # (the records do not depend on the root)
    # the root of a file of one chunk (sample 12): no stored node at all, the chunk's ROOT output against the root
    wrong1 = roots.clone()
    wrong1[4, 0] ^= 1
    st, recs = plan(roots_t=wrong1)
    assert st == expect(s12=1)                                    # (as the existing planner: with no stored node on the path the mismatch is the bytes')
    untouched_equal(recs, set())
    # a wrong header of file 3
    bad3 = obs.clone()
    bad3[int(ob["ob_first"][3])] ^= 1
    st, recs = plan(obs_t=bad3)
    assert st == expect(s10=3, s11=3)
    untouched_equal(recs, set())
    # all at once
    bad3[int(ob["ob_first"][1]) + 8 + 64 * node + 3] ^= 1
    st, recs = plan(obs_t=bad3, gb=cb1, roots_t=wrong)
    want = [2 if s in hit else 0 for s in range(N)]
    if want[4] == 0:
        want[4] = 1
    for s in (2, 5, 8):
        want[s] = 2
    want[10] = want[11] = 3
    assert st == want
    untouched_equal(recs, hit | {4})
    ctx.close()


def test_prove_samples_groups_batch_equals_prove_samples_batch():
    import torch
    import ec_ref as E
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    g = 4
    lens = [43 * 1024 + 33, 16 * 1024, 700, 32 * 1024]
    arena, offsets = _arena(lens, seed=2)
    d_arena = torch.from_numpy(arena).cuda()
    full = m.bao.outboard_batch(ctx, d_arena, offsets, lens)
    grp = m.bao.outboard_groups_batch(ctx, d_arena, offsets, lens, g)
    files = np.array([0, 1, 0, 2, 1, 0, 3, 3], dtype=np.uint32)
    chunks = np.array([3, 4, 43, 0, 15, 32, 16, 0], dtype=np.uint64)
    cb = m.bao.chunk_bytes_batch(arena, offsets, lens, files, chunks)
    gb = m.bao.group_bytes_batch(arena, offsets, lens, files, chunks, g)
    roots = full["roots"].cpu().numpy().view(np.uint32)
    key = m.CommitKey(ctx, "pallas", E.points_to_bytes(E.random_points("pallas", ctx.witness_size)), window=12)
    r1cs = m.R1cs(ctx)
    want = m.bao.prove_samples_batch(ctx, full["outboards"], lens, full["roots"], files, chunks, cb, batch_steps=16, commit_key=key)
    got = m.bao.prove_samples_groups_batch(ctx, grp["outboards"], lens, grp["roots"], files, chunks, gb, g, batch_steps=16, commit_key=key)
    want2 = m.bao.prove_samples_batch(ctx, full["outboards"], lens, full["roots"], files, chunks, cb, batch_steps=7, r1cs=r1cs)
    got2 = m.bao.prove_samples_groups_batch(ctx, grp["outboards"], lens, grp["roots"], files, chunks, gb, g, batch_steps=7, r1cs=r1cs)
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
