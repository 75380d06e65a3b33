"""Challenged paths and slices read in place from the file arena (bao.plan_samples_arena / prove_samples_arena / slices_arena,
b3w_sample_plan_arena_device / b3w_bao_slice_arena_device) against the gathered route: plan_samples_batch /
plan_samples_groups_batch / slices_batch fed by chunk_bytes_batch / group_bytes_batch of the same arena.  The arena is random
everywhere, between and behind the files too: the gathered route pads with zeros and the arena route sees the file's own
neighbourhood, so the two can only agree if nothing past a file's end enters a hash.  The files start at every class of byte
alignment the kernels tell apart (offset mod 16 in 0, 1, 4, 8, 12, 15)."""
import ctypes
import gzip
import json
import os

import numpy as np
import pytest

import b3w_testlib as T
import bao_ref as R
from test_gpu_bao_groups import _sample_chunks

pytestmark = pytest.mark.gpu

GS = [0, 1, 4, 6]
K = 1024
# (length, offset mod 16): the 3 Mi + 5 file and one file of each group size (2 048, 16 Ki, 64 Ki bytes) start odd
FILES = [(0, 4), (1, 15), (1023, 0), (K, 8), (1025, 12), (2 * K, 1), (3073, 4), (16 * K - 1, 0), (16 * K, 15), (16 * K + 1, 8),
         (64 * K - 1, 12), (64 * K, 1), (64 * K + 1, 0), (65 * K + 7, 4), (1 << 20, 8), ((1 << 20) + 1025, 12), ((3 << 20) + 5, 15)]
LENS = [ln for ln, _ in FILES]
ONE_GROUP = {0: LENS.index(K), 1: LENS.index(2 * K), 4: LENS.index(16 * K), 6: LENS.index(64 * K)}     # a file of exactly one group
ONE_CHUNK, BIG, RAGGED = LENS.index(1023), LENS.index((3 << 20) + 5), LENS.index((1 << 20) + 1025)
_WORLD = {}


def _place(lens_mods, rng, tail=257):
    """-> (arena, offsets): the files one behind the other with a gap of 16 .. 47 bytes in front of each, file f at its offset mod 16;
    every byte of the arena random (the callers put their own bytes into the files where they need to)"""
    at, offsets = 0, []
    for ln, mod in lens_mods:
        at = (at + 32 + 15) // 16 * 16 + mod
        offsets.append(at)
        at += ln
    return rng.integers(0, 256, at + tail, dtype=np.uint8), np.array(offsets, dtype=np.uint64)


def _world():
    import torch
    if not _WORLD:
        arena, offsets = _place(FILES, np.random.default_rng(13))
        assert sorted(set(int(o) % 16 for o in offsets)) == [0, 1, 4, 8, 12, 15]
        assert int(offsets[BIG]) % 2 == 1 and all(int(offsets[ONE_GROUP[g]]) % 2 == 1 for g in (1, 4, 6))
        _WORLD.update(arena=arena, offsets=offsets, d_arena=torch.from_numpy(arena).cuda(), per_g={})
    return _WORLD


def _made(m, ctx, g):
    """what the tests of one group size share, made once: the outboards (full and over groups of 1 << g chunks), the listed samples
    and the gathered route's plan and slices for them"""
    import torch
    w = _world()
    if g not in w["per_g"]:
        d_arena, offsets = w["d_arena"], w["offsets"]
        full = m.bao.outboard_batch(ctx, d_arena, offsets, LENS)
        obs = full if g == 0 else m.bao.outboard_groups_batch(ctx, d_arena, offsets, LENS, g)
        rng = np.random.default_rng(900 + g)
        files, chunks = [], []
        for f, ln in enumerate(LENS):
            for c in _sample_chunks(m.bao.num_chunks(ln), g, rng):
                files.append(f)
                chunks.append(c)
        perm = rng.permutation(len(files))
        files, chunks = np.array(files, dtype=np.uint32)[perm], np.array(chunks, dtype=np.uint64)[perm]
        plan, slices = _gathered(m, ctx, g, d_arena, obs["outboards"], obs["roots"], files, chunks, want_slices=True)
        assert (plan["sample_status"] == 0).all()
        torch.cuda.synchronize()
        w["per_g"][g] = dict(full=full, obs=obs, files=files, chunks=chunks, plan=plan, slices=slices)
    return w["per_g"][g]


def _gathered(m, ctx, g, d_arena, d_obs, d_roots, files, chunks, want_slices=False):
    """the yardstick: the existing calls on the bytes gathered from d_arena -> (plan, slices or None)"""
    offsets = _world()["offsets"]
    if g == 0:
        d_bytes = m.bao.chunk_bytes_batch(d_arena, offsets, LENS, files, chunks)
        plan = m.bao.plan_samples_batch(ctx, d_obs, LENS, d_roots, files, chunks, d_bytes)
    else:
        d_bytes = m.bao.group_bytes_batch(d_arena, offsets, LENS, files, chunks, g)
        plan = m.bao.plan_samples_groups_batch(ctx, d_obs, LENS, d_roots, files, chunks, d_bytes, g)
    return plan, (m.bao.slices_batch(ctx, d_obs, LENS, files, chunks, d_bytes, group_log=g) if want_slices else None)


def _assert_plans_equal(got, want, files, chunks, what):
    import torch
    assert list(got["row_first"]) == list(want["row_first"]) and got["records"].shape == want["records"].shape, what
    assert list(got["sample_status"]) == list(want["sample_status"]), (what, [(int(files[s]), int(chunks[s]), int(got["sample_status"][s]), int(want["sample_status"][s]))
                                                                         for s in np.nonzero(got["sample_status"] != want["sample_status"])[0][:10]])
    assert list(got["provable"]) == list(want["provable"]), what
    if not torch.equal(got["records"], want["records"]):
        rf = want["row_first"]
        diff = [(int(files[s]), int(chunks[s])) for s in range(files.size)
                if not torch.equal(got["records"][int(rf[s]):int(rf[s + 1])], want["records"][int(rf[s]):int(rf[s + 1])])]
        raise AssertionError(f"{what}: the records of {len(diff)} of {files.size} samples differ, first (file, chunk): {diff[:10]}")


def _assert_slices_equal(m, got, want, files, chunks, what):
    """byte for byte over every [slice_first[s], + slice_size)"""
    assert list(got["slice_first"]) == list(want["slice_first"]), what
    a, b, sf = got["slices"].cpu().numpy(), want["slices"].cpu().numpy(), want["slice_first"]
    for s in range(files.size):
        lo, size = int(sf[s]), m.bao.slice_size(LENS[files[s]], int(chunks[s]))
        assert a[lo:lo + size].tobytes() == b[lo:lo + size].tobytes(), (what, s, int(files[s]), int(chunks[s]))


@pytest.mark.parametrize("g", GS)
def test_records_equal_the_gathered_route(g):
    m = T.pkg()
    ctx = m.Context("nova_bn254", 0)
    w = _world()
    k = _made(m, ctx, g)
    files, chunks = k["files"], k["chunks"]
    n_of = np.array([m.bao.num_chunks(x) for x in LENS])
    assert all(((files == f) & (chunks == 0)).any() and ((files == f) & (chunks == n_of[f] - 1)).any() for f in range(len(LENS)))
    assert g == 0 or any(n_of[f] % (1 << g) and c >= n_of[f] // (1 << g) * (1 << g) for f, c in zip(files, chunks))   # a short last group
    got = m.bao.plan_samples_arena(ctx, w["d_arena"], w["offsets"], LENS, k["obs"]["outboards"], k["obs"]["roots"], files, chunks, group_log=g)
    assert (got["sample_status"] == 0).all(), [(int(files[s]), int(chunks[s]), int(got["sample_status"][s])) for s in np.nonzero(got["sample_status"])[0][:10]]
    _assert_plans_equal(got, k["plan"], files, chunks, f"g = {g}")
    assert got["provable"].any() and not got["provable"].all()
    print(f"g = {g}: {files.size} samples of {len(LENS)} files, {got['records'].shape[0]} rows compared word for word")
    none = m.bao.plan_samples_arena(ctx, w["d_arena"], w["offsets"], LENS, k["obs"]["outboards"], k["obs"]["roots"], [], [], group_log=g)
    assert none["records"].shape == (0, 32) and none["sample_status"].size == 0
    ctx.close()


@pytest.mark.parametrize("g", [0, 4])
def test_reference_transcript_through_the_arena(g):
    """the incomplete-trees golden (the reference WASM driven along every path of 2 ... 100-chunk trees) replayed through the arena
    planner: the last leaf block and every parent step, all trees one batch, the files at every byte alignment"""
    import torch
    m = T.pkg()
    W = T.workloads()
    ctx = m.Context("nova_vesta", 0)
    doc = json.load(gzip.open(os.path.join(T.GOLD, "incomplete_trees.nova_vesta.json.gz"), "rt"))
    lens = [tree["n_chunks"] * 1024 for tree in doc["trees"]]
    arena, offsets = _place([(ln, (5 * f + 1) % 16) for f, ln in enumerate(lens)], np.random.default_rng(3))
    for f, ln in enumerate(lens):
        arena[int(offsets[f]):int(offsets[f]) + ln] = np.frombuffer(W.lcg_preimage(ln, seed=1).tobytes(), dtype=np.uint8)
    d_arena = torch.from_numpy(arena).cuda()
    out = m.bao.outboard_groups_batch(ctx, d_arena, offsets, lens, g)
    roots = out["roots"].cpu().numpy().view(np.uint32)
    files = np.array([f for f, tree in enumerate(doc["trees"]) for _ in tree["leaves"]], dtype=np.uint32)
    chunks = np.array([leaf["leaf"] for tree in doc["trees"] for leaf in tree["leaves"]], dtype=np.uint64)
    plan = m.bao.plan_samples_arena(ctx, d_arena, offsets, lens, out["outboards"], out["roots"], files, chunks, group_log=g)
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
            for j, stp in enumerate(steps):
                assert list(recs[int(rf[s]) + 15 + j]) == stp["record"], (tree["n_chunks"], leaf["leaf"], j)
            s += 1
    assert s == files.size
    ctx.close()


@pytest.mark.parametrize("g", GS)
def test_slices_equal_the_gathered_route(g):
    import torch
    m = T.pkg()
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    w = _world()
    k = _made(m, ctx, g)
    files, chunks, want = k["files"], k["chunks"], k["slices"]
    arena, offsets, d_arena = w["arena"], w["offsets"], w["d_arena"]
    ln, off = np.array(LENS, dtype=np.uint64), w["offsets"]
    got = m.bao.slices_arena(ctx, d_arena, offsets, LENS, k["obs"]["outboards"], files, chunks, group_log=g)
    _assert_slices_equal(m, got, want, files, chunks, f"g = {g}")
    # through the C entry into a prefilled buffer: the same bytes, every padding byte and everything behind the slices untouched
    sf = want["slice_first"]
    total, guard = int(sf[-1]), 4096
    d_slices = torch.full((total + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    s0 = torch.cuda.current_stream().cuda_stream
    assert L.b3w_bao_slice_arena_device(ctx.handle, d_arena.data_ptr(), d_arena.numel(), off.ctypes.data, ln.ctypes.data, ln.size, g,
                                        k["obs"]["outboards"].data_ptr(), None, None, 0, d_slices.data_ptr(), s0) == 0     # no samples: nothing
    torch.cuda.synchronize()
    assert bool((d_slices == 0xA5).all().item())
    assert L.b3w_bao_slice_arena_device(ctx.handle, d_arena.data_ptr(), d_arena.numel(), off.ctypes.data, ln.ctypes.data, ln.size, g,
                                        k["obs"]["outboards"].data_ptr(), files.ctypes.data, chunks.ctypes.data, files.size, d_slices.data_ptr(), s0) == 0, ctx.last_error()
    torch.cuda.synchronize()
    host, ref = d_slices.cpu().numpy(), want["slices"].cpu().numpy()
    assert (host[total:] == 0xA5).all(), "the call wrote behind the slices"
    at = 0
    for s in range(files.size):
        a, size = int(sf[s]), m.bao.slice_size(LENS[files[s]], int(chunks[s]))
        assert (host[at:a] == 0xA5).all(), f"padding in front of slice {s} was written"
        assert host[a:a + size].tobytes() == ref[a:a + size].tobytes(), (s, int(files[s]), int(chunks[s]))
        at = a + size
    assert (host[at:total] == 0xA5).all()
    if g == 0:                                                     # the restatement's slice, and the host decoder against the file's root
        full_host = k["full"]["outboards"].cpu().numpy()
        ob_first = k["full"]["ob_first"]
        roots = k["full"]["roots"].cpu().numpy().view(np.uint32)
        for s in range(files.size):
            f, c = int(files[s]), int(chunks[s])
            data = arena[int(offsets[f]):int(offsets[f]) + LENS[f]].tobytes()
            a, size = int(sf[s]), m.bao.slice_size(LENS[f], c)
            sl = host[a:a + size].tobytes()
            assert sl == R.slice_chunk(full_host[int(ob_first[f]):int(ob_first[f + 1])].tobytes(), data, c), (s, f, c)
            assert m.bao.decode_slice(sl, LENS[f], c, roots[f]) == (0, data[c * 1024:c * 1024 + 1024]), (s, f, c)
    ctx.close()


@pytest.mark.parametrize("g", GS)
def test_tampering_equals_the_gathered_route_and_stays_local(g):
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    w = _world()
    k = _made(m, ctx, g)
    files, chunks, offsets = k["files"], k["chunks"], w["offsets"]
    d_obs, d_roots = k["obs"]["outboards"], k["obs"]["roots"]
    G = 1 << g
    N = files.size

    def both(d_arena=w["d_arena"], obs=d_obs, roots=d_roots):
        got = m.bao.plan_samples_arena(ctx, d_arena, offsets, LENS, obs, roots, files, chunks, group_log=g)
        want, _ = _gathered(m, ctx, g, d_arena, obs, roots, files, chunks)
        _assert_plans_equal(got, want, files, chunks, f"g = {g}")
        return got
    sampled = set(zip(files.tolist(), chunks.tolist()))
    # 1. a byte in the gap right behind a file's end (a ragged last chunk in a short last group): nothing changes
    t = w["d_arena"].clone()
    for f in (RAGGED, BIG, ONE_CHUNK):
        t[int(offsets[f]) + LENS[f]] ^= 0x40
    got = both(d_arena=t)
    assert (got["sample_status"] == 0).all() and torch.equal(got["records"], k["plan"]["records"])
    # 2. a byte in a sampled chunk of a one-chunk file, of a file of exactly one group and of a multi-tile file, and (g >= 1) a byte in
    #    a chunk that is not sampled but lies in a sampled group: status 1 for exactly the samples of those chunks' groups
    hit = [(ONE_CHUNK, 0, 700), (ONE_GROUP[g], G - 1, 1000), (BIG, 2048, 0)]
    assert all((f, c) in sampled for f, c, _ in hit)
    if g:
        f2, c2 = next((f, (c ^ 1)) for f, c in sorted(sampled) if f == RAGGED and (f, c ^ 1) not in sampled and (c ^ 1) * 1024 + 5 < LENS[f])
        hit.append((f2, c2, 5))
    t = w["d_arena"].clone()
    for f, c, b in hit:
        t[int(offsets[f]) + c * 1024 + b] ^= 1
    got = both(d_arena=t)
    want_st = [1 if any(f == hf and (c >> g) == (hc >> g) for hf, hc, _ in hit) else 0 for f, c in zip(files.tolist(), chunks.tolist())]
    assert list(got["sample_status"]) == want_st and 3 <= sum(want_st) < N
    # 3. a stored node of the multi-tile file: 2 for exactly the samples whose path holds it
    mine = [s for s in range(N) if files[s] == BIG]
    n_big = m.bao.num_chunks(LENS[BIG])
    paths = {s: m.bao.group_path_nodes(int(chunks[s]), n_big, g) for s in mine}
    node = paths[mine[0]][-1]
    held = {s for s in mine if node in paths[s]}
    assert held and held != set(mine)
    bad = d_obs.clone()
    bad[int(k["obs"]["ob_first"][BIG]) + 8 + 64 * node + 35] ^= 1
    got = both(obs=bad)
    assert list(got["sample_status"]) == [2 if s in held else 0 for s in range(N)]
    # 4. a wrong root: 2 for every sample of a file with stored nodes, 1 for those of a file of one unit; a wrong header: 3
    wrong = d_roots.clone()
    wrong[BIG, 3] ^= 1
    wrong[ONE_CHUNK, 0] ^= 1
    bad = d_obs.clone()
    bad[int(k["obs"]["ob_first"][RAGGED]) + 1] ^= 1
    got = both(obs=bad, roots=wrong)
    assert list(got["sample_status"]) == [2 if f == BIG else 1 if f == ONE_CHUNK else 3 if f == RAGGED else 0 for f in files.tolist()]
    ctx.close()


@pytest.mark.parametrize("g", [4, 6])
def test_forty_calls_on_fresh_samples(g):
    """the grouped bodies merge in LDS and store almost nothing, the case in which a missing LDS wait showed as a wrong CV in some
    calls only: 40 calls, every record, status and slice byte of every call against the gathered route"""
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    w = _world()
    k = _made(m, ctx, g)
    d_arena, offsets, d_obs, d_roots = w["d_arena"], w["offsets"], k["obs"]["outboards"], k["obs"]["roots"]
    rng = np.random.default_rng(700 + g)
    n_of = np.array([m.bao.num_chunks(x) for x in LENS])
    rows = 0
    for call in range(40):
        files = rng.integers(0, len(LENS), 48).astype(np.uint32)
        chunks = np.array([rng.integers(0, n_of[f]) for f in files], dtype=np.uint64)
        got = m.bao.plan_samples_arena(ctx, d_arena, offsets, LENS, d_obs, d_roots, files, chunks, group_log=g)
        got_sl = m.bao.slices_arena(ctx, d_arena, offsets, LENS, d_obs, files, chunks, group_log=g)
        want, want_sl = _gathered(m, ctx, g, d_arena, d_obs, d_roots, files, chunks, want_slices=True)
        assert (got["sample_status"] == 0).all(), (g, call)
        _assert_plans_equal(got, want, files, chunks, f"g = {g}, call {call}")
        assert torch.equal(got_sl["slices"], want_sl["slices"]), f"g = {g}, call {call}: the slices differ"      # (both start from zeros)
        rows += got["records"].shape[0]
    print(f"g = {g}: 40 calls, {rows} rows compared")
    ctx.close()


def test_prove_samples_arena_equals_prove_samples_groups_batch():
    import torch
    import ec_ref as E
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    w = _world()
    g = 4
    k = _made(m, ctx, g)
    d_arena, offsets, d_obs, d_roots = w["d_arena"], w["offsets"], k["obs"]["outboards"], k["obs"]["roots"]
    files = np.array([LENS.index(65 * K + 7), ONE_GROUP[4], ONE_CHUNK, LENS.index(3073), LENS.index(65 * K + 7), 0], dtype=np.uint32)
    chunks = np.array([3, 15, 0, 3, 65, 0], dtype=np.uint64)
    gb = m.bao.group_bytes_batch(d_arena, offsets, LENS, files, chunks, g)
    key = m.CommitKey(ctx, "pallas", E.points_to_bytes(E.random_points("pallas", ctx.witness_size)), window=12)
    want = m.bao.prove_samples_groups_batch(ctx, d_obs, LENS, d_roots, files, chunks, gb, g, batch_steps=16, commit_key=key)
    got = m.bao.prove_samples_arena(ctx, d_arena, offsets, LENS, d_obs, d_roots, files, chunks, group_log=g, batch_steps=16, commit_key=key)
    assert (got["sample_status"] == 0).all()
    assert torch.equal(got["records"], want["records"]) and list(got["row_first"]) == list(want["row_first"])
    assert torch.equal(got["public"], want["public"]) and torch.equal(got["status"], want["status"]) and (got["status"] == 0).all().item()
    assert torch.equal(got["points"], want["points"]) and got["violations"] is None
    key.close()
    ctx.close()


def test_no_gathered_copy_is_made():
    """256 samples at g = 6: the gathered route needs 16 MiB of group bytes; the arena route may allocate the tensors it returns
    and at most 1 MiB more"""
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    w = _world()
    g = 6
    k = _made(m, ctx, g)
    rng = np.random.default_rng(6)
    n_of = np.array([m.bao.num_chunks(x) for x in LENS])
    files = rng.integers(0, len(LENS), 256).astype(np.uint32)
    chunks = np.array([rng.integers(0, n_of[f]) for f in files], dtype=np.uint64)
    args = (ctx, w["d_arena"], w["offsets"], LENS, k["obs"]["outboards"], k["obs"]["roots"], files, chunks)
    m.bao.plan_samples_arena(*args, group_log=g)                     # (the context's staging is its own, made here once)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    out = m.bao.plan_samples_arena(*args, group_log=g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    returned = out["records"].numel() * 4
    print(f"start {start}, peak {peak}: {peak - start} bytes above the start, {returned} of them returned; the gathered bytes would be {256 * (1024 << g)}")
    assert (out["sample_status"] == 0).all()
    assert peak - start <= returned + (1 << 20)
    ctx.close()


def test_refusals_write_nothing():
    import torch
    m = T.pkg()
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    w = _world()
    g = 4
    k = _made(m, ctx, g)
    d_arena, d_obs, d_roots = w["d_arena"], k["obs"]["outboards"], k["obs"]["roots"]
    ln, off = np.array(LENS, dtype=np.uint64), w["offsets"]
    fi, ch = np.array([BIG, ONE_CHUNK], dtype=np.uint32), np.array([7, 0], dtype=np.uint64)
    rows = int(m.bao.sample_rows_batch(ln, fi, ch)[-1])
    d_recs = torch.full((rows, 32), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_st = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    d_slices = torch.full((int(m.bao.slice_layout(ln, fi, ch)[-1]),), 0xA5, dtype=torch.uint8, device="cuda")
    ok = dict(ctx=ctx.handle, arena=d_arena.data_ptr(), arena_bytes=d_arena.numel(), off=off.ctypes.data, ln=ln.ctypes.data, n_files=ln.size, g=g,
              obs=d_obs.data_ptr(), roots=d_roots.data_ptr(), fi=fi.ctypes.data, ch=ch.ctypes.data, n=2)

    def plan(**kw):
        a = {**ok, **kw}
        return L.b3w_sample_plan_arena_device(a["ctx"], a["arena"], a["arena_bytes"], a["off"], a["ln"], a["n_files"], a["g"], a["obs"], a["roots"], a["fi"],
                                              a["ch"], a["n"], d_recs.data_ptr(), d_st.data_ptr(), 0)

    def slices(**kw):
        a = {**ok, **kw}
        return L.b3w_bao_slice_arena_device(a["ctx"], a["arena"], a["arena_bytes"], a["off"], a["ln"], a["n_files"], a["g"], a["obs"], a["fi"], a["ch"], a["n"],
                                            d_slices.data_ptr(), 0)
    bad_file, bad_chunk = np.array([BIG, len(LENS)], dtype=np.uint32), np.array([7, 1], dtype=np.uint64)
    short = int(off[BIG]) + LENS[BIG] - 1                           # an arena one byte too short for the sampled multi-tile file
    cases = [(dict(obs=None), "null"), (dict(arena=None), "null arena"), (dict(off=None), "null"), (dict(g=7), "group_log"),
             (dict(fi=bad_file.ctypes.data), "file index"), (dict(ch=bad_chunk.ctypes.data), "chunk index"), (dict(arena_bytes=short), "arena_bytes"),
             (dict(obs=d_obs.data_ptr() + 4), "aligned")]
    for call in (plan, slices):
        for kw, word in cases:
            assert call(**kw) == m.B3W_E_BAD_ARGUMENT, (call.__name__, kw)
            assert word in ctx.last_error(), (call.__name__, kw, ctx.last_error())
    assert plan(roots=None) == m.B3W_E_BAD_ARGUMENT and "null" in ctx.last_error()
    assert plan(ctx=None) == m.B3W_E_BAD_ARGUMENT and slices(ctx=None) == m.B3W_E_BAD_ARGUMENT
    comp = m.Context("compression", 0)                              # the planner's records are the nova step circuits'; slices are anyone's
    assert plan(ctx=comp.handle) == m.B3W_E_BAD_ARGUMENT and "nova" in comp.last_error()
    with pytest.raises(m.B3WError):
        m.bao.plan_samples_arena(comp, d_arena, off, LENS, d_obs, d_roots, fi, ch, group_log=g)
    torch.cuda.synchronize()
    assert bool((d_recs == 0x5A5A5A5A).all().item()) and bool((d_st == -7).all().item()) and bool((d_slices == 0xA5).all().item())
    assert slices(ctx=comp.handle) == 0
    comp.close()
    with pytest.raises(m.B3WError):
        m.bao.plan_samples_arena(ctx, d_arena, off, LENS, d_obs, d_roots, [len(LENS)], [0], group_log=g)
    with pytest.raises(m.B3WError):
        m.bao.slices_arena(ctx, d_arena[:short], off, LENS, d_obs, fi, ch, group_log=g)
    with pytest.raises(m.B3WError):
        m.bao.slices_arena(ctx, d_arena, off, LENS, d_obs, fi, ch, group_log=7)
    # and the same arguments untouched are accepted
    assert plan() == 0 and slices() == 0
    torch.cuda.synchronize()
    assert bool((d_st == 0).all().item())
    ctx.close()
