"""Bao outboards and challenged paths over a batch of files in one pass (bao.outboard_batch / plan_samples_batch /
prove_samples_batch, b3w_bao_outboard_batch_device / b3w_sample_plan_batch_device): every file's outboard and root are those of the
plain-Python restatement (tests/bao_ref.py) or of the single-file call on that file alone, the planned records are sample by sample
those of the single-file planner, tampering stays with the sample it hits, and the batch call beats a loop of single-file calls."""
import statistics
import time

import numpy as np
import pytest

import b3w_testlib as T
import bao_ref as R
import blake3_ref as B

pytestmark = pytest.mark.gpu


def _arena(lens, starts_odd=(), gap=48, seed=1):
    """an arena holding files of these lengths one behind the other, 16-byte aligned starts with a gap in front of each, except the
    files in starts_odd, which start on an odd byte.  -> (numpy arena, offsets)"""
    at, offsets = 0, []
    for f, ln in enumerate(lens):
        at = (at + gap + 15) // 16 * 16 + (1 + 2 * (f % 7) if f in starts_odd else 0)
        offsets.append(at)
        at += ln
    arena = np.random.default_rng(seed).integers(0, 256, at + 64, dtype=np.uint8)
    return arena, np.array(offsets, dtype=np.uint64)


def _file(arena, offsets, lens, f):
    return arena[int(offsets[f]):int(offsets[f]) + int(lens[f])].tobytes()


def _slices(out, f):
    a, b = int(out["ob_first"][f]), int(out["ob_first"][f + 1])
    return out["outboards"][a:b], out["roots"][f]


def _check_against_restatement(out, arena, offsets, lens, files):
    obs = out["outboards"].cpu().numpy()
    roots = out["roots"].cpu().numpy().view(np.uint32)
    cache = {}
    for f in files:
        data = _file(arena, offsets, lens, f)
        if data not in cache:
            cache[data] = R.outboard(data)
        want_ob, want_root = cache[data]
        assert want_root == B.hash_words(data)
        a, b = int(out["ob_first"][f]), int(out["ob_first"][f + 1])
        assert obs[a:b].tobytes() == want_ob, (f, lens[f])
        assert list(roots[f]) == want_root, (f, lens[f])


def test_every_shape_against_the_restatement():
    import torch
    m = T.pkg()
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    K = 1024
    base = [0, 1, 1023, K, 1025, 3 * K + 5, 37 * K, 100 * K + 77, 1023 * K, 1 << 20, (1 << 20) + 1, 1025 * K, 2049 * K + 3, 3 << 20]
    order = np.random.default_rng(3).permutation(len(base))
    lens = [base[i] for i in order]
    arena, offsets = _arena(lens, starts_odd=(2, 9))
    assert int(offsets[2]) % 2 == 1 and int(offsets[9]) % 2 == 1
    dup = lens.index(100 * K + 77)                               # one length listed twice at the same offset
    lens.append(lens[dup])
    offsets = np.append(offsets, offsets[dup])
    ln = np.array(lens, dtype=np.uint64)
    d_arena = torch.from_numpy(arena).cuda()
    ob_first = m.bao.batch_layout(ln)
    total = int(ob_first[-1])
    guard = 4096
    d_obs = torch.full((total + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    d_roots = torch.zeros((len(lens), 8), dtype=torch.int32, device="cuda")
    need = L.b3w_bao_batch_scratch_bytes(ln.ctypes.data, ln.size)
    d_scratch = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    # a scratch one byte short is refused before anything runs
    assert L.b3w_bao_outboard_batch_device(ctx.handle, d_arena.data_ptr(), offsets.ctypes.data, ln.ctypes.data, ln.size, d_obs.data_ptr(),
                                           d_roots.data_ptr(), d_scratch.data_ptr(), need - 1, 0) == m.B3W_E_BAD_ARGUMENT
    assert "scratch" in ctx.last_error()
    torch.cuda.synchronize()
    assert bool((d_obs == 0xA5).all().item())
    assert L.b3w_bao_outboard_batch_device(ctx.handle, d_arena.data_ptr(), offsets.ctypes.data, ln.ctypes.data, ln.size, d_obs.data_ptr(),
                                           d_roots.data_ptr(), d_scratch.data_ptr(), need, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert bool((d_obs[total:] == 0xA5).all().item()), "the batch call wrote behind the outboards"
    out = dict(outboards=d_obs[:total], ob_first=ob_first, roots=d_roots)
    _check_against_restatement(out, arena, offsets, lens, range(len(lens)))
    # and through bao.outboard_batch: the same bytes; no files: nothing
    again = m.bao.outboard_batch(ctx, d_arena, offsets, ln)
    assert torch.equal(again["outboards"], d_obs[:total]) and torch.equal(again["roots"], d_roots) and list(again["ob_first"]) == list(ob_first)
    none = m.bao.outboard_batch(ctx, d_arena, [], [])
    assert none["outboards"].numel() == 0 and none["roots"].shape == (0, 8) and list(none["ob_first"]) == [0]
    ctx.close()


def test_many_small_files():
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    rng = np.random.default_rng(2048)
    lens = rng.integers(0, 8 * 1024 + 1, 2048).astype(np.uint64)
    arena, offsets = _arena([int(x) for x in lens], starts_odd=set(range(0, 2048, 3)), gap=0)
    out = m.bao.outboard_batch(ctx, torch.from_numpy(arena).cuda(), offsets, lens)
    _check_against_restatement(out, arena, offsets, [int(x) for x in lens], range(2048))
    # 100 000 files packed back to back, made on the device
    n_files = 100000
    lens = rng.integers(0, 32 * 1024 + 1, n_files).astype(np.uint64)
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    d_arena = torch.randint(0, 256, (int(lens.sum()),), dtype=torch.uint8, device="cuda", generator=g)
    out = m.bao.outboard_batch(ctx, d_arena, offsets, lens)
    torch.cuda.synchronize()
    first = torch.from_numpy(out["ob_first"][:-1].astype(np.int64)).cuda()
    hdr = out["outboards"][first[:, None] + torch.arange(8, device="cuda")[None, :]].cpu().numpy()
    assert np.array_equal(hdr.copy().view("<u8").reshape(-1), lens), "a header is not its file's length"
    roots = out["roots"].cpu().numpy().view(np.uint32)
    for f in rng.choice(n_files, 256, replace=False):
        a, ln = int(offsets[f]), int(lens[f])
        ob, root = m.bao.outboard(ctx, d_arena[a:a + ln].clone() if ln else b"")
        got_ob, _ = _slices(out, f)
        assert torch.equal(got_ob, ob), (f, ln)
        assert list(roots[f]) == list(root), (f, ln)
    ctx.close()


def test_large_files_in_a_batch():
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    g = torch.Generator(device="cuda")
    g.manual_seed(256)
    rng = np.random.default_rng(5)
    small = [int(rng.integers(1, 6)) * 1024 - int(rng.integers(0, 1024)) for _ in range(20)]      # 1 ... 5 chunks
    lens = small[:7] + [256 << 20] + small[7:15] + [(257 << 20) + 5] + small[15:]
    big = [7, 16]
    at, offsets = 0, []
    for f, ln in enumerate(lens):                                 # back to back; the first large file starts 16-byte aligned, the second does not
        at = (at + 15) // 16 * 16 if f == big[0] else at | 1 if f == big[1] else at
        offsets.append(at)
        at += ln
    offsets = np.array(offsets, dtype=np.uint64)
    d_arena = torch.randint(0, 256, (int(sum(lens)) + 16,), dtype=torch.uint8, device="cuda", generator=g)
    out = m.bao.outboard_batch(ctx, d_arena, offsets, lens)
    roots = out["roots"].cpu().numpy().view(np.uint32)
    for f in big:
        a = int(offsets[f])
        ob, root = m.bao.outboard(ctx, d_arena[a:a + lens[f]].clone())
        assert torch.equal(_slices(out, f)[0], ob) and list(roots[f]) == list(root), f
        del ob
    host = {f: d_arena[int(offsets[f]):int(offsets[f]) + lens[f]].cpu().numpy() for f in range(len(lens)) if f not in big}
    obs = out["outboards"].cpu().numpy()
    for f, data in host.items():
        want_ob, want_root = R.outboard(data.tobytes())
        assert obs[int(out["ob_first"][f]):int(out["ob_first"][f + 1])].tobytes() == want_ob and list(roots[f]) == want_root, f
    del out, d_arena, obs
    # past what one finishing workgroup takes: 1 026 tiles
    lens = [3000, (1 << 30) + (1 << 20) + 5, 1, 70 * 1024]
    offsets = np.array([0, 3008, 3008 + lens[1] + 3, 3008 + lens[1] + 16], dtype=np.uint64)
    d_arena = torch.randint(0, 256, (int(offsets[3]) + lens[3],), dtype=torch.uint8, device="cuda", generator=g)
    out = m.bao.outboard_batch(ctx, d_arena, offsets, lens)
    ob, root = m.bao.outboard(ctx, d_arena[3008:3008 + lens[1]])
    roots = out["roots"].cpu().numpy().view(np.uint32)
    assert torch.equal(_slices(out, 1)[0], ob) and list(roots[1]) == list(root)
    for f in (0, 2, 3):
        data = d_arena[int(offsets[f]):int(offsets[f]) + lens[f]].cpu().numpy().tobytes()
        want_ob, want_root = R.outboard(data)
        assert _slices(out, f)[0].cpu().numpy().tobytes() == want_ob and list(roots[f]) == want_root, f
    ctx.close()


PLAN_LENGTHS = [1, 700, 2048, 64 * 1024, 3 * 1024 + 5, 37 * 1024 + 64, 100 * 1024 + 77, 1 << 20, (2 << 20) + 7]


def _samples(m, lens, per_file, seed):
    """(files, chunks): per file `per_file` random chunks, its last chunk twice and chunk 0, interleaved over the files"""
    rng = np.random.default_rng(seed)
    files, chunks = [], []
    for f, ln in enumerate(lens):
        n = m.bao.num_chunks(ln)
        for c in list(rng.integers(0, n, per_file)) + [n - 1, 0, n - 1]:
            files.append(f)
            chunks.append(int(c))
    perm = rng.permutation(len(files))
    return np.array(files, dtype=np.uint32)[perm], np.array(chunks, dtype=np.uint64)[perm]


def test_planning_across_files():
    import torch
    m = T.pkg()
    ctx = m.Context("nova_bn254", 0)
    lens = PLAN_LENGTHS
    arena, offsets = _arena(lens, starts_odd=(1, 4), seed=5)
    d_arena = torch.from_numpy(arena).cuda()
    ob = m.bao.outboard_batch(ctx, d_arena, offsets, lens)
    files, chunks = _samples(m, lens, 19, 17)
    assert 190 <= files.size <= 210
    cb = m.bao.chunk_bytes_batch(arena, offsets, lens, files, chunks)
    assert torch.equal(cb, m.bao.chunk_bytes_batch(d_arena, offsets, lens, files, chunks))
    out = m.bao.plan_samples_batch(ctx, ob["outboards"], lens, ob["roots"], files, chunks, cb)
    rf = out["row_first"]
    assert list(rf) == list(m.bao.sample_rows_batch(lens, files, chunks)) and out["records"].shape[0] == int(rf[-1])
    assert (out["sample_status"] == 0).all()
    roots = ob["roots"].cpu().numpy().view(np.uint32)
    for f, ln in enumerate(lens):
        idx = np.nonzero(files == f)[0]
        ob_f, _ = _slices(ob, f)
        assert torch.equal(cb[torch.from_numpy(idx).cuda()], m.bao.chunk_bytes(_file(arena, offsets, lens, f), chunks[idx]))
        one = m.bao.plan_samples(ctx, ob_f, ln, roots[f], chunks[idx], cb[torch.from_numpy(idx).cuda()].contiguous())
        assert (one["sample_status"] == 0).all()
        for k, s in enumerate(idx):
            a, b = int(rf[s]), int(rf[s + 1])
            a1, b1 = int(one["row_first"][k]), int(one["row_first"][k + 1])
            assert b - a == b1 - a1 and torch.equal(out["records"][a:b], one["records"][a1:b1]), (f, s)
            assert bool(out["provable"][s]) == bool(one["provable"][k])
    # their witnesses
    recs = out["records"]
    k = recs.shape[0]
    d_b = torch.empty((k, ctx.body_bytes), dtype=torch.uint8, device="cuda")
    d_p = torch.zeros((k, 15), dtype=torch.int32, device="cuda")
    d_s = torch.full((k,), -1, dtype=torch.int32, device="cuda")
    ctx.run_device(recs.data_ptr(), k, d_b.data_ptr(), 0, d_p.data_ptr(), d_s.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (d_s.cpu().numpy() == 0).all()
    pub = d_p.cpu().numpy().view(np.uint32)
    assert out["provable"].sum() > files.size // 2
    for s in range(files.size):
        if out["provable"][s]:
            assert list(pub[int(rf[s + 1]) - 1][2:10]) == list(roots[files[s]]), s
    # argument errors, before anything is launched
    with pytest.raises(m.B3WError):
        m.bao.plan_samples_batch(ctx, ob["outboards"], lens, ob["roots"], [len(lens)], [0], cb[:1])
    with pytest.raises(m.B3WError):
        m.bao.plan_samples_batch(ctx, ob["outboards"], lens, ob["roots"], [1], [1], cb[:1])          # chunk 1 of 1
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    ln64 = np.array(lens, dtype=np.uint64)
    f1, c1 = np.array([len(lens)], dtype=np.uint32), np.array([0], dtype=np.uint64)
    assert m.lib().b3w_sample_plan_batch_device(ctx.handle, ln64.ctypes.data, ln64.size, ob["outboards"].data_ptr(), ob["roots"].data_ptr(),
                                                 f1.ctypes.data, c1.ctypes.data, 1, cb.data_ptr(), recs.data_ptr(), st.data_ptr(), 0) == m.B3W_E_BAD_ARGUMENT
    assert "file index" in ctx.last_error()
    assert m.lib().b3w_sample_plan_batch_device(ctx.handle, ln64.ctypes.data, ln64.size, ob["outboards"].data_ptr(), ob["roots"].data_ptr(),
                                                 f1.ctypes.data, c1.ctypes.data, 0, None, None, None, 0) == 0      # no samples: nothing
    comp = m.Context("compression", 0)
    with pytest.raises(m.B3WError):
        m.bao.plan_samples_batch(comp, ob["outboards"], lens, ob["roots"], files, chunks, cb)
    comp.close()
    ctx.close()


def test_tampering_stays_local():
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    lens = [37 * 1024 + 500, 21 * 1024, 9 * 1024 + 1, 4 * 1024 + 9]
    arena, offsets = _arena(lens, starts_odd=(1,), seed=9)
    ob = m.bao.outboard_batch(ctx, torch.from_numpy(arena).cuda(), offsets, lens)
    n = [m.bao.num_chunks(x) for x in lens]
    files = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 1, 3, 3], dtype=np.uint32)
    chunks = np.array([0, 3, 8, 17, 20, 0, n[0] - 1, 3, 4, 11, 2, 4], dtype=np.uint64)
    good = m.bao.chunk_bytes_batch(arena, offsets, lens, files, chunks)
    obs, roots = ob["outboards"], ob["roots"]

    def plan(obs_t=obs, cb=good, roots_t=roots):
        out = m.bao.plan_samples_batch(ctx, obs_t, lens, roots_t, files, chunks, cb)
        return list(out["sample_status"]), out["records"]
    st0, recs0 = plan()
    assert st0 == [0] * 12
    rf = m.bao.sample_rows_batch(lens, files, chunks)

    def untouched_equal(recs, touched):
        for s in range(files.size):
            if s not in touched:
                assert torch.equal(recs[int(rf[s]):int(rf[s + 1])], recs0[int(rf[s]):int(rf[s + 1])]), s
    # a flipped chunk byte of sample 3 (file 0, chunk 17)
    cb = good.clone()
    cb[3, 100] ^= 1
    st, recs = plan(cb=cb)
    assert st == [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    untouched_equal(recs, {3})
    # a flipped byte in a node of file 1 that lies on chunk 20's path alone among the sampled chunks of file 1
    path20 = m.bao.path_nodes(20, n[1])
    others = set(m.bao.path_nodes(3, n[1])) | set(m.bao.path_nodes(11, n[1]))
    node = path20[-1]
    assert node not in others
    bad = obs.clone()
    bad[int(ob["ob_first"][1]) + 8 + 64 * node + 3] ^= 1
    st, recs = plan(obs_t=bad)
    assert st == [0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0]
    untouched_equal(recs, {4})
    # a flipped root word of file 2: its three samples, no other
    wrong = roots.clone()
    wrong[2, 4] ^= 1
    st, recs = plan(roots_t=wrong)
    assert st == [0, 0, 2, 0, 0, 2, 0, 0, 2, 0, 0, 0]
    untouched_equal(recs, set())                                  # (the records do not depend on the root)
    # a wrong header of file 3
    bad = obs.clone()
    bad[int(ob["ob_first"][3])] ^= 1
    st, recs = plan(obs_t=bad)
    assert st == [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 3]
    untouched_equal(recs, set())
    # all four at once: the named samples get 1 (chunk), 2 (node), 2 (root), 3 (header), every other sample of every file 0
    bad[int(ob["ob_first"][1]) + 8 + 64 * node + 3] ^= 1
    st, recs = plan(obs_t=bad, cb=cb, roots_t=wrong)
    assert st == [0, 0, 2, 1, 2, 2, 0, 0, 2, 0, 3, 3]
    untouched_equal(recs, {3, 4})
    ctx.close()


def test_prove_samples_batch_equals_prove_samples_per_file():
    import torch
    import ec_ref as E
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    lens = [11 * 1024 + 33, 5 * 1024, 700]
    arena, offsets = _arena(lens, seed=2)
    ob = m.bao.outboard_batch(ctx, torch.from_numpy(arena).cuda(), offsets, lens)
    files = np.array([0, 1, 0, 2, 1, 0], dtype=np.uint32)
    chunks = np.array([3, 4, 10, 0, 0, 3], dtype=np.uint64)
    cb = m.bao.chunk_bytes_batch(arena, offsets, lens, files, chunks)
    roots = ob["roots"].cpu().numpy().view(np.uint32)
    key = m.CommitKey(ctx, "pallas", E.points_to_bytes(E.random_points("pallas", ctx.witness_size)), window=12)
    res = m.bao.prove_samples_batch(ctx, ob["outboards"], lens, ob["roots"], files, chunks, cb, batch_steps=16, commit_key=key)
    seen = []
    r1cs = m.R1cs(ctx)
    res2 = m.bao.prove_samples_batch(ctx, ob["outboards"], lens, ob["roots"], files, chunks, cb, batch_steps=7, r1cs=r1cs,
                                     consumer=lambda bodies, pitch, first_row, count: seen.append((first_row, count)))
    rows = res["records"].shape[0]
    assert sorted(seen) == [(r, min(7, rows - r)) for r in range(0, rows, 7)]
    assert (res["status"] == 0).all().item() and (res2["status"] == 0).all().item() and (res2["violations"] == 0).all().item()
    rf = res["row_first"]
    for f, ln in enumerate(lens):
        idx = np.nonzero(files == f)[0]
        sel = torch.from_numpy(idx).cuda()
        one = m.bao.prove_samples(ctx, _slices(ob, f)[0], ln, roots[f], chunks[idx], cb[sel].contiguous(), batch_steps=16, commit_key=key)
        two = m.bao.prove_samples(ctx, _slices(ob, f)[0], ln, roots[f], chunks[idx], cb[sel].contiguous(), batch_steps=7, consumer=lambda *a: None)
        for k, s in enumerate(idx):
            a, b = int(rf[s]), int(rf[s + 1])
            a1, b1 = int(one["row_first"][k]), int(one["row_first"][k + 1])
            assert torch.equal(res["points"][a:b], one["points"][a1:b1]), (f, s)
            assert torch.equal(res["public"][a:b], one["public"][a1:b1]), (f, s)
            assert torch.equal(res2["public"][a:b], two["public"][a1:b1]), (f, s)
    key.close()
    r1cs.close()
    ctx.close()


def test_it_is_a_batch():
    """4 096 files of 16 KiB: the batch call against the route the library offered before it, a loop of b3w_bao_outboard_device"""
    import torch
    m = T.pkg()
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    n_files, ln = 4096, 16 * 1024
    lens = np.full(n_files, ln, dtype=np.uint64)
    offsets = (np.arange(n_files, dtype=np.uint64) * ln)
    g = torch.Generator(device="cuda")
    g.manual_seed(16)
    d_arena = torch.randint(0, 256, (n_files * ln,), dtype=torch.uint8, device="cuda", generator=g)
    ob_first = m.bao.batch_layout(lens)
    d_obs = torch.empty(int(ob_first[-1]), dtype=torch.uint8, device="cuda")
    d_roots = torch.empty((n_files, 8), dtype=torch.int32, device="cuda")
    need = L.b3w_bao_batch_scratch_bytes(lens.ctypes.data, n_files)
    d_scratch = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    d_obs1 = torch.empty_like(d_obs)
    d_roots1 = torch.empty_like(d_roots)
    d_levels = torch.empty((2 * 16 + 64) * 8, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    base, obs1, roots1, lev = d_arena.data_ptr(), d_obs1.data_ptr(), d_roots1.data_ptr(), d_levels.data_ptr()
    firsts = [int(x) for x in ob_first]

    def batch():
        t = time.perf_counter()
        rc = L.b3w_bao_outboard_batch_device(ctx.handle, base, offsets.ctypes.data, lens.ctypes.data, n_files, d_obs.data_ptr(), d_roots.data_ptr(),
                                             d_scratch.data_ptr(), need, stream)
        torch.cuda.synchronize()
        assert rc == 0
        return time.perf_counter() - t

    def loop():
        t = time.perf_counter()
        for f in range(n_files):
            rc = L.b3w_bao_outboard_device(ctx.handle, base + f * ln, ln, obs1 + firsts[f], lev, roots1 + 32 * f, stream)
            assert rc == 0
        torch.cuda.synchronize()
        return time.perf_counter() - t
    for _ in range(3):
        batch()
        loop()
    assert torch.equal(d_obs, d_obs1) and torch.equal(d_roots, d_roots1)
    t_batch = statistics.median(batch() for _ in range(5))
    t_loop = statistics.median(loop() for _ in range(5))
    print(f"4096 x 16 KiB: batch {t_batch * 1e3:.3f} ms, loop of single-file calls {t_loop * 1e3:.3f} ms, ratio {t_loop / t_batch:.1f}")
    assert t_batch < t_loop
    ctx.close()
