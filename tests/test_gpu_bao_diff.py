"""The outboard diff on the device (bao.outboard_diff; b3w_bao_outboard_diff_device) against the host mirror (bao.diff_host), the
restatement in tests/bao_diff_ref.py and what the bytes say.
  parity        one call over every pair of test_bao_diff_cpu.cases(): the versions lie in one arena at odd offsets, their outboards are
                outboard_batch's / outboard_groups_batch's moved to 8-byte-aligned places of the test's own between 0xA5 guards; the two
                sides in two buffers, and (equal group_logs) in one; a base is paired with its four versions
  positions     fabricated outboards of 2^20 + 5 chunks (random bytes: nothing is hashed) that differ in a few thousand stored halves,
                among them the first and last chunk's and those on both sides of tile boundaries, as full outboards, as group outboards
                of 64 chunks and one of each; and 1 025 against 2^20 + 5 chunks; against the numpy restatement
  closed loops  a replica with a stale copy ends with the provider's bytes and outboards byte for byte: equal lengths (diff, have_runs,
                set_slices_arena, ingest_set_slices with d_have = the diff), changed lengths (outboard_resize_batch over what the replica
                holds first)
  refusals      every one b3wit.h lists, with every output byte unchanged"""
import functools

import numpy as np
import pytest

import b3w_testlib as T
import bao_diff_ref as D
import bao_have_ref as H
from test_bao_diff_cpu import cases

pytestmark = pytest.mark.gpu

K = 1024
GUARD = 4096
FILL, WALL = 0xEE, 0xA5
GS = [0, 1, 4, 6]
BAD = 100
BIG = (1 << 20) + 5


@functools.lru_cache(maxsize=None)
def _setup():
    """every version of the CPU test's cases once in one arena, the outboards of the arena at every g, the pairs as (file of a, file of b)"""
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    index, versions, pairs = {}, [], []
    for _, a, b in cases():
        for v in (a, b):
            if id(v) not in index:
                index[id(v)] = len(versions)
                versions.append(v)
        pairs.append((index[id(a)], index[id(b)]))
    offsets, at = [], 3
    for f, v in enumerate(versions):
        at = (at + 48 + 15) // 16 * 16 + (5 * f + 1) % 16
        offsets.append(at)
        at += v.size
    arena = np.random.default_rng(40).integers(0, 256, at + 64, dtype=np.uint8)
    for o, v in zip(offsets, versions):
        arena[o:o + v.size] = v
    lens = np.array([v.size for v in versions], dtype=np.uint64)
    offsets = np.array(offsets, dtype=np.uint64)
    assert {int(o) % 16 for o in offsets} >= {1, 4, 8, 11}
    d_arena = torch.from_numpy(arena).cuda()
    made = {0: m.bao.outboard_batch(ctx, d_arena, offsets, lens)}
    for g in GS[1:]:
        made[g] = m.bao.outboard_groups_batch(ctx, d_arena, offsets, lens, g)
    torch.cuda.synchronize()
    host = {g: made[g]["outboards"].cpu().numpy() for g in GS}
    roots = made[0]["roots"].cpu().numpy().view(np.uint32)
    return dict(m=m, ctx=ctx, versions=versions, pairs=pairs, lens=lens, made=made, host=host, roots=roots, truth={})


@pytest.fixture(scope="module", autouse=True)
def _a_memory_pool_of_its_own():
    """every device tensor of this module comes from a pool of the allocator that is the module's own and goes with it: the modules
    behind this one that measure device memory find the default pool's cached blocks as they would without this one"""
    import gc
    import torch
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        torch.cuda.synchronize()
        if _setup.cache_info().currsize:
            _setup()["ctx"].close()
        _setup.cache_clear()
        _placed.cache_clear()
        gc.collect()
    del pool


def _walled(size):
    """-> (the whole tensor, its middle `size` bytes): 0xEE between 0xA5 guards (the guards keep the middle's alignment)"""
    import torch
    whole = torch.full((size + 2 * GUARD,), WALL, dtype=torch.uint8, device="cuda")
    whole[GUARD:GUARD + size] = FILL
    return whole, whole[GUARD:GUARD + size]


def _walls_intact(whole, size):
    return bool((whole[:GUARD] == WALL).all().item()) and bool((whole[GUARD + size:] == WALL).all().item())


def _walled_words(words):
    import torch
    whole, mid = _walled(8 * words)
    return whole, mid.view(torch.int64)


def _host_words(t):
    return t.cpu().numpy().view(np.uint64)


def _file_ob(s, g, f):
    a, b = int(s["made"][g]["ob_first"][f]), int(s["made"][g]["ob_first"][f + 1])
    return s["host"][g][a:b]


@functools.lru_cache(maxsize=None)
def _placed(g, phase):
    """the outboards of group_log g at places that are not the batch layout's: 8-byte aligned, one to three words of 0xA5 between them
    -> (the device buffer, the places: numpy uint64 [n_files], the host copy)"""
    import torch
    s = _setup()
    n = len(s["versions"])
    places, at = [], 8 * (phase + 1)
    for f in range(n):
        places.append(at)
        at += _file_ob(s, g, f).size + 8 * (1 + (f + phase) % 3)
    buf = np.full(at + 8, WALL, dtype=np.uint8)
    for f in range(n):
        ob = _file_ob(s, g, f)
        buf[places[f]:places[f] + ob.size] = ob
    places = np.array(places, dtype=np.uint64)
    assert not (places % 8).any() and (places % 16 == 8).any() and (places % 16 == 0).any()
    assert (places != s["made"][g]["ob_first"][:-1]).all()
    return torch.from_numpy(buf).cuda(), places, buf


def _truth(s, i, G):
    if (i, G) not in s["truth"]:
        fa, fb = s["pairs"][i]
        s["truth"][(i, G)] = H.pack(D.truth(s["versions"][fa], s["versions"][fb], G))
    return s["truth"][(i, G)]


@pytest.mark.parametrize("ga,gb", [(0, 0), (4, 4), (6, 6), (0, 4), (4, 0), (1, 6), (6, 1), (1, 0)])
def test_one_call_over_the_cpu_tests_pairs_is_the_host_mirror_and_the_bytes(ga, gb):
    import torch
    s = _setup()
    m = s["m"]
    G = max(ga, gb)
    order = np.random.default_rng(100 + 8 * ga + gb).permutation(len(s["pairs"]))
    pa = np.array([s["pairs"][i][0] for i in order], dtype=np.uint32)
    pb = np.array([s["pairs"][i][1] for i in order], dtype=np.uint32)
    assert len(order) >= 36 and np.bincount(pa).max() >= 4, "a few dozen pairs, a base paired with several versions"
    host, true = [], []
    for i, fa, fb in zip(order.tolist(), pa.tolist(), pb.tolist()):
        host.append(m.bao.diff_host(_file_ob(s, ga, fa).tobytes(), int(s["lens"][fa]), s["roots"][fa], _file_ob(s, gb, fb).tobytes(), int(s["lens"][fb]),
                                    s["roots"][fb], ga, gb))
        true.append(_truth(s, i, G))
    host, true = np.concatenate(host), np.concatenate(true)
    assert (host == true).all(), "the host mirror is not what the bytes say"
    assert true.any() and (true == 0).any()
    sides = [(_placed(ga, 0), _placed(gb, 1))]
    if ga == gb:
        sides.append((_placed(ga, 0), _placed(ga, 0)))                        # both sides in one buffer
    roots = s["made"][0]["roots"]
    for (d_a, at_a, host_a), (d_b, at_b, host_b) in sides:
        whole, d_same = _walled_words(host.size)
        out = m.bao.outboard_diff(s["ctx"], s["lens"], d_a, roots, s["lens"], d_b, roots, pa, pb, ga, gb, at_a, at_b, d_same=d_same)
        torch.cuda.synchronize()
        assert out["same"] is d_same and (out["pair_lens"] == s["lens"][pb]).all()
        assert [int(x) for x in out["word_first"]] == H.layout(out["pair_lens"].tolist()) and int(out["word_first"][-1]) == host.size
        got = _host_words(d_same)
        assert (got == host).all(), (ga, gb, "not the host mirror's words", np.flatnonzero(got != host)[:8])
        assert _walls_intact(whole, 8 * host.size)
        assert (d_a.cpu().numpy() == host_a).all() and (d_b.cpu().numpy() == host_b).all(), "an outboard or a guard between them was written"
    made = m.bao.outboard_diff(s["ctx"], s["lens"], d_a, roots, s["lens"], d_b, roots, pa, pb, ga, gb, at_a, at_b)      # (a tensor of its own when none is given)
    assert made["same"].dtype == torch.int64 and (_host_words(made["same"]) == host).all()
    print(f"group_logs {ga}, {gb}: {len(order)} pairs, {host.size} words, {int(np.unpackbits(host.view(np.uint8)).sum())} chunks same")


def test_no_pair_lists_pair_file_i_with_file_i_in_the_batch_layout():
    """the defaults: no pair lists, no places (the batch layout of each side's lens), two sides of their own"""
    import torch
    s = _setup()
    m = s["m"]
    same_len = [(fa, fb) for fa, fb in s["pairs"] if s["lens"][fa] == s["lens"][fb]][1::3]
    fa = np.array([p[0] for p in same_len])
    fb = np.array([p[1] for p in same_len])
    for g in (0, 4):
        sides = []
        for files in (fa, fb):
            lens = s["lens"][files]
            obs = np.concatenate([_file_ob(s, g, int(f)) for f in files])
            sides.append((lens, torch.from_numpy(obs).cuda(), s["made"][0]["roots"][torch.from_numpy(files).cuda()].contiguous()))
        out = m.bao.outboard_diff(s["ctx"], *sides[0], *sides[1], group_log_a=g, group_log_b=g)
        want = np.concatenate([_truth(s, s["pairs"].index(p), g) for p in same_len])
        assert (_host_words(out["same"]) == want).all() and (out["pair_lens"] == sides[1][0]).all()


# ---- positions --------------------------------------------------------------------------------------------------------------------
def _copy_halves(dst, dst_at, src, src_at, units):
    cols = np.arange(32, dtype=np.int64)
    dst[dst_at[units][:, None] + cols] = src[src_at[units][:, None] + cols]


def test_the_places_of_a_million_chunks():
    import torch
    s = _setup()
    m = s["m"]
    rng = np.random.default_rng(50)
    n, small = BIG, 1025
    size0, size6, size_s = 8 + 64 * (n - 1), 8 + 64 * (D.GR.num_groups(n, 6) - 1), 8 + 64 * (small - 1)
    at0, at6 = D.places_np(n, 0, 0), D.places_np(n, 6, 6)
    ob_a = rng.integers(0, 256, size0, dtype=np.uint8)
    # b: a copy with a few thousand halves changed - as a full outboard and as a group outboard of 64 chunks
    ob_b = ob_a.copy()
    edges = [0, 1, n - 1, n - 2, n - 5, n - 6, 1 << 20, (1 << 20) - 1] + [t * 1024 + d for t in (1, 2, 512, 1023) for d in (-1, 0)]
    changed = np.unique(np.concatenate([np.array(edges), rng.integers(0, n, 3000)]))
    ob_b[at0[changed] + rng.integers(0, 32, changed.size)] ^= 1
    units6 = np.unique(np.concatenate([np.array([0, 15, 16, at6.size - 1, at6.size - 2]), rng.integers(0, at6.size, 300)]))
    ob_b[at6[units6] + rng.integers(0, 32, units6.size)] ^= 0x80
    # c: a group outboard of 64 chunks that shares a's CVs of that level but for every seventh unit, the first and the last
    ob_c = rng.integers(0, 256, size6, dtype=np.uint8)
    shared = np.array([u for u in range(at6.size) if u % 7 and u not in (0, at6.size - 1)])
    _copy_halves(ob_c, at6, ob_a, D.places_np(n, 0, 6), shared)
    # s: a file of 1 025 chunks that shares a few chunks' CVs with a
    ob_s = rng.integers(0, 256, size_s, dtype=np.uint8)
    _copy_halves(ob_s, D.places_np(small, 0, 0), ob_a, at0, np.array([0, 5, 600, 1023, 1024]))
    parts, places, at = [ob_a, ob_b, ob_s, ob_c], [], 8
    for p in parts:
        places.append(at)
        at += p.size + 24
    buf = np.full(at, WALL, dtype=np.uint8)
    for p, o in zip(parts, places):
        buf[o:o + p.size] = p
    d_buf = torch.from_numpy(buf).cuda()
    places = np.array(places, dtype=np.uint64)
    lens = np.array([n * K - 3, n * K - 3, small * K, n * K - 3], dtype=np.uint64)
    d_roots = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, (4, 8), dtype=np.int64).astype(np.int32)).cuda()
    runs = [(0, 0, [(0, 1), (2, 0)], [D.same_chunks_np(ob_a, n, 0, ob_b, n, 0), D.same_chunks_np(ob_s, small, 0, ob_a, n, 0)]),
            (6, 6, [(0, 1), (2, 0)], [D.same_chunks_np(ob_a, n, 6, ob_b, n, 6), D.same_chunks_np(ob_s, small, 6, ob_a, n, 6)]),
            (0, 6, [(0, 3)], [D.same_chunks_np(ob_a, n, 0, ob_c, n, 6)]),
            (6, 0, [(3, 0)], [D.same_chunks_np(ob_c, n, 6, ob_a, n, 0)])]
    differs = ~runs[0][3][0]                                                    # (a change made for the level of 64 may hit a chunk's half too)
    assert differs[changed].all() and changed.size <= int(differs.sum()) <= changed.size + units6.size
    assert np.flatnonzero(runs[0][3][1]).tolist() == [0, 5, 600, 1023, 1024]
    unit_shared = np.zeros(at6.size, bool)
    unit_shared[shared] = True
    assert (runs[2][3][0] == np.repeat(unit_shared, 64)[:n]).all() and (runs[3][3][0] == runs[2][3][0]).all()
    for ga, gb, pairs, want in runs:
        pa, pb = np.array([p[0] for p in pairs], dtype=np.uint32), np.array([p[1] for p in pairs], dtype=np.uint32)
        want = np.concatenate([H.pack(w) for w in want])
        whole, d_same = _walled_words(want.size)
        m.bao.outboard_diff(s["ctx"], lens, d_buf, d_roots, lens, d_buf, d_roots, pa, pb, ga, gb, places, places, d_same=d_same)
        got = _host_words(d_same)
        assert (got == want).all(), (ga, gb, np.flatnonzero(got != want)[:8])
        assert _walls_intact(whole, 8 * want.size) and want.any() and (want != np.uint64(2 ** 64 - 1)).any()
    assert (d_buf.cpu().numpy() == buf).all()


# ---- the closed loops ---------------------------------------------------------------------------------------------------------------
def _rewrite(arena, offset, length, chunks, rng):
    for c in chunks:
        a, b = c * K, min(length, (c + 1) * K)
        arena[offset + a:offset + b] = rng.integers(0, 256, b - a, dtype=np.uint8)
        arena[offset + a] ^= 0xFF                                                # (never the bytes that were there)


def _sync(s, g, d_replica, d_provider, offsets, lens, replica_obs, replica_roots):
    """recipe one, from the replica's outboards of what it holds at these lengths -> the number of chunks fetched"""
    import torch
    m, ctx = s["m"], s["ctx"]
    make = (lambda d: m.bao.outboard_batch(ctx, d, offsets, lens)) if g == 0 else (lambda d: m.bao.outboard_groups_batch(ctx, d, offsets, lens, g))
    provider = make(d_provider)
    diff = m.bao.outboard_diff(ctx, lens, replica_obs, replica_roots, lens, provider["outboards"], provider["roots"], group_log_a=g, group_log_b=g)
    assert (diff["pair_lens"] == lens).all()
    missing = m.bao.have_runs(ctx, diff["same"], diff["pair_lens"], "missing")
    fetched = int(missing["n_chunks"].sum())
    assert 0 < fetched < sum(H.num_chunks(int(x)) for x in lens)
    sl = m.bao.set_slices_arena(ctx, d_provider, offsets, lens, provider["outboards"], missing["files"], missing["first_chunks"], missing["n_chunks"], group_log=g)
    res = m.bao.ingest_set_slices(ctx, d_replica, offsets, lens, replica_obs, provider["roots"], missing["files"], missing["first_chunks"], missing["n_chunks"],
                                  sl["slices"], group_log=g, d_have=diff["same"])
    assert not res["set_status"].any().item() and not res["chunk_status"].any().item()
    assert torch.equal(d_replica, d_provider), "the replica's arena is not the provider's"
    assert torch.equal(replica_obs, provider["outboards"]), "the replica's outboards are not the provider's"
    after = m.bao.have_runs(ctx, diff["same"], lens, "missing")
    assert int(after["n_runs"].item()) == 0 and after["file_have"].cpu().tolist() == [H.num_chunks(int(x)) for x in lens]
    assert (_host_words(diff["same"]) == np.concatenate([H.pack(np.ones(H.num_chunks(int(x)), bool)) for x in lens])).all()
    ver = m.bao.verify_batch(ctx, d_replica, offsets, lens, replica_obs, provider["roots"], group_log=g)
    assert not ver["unit_status"].any().item() and not ver["file_status"].any().item()
    return fetched


@pytest.mark.parametrize("g", [0, 4])
def test_a_stale_replica_of_equal_lengths_ends_with_the_providers_bytes(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    rng = np.random.default_rng(60 + g)
    n_of = [5, 65, 1025, 2049]
    lens = np.array([n * K - 300 for n in n_of], dtype=np.uint64)
    offsets, at = [], 1
    for f, ln in enumerate(lens.tolist()):
        at = (at + 15) // 16 * 16 + 2 * f + 1
        offsets.append(at)
        at += ln + 40
    offsets = np.array(offsets, dtype=np.uint64)
    old = rng.integers(0, 256, at, dtype=np.uint8)
    new = old.copy()
    rewritten = 0
    for o, ln, n in zip(offsets.tolist(), lens.tolist(), n_of):
        chunks = np.unique(np.concatenate([rng.permutation(n)[:max(1, n // 10)], [n - 1] if n > 1000 else []])).astype(np.int64).tolist()
        _rewrite(new, o, ln, chunks, rng)
        rewritten += len(chunks)
    d_replica, d_provider = torch.from_numpy(old).cuda(), torch.from_numpy(new).cuda()
    mine = m.bao.outboard_batch(ctx, d_replica, offsets, lens) if g == 0 else m.bao.outboard_groups_batch(ctx, d_replica, offsets, lens, g)
    fetched = _sync(s, g, d_replica, d_provider, offsets, lens, mine["outboards"], mine["roots"])
    assert fetched == rewritten if g == 0 else rewritten <= fetched <= 16 * rewritten
    print(f"group_log {g}: {rewritten} chunks of {sum(n_of)} rewritten, {fetched} fetched")


@pytest.mark.parametrize("g", [0, 4])
def test_a_stale_replica_of_other_lengths_resizes_what_it_holds_first(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    rng = np.random.default_rng(70 + g)
    old_lens = np.array([1000 * K - 17, 70 * K], dtype=np.uint64)               # grown across the tile of 1 024 chunks; shrunk
    new_lens = np.array([1100 * K + 5, 40 * K - 500], dtype=np.uint64)
    offsets = np.array([7, 7 + 1100 * K + 64 + 2], dtype=np.uint64)
    size = int(offsets[1]) + 70 * K + 64
    old = rng.integers(0, 256, size, dtype=np.uint8)                            # (behind a file's old end: whatever lies there)
    new = old.copy()
    for o, lo, ln in zip(offsets.tolist(), old_lens.tolist(), new_lens.tolist()):
        if ln > lo:
            new[o + lo:o + ln] = rng.integers(0, 256, ln - lo, dtype=np.uint8)
        n = H.num_chunks(min(lo, ln))
        _rewrite(new, o, ln, rng.permutation(n)[:n // 10].tolist(), rng)
    d_replica, d_provider = torch.from_numpy(old).cuda(), torch.from_numpy(new).cuda()
    make = (lambda d, lens: m.bao.outboard_batch(ctx, d, offsets, lens)) if g == 0 else (lambda d, lens: m.bao.outboard_groups_batch(ctx, d, offsets, lens, g))
    stale = make(d_replica, old_lens)
    new_first = m.bao.group_batch_layout(new_lens, g)
    resized = torch.full((int(new_first[-1]),), FILL, dtype=torch.uint8, device="cuda")
    roots = stale["roots"].clone()
    m.bao.outboard_resize_batch(ctx, d_replica, offsets, old_lens, new_lens, stale["outboards"], stale["ob_first"], resized, new_first, roots, [0, 1], group_log=g)
    fetched = _sync(s, g, d_replica, d_provider, offsets, new_lens, resized, roots)
    assert fetched >= 100 + 100 + 4                                              # the grown tail, a tenth of what was kept
    print(f"group_log {g}: {fetched} chunks fetched of {sum(H.num_chunks(int(x)) for x in new_lens)}")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_output_untouched():
    import torch
    s = _setup()
    m = s["m"]
    L = m.lib()
    ctx = s["ctx"]
    stream = torch.cuda.current_stream().cuda_stream
    of = {n: [f for f in range(len(s["versions"])) if H.num_chunks(int(s["lens"][f])) == n] for n in (3, 65)}
    pick = [of[3][0], of[65][0], of[65][1]]
    lens = s["lens"][pick].copy()
    obs = [_file_ob(s, 0, f) for f in pick]
    first = np.cumsum([0] + [o.size for o in obs]).astype(np.uint64)
    d_obs = torch.from_numpy(np.concatenate(obs + [np.zeros(16, dtype=np.uint8)])).cuda()
    d_roots = torch.from_numpy(np.concatenate([s["roots"][f] for f in pick] + [np.zeros(4, dtype=np.uint32)]).view(np.int32)).cuda()
    pa, pb = np.array([0, 1, 2, 0], dtype=np.uint32), np.array([1, 0, 2, 2], dtype=np.uint32)
    word_first = m.bao.have_layout(lens[pb])
    words = int(word_first[-1])
    whole, d_same = _walled_words(words)
    good = dict(ctx=ctx.handle, la=lens.ctypes.data, fa=first.ctypes.data, oa=d_obs.data_ptr(), ba=int(first[-1]), ra=d_roots.data_ptr(), na=3, ga=0,
                lb=lens.ctypes.data, fb=first.ctypes.data, ob=d_obs.data_ptr(), bb=int(first[-1]), rb=d_roots.data_ptr(), nb=3, gb=0,
                pa=pa.ctypes.data, pb=pb.ctypes.data, n=4, wf=word_first.ctypes.data, same=d_same.data_ptr())

    def call(**change):
        kw = dict(good)
        kw.update(change)
        rc = L.b3w_bao_outboard_diff_device(kw["ctx"], kw["la"], kw["fa"], kw["oa"], kw["ba"], kw["ra"], kw["na"], kw["ga"], kw["lb"], kw["fb"], kw["ob"], kw["bb"],
                                            kw["rb"], kw["nb"], kw["gb"], kw["pa"], kw["pb"], kw["n"], kw["wf"], kw["same"], stream)
        torch.cuda.synchronize()
        return rc

    def untouched():
        return bool((d_same.view(torch.uint8) == FILL).all().item()) and _walls_intact(whole, 8 * words)
    bad_first = first.copy()
    bad_first[1] += 4                                                            # an outboard's place that is not 8-byte aligned
    far_first = first.copy()
    far_first[2] += 8                                                            # the last outboard reaches 8 bytes past the buffer
    bad_pair = np.array([0, 1, 3, 0], dtype=np.uint32)
    long_lens = lens.copy()
    long_lens[1] = ((1 << 30) + 1) * K
    wf_mid, wf_end = word_first.copy(), word_first.copy()
    wf_mid[2] += 1
    wf_end[-1] += 1
    refusals = [dict(ctx=None)] + [{k: None} for k in ("la", "fa", "oa", "ra", "lb", "fb", "ob", "rb", "pa", "pb", "wf", "same")] + \
        [dict(oa=good["oa"] + 4), dict(ob=good["ob"] + 4), dict(ra=good["ra"] + 2), dict(rb=good["rb"] + 2), dict(same=good["same"] + 4),
         dict(fa=bad_first.ctypes.data), dict(fb=bad_first.ctypes.data), dict(ga=7), dict(gb=7), dict(pa=bad_pair.ctypes.data), dict(pb=bad_pair.ctypes.data),
         dict(na=2), dict(nb=2), dict(la=long_lens.ctypes.data, ba=1 << 40), dict(lb=long_lens.ctypes.data, bb=1 << 40), dict(ba=good["ba"] - 1),
         dict(bb=good["bb"] - 1), dict(fa=far_first.ctypes.data), dict(fb=far_first.ctypes.data), dict(wf=wf_mid.ctypes.data), dict(wf=wf_end.ctypes.data)]
    for change in refusals:
        assert call(**change) == BAD and untouched(), change
        if change.get("ctx", 1) is not None:
            assert "bao outboard diff" in ctx.last_error(), change
    # more than 2^26 words: five files of 2^30 chunks (nothing is read before the refusal)
    huge = np.full(5, (1 << 30) * K, dtype=np.uint64)
    zeros, five = np.zeros(5, dtype=np.uint64), np.arange(5, dtype=np.uint32)
    wf = m.bao.have_layout(huge)
    assert int(wf[-1]) == 5 << 24
    assert call(la=huge.ctypes.data, lb=huge.ctypes.data, fa=zeros.ctypes.data, fb=zeros.ctypes.data, ba=1 << 40, bb=1 << 40, na=5, nb=5, pa=five.ctypes.data,
                pb=five.ctypes.data, n=5, wf=wf.ctypes.data) == BAD and untouched()
    assert "2^26" in ctx.last_error()
    # the wrapper's own
    for kw in (dict(pairs_a=[0]), dict(pairs_a=[0, 1], pairs_b=[0]), dict(pairs_a=[3], pairs_b=[0]), dict(group_log_a=7), dict(d_same=d_same[:1]),
               dict(d_same=d_same.to(torch.int32))):
        with pytest.raises(m.B3WError):
            m.bao.outboard_diff(ctx, lens, d_obs, d_roots, lens, d_obs, d_roots, **kw)
    assert untouched()
    # no pairs: a no-op, whatever else is passed
    assert call(n=0, la=None, fa=None, oa=None, ra=None, lb=None, fb=None, ob=None, rb=None, pa=None, pb=None, wf=None, same=None) == 0 and untouched()
    # the good arguments are taken, and the place of a file that is in no pair is never read
    only = dict(pa=np.array([0, 0], dtype=np.uint32), pb=np.array([1, 0], dtype=np.uint32))
    wild = first.copy()
    wild[2] = (1 << 60) + 3
    wf2 = m.bao.have_layout(lens[only["pb"]])
    assert call(fa=wild.ctypes.data, fb=wild.ctypes.data, pa=only["pa"].ctypes.data, pb=only["pb"].ctypes.data, n=2, wf=wf2.ctypes.data) == 0, ctx.last_error()
    d_same.view(torch.uint8).fill_(FILL)
    assert call() == 0, ctx.last_error()
    want = np.concatenate([m.bao.diff_host(obs[a].tobytes(), int(lens[a]), s["roots"][pick[a]], obs[b].tobytes(), int(lens[b]), s["roots"][pick[b]])
                           for a, b in zip(pa.tolist(), pb.tolist())])
    assert (_host_words(d_same) == want).all() and _walls_intact(whole, 8 * words)


def test_the_call_allocates_nothing():
    import torch
    s = _setup()
    m = s["m"]
    L = m.lib()
    ctx = s["ctx"]
    stream = torch.cuda.current_stream().cuda_stream
    d_obs, places, _ = _placed(0, 0)
    lens = s["lens"]
    pa = np.array([p[0] for p in s["pairs"]], dtype=np.uint32)
    pb = np.array([p[1] for p in s["pairs"]], dtype=np.uint32)
    word_first = m.bao.have_layout(lens[pb])
    d_same = torch.empty(int(word_first[-1]), dtype=torch.int64, device="cuda")
    roots = s["made"][0]["roots"]

    def once():
        assert L.b3w_bao_outboard_diff_device(ctx.handle, lens.ctypes.data, places.ctypes.data, d_obs.data_ptr(), d_obs.numel(), roots.data_ptr(), lens.size, 0,
                                              lens.ctypes.data, places.ctypes.data, d_obs.data_ptr(), d_obs.numel(), roots.data_ptr(), lens.size, 0,
                                              pa.ctypes.data, pb.ctypes.data, pa.size, word_first.ctypes.data, d_same.data_ptr(), stream) == 0, ctx.last_error()
        torch.cuda.synchronize()
    once()                                                                    # (the context's staging grows here, outside the allocator)
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    once()
    assert torch.cuda.max_memory_allocated() == before
    assert (_host_words(d_same) == np.concatenate([_truth(s, i, 0) for i in range(len(s["pairs"]))])).all()
