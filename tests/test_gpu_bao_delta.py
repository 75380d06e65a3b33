"""Outboard deltas on the device (bao.outboard_delta / apply_outboard_delta / outboard_check; b3w_bao_outboard_delta_device /
_apply_device) against the host mirrors, the restatement in tests/bao_delta_ref.py and the provider's own outboards.
  batch         one call over every pair of test_bao_delta_cpu.cases(g): outboards and outputs at odd 8-byte-aligned places with 0xA5
                between them, the blobs in extents of the test's own (some one node short: the capacity rule) between 0xA5 walls
  places        real outboards of 2^16 + 5 chunks with a few hundred chunks rewritten (delta, apply, byte equality with the provider's
                outboard); fabricated outboards of 2^20 + 5 units for the provider's bitmap and ranks alone, against the numpy form
  recipes       a stale replica ends with the provider's arena and outboards byte for byte: equal lengths in place, changed lengths
                into a fresh extent, each followed by outboard_diff -> have_runs -> set_slices_arena -> ingest_set_slices
  check         outboard_check passes honest outboards, names the node of a flipped byte and catches what the diff cannot
  tampered      every tampered blob of the CPU test once on the device: ordinary inputs that end in a status
  refusals      every one b3wit.h lists, with every output byte unchanged; and the calls allocate nothing"""
import functools

import numpy as np
import pytest

import b3w_testlib as T
import bao_delta_ref as D
import bao_have_ref as H
from test_bao_delta_cpu import cases, delta_c, tamper_base, tampers

pytestmark = pytest.mark.gpu

K = 1024
GUARD = 4096
FILL, WALL = 0xEE, 0xA5
GS = [0, 4, 6]
BAD = 100
NO_A = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def _setup():
    m = T.pkg()
    return dict(m=m, ctx=m.Context("nova_vesta", 0))


@pytest.fixture(scope="module", autouse=True)
def _a_memory_pool_of_its_own():
    """every device tensor of this module comes from a pool of the allocator that is the module's own and goes with it"""
    import gc
    import torch
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        torch.cuda.synchronize()
        if _setup.cache_info().currsize:
            _setup()["ctx"].close()
        _setup.cache_clear()
        _real.cache_clear()
        gc.collect()
    del pool


def _walled(size):
    """-> (the whole tensor, its middle `size` bytes): 0xEE between 0xA5 guards"""
    import torch
    whole = torch.full((size + 2 * GUARD,), WALL, dtype=torch.uint8, device="cuda")
    whole[GUARD:GUARD + size] = FILL
    return whole, whole[GUARD:GUARD + size]


def _walls_intact(whole, size):
    return bool((whole[:GUARD] == WALL).all().item()) and bool((whole[GUARD + size:] == WALL).all().item())


def _placed(obs, phase, fill=None):
    """byte strings at 8-byte-aligned places with one to three words of 0xA5 between them -> (device buffer, places, host copy)"""
    import torch
    places, at = [], 8 * (phase + 1)
    for f, ob in enumerate(obs):
        places.append(at)
        at += len(ob) + 8 * (1 + (f + phase) % 3)
    buf = np.full(at + 8, WALL, dtype=np.uint8)
    for o, ob in zip(places, obs):
        buf[o:o + len(ob)] = np.frombuffer(ob, dtype=np.uint8) if fill is None else fill
    return torch.from_numpy(buf).cuda(), np.array(places, dtype=np.uint64), buf


def _roots(sides):
    import torch
    words = np.concatenate([np.frombuffer(s[2], dtype=np.uint32) for s in sides] + [np.zeros(8, dtype=np.uint32)])
    return torch.from_numpy(words.view(np.int32).copy()).cuda()


def _batch(pairs):
    """[(side a or None, side b)] -> the distinct sides of each kind and the pair lists"""
    a_sides, b_sides, ia, ib, pa, pb = [], [], {}, {}, [], []
    for a, b in pairs:
        if a is not None and id(a) not in ia:
            ia[id(a)] = len(a_sides)
            a_sides.append(a)
        if id(b) not in ib:
            ib[id(b)] = len(b_sides)
            b_sides.append(b)
        pa.append(NO_A if a is None else ia[id(a)])
        pb.append(ib[id(b)])
    return a_sides, b_sides, np.array(pa, dtype=np.uint32), np.array(pb, dtype=np.uint32)


def _lens(sides):
    return np.array([s[1] for s in sides], dtype=np.uint64)


@pytest.mark.parametrize("g", GS)
def test_one_call_over_the_cpu_tests_pairs_is_the_host_mirror_and_bs_outboard(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    pairs = [(a, b) for _, a, b in cases(g)]
    a_sides, b_sides, pa, pb = _batch(pairs)
    assert len(pairs) >= 100 and (pa == NO_A).sum() >= 5 and np.bincount(pa[pa != NO_A]).max() >= 5
    d_a, at_a, host_a = _placed([x[0] for x in a_sides], 0)
    d_b, at_b, host_b = _placed([x[0] for x in b_sides], 1)
    lens_a, lens_b, roots_a, roots_b = _lens(a_sides), _lens(b_sides), _roots(a_sides), _roots(b_sides)
    mirror = [delta_c(m, a, b, g) for a, b in pairs]
    heads = [16 + 8 * D.words(D.units(b[1], g)) for _, b in pairs]
    extents, short = [], []
    for i, ((blob, k), head) in enumerate(zip(mirror, heads)):
        cut = i % 5 == 4 and k >= 2                                             # one node short, with or without a word of slack
        short.append(cut)
        extents.append(head + 64 * (k - 1) + 8 * (i % 2) if cut else len(blob) + 8 * (i % 3))
    first = np.cumsum([0] + extents).astype(np.uint64)
    assert sum(short) >= 10
    whole, d_delta = _walled(int(first[-1]))
    out = m.bao.outboard_delta(ctx, lens_a, d_a, roots_a, lens_b, d_b, roots_b, pa, pb, g, at_a, at_b, delta_first=first, d_delta=d_delta)
    torch.cuda.synchronize()
    assert out["delta"] is d_delta and (out["pair_lens"] == lens_b[pb]).all()
    got, n_nodes = d_delta.cpu().numpy(), out["n_nodes"].cpu().numpy()
    for i, ((blob, k), head) in enumerate(zip(mirror, heads)):
        ext = got[int(first[i]):int(first[i + 1])]
        used = head + 64 * min(k, (ext.size - head) // 64)
        assert int(n_nodes[i]) == k, (i, "k as found")
        assert ext[:used].tobytes() == blob[:used], (i, cases(g)[i][0], "not the host mirror's blob")
        assert (ext[used:] == FILL).all(), (i, "written behind the last node that fits")
    assert _walls_intact(whole, int(first[-1]))
    assert (d_a.cpu().numpy() == host_a).all() and (d_b.cpu().numpy() == host_b).all(), "an outboard or a guard between them was written"
    # the replica: into places of the test's own
    d_out, at_out, host_out = _placed([b[0] for _, b in pairs], 2, fill=FILL)
    res = m.bao.apply_outboard_delta(ctx, lens_a, d_a, roots_a, lens_b, roots_b, d_delta, first, pa, pb, g, at_a, ob_first_out=at_out, d_outboards_out=d_out)
    torch.cuda.synchronize()
    status, bad, after = res["pair_status"].cpu().numpy(), res["first_bad"].cpu().numpy(), d_out.cpu().numpy()
    for i, (_, b) in enumerate(pairs):
        o = int(at_out[i])
        if short[i]:
            assert (int(status[i]), int(bad[i])) == (D.MALFORMED, 0), (i, "a blob one node short")
            host_out[o:o + len(b[0])] = FILL
        else:
            assert (int(status[i]), int(bad[i])) == (0, -1), (i, cases(g)[i][0])
            host_out[o:o + len(b[0])] = np.frombuffer(b[0], dtype=np.uint8)
    assert (after == host_out).all(), "an output outboard is not b's, or a byte between them was written"
    assert (d_delta.cpu().numpy() == got).all() and (d_a.cpu().numpy() == host_a).all()
    # the defaults: a buffer of its own in the batch layout, which always suffices
    made = m.bao.outboard_delta(ctx, lens_a, d_a, roots_a, lens_b, d_b, roots_b, pa, pb, g, at_a, at_b)
    assert made["delta_first"].tolist() == m.bao.delta_layout(lens_b, g, pb).tolist()
    res = m.bao.apply_outboard_delta(ctx, lens_a, d_a, roots_a, lens_b, roots_b, made["delta"], made["delta_first"], pa, pb, g, at_a)
    assert not res["pair_status"].any().item() and (res["first_bad"] == -1).all().item()
    assert res["outboards"].cpu().numpy().tobytes() == b"".join(b[0] for _, b in pairs)
    print(f"group_log {g}: {len(pairs)} pairs, {int(n_nodes.sum())} nodes sent of {sum(D.units(b[1], g) - 1 for _, b in pairs)}")


# ---- places -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _real():
    """a file of 2^16 + 5 chunks and a version with a few hundred chunks rewritten, their outboards from outboard_batch"""
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    rng = np.random.default_rng(80)
    n = (1 << 16) + 5
    ln = n * K - 300
    old = rng.integers(0, 256, 16 + ln + 64, dtype=np.uint8)                     # (the file lies at byte 16)
    new = old.copy()
    edges = [0, n - 1, 1023, 1024, 63, 64, 65, 127, 128, 2047, 2048, 1 << 15, (1 << 15) - 1, 1 << 16, (1 << 16) - 1]
    chunks = np.unique(np.concatenate([np.array(edges), rng.integers(0, n, 300)]))
    for c in chunks.tolist():
        new[16 + c * K + 5] ^= 0x40
    offsets, lens = np.array([16], dtype=np.uint64), np.array([ln], dtype=np.uint64)
    sides = [m.bao.outboard_batch(ctx, torch.from_numpy(data).cuda(), offsets, lens) for data in (old, new)]
    torch.cuda.synchronize()
    return dict(n=n, lens=lens, chunks=chunks, a=sides[0], b=sides[1])


def test_real_outboards_of_65541_chunks():
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    r = _real()
    n, lens, a, b = r["n"], r["lens"], r["a"], r["b"]
    ob_a, ob_b = a["outboards"].cpu().numpy(), b["outboards"].cpu().numpy()
    same = D.same_np(ob_a, n, ob_b, n, 0)
    assert not same[0] and r["chunks"].size <= (~same).sum() <= 17 * r["chunks"].size
    out = m.bao.outboard_delta(ctx, lens, a["outboards"], a["roots"], lens, b["outboards"], b["roots"])
    k = int(out["n_nodes"].item())
    assert k == int((~same).sum())
    W = D.words(n)
    blob = out["delta"].cpu().numpy()
    assert blob[:16].view(np.uint64).tolist() == [int(lens[0]), k]
    assert blob[16:16 + 8 * W].tobytes() == D.pack(~same)
    assert (blob[16 + 8 * W:16 + 8 * W + 64 * k].reshape(-1, 64) == ob_b[8:].reshape(-1, 64)[~same]).all()
    exact = np.array([0, 16 + 8 * W + 64 * k], dtype=np.uint64)
    res = m.bao.apply_outboard_delta(ctx, lens, a["outboards"], a["roots"], lens, b["roots"], out["delta"][:int(exact[1])], exact)
    assert res["pair_status"].tolist() == [0] and res["first_bad"].tolist() == [-1]
    assert torch.equal(res["outboards"], b["outboards"])
    mine = a["outboards"].clone()                                                # in place
    res = m.bao.apply_outboard_delta(ctx, lens, mine, a["roots"], lens, b["roots"], out["delta"], out["delta_first"], ob_first_out=np.zeros(1, dtype=np.uint64),
                                     d_outboards_out=mine)
    assert res["pair_status"].tolist() == [0] and torch.equal(mine, b["outboards"])
    print(f"{n} chunks, {r['chunks'].size} rewritten: {k} of {n - 1} nodes sent, {16 + 8 * W + 64 * k} bytes against {ob_b.size}")


def test_the_bitmap_and_ranks_of_a_million_units():
    """fabricated outboards (random bytes: the provider hashes nothing) that differ in a few thousand stored halves"""
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    rng = np.random.default_rng(81)
    n = (1 << 20) + 5
    ob_a = rng.integers(0, 256, 8 + 64 * (n - 1), dtype=np.uint8)
    ob_b = ob_a.copy()
    halves = np.unique(np.concatenate([np.array([0, 1, 2, 3, 126, 127, 128, 129, 2 * (n - 1) - 1, 2 * (n - 1) - 2]), rng.integers(0, 2 * (n - 1), 4000)]))
    ob_b[8 + 32 * halves + rng.integers(0, 32, halves.size)] ^= 1
    # a shorter a, whose nodes lie at other places: every span it has in common with b stores what ob_a stores for it in b's shape
    short = n - 70000
    ob_s = rng.integers(0, 256, 8 + 64 * (short - 1), dtype=np.uint8)
    lo_s, cnt_s, par_s, side_s = D.nodes_np(short)
    lo_b, cnt_b, par_b, side_b = D.nodes_np(n)
    key_b = lo_b * (1 << 32) + cnt_b
    order = np.argsort(key_b)
    hit = order[np.clip(np.searchsorted(key_b[order], lo_s * (1 << 32) + cnt_s), 0, n - 2)]
    both = np.flatnonzero((key_b[hit] == lo_s * (1 << 32) + cnt_s) & (hit != 0) & (np.arange(short - 1) != 0))
    cols = np.arange(32, dtype=np.int64)
    ob_s[(8 + 64 * par_s[both] + 32 * side_s[both])[:, None] + cols] = ob_a[(8 + 64 * par_b[hit[both]] + 32 * side_b[hit[both]])[:, None] + cols]
    for na, ob in ((n, ob_a), (short, ob_s)):
        same = D.same_np(ob, na, ob_b, n, 0, roots_equal=True)
        if na == n:                                                             # (a changed half is a node's stored CV where the child is no leaf)
            _, _, parent, side = D.nodes_np(n)
            assert (~same[1:] == np.isin(2 * parent[1:] + side[1:], halves)).all() and same[0] and 1000 < (~same).sum() < halves.size
        else:
            assert same.any() and (~same).sum() >= 60000
        lens_a, lens_b = np.array([na * K], dtype=np.uint64), np.array([n * K], dtype=np.uint64)
        d_a, d_b = torch.from_numpy(np.ascontiguousarray(ob)).cuda(), torch.from_numpy(ob_b).cuda()
        roots = torch.zeros(8, dtype=torch.int32, device="cuda")
        first = np.array([0, D.bound(n * K, 0) + 64], dtype=np.uint64)
        whole, d_delta = _walled(int(first[1]))
        out = m.bao.outboard_delta(ctx, lens_a, d_a, roots, lens_b, d_b, roots, delta_first=first, d_delta=d_delta)
        k, W = int(out["n_nodes"].item()), D.words(n)
        blob = d_delta.cpu().numpy()
        assert k == int((~same).sum()) and blob[:16].view(np.uint64).tolist() == [n * K, k]
        assert blob[16:16 + 8 * W].tobytes() == D.pack(~same), "the bitmap"
        assert (blob[16 + 8 * W:16 + 8 * W + 64 * k].reshape(-1, 64) == ob_b[8:].reshape(-1, 64)[~same]).all(), "a node is not at its rank"
        assert (blob[16 + 8 * W + 64 * k:] == FILL).all() and _walls_intact(whole, int(first[1]))
        del d_a, d_b, d_delta, whole


# ---- the recipes to the end ---------------------------------------------------------------------------------------------------------
def _rewrite(arena, offset, length, chunks, rng):
    for c in chunks:
        a, b = c * K, min(length, (c + 1) * K)
        arena[offset + a:offset + b] = rng.integers(0, 256, b - a, dtype=np.uint8)
        arena[offset + a] ^= 0xFF


def _finish(s, g, d_replica, d_provider, offsets, old_lens, old_obs, old_roots, new_lens, trusted, provider):
    """outboard_diff -> have_runs -> set_slices_arena -> ingest_set_slices against the outboards the apply left -> the chunks fetched"""
    import torch
    m, ctx = s["m"], s["ctx"]
    assert torch.equal(trusted, provider["outboards"]), "the applied outboards are not the provider's"
    diff = m.bao.outboard_diff(ctx, old_lens, old_obs, old_roots, new_lens, trusted, provider["roots"], group_log_a=g, group_log_b=g)
    missing = m.bao.have_runs(ctx, diff["same"], diff["pair_lens"], "missing")
    fetched = int(missing["n_chunks"].sum())
    assert 0 < fetched < sum(H.num_chunks(int(x)) for x in new_lens)
    sl = m.bao.set_slices_arena(ctx, d_provider, offsets, new_lens, provider["outboards"], missing["files"], missing["first_chunks"], missing["n_chunks"], group_log=g)
    res = m.bao.ingest_set_slices(ctx, d_replica, offsets, new_lens, trusted, provider["roots"], missing["files"], missing["first_chunks"], missing["n_chunks"],
                                  sl["slices"], group_log=g, d_have=diff["same"])
    assert not res["set_status"].any().item() and not res["chunk_status"].any().item()
    assert torch.equal(d_replica, d_provider), "the replica's arena is not the provider's"
    assert torch.equal(trusted, provider["outboards"]), "the replica's outboards are not the provider's"
    ver = m.bao.verify_batch(ctx, d_replica, offsets, new_lens, trusted, provider["roots"], group_log=g)
    assert not ver["unit_status"].any().item() and not ver["file_status"].any().item()
    return fetched


def _outboards(s, g, d, offsets, lens):
    m, ctx = s["m"], s["ctx"]
    return m.bao.outboard_batch(ctx, d, offsets, lens) if g == 0 else m.bao.outboard_groups_batch(ctx, d, offsets, lens, g)


@pytest.mark.parametrize("g", [0, 4])
def test_equal_lengths_in_place_and_then_the_chunks(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    rng = np.random.default_rng(90 + g)
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
    for o, ln, n in zip(offsets.tolist(), lens.tolist(), n_of):
        _rewrite(new, o, ln, np.unique(np.concatenate([rng.permutation(n)[:max(1, n // 10)], [n - 1]])).astype(np.int64).tolist(), rng)
    d_replica, d_provider = torch.from_numpy(old).cuda(), torch.from_numpy(new).cuda()
    mine, provider = _outboards(s, g, d_replica, offsets, lens), _outboards(s, g, d_provider, offsets, lens)
    delta = m.bao.outboard_delta(ctx, lens, mine["outboards"], mine["roots"], lens, provider["outboards"], provider["roots"], group_log=g)
    sent = int(delta["n_nodes"].sum().item())
    assert 0 < sent < sum(D.units(int(x), g) - 1 for x in lens)
    kept = mine["outboards"].clone()                                             # (the diff below still wants the stale outboards)
    res = m.bao.apply_outboard_delta(ctx, lens, mine["outboards"], mine["roots"], lens, provider["roots"], delta["delta"], delta["delta_first"], group_log=g,
                                     ob_first_out=np.ascontiguousarray(mine["ob_first"][:-1], dtype=np.uint64), d_outboards_out=mine["outboards"])
    assert not res["pair_status"].any().item() and res["outboards"] is mine["outboards"]
    fetched = _finish(s, g, d_replica, d_provider, offsets, lens, kept, mine["roots"], lens, mine["outboards"], provider)
    print(f"group_log {g}: {sent} nodes sent, {fetched} chunks fetched")


@pytest.mark.parametrize("g", [0, 4])
def test_changed_lengths_into_a_fresh_extent_and_then_the_chunks(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    rng = np.random.default_rng(95 + g)
    old_lens = np.array([1000 * K - 17, 70 * K], dtype=np.uint64)               # grown across the tile of 1 024 chunks; shrunk
    new_lens = np.array([1100 * K + 5, 40 * K - 500], dtype=np.uint64)
    offsets = np.array([7, 7 + 1100 * K + 64 + 2], dtype=np.uint64)
    size = int(offsets[1]) + 70 * K + 64
    old = rng.integers(0, 256, size, dtype=np.uint8)
    new = old.copy()
    for o, lo, ln in zip(offsets.tolist(), old_lens.tolist(), new_lens.tolist()):
        if ln > lo:
            new[o + lo:o + ln] = rng.integers(0, 256, ln - lo, dtype=np.uint8)
        n = H.num_chunks(min(lo, ln))
        _rewrite(new, o, ln, rng.permutation(n)[:n // 10].tolist(), rng)
    d_replica, d_provider = torch.from_numpy(old).cuda(), torch.from_numpy(new).cuda()
    stale, provider = _outboards(s, g, d_replica, offsets, old_lens), _outboards(s, g, d_provider, offsets, new_lens)
    delta = m.bao.outboard_delta(ctx, old_lens, stale["outboards"], stale["roots"], new_lens, provider["outboards"], provider["roots"], group_log=g)
    sent = int(delta["n_nodes"].sum().item())
    assert 0 < sent < sum(D.units(int(x), g) - 1 for x in new_lens)
    res = m.bao.apply_outboard_delta(ctx, old_lens, stale["outboards"], stale["roots"], new_lens, provider["roots"], delta["delta"], delta["delta_first"], group_log=g)
    assert not res["pair_status"].any().item()
    fetched = _finish(s, g, d_replica, d_provider, offsets, old_lens, stale["outboards"], stale["roots"], new_lens, res["outboards"], provider)
    print(f"group_log {g}: {sent} nodes sent of {sum(D.units(int(x), g) - 1 for x in new_lens)}, {fetched} chunks fetched")


# ---- an outboard against its root, without the file -------------------------------------------------------------------------------
def test_outboard_check():
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    r = _real()
    n, lens, a, b = r["n"], r["lens"], r["a"], r["b"]
    both = torch.cat([a["outboards"], b["outboards"]])
    lens2, first2, roots2 = np.concatenate([lens, lens]), np.array([0, a["outboards"].numel()], dtype=np.uint64), torch.cat([a["roots"].view(-1), b["roots"].view(-1)])
    res = m.bao.outboard_check(ctx, lens2, both, roots2, ob_first=first2)
    assert res["file_status"].tolist() == [0, 0] and res["first_bad"].tolist() == [-1, -1]
    spans = {(int(lo), int(cnt)): p for p, (lo, cnt) in enumerate(zip(*D.nodes_np(n)[:2]))}
    # a flipped byte: the node that holds it no longer hashes to what is stored above it
    p = spans[(1024, 1024)]
    lied = both.clone()
    lied[8 + 64 * p + 37] ^= 2
    res = m.bao.outboard_check(ctx, lens2, lied, roots2, ob_first=first2)
    assert res["file_status"].tolist() == [D.BAD_HASH, 0] and res["first_bad"].tolist() == [p, -1]
    # what the diff cannot see: b's outboard with the CV of a rewritten chunk overwritten by a's - the diff would call the chunk same
    assert 1024 in r["chunks"].tolist()
    p = spans[(1024, 2)]                                                         # (chunk 1024 is the left half of this leaf parent)
    at = int(first2[1]) + 8 + 64 * p
    lied = both.clone()
    lied[at:at + 32] = a["outboards"][8 + 64 * p:8 + 64 * p + 32]
    assert not torch.equal(lied, both)
    diff = m.bao.outboard_diff(ctx, lens, a["outboards"], a["roots"], lens, lied[int(first2[1]):].contiguous(), b["roots"])
    assert (int(diff["same"][1024 >> 6].item()) >> (1024 & 63)) & 1, "the diff believes the lie"
    res = m.bao.outboard_check(ctx, lens2, lied, roots2, ob_first=first2)
    assert res["file_status"].tolist() == [0, D.BAD_HASH] and res["first_bad"].tolist() == [-1, p]
    # a wrong root
    wrong = roots2.clone()
    wrong[3] ^= 1
    res = m.bao.outboard_check(ctx, lens2, both, wrong, ob_first=first2)
    assert res["file_status"].tolist() == [D.BAD_HASH, 0] and res["first_bad"].tolist() == [0, -1]
    # group outboards, and files of one unit (nothing to check: the outboard is its length)
    small = np.array([1, 700, 17 * K, 16 * K], dtype=np.uint64)
    arena = torch.from_numpy(np.random.default_rng(5).integers(0, 256, 40 * K, dtype=np.uint8)).cuda()
    offs = np.array([0, 8, 1024, 20 * K], dtype=np.uint64)
    made = m.bao.outboard_groups_batch(ctx, arena, offs, small, 4)
    res = m.bao.outboard_check(ctx, small, made["outboards"], made["roots"], group_log=4)
    assert res["file_status"].tolist() == [0, 0, 0, 0]


# ---- tampered blobs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", GS)
def test_every_tampered_blob_ends_in_its_status_on_the_device(g):
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    _, b, good, _ = tamper_base(g)
    cases_ = [("the blob as it was made", tamper_base(g)[0], good, 0, -1)] + list(tampers(g))
    a_sides, b_sides, pa, pb = _batch([(a, b) for _, a, _, _, _ in cases_])
    assert len(b_sides) == 1
    d_a, at_a, host_a = _placed([x[0] for x in a_sides], 0)
    blobs = [blob for _, _, blob, _, _ in cases_]
    assert all(len(x) % 8 == 0 for x in blobs)
    first = np.cumsum([0] + [len(x) for x in blobs]).astype(np.uint64)
    d_delta = torch.from_numpy(np.frombuffer(b"".join(blobs), dtype=np.uint8).copy()).cuda()
    d_out, at_out, host_out = _placed([b[0]] * len(cases_), 1, fill=FILL)
    res = m.bao.apply_outboard_delta(ctx, _lens(a_sides), d_a, _roots(a_sides), _lens(b_sides), _roots(b_sides), d_delta, first, pa, pb, g, at_a, ob_first_out=at_out,
                                     d_outboards_out=d_out)
    torch.cuda.synchronize()
    status, bad = res["pair_status"].cpu().tolist(), res["first_bad"].cpu().tolist()
    for i, (name, _, _, want_status, want_bad) in enumerate(cases_):
        assert (status[i], bad[i]) == (want_status, want_bad), (name, status[i], bad[i])
        if want_status == 0:
            host_out[int(at_out[i]):int(at_out[i]) + len(b[0])] = np.frombuffer(b[0], dtype=np.uint8)
    assert (d_out.cpu().numpy() == host_out).all(), "a pair with a status had its output written, or a passed one is not b's outboard"
    assert (d_a.cpu().numpy() == host_a).all()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_output_untouched():
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    L = m.lib()
    stream = torch.cuda.current_stream().cuda_stream
    a, b, blob, _ = tamper_base(0)
    one = (b"\xbc\x02" + bytes(6), 700, bytes(range(32)))
    sides = [a, b, one]
    lens = _lens(sides)
    obs = [x[0] for x in sides]
    first = np.cumsum([0] + [len(o) for o in obs]).astype(np.uint64)
    d_obs = torch.from_numpy(np.frombuffer(b"".join(obs) + bytes(16), dtype=np.uint8).copy()).cuda()
    d_roots = _roots(sides)
    pa, pb = np.array([0, NO_A, 1, 2], dtype=np.uint32), np.array([1, 1, 2, 2], dtype=np.uint32)
    dfirst = m.bao.delta_layout(lens, 0, pb)
    whole, d_delta = _walled(int(dfirst[-1]))
    wn, d_n = _walled(8 * 4)
    scratch_bytes = int(L.b3w_bao_outboard_delta_scratch_bytes(lens.ctypes.data, 3, pb.ctypes.data, 4, 0))
    ws, d_scratch = _walled(scratch_bytes)
    good = dict(ctx=ctx.handle, la=lens.ctypes.data, fa=first.ctypes.data, oa=d_obs.data_ptr(), ba=int(first[-1]), ra=d_roots.data_ptr(), na=3, lb=lens.ctypes.data,
                fb=first.ctypes.data, ob=d_obs.data_ptr(), bb=int(first[-1]), rb=d_roots.data_ptr(), nb=3, ga=0, gb=0, pa=pa.ctypes.data, pb=pb.ctypes.data, n=4,
                df=dfirst.ctypes.data, dd=d_delta.data_ptr(), db=int(dfirst[-1]), dn=d_n.data_ptr(), sc=d_scratch.data_ptr(), sb=scratch_bytes)

    def provider(**change):
        kw = dict(good)
        kw.update(change)
        rc = L.b3w_bao_outboard_delta_device(kw["ctx"], kw["la"], kw["fa"], kw["oa"], kw["ba"], kw["ra"], kw["na"], kw["lb"], kw["fb"], kw["ob"], kw["bb"], kw["rb"], kw["nb"],
                                             kw["ga"], kw["gb"], kw["pa"], kw["pb"], kw["n"], kw["df"], kw["dd"], kw["db"], kw["dn"], kw["sc"], kw["sb"], stream)
        torch.cuda.synchronize()
        return rc

    def untouched():
        return bool((d_delta == FILL).all().item()) and bool((d_n == FILL).all().item()) and _walls_intact(whole, int(dfirst[-1])) and _walls_intact(wn, 32)
    bad_first, far_first = first.copy(), first.copy()
    bad_first[1] += 4
    far_first[2] += 16
    bad_pair = np.array([0, NO_A, 3, 2], dtype=np.uint32)
    long_lens = lens.copy()
    long_lens[1] = ((1 << 30) + 1) * K
    df_odd, df_back, df_small, df_far = dfirst.copy(), dfirst.copy(), dfirst.copy(), dfirst.copy()
    df_odd[1] += 4
    df_back[2] = df_back[1] - 8
    df_small[1] = df_small[0] + 16 + 8 * 2 - 8
    df_far[-1] += 8
    refusals = [dict(ctx=None)] + [{k: None} for k in ("la", "fa", "oa", "ra", "lb", "fb", "ob", "rb", "pa", "pb", "df", "dd", "dn", "sc")] + \
        [dict(oa=good["oa"] + 4), dict(ob=good["ob"] + 4), dict(ra=good["ra"] + 2), dict(rb=good["rb"] + 2), dict(dd=good["dd"] + 4), dict(dn=good["dn"] + 4),
         dict(sc=good["sc"] + 4), dict(sb=scratch_bytes - 16), dict(fa=bad_first.ctypes.data), dict(fb=bad_first.ctypes.data), dict(ga=7, gb=7), dict(ga=4), dict(gb=4),
         dict(pa=bad_pair.ctypes.data), dict(pb=bad_pair.ctypes.data), dict(na=0), dict(nb=2), dict(la=long_lens.ctypes.data, ba=1 << 40),
         dict(lb=long_lens.ctypes.data, bb=1 << 40), dict(ba=good["ba"] - 1), dict(bb=good["bb"] - 1), dict(fb=far_first.ctypes.data),
         dict(df=df_odd.ctypes.data), dict(df=df_back.ctypes.data), dict(df=df_small.ctypes.data), dict(df=df_far.ctypes.data), dict(db=good["db"] - 8),
         dict(dd=good["oa"] + 64, db=int(dfirst[-1])), dict(dd=good["oa"] + int(first[-1]) - 8)]
    for change in refusals:
        assert provider(**change) == BAD and untouched(), change
        if change.get("ctx", 1) is not None:
            assert "bao outboard delta" in ctx.last_error(), change
    assert provider(n=0, la=None, fa=None, oa=None, ra=None, lb=None, fb=None, ob=None, rb=None, pa=None, pb=None, df=None, dd=None, dn=None, sc=None) == 0 and untouched()
    assert provider() == 0, ctx.last_error()
    blobs = d_delta.cpu().numpy()
    want = [delta_c(m, x, y, 0) for x, y in ((a, b), (None, b), (b, one), (one, one))]
    for i, (w, k) in enumerate(want):
        used = 16 + 8 * D.words(D.units(int(lens[pb[i]]), 0)) + 64 * k
        assert blobs[int(dfirst[i]):int(dfirst[i]) + used].tobytes() == w[:used] and int(d_n.view(torch.int64)[i].item()) == k
    assert _walls_intact(whole, int(dfirst[-1])) and _walls_intact(ws, scratch_bytes)
    # the replica
    out_first = np.cumsum([0] + [len(sides[f][0]) + 8 for f in pb.tolist()]).astype(np.uint64)
    wo, d_out = _walled(int(out_first[-1]))
    wst, d_status = _walled(4 * 4)
    wb, d_bad = _walled(8 * 4)
    good2 = dict(ctx=ctx.handle, la=good["la"], fa=good["fa"], oa=good["oa"], ba=good["ba"], ra=good["ra"], na=3, lb=good["lb"], rb=good["rb"], nb=3, g=0, pa=good["pa"],
                 pb=good["pb"], n=4, df=good["df"], dd=good["dd"], db=good["db"], of=out_first.ctypes.data, oo=d_out.data_ptr(), obytes=int(out_first[-1]),
                 st=d_status.data_ptr(), bd=d_bad.data_ptr(), sc=good["sc"], sb=scratch_bytes)

    def replica(**change):
        kw = dict(good2)
        kw.update(change)
        rc = L.b3w_bao_outboard_delta_apply_device(kw["ctx"], kw["la"], kw["fa"], kw["oa"], kw["ba"], kw["ra"], kw["na"], kw["lb"], kw["rb"], kw["nb"], kw["g"], kw["pa"],
                                                   kw["pb"], kw["n"], kw["df"], kw["dd"], kw["db"], kw["of"], kw["oo"], kw["obytes"], kw["st"], kw["bd"], kw["sc"], kw["sb"],
                                                   stream)
        torch.cuda.synchronize()
        return rc

    def untouched2():
        return all(bool((t == FILL).all().item()) for t in (d_out, d_status, d_bad)) and _walls_intact(wo, int(out_first[-1])) and _walls_intact(wst, 16) and \
            _walls_intact(wb, 32)
    of_odd, of_back, of_far = out_first.copy(), out_first.copy(), out_first.copy()
    of_odd[1] += 4
    of_back[1], of_back[2] = out_first[2], out_first[1]
    of_far[3] = out_first[-1]
    snapshot = d_obs.clone()
    refusals = [dict(ctx=None)] + [{k: None} for k in ("la", "fa", "oa", "ra", "lb", "rb", "pa", "pb", "df", "dd", "of", "oo", "st", "bd", "sc")] + \
        [dict(oa=good["oa"] + 4), dict(ra=good["ra"] + 2), dict(rb=good["rb"] + 2), dict(dd=good["dd"] + 4), dict(oo=good2["oo"] + 4), dict(st=good2["st"] + 2),
         dict(bd=good2["bd"] + 4), dict(sc=good["sc"] + 4), dict(sb=scratch_bytes - 16), dict(fa=bad_first.ctypes.data), dict(g=7), dict(pa=bad_pair.ctypes.data),
         dict(pb=bad_pair.ctypes.data), dict(na=0), dict(nb=2), dict(la=long_lens.ctypes.data, ba=1 << 40), dict(lb=long_lens.ctypes.data), dict(ba=good["ba"] - 1),
         dict(df=df_odd.ctypes.data), dict(df=df_back.ctypes.data), dict(df=df_small.ctypes.data), dict(df=df_far.ctypes.data), dict(db=good["db"] - 8),
         dict(of=of_odd.ctypes.data), dict(of=of_back.ctypes.data), dict(of=of_far.ctypes.data), dict(obytes=int(out_first[-1]) - 16),
         dict(oo=good["dd"] + 8, obytes=int(out_first[-1])),                    # the outputs in the blob buffer
         dict(oo=good["oa"], obytes=int(first[-1])),                            # the outputs in a's buffer, but not every pair at a's own place
         dict(oo=good["oa"] + 8, obytes=int(first[-1]) - 8)]
    for change in refusals:
        assert replica(**change) == BAD and untouched2(), change
        if change.get("ctx", 1) is not None:
            assert "bao outboard delta apply" in ctx.last_error(), change
    assert torch.equal(d_obs, snapshot) and (d_delta.cpu().numpy() == blobs).all()
    assert replica(n=0, la=None, fa=None, oa=None, ra=None, lb=None, rb=None, pa=None, pb=None, df=None, dd=None, of=None, oo=None, st=None, bd=None, sc=None) == 0 and untouched2()
    assert replica() == 0, ctx.last_error()
    assert d_status.view(torch.int32).tolist() == [0, 0, 0, 0] and d_bad.view(torch.int64).tolist() == [-1] * 4
    got = d_out.cpu().numpy()
    for i, f in enumerate(pb.tolist()):
        o = int(out_first[i])
        assert got[o:o + len(sides[f][0])].tobytes() == sides[f][0] and (got[o + len(sides[f][0]):int(out_first[i + 1])] == FILL).all()
    assert _walls_intact(wo, int(out_first[-1]))
    # the wrappers' own
    for kw in (dict(pairs_a=[0]), dict(pairs_a=[0, 1], pairs_b=[0]), dict(pairs_a=[3], pairs_b=[0]), dict(group_log=7), dict(d_delta=d_delta.to(torch.int32)),
               dict(delta_first=dfirst[:2]), dict(d_scratch=d_scratch[:8])):
        with pytest.raises(m.B3WError):
            m.bao.outboard_delta(ctx, lens, d_obs, d_roots, lens, d_obs, d_roots, **kw)


def test_the_calls_allocate_nothing():
    import torch
    s = _setup()
    m, ctx = s["m"], s["ctx"]
    L = m.lib()
    stream = torch.cuda.current_stream().cuda_stream
    pairs = [(a, b) for _, a, b in cases(0)][::3]
    a_sides, b_sides, pa, pb = _batch(pairs)
    d_a, at_a, _ = _placed([x[0] for x in a_sides], 0)
    d_b, at_b, _ = _placed([x[0] for x in b_sides], 1)
    lens_a, lens_b, roots_a, roots_b = _lens(a_sides), _lens(b_sides), _roots(a_sides), _roots(b_sides)
    first = m.bao.delta_layout(lens_b, 0, pb)
    out_first = np.ascontiguousarray(m.bao.group_batch_layout(lens_b[pb], 0), dtype=np.uint64)
    d_delta = torch.empty(int(first[-1]), dtype=torch.uint8, device="cuda")
    d_out = torch.empty(int(out_first[-1]), dtype=torch.uint8, device="cuda")
    d_n, d_bad = torch.empty(len(pairs), dtype=torch.int64, device="cuda"), torch.empty(len(pairs), dtype=torch.int64, device="cuda")
    d_status = torch.empty(len(pairs), dtype=torch.int32, device="cuda")
    need = int(L.b3w_bao_outboard_delta_scratch_bytes(lens_b.ctypes.data, lens_b.size, pb.ctypes.data, pb.size, 0))
    d_scratch = torch.empty(need, dtype=torch.uint8, device="cuda")

    def once():
        assert L.b3w_bao_outboard_delta_device(ctx.handle, lens_a.ctypes.data, at_a.ctypes.data, d_a.data_ptr(), d_a.numel(), roots_a.data_ptr(), lens_a.size,
                                               lens_b.ctypes.data, at_b.ctypes.data, d_b.data_ptr(), d_b.numel(), roots_b.data_ptr(), lens_b.size, 0, 0, pa.ctypes.data,
                                               pb.ctypes.data, pa.size, first.ctypes.data, d_delta.data_ptr(), d_delta.numel(), d_n.data_ptr(), d_scratch.data_ptr(), need,
                                               stream) == 0, ctx.last_error()
        assert L.b3w_bao_outboard_delta_apply_device(ctx.handle, lens_a.ctypes.data, at_a.ctypes.data, d_a.data_ptr(), d_a.numel(), roots_a.data_ptr(), lens_a.size,
                                                     lens_b.ctypes.data, roots_b.data_ptr(), lens_b.size, 0, pa.ctypes.data, pb.ctypes.data, pa.size, first.ctypes.data,
                                                     d_delta.data_ptr(), d_delta.numel(), out_first.ctypes.data, d_out.data_ptr(), d_out.numel(), d_status.data_ptr(),
                                                     d_bad.data_ptr(), d_scratch.data_ptr(), need, stream) == 0, ctx.last_error()
        torch.cuda.synchronize()
    once()                                                                    # (the context's staging grows here, outside the allocator)
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    once()
    assert torch.cuda.max_memory_allocated() == before
    assert not d_status.any().item() and d_out.cpu().numpy().tobytes() == b"".join(b[0] for _, b in pairs)
