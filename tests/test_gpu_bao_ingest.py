"""Verified slices taken into resident files and their outboards on the device (bao.ingest_slices, b3w_bao_slice_ingest_device): the
receiver's side of bao slices.  The source arena is test_gpu_bao_slices._world()'s (16-byte aligned and odd starts) with files of the
module's own behind it at 4, 8 and 12 modulo 16 and at an odd byte, all with a ragged last chunk, 1 024 * 1 025 and 2^20 + 300 bytes
among them (the smallest lengths that cross a tile).  The provider's side (outboard_batch / outboard_groups_batch and slices_arena over
the source arena) is computed once and left unchanged; the receiver starts from buffers of 0xEE between 0xA5 guards and holds only the
roots.  Every chunk taken in gives the source's bytes and the provider's outboards byte for byte; a subset writes what the host call
(b3w_bao_slice_ingest) writes and nothing else; a tampered slice has the planner's and the decoder's status and writes nothing."""
import ctypes
import functools
import struct

import numpy as np
import pytest

import b3w_testlib as T
import bao_ref as R
import blake3_ref as B
from test_gpu_bao_slices import _listed_samples, _world

pytestmark = pytest.mark.gpu

K = 1024
GUARD = 4096
FILL, WALL = 0xEE, 0xA5
GS = [0, 1, 4, 6]
BAD = 100
OWN = [(K * 1025, 8), ((1 << 20) + 300, 1), (5 * K + 300, 4), (3 * K + 17, 12), (70 * K + 1, 7), (64 * K + 999, 4)]      # (length, start modulo 16)


@functools.lru_cache(maxsize=None)
def _setup():
    """the source arena, the provider's outboards of it at every g and the slices of every chunk of every file, shuffled"""
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    w_arena, w_offsets, w_lens, _ = _world()
    at = (w_arena.size + 15) // 16 * 16
    offsets, lens = [int(x) for x in w_offsets], [int(x) for x in w_lens]
    for ln, phase in OWN:
        at = (at + 48 + 15) // 16 * 16 + phase
        offsets.append(at)
        lens.append(ln)
        at += ln
    arena = np.random.default_rng(20).integers(0, 256, at + 64, dtype=np.uint8)
    arena[:w_arena.size] = w_arena
    offsets = np.array(offsets, dtype=np.uint64)
    assert {int(o) % 16 for o in offsets} >= {0, 4, 8, 12} and any(int(o) % 2 for o in offsets)
    in_file = np.zeros(arena.size, dtype=bool)
    for o, ln in zip(offsets, lens):
        in_file[int(o):int(o) + ln] = True
    d_src = torch.from_numpy(arena).cuda()
    made = {0: m.bao.outboard_batch(ctx, d_src, offsets, lens)}
    for g in GS[1:]:
        made[g] = m.bao.outboard_groups_batch(ctx, d_src, offsets, lens, g)
        assert torch.equal(made[g]["roots"], made[0]["roots"])
    files = np.concatenate([np.full(m.bao.num_chunks(ln), f, dtype=np.uint32) for f, ln in enumerate(lens)])
    chunks = np.concatenate([np.arange(m.bao.num_chunks(ln), dtype=np.uint64) for ln in lens])
    perm = np.random.default_rng(21).permutation(files.size)
    files, chunks = files[perm], chunks[perm]
    every = m.bao.slices_arena(ctx, d_src, offsets, lens, made[0]["outboards"], files, chunks)
    torch.cuda.synchronize()
    return dict(m=m, ctx=ctx, arena=arena, offsets=offsets, lens=lens, ln=np.array(lens, dtype=np.uint64), in_file=in_file, d_src=d_src, made=made,
                roots=made[0]["roots"], roots_host=made[0]["roots"].cpu().numpy().view(np.uint32).reshape(-1, 8).copy(), files=files, chunks=chunks,
                every=every["slices"])


@pytest.fixture(scope="module", autouse=True)
def _a_memory_pool_of_its_own():
    """every device tensor of this module (the arenas, the provider's side, the 5 GiB file) comes from a pool of the allocator that is the
    module's own and goes with it: the modules behind this one that measure device memory find the default pool's cached blocks as they
    would without this one"""
    import gc
    import torch
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        torch.cuda.synchronize()
        if _setup.cache_info().currsize:
            _setup()["ctx"].close()
        _setup.cache_clear()
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


def _ob_total(s, g):
    return int(s["made"][g]["ob_first"][-1])


def _host_ingest(s, g, files, chunks, slices, roots):
    """the host call over the same samples in order -> (arena, outboards, statuses) from buffers of 0xEE"""
    m = s["m"]
    ob_first = s["made"][g]["ob_first"]
    arena, obs = np.full(s["arena"].size, FILL, dtype=np.uint8), np.full(_ob_total(s, g), FILL, dtype=np.uint8)
    st = []
    for f, c, sl in zip(files.tolist(), chunks.tolist(), slices):
        a, ln = int(s["offsets"][f]), s["lens"][f]
        st.append(m.bao.ingest_slice_host(arena[a:a + ln], obs[int(ob_first[f]):int(ob_first[f + 1])], ln, c, roots[f], sl, g))
    return arena, obs, np.array(st, dtype=np.int32)


def _packed(m, ln, files, chunks, slices):
    """the slices packed as slice_layout says (numpy), the padding 0x5C"""
    sf = m.bao.slice_layout(ln, files, chunks)
    out = np.full(int(sf[-1]), 0x5C, dtype=np.uint8)
    for a, sl in zip(sf[:-1], slices):
        out[int(a):int(a) + len(sl)] = np.frombuffer(sl, dtype=np.uint8)
    return out


def _source_slices(s, files, chunks):
    """-> the samples' slices as bytes, extracted on the device from the source arena"""
    m = s["m"]
    out = m.bao.slices_arena(s["ctx"], s["d_src"], s["offsets"], s["lens"], s["made"][0]["outboards"], files, chunks)
    host, sf = out["slices"].cpu().numpy(), out["slice_first"]
    return [host[int(sf[i]):int(sf[i]) + m.bao.slice_size(s["lens"][f], c)].tobytes() for i, (f, c) in enumerate(zip(files.tolist(), chunks.tolist()))]


@pytest.mark.parametrize("g", GS)
def test_every_chunk_of_every_file(g):
    import torch
    s = _setup()
    m = s["m"]
    size, total = s["arena"].size, _ob_total(s, g)
    whole_a, d_arena = _walled(size)
    whole_o, d_obs = _walled(total)
    out = m.bao.ingest_slices(s["ctx"], d_arena, s["offsets"], s["lens"], d_obs, s["roots"], s["files"], s["chunks"], s["every"], group_log=g)
    st = out["sample_status"]
    assert st.is_cuda and st.dtype == torch.int32 and st.numel() == s["files"].size
    bad = torch.nonzero(st).flatten()[:10].tolist()
    assert not bad, [(int(s["files"][i]), int(s["chunks"][i]), int(st[i].item())) for i in bad]
    got = d_arena.cpu().numpy()
    assert (got[s["in_file"]] == s["arena"][s["in_file"]]).all(), "a file differs from the source"
    assert (got[~s["in_file"]] == FILL).all(), "a byte between the files was written"
    assert _walls_intact(whole_a, size) and _walls_intact(whole_o, total)
    assert torch.equal(d_obs, s["made"][g]["outboards"][:total]), f"g = {g}: the received outboards are not the provider's"
    print(f"g = {g}: {s['files'].size} slices of {len(s['lens'])} files, {int(s['in_file'].sum())} bytes and {total} outboard bytes compared")


@pytest.mark.parametrize("lanes", ["1", "4", "16"])
def test_every_lane_count_places_the_same_bytes(lanes, monkeypatch):
    """the kernel's three instantiations (the host picks one from the batch's longest path; B3W_SLICE_INGEST_LANES is the measurement
    switch): every chunk of every file at g = 4, the same files and outboards"""
    import torch
    s = _setup()
    m = s["m"]
    monkeypatch.setenv("B3W_SLICE_INGEST_LANES", lanes)
    g = 4
    size, total = s["arena"].size, _ob_total(s, g)
    whole_a, d_arena = _walled(size)
    whole_o, d_obs = _walled(total)
    st = m.bao.ingest_slices(s["ctx"], d_arena, s["offsets"], s["lens"], d_obs, s["roots"], s["files"], s["chunks"], s["every"], group_log=g)["sample_status"]
    assert not st.any().item()
    got = d_arena.cpu().numpy()
    assert (got[s["in_file"]] == s["arena"][s["in_file"]]).all() and (got[~s["in_file"]] == FILL).all()
    assert torch.equal(d_obs, s["made"][g]["outboards"][:total])
    assert _walls_intact(whole_a, size) and _walls_intact(whole_o, total)


@pytest.mark.parametrize("g", GS)
def test_a_subset_with_duplicates_writes_what_the_host_call_writes(g):
    import torch
    s = _setup()
    m = s["m"]
    rng = np.random.default_rng(200 + g)
    files, chunks = _listed_samples(m, s["lens"], g, rng)
    assert len(set(zip(files.tolist(), chunks.tolist()))) < files.size and any(s["lens"][f] == 0 for f in files)
    slices = _source_slices(s, files, chunks)
    d_slices = torch.from_numpy(_packed(m, s["ln"], files, chunks, slices)).cuda()
    size, total = s["arena"].size, _ob_total(s, g)
    whole_a, d_arena = _walled(size)
    whole_o, d_obs = _walled(total)
    st = m.bao.ingest_slices(s["ctx"], d_arena, s["offsets"], s["lens"], d_obs, s["roots"], files, chunks, d_slices, group_log=g)["sample_status"]
    want_arena, want_obs, want_st = _host_ingest(s, g, files, chunks, slices, s["roots_host"])
    assert not want_st.any() and not st.any().item()
    got_arena, got_obs = d_arena.cpu().numpy(), d_obs.cpu().numpy()
    assert (got_arena == want_arena).all() and (got_obs == want_obs).all()
    assert (want_arena == FILL).sum() > size // 2 and (want_obs == FILL).any()          # (a subset: most of both is still the fill)
    assert _walls_intact(whole_a, size) and _walls_intact(whole_o, total)
    if g == 0:                                                            # what came in verifies where it lies, against the nodes that came with it
        big = [i for i, f in enumerate(files.tolist()) if m.bao.num_chunks(s["lens"][f]) > 64]
        assert len(big) > 20
        res = m.bao.verify_ranges_batch(s["ctx"], d_arena, s["offsets"], s["lens"], d_obs, s["roots"], files[big], chunks[big], np.ones(len(big), dtype=np.uint64))
        assert not res["range_status"].any().item(), res["range_status"].cpu().numpy()


TAMPERS = ["header", "first node", "last node", "chunk byte", "root"]


@pytest.mark.parametrize("g,lanes", [(0, None), (4, "16"), (0, "1")])
@pytest.mark.parametrize("what", TAMPERS)
def test_a_tampered_slice_writes_nothing_and_the_others_land_whole(what, g, lanes, monkeypatch):
    import torch
    s = _setup()
    m = s["m"]
    if lanes is not None:
        monkeypatch.setenv("B3W_SLICE_INGEST_LANES", lanes)
    rng = np.random.default_rng(300 + g)
    files, chunks = _listed_samples(m, s["lens"], g, rng, dups=0)
    # the victim: a chunk listed once, with a path of several nodes and bytes of its own; its good slice once more at the end
    # (of a file whose place in the arena no other file shares: the world lists one file twice)
    n_of = [m.bao.num_chunks(x) for x in s["lens"]]
    alone = [int((s["offsets"] == o).sum()) == 1 for o in s["offsets"]]
    v = next(i for i, (f, c) in enumerate(zip(files.tolist(), chunks.tolist())) if n_of[f] > 64 and alone[f] and 0 < c < n_of[f] - 1)
    files, chunks = np.append(files, files[v]), np.append(chunks, chunks[v])
    f, c = int(files[v]), int(chunks[v])
    slices = _source_slices(s, files, chunks)
    P = len(R.path_nodes(c, n_of[f]))
    roots = s["roots_host"].copy()
    at, want_v = {"header": (3, 3), "first node": (8 + 21, 2), "last node": (8 + 64 * (P - 1) + 40, 2), "chunk byte": (8 + 64 * P + 500, 1), "root": (None, 2)}[what]
    if at is None:
        roots[f, 3] ^= 0x10000                                            # every sample of the victim's file fails; the other files' land
    else:
        sl = bytearray(slices[v])
        sl[at] ^= 1
        slices[v] = bytes(sl)
    d_roots = torch.from_numpy(roots.view(np.int32)).cuda()
    d_slices = torch.from_numpy(_packed(m, s["ln"], files, chunks, slices)).cuda()
    size, total = s["arena"].size, _ob_total(s, g)
    whole_a, d_arena = _walled(size)
    whole_o, d_obs = _walled(total)
    st = m.bao.ingest_slices(s["ctx"], d_arena, s["offsets"], s["lens"], d_obs, d_roots, files, chunks, d_slices, group_log=g)["sample_status"].cpu().numpy()
    planned = m.bao.plan_samples_slices(s["ctx"], s["lens"], d_roots, files, chunks, d_slices)["sample_status"]
    decoded = np.array([m.bao.decode_slice(sl, s["lens"][ff], cc, roots[ff])[0] for ff, cc, sl in zip(files.tolist(), chunks.tolist(), slices)])
    assert (st == planned).all() and (st == decoded).all()
    assert st[v] == want_v
    failed = (files == f) if at is None else (np.arange(files.size) == v)
    assert (st[failed] != 0).all() and (st[~failed] == 0).all()
    want_arena, want_obs, want_st = _host_ingest(s, g, files, chunks, slices, roots)
    assert (want_st == st).all()
    got_arena, got_obs = d_arena.cpu().numpy(), d_obs.cpu().numpy()
    assert (got_arena == want_arena).all() and (got_obs == want_obs).all()
    assert _walls_intact(whole_a, size) and _walls_intact(whole_o, total)
    a = int(s["offsets"][f]) + c * K
    if at is None:                                                        # nothing of the victim's file, header included
        o = int(s["made"][g]["ob_first"][f])
        assert (got_arena[a:a + K] == FILL).all() and (got_obs[o:o + 8] == FILL).all()
    else:                                                                 # the good slice of the same chunk left its bytes
        assert (got_arena[a:a + K] == s["arena"][a:a + K]).all()


def _sparse_file(n, chosen, rng):
    """a file of n chunks of which only the chunks `chosen` (index -> bytes) are known: their chunk CVs, arbitrary CVs for every subtree
    without a chosen chunk, parents hashed up to a root -> (root words, {pre-order index: node bytes} of the nodes above chosen chunks)"""
    nodes = {}

    def walk(first, m, pos, root):
        if not any(first <= c < first + m for c in chosen):
            return [int(x) for x in rng.integers(0, 1 << 32, 8)]
        if m == 1:
            return B.chunk_cv(chosen[first], first, root)
        k = R._split(m)
        left, right = walk(first, k, pos + 1, False), walk(first + k, m - k, pos + k, False)
        nodes[pos] = struct.pack("<16I", *(left + right))
        return B.compress(B.IV, left + right, 0, 64, B.PARENT | (B.ROOT if root else 0))[:8]
    return walk(0, n, 0, True), nodes


def test_places_past_4_gib():
    """one fictitious file of 5 GiB + 300 B in an arena that is never initialised: chunk 0, a chunk past the 4 GiB mark and the ragged last
    chunk, their slices built on the host; only their own places are read back"""
    import torch
    s = _setup()
    m = s["m"]
    length = (5 << 30) + 300
    n = m.bao.num_chunks(length)
    rng = np.random.default_rng(64)
    picks = [0, (4 << 20) + 12345, n - 1]
    chosen = {c: rng.integers(0, 256, min(K, length - c * K), dtype=np.uint8).tobytes() for c in picks}
    assert len(chosen[n - 1]) == 300
    root, nodes = _sparse_file(n, chosen, rng)
    header = struct.pack("<Q", length)
    order = [picks[1], picks[2], picks[0]]
    slices = [header + b"".join(nodes[i] for i in R.path_nodes(c, n)) + chosen[c] for c in order]
    assert [m.bao.decode_slice(sl, length, c, root)[0] for c, sl in zip(order, slices)] == [0, 0, 0]
    files, chunks = np.zeros(3, dtype=np.uint32), np.array(order, dtype=np.uint64)
    d_slices = torch.from_numpy(_packed(m, np.array([length], dtype=np.uint64), files, chunks, slices)).cuda()
    d_roots = torch.from_numpy(np.array(root, dtype=np.uint32).view(np.int32)).cuda()
    skew = 1                                                              # the file starts at an odd byte of the arena
    d_arena = torch.empty(length + 16, dtype=torch.uint8, device="cuda")
    d_obs = torch.empty(m.bao.outboard_size(length), dtype=torch.uint8, device="cuda")
    st = m.bao.ingest_slices(s["ctx"], d_arena, [skew], [length], d_obs, d_roots, files, chunks, d_slices)["sample_status"]
    assert st.cpu().tolist() == [0, 0, 0]
    assert d_obs[:8].cpu().numpy().tobytes() == header
    for c in picks:
        a = skew + c * K
        assert d_arena[a:a + len(chosen[c])].cpu().numpy().tobytes() == chosen[c], c
        for i in R.path_nodes(c, n):
            assert d_obs[8 + 64 * i:8 + 64 * i + 64].cpu().numpy().tobytes() == nodes[i], (c, i)
    del d_arena, d_obs


def _c_call(s, g, d_arena, arena_bytes, d_obs, d_roots, files, chunks, n_samples, d_slices, d_st, offsets=True, lens=True, ctx=True):
    import torch
    L = s["m"].lib()
    ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr())
    return L.b3w_bao_slice_ingest_device(s["ctx"].handle if ctx else None, ptr(d_arena), arena_bytes, s["offsets"].ctypes.data if offsets else None,
                                         s["ln"].ctypes.data if lens else None, len(s["lens"]), g, ptr(d_obs), ptr(d_roots),
                                         None if files is None else files.ctypes.data, None if chunks is None else chunks.ctypes.data, n_samples, ptr(d_slices),
                                         ptr(d_st), torch.cuda.current_stream().cuda_stream)


def test_the_call_allocates_nothing():
    import torch
    s = _setup()
    g = 0
    _, d_arena = _walled(s["arena"].size)
    _, d_obs = _walled(_ob_total(s, g))
    d_st = torch.full((s["files"].size,), -1, dtype=torch.int32, device="cuda")
    args = (s, g, d_arena, d_arena.numel(), d_obs, s["roots"], s["files"], s["chunks"], s["files"].size, s["every"], d_st)
    assert _c_call(*args) == 0, s["ctx"].last_error()                     # (the context's staging grows here, outside the allocator)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    assert _c_call(*args) == 0, s["ctx"].last_error()
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == before
    assert not d_st.any().item()


def test_refusals_leave_every_output_untouched():
    import torch
    s = _setup()
    m = s["m"]
    g = 0
    size, total = s["arena"].size, _ob_total(s, g)
    whole_a, d_arena = _walled(size)
    whole_o, d_obs = _walled(total)
    k = 64
    files, chunks = s["files"][:k].copy(), s["chunks"][:k].copy()
    slices = _source_slices(s, files, chunks)
    d_slices = torch.from_numpy(_packed(m, s["ln"], files, chunks, slices)).cuda()
    d_st = torch.full((k,), -1, dtype=torch.int32, device="cuda")
    good = dict(g=g, d_arena=d_arena, arena_bytes=size, d_obs=d_obs, d_roots=s["roots"], files=files, chunks=chunks, n_samples=k, d_slices=d_slices, d_st=d_st)

    def refused(**change):
        kw = dict(good)
        kw.update(change)
        rc = _c_call(s, **kw)
        torch.cuda.synchronize()
        untouched = bool((d_arena == FILL).all().item()) and bool((d_obs == FILL).all().item()) and bool((d_st == -1).all().item())
        return rc == BAD and untouched
    assert refused(ctx=False)
    assert refused(g=7)
    for name in ("d_arena", "d_obs", "d_roots", "files", "chunks", "d_slices", "d_st"):
        assert refused(**{name: None}), name
    assert refused(offsets=False) and refused(lens=False)
    assert refused(d_obs=d_obs.data_ptr() + 4), "an outboard buffer that is not 8-byte aligned"
    assert refused(d_slices=d_slices.data_ptr() + 8), "slices that are not 16-byte aligned"
    bad_file, bad_chunk = files.copy(), chunks.copy()
    bad_file[-1] = len(s["lens"])                                         # a bad index behind good samples
    bad_chunk[-1] = m.bao.num_chunks(s["lens"][int(files[-1])])
    assert refused(files=bad_file) and refused(chunks=bad_chunk)
    reach = max(int(s["offsets"][f]) + s["lens"][f] for f in files.tolist())
    assert refused(arena_bytes=reach - 1), "a sampled file that reaches past arena_bytes"
    with pytest.raises(m.B3WError):
        m.bao.ingest_slices(s["ctx"], d_arena, s["offsets"], s["lens"], d_obs, s["roots"], files, chunks, d_slices, group_log=7)
    # no samples: a no-op, whatever else is handed in
    assert _c_call(s, g, None, 0, None, None, None, None, 0, None, None) == 0
    torch.cuda.synchronize()
    assert bool((d_arena == FILL).all().item()) and bool((d_obs == FILL).all().item())
    # and the same arguments unchanged are taken
    assert _c_call(s, **good) == 0, s["ctx"].last_error()
    torch.cuda.synchronize()
    assert not d_st.any().item() and _walls_intact(whole_a, size) and _walls_intact(whole_o, total)
    a = int(s["offsets"][int(files[0])]) + int(chunks[0]) * K
    b = min(a + K, int(s["offsets"][int(files[0])]) + s["lens"][int(files[0])])
    assert torch.equal(d_arena[a:b], s["d_src"][a:b])
