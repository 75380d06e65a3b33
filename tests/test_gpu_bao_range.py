"""Range slices on the device (bao.range_slices_arena, bao.ingest_range_slices; b3w_bao_range_slice_arena_device,
b3w_bao_range_slice_ingest_device): the slice of a run of chunks extracted where the files lie and taken in again.  The arena and the
provider's side are test_gpu_bao_ingest._setup()'s (test_gpu_bao_slices._world() with the six files of that module behind it: starts at
4, 8, 12 modulo 16 and at odd bytes, 1 024 * 1 025 and 2^20 + 300 bytes among them).  The provider is held against the restatement
(tests/bao_range_ref.py) byte for byte; the receiver against the host call (b3w_bao_range_slice_ingest, itself held against the
projections on the CPU), against the projections through the one-chunk device call, and against the source's bytes and the provider's
outboards; receivers start from 0xEE between 0xA5 guards and hold only the roots."""
import functools
import struct

import numpy as np
import pytest

import b3w_testlib as T
import bao_range_ref as RR
import bao_ref as R
import blake3_ref as B
from test_bao_range_cpu import _long_ranges, _tampers
from test_gpu_bao_ingest import BAD, FILL, GS, GUARD, K, _ob_total, _packed, _setup, _walled, _walls_intact

pytestmark = pytest.mark.gpu

LENGTHS_DRAWN = [1, 2, 5, 63, 64, 65, 1023, 1024, 1025]
PAD = 0x5C


@pytest.fixture(scope="module", autouse=True)
def _a_memory_pool_of_its_own():
    """as test_gpu_bao_ingest does it: the module's device tensors come from a pool of its own and go with it"""
    import gc
    import torch
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        torch.cuda.synchronize()
        if _setup.cache_info().currsize:
            _setup()["ctx"].close()
        _setup.cache_clear()
        _expected.cache_clear()
        gc.collect()
    del pool


def _data(s, f):
    a = int(s["offsets"][f])
    return s["arena"][a:a + s["lens"][f]].tobytes()


@functools.lru_cache(maxsize=None)
def _expected(f, a, k):
    """the restatement's slice of chunks [a, a + k) of file f, and its places (computed once, left unchanged)"""
    s = _setup()
    data = _data(s, f)
    key = ("world", hash(data))
    RR.seed(data, key)
    return RR.encode(data, a, k, key=key)


def _arrays(ranges):
    return (np.array([r[0] for r in ranges], dtype=np.uint32), np.array([r[1] for r in ranges], dtype=np.uint64),
            np.array([r[2] for r in ranges], dtype=np.uint64))


def _pack(m, ln, ranges, slices):
    """the slices packed as range_slice_layout says, the padding 0x5C -> (numpy, slice_first)"""
    files, first, count = _arrays(ranges)
    sf = m.bao.range_slice_layout(ln, files, first, count)
    out = np.full(int(sf[-1]), PAD, dtype=np.uint8)
    for at, sl in zip(sf[:-1], slices):
        out[int(at):int(at) + len(sl)] = np.frombuffer(sl, dtype=np.uint8)
    return out, sf


def _provide(s, g, ranges):
    """the device provider into 0x5C between guards -> (the packed slices on the device, slice_first, the slices as bytes)"""
    import torch
    m = s["m"]
    files, first, count = _arrays(ranges)
    sf = m.bao.range_slice_layout(s["ln"], files, first, count)
    total = int(sf[-1])
    whole = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    d_slices = whole[GUARD:GUARD + total]
    d_slices.fill_(PAD)
    rc = m.lib().b3w_bao_range_slice_arena_device(s["ctx"].handle, s["d_src"].data_ptr(), s["d_src"].numel(), s["offsets"].ctypes.data, s["ln"].ctypes.data,
                                                  len(s["lens"]), g, s["made"][g]["outboards"].data_ptr(), files.ctypes.data, first.ctypes.data,
                                                  count.ctypes.data, len(ranges), d_slices.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, s["ctx"].last_error()
    torch.cuda.synchronize()
    assert _walls_intact(whole, total)
    host = d_slices.cpu().numpy()
    sizes = [m.bao.range_slice_size(s["lens"][f], a, k) for f, a, k in ranges]
    covered = np.zeros(total, dtype=bool)
    for at, size in zip(sf[:-1], sizes):
        covered[int(at):int(at) + size] = True
    assert (host[~covered] == PAD).all()                                   # the padding is not written
    return d_slices, sf, [host[int(at):int(at) + size].tobytes() for at, size in zip(sf[:-1], sizes)]


def _test_ranges(n):
    """the CPU test's kinds: every single chunk of the files up to 70 chunks (the ends and the tile boundary of the longer ones), the whole
    file, the splits, the ragged end, the group boundaries, the tile boundary"""
    singles = range(n) if n <= 70 else sorted({0, 1, 63, 64, 1023, 1024, n - 1} & set(range(n)))
    return sorted(set(_long_ranges(n)) | {(c, 1) for c in singles})


@pytest.mark.parametrize("g", GS)
def test_the_provider_equals_the_restatement(g):
    s = _setup()
    m = s["m"]
    ranges = [(f, a, k) for f, ln in enumerate(s["lens"]) for a, k in _test_ranges(m.bao.num_chunks(ln))]
    perm = np.random.default_rng(300 + g).permutation(len(ranges))
    ranges = [ranges[i] for i in perm]
    _, _, got = _provide(s, g, ranges)
    for (f, a, k), sl in zip(ranges, got):
        assert sl == _expected(f, a, k)[0], (g, f, a, k)


def _partition(n, rng):
    """[(first, count)] that covers [0, n): lengths drawn from LENGTHS_DRAWN, the rest at the end"""
    out, at = [], 0
    while at < n:
        k = int(rng.choice(LENGTHS_DRAWN))
        if at + k > n or rng.random() < 0.05:
            k = n - at
        out.append((at, k))
        at += k
    return out


def _receiver(s, g, with_have=True, seed=5):
    import torch
    size, total = s["arena"].size, _ob_total(s, g)
    whole_a, d_arena = _walled(size)
    whole_o, d_obs = _walled(total)
    words = int(s["m"].bao.have_layout(s["lens"])[-1])
    pre = np.random.default_rng(seed).integers(0, 1 << 63, words, dtype=np.int64)
    valid = _have_bits(s, [(f, 0, s["m"].bao.num_chunks(ln)) for f, ln in enumerate(s["lens"])])
    pre &= valid                                                           # (the pad bits are the library's to leave clear)
    d_have = torch.from_numpy(pre.copy()).cuda() if with_have else None
    return dict(whole_a=whole_a, d_arena=d_arena, whole_o=whole_o, d_obs=d_obs, d_have=d_have, pre=pre, size=size, total=total)


def _have_bits(s, ranges):
    """the bitmap (int64 words) with the chunks of these (file, first, count) set"""
    wf = s["m"].bao.have_layout(s["lens"])
    out = np.zeros(int(wf[-1]), dtype=np.uint64)
    for f, a, k in ranges:
        for c in range(a, a + k):
            out[int(wf[f]) + (c >> 6)] |= np.uint64(1) << np.uint64(c & 63)
    return out.view(np.int64)


def _ingest(s, g, r, ranges, d_slices):
    files, first, count = _arrays(ranges)
    return s["m"].bao.ingest_range_slices(s["ctx"], r["d_arena"], s["offsets"], s["lens"], r["d_obs"], s["roots"], files, first, count, d_slices,
                                          group_log=g, d_have=r["d_have"])


@pytest.mark.parametrize("g", GS)
def test_every_file_received_as_a_shuffled_partition(g):
    import torch
    s = _setup()
    m = s["m"]
    rng = np.random.default_rng(400 + g)
    ranges = [(f, a, k) for f, ln in enumerate(s["lens"]) for a, k in _partition(m.bao.num_chunks(ln), rng)]
    for i in rng.choice(len(ranges), 12, replace=False):                  # some twice, some overlapping their neighbours
        f, a, k = ranges[i]
        n = m.bao.num_chunks(s["lens"][f])
        ranges.append((f, a, k))
        ranges.append((f, max(0, a - 3), min(n, a + k + 2) - max(0, a - 3)))
    ranges = [ranges[i] for i in rng.permutation(len(ranges))]
    d_slices, _, _ = _provide(s, g, ranges)
    r = _receiver(s, g)
    out = _ingest(s, g, r, ranges, d_slices)
    st, fb = out["range_status"], out["range_first_bad"]
    assert st.dtype == torch.int32 and st.numel() == len(ranges) and not st.any().item()
    assert bool((fb == -1).all().item())
    got = r["d_arena"].cpu().numpy()
    assert (got[s["in_file"]] == s["arena"][s["in_file"]]).all() and (got[~s["in_file"]] == FILL).all()
    assert torch.equal(r["d_obs"], s["made"][g]["outboards"][:r["total"]])
    everything = _have_bits(s, [(f, 0, m.bao.num_chunks(ln)) for f, ln in enumerate(s["lens"])])
    assert (r["d_have"].cpu().numpy() == (r["pre"] | everything)).all()
    assert _walls_intact(r["whole_a"], r["size"]) and _walls_intact(r["whole_o"], r["total"])


def _host_ingest(s, g, ranges, slices, roots):
    """the host call over the same ranges in order -> (arena, outboards, have, statuses, first bad) from buffers of 0xEE"""
    m = s["m"]
    ob_first, wf = s["made"][g]["ob_first"], m.bao.have_layout(s["lens"])
    arena, obs = np.full(s["arena"].size, FILL, dtype=np.uint8), np.full(_ob_total(s, g), FILL, dtype=np.uint8)
    have = np.zeros(int(wf[-1]), dtype=np.uint64)
    st, fb = [], []
    for (f, a, k), sl in zip(ranges, slices):
        o, ln = int(s["offsets"][f]), s["lens"][f]
        x, y = m.bao.ingest_range_slice_host(arena[o:o + ln], obs[int(ob_first[f]):int(ob_first[f + 1])], ln, a, k, roots[f], sl, g,
                                             have[int(wf[f]):int(wf[f + 1])])
        st.append(x)
        fb.append(-1 if y is None else y)
    return arena, obs, have.view(np.int64), st, fb


def _same_as_host(s, g, r, out, ranges, slices, roots):
    want_arena, want_obs, want_have, want_st, want_fb = _host_ingest(s, g, ranges, slices, roots)
    assert out["range_status"].cpu().tolist() == want_st and out["range_first_bad"].cpu().tolist() == want_fb
    assert (r["d_arena"].cpu().numpy() == want_arena).all() and (r["d_obs"].cpu().numpy() == want_obs).all()
    assert (r["d_have"].cpu().numpy() == (r["pre"] | want_have)).all()
    assert _walls_intact(r["whole_a"], r["size"]) and _walls_intact(r["whole_o"], r["total"])
    return want_st


@pytest.mark.parametrize("g", GS)
def test_a_third_of_each_file_against_the_host_call_and_the_projections(g):
    import torch
    s = _setup()
    m = s["m"]
    ranges = []
    for f, ln in enumerate(s["lens"]):
        n = m.bao.num_chunks(ln)
        k = max(1, n // 3)
        a = (n - k) // 2 + (1 if n > 4 else 0)                            # (off the tile and group boundaries)
        ranges += [(f, a, min(k, n - a))] + ([(f, n - 1, 1)] if n > 1 and a + k < n else [])
    d_slices, _, slices = _provide(s, g, ranges)
    r = _receiver(s, g)
    out = _ingest(s, g, r, ranges, d_slices)
    assert not any(_same_as_host(s, g, r, out, ranges, slices, s["roots_host"]))
    # the projections through the one-chunk device call write the same bytes
    files = np.concatenate([np.full(k, f, dtype=np.uint32) for f, a, k in ranges])
    chunks = np.concatenate([np.arange(a, a + k, dtype=np.uint64) for f, a, k in ranges])
    proj = [RR.project(sl, _expected(f, a, k)[1], s["lens"][f], c) for (f, a, k), sl in zip(ranges, slices) for c in range(a, a + k)]
    p = _receiver(s, g)
    st = m.bao.ingest_slices(s["ctx"], p["d_arena"], s["offsets"], s["lens"], p["d_obs"], s["roots"], files, chunks,
                             torch.from_numpy(_packed(m, s["ln"], files, chunks, proj)).cuda(), group_log=g, d_have=p["d_have"])["sample_status"]
    assert not st.any().item()
    assert torch.equal(p["d_arena"], r["d_arena"]) and torch.equal(p["d_obs"], r["d_obs"]) and torch.equal(p["d_have"], r["d_have"])


@pytest.mark.parametrize("g", [0, 4])
def test_tampered_ranges_beside_good_ones(g):
    import torch
    s = _setup()
    m = s["m"]
    big = s["lens"].index(K * 1025)
    mid = s["lens"].index(70 * K + 1)
    victims = [(big, 1022, 3), (big, 1000, 25), (mid, 3, 66), (mid, 69, 2)]
    ranges, slices, roots = [], [], []
    for f, a, k in victims:
        sl, places = _expected(f, a, k)
        for what, bad_sl, rt, _ in _tampers(sl, places, a, k, s["lens"][f], [int(x) for x in s["roots_host"][f]]):
            if what != "root":                                            # (the roots are the call's, one a file: see below)
                ranges.append((f, a, k))
                slices.append(bad_sl)
    good = [(big, 0, 1025), (mid, 0, 10), (big, 1020, 5), (mid, 60, 11)]   # beside them, and over the tampered chunks
    ranges += good
    slices += [_expected(f, a, k)[0] for f, a, k in good]
    order = np.random.default_rng(600 + g).permutation(len(ranges))
    ranges, slices = [ranges[i] for i in order], [slices[i] for i in order]
    packed, _ = _pack(m, s["ln"], ranges, slices)
    r = _receiver(s, g)
    out = _ingest(s, g, r, ranges, torch.from_numpy(packed).cuda())
    st = _same_as_host(s, g, r, out, ranges, slices, s["roots_host"])
    assert sorted(set(st)) == [0, 1, 2, 3] and all(st[i] == 0 for i, x in enumerate(ranges) if x in good)
    for f in (big, mid):                                                  # the good ranges left every byte of the two files
        o = int(s["offsets"][f])
        assert torch.equal(r["d_arena"][o:o + s["lens"][f]], s["d_src"][o:o + s["lens"][f]])
    # a wrong root: every range of that file is 2 (1 for a one-chunk file) and writes nothing
    roots = s["roots"].clone()
    roots.view(-1)[8 * mid + 3] ^= 0x10000
    one = s["lens"].index(next(ln for ln in s["lens"] if 0 < ln <= K))
    roots.view(-1)[8 * one] ^= 1
    ranges = [(mid, 0, 71), (mid, 5, 1), (one, 0, 1), (big, 7, 2)]
    d_slices, _, slices = _provide(s, g, ranges)
    r = _receiver(s, g)
    files, first, count = _arrays(ranges)
    out = m.bao.ingest_range_slices(s["ctx"], r["d_arena"], s["offsets"], s["lens"], r["d_obs"], roots, files, first, count, d_slices, group_log=g,
                                    d_have=r["d_have"])
    assert out["range_status"].cpu().tolist() == [2, 2, 1, 0] and out["range_first_bad"].cpu().tolist() == [0, 5, 0, -1]
    _same_as_host(s, g, r, out, ranges, slices, roots.cpu().numpy().view(np.uint32).reshape(-1, 8))


@pytest.mark.parametrize("g", [0, 4])
def test_the_loop_closes_with_ranges(g):
    """test_gpu_bao_have's loop with ranges in place of runs_chunks: have_runs -> the rows on the host -> range_slices_arena ->
    ingest_range_slices, 30 % of the slices tampered in the first round"""
    import torch
    s = _setup()
    m = s["m"]
    r = _receiver(s, g)
    r["d_have"].zero_()
    rng = np.random.default_rng(700 + g)
    # a first arrival of scattered chunks, so that the missing runs have every shape
    every = [(f, c, 1) for f, ln in enumerate(s["lens"]) for c in range(m.bao.num_chunks(ln)) if rng.random() < 0.4]
    d_slices, _, _ = _provide(s, g, every)
    assert not _ingest(s, g, r, every, d_slices)["range_status"].any().item()
    rounds = 0
    while True:
        runs = m.bao.have_runs(s["ctx"], r["d_have"], s["lens"], kind="missing")
        ranges = list(zip(runs["files"].tolist(), runs["first_chunks"].tolist(), runs["n_chunks"].tolist()))
        if not ranges:
            break
        assert rounds < 4
        d_slices, sf, _ = _provide(s, g, ranges)
        bad = np.zeros(len(ranges), dtype=bool)
        if rounds == 0:                                                   # (an empty file's slice has no byte behind the header)
            bad = (rng.random(len(ranges)) < 0.3) & np.array([m.bao.range_slice_size(s["lens"][f], a, k) > 8 for f, a, k in ranges])
            at = torch.from_numpy(np.array([int(sf[i]) + 8 for i in np.flatnonzero(bad)], dtype=np.int64)).cuda()
            d_slices[at] ^= 1                                             # the first byte behind the header: the root node, or the only chunk
        st = _ingest(s, g, r, ranges, d_slices)["range_status"].cpu().numpy()
        assert ((st != 0) == bad).all()
        rounds += 1
    assert rounds >= 2
    n_chunks = [m.bao.num_chunks(ln) for ln in s["lens"]]
    assert runs["file_have"].cpu().tolist() == n_chunks and int(runs["n_runs"].item()) == 0
    got = r["d_arena"].cpu().numpy()
    assert (got[s["in_file"]] == s["arena"][s["in_file"]]).all() and (got[~s["in_file"]] == FILL).all()
    assert torch.equal(r["d_obs"], s["made"][g]["outboards"][:r["total"]])
    present = m.bao.have_runs(s["ctx"], r["d_have"], s["lens"], kind="present")
    ver = m.bao.verify_ranges_batch(s["ctx"], r["d_arena"], s["offsets"], s["lens"], r["d_obs"], s["roots"], present["files"], present["first_chunks"],
                                    present["n_chunks"], group_log=g)
    assert not ver["range_status"].any().item()
    assert _walls_intact(r["whole_a"], r["size"]) and _walls_intact(r["whole_o"], r["total"])


def test_4096_ranges_of_2_chunks_in_one_call():
    import torch
    s = _setup()
    m = s["m"]
    rng = np.random.default_rng(800)
    bigs = [f for f, ln in enumerate(s["lens"]) if m.bao.num_chunks(ln) >= 1025]
    ranges = [(int(rng.choice(bigs)), int(rng.integers(0, 1024)), 2) for _ in range(4096)]
    d_slices, _, _ = _provide(s, 0, ranges)
    r = _receiver(s, 0)
    out = _ingest(s, 0, r, ranges, d_slices)
    assert not out["range_status"].any().item() and bool((out["range_first_bad"] == -1).all().item())
    want = np.full(s["arena"].size, FILL, dtype=np.uint8)
    for f, a, k in set(ranges):
        o = int(s["offsets"][f])
        lo, hi = o + a * K, o + min(s["lens"][f], (a + k) * K)
        want[lo:hi] = s["arena"][lo:hi]
    assert (r["d_arena"].cpu().numpy() == want).all()
    assert (r["d_have"].cpu().numpy() == (r["pre"] | _have_bits(s, set(ranges)))).all()
    assert _walls_intact(r["whole_a"], r["size"]) and _walls_intact(r["whole_o"], r["total"])


def _fabricate(length, a, k, chosen, rng):
    """the slice of chunks [a, a + k) of a file of which only those chunks (index -> bytes) are known: arbitrary CVs for every subtree that
    does not meet the range, parents hashed up to a root -> (slice, root words, {(lo, size): node bytes})"""
    n = R.num_chunks(length)
    out, nodes = [struct.pack("<Q", length)], {}

    def walk(lo, m, root):
        if lo >= a + k or lo + m <= a:
            return [int(x) for x in rng.integers(0, 1 << 32, 8)]
        if m == 1:
            out.append(chosen[lo])
            return B.chunk_cv(chosen[lo], lo, root)
        at = len(out)
        out.append(None)
        split = R._split(m)
        left = walk(lo, split, False)
        right = walk(lo + split, m - split, False)
        out[at] = nodes[(lo, m)] = struct.pack("<16I", *(left + right))
        return B.compress(B.IV, left + right, 0, 64, B.PARENT | (B.ROOT if root else 0))[:8]
    root = walk(0, n, True)
    return b"".join(out), root, nodes


def test_places_past_4_gib():
    """one fictitious file of 5 GiB + 300 B in an arena that is never initialised: a range across chunk 2^22 (the 4 GiB offset) and one onto
    the ragged last chunk, their slices built on the host with blake3_ref; only their own places are read back"""
    import torch
    s = _setup()
    m = s["m"]
    length = (5 << 30) + 300
    n = m.bao.num_chunks(length)
    rng = np.random.default_rng(64)
    ranges = [(0, (1 << 22) - 3, 7), (0, n - 2, 2)]
    parts = []
    for _, a, k in ranges:
        chosen = {c: rng.integers(0, 256, min(K, length - c * K), dtype=np.uint8).tobytes() for c in range(a, a + k)}
        parts.append((chosen,) + _fabricate(length, a, k, chosen, rng))
    # each range is made under a tree of its own (the subtrees beside it are arbitrary): two files of the same length in one arena
    lens = np.array([length, length], dtype=np.uint64)
    ranges = [(0,) + ranges[0][1:], (1,) + ranges[1][1:]]
    slices = [p[1] for p in parts]
    assert [m.bao.decode_range_slice(sl, length, a, k, p[2])[:2] for (_, a, k), sl, p in zip(ranges, slices, parts)] == [(0, None), (0, None)]
    packed, _ = _pack(m, lens, ranges, slices)
    d_roots = torch.from_numpy(np.array([p[2] for p in parts], dtype=np.uint32).view(np.int32)).cuda()
    skew = 1                                                              # the files start at an odd byte of the arena (and overlap: one arena)
    d_arena = torch.empty(length + 16, dtype=torch.uint8, device="cuda")
    ob_first = m.bao.batch_layout(lens)
    d_obs = torch.empty(int(ob_first[-1]), dtype=torch.uint8, device="cuda")
    d_have = m.bao.have_new(lens)
    files, first, count = _arrays(ranges)
    out = m.bao.ingest_range_slices(s["ctx"], d_arena, [skew, skew], lens, d_obs, d_roots, files, first, count, torch.from_numpy(packed).cuda(), d_have=d_have)
    assert out["range_status"].cpu().tolist() == [0, 0] and out["range_first_bad"].cpu().tolist() == [-1, -1]
    wf = m.bao.have_layout(lens)
    for (f, a, k), (chosen, _, _, nodes) in zip(ranges, parts):
        o = int(ob_first[f])
        assert d_obs[o:o + 8].cpu().numpy().tobytes() == struct.pack("<Q", length)
        for (lo, size), node in nodes.items():
            i = _preorder(n, lo, size)
            assert d_obs[o + 8 + 64 * i:o + 8 + 64 * i + 64].cpu().numpy().tobytes() == node, (f, lo, size)
    # (the two ranges' chunks share no place of the arena)
    for (f, a, k), (chosen, _, _, _) in zip(ranges, parts):
        for c in range(a, a + k):
            at = skew + c * K
            assert d_arena[at:at + len(chosen[c])].cpu().numpy().tobytes() == chosen[c], (f, c)
            assert (int(d_have[int(wf[f]) + (c >> 6)].item()) >> (c & 63)) & 1
    assert int((d_have != 0).sum().item()) <= 4
    del d_arena, d_obs


def _preorder(n, lo, size):
    """pre-order index of the node over [lo, lo + size) of a tree over n chunks"""
    p, first, m = 0, 0, n
    while (first, m) != (lo, size):
        k = R._split(m)
        if lo < first + k:
            p, m = p + 1, k
        else:
            p, first, m = p + k, first + k, m - k
    return p


def _c_ingest(s, g0, r, ranges, slices0, st0, fb0, scratch0, **change):
    import torch
    files, first, count = _arrays(ranges)
    kw = dict(ctx=s["ctx"].handle, d_arena=r["d_arena"].data_ptr(), arena_bytes=r["size"], offsets=s["offsets"].ctypes.data, lens=s["ln"].ctypes.data,
              n_files=len(s["lens"]), g=g0, d_obs=r["d_obs"].data_ptr(), d_roots=s["roots"].data_ptr(), files=files.ctypes.data, first=first.ctypes.data,
              count=count.ctypes.data, n_ranges=len(ranges), d_slices=slices0.data_ptr(), d_st=st0.data_ptr(), d_fb=fb0.data_ptr(),
              d_have=r["d_have"].data_ptr(), d_scratch=scratch0.data_ptr(), scratch_bytes=scratch0.numel())
    for name, value in change.items():
        kw[name] = value.ctypes.data if isinstance(value, np.ndarray) else value
    return s["m"].lib().b3w_bao_range_slice_ingest_device(*kw.values(), torch.cuda.current_stream().cuda_stream)


def _c_provide(s, g0, ranges, slices0, **change):
    import torch
    files, first, count = _arrays(ranges)
    kw = dict(ctx=s["ctx"].handle, d_arena=s["d_src"].data_ptr(), arena_bytes=s["d_src"].numel(), offsets=s["offsets"].ctypes.data, lens=s["ln"].ctypes.data,
              n_files=len(s["lens"]), g=g0, d_obs=s["made"][g0]["outboards"].data_ptr(), files=files.ctypes.data, first=first.ctypes.data,
              count=count.ctypes.data, n_ranges=len(ranges), d_slices=slices0.data_ptr())
    for name, value in change.items():
        kw[name] = value.ctypes.data if isinstance(value, np.ndarray) else value
    return s["m"].lib().b3w_bao_range_slice_arena_device(*kw.values(), torch.cuda.current_stream().cuda_stream)


def _some_ranges(s):
    m = s["m"]
    big = s["lens"].index(K * 1025)
    return [(big, 1000, 25), (big, 3, 1021), (0, 0, 1), (big, 1024, 1)] + [(f, 0, m.bao.num_chunks(ln)) for f, ln in enumerate(s["lens"]) if ln <= 40 * K][:8]


def test_the_two_calls_allocate_nothing():
    import torch
    s = _setup()
    m = s["m"]
    ranges = _some_ranges(s)
    files, first, count = _arrays(ranges)
    sf = m.bao.range_slice_layout(s["ln"], files, first, count)
    d_slices = torch.empty(int(sf[-1]), dtype=torch.uint8, device="cuda")
    r = _receiver(s, 0)
    d_st = torch.full((len(ranges),), -1, dtype=torch.int32, device="cuda")
    d_fb = torch.full((len(ranges),), -2, dtype=torch.int64, device="cuda")
    need = m.lib().b3w_bao_range_slice_ingest_scratch_bytes(s["ln"].ctypes.data, len(s["lens"]), files.ctypes.data, first.ctypes.data, count.ctypes.data, len(ranges))
    assert need == 16 * sum((a + k - 1) // (64 if k <= 64 else 1024) - a // (64 if k <= 64 else 1024) + 1 for _, a, k in ranges)
    d_scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    for _ in range(2):                                                    # (the context's staging grows in the first round, outside the allocator)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        assert _c_provide(s, 0, ranges, d_slices) == 0, s["ctx"].last_error()
        assert _c_ingest(s, 0, r, ranges, d_slices, d_st, d_fb, d_scratch) == 0, s["ctx"].last_error()
        torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == before
    assert not d_st.any().item() and bool((d_fb == -1).all().item())


def test_refusals_leave_every_output_and_the_scratch_untouched():
    import torch
    s = _setup()
    m = s["m"]
    g = 0
    ranges = _some_ranges(s)
    d_good, sf, _ = _provide(s, g, ranges)
    r = _receiver(s, g)
    d_st = torch.full((len(ranges),), -1, dtype=torch.int32, device="cuda")
    d_fb = torch.full((len(ranges),), -2, dtype=torch.int64, device="cuda")
    d_scratch = torch.full((16 * 64,), 0x77, dtype=torch.uint8, device="cuda")
    d_slices = torch.full((int(sf[-1]),), PAD, dtype=torch.uint8, device="cuda")
    pre = r["d_have"].clone()

    def untouched():
        torch.cuda.synchronize()
        return (bool((r["d_arena"] == FILL).all().item()) and bool((r["d_obs"] == FILL).all().item()) and bool((d_st == -1).all().item())
                and bool((d_fb == -2).all().item()) and bool((d_scratch == 0x77).all().item()) and torch.equal(r["d_have"], pre)
                and bool((d_slices == PAD).all().item()))

    def both(**change):
        """refused by the receiver, and by the provider where it takes the argument"""
        rc = _c_ingest(s, g, r, ranges, d_good, d_st, d_fb, d_scratch, **change)
        mine = {k: v for k, v in change.items() if k in ("ctx", "arena_bytes", "offsets", "lens", "g", "files", "first", "count")}
        rc2 = _c_provide(s, g, ranges, d_slices, **mine) if mine else BAD
        return rc == BAD and rc2 == BAD and untouched()
    files, first, count = _arrays(ranges)
    assert both(ctx=None) and both(g=7)
    for name in ("offsets", "lens", "files", "first", "count", "d_obs", "d_roots", "d_slices", "d_st", "d_fb", "d_scratch"):
        assert both(**{name: None}), name
    assert _c_provide(s, g, ranges, d_slices, d_obs=None) == BAD and _c_provide(s, g, ranges, d_slices, d_slices=None) == BAD and untouched()
    assert both(d_obs=r["d_obs"].data_ptr() + 4) and both(d_slices=d_good.data_ptr() + 8) and both(d_fb=d_fb.data_ptr() + 4)
    assert _c_provide(s, g, ranges, d_slices, d_slices=d_slices.data_ptr() + 8) == BAD and untouched()
    assert both(d_have=r["d_have"].data_ptr() + 4), "a misaligned bitmap"
    assert both(d_scratch=d_scratch.data_ptr() + 8), "a misaligned scratch"
    assert both(scratch_bytes=16 * 3), "a scratch that is too small"
    for k, (what, value) in enumerate([("files", len(s["lens"])), ("count", 0), ("first", 1025), ("count", 26)]):
        bad = {"files": files, "first": first, "count": count}[what].copy()
        bad[0 if what != "files" else -1] = value                          # (the first range, or the last one behind good ranges)
        assert both(**{what: bad}), (what, value)
        assert "range" in s["ctx"].last_error()
    reach = max(int(s["offsets"][f]) + s["lens"][f] for f, _, _ in ranges)
    assert both(arena_bytes=reach - 1), "a file that reaches past arena_bytes"
    with pytest.raises(m.B3WError):
        m.bao.ingest_range_slices(s["ctx"], r["d_arena"], s["offsets"], s["lens"], r["d_obs"], s["roots"], files, first, count, d_good, group_log=7)
    with pytest.raises(m.B3WError):
        m.bao.range_slices_arena(s["ctx"], s["d_src"], s["offsets"], s["lens"], s["made"][0]["outboards"], [0], [0], [0])
    # no ranges: a no-op, whatever else is handed in
    L = m.lib()
    assert L.b3w_bao_range_slice_ingest_device(s["ctx"].handle, None, 0, None, None, 0, 0, None, None, None, None, None, 0, None, None, None, None, None, 0, None) == 0
    assert L.b3w_bao_range_slice_arena_device(s["ctx"].handle, None, 0, None, None, 0, 0, None, None, None, None, 0, None, None) == 0
    assert untouched()
    # and the same arguments unchanged are taken, with and without a bitmap
    assert _c_ingest(s, g, r, ranges, d_good, d_st, d_fb, d_scratch) == 0, s["ctx"].last_error()
    torch.cuda.synchronize()
    assert not d_st.any().item() and bool((d_fb == -1).all().item())
    kept = r["d_have"].clone()
    assert _c_ingest(s, g, r, ranges, d_good, d_st, d_fb, d_scratch, d_have=None) == 0, s["ctx"].last_error()
    torch.cuda.synchronize()
    assert torch.equal(r["d_have"], kept) and not d_st.any().item()
    assert _walls_intact(r["whole_a"], r["size"]) and _walls_intact(r["whole_o"], r["total"])
