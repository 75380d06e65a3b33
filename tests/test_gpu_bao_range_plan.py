"""Step records of challenged chunk runs planned from range slices (bao.plan_samples_range_slices, prove_samples_range_slices;
b3w_sample_plan_range_slices_device).  The world is test_gpu_bao_ingest._setup()'s, as tests/test_gpu_bao_range.py uses it.  THE YARDSTICK
is always the one-chunk planner this call is defined by: b3w_sample_plan_slices_device over the projections of the same packed range
slices (bao_range_ref.project, packed with bao.slice_layout) — records and statuses word for word — and, for untampered slices,
bao.plan_samples_arena over the provider's arena as well.  Range status and first bad chunk are held against the per-chunk statuses.
The new call's outputs (records, chunk statuses, range outputs, scratch) start as 0xEE between 0xA5 guards."""
import functools

import numpy as np
import pytest

import b3w_testlib as T
import bao_range_ref as RR
import bao_ref as R
from test_bao_range_cpu import _tampers
from test_gpu_bao_ingest import BAD, K, _packed, _setup, _walled, _walls_intact
from test_gpu_bao_range import _arrays, _fabricate, _pack, _partition, _provide, _some_ranges, _test_ranges

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _a_memory_pool_of_its_own():
    """as test_gpu_bao_range does it: the module's device tensors (the 1 GiB file's records among them) come from a pool of its own"""
    import gc
    import torch
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        torch.cuda.synchronize()
        if _setup.cache_info().currsize:
            _setup()["ctx"].close()
        _setup.cache_clear()
        _places.cache_clear()
        gc.collect()
    del pool


@functools.lru_cache(maxsize=None)
def _places(length, a, k):
    """where the parts of the slice of chunks [a, a + k) lie, from the format alone (bao_range_ref.encode's walk without the hashing):
    ("chunk", c) and ("node", lo, size) -> offset"""
    n = R.num_chunks(length)
    places, at = {}, [8]

    def walk(lo, m):
        if m == 1:
            places[("chunk", lo)] = at[0]
            at[0] += min(length, (lo + 1) * K) - lo * K
            return
        s = R._split(m)
        places[("node", lo, m)] = at[0]
        at[0] += 64
        if a < lo + s:
            walk(lo, s)
        if a + k > lo + s:
            walk(lo + s, m - s)
    walk(0, n)
    return places


def _rows_of(ranges):
    """the table rows of these ranges: a wave per block of 64 chunks a short range touches, a workgroup per tile a longer one does"""
    return sum((a + k - 1) // (64 if k <= 64 else 1024) - a // (64 if k <= 64 else 1024) + 1 for _, a, k in ranges)


def _plan(m, ctx, ln, d_roots, ranges, d_slices):
    """the C call into walled outputs -> dict(records, chunk_status, range_status, range_first_bad: CUDA tensors; rrf, crf, provable)"""
    import torch
    files, first, count = _arrays(ranges)
    rrf, crf, provable = m.bao.sample_rows_ranges(ln, files, first, count)
    rows, chunks, n = int(rrf[-1]), int(count.sum()), len(ranges)
    need = m.lib().b3w_bao_range_slice_ingest_scratch_bytes(ln.ctypes.data, ln.size, files.ctypes.data, first.ctypes.data, count.ctypes.data, n)
    assert need == 16 * _rows_of(ranges)
    walls = [_walled(x) for x in (rows * 128, chunks * 4, n * 4, n * 8, need)]
    recs, st, rst, rfb, scratch = (w[1] for w in walls)
    rc = m.lib().b3w_sample_plan_range_slices_device(ctx.handle, ln.ctypes.data, ln.size, d_roots.data_ptr(), files.ctypes.data, first.ctypes.data,
                                                     count.ctypes.data, n, d_slices.data_ptr(), recs.data_ptr(), st.data_ptr(), rst.data_ptr(), rfb.data_ptr(),
                                                     scratch.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, ctx.last_error()
    torch.cuda.synchronize()
    for (whole, _), size in zip(walls, (rows * 128, chunks * 4, n * 4, n * 8, need)):
        assert _walls_intact(whole, size)
    return dict(records=recs.view(torch.int32).view(rows, 32), chunk_status=st.view(torch.int32), range_status=rst.view(torch.int32),
                range_first_bad=rfb.view(torch.int64), rrf=rrf, crf=crf, provable=provable)


def _yardstick(m, ctx, ln, d_roots, ranges, slices):
    """b3w_sample_plan_slices_device over the projections of these range slices (bytes) onto every chunk, in runs_chunks order"""
    import torch
    files, first, count = _arrays(ranges)
    c_files, chunks = m.bao.runs_chunks(files, first, count)
    proj = [RR.project(sl, _places(int(ln[f]), a, k), int(ln[f]), c) for (f, a, k), sl in zip(ranges, slices) for c in range(a, a + k)]
    d_proj = torch.from_numpy(_packed(m, ln, c_files, chunks, proj)).cuda()
    out = m.bao.plan_samples_slices(ctx, ln, d_roots, c_files, chunks, d_proj)
    torch.cuda.synchronize()
    return out, c_files, chunks


def _same(got, want, ranges):
    """records and statuses word for word; the rows; the range outputs from the per-chunk statuses -> the statuses (numpy)"""
    import torch
    st = got["chunk_status"].cpu().numpy()
    assert np.array_equal(st, want["sample_status"])
    assert np.array_equal(got["crf"], want["row_first"]) and np.array_equal(got["provable"], want["provable"])
    assert got["records"].shape == want["records"].shape and torch.equal(got["records"], want["records"])
    at, rst, rfb = 0, [], []
    for _, a, k in ranges:
        mine = st[at:at + k]
        bad = np.flatnonzero(mine)
        rst.append(int(mine.max()))
        rfb.append(a + int(bad[0]) if bad.size else -1)
        at += k
    assert got["range_status"].cpu().tolist() == rst and got["range_first_bad"].cpu().tolist() == rfb
    return st


@pytest.mark.parametrize("g", [0, 4])
def test_every_file_equals_the_one_chunk_planner_on_the_projections(g):
    import torch
    s = _setup()
    m = s["m"]
    ranges = [(f, a, k) for f, ln in enumerate(s["lens"]) for a, k in _test_ranges(m.bao.num_chunks(ln))]
    n_of = [m.bao.num_chunks(ln) for ln in s["lens"]]
    assert 0 in s["lens"] and 1 in s["lens"] and {5, 6, 7} & set(n_of)                   # the empty and the one-byte file; incomplete trees
    assert any(k > 64 and a // 1024 != (a + k - 1) // 1024 for _, a, k in ranges)         # two tiles
    assert any(k <= 64 and a // 64 != (a + k - 1) // 64 for _, a, k in ranges)            # two wave rows
    perm = np.random.default_rng(900 + g).permutation(len(ranges))
    ranges = [ranges[i] for i in perm]
    d_slices, _, slices = _provide(s, g, ranges)                                          # (the same standard bytes at every g)
    got = _plan(m, s["ctx"], s["ln"], s["roots"], ranges, d_slices)
    want, c_files, chunks = _yardstick(m, s["ctx"], s["ln"], s["roots"], ranges, slices)
    st = _same(got, want, ranges)
    assert not st.any() and not got["provable"].all() and got["provable"].any()
    arena = m.bao.plan_samples_arena(s["ctx"], s["d_src"], s["offsets"], s["lens"], s["made"][0]["outboards"], s["roots"], c_files, chunks)
    assert torch.equal(got["records"], arena["records"]) and not arena["sample_status"].any()
    # the Python call: the same plan, keyed per chunk, plus the range outputs
    out = m.bao.plan_samples_range_slices(s["ctx"], s["lens"], s["roots"], *_arrays(ranges), d_slices)
    assert torch.equal(out["records"], got["records"]) and np.array_equal(out["row_first"], want["row_first"])
    assert np.array_equal(out["sample_status"], want["sample_status"]) and np.array_equal(out["provable"], want["provable"])
    assert np.array_equal(out["range_row_first"], got["rrf"]) and not out["range_status"].any().item() and bool((out["range_first_bad"] == -1).all().item())


def test_tampered_ranges_beside_good_ones():
    import torch
    s = _setup()
    m = s["m"]
    big = s["lens"].index(K * 1025)
    mid = s["lens"].index(70 * K + 1)
    one = s["lens"].index(next(ln for ln in s["lens"] if 0 < ln <= K))
    victims = [(big, 1022, 3), (big, 1000, 25), (big, 958, 66), (big, 3, 1021), (mid, 3, 66), (mid, 69, 2), (one, 0, 1)]
    ranges, slices, kinds = [], [], []
    for f, a, k in victims:
        _, _, (sl,) = _provide(s, 0, [(f, a, k)])
        places = _places(s["lens"][f], a, k)
        for what, bad_sl, rt, node in _tampers(sl, places, a, k, s["lens"][f], [int(x) for x in s["roots_host"][f]]):
            if what != "root":                                            # (the roots are the call's, one a file: below)
                ranges.append((f, a, k))
                slices.append(bad_sl)
                kinds.append((what, node))
    good = [(big, 0, 1025), (mid, 0, 10), (big, 1020, 5), (mid, 60, 11), (one, 0, 1)]     # beside them, and over the tampered chunks
    _, _, good_slices = _provide(s, 0, good)
    ranges += good
    slices += good_slices
    kinds += [("good", None)] * len(good)
    order = np.random.default_rng(910).permutation(len(ranges))
    ranges, slices, kinds = [ranges[i] for i in order], [slices[i] for i in order], [kinds[i] for i in order]
    packed, _ = _pack(m, s["ln"], ranges, slices)
    got = _plan(m, s["ctx"], s["ln"], s["roots"], ranges, torch.from_numpy(packed).cuda())
    want, _, _ = _yardstick(m, s["ctx"], s["ln"], s["roots"], ranges, slices)
    st = _same(got, want, ranges)                                         # (the chained records of the spoiled chunks among them)
    assert sorted(set(st.tolist())) == [0, 1, 2, 3]
    at, seen = 0, set()
    for (f, a, k), (what, node) in zip(ranges, kinds):
        mine = st[at:at + k].tolist()
        at += k
        if what == "good":
            assert not any(mine), (f, a, k)
        elif node:                                                        # a bad node spoils the chunks below it and no other
            assert mine == [2 if node[0] <= c < node[0] + node[1] else 0 for c in range(a, a + k)], (f, a, k, what)
            seen.add("above" if node[1] > (64 if k <= 64 else 1024) else "inside")
        elif what == "header":
            assert mine == [3] * k
        else:
            assert sorted(set(mine)) == ([1] if k == 1 else [0, 1]) and mine.count(1) == 1, (f, a, k, what)
    assert seen == {"above", "inside"}
    # a wrong root: every chunk of that file is 2 (1 on a one-chunk file), chained records and all
    roots = s["roots"].clone()
    roots.view(-1)[8 * mid + 3] ^= 0x10000
    roots.view(-1)[8 * one] ^= 1
    ranges = [(mid, 0, 71), (mid, 5, 1), (one, 0, 1), (big, 7, 2), (mid, 2, 65)]
    d_slices, _, slices = _provide(s, 0, ranges)
    got = _plan(m, s["ctx"], s["ln"], roots, ranges, d_slices)
    want, _, _ = _yardstick(m, s["ctx"], s["ln"], roots, ranges, slices)
    _same(got, want, ranges)
    assert got["range_status"].cpu().tolist() == [2, 2, 1, 0, 2] and got["range_first_bad"].cpu().tolist() == [0, 5, 0, -1, 2]


def test_shuffled_partitions_with_repeats_and_overlaps():
    import torch
    s = _setup()
    m = s["m"]
    rng = np.random.default_rng(920)
    ranges = [(f, a, k) for f, ln in enumerate(s["lens"]) for a, k in _partition(m.bao.num_chunks(ln), rng)]
    for i in rng.choice(len(ranges), 12, replace=False):                  # some twice, some overlapping their neighbours
        f, a, k = ranges[i]
        n = m.bao.num_chunks(s["lens"][f])
        ranges.append((f, a, k))
        ranges.append((f, max(0, a - 3), min(n, a + k + 2) - max(0, a - 3)))
    ranges = [ranges[i] for i in rng.permutation(len(ranges))]
    d_slices, sf, slices = _provide(s, 0, ranges)
    got = _plan(m, s["ctx"], s["ln"], s["roots"], ranges, d_slices)
    want, _, _ = _yardstick(m, s["ctx"], s["ln"], s["roots"], ranges, slices)
    assert not _same(got, want, ranges).any()
    alone = {}
    for i, r in enumerate(ranges):                                        # every range's rows are those of the same range planned alone
        if r not in alone:
            at = int(sf[i]) - 8                                           # (16-byte aligned: the slice starts 8 behind it, as in a pack of one)
            alone[r] = _plan(m, s["ctx"], s["ln"], s["roots"], [r], d_slices[at:])["records"]
        assert torch.equal(got["records"][int(got["rrf"][i]):int(got["rrf"][i + 1])], alone[r]), r


def test_4096_ranges_of_2_chunks_in_one_call():
    import torch
    s = _setup()
    m = s["m"]
    rng = np.random.default_rng(930)
    bigs = [f for f, ln in enumerate(s["lens"]) if m.bao.num_chunks(ln) >= 1025]
    ranges = [(int(rng.choice(bigs)), int(rng.integers(0, 1024)), 2) for _ in range(4096)]
    d_slices, _, slices = _provide(s, 0, ranges)
    got = _plan(m, s["ctx"], s["ln"], s["roots"], ranges, d_slices)
    want, c_files, chunks = _yardstick(m, s["ctx"], s["ln"], s["roots"], ranges, slices)
    assert not _same(got, want, ranges).any()
    arena = m.bao.plan_samples_arena(s["ctx"], s["d_src"], s["offsets"], s["lens"], s["made"][0]["outboards"], s["roots"], c_files, chunks)
    assert torch.equal(got["records"], arena["records"])


def test_places_past_4_gib():
    """one fabricated file of 5 GiB + 300 B (test_gpu_bao_range's: the planner reads only slices, so there is no arena at all): a range
    across chunk 2^22 and one onto the ragged last chunk"""
    import torch
    s = _setup()
    m = s["m"]
    length = (5 << 30) + 300
    n = m.bao.num_chunks(length)
    rng = np.random.default_rng(64)
    parts, ranges = [], []
    for f, (a, k) in enumerate([((1 << 22) - 3, 7), (n - 2, 2)]):          # each under a tree of its own: two files of the same length
        chosen = {c: rng.integers(0, 256, min(K, length - c * K), dtype=np.uint8).tobytes() for c in range(a, a + k)}
        parts.append(_fabricate(length, a, k, chosen, rng))
        ranges.append((f, a, k))
    lens = np.array([length, length], dtype=np.uint64)
    slices = [p[0] for p in parts]
    packed, _ = _pack(m, lens, ranges, slices)
    d_roots = torch.from_numpy(np.array([p[1] for p in parts], dtype=np.uint32).view(np.int32)).cuda()
    got = _plan(m, s["ctx"], lens, d_roots, ranges, torch.from_numpy(packed).cuda())
    want, _, _ = _yardstick(m, s["ctx"], lens, d_roots, ranges, slices)
    assert not _same(got, want, ranges).any()
    recs = got["records"].cpu().numpy().view(np.uint32)
    assert [int(x) for x in recs[int(got["crf"][3])][10:12]] == [1 << 22, 0] and [int(x) for x in recs[-1][10:12]] == [n - 1, 0]      # the chunk index words


def test_one_range_of_a_whole_gib_file_writes_records_past_4_gib():
    """the smallest shape at which a 32-bit byte offset into the records goes wrong: 37 748 736 rows, 4.8 GB, compared whole on the device
    with the arena planner over the same chunks (its C call: the Python wrapper walks the chunks for the provable flags)"""
    import torch
    s = _setup()
    m = s["m"]
    ctx, L = s["ctx"], m.lib()
    GIB = 1 << 30
    gen = torch.Generator(device="cuda").manual_seed(6)
    d_arena = torch.randint(0, 256, (GIB,), dtype=torch.uint8, device="cuda", generator=gen)
    lens, offs = np.array([GIB], dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    prov = m.bao.outboard_batch(ctx, d_arena, offs, lens)
    files, first, count = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64), np.array([1 << 20], dtype=np.uint64)
    d_slices = m.bao.range_slices_arena(ctx, d_arena, offs, lens, prov["outboards"], files, first, count)["slices"]
    rrf = np.zeros(2, dtype=np.uint64)
    rows = L.b3w_sample_rows_ranges(lens.ctypes.data, 1, files.ctypes.data, first.ctypes.data, count.ctypes.data, 1, rrf.ctypes.data, None, None)
    assert rows == 37748736 and rows * 128 > 1 << 32
    recs = torch.full((rows, 32), -1, dtype=torch.int32, device="cuda")
    st = torch.full((1 << 20,), -1, dtype=torch.int32, device="cuda")
    rst = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    rfb = torch.full((1,), -2, dtype=torch.int64, device="cuda")
    scratch = torch.empty(16 * 1024, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rc = L.b3w_sample_plan_range_slices_device(ctx.handle, lens.ctypes.data, 1, prov["roots"].data_ptr(), files.ctypes.data, first.ctypes.data, count.ctypes.data, 1,
                                               d_slices.data_ptr(), recs.data_ptr(), st.data_ptr(), rst.data_ptr(), rfb.data_ptr(), scratch.data_ptr(),
                                               scratch.numel(), stream)
    assert rc == 0, ctx.last_error()
    del d_slices
    c_files, chunks = np.zeros(1 << 20, dtype=np.uint32), np.arange(1 << 20, dtype=np.uint64)
    want = torch.full((rows, 32), -2, dtype=torch.int32, device="cuda")
    want_st = torch.full((1 << 20,), -1, dtype=torch.int32, device="cuda")
    rc = L.b3w_sample_plan_arena_device(ctx.handle, d_arena.data_ptr(), GIB, offs.ctypes.data, lens.ctypes.data, 1, 0, prov["outboards"].data_ptr(),
                                        prov["roots"].data_ptr(), c_files.ctypes.data, chunks.ctypes.data, 1 << 20, want.data_ptr(), want_st.data_ptr(), stream)
    assert rc == 0, ctx.last_error()
    torch.cuda.synchronize()
    assert not st.any().item() and not want_st.any().item() and rst.tolist() == [0] and rfb.tolist() == [-1]
    assert torch.equal(recs, want)
    del recs, want, d_arena


def test_prove_samples_range_slices_equals_prove_samples_slices():
    import torch
    import ec_ref as E
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    lens = np.array([43 * K + 33, 16 * K, 700, 70 * K], dtype=np.uint64)
    offsets = np.array([0, 44 * K + 16, 61 * K, 62 * K + 7], dtype=np.uint64)
    d_arena = torch.from_numpy(np.random.default_rng(940).integers(0, 256, 133 * K, dtype=np.uint8)).cuda()
    full = m.bao.outboard_batch(ctx, d_arena, offsets, lens)
    ranges = [(0, 40, 4), (1, 3, 2), (2, 0, 1), (3, 62, 5), (0, 0, 3)]
    files, first, count = _arrays(ranges)
    rs = m.bao.range_slices_arena(ctx, d_arena, offsets, lens, full["outboards"], files, first, count)
    host, sf = rs["slices"].cpu().numpy(), rs["slice_first"]
    slices = [host[int(sf[i]):int(sf[i]) + m.bao.range_slice_size(int(lens[f]), a, k)].tobytes() for i, (f, a, k) in enumerate(ranges)]
    c_files, chunks = m.bao.runs_chunks(files, first, count)
    proj = [RR.project(sl, _places(int(lens[f]), a, k), int(lens[f]), c) for (f, a, k), sl in zip(ranges, slices) for c in range(a, a + k)]
    d_proj = torch.from_numpy(_packed(m, lens, c_files, chunks, proj)).cuda()
    key = m.CommitKey(ctx, "pallas", E.points_to_bytes(E.random_points("pallas", ctx.witness_size)), window=12)
    r1cs = m.R1cs(ctx)
    want = m.bao.prove_samples_slices(ctx, lens, full["roots"], c_files, chunks, d_proj, batch_steps=16, commit_key=key)
    got = m.bao.prove_samples_range_slices(ctx, lens, full["roots"], files, first, count, rs["slices"], batch_steps=16, commit_key=key)
    want2 = m.bao.prove_samples_slices(ctx, lens, full["roots"], c_files, chunks, d_proj, batch_steps=7, r1cs=r1cs)
    got2 = m.bao.prove_samples_range_slices(ctx, lens, full["roots"], files, first, count, rs["slices"], batch_steps=7, r1cs=r1cs)
    assert (got["sample_status"] == 0).all() and (got2["sample_status"] == 0).all() and got["provable"].any() and not got["provable"].all()
    for a, b in ((got, want), (got2, want2)):
        assert torch.equal(a["records"], b["records"]) and list(a["row_first"]) == list(b["row_first"]) and list(a["provable"]) == list(b["provable"])
        assert torch.equal(a["public"], b["public"]) and torch.equal(a["status"], b["status"]) and (a["status"] == 0).all().item()
        assert not a["range_status"].any().item()
    assert torch.equal(got["points"], want["points"]) and got2["points"] is None
    assert torch.equal(got2["violations"], want2["violations"]) and (got2["violations"] == 0).all().item()
    r1cs.close()
    key.close()
    ctx.close()


def _c_plan(s, ranges, o, **change):
    import torch
    files, first, count = _arrays(ranges)
    kw = dict(ctx=s["ctx"].handle, lens=s["ln"].ctypes.data, n_files=len(s["lens"]), d_roots=s["roots"].data_ptr(), files=files.ctypes.data,
              first=first.ctypes.data, count=count.ctypes.data, n_ranges=len(ranges), d_slices=o["slices"].data_ptr(), d_recs=o["recs"].data_ptr(),
              d_st=o["st"].data_ptr(), d_rst=o["rst"].data_ptr(), d_rfb=o["rfb"].data_ptr(), d_scratch=o["scratch"].data_ptr(), scratch_bytes=o["scratch"].numel())
    for name, value in change.items():
        kw[name] = value.ctypes.data if isinstance(value, np.ndarray) else value
    return s["m"].lib().b3w_sample_plan_range_slices_device(*kw.values(), torch.cuda.current_stream().cuda_stream)


def _outputs(s, ranges, fill=None):
    import torch
    m = s["m"]
    files, first, count = _arrays(ranges)
    rrf, _, _ = m.bao.sample_rows_ranges(s["ln"], files, first, count)
    make = (lambda n, dt: torch.empty(n, dtype=dt, device="cuda")) if fill is None else (lambda n, dt: torch.full((n,), fill, dtype=dt, device="cuda"))
    return dict(recs=make(int(rrf[-1]) * 32, torch.int32), st=make(int(count.sum()), torch.int32), rst=make(len(ranges), torch.int32),
                rfb=make(len(ranges), torch.int64), scratch=make(16 * _rows_of(ranges), torch.uint8))


def test_the_call_allocates_nothing():
    import torch
    s = _setup()
    ranges = _some_ranges(s)
    d_slices, _, _ = _provide(s, 0, ranges)
    o = dict(_outputs(s, ranges), slices=d_slices)
    for _ in range(2):                                                    # (the context's staging grows in the first round, outside the allocator)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        assert _c_plan(s, ranges, o) == 0, s["ctx"].last_error()
        torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == before
    assert not o["st"].any().item() and not o["rst"].any().item() and bool((o["rfb"] == -1).all().item())


def test_refusals_leave_every_output_and_the_scratch_untouched():
    import torch
    s = _setup()
    m = s["m"]
    ranges = _some_ranges(s)
    d_slices, _, _ = _provide(s, 0, ranges)
    o = dict(_outputs(s, ranges, fill=0x77), slices=d_slices)
    files, first, count = _arrays(ranges)

    def refused(**change):
        rc = _c_plan(s, ranges, o, **change)
        torch.cuda.synchronize()
        return rc == BAD and all(bool((o[k] == 0x77).all().item()) for k in ("recs", "st", "rst", "rfb", "scratch"))
    assert _c_plan(s, ranges, o, ctx=None) == BAD
    for name in ("lens", "d_roots", "files", "first", "count", "d_slices", "d_recs", "d_st", "d_rst", "d_rfb", "d_scratch"):
        assert refused(**{name: None}), name
    assert refused(d_slices=d_slices.data_ptr() + 8) and refused(d_recs=o["recs"].data_ptr() + 2) and refused(d_st=o["st"].data_ptr() + 1)
    assert refused(d_rst=o["rst"].data_ptr() + 2) and refused(d_rfb=o["rfb"].data_ptr() + 4) and refused(d_roots=s["roots"].data_ptr() + 1)
    assert refused(d_scratch=o["scratch"].data_ptr() + 8), "a misaligned scratch"
    assert refused(scratch_bytes=o["scratch"].numel() - 16), "a scratch that is too small"
    for what, value in (("files", len(s["lens"])), ("count", 0), ("first", 1025), ("count", 26)):
        bad = {"files": files, "first": first, "count": count}[what].copy()
        bad[0 if what != "files" else -1] = value                          # (the first range, or the last one behind good ranges)
        assert refused(**{what: bad}), (what, value)
        assert "range" in s["ctx"].last_error()
    long_lens = s["ln"].copy()
    long_lens[ranges[1][0]] = ((1 << 30) + 1) * 1024                        # a file of 2^30 + 1 chunks
    assert refused(lens=long_lens) and "2^30" in s["ctx"].last_error()
    comp = m.Context("compression", 0)                                     # nova contexts only, as for every planner
    assert refused(ctx=comp.handle)
    comp.close()
    with pytest.raises(m.B3WError):
        m.bao.plan_samples_range_slices(s["ctx"], s["lens"], s["roots"], [0], [0], [0], d_slices)
    # no ranges: a no-op, whatever else is handed in
    assert m.lib().b3w_sample_plan_range_slices_device(s["ctx"].handle, None, 0, None, None, None, None, 0, None, None, None, None, None, None, 0, None) == 0
    assert refused(ctx=None)
    # and the same arguments unchanged are taken
    assert _c_plan(s, ranges, o) == 0, s["ctx"].last_error()
    torch.cuda.synchronize()
    assert not o["st"].any().item() and not o["rst"].any().item() and bool((o["rfb"] == -1).all().item())
