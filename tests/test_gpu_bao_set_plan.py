"""Step records planned from SET slices (bao.plan_samples_set_slices, prove_samples_set_slices; b3w_sample_plan_set_slices_device).  A small
world of its own: ten files from 0 bytes to 3 MiB + 5, some at odd arena offsets, the slices from bao.set_slices_arena.  THE YARDSTICK is
the one-chunk planner this call is defined by: bao.plan_samples_slices over the projections of the same packed set slices
(bao_set_ref.project over places read off the format alone) - records, row_first and statuses chunk by chunk - and, untampered, the whole
records and sample_status tensors of bao.plan_samples_range_slices over bao.range_slices_arena of the same list and of
bao.plan_samples_arena.  The set outputs are held against bao.ingest_set_slices' statuses.  The call's outputs (records, chunk statuses,
set outputs, scratch) start as 0xEE between 0xA5 guards.  Expected statuses of tampered slices come from the one-chunk planner on the
projections, never written by hand."""
import functools

import numpy as np
import pytest

import b3w_testlib as T
import bao_ref as R
import bao_set_ref as RS
from test_gpu_bao_ingest import BAD, K, _packed, _walled, _walls_intact

pytestmark = pytest.mark.gpu

PAD = 0x5C
MIB = 1 << 20
FILES = [(0, 0), (1, 3), (K, 8), (K + 1, 1), (2 * K, 0), (64 * K, 5), (64 * K + 1, 7), (MIB, 0), (MIB + 1, 9), (3 * MIB + 5, 1)]      # (length, start modulo 16)
ONE, F65, F1025, BIG = 1, 6, 8, 9


@functools.lru_cache(maxsize=None)
def _world():
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    offsets, at = [], 0
    for ln, phase in FILES:
        at = (at + 15) // 16 * 16 + phase
        offsets.append(at)
        at += ln
    lens = [ln for ln, _ in FILES]
    arena = np.random.default_rng(29).integers(0, 256, at + 64, dtype=np.uint8)
    d_src = torch.from_numpy(arena).cuda()
    offsets = np.array(offsets, dtype=np.uint64)
    made = m.bao.outboard_batch(ctx, d_src, offsets, lens)
    torch.cuda.synchronize()
    return dict(m=m, ctx=ctx, arena=arena, d_src=d_src, offsets=offsets, lens=lens, ln=np.array(lens, dtype=np.uint64), n=[m.bao.num_chunks(x) for x in lens],
                outboards=made["outboards"], roots=made["roots"])


@pytest.fixture(scope="module", autouse=True)
def _a_memory_pool_of_its_own():
    """the module's device tensors come from a pool of its own and go with it"""
    import gc
    import torch
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        torch.cuda.synchronize()
        if _world.cache_info().currsize:
            _world()["ctx"].close()
        _world.cache_clear()
        _places.cache_clear()
        gc.collect()
    del pool


def shapes(n):
    """-> {name: runs}: the sets that fit a file of n chunks"""
    out = {"one run": ((n // 3, max(1, n // 4)),), "the whole file": ((0, n),), "a run onto the last chunk": ((max(0, n - 3), min(3, n)),)}
    for a, b in ((0, 2), (63, 65), (1023, 1025)):
        if b < n:
            out[f"{{{a}, {b}}}"] = ((a, 1), (b, 1))
    if n >= 2:
        out["first and last chunk"] = ((0, 1), (n - 1, 1))
        out["every second chunk"] = tuple((c, 1) for c in range(0, n, 2))
    if n >= 8:
        out["touching runs"] = ((1, 2), (3, 1), (4, 3), (n - 1, 1))
    return out


@functools.lru_cache(maxsize=None)
def _places(length, runs):
    """where the parts of the set slice of these runs lie, from the format alone (bao_set_ref.encode's walk without the hashing):
    ("chunk", c) and ("node", lo, size) -> offset"""
    n = R.num_chunks(length)
    wanted = RS.chunks_of(runs)
    places, at = {}, [8]

    def walk(lo, m):
        if m == 1:
            places[("chunk", lo)] = at[0]
            at[0] += min(length, (lo + 1) * K) - lo * K
            return
        s = R._split(m)
        places[("node", lo, m)] = at[0]
        at[0] += 64
        if RS._meets(wanted, lo, lo + s):
            walk(lo, s)
        if RS._meets(wanted, lo + s, lo + m):
            walk(lo + s, m - s)
    walk(0, n)
    return places


def _arrays(sets):
    """sets: [(file, runs)] ascending by file -> the range list"""
    files = np.array([f for f, runs in sets for _ in runs], dtype=np.uint32)
    first = np.array([a for _, runs in sets for a, _ in runs], dtype=np.uint64)
    count = np.array([k for _, runs in sets for _, k in runs], dtype=np.uint64)
    return files, first, count


def _rows_of(sets):
    rows = 0
    for _, runs in sets:                                                   # a row per touched block of 64 or of 1 024 chunks
        c = RS.chunks_of(runs)
        B_ = 64 if c[-1] // 64 - c[0] // 64 <= 1 else 1024
        rows += len({x // B_ for x in c})
    return rows


def _provide(w, sets):
    """-> (the packed set slices on the device, the layout)"""
    files, first, count = _arrays(sets)
    out = w["m"].bao.set_slices_arena(w["ctx"], w["d_src"], w["offsets"], w["lens"], w["outboards"], files, first, count)
    assert out["set_file"].tolist() == [f for f, _ in sets]
    return out["slices"], out


def _plan(m, ctx, ln, d_roots, sets, d_slices):
    """the C call into walled outputs -> dict(records, chunk_status, set_status, set_first_bad: CUDA tensors; rrf, crf, provable, lay)"""
    import torch
    files, first, count = _arrays(sets)
    rrf, crf, provable = m.bao.sample_rows_ranges(ln, files, first, count)
    lay = m.bao.set_slice_layout(ln, files, first, count)
    rows, chunks, n_sets = int(rrf[-1]), int(count.sum()), len(sets)
    need = m.lib().b3w_bao_set_slice_ingest_scratch_bytes(ln.ctypes.data, ln.size, files.ctypes.data, first.ctypes.data, count.ctypes.data, files.size)
    assert need == 16 * _rows_of(sets)
    sizes = (rows * 128, chunks * 4, n_sets * 4, n_sets * 8, need)
    walls = [_walled(x) for x in sizes]
    recs, st, sst, sfb, scratch = (x[1] for x in walls)
    rc = m.lib().b3w_sample_plan_set_slices_device(ctx.handle, ln.ctypes.data, ln.size, d_roots.data_ptr(), files.ctypes.data, first.ctypes.data, count.ctypes.data,
                                                   files.size, d_slices.data_ptr(), recs.data_ptr(), st.data_ptr(), sst.data_ptr(), sfb.data_ptr(), scratch.data_ptr(),
                                                   need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, ctx.last_error()
    torch.cuda.synchronize()
    for (whole, _), size in zip(walls, sizes):
        assert _walls_intact(whole, size)
    return dict(records=recs.view(torch.int32).view(rows, 32), chunk_status=st.view(torch.int32), set_status=sst.view(torch.int32),
                set_first_bad=sfb.view(torch.int64), rrf=rrf, crf=crf, provable=provable, lay=lay)


def _slices_of(m, ln, sets, d_slices, lay):
    host = d_slices.cpu().numpy()
    return [host[int(at):int(at) + m.bao.set_slice_size(int(ln[f]), [a for a, _ in runs], [k for _, k in runs])].tobytes()
            for at, (f, runs) in zip(lay["slice_first"][:-1], sets)]


def _yardstick(m, ctx, ln, d_roots, sets, slices):
    """bao.plan_samples_slices over the projections of these set slices (bytes) onto every wanted chunk, in runs_chunks order"""
    import torch
    c_files, chunks = m.bao.runs_chunks(*_arrays(sets))
    proj = [RS.project(sl, _places(int(ln[f]), tuple(runs)), int(ln[f]), c) for (f, runs), sl in zip(sets, slices) for c in RS.chunks_of(runs)]
    d_proj = torch.from_numpy(_packed(m, ln, c_files, chunks, proj)).cuda()
    out = m.bao.plan_samples_slices(ctx, ln, d_roots, c_files, chunks, d_proj)
    torch.cuda.synchronize()
    return out, c_files, chunks


def _same(got, want, sets):
    """records, rows and statuses word for word with the one-chunk planner's; the layout facts; the set outputs from the per-chunk
    statuses -> the statuses (numpy)"""
    import torch
    st = got["chunk_status"].cpu().numpy()
    assert np.array_equal(st, want["sample_status"])
    assert np.array_equal(got["crf"], want["row_first"]) and np.array_equal(got["provable"], want["provable"])
    assert got["records"].shape == want["records"].shape and torch.equal(got["records"], want["records"])
    lay = got["lay"]
    assert np.array_equal(lay["set_chunk_first"], np.concatenate([[0], np.cumsum([len(RS.chunks_of(runs)) for _, runs in sets])]).astype(np.uint64))
    sst, sfb = [], []
    for s, (_, runs) in enumerate(sets):
        mine, wanted = st[int(lay["set_chunk_first"][s]):int(lay["set_chunk_first"][s + 1])], RS.chunks_of(runs)
        assert got["crf"][int(lay["set_chunk_first"][s])] == got["rrf"][int(lay["set_range_first"][s])]      # set s owns the rows from there
        bad = np.flatnonzero(mine)
        sst.append(int(mine.max()))
        sfb.append(wanted[int(bad[0])] if bad.size else -1)
    assert got["set_status"].cpu().tolist() == sst and got["set_first_bad"].cpu().tolist() == sfb
    return st


def _ingest(w, sets, d_slices, roots=None, lens=None, offsets=None):
    """bao.ingest_set_slices of the same slices into a receiver that holds only the roots"""
    import torch
    m = w["m"]
    lens = w["lens"] if lens is None else lens
    offsets = w["offsets"] if offsets is None else offsets
    d_arena = torch.empty(w["arena"].size, dtype=torch.uint8, device="cuda")
    d_obs = torch.empty(int(m.bao.batch_layout(lens)[-1]), dtype=torch.uint8, device="cuda")
    return m.bao.ingest_set_slices(w["ctx"], d_arena, offsets, lens, d_obs, w["roots"] if roots is None else roots, *_arrays(sets), d_slices)


def _same_as_ingest(got, taken):
    import torch
    assert torch.equal(got["set_status"], taken["set_status"]) and torch.equal(got["set_first_bad"], taken["set_first_bad"])
    assert torch.equal(got["chunk_status"], taken["chunk_status"])


def _calls(w):
    """-> [(name, [(file, runs)])]: every shape on every file it fits, a call a shape (a file is in one set a call)"""
    per = [shapes(n) for n in w["n"]]
    return [(name, [(f, sh[name]) for f, sh in enumerate(per) if name in sh]) for name in sorted({name for sh in per for name in sh})]


def test_every_file_equals_the_yardsticks():
    import torch
    w = _world()
    m, ctx = w["m"], w["ctx"]
    calls = _calls(w)
    assert {name for name, _ in calls} >= {"{0, 2}", "{63, 65}", "{1023, 1025}", "first and last chunk", "every second chunk", "a run onto the last chunk",
                                            "touching runs", "one run", "the whole file"}
    assert any(len(sets) == len(FILES) for _, sets in calls) and any(int(o) % 2 for o in w["offsets"])
    seen_tiles = seen_waves = False
    for name, sets in calls:
        files, first, count = _arrays(sets)
        d_slices, lay = _provide(w, sets)
        got = _plan(m, ctx, w["ln"], w["roots"], sets, d_slices)
        want, c_files, chunks = _yardstick(m, ctx, w["ln"], w["roots"], sets, _slices_of(m, w["ln"], sets, d_slices, lay))
        st = _same(got, want, sets)
        assert not st.any(), name
        seen_tiles |= _rows_of([s for s in sets if s[0] == BIG]) > 1
        seen_waves |= any(_rows_of([s]) == 2 and RS.chunks_of(s[1])[-1] < 128 for s in sets)
        # the range planner over range slices of the same list, and the arena planner: the whole tensors
        rs = m.bao.range_slices_arena(ctx, w["d_src"], w["offsets"], w["lens"], w["outboards"], files, first, count)
        ranged = m.bao.plan_samples_range_slices(ctx, w["lens"], w["roots"], files, first, count, rs["slices"])
        assert torch.equal(got["records"], ranged["records"]) and np.array_equal(st, ranged["sample_status"]), name
        assert np.array_equal(got["rrf"], ranged["range_row_first"])
        arena = m.bao.plan_samples_arena(ctx, w["d_src"], w["offsets"], w["lens"], w["outboards"], w["roots"], c_files, chunks)
        assert torch.equal(got["records"], arena["records"]) and not arena["sample_status"].any(), name
        _same_as_ingest(got, _ingest(w, sets, d_slices))
        # the Python call: the same plan, keyed per chunk, plus the set outputs and the layout
        out = m.bao.plan_samples_set_slices(ctx, w["lens"], w["roots"], files, first, count, d_slices)
        assert torch.equal(out["records"], got["records"]) and np.array_equal(out["row_first"], want["row_first"])
        assert np.array_equal(out["sample_status"], want["sample_status"]) and np.array_equal(out["provable"], want["provable"])
        assert np.array_equal(out["range_row_first"], got["rrf"]) and not out["set_status"].any().item() and bool((out["set_first_bad"] == -1).all().item())
        assert np.array_equal(out["set_chunk_first"], lay["set_chunk_first"]) and np.array_equal(out["set_range_first"], lay["set_range_first"])
    assert seen_tiles and seen_waves


VICTIM = ((4, 1), (7, 1), (1500, 1), (2500, 1))                             # of the 3 MiB + 5 file: two tiles under the root's left child, one outside it
TAMPERS = ["a wanted chunk's byte", "a node inside a block", "a node above the blocks", "the header", "a wrong root", "a one-chunk file's wrong root"]


@pytest.mark.parametrize("what", TAMPERS)
def test_a_tampered_set_beside_a_good_set_of_another_file(what):
    import torch
    w = _world()
    m, ctx = w["m"], w["ctx"]
    sets = [(ONE, ((0, 1),)), (F1025, ((0, 1), (2, 1), (1023, 2))), (BIG, VICTIM)]
    d_slices, lay = _provide(w, sets)
    d_slices = d_slices.clone()
    roots = w["roots"].clone()
    places, at = _places(w["lens"][BIG], VICTIM), int(lay["slice_first"][2])
    assert w["n"][BIG] == 3073 and R._split(3073) == 2048
    below = None                                                            # the chunks under the tampered node
    if what == "a wanted chunk's byte":
        d_slices[at + places[("chunk", 1500)] + 77] ^= 1
    elif what == "a node inside a block":
        d_slices[at + places[("node", 4, 4)] + 5] ^= 0x40
        below = range(4, 8)
    elif what == "a node above the blocks":
        d_slices[at + places[("node", 0, 2048)] + 40] ^= 2
        below = range(0, 2048)
    elif what == "the header":
        d_slices[at + 1] ^= 0x80
    elif what == "a wrong root":
        roots.view(-1)[8 * BIG + 3] ^= 0x10000
    else:
        roots.view(-1)[8 * ONE] ^= 1
    got = _plan(m, ctx, w["ln"], roots, sets, d_slices)
    want, _, _ = _yardstick(m, ctx, w["ln"], roots, sets, _slices_of(m, w["ln"], sets, d_slices, lay))
    st = _same(got, want, sets)                                             # (the chained records of the spoiled chunks among them)
    _same_as_ingest(got, _ingest(w, sets, d_slices, roots=roots))
    one, good, mine = st[:1].tolist(), st[1:5].tolist(), st[5:].tolist()
    assert good == [0] * 4                                                  # the good set of another file
    wanted = RS.chunks_of(VICTIM)
    if below is not None:                                                   # a bad node spoils the wanted chunks below it, in every row under it, and no other
        assert mine == [2 if c in below else 0 for c in wanted] and 0 in mine and mine.count(2) >= 2
    assert (one, mine) == {"a wanted chunk's byte": ([0], [0, 0, 1, 0]), "a node inside a block": ([0], mine), "a node above the blocks": ([0], mine),
                           "the header": ([0], [3] * 4), "a wrong root": ([0], [2] * 4), "a one-chunk file's wrong root": ([1], [0] * 4)}[what]


def test_4096_one_chunk_runs_in_one_call():
    """every second chunk of an 8 MiB file: four tile rows with every second lane busy"""
    import torch
    w = _world()
    m, ctx = w["m"], w["ctx"]
    lens, offs = [8 * MIB], np.array([3], dtype=np.uint64)
    ln = np.array(lens, dtype=np.uint64)
    d_arena = torch.from_numpy(np.random.default_rng(291).integers(0, 256, 8 * MIB + 16, dtype=np.uint8)).cuda()
    made = m.bao.outboard_batch(ctx, d_arena, offs, lens)
    sets = [(0, tuple((c, 1) for c in range(0, 8192, 2)))]
    files, first, count = _arrays(sets)
    assert files.size == 4096
    out = m.bao.set_slices_arena(ctx, d_arena, offs, lens, made["outboards"], files, first, count)
    got = _plan(m, ctx, ln, made["roots"], sets, out["slices"])
    want, c_files, chunks = _yardstick(m, ctx, ln, made["roots"], sets, _slices_of(m, ln, sets, out["slices"], out))
    assert not _same(got, want, sets).any()
    rs = m.bao.range_slices_arena(ctx, d_arena, offs, lens, made["outboards"], files, first, count)
    ranged = m.bao.plan_samples_range_slices(ctx, lens, made["roots"], files, first, count, rs["slices"])
    assert torch.equal(got["records"], ranged["records"]) and not ranged["sample_status"].any()
    arena = m.bao.plan_samples_arena(ctx, d_arena, offs, lens, made["outboards"], made["roots"], c_files, chunks)
    assert torch.equal(got["records"], arena["records"])


def test_places_past_4_gib():
    """the fabricated set slice of one fictitious file of 5 GiB + 300 B (test_gpu_bao_set's): a chunk in the first tile, a run across chunk
    2^22 (past byte 2^32) and the ragged last chunk; the planner reads only slices, so there is no arena at all"""
    import torch
    from test_gpu_bao_set import _fabricate
    w = _world()
    m, ctx = w["m"], w["ctx"]
    length = (5 << 30) + 300
    n = m.bao.num_chunks(length)
    rng = np.random.default_rng(65)
    runs = ((7, 1), ((1 << 22) - 1, 3), (n - 1, 1))
    wanted = RS.chunks_of(runs)
    chosen = {c: rng.integers(0, 256, min(K, length - c * K), dtype=np.uint8).tobytes() for c in wanted}
    sl, root, _ = _fabricate(length, wanted, chosen, rng)
    sets = [(0, runs)]
    files, first, count = _arrays(sets)
    assert len(sl) == m.bao.set_slice_size(length, first, count)
    lens = np.array([length], dtype=np.uint64)
    packed = np.full(int(m.bao.set_slice_layout(lens, files, first, count)["slice_first"][-1]), PAD, dtype=np.uint8)
    packed[8:8 + len(sl)] = np.frombuffer(sl, dtype=np.uint8)
    d_roots = torch.from_numpy(np.array(root, dtype=np.uint32).view(np.int32)).cuda()
    got = _plan(m, ctx, lens, d_roots, sets, torch.from_numpy(packed).cuda())
    want, _, _ = _yardstick(m, ctx, lens, d_roots, sets, [sl])
    assert not _same(got, want, sets).any()
    recs = got["records"].cpu().numpy().view(np.uint32)
    assert [int(x) for x in recs[int(got["crf"][2])][10:12]] == [1 << 22, 0] and [int(x) for x in recs[-1][10:12]] == [n - 1, 0]      # the chunk index words


def test_prove_samples_set_slices_equals_prove_samples_slices():
    import torch
    import ec_ref as E
    w = _world()
    m, ctx = w["m"], w["ctx"]
    sets = [(F65, ((0, 1), (2, 1), (63, 2)))]                                # {0, 2, 63, 64} of the 65-chunk file
    files, first, count = _arrays(sets)
    d_slices, lay = _provide(w, sets)
    c_files, chunks = m.bao.runs_chunks(files, first, count)
    assert chunks.tolist() == [0, 2, 63, 64]
    (sl,) = _slices_of(m, w["ln"], sets, d_slices, lay)
    proj = [RS.project(sl, _places(w["lens"][F65], sets[0][1]), w["lens"][F65], int(c)) for c in chunks]
    d_proj = torch.from_numpy(_packed(m, w["ln"], c_files, chunks, proj)).cuda()
    key = m.CommitKey(ctx, "pallas", E.points_to_bytes(E.random_points("pallas", ctx.witness_size)), window=12)
    r1cs = m.R1cs(ctx)
    want = m.bao.prove_samples_slices(ctx, w["lens"], w["roots"], c_files, chunks, d_proj, batch_steps=16, commit_key=key)
    got = m.bao.prove_samples_set_slices(ctx, w["lens"], w["roots"], files, first, count, d_slices, batch_steps=16, commit_key=key)
    want2 = m.bao.prove_samples_slices(ctx, w["lens"], w["roots"], c_files, chunks, d_proj, batch_steps=7, r1cs=r1cs)
    got2 = m.bao.prove_samples_set_slices(ctx, w["lens"], w["roots"], files, first, count, d_slices, batch_steps=7, r1cs=r1cs)
    assert (got["sample_status"] == 0).all() and (got2["sample_status"] == 0).all()
    for a, b in ((got, want), (got2, want2)):
        assert torch.equal(a["records"], b["records"]) and list(a["row_first"]) == list(b["row_first"]) and list(a["provable"]) == list(b["provable"])
        assert torch.equal(a["public"], b["public"]) and torch.equal(a["status"], b["status"]) and (a["status"] == 0).all().item()
        assert not a["set_status"].any().item()
    assert torch.equal(got["points"], want["points"]) and got2["points"] is None
    assert torch.equal(got2["violations"], want2["violations"]) and (got2["violations"] == 0).all().item()
    r1cs.close()
    key.close()


def _some_sets(w):
    return [(ONE, ((0, 1),)), (F65, ((0, 1), (2, 1), (63, 2))), (F1025, ((1, 2), (3, 1), (1000, 25))), (BIG, ((5, 1), (1020, 10), (3070, 3)))]


def _c_plan(w, sets, o, **change):
    import torch
    files, first, count = _arrays(sets)
    kw = dict(ctx=w["ctx"].handle, lens=w["ln"].ctypes.data, n_files=len(w["lens"]), d_roots=w["roots"].data_ptr(), files=files.ctypes.data,
              first=first.ctypes.data, count=count.ctypes.data, n_ranges=files.size, d_slices=o["slices"].data_ptr(), d_recs=o["recs"].data_ptr(),
              d_st=o["st"].data_ptr(), d_sst=o["sst"].data_ptr(), d_sfb=o["sfb"].data_ptr(), d_scratch=o["scratch"].data_ptr(), scratch_bytes=o["scratch"].numel())
    for name, value in change.items():
        kw[name] = value.ctypes.data if isinstance(value, np.ndarray) else value
    return w["m"].lib().b3w_sample_plan_set_slices_device(*kw.values(), torch.cuda.current_stream().cuda_stream)


def _outputs(w, sets, fill=None):
    import torch
    files, first, count = _arrays(sets)
    rrf, _, _ = w["m"].bao.sample_rows_ranges(w["ln"], files, first, count)
    make = (lambda n, dt: torch.empty(n, dtype=dt, device="cuda")) if fill is None else (lambda n, dt: torch.full((n,), fill, dtype=dt, device="cuda"))
    return dict(recs=make(int(rrf[-1]) * 32, torch.int32), st=make(int(count.sum()), torch.int32), sst=make(len(sets), torch.int32),
                sfb=make(len(sets), torch.int64), scratch=make(16 * _rows_of(sets), torch.uint8))


def test_the_call_allocates_nothing():
    import torch
    w = _world()
    sets = _some_sets(w)
    d_slices, _ = _provide(w, sets)
    o = dict(_outputs(w, sets), slices=d_slices)
    for _ in range(2):                                                    # (the context's staging grows in the first round, outside the allocator)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        assert _c_plan(w, sets, o) == 0, w["ctx"].last_error()
        torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == before
    assert not o["st"].any().item() and not o["sst"].any().item() and bool((o["sfb"] == -1).all().item())


def test_refusals_leave_every_output_and_the_scratch_untouched():
    import torch
    w = _world()
    m = w["m"]
    sets = _some_sets(w)
    d_slices, _ = _provide(w, sets)
    o = dict(_outputs(w, sets, fill=0x77), slices=d_slices)
    files, first, count = _arrays(sets)

    def refused(**change):
        rc = _c_plan(w, sets, o, **change)
        torch.cuda.synchronize()
        return rc == BAD and all(bool((o[k] == 0x77).all().item()) for k in ("recs", "st", "sst", "sfb", "scratch"))
    assert _c_plan(w, sets, o, ctx=None) == BAD
    for name in ("lens", "d_roots", "files", "first", "count", "d_slices", "d_recs", "d_st", "d_sst", "d_sfb", "d_scratch"):
        assert refused(**{name: None}), name
    assert refused(d_slices=d_slices.data_ptr() + 8) and refused(d_recs=o["recs"].data_ptr() + 2) and refused(d_st=o["st"].data_ptr() + 1)
    assert refused(d_sst=o["sst"].data_ptr() + 2) and refused(d_sfb=o["sfb"].data_ptr() + 4) and refused(d_roots=w["roots"].data_ptr() + 1)
    assert refused(d_scratch=o["scratch"].data_ptr() + 8), "a misaligned scratch"
    assert refused(scratch_bytes=o["scratch"].numel() - 16), "a scratch that is too small"
    last = files.size - 1
    j = next(i for i in range(2, files.size) if files[i] == files[i - 2])  # the third run of a set
    for what, at, value, named in (("files", last, len(w["lens"]), "file index"), ("count", 0, 0, "no chunk"), ("first", last, 1 << 40, "past"),
                                   ("count", last, 1 << 40, "past"), ("first", j, int(first[j - 1]), "disjoint"), ("first", j, int(first[j - 2]), "ascending"),
                                   ("files", last, 0, "ascending")):
        bad = {"files": files, "first": first, "count": count}[what].copy()
        bad[at] = value
        assert refused(**{what: bad}), (what, at, value)
        assert "range" in w["ctx"].last_error() and named in w["ctx"].last_error(), w["ctx"].last_error()
    long_lens = w["ln"].copy()
    long_lens[F1025] = ((1 << 30) + 1) * 1024                               # a file of 2^30 + 1 chunks
    assert refused(lens=long_lens) and "2^30" in w["ctx"].last_error()
    comp = m.Context("compression", 0)                                     # nova contexts only, as for every planner
    assert refused(ctx=comp.handle)
    comp.close()
    with pytest.raises(m.B3WError):
        m.bao.plan_samples_set_slices(w["ctx"], w["lens"], w["roots"], [0, 0], [1, 0], [1, 1], d_slices)
    # no ranges: a no-op, whatever else is handed in
    assert m.lib().b3w_sample_plan_set_slices_device(w["ctx"].handle, None, 0, None, None, None, None, 0, None, None, None, None, None, None, 0, None) == 0
    assert refused(ctx=None)
    # and the same arguments unchanged are taken
    assert _c_plan(w, sets, o) == 0, w["ctx"].last_error()
    torch.cuda.synchronize()
    assert not o["st"].any().item() and not o["sst"].any().item() and bool((o["sfb"] == -1).all().item())
