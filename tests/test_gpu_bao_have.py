"""The arrival bitmap on the device (bao.have_new / ingest_slices(d_have=) / have_runs / have_from_status; b3w_bao_slice_ingest_have_device,
b3w_bao_have_runs_device, b3w_bao_have_from_status_device) against the restatement in tests/bao_have_ref.py.  The source arena is
test_gpu_bao_slices._world()'s with files of the module's own behind it (starts at 4, 8 and 12 modulo 16 and at odd bytes; 64 * 1 024 + 999,
1 024 * 1 025 and 2^20 + 300 bytes among them); the provider's side is computed once and left unchanged, the receiver starts from buffers
of 0xEE between 0xA5 guards and holds only the roots.
  ingest parity   the same shuffled third of every file through ingest_slices without and with d_have: arena, outboards and statuses byte
                  for byte equal, d_have = what was there | the verified samples' bits
  runs            one batch of bitmaps with no arena behind it (the CPU test's patterns, a file of 2^24 + 5 chunks at density 0.5, one
                  that lacks three chunks) against the restatement row for row, both kinds, four unit sizes
  rebuild         verify_batch over what the receiver holds, have_from_status: the ingest's bitmap seen through units
  closed loop     a zero bitmap, 30 % of every file, have_runs("missing") -> runs_chunks -> slices_arena -> ingest: every file complete"""
import functools

import numpy as np
import pytest

import b3w_testlib as T
import bao_have_ref as H
import bao_ref as R
from test_bao_have_cpu import _patterns
from test_gpu_bao_slices import _world

pytestmark = pytest.mark.gpu

K = 1024
GUARD = 4096
FILL, WALL = 0xEE, 0xA5
GS = [0, 1, 4, 6]
BAD = 100
OWN = [(K * 1025, 8), ((1 << 20) + 300, 1), (5 * K + 300, 4), (3 * K + 17, 12), (70 * K + 1, 7), (64 * K + 999, 4)]      # (length, start modulo 16)
BIG = (1 << 24) + 5


@functools.lru_cache(maxsize=None)
def _setup():
    """the source arena, the provider's outboards of it at every g, and the slices of a shuffled third of every file (files that share
    their place in the arena take the same third), one sample twice"""
    import torch
    m = T.pkg()
    ctx = m.Context("nova_vesta", 0)
    w_arena, w_offsets, w_lens, _ = _world()
    at = (w_arena.size + 15) // 16 * 16
    offsets, lens = [int(x) for x in w_offsets], [int(x) for x in w_lens]
    first_own = len(lens)
    for ln, phase in OWN:
        at = (at + 48 + 15) // 16 * 16 + phase
        offsets.append(at)
        lens.append(ln)
        at += ln
    arena = np.random.default_rng(20).integers(0, 256, at + 64, dtype=np.uint8)
    arena[:w_arena.size] = w_arena
    offsets = np.array(offsets, dtype=np.uint64)
    assert {int(o) % 16 for o in offsets} >= {0, 4, 8, 12} and any(int(o) % 2 for o in offsets)
    n_of = [m.bao.num_chunks(x) for x in lens]
    d_src = torch.from_numpy(arena).cuda()
    made = {0: m.bao.outboard_batch(ctx, d_src, offsets, lens)}
    for g in GS[1:]:
        made[g] = m.bao.outboard_groups_batch(ctx, d_src, offsets, lens, g)
    files, chunks = [], []
    for f, (o, ln, n) in enumerate(zip(offsets.tolist(), lens, n_of)):
        take = set(np.random.default_rng([o, ln]).permutation(n)[:(n + 2) // 3].tolist())
        if 0 < ln % K < 4:
            take.add(n - 1)               # (a last chunk of one to three bytes: never left to the fill, which may hold its bytes by chance)
        files += [f] * len(take)
        chunks += sorted(take)
    files.append(files[5])
    chunks.append(chunks[5])
    perm = np.random.default_rng(21).permutation(len(files))
    files, chunks = np.array(files, dtype=np.uint32)[perm], np.array(chunks, dtype=np.uint64)[perm]
    third = m.bao.slices_arena(ctx, d_src, offsets, lens, made[0]["outboards"], files, chunks)
    word_first = m.bao.have_layout(lens)
    assert [int(x) for x in word_first] == H.layout(lens)
    bits = [np.zeros(n, bool) for n in n_of]
    for f, c in zip(files.tolist(), chunks.tolist()):
        bits[f][c] = True
    torch.cuda.synchronize()
    return dict(m=m, ctx=ctx, arena=arena, offsets=offsets, lens=lens, ln=np.array(lens, dtype=np.uint64), n_of=n_of, d_src=d_src, made=made,
                roots=made[0]["roots"], files=files, chunks=chunks, slices=third["slices"], slice_first=third["slice_first"], word_first=word_first,
                bits=bits, expected=np.concatenate([H.pack(b) for b in bits]), first_own=first_own)


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
        _runs_batch.cache_clear()
        _received.cache_clear()
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


def _walled_words(words, fill=None):
    """-> (whole, the middle as int64 [words]): a bitmap between guards, holding `fill` (numpy uint64) or the 0xEE fill"""
    import torch
    whole, mid = _walled(8 * words)
    have = mid.view(torch.int64)
    if fill is not None:
        have.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype=np.uint64).view(np.int64)))
    return whole, have


def _host_words(t):
    return t.cpu().numpy().view(np.uint64)


def _ob_total(s, g):
    return int(s["made"][g]["ob_first"][-1])


def _ingest(s, g, d_have, files=None, chunks=None, d_slices=None, d_roots=None):
    """one ingest into fresh walled buffers -> (arena bytes, outboard bytes, statuses: host numpy; the two device tensors)"""
    m = s["m"]
    size, total = s["arena"].size, _ob_total(s, g)
    whole_a, d_arena = _walled(size)
    whole_o, d_obs = _walled(total)
    st = m.bao.ingest_slices(s["ctx"], d_arena, s["offsets"], s["lens"], d_obs, s["roots"] if d_roots is None else d_roots,
                             s["files"] if files is None else files, s["chunks"] if chunks is None else chunks,
                             s["slices"] if d_slices is None else d_slices, group_log=g, d_have=d_have)["sample_status"]
    assert _walls_intact(whole_a, size) and _walls_intact(whole_o, total)
    return d_arena.cpu().numpy(), d_obs.cpu().numpy(), st.cpu().numpy(), d_arena, d_obs


@pytest.mark.parametrize("lanes", ["1", "4", "16"])
@pytest.mark.parametrize("g", GS)
def test_ingest_with_the_bitmap_writes_what_ingest_writes_and_the_bits(g, lanes, monkeypatch):
    s = _setup()
    monkeypatch.setenv("B3W_SLICE_INGEST_LANES", lanes)
    words = int(s["word_first"][-1])
    pre = np.random.default_rng(500 + g).integers(0, 1 << 63, words, dtype=np.uint64) & np.random.default_rng(501).integers(0, 1 << 63, words, dtype=np.uint64)
    whole_h, d_have = _walled_words(words, pre)
    plain = _ingest(s, g, None)
    with_have = _ingest(s, g, d_have)
    assert not plain[2].any() and (plain[2] == with_have[2]).all()
    assert (plain[0] == with_have[0]).all() and (plain[1] == with_have[1]).all()
    assert (plain[0] != FILL).sum() > 1000 and (plain[0] == FILL).sum() > plain[0].size // 2        # a third came in, not more
    got = _host_words(d_have)
    assert (got == (pre | s["expected"])).all(), "d_have is not what was there | the verified samples' bits"
    assert (pre & ~s["expected"]).any() and (s["expected"] & ~pre).any()
    assert _walls_intact(whole_h, 8 * words)


TAMPERS = ["header", "first node", "last node", "chunk byte", "root"]


@pytest.mark.parametrize("g", [0, 4])
def test_tampered_slices_set_no_bit(g):
    """the five tampers of the ingest tests in one call, beside good slices of other chunks and one sample twice"""
    import torch
    s = _setup()
    m = s["m"]
    o = s["first_own"]
    victims = {"header": (o, 5), "first node": (o, 700), "last node": (o + 1, 3), "chunk byte": (o + 4, 33), "root": (o + 5, 10)}
    good = [(o, 6), (o + 1, 1024), (o + 4, 70), (o + 2, 5), (o, 701), (o + 1, 2), (o + 4, 32), (o, 6)]
    also_bad = [(o + 5, 64)]                                                   # (every sample of the file whose root is wrong fails)
    samples = [victims[t] for t in TAMPERS] + good + also_bad
    order = np.random.default_rng(600 + g).permutation(len(samples))
    files = np.array([samples[i][0] for i in order], dtype=np.uint32)
    chunks = np.array([samples[i][1] for i in order], dtype=np.uint64)
    out = m.bao.slices_arena(s["ctx"], s["d_src"], s["offsets"], s["lens"], s["made"][0]["outboards"], files, chunks)
    host, sf = out["slices"].cpu().numpy().copy(), out["slice_first"]
    want = np.zeros(len(samples), dtype=np.int32)
    roots = s["roots"].cpu().numpy().view(np.uint32).reshape(-1, 8).copy()
    for i, k in enumerate(order.tolist()):
        f, c = samples[k]
        if k >= len(TAMPERS):
            want[i] = 2 if f == o + 5 else 0
            continue
        P = len(R.path_nodes(c, s["n_of"][f]))
        at, status = {"header": (3, 3), "first node": (8 + 21, 2), "last node": (8 + 64 * (P - 1) + 40, 2), "chunk byte": (8 + 64 * P + 500, 1),
                      "root": (None, 2)}[TAMPERS[k]]
        want[i] = status
        if at is None:
            roots[f, 3] ^= 0x10000
        else:
            host[int(sf[i]) + at] ^= 1
    d_slices = torch.from_numpy(host).cuda()
    d_roots = torch.from_numpy(roots.view(np.int32)).cuda()
    words = int(s["word_first"][-1])
    whole_h, d_have = _walled_words(words, np.zeros(words, dtype=np.uint64))
    plain = _ingest(s, g, None, files, chunks, d_slices, d_roots)
    with_have = _ingest(s, g, d_have, files, chunks, d_slices, d_roots)
    assert (with_have[2] == want).all(), (with_have[2], want)
    assert (plain[2] == want).all() and (plain[0] == with_have[0]).all() and (plain[1] == with_have[1]).all()
    bits = [np.zeros(n, bool) for n in s["n_of"]]
    for f, c in good:
        bits[f][c] = True
    assert (_host_words(d_have) == np.concatenate([H.pack(b) for b in bits])).all()
    assert _walls_intact(whole_h, 8 * words)


# ---- runs ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _runs_batch():
    """one batch of bitmaps: the CPU test's patterns on files of 129 and 70 chunks, the two long files, each between files of 1, 63, 64, 65
    and 1 025 chunks with random bits (pad bits set in every second one) -> lens, chunk counts, the files' words, the device tensor"""
    import torch
    rng = np.random.default_rng(77)
    seps = [1, 63, 64, 65, 1025]
    n_of, haves = [], []

    def add(n, bits, pad):
        n_of.append(n)
        haves.append(H.pack(bits, pad))

    def sep():
        n = seps[len(n_of) % len(seps)]
        add(n, rng.random(n) < rng.choice([0.0, 0.3, 1.0]), len(n_of) % 2 == 0)
    for n in (129, 70):
        for _, bits, pad in _patterns(n, n):
            sep()
            add(n, bits, pad)
    sep()
    dense = len(n_of)
    add(BIG, rng.random(BIG) < 0.5, False)
    sep()
    holes = np.ones(BIG, bool)
    holes[[0, 1 << 23, BIG - 1]] = False
    add(BIG, holes, True)
    sep()
    lens = [n * K - 7 if n > 1 else 1 for n in n_of]                             # (only the chunk counts matter: ragged last chunks)
    lens[n_of.index(1)] = 0                                                    # an empty file: one chunk, one bit
    assert [H.num_chunks(x) for x in lens] == n_of
    d_have = torch.from_numpy(np.concatenate(haves).view(np.int64)).cuda()
    return dict(lens=np.array(lens, dtype=np.uint64), n_of=n_of, haves=haves, d_have=d_have, dense=dense, want={})


def _want_runs(b, g, kind):
    if (g, kind) not in b["want"]:
        b["want"][(g, kind)] = H.batch_runs(b["haves"], b["n_of"], g, H.KINDS[kind])
    return b["want"][(g, kind)]


def _runs_c(m, ctx, d_have, lens, g, kind, cap, null_rows=False, with_file_have=True):
    """the C call into walled outputs of 0xEE -> (files, first, count: device tensors [cap]; n_runs; file_have: host) after the walls were checked"""
    import torch
    L = m.lib()
    w_f, d_f = _walled(4 * cap)
    w_a, d_a = _walled(8 * cap)
    w_c, d_c = _walled(8 * cap)
    w_n, d_n = _walled(8)
    w_h, d_h = _walled(8 * lens.size)
    need = L.b3w_bao_have_runs_scratch_bytes(lens.ctypes.data, lens.size)
    w_s, d_s = _walled(need)
    rc = L.b3w_bao_have_runs_device(ctx.handle, d_have.data_ptr(), lens.ctypes.data, lens.size, g, H.KINDS[kind], cap, None if null_rows else d_f.data_ptr(),
                                    None if null_rows else d_a.data_ptr(), None if null_rows else d_c.data_ptr(), d_n.data_ptr(),
                                    d_h.data_ptr() if with_file_have else None, d_s.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, ctx.last_error()
    torch.cuda.synchronize()
    for whole, size in ((w_f, 4 * cap), (w_a, 8 * cap), (w_c, 8 * cap), (w_n, 8), (w_h, 8 * lens.size), (w_s, need)):
        assert _walls_intact(whole, size)
    return d_f.view(torch.int32), d_a.view(torch.int64), d_c.view(torch.int64), int(d_n.view(torch.int64).item()), d_h.view(torch.int64).cpu().numpy()


def _rows_equal(got, want, rows):
    return all((t[:rows].cpu().numpy().view(w.dtype) == w[:rows]).all() for t, w in zip(got, want))


def _untouched_behind(got, rows):
    return all(bool((t[rows:].contiguous().view(-1).view(__import__("torch").uint8) == FILL).all().item()) for t in got)


@pytest.mark.parametrize("kind", ["missing", "present"])
@pytest.mark.parametrize("g", GS)
def test_runs_equal_the_restatement(g, kind):
    s = _setup()
    m = s["m"]
    b = _runs_batch()
    files, first, count, file_have = _want_runs(b, g, kind)
    cap = m.bao.have_runs_bound(b["lens"], g)
    assert cap >= files.size
    d_f, d_a, d_c, n_runs, got_have = _runs_c(m, s["ctx"], b["d_have"], b["lens"], g, kind, cap)
    assert n_runs == files.size, (n_runs, files.size)
    assert got_have.tolist() == file_have
    assert _rows_equal((d_f, d_a, d_c), (files, first, count), n_runs)
    assert _untouched_behind((d_f, d_a, d_c), n_runs)
    print(f"g = {g}, {kind}: {n_runs} runs of {len(b['n_of'])} files, {int(b['d_have'].numel())} words")


def test_the_python_call_and_the_partition():
    s = _setup()
    m = s["m"]
    b = _runs_batch()
    small = slice(0, b["dense"])                                               # the files in front of the long ones
    lens = b["lens"][small]
    words = int(m.bao.have_layout(lens)[-1])
    d_have = b["d_have"][:words]
    for g in GS:
        covered = [np.zeros((n + (1 << g) - 1) >> g, dtype=np.int32) for n in b["n_of"][small]]
        for kind in ("missing", "present"):
            out = m.bao.have_runs(s["ctx"], d_have, lens, kind, g)
            files, first, count, file_have = H.batch_runs(b["haves"][small], b["n_of"][small], g, H.KINDS[kind])
            assert out["files"].dtype == np.uint32 and out["first_chunks"].dtype == np.uint64 and out["n_chunks"].dtype == np.uint64
            assert (out["files"] == files).all() and (out["first_chunks"] == first).all() and (out["n_chunks"] == count).all()
            assert out["n_runs"].is_cuda and int(out["n_runs"].item()) == files.size
            assert out["file_have"].is_cuda and out["file_have"].cpu().tolist() == file_have
            for f, a, k in zip(out["files"].tolist(), out["first_chunks"].tolist(), out["n_chunks"].tolist()):
                covered[f][a >> g:(a + k + (1 << g) - 1) >> g] += 1
        assert all((c == 1).all() for c in covered), (g, "PRESENT and MISSING do not partition the units")
    fi, ch = m.bao.runs_chunks(out["files"], out["first_chunks"], out["n_chunks"])
    assert fi.size == int(out["n_chunks"].sum()) == ch.size


@pytest.mark.parametrize("g", [0, 1])
def test_a_capacity_below_the_total_and_a_count_only_call(g):
    s = _setup()
    m = s["m"]
    b = _runs_batch()
    f = b["dense"]
    word_first = m.bao.have_layout(b["lens"])
    one = b["lens"][f:f + 1].copy()
    d_one = b["d_have"][int(word_first[f]):int(word_first[f + 1])]
    rows, n_have = H.runs(H.unpack(b["haves"][f], BIG), g, H.MISSING)
    assert len(rows) > 100000
    want = (np.zeros(1000, dtype=np.uint32), np.array([r[0] for r in rows[:1000]], dtype=np.uint64), np.array([r[1] for r in rows[:1000]], dtype=np.uint64))
    # room for 1 500 rows, a capacity of 1 000: the rows behind it keep the fill
    import torch
    L = m.lib()
    w_f, d_f = _walled(4 * 1500)
    w_a, d_a = _walled(8 * 1500)
    w_c, d_c = _walled(8 * 1500)
    d_n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    d_h = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    need = L.b3w_bao_have_runs_scratch_bytes(one.ctypes.data, 1)
    d_s = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert L.b3w_bao_have_runs_device(s["ctx"].handle, d_one.data_ptr(), one.ctypes.data, 1, g, H.MISSING, 1000, d_f.data_ptr(), d_a.data_ptr(), d_c.data_ptr(),
                                      d_n.data_ptr(), d_h.data_ptr(), d_s.data_ptr(), need, torch.cuda.current_stream().cuda_stream) == 0, s["ctx"].last_error()
    torch.cuda.synchronize()
    got = (d_f.view(torch.int32), d_a.view(torch.int64), d_c.view(torch.int64))
    assert int(d_n.item()) == len(rows) and int(d_h.item()) == n_have
    assert _rows_equal(got, want, 1000) and _untouched_behind(got, 1000)
    assert _walls_intact(w_f, 4 * 1500) and _walls_intact(w_a, 8 * 1500) and _walls_intact(w_c, 8 * 1500)
    # the whole batch with a capacity of 1 000
    files, first, count, file_have = _want_runs(b, g, "missing")
    got = _runs_c(m, s["ctx"], b["d_have"], b["lens"], g, "missing", 1000)
    assert got[3] == files.size > 1000 and got[4].tolist() == file_have and _rows_equal(got[:3], (files, first, count), 1000)
    # no capacity, null rows: the counts alone; and without the per-file counts
    got = _runs_c(m, s["ctx"], b["d_have"], b["lens"], g, "missing", 0, null_rows=True)
    assert got[3] == files.size and got[4].tolist() == file_have
    got = _runs_c(m, s["ctx"], b["d_have"], b["lens"], g, "missing", 0, null_rows=True, with_file_have=False)
    assert got[3] == files.size and (got[4].view(np.uint8) == FILL).all()


# ---- rebuild and the closed loop ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _received(g):
    """the parity test's ingest at this g from a zero bitmap -> (the receiver's arena and outboards on the device, the bitmap)"""
    s = _setup()
    d_have = s["m"].bao.have_new(s["lens"])
    _, _, st, d_arena, d_obs = _ingest(s, g, d_have)
    assert not st.any()
    return d_arena, d_obs, d_have


@pytest.mark.parametrize("g", GS)
def test_rebuilding_from_verification_gives_the_ingests_bitmap(g):
    import torch
    s = _setup()
    m = s["m"]
    d_arena, d_obs, d_have = _received(g)
    assert (_host_words(d_have) == s["expected"]).all()
    res = m.bao.verify_batch(s["ctx"], d_arena, s["offsets"], s["lens"], d_obs, s["roots"], group_log=g)
    words = int(s["word_first"][-1])
    whole, rebuilt = _walled_words(words, np.full(words, (1 << 64) - 1, dtype=np.uint64))
    assert m.bao.have_from_status(s["ctx"], res["unit_status"], s["lens"], g, d_have=rebuilt) is rebuilt
    want = np.concatenate([H.pack(H.collapse(b, g)) for b in s["bits"]])
    assert (_host_words(rebuilt) == want).all(), f"g = {g}: the rebuilt bitmap is not the ingest's seen through units of {1 << g}"
    assert _walls_intact(whole, 8 * words)
    status = res["unit_status"].cpu().numpy()
    unit_first = res["unit_first"]
    ref = np.concatenate([H.from_status(status[int(unit_first[f]):int(unit_first[f + 1])], n, g) for f, n in enumerate(s["n_of"])])
    assert (ref == want).all()
    made = m.bao.have_from_status(s["ctx"], res["unit_status"], s["lens"], g)        # (a tensor of its own when none is given)
    assert made.dtype == torch.int64 and (_host_words(made) == want).all()
    mixed = status.copy()                                                            # 1, 2, 3 and 0xFF read as absent
    mixed[::3] = np.resize(np.array([1, 2, 3, 0xFF, 0], dtype=np.uint8), mixed[::3].size)
    got = m.bao.have_from_status(s["ctx"], torch.from_numpy(mixed).cuda(), s["lens"], g)
    ref = np.concatenate([H.from_status(mixed[int(unit_first[f]):int(unit_first[f + 1])], n, g) for f, n in enumerate(s["n_of"])])
    assert (_host_words(got) == ref).all()


@pytest.mark.parametrize("g", [0, 4])
def test_the_closed_loop_completes_every_file(g):
    import torch
    s = _setup()
    m = s["m"]
    ctx = s["ctx"]
    rng = np.random.default_rng(900 + g)
    size, total = s["arena"].size, _ob_total(s, g)
    whole_a, d_arena = _walled(size)
    whole_o, d_obs = _walled(total)
    d_have = m.bao.have_new(s["lens"])
    assert d_have.dtype == torch.int64 and d_have.numel() == int(s["word_first"][-1]) and not d_have.any().item()
    # round 1: 30 % of every file, some of the slices tampered with
    files, chunks = [], []
    for f, n in enumerate(s["n_of"]):
        take = rng.permutation(n)[:max(1, (3 * n) // 10)]
        files += [f] * take.size
        chunks += take.tolist()
    perm = rng.permutation(len(files))
    files, chunks = np.array(files, dtype=np.uint32)[perm], np.array(chunks, dtype=np.uint64)[perm]
    out = m.bao.slices_arena(ctx, s["d_src"], s["offsets"], s["lens"], s["made"][0]["outboards"], files, chunks)
    host, sf = out["slices"].cpu().numpy().copy(), out["slice_first"]
    spoiled = [i for i in rng.permutation(files.size)[:40].tolist() if s["lens"][int(files[i])] > 0][:25]
    for i in spoiled:
        host[int(sf[i]) + m.bao.slice_size(s["lens"][int(files[i])], int(chunks[i])) - 1] ^= 0x40         # the chunk's last byte
    st = m.bao.ingest_slices(ctx, d_arena, s["offsets"], s["lens"], d_obs, s["roots"], files, chunks, torch.from_numpy(host).cuda(), group_log=g,
                             d_have=d_have)["sample_status"].cpu().numpy()
    assert (st[spoiled] == 1).all() and int((st != 0).sum()) == len(spoiled)
    first_round = m.bao.have_runs(ctx, d_have, s["lens"], "missing")
    held = first_round["file_have"].cpu().numpy()
    assert (held < np.array(s["n_of"]))[np.array(s["n_of"]) > 1].all() and int(first_round["n_runs"].item()) == first_round["files"].size > 0
    # round 2: exactly what is missing
    fi, ch = m.bao.runs_chunks(first_round["files"], first_round["first_chunks"], first_round["n_chunks"])
    assert fi.size + int(held.sum()) == sum(s["n_of"])
    more = m.bao.slices_arena(ctx, s["d_src"], s["offsets"], s["lens"], s["made"][0]["outboards"], fi, ch)
    st = m.bao.ingest_slices(ctx, d_arena, s["offsets"], s["lens"], d_obs, s["roots"], fi, ch, more["slices"], group_log=g, d_have=d_have)["sample_status"]
    assert not st.any().item()
    after = m.bao.have_runs(ctx, d_have, s["lens"], "missing")
    assert after["file_have"].cpu().tolist() == s["n_of"]
    assert int(after["n_runs"].item()) == 0 and after["files"].size == 0
    assert torch.equal(d_obs, s["made"][g]["outboards"][:total]), "the received outboards are not the provider's"
    assert _walls_intact(whole_a, size) and _walls_intact(whole_o, total)
    for report in GS:
        have = m.bao.have_runs(ctx, d_have, s["lens"], "present", report)
        assert have["files"].tolist() == list(range(len(s["lens"]))) and not have["first_chunks"].any() and have["n_chunks"].tolist() == s["n_of"]
        res = m.bao.verify_ranges_batch(ctx, d_arena, s["offsets"], s["lens"], d_obs, s["roots"], have["files"], have["first_chunks"], have["n_chunks"],
                                        group_log=g)
        assert not res["range_status"].any().item(), (report, res["range_status"].cpu().numpy())


# ---- refusals and allocations ---------------------------------------------------------------------------------------------------
def test_refusals_leave_every_output_untouched():
    import torch
    s = _setup()
    m = s["m"]
    L = m.lib()
    ctx = s["ctx"]
    stream = torch.cuda.current_stream().cuda_stream
    lens = np.array([129 * K, 0, 70 * K + 1], dtype=np.uint64)
    words = 3 + 1 + 2
    bits = np.random.default_rng(5).integers(0, 1 << 63, words, dtype=np.uint64)
    d_have = torch.from_numpy(bits.view(np.int64)).cuda()
    cap = m.bao.have_runs_bound(lens)
    outs = [_walled(4 * cap), _walled(8 * cap), _walled(8 * cap), _walled(8), _walled(8 * 3), _walled(64)]
    d_f, d_a, d_c, d_n, d_h, d_s = [o[1] for o in outs]
    good = dict(ctx=ctx.handle, have=d_have.data_ptr(), lens=lens.ctypes.data, n=3, g=0, kind=0, cap=cap, f=d_f.data_ptr(), a=d_a.data_ptr(), c=d_c.data_ptr(),
                nr=d_n.data_ptr(), fh=d_h.data_ptr(), scr=d_s.data_ptr(), scr_bytes=64)

    def call(**change):
        kw = dict(good)
        kw.update(change)
        rc = L.b3w_bao_have_runs_device(kw["ctx"], kw["have"], kw["lens"], kw["n"], kw["g"], kw["kind"], kw["cap"], kw["f"], kw["a"], kw["c"], kw["nr"], kw["fh"],
                                        kw["scr"], kw["scr_bytes"], stream)
        torch.cuda.synchronize()
        return rc

    def untouched():
        return all(bool((mid == FILL).all().item()) and _walls_intact(whole, mid.numel()) for whole, mid in outs)
    refusals = [dict(ctx=None), dict(have=None), dict(have=good["have"] + 4), dict(lens=None), dict(g=7), dict(kind=2), dict(f=None), dict(a=None), dict(c=None),
                dict(f=good["f"] + 2), dict(a=good["a"] + 4), dict(c=good["c"] + 4), dict(nr=None), dict(nr=good["nr"] + 4), dict(fh=good["fh"] + 4),
                dict(scr=None), dict(scr=good["scr"] + 4), dict(scr_bytes=8)]
    for change in refusals:
        assert call(**change) == BAD and untouched(), change
    # more than 2^26 words in all: 2^32 + 64 chunks
    huge = np.array([((1 << 32) + 1) * K], dtype=np.uint64)
    assert call(lens=huge.ctypes.data, n=1, scr_bytes=1 << 30) == BAD and untouched()
    assert L.b3w_bao_have_from_status_device(ctx.handle, d_s.data_ptr(), huge.ctypes.data, 1, 0, d_a.data_ptr(), stream) == BAD
    # the pack call
    d_st = torch.zeros(200, dtype=torch.uint8, device="cuda")
    for args in ((None, d_st.data_ptr(), lens.ctypes.data, 3, 0, d_a.data_ptr()), (ctx.handle, None, lens.ctypes.data, 3, 0, d_a.data_ptr()),
                 (ctx.handle, d_st.data_ptr(), None, 3, 0, d_a.data_ptr()), (ctx.handle, d_st.data_ptr(), lens.ctypes.data, 3, 7, d_a.data_ptr()),
                 (ctx.handle, d_st.data_ptr(), lens.ctypes.data, 3, 0, None), (ctx.handle, d_st.data_ptr(), lens.ctypes.data, 3, 0, d_a.data_ptr() + 4)):
        assert L.b3w_bao_have_from_status_device(*args, stream) == BAD
        torch.cuda.synchronize()
        assert untouched(), args
    # the ingest: what the plain call refuses is covered by its own tests; here the bitmap's pointer
    k = 32
    files, chunks = s["files"][:k].copy(), s["chunks"][:k].copy()
    sl = m.bao.slices_arena(ctx, s["d_src"], s["offsets"], s["lens"], s["made"][0]["outboards"], files, chunks)["slices"]
    whole_a, d_arena = _walled(s["arena"].size)
    whole_o, d_obs = _walled(_ob_total(s, 0))
    d_st32 = torch.full((k,), -1, dtype=torch.int32, device="cuda")
    whole_h, d_hv = _walled_words(int(s["word_first"][-1]))

    def ingest(have_ptr, g=0):
        rc = L.b3w_bao_slice_ingest_have_device(ctx.handle, d_arena.data_ptr(), d_arena.numel(), s["offsets"].ctypes.data, s["ln"].ctypes.data, len(s["lens"]), g,
                                                d_obs.data_ptr(), s["roots"].data_ptr(), files.ctypes.data, chunks.ctypes.data, k, sl.data_ptr(), d_st32.data_ptr(),
                                                have_ptr, stream)
        torch.cuda.synchronize()
        return rc
    for ptr, g in ((None, 0), (d_hv.data_ptr() + 4, 0), (d_hv.data_ptr(), 7)):
        assert ingest(ptr, g) == BAD
        assert bool((d_arena == FILL).all().item()) and bool((d_obs == FILL).all().item()) and bool((d_st32 == -1).all().item())
        assert bool((d_hv.view(torch.uint8) == FILL).all().item())
    with pytest.raises(m.B3WError):
        m.bao.have_runs(ctx, d_have, lens, "absent")
    with pytest.raises(m.B3WError):
        m.bao.have_runs(ctx, d_have, lens, "missing", 7)
    with pytest.raises(m.B3WError):
        m.bao.have_runs(ctx, d_have[:3], lens)
    with pytest.raises(m.B3WError):
        m.bao.have_runs(ctx, d_have.to(torch.int32), lens)
    # no files: the count is written and is 0
    assert call(n=0, have=None, lens=None, cap=0, f=None, a=None, c=None, fh=None, scr=None, scr_bytes=0) == 0
    assert int(d_n.view(torch.int64).item()) == 0
    d_n.fill_(FILL)
    # and the good arguments are taken
    assert call() == 0, ctx.last_error()
    rows, file_have = [], []
    for f, n in enumerate((129, 1, 71)):
        a, b = int(m.bao.have_layout(lens)[f]), int(m.bao.have_layout(lens)[f + 1])
        r, h = H.runs(H.unpack(bits[a:b], n))
        rows += [(f,) + x for x in r]
        file_have.append(h)
    n_runs = int(d_n.view(torch.int64).item())
    assert n_runs == len(rows) and d_h.view(torch.int64).cpu().tolist() == file_have
    assert list(zip(d_f.view(torch.int32)[:n_runs].cpu().tolist(), d_a.view(torch.int64)[:n_runs].cpu().tolist(), d_c.view(torch.int64)[:n_runs].cpu().tolist())) == rows
    assert ingest(d_hv.data_ptr()) == 0 and not d_st32.any().item() and _walls_intact(whole_h, 8 * d_hv.numel())


def test_the_three_calls_allocate_nothing():
    import torch
    s = _setup()
    m = s["m"]
    L = m.lib()
    ctx = s["ctx"]
    stream = torch.cuda.current_stream().cuda_stream
    g = 0
    _, d_arena = _walled(s["arena"].size)
    _, d_obs = _walled(_ob_total(s, g))
    k = s["files"].size
    d_st = torch.full((k,), -1, dtype=torch.int32, device="cuda")
    d_have = m.bao.have_new(s["lens"])
    ln = s["ln"]
    cap = m.bao.have_runs_bound(ln)
    d_f = torch.empty(cap, dtype=torch.int32, device="cuda")
    d_a, d_c = torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int64, device="cuda")
    d_n, d_h = torch.empty(1, dtype=torch.int64, device="cuda"), torch.empty(ln.size, dtype=torch.int64, device="cuda")
    need = L.b3w_bao_have_runs_scratch_bytes(ln.ctypes.data, ln.size)
    d_s = torch.empty(need, dtype=torch.uint8, device="cuda")
    d_units = torch.zeros(int(m.bao.verify_layout(ln)[-1]), dtype=torch.uint8, device="cuda")
    d_back = torch.empty_like(d_have)

    def all_three():
        assert L.b3w_bao_slice_ingest_have_device(ctx.handle, d_arena.data_ptr(), d_arena.numel(), s["offsets"].ctypes.data, ln.ctypes.data, ln.size, g,
                                                  d_obs.data_ptr(), s["roots"].data_ptr(), s["files"].ctypes.data, s["chunks"].ctypes.data, k,
                                                  s["slices"].data_ptr(), d_st.data_ptr(), d_have.data_ptr(), stream) == 0, ctx.last_error()
        assert L.b3w_bao_have_runs_device(ctx.handle, d_have.data_ptr(), ln.ctypes.data, ln.size, g, H.MISSING, cap, d_f.data_ptr(), d_a.data_ptr(), d_c.data_ptr(),
                                          d_n.data_ptr(), d_h.data_ptr(), d_s.data_ptr(), need, stream) == 0, ctx.last_error()
        assert L.b3w_bao_have_from_status_device(ctx.handle, d_units.data_ptr(), ln.ctypes.data, ln.size, g, d_back.data_ptr(), stream) == 0, ctx.last_error()
        torch.cuda.synchronize()
    all_three()                                                               # (the context's staging grows here, outside the allocator)
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    all_three()
    assert torch.cuda.max_memory_allocated() == before
    assert not d_st.any().item() and (_host_words(d_have) == s["expected"]).all()
    assert d_h.cpu().tolist() == [int(b.sum()) for b in s["bits"]]
    assert (_host_words(d_back) == np.concatenate([H.pack(np.ones(n, bool)) for n in s["n_of"]])).all()
