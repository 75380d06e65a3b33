"""Set slices on the device (bao.set_slices_arena, bao.ingest_set_slices; b3w_bao_set_slice_arena_device,
b3w_bao_set_slice_ingest_device): one slice for all the wanted runs of a file, extracted where the files lie and taken in again.  The
world is test_gpu_bao_ingest._setup()'s files with, behind them in this module's own arena, files of 3 MiB + 5 and 5 MiB + 300 bytes
(several tiles under a ragged upper tree).  The provider is held against the restatement (tests/bao_set_ref.py) byte for byte; the
receiver against the host call (b3w_bao_set_slice_ingest, itself held against the projections on the CPU), against the projections
through the one-chunk device call, and against the source's bytes and the provider's outboards; receivers start from 0xEE between 0xA5
guards and hold only the roots."""
import functools
import struct

import numpy as np
import pytest

import b3w_testlib as T
import bao_range_ref as RR
import bao_ref as R
import bao_set_ref as RS
import blake3_ref as B
from test_bao_set_cpu import set_shapes, tampers
from test_gpu_bao_ingest import BAD, FILL, GUARD, K, _packed, _setup, _walled, _walls_intact

pytestmark = pytest.mark.gpu

GS = [0, 4, 6]
PAD = 0x5C
OWN = [(3 * (1 << 20) + 5, 8), (5 * (1 << 20) + 300, 1)]                  # (length, start modulo 16)


@functools.lru_cache(maxsize=None)
def _world():
    """_setup()'s files and the module's two behind them: the source arena, and the provider's outboards and roots at every g"""
    import torch
    s = _setup()
    m = s["m"]
    offsets, lens = [int(x) for x in s["offsets"]], list(s["lens"])
    at = s["arena"].size
    for ln, phase in OWN:
        at = (at + 48 + 15) // 16 * 16 + phase
        offsets.append(at)
        lens.append(ln)
        at += ln
    arena = np.random.default_rng(28).integers(0, 256, at + 64, dtype=np.uint8)
    arena[:s["arena"].size] = s["arena"]
    offsets = np.array(offsets, dtype=np.uint64)
    in_file = np.zeros(arena.size, dtype=bool)
    for o, ln in zip(offsets, lens):
        in_file[int(o):int(o) + ln] = True
    d_src = torch.from_numpy(arena).cuda()
    ctx = s["ctx"]
    made = {g: m.bao.outboard_batch(ctx, d_src, offsets, lens) if g == 0 else m.bao.outboard_groups_batch(ctx, d_src, offsets, lens, g) for g in GS}
    torch.cuda.synchronize()
    roots = made[0]["roots"]
    n = [m.bao.num_chunks(ln) for ln in lens]
    return dict(m=m, ctx=ctx, arena=arena, offsets=offsets, lens=lens, ln=np.array(lens, dtype=np.uint64), n=n, in_file=in_file, d_src=d_src, made=made,
                roots=roots, roots_host=roots.cpu().numpy().view(np.uint32).reshape(-1, 8).copy(), wf=m.bao.have_layout(lens))


@pytest.fixture(scope="module", autouse=True)
def _a_memory_pool_of_its_own():
    """as test_gpu_bao_ingest does it: the module's device tensors come from a pool of its own and go with it"""
    import gc
    import torch
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        torch.cuda.synchronize()
        _world.cache_clear()
        _expected.cache_clear()
        if _setup.cache_info().currsize:
            _setup()["ctx"].close()
        _setup.cache_clear()
        gc.collect()
    del pool


def _data(w, f):
    a = int(w["offsets"][f])
    return w["arena"][a:a + w["lens"][f]].tobytes()


@functools.lru_cache(maxsize=None)
def _expected(f, runs):
    """the restatement's set slice of the runs (a tuple of (first, count)) of file f, and its places (computed once, left unchanged)"""
    w = _world()
    data = _data(w, f)
    key = ("set world", f)
    RR.seed(data, key)
    return RS.encode(data, list(runs), key=key)


def _arrays(sets):
    """sets: [(file, runs)] ascending by file -> the range list"""
    files = np.array([f for f, runs in sets for _ in runs], dtype=np.uint32)
    first = np.array([a for _, runs in sets for a, _ in runs], dtype=np.uint64)
    count = np.array([k for _, runs in sets for _, k in runs], dtype=np.uint64)
    return files, first, count


def _sizes(w, sets):
    return [w["m"].bao.set_slice_size(w["lens"][f], [a for a, _ in runs], [k for _, k in runs]) for f, runs in sets]


def _pack(w, sets, slices):
    """the slices packed as set_slice_layout says, the padding 0x5C -> numpy"""
    sf = w["m"].bao.set_slice_layout(w["ln"], *_arrays(sets))["slice_first"]
    out = np.full(int(sf[-1]), PAD, dtype=np.uint8)
    for at, sl in zip(sf[:-1], slices):
        out[int(at):int(at) + len(sl)] = np.frombuffer(sl, dtype=np.uint8)
    return out


def _provide(w, g, sets):
    """the device provider into 0x5C between guards -> (the packed slices on the device, the layout, the slices as bytes)"""
    import torch
    m = w["m"]
    files, first, count = _arrays(sets)
    lay = m.bao.set_slice_layout(w["ln"], files, first, count)
    assert lay["set_file"].tolist() == [f for f, _ in sets]
    sf = lay["slice_first"]
    total = int(sf[-1])
    whole = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    d_slices = whole[GUARD:GUARD + total]
    d_slices.fill_(PAD)
    rc = m.lib().b3w_bao_set_slice_arena_device(w["ctx"].handle, w["d_src"].data_ptr(), w["d_src"].numel(), w["offsets"].ctypes.data, w["ln"].ctypes.data,
                                                len(w["lens"]), g, w["made"][g]["outboards"].data_ptr(), files.ctypes.data, first.ctypes.data,
                                                count.ctypes.data, files.size, d_slices.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, w["ctx"].last_error()
    torch.cuda.synchronize()
    assert _walls_intact(whole, total)
    host = d_slices.cpu().numpy()
    sizes = _sizes(w, sets)
    covered = np.zeros(total, dtype=bool)
    for at, size in zip(sf[:-1], sizes):
        covered[int(at):int(at) + size] = True
    assert (host[~covered] == PAD).all()                                   # the padding is not written
    return d_slices, lay, [host[int(at):int(at) + size].tobytes() for at, size in zip(sf[:-1], sizes)]


def _tile_sets(w):
    """the 5 MiB file's own: one chunk in each tile; only the first and the last tile"""
    f = len(w["lens"]) - 1
    n = w["n"][f]
    each = tuple((t * 1024 + (37 * t + 5) % min(1024, n - t * 1024), 1) for t in range((n + 1023) // 1024))
    ends = ((3, 2), (1000, 24), (n - 70, 3), (n - 1, 1))
    return f, each, ends


def _calls(w):
    """-> [[(file, runs)]]: every shape of the CPU test on every file it fits, a call a shape (a file is in one set a call); then the
    5 MiB file's tile sets, a call of their own each"""
    shapes = [set_shapes(n) for n in w["n"]]
    names = sorted({name for sh in shapes for name in sh})
    f5, each, ends = _tile_sets(w)
    calls = [[(f, tuple(sh[name])) for f, sh in enumerate(shapes) if name in sh] for name in names]
    return calls + [[(f5, each)], [(0, tuple(shapes[0]["the whole file"])), (f5, ends)]]


@pytest.mark.parametrize("g", GS)
def test_the_provider_equals_the_restatement(g):
    w = _world()
    calls = _calls(w)
    assert any(len(sets) == len(w["lens"]) for sets in calls)              # many files, one set each, in one call
    for sets in calls:
        _, _, got = _provide(w, g, sets)
        for (f, runs), sl in zip(sets, got):
            assert sl == _expected(f, runs)[0], (g, f, runs[:4])


def test_one_run_a_file_is_the_range_call():
    import torch
    w = _world()
    m = w["m"]
    sets = [(f, ((n // 3, max(1, n // 2)),)) for f, n in enumerate(w["n"])]
    files, first, count = _arrays(sets)
    for g in (0, 4):
        d_slices, lay, _ = _provide(w, g, sets)
        ranged = m.bao.range_slices_arena(w["ctx"], w["d_src"], w["offsets"], w["lens"], w["made"][g]["outboards"], files, first, count, group_log=g)
        assert (ranged["slice_first"] == lay["slice_first"]).all()
        sizes = _sizes(w, sets)
        a, b = d_slices.cpu().numpy(), ranged["slices"].cpu().numpy()
        for at, size in zip(lay["slice_first"][:-1], sizes):
            assert (a[int(at):int(at) + size] == b[int(at):int(at) + size]).all()


def _have_bits(w, sets, ok=None):
    """the bitmap (int64 words) with the wanted chunks set (ok: per set, which of them)"""
    out = np.zeros(int(w["wf"][-1]), dtype=np.uint64)
    for i, (f, runs) in enumerate(sets):
        c = np.array(RS.chunks_of(runs), dtype=np.uint64)
        if ok is not None:
            c = c[np.asarray(ok[i], dtype=bool)]
        np.bitwise_or.at(out, (int(w["wf"][f]) + (c >> np.uint64(6))).astype(np.int64), np.uint64(1) << (c & np.uint64(63)))
    return out.view(np.int64)


def _receiver(w, g, seed=5):
    import torch
    size, total = w["arena"].size, int(w["made"][g]["ob_first"][-1])
    whole_a, d_arena = _walled(size)
    whole_o, d_obs = _walled(total)
    pre = np.random.default_rng(seed).integers(0, 1 << 63, int(w["wf"][-1]), dtype=np.int64)
    pre &= _have_bits(w, [(f, ((0, n),)) for f, n in enumerate(w["n"])])       # (the pad bits are the library's to leave clear)
    return dict(whole_a=whole_a, d_arena=d_arena, whole_o=whole_o, d_obs=d_obs, d_have=torch.from_numpy(pre.copy()).cuda(), pre=pre, size=size, total=total)


def _ingest(w, g, r, sets, d_slices, roots=None):
    files, first, count = _arrays(sets)
    return w["m"].bao.ingest_set_slices(w["ctx"], r["d_arena"], w["offsets"], w["lens"], r["d_obs"], w["roots"] if roots is None else roots, files, first, count,
                                        d_slices, group_log=g, d_have=r["d_have"])


def _host_ingest(w, g, sets, slices, roots):
    """the host call set by set -> (arena, outboards, have, set statuses, first bad, chunk statuses) from buffers of 0xEE"""
    m = w["m"]
    ob_first, wf = w["made"][g]["ob_first"], w["wf"]
    arena, obs = np.full(w["arena"].size, FILL, dtype=np.uint8), np.full(int(ob_first[-1]), FILL, dtype=np.uint8)
    have = np.zeros(int(wf[-1]), dtype=np.uint64)
    st, fb, cs = [], [], []
    for (f, runs), sl in zip(sets, slices):
        o, ln = int(w["offsets"][f]), w["lens"][f]
        x, y, z = m.bao.ingest_set_slice_host(arena[o:o + ln], obs[int(ob_first[f]):int(ob_first[f + 1])], ln, [a for a, _ in runs], [k for _, k in runs],
                                              roots[f], sl, g, have[int(wf[f]):int(wf[f + 1])])
        st.append(x)
        fb.append(-1 if y is None else y)
        cs += z.tolist()
    return arena, obs, have.view(np.int64), st, fb, cs


def _same_as_host(w, g, r, out, sets, slices, roots):
    want_arena, want_obs, want_have, st, fb, cs = _host_ingest(w, g, sets, slices, roots)
    assert out["set_status"].cpu().tolist() == st and out["set_first_bad"].cpu().tolist() == fb
    assert out["chunk_status"].cpu().tolist() == cs
    assert (r["d_arena"].cpu().numpy() == want_arena).all() and (r["d_obs"].cpu().numpy() == want_obs).all()
    assert (r["d_have"].cpu().numpy() == (r["pre"] | want_have)).all()
    assert _walls_intact(r["whole_a"], r["size"]) and _walls_intact(r["whole_o"], r["total"])
    return st, cs


def _receiver_sets(w):
    """a set a file: sparse, dense, across tiles and blocks"""
    f5, each, ends = _tile_sets(w)
    sets = []
    for f, n in enumerate(w["n"]):
        sh = set_shapes(n)
        name = ("every second chunk", "touching runs", "first and last chunk", "runs across the 64-chunk blocks", "the odd chunks", "one run")[f % 6]
        sets.append((f, tuple(sh.get(name, sh["the whole file"]))))
    sets[f5] = (f5, each[:-1] + ends[-2:])
    sets[f5 - 1] = (f5 - 1, tuple((c, 1) for c in range(0, w["n"][f5 - 1], 2)))
    return sets


@pytest.mark.parametrize("g", GS)
def test_the_receiver_against_the_host_call_and_the_projections(g):
    import torch
    w = _world()
    m = w["m"]
    sets = _receiver_sets(w)
    d_slices, lay, slices = _provide(w, g, sets)
    r = _receiver(w, g)
    out = _ingest(w, g, r, sets, d_slices)
    st, cs = _same_as_host(w, g, r, out, sets, slices, w["roots_host"])
    assert not any(st) and not any(cs)
    assert (out["set_chunk_first"] == lay["set_chunk_first"]).all()
    # the projections through the one-chunk device call write the same bytes
    files = np.concatenate([np.full(len(RS.chunks_of(runs)), f, dtype=np.uint32) for f, runs in sets])
    chunks = np.concatenate([np.array(RS.chunks_of(runs), dtype=np.uint64) for f, runs in sets])
    proj = [RS.project(sl, _expected(f, runs)[1], w["lens"][f], c) for (f, runs), sl in zip(sets, slices) for c in RS.chunks_of(runs)]
    p = _receiver(w, g)
    one = m.bao.ingest_slices(w["ctx"], p["d_arena"], w["offsets"], w["lens"], p["d_obs"], w["roots"], files, chunks,
                              torch.from_numpy(_packed(m, w["ln"], files, chunks, proj)).cuda(), group_log=g, d_have=p["d_have"])["sample_status"]
    assert not one.any().item()
    assert torch.equal(p["d_arena"], r["d_arena"]) and torch.equal(p["d_obs"], r["d_obs"]) and torch.equal(p["d_have"], r["d_have"])
    # without a chunk status and without a bitmap: the same sets' verdicts
    files, first, count = _arrays(sets)
    q = _receiver(w, g)
    d_st = torch.full((len(sets),), -1, dtype=torch.int32, device="cuda")
    d_fb = torch.full((len(sets),), -2, dtype=torch.int64, device="cuda")
    need = m.lib().b3w_bao_set_slice_ingest_scratch_bytes(w["ln"].ctypes.data, len(w["lens"]), files.ctypes.data, first.ctypes.data, count.ctypes.data, files.size)
    d_scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert _c_ingest(w, g, q, sets, d_slices, d_st, d_fb, None, d_scratch, d_have=None) == 0, w["ctx"].last_error()
    torch.cuda.synchronize()
    assert not d_st.any().item() and bool((d_fb == -1).all().item())
    assert torch.equal(q["d_arena"], r["d_arena"]) and torch.equal(q["d_obs"], r["d_obs"]) and (q["d_have"].cpu().numpy() == q["pre"]).all()


@pytest.mark.parametrize("g", [0, 4])
def test_tampered_sets_beside_good_ones(g):
    import torch
    w = _world()
    m = w["m"]
    sets = _receiver_sets(w)
    one = next(f for f, ln in enumerate(w["lens"]) if 0 < ln <= K)
    victims = [w["lens"].index(K * 1025), w["lens"].index(70 * K + 1), len(w["lens"]) - 1, len(w["lens"]) - 2, one]
    kinds = {f: tampers(*_expected(f, sets[f][1]), RS.chunks_of(sets[f][1]), w["lens"][f], [int(x) for x in w["roots_host"][f]]) for f in victims}
    seen = set()
    for i in range(max(len(k) for k in kinds.values())):
        slices, hit = [_expected(f, runs)[0] for f, runs in sets], {}
        for f in victims:                                                  # tamper i of every victim that has one, beside the good sets
            what, bad_sl, rt, node = kinds[f][i % len(kinds[f])]
            if what != "wrong root" and i < len(kinds[f]):                 # (the roots are the call's, one a file: see below)
                slices[f], hit[f] = bad_sl, (what, node)
        r = _receiver(w, g)
        out = _ingest(w, g, r, sets, torch.from_numpy(_pack(w, sets, slices)).cuda())
        st, cs = _same_as_host(w, g, r, out, sets, slices, w["roots_host"])
        assert all((st[f] != 0) == (f in hit) for f in range(len(sets))), (g, i, st, hit)
        at = out["set_chunk_first"]
        for f, (what, node) in hit.items():
            mine, wanted = cs[int(at[f]):int(at[f + 1])], RS.chunks_of(sets[f][1])
            if node:                                                       # a bad node keeps out the chunks below it and no other
                assert mine == [2 if node[0] <= c < node[0] + node[1] else 0 for c in wanted], (g, f, what)
            seen |= set(mine)
    assert seen == {0, 1, 2, 3}
    # a wrong root: every chunk of that file is 2 (1 for a one-chunk file) and nothing of it is written
    roots = w["roots"].clone()
    for f in victims:
        roots.view(-1)[8 * f + 3] ^= 0x10000
    slices = [_expected(f, runs)[0] for f, runs in sets]
    r = _receiver(w, g)
    out = _ingest(w, g, r, sets, torch.from_numpy(_pack(w, sets, slices)).cuda(), roots=roots)
    st, cs = _same_as_host(w, g, r, out, sets, slices, roots.cpu().numpy().view(np.uint32).reshape(-1, 8))
    assert [st[f] for f in victims] == [2, 2, 2, 2, 1] and sum(1 for x in st if x) == len(victims)


@pytest.mark.parametrize("g", [0, 4])
def test_the_loop_closes_with_sets(g):
    """have_runs -> set_slices_arena -> ingest_set_slices until nothing is missing, about 30 % of the first round's chunks tampered"""
    import torch
    w = _world()
    m = w["m"]
    r = _receiver(w, g)
    r["d_have"].zero_()
    rng = np.random.default_rng(900 + g)
    rounds = 0
    while True:
        runs = m.bao.have_runs(w["ctx"], r["d_have"], w["lens"], kind="missing")
        files, first, count = runs["files"], runs["first_chunks"], runs["n_chunks"]
        if not len(files):
            break
        assert rounds < 4
        out = m.bao.set_slices_arena(w["ctx"], w["d_src"], w["offsets"], w["lens"], w["made"][g]["outboards"], files, first, count, group_log=g)
        d_slices = out["slices"]
        total = int(out["set_chunk_first"][-1])
        bad = np.zeros(total, dtype=bool)
        if rounds == 0:
            assert total == sum(w["n"])
            sets = [(f, ((0, n),)) for f, n in enumerate(w["n"])]
            bad = rng.random(total) < 0.3
            at = []
            for s, (f, runs_f) in enumerate(sets):
                places = _expected(f, runs_f)[1]
                for c in range(w["n"][f]):
                    i = int(out["set_chunk_first"][s]) + c
                    size = min(w["lens"][f], (c + 1) * K) - c * K
                    if size == 0:
                        bad[i] = False                                     # (an empty chunk has no byte to flip)
                    if bad[i]:
                        at.append(int(out["slice_first"][s]) + places[("chunk", c)] + (c * 13) % size)
            d_slices[torch.from_numpy(np.array(at, dtype=np.int64)).cuda()] ^= 1
        got = m.bao.ingest_set_slices(w["ctx"], r["d_arena"], w["offsets"], w["lens"], r["d_obs"], w["roots"], files, first, count, d_slices, group_log=g,
                                      d_have=r["d_have"])
        cs = got["chunk_status"].cpu().numpy()
        assert ((cs != 0) == bad).all() and set(cs[bad].tolist()) <= {1}
        rounds += 1
    assert rounds == 2
    assert runs["file_have"].cpu().tolist() == w["n"] and int(runs["n_runs"].item()) == 0
    got = r["d_arena"].cpu().numpy()
    assert (got[w["in_file"]] == w["arena"][w["in_file"]]).all() and (got[~w["in_file"]] == FILL).all()
    assert torch.equal(r["d_obs"], w["made"][g]["outboards"][:r["total"]])
    assert _walls_intact(r["whole_a"], r["size"]) and _walls_intact(r["whole_o"], r["total"])


def _fabricate(length, wanted, chosen, rng):
    """the set slice of a file of which only the wanted chunks (index -> bytes) are known: arbitrary CVs for every subtree that does not
    meet the set, parents hashed up to a root -> (slice, root words, {(lo, size): node bytes})"""
    n = R.num_chunks(length)
    out, nodes = [struct.pack("<Q", length)], {}

    def walk(lo, m, root):
        if not RS._meets(wanted, lo, lo + m):
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


def _preorder(n, lo, size):
    p, first, m = 0, 0, n
    while (first, m) != (lo, size):
        k = R._split(m)
        if lo < first + k:
            p, m = p + 1, k
        else:
            p, first, m = p + k, first + k, m - k
    return p


def test_places_past_4_gib():
    """one fictitious file of 5 GiB + 300 B in an arena that is never initialised: a set of a chunk in the first tile, a run across chunk
    2^22 (past byte 2^32) and the ragged last chunk, its slice built on the host with blake3_ref; only its own places are read back"""
    import torch
    w = _world()
    m = w["m"]
    length = (5 << 30) + 300
    n = m.bao.num_chunks(length)
    rng = np.random.default_rng(65)
    runs = [(7, 1), ((1 << 22) - 1, 3), (n - 1, 1)]
    wanted = RS.chunks_of(runs)
    chosen = {c: rng.integers(0, 256, min(K, length - c * K), dtype=np.uint8).tobytes() for c in wanted}
    sl, root, nodes = _fabricate(length, wanted, chosen, rng)
    first, count = [a for a, _ in runs], [k for _, k in runs]
    assert len(sl) == m.bao.set_slice_size(length, first, count)
    st, fb, cs, _ = m.bao.decode_set_slice(sl, length, first, count, root)
    assert (st, fb, cs.tolist()) == (0, None, [0] * 5)
    lens = np.array([length], dtype=np.uint64)
    packed = np.full(int(m.bao.set_slice_layout(lens, [0, 0, 0], first, count)["slice_first"][-1]), PAD, dtype=np.uint8)
    packed[8:8 + len(sl)] = np.frombuffer(sl, dtype=np.uint8)
    d_roots = torch.from_numpy(np.array(root, dtype=np.uint32).view(np.int32)).cuda()
    skew = 1                                                              # the file starts at an odd byte of the arena
    d_arena = torch.empty(length + 16, dtype=torch.uint8, device="cuda")
    d_obs = torch.empty(int(m.bao.batch_layout(lens)[-1]), dtype=torch.uint8, device="cuda")
    d_have = m.bao.have_new(lens)
    out = m.bao.ingest_set_slices(w["ctx"], d_arena, [skew], lens, d_obs, d_roots, [0, 0, 0], first, count, torch.from_numpy(packed).cuda(), d_have=d_have)
    assert out["set_status"].cpu().tolist() == [0] and out["set_first_bad"].cpu().tolist() == [-1] and out["chunk_status"].cpu().tolist() == [0] * 5
    assert d_obs[:8].cpu().numpy().tobytes() == struct.pack("<Q", length)
    for (lo, size), node in nodes.items():
        i = _preorder(n, lo, size)
        assert d_obs[8 + 64 * i:8 + 64 * i + 64].cpu().numpy().tobytes() == node, (lo, size)
    for c in wanted:
        at = skew + c * K
        assert d_arena[at:at + len(chosen[c])].cpu().numpy().tobytes() == chosen[c], c
        assert (int(d_have[c >> 6].item()) >> (c & 63)) & 1
    assert int((d_have != 0).sum().item()) == 4
    # and the provider's places: the slice back out of what was taken in
    back = torch.full((packed.size,), PAD, dtype=torch.uint8, device="cuda")
    fi, fc, nc = np.zeros(3, dtype=np.uint32), np.array(first, dtype=np.uint64), np.array(count, dtype=np.uint64)
    off = np.array([skew], dtype=np.uint64)
    assert m.lib().b3w_bao_set_slice_arena_device(w["ctx"].handle, d_arena.data_ptr(), d_arena.numel(), off.ctypes.data, lens.ctypes.data, 1, 0, d_obs.data_ptr(),
                                                  fi.ctypes.data, fc.ctypes.data, nc.ctypes.data, 3, back.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    assert back.cpu().numpy().tobytes() == packed.tobytes()
    del d_arena, d_obs


def _c_ingest(w, g0, r, sets, slices0, st0, fb0, cs0, scratch0, **change):
    import torch
    files, first, count = _arrays(sets)
    kw = dict(ctx=w["ctx"].handle, d_arena=r["d_arena"].data_ptr(), arena_bytes=r["size"], offsets=w["offsets"].ctypes.data, lens=w["ln"].ctypes.data,
              n_files=len(w["lens"]), g=g0, d_obs=r["d_obs"].data_ptr(), d_roots=w["roots"].data_ptr(), files=files.ctypes.data, first=first.ctypes.data,
              count=count.ctypes.data, n_ranges=files.size, d_slices=slices0.data_ptr(), d_st=st0.data_ptr(), d_fb=fb0.data_ptr(),
              d_cs=cs0.data_ptr() if cs0 is not None else None, d_have=r["d_have"].data_ptr(), d_scratch=scratch0.data_ptr(), scratch_bytes=scratch0.numel())
    for name, value in change.items():
        kw[name] = value.ctypes.data if isinstance(value, np.ndarray) else value
    return w["m"].lib().b3w_bao_set_slice_ingest_device(*kw.values(), torch.cuda.current_stream().cuda_stream)


def _c_provide(w, g0, sets, slices0, **change):
    import torch
    files, first, count = _arrays(sets)
    kw = dict(ctx=w["ctx"].handle, d_arena=w["d_src"].data_ptr(), arena_bytes=w["d_src"].numel(), offsets=w["offsets"].ctypes.data, lens=w["ln"].ctypes.data,
              n_files=len(w["lens"]), g=g0, d_obs=w["made"][g0]["outboards"].data_ptr(), files=files.ctypes.data, first=first.ctypes.data,
              count=count.ctypes.data, n_ranges=files.size, d_slices=slices0.data_ptr())
    for name, value in change.items():
        kw[name] = value.ctypes.data if isinstance(value, np.ndarray) else value
    return w["m"].lib().b3w_bao_set_slice_arena_device(*kw.values(), torch.cuda.current_stream().cuda_stream)


def _outputs(w, sets):
    import torch
    m = w["m"]
    files, first, count = _arrays(sets)
    lay = m.bao.set_slice_layout(w["ln"], files, first, count)
    d_st = torch.full((len(sets),), -1, dtype=torch.int32, device="cuda")
    d_fb = torch.full((len(sets),), -2, dtype=torch.int64, device="cuda")
    d_cs = torch.full((int(lay["set_chunk_first"][-1]),), -3, dtype=torch.int32, device="cuda")
    need = m.lib().b3w_bao_set_slice_ingest_scratch_bytes(w["ln"].ctypes.data, len(w["lens"]), files.ctypes.data, first.ctypes.data, count.ctypes.data, files.size)
    return lay, d_st, d_fb, d_cs, need


def test_the_two_calls_allocate_nothing():
    import torch
    w = _world()
    sets = _receiver_sets(w)
    lay, d_st, d_fb, d_cs, need = _outputs(w, sets)
    rows = 0
    for f, runs in sets:                                                   # a row per touched block of 64 or of 1 024 chunks
        c = RS.chunks_of(runs)
        B_ = 64 if c[-1] // 64 - c[0] // 64 <= 1 else 1024
        rows += len({x // B_ for x in c})
    assert need == 16 * rows
    d_slices = torch.empty(int(lay["slice_first"][-1]), dtype=torch.uint8, device="cuda")
    d_scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    r = _receiver(w, 0)
    for _ in range(2):                                                    # (the context's staging grows in the first round, outside the allocator)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        assert _c_provide(w, 0, sets, d_slices) == 0, w["ctx"].last_error()
        assert _c_ingest(w, 0, r, sets, d_slices, d_st, d_fb, d_cs, d_scratch) == 0, w["ctx"].last_error()
        torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == before
    assert not d_st.any().item() and bool((d_fb == -1).all().item()) and not d_cs.any().item()


def test_refusals_leave_every_output_and_the_scratch_untouched():
    import torch
    w = _world()
    m = w["m"]
    g = 0
    sets = _receiver_sets(w)
    d_good, lay, _ = _provide(w, g, sets)
    _, d_st, d_fb, d_cs, need = _outputs(w, sets)
    r = _receiver(w, g)
    d_scratch = torch.full((need,), 0x77, dtype=torch.uint8, device="cuda")
    d_slices = torch.full((int(lay["slice_first"][-1]),), PAD, dtype=torch.uint8, device="cuda")
    pre = r["d_have"].clone()
    src_obs = w["made"][g]["outboards"].clone()

    def untouched():
        torch.cuda.synchronize()
        return (bool((r["d_arena"] == FILL).all().item()) and bool((r["d_obs"] == FILL).all().item()) and bool((d_st == -1).all().item())
                and bool((d_fb == -2).all().item()) and bool((d_cs == -3).all().item()) and bool((d_scratch == 0x77).all().item())
                and torch.equal(r["d_have"], pre) and bool((d_slices == PAD).all().item()) and torch.equal(w["made"][g]["outboards"], src_obs))

    def both(**change):
        """refused by the receiver, and by the provider where it takes the argument"""
        rc = _c_ingest(w, g, r, sets, d_good, d_st, d_fb, d_cs, d_scratch, **change)
        mine = {k: v for k, v in change.items() if k in ("ctx", "arena_bytes", "offsets", "lens", "g", "files", "first", "count", "n_ranges")}
        rc2 = _c_provide(w, g, sets, d_slices, **mine) if mine else BAD
        return rc == BAD and rc2 == BAD and untouched()
    files, first, count = _arrays(sets)
    assert both(ctx=None) and both(g=7)
    for name in ("offsets", "lens", "files", "first", "count", "d_obs", "d_roots", "d_slices", "d_st", "d_fb", "d_scratch"):
        assert both(**{name: None}), name
    assert _c_provide(w, g, sets, d_slices, d_obs=None) == BAD and _c_provide(w, g, sets, d_slices, d_slices=None) == BAD and untouched()
    assert both(d_obs=r["d_obs"].data_ptr() + 4) and both(d_slices=d_good.data_ptr() + 8) and both(d_fb=d_fb.data_ptr() + 4) and both(d_st=d_st.data_ptr() + 2)
    assert _c_provide(w, g, sets, d_slices, d_slices=d_slices.data_ptr() + 8) == BAD and untouched()
    assert both(d_have=r["d_have"].data_ptr() + 4), "a misaligned bitmap"
    assert both(d_cs=d_cs.data_ptr() + 2), "a misaligned chunk status"
    assert both(d_scratch=d_scratch.data_ptr() + 8), "a misaligned scratch"
    assert both(scratch_bytes=need - 16), "a scratch that is too small"
    last = files.size - 1
    j = next(i for i in range(2, files.size) if files[i] == files[i - 2])  # the third run of a set
    assert files[last - 1] > 0
    for what, at, value, named in (("files", last, len(w["lens"]), "file index"), ("count", 0, 0, "no chunk"), ("first", last, 1 << 40, "past"),
                                   ("count", last, 1 << 40, "past"), ("first", j, int(first[j - 1]), "disjoint"), ("first", j, int(first[j - 2]), "ascending"),
                                   ("files", last, 0, "ascending")):
        bad = {"files": files, "first": first, "count": count}[what].copy()
        bad[at] = value
        assert both(**{what: bad}), (what, at, value)
        assert "range" in w["ctx"].last_error() and named in w["ctx"].last_error(), w["ctx"].last_error()
    reach = max(int(w["offsets"][f]) + w["lens"][f] for f, _ in sets)
    assert both(arena_bytes=reach - 1), "a file that reaches past arena_bytes"
    with pytest.raises(m.B3WError):
        m.bao.ingest_set_slices(w["ctx"], r["d_arena"], w["offsets"], w["lens"], r["d_obs"], w["roots"], files, first, count, d_good, group_log=7)
    with pytest.raises(m.B3WError):
        m.bao.set_slices_arena(w["ctx"], w["d_src"], w["offsets"], w["lens"], w["made"][0]["outboards"], [0, 0], [1, 0], [1, 1])
    # no ranges: a no-op, whatever else is handed in
    L = m.lib()
    assert L.b3w_bao_set_slice_ingest_device(w["ctx"].handle, None, 0, None, None, 0, 0, None, None, None, None, None, 0, None, None, None, None, None, None, 0, None) == 0
    assert L.b3w_bao_set_slice_arena_device(w["ctx"].handle, None, 0, None, None, 0, 0, None, None, None, None, 0, None, None) == 0
    assert untouched()
    # and the same arguments unchanged are taken
    assert _c_ingest(w, g, r, sets, d_good, d_st, d_fb, d_cs, d_scratch) == 0, w["ctx"].last_error()
    torch.cuda.synchronize()
    assert not d_st.any().item() and bool((d_fb == -1).all().item()) and not d_cs.any().item()
    assert _walls_intact(r["whole_a"], r["size"]) and _walls_intact(r["whole_o"], r["total"])
