"""Slices taken into packed chunk slots, without a GPU (b3w_bao_slice_ingest_packed_device, b3w_bao_range_slice_ingest_packed_device,
b3w_bao_set_slice_ingest_packed_device; bao.ingest_slices_packed, ingest_range_slices_packed, ingest_set_slices_packed, chunk_slots,
scatter_chunks): the names and their argument lists against the arena twins', chunk_slots against a plain loop, scatter_chunks there and
back (buffers and file objects, touching chunks in one write), the refusals that need no device, and the stand-alone check of the host
side (tools/bao_receive_packed_host_check.cpp) compiled and run."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import b3w_testlib as T

BAD = 100
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWINS = {"b3w_bao_slice_ingest_packed_device": "b3w_bao_slice_ingest_have_device", "b3w_bao_range_slice_ingest_packed_device": "b3w_bao_range_slice_ingest_device",
         "b3w_bao_set_slice_ingest_packed_device": "b3w_bao_set_slice_ingest_device"}
LENS = [0, 1, 1023, 1024, 1025, 3 * 1024 + 17, 5 * 1024 + 300, 64 * 1024 + 999, 70 * 1024 + 1, 1025 * 1024]


def _declared(header, name):
    """the parameter names of the header's declaration of `name`"""
    decl = re.search(r"int32_t " + name + r"\(([^;]*)\);", header).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    return [re.search(r"(\w+)\s*$", p.strip()).group(1) for p in decl.split(",")]


def test_the_names_and_their_argument_lists():
    m = T.pkg()
    L = m.lib()
    assert L.b3w_abi_version() == (1 << 16) | 4                            # new names only
    header = open(os.path.join(ROOT, "include", "b3wit.h")).read()
    for name, twin in TWINS.items():
        assert name in m.EXPORTED_SYMBOLS and hasattr(L, name)
        args, arena = _declared(header, name), _declared(header, twin)
        assert arena[:4] == ["ctx", "d_arena", "arena_bytes", "host_offsets"] and args == ["ctx", "d_chunks", "chunks_bytes"] + arena[4:], name
        assert len(getattr(L, name).argtypes) == len(args), name
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(m.bao.ingest_slices_packed) == ["ctx", "lens", "d_outboards", "d_roots", "files", "chunks", "d_slices", "group_log", "stream", "d_have", "d_chunks"]
    ranged = ["ctx", "lens", "d_outboards", "d_roots", "files", "first_chunks", "n_chunks", "d_slices", "group_log", "stream", "d_have", "d_chunks"]
    assert sig(m.bao.ingest_range_slices_packed) == ranged and sig(m.bao.ingest_set_slices_packed) == ranged
    for fn, twin in ((m.bao.ingest_slices_packed, m.bao.ingest_slices), (m.bao.ingest_range_slices_packed, m.bao.ingest_range_slices),
                     (m.bao.ingest_set_slices_packed, m.bao.ingest_set_slices)):
        assert [a for a in sig(twin) if a not in ("d_arena", "offsets")] + ["d_chunks"] == sig(fn)
        assert all(inspect.signature(fn).parameters[a].default is None for a in ("d_have", "d_chunks"))
    assert sig(m.bao.chunk_slots) == ["lens", "files", "first_chunks", "n_chunks"] and sig(m.bao.scatter_chunks) == ["dest", "chunks_host", "chunk_status", "slots"]


def _some_list(rng):
    """ranges over LENS that overlap, repeat and come in any order, the empty file and the short last chunks among them"""
    files, first, count = [], [], []
    for f, ln in enumerate(LENS):
        n = max(1, (ln + 1023) // 1024)
        files += [f, f]
        first += [0, n - 1]
        count += [n, 1]
        for _ in range(3):
            a = int(rng.integers(0, n))
            files.append(f)
            first.append(a)
            count.append(int(rng.integers(1, n - a + 1)))
    perm = rng.permutation(len(files))
    return np.array(files, dtype=np.uint32)[perm], np.array(first, dtype=np.uint64)[perm], np.array(count, dtype=np.uint64)[perm]


def test_chunk_slots_against_a_plain_loop():
    m = T.pkg()
    files, first, count = _some_list(np.random.default_rng(1))
    f, c, off, nb = m.bao.chunk_slots(LENS, files, first, count)
    want = [(int(fi), ch, 1024 * ch, max(0, min(1024, LENS[fi] - 1024 * ch))) for fi, a, k in zip(files, first.tolist(), count.tolist()) for ch in range(a, a + k)]
    assert (f.dtype, c.dtype, off.dtype, nb.dtype) == (np.uint32, np.uint64, np.uint64, np.uint32)
    assert list(zip(f.tolist(), c.tolist(), off.tolist(), nb.tolist())) == want and len(want) == int(count.sum())
    assert 0 in nb.tolist() and 1 in nb.tolist() and 300 in nb.tolist()     # the empty file's chunk and the short last ones
    # the slots are the status indices the existing layouts give: the running sum of the counts, and set_chunk_first for a set list
    order = np.lexsort((first, files))
    sf, sa, sk = files[order][::5], np.zeros(len(LENS), dtype=np.uint64), np.ones(len(LENS), dtype=np.uint64)
    lay = m.bao.set_slice_layout(LENS, sf, sa, sk)
    assert lay["set_chunk_first"].tolist() == list(range(len(LENS) + 1)) and m.bao.chunk_slots(LENS, sf, sa, sk)[0].tolist() == sf.tolist()
    one = m.bao.chunk_slots(LENS, [9, 6, 9], [1024, 5, 1024], np.ones(3, dtype=np.uint64))     # one-chunk samples: counts of one
    assert one[1].tolist() == [1024, 5, 1024] and one[3].tolist() == [1024, 300, 1024]
    assert all(x.size == 0 for x in m.bao.chunk_slots(LENS, [], [], []))
    for fi, fc, nc in (([10], [0], [1]), ([4], [2], [1]), ([4], [1], [2]), ([0], [1], [1]), ([0, 1], [0], [1])):
        with pytest.raises(m.B3WError):
            m.bao.chunk_slots(LENS, fi, fc, nc)


class _File:
    """a file object that keeps its writes"""

    def __init__(self, size):
        self.data, self.at, self.writes = bytearray(size), 0, []

    def seek(self, at):
        self.at = at

    def write(self, b):
        self.data[self.at:self.at + len(b)] = b
        self.writes.append((self.at, len(b)))
        self.at += len(b)


def test_scatter_chunks_there_and_back():
    import torch
    m = T.pkg()
    rng = np.random.default_rng(2)
    source = [rng.integers(1, 256, ln, dtype=np.uint8) for ln in LENS]      # (no zero byte: an unwritten place shows)
    files, first, count = _some_list(rng)
    slots = m.bao.chunk_slots(LENS, files, first, count)
    f, c, off, nb = slots
    buf = np.full((f.size, 1024), 0xEE, dtype=np.uint8)
    for k in range(f.size):
        buf[k, :nb[k]] = source[f[k]][int(off[k]):int(off[k]) + int(nb[k])]
    # every slot verified: the files come back whole (every file has a whole-file range), into buffers of three kinds
    dest = [np.zeros(ln, dtype=np.uint8) if i % 3 == 0 else bytearray(ln) if i % 3 == 1 else memoryview(bytearray(ln)) for i, ln in enumerate(LENS)]
    assert m.bao.scatter_chunks(dest, buf, None, slots) == int(nb.sum())
    assert all(bytes(d) == s.tobytes() for d, s in zip(dest, source))
    # a status a slot: exactly the verified slots' bytes, whatever the others hold
    status = (rng.random(f.size) < 0.4).astype(np.int32) * rng.integers(1, 4, f.size).astype(np.int32)
    spoiled = buf.copy()
    spoiled[status != 0] = 0x5A
    want = [np.zeros(ln, dtype=np.uint8) for ln in LENS]
    for k in np.flatnonzero(status == 0):
        want[f[k]][int(off[k]):int(off[k]) + int(nb[k])] = source[f[k]][int(off[k]):int(off[k]) + int(nb[k])]
    for chunks_host, st in ((spoiled, status), (torch.from_numpy(spoiled).reshape(-1), torch.from_numpy(status))):
        dest = [np.zeros(ln, dtype=np.uint8) for ln in LENS]
        assert m.bao.scatter_chunks(dest, chunks_host, st, slots) == int(nb[status == 0].sum())
        assert all((d == x).all() for d, x in zip(dest, want))
    # file objects, and touching chunks in ONE write: a run of k chunks is one write, a bad chunk in its middle makes it two
    order = np.lexsort((first, files))
    files, first, count = files[order], first[order], count[order]
    slots = f, c, off, nb = m.bao.chunk_slots(LENS, files, first, count)
    buf = np.zeros((f.size, 1024), dtype=np.uint8)
    for k in range(f.size):
        buf[k, :nb[k]] = source[f[k]][int(off[k]):int(off[k]) + int(nb[k])]
    out = [_File(ln) for ln in LENS]
    m.bao.scatter_chunks(out, buf, None, slots)
    assert all(bytes(o.data) == s.tobytes() for o, s in zip(out, source))
    ranges_with_bytes = sum(1 for fi, a in zip(files.tolist(), first.tolist()) if LENS[fi] > 1024 * a)
    assert sum(len(o.writes) for o in out) <= ranges_with_bytes < int((nb > 0).sum())
    whole = next(i for i, (fi, k) in enumerate(zip(files.tolist(), count.tolist())) if fi == 9 and k == 1025)
    k0 = int(count[:whole].sum())
    status = np.zeros(f.size, dtype=np.int32)
    status[k0 + 500] = 1
    one = [_File(ln) for ln in LENS]
    part = tuple(x[k0:k0 + 1025] for x in slots)
    m.bao.scatter_chunks(one, buf[k0:k0 + 1025], status[k0:k0 + 1025], part)
    assert one[9].writes == [(0, 500 * 1024), (501 * 1024, 524 * 1024)]
    # refusals: a slot buffer or a status list of another size, a destination that is too short
    with pytest.raises(m.B3WError):
        m.bao.scatter_chunks(out, buf[:-1], None, slots)
    with pytest.raises(m.B3WError):
        m.bao.scatter_chunks(out, buf, np.zeros(3), slots)
    with pytest.raises(m.B3WError):
        m.bao.scatter_chunks([np.zeros(max(0, ln - 1), dtype=np.uint8) for ln in LENS], buf, None, slots)


def test_a_null_context_and_a_malformed_list_are_refused_and_nothing_is_written():
    m = T.pkg()
    L = m.lib()
    lens = np.array([5 * 1024 + 7, 70 * 1024], dtype=np.uint64)
    files, first, count = np.array([0, 0, 1], dtype=np.uint32), np.array([1, 4, 3], dtype=np.uint64), np.array([2, 2, 62], dtype=np.uint64)
    out = [np.full(64, 0xEE, dtype=np.uint8) for _ in range(9)]              # host memory in the device pointers' places: a refusal reads and writes none of it
    chunks, obs, roots, slices, st, fb, cs, have, scratch = (x.ctypes.data for x in out)
    a = (lens.ctypes.data, 2, 0, obs, roots, files.ctypes.data, first.ctypes.data)
    assert L.b3w_bao_slice_ingest_packed_device(None, chunks, 64, *a, 3, slices, st, have, None) == BAD
    assert L.b3w_bao_range_slice_ingest_packed_device(None, chunks, 64, *a, count.ctypes.data, 3, slices, st, fb, have, scratch, 64, None) == BAD
    assert L.b3w_bao_set_slice_ingest_packed_device(None, chunks, 64, *a, count.ctypes.data, 3, slices, st, fb, cs, have, scratch, 64, None) == BAD
    assert L.b3w_bao_set_slice_ingest_packed_device(None, None, 0, None, 0, 0, None, None, None, None, None, 0, None, None, None, None, None, None, 0, None) == BAD
    assert all((x == 0xEE).all() for x in out)
    # the list is looked at before any tensor: a file index, an empty range, one past the file; sets: unsorted, overlapping, a file that comes back
    for fi, fc, nc in (([2], [0], [1]), ([0], [1], [0]), ([0], [5], [2])):
        with pytest.raises(m.B3WError):
            m.bao.ingest_range_slices_packed(None, lens, None, None, fi, fc, nc, None)
        with pytest.raises(m.B3WError):
            m.bao.ingest_set_slices_packed(None, lens, None, None, fi, fc, nc, None)
    for fi, fc, nc in (([0, 0], [4, 1], [1, 1]), ([0, 0], [1, 2], [2, 1]), ([1, 0], [0, 0], [1, 1])):
        with pytest.raises(m.B3WError):
            m.bao.ingest_set_slices_packed(None, lens, None, None, fi, fc, nc, None)
    for fi, ch in (([2], [0]), ([0], [6])):
        with pytest.raises(m.B3WError):
            m.bao.ingest_slices_packed(None, lens, None, None, fi, ch, None)
    for fn in (m.bao.ingest_range_slices_packed, m.bao.ingest_set_slices_packed):
        with pytest.raises(m.B3WError):
            fn(None, lens, None, None, [0], [1], [1], None, group_log=7)
    with pytest.raises(m.B3WError):
        m.bao.ingest_slices_packed(None, lens, None, None, [0], [1], None, group_log=7)


def test_the_stand_alone_host_check_builds_and_passes(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    pkg = os.path.join(ROOT, "hot-proofs-blake3-circom_amd", "csrc")
    exe = str(tmp_path / "bao_receive_packed_host_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", pkg, os.path.join(pkg, "b3w_bao_host.cpp"),
                    os.path.join(ROOT, "tools", "bao_receive_packed_host_check.cpp"), "-o", exe], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "checks passed" in done.stdout
