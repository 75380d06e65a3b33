"""The set planner and the packed set provider without a GPU (b3w_sample_plan_set_slices_device, b3w_bao_set_slice_packed_device;
bao.plan_samples_set_slices, prove_samples_set_slices, set_slices_packed): the names and their argument lists, the refusals that need no
device, the facts the planner's output layout rests on - for an ascending disjoint list the record rows are b3w_sample_rows_ranges' and
the chunk statuses' places the running sum of the counts - through the existing host calls over test_bao_set_cpu's 51 lengths and shapes,
and the stand-alone check of the host arithmetic beside the set table (tools/bao_set_plan_host_check.cpp) compiled and run."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import b3w_testlib as T
import bao_set_ref as RS
from test_bao_range_cpu import ALL_LENGTHS
from test_bao_set_cpu import set_shapes

BAD = 100
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_ARGS = ["ctx", "host_lens", "n_files", "d_roots", "host_files", "host_first", "host_count", "n_ranges", "d_slices", "d_records", "d_chunk_status",
             "d_set_status", "d_set_first_bad", "d_scratch", "scratch_bytes", "stream"]
PACKED_ARGS = ["ctx", "d_packed", "packed_bytes", "host_lens", "n_files", "group_log", "d_outboards", "host_files", "host_first", "host_count", "n_ranges",
               "d_slices", "stream"]


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
    for name, args in (("b3w_sample_plan_set_slices_device", PLAN_ARGS), ("b3w_bao_set_slice_packed_device", PACKED_ARGS)):
        assert name in m.EXPORTED_SYMBOLS and hasattr(L, name)
        assert _declared(header, name) == args and len(getattr(L, name).argtypes) == len(args), name
    # the twins' lists: the range planner's with the set pair, the arena provider's with (d_packed, packed_bytes) for the arena's three
    assert [a.replace("d_range_", "d_set_") for a in _declared(header, "b3w_sample_plan_range_slices_device")] == PLAN_ARGS
    arena = _declared(header, "b3w_bao_set_slice_arena_device")
    assert arena[:4] == ["ctx", "d_arena", "arena_bytes", "host_offsets"] and ["ctx", "d_packed", "packed_bytes"] + arena[4:] == PACKED_ARGS
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(m.bao.plan_samples_set_slices) == ["ctx", "lens", "d_roots", "files", "first_chunks", "n_chunks", "d_slices", "stream"]
    assert sig(m.bao.plan_samples_set_slices) == sig(m.bao.plan_samples_range_slices)
    assert sig(m.bao.prove_samples_set_slices) == sig(m.bao.prove_samples_range_slices)
    assert sig(m.bao.set_slices_packed) == ["ctx", "d_packed", "lens", "d_outboards", "files", "first_chunks", "n_chunks", "group_log", "stream"]
    assert sig(m.bao.set_slices_packed) == sig(m.bao.range_slices_packed)
    assert inspect.signature(m.bao.set_slices_packed).parameters["group_log"].default == 0


def test_a_null_context_and_a_malformed_list_are_refused_and_nothing_is_written():
    m = T.pkg()
    L = m.lib()
    lens = np.array([5 * 1024 + 7, 70 * 1024], dtype=np.uint64)
    files, first, count = np.array([0, 0, 1], dtype=np.uint32), np.array([1, 4, 3], dtype=np.uint64), np.array([2, 2, 62], dtype=np.uint64)
    out = [np.full(64, 0xEE, dtype=np.uint8) for _ in range(8)]              # host memory in the device pointers' places: a refusal reads and writes none of it
    roots, slices, recs, st, sst, sfb, scratch, obs = (x.ctypes.data for x in out)
    assert L.b3w_sample_plan_set_slices_device(None, lens.ctypes.data, 2, roots, files.ctypes.data, first.ctypes.data, count.ctypes.data, 3, slices, recs, st, sst, sfb,
                                               scratch, 64, None) == BAD
    assert L.b3w_bao_set_slice_packed_device(None, slices, 64, lens.ctypes.data, 2, 0, obs, files.ctypes.data, first.ctypes.data, count.ctypes.data, 3, recs, None) == BAD
    assert L.b3w_sample_plan_set_slices_device(None, None, 0, None, None, None, None, 0, None, None, None, None, None, None, 0, None) == BAD
    assert all((x == 0xEE).all() for x in out)
    # the list is looked at before any tensor: unsorted, overlapping, empty, past the file, a file that comes back
    for fi, fc, nc in (([0, 0], [4, 1], [1, 1]), ([0, 0], [1, 2], [2, 1]), ([0], [1], [0]), ([0], [5], [2]), ([1, 0], [0, 0], [1, 1]), ([2], [0], [1])):
        with pytest.raises(m.B3WError):
            m.bao.plan_samples_set_slices(None, lens, None, fi, fc, nc, None)
        with pytest.raises(m.B3WError):
            m.bao.set_slices_packed(None, None, lens, None, fi, fc, nc)
    with pytest.raises(m.B3WError):
        m.bao.set_slices_packed(None, None, lens, None, [0], [1], [1], group_log=7)


def test_the_layout_the_planner_rests_on():
    """over the set CPU test's 51 lengths and shapes, a call a shape with every file that fits it: sample_rows_ranges' firsts indexed by
    set_range_first give the per-set row spans, and set_chunk_first is the running sum of the counts"""
    m = T.pkg()
    lens = list(ALL_LENGTHS)
    assert len(lens) == 51
    per = [set_shapes(m.bao.num_chunks(ln)) for ln in lens]
    seen = 0
    for name in sorted({name for sh in per for name in sh}):
        sets = [(f, sh[name]) for f, sh in enumerate(per) if name in sh]
        files = np.array([f for f, runs in sets for _ in runs], dtype=np.uint32)
        first = np.array([a for _, runs in sets for a, _ in runs], dtype=np.uint64)
        count = np.array([k for _, runs in sets for _, k in runs], dtype=np.uint64)
        lay = m.bao.set_slice_layout(lens, files, first, count)
        rrf, crf, provable = m.bao.sample_rows_ranges(lens, files, first, count)
        c_files, chunks = m.bao.runs_chunks(files, first, count)
        assert np.array_equal(lay["set_chunk_first"], np.concatenate([[0], np.cumsum([sum(k for _, k in runs) for _, runs in sets])]).astype(np.uint64))
        assert np.array_equal(crf, m.bao.sample_rows_batch(lens, c_files, chunks))     # the rows are the one-chunk planner's over the chunks in order
        at = 0
        for s, (f, runs) in enumerate(sets):
            wanted = RS.chunks_of(runs)
            lo, hi = int(lay["set_range_first"][s]), int(lay["set_range_first"][s + 1])
            assert files[lo:hi].tolist() == [f] * len(runs) and int(lay["set_chunk_first"][s]) == at
            # the set's wanted chunks ascending are the list's chunks in runs_chunks order, so its rows are one span of the ranges' rows
            assert chunks[at:at + len(wanted)].tolist() == wanted and (c_files[at:at + len(wanted)] == f).all()
            assert int(crf[at]) == int(rrf[lo]) and int(crf[at + len(wanted)]) == int(rrf[hi])
            at += len(wanted)
            seen += 1
        assert at == int(lay["set_chunk_first"][-1]) == provable.size
    assert seen > 300


def test_the_stand_alone_host_check_builds_and_passes(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    pkg = os.path.join(ROOT, "hot-proofs-blake3-circom_amd", "csrc")
    exe = str(tmp_path / "bao_set_plan_host_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", pkg, os.path.join(pkg, "b3w_bao_host.cpp"),
                    os.path.join(ROOT, "tools", "bao_set_plan_host_check.cpp"), "-o", exe], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "checks passed" in done.stdout
