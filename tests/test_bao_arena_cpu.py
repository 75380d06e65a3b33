"""The arena calls without a GPU: the library exports b3w_sample_plan_arena_device and b3w_bao_slice_arena_device, the header
declares them, the Python layer knows their signatures, and the ABI number has not moved (new names only)."""
import os
import re

import b3w_testlib as T

NAMES = ("b3w_sample_plan_arena_device", "b3w_bao_slice_arena_device")


def test_the_library_exports_both_calls_and_the_abi_is_still_1_4():
    m = T.pkg()
    L = m.lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in m.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert L.b3w_abi_version() == (1 << 16) | 4
    for name in ("plan_samples_arena", "prove_samples_arena", "slices_arena"):
        assert callable(getattr(m.bao, name)), name


def test_the_prototypes_are_in_the_header():
    hdr = open(os.path.join(T.ROOT, "include", "b3wit.h")).read()
    plan = re.search(r"int32_t\s+b3w_sample_plan_arena_device\s*\(([^;]*)\)\s*;", hdr)
    slices = re.search(r"int32_t\s+b3w_bao_slice_arena_device\s*\(([^;]*)\)\s*;", hdr)
    assert plan and slices
    args = [" ".join(a.split()) for a in plan.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "d_arena", "arena_bytes", "host_offsets", "host_lens", "n_files", "group_log", "d_outboards",
                                                         "d_roots", "host_files", "host_chunks", "n_samples", "d_records", "d_sample_status", "stream"]
    args = [" ".join(a.split()) for a in slices.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "d_arena", "arena_bytes", "host_offsets", "host_lens", "n_files", "group_log", "d_outboards",
                                                         "host_files", "host_chunks", "n_samples", "d_slices", "stream"]
    # the ctypes signatures have one entry per parameter
    L = T.pkg().lib()
    assert len(L.b3w_sample_plan_arena_device.argtypes) == 15 and len(L.b3w_bao_slice_arena_device.argtypes) == 13


def test_null_contexts_are_refused_on_the_host():
    L = T.pkg().lib()
    assert L.b3w_sample_plan_arena_device(None, None, 0, None, None, 0, 0, None, None, None, None, 0, None, None, None) == 100
    assert L.b3w_bao_slice_arena_device(None, None, 0, None, None, 0, 0, None, None, None, 0, None, None) == 100
