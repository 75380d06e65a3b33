#!/usr/bin/env python3
"""tools/bao_set_stream_measure.py <out_dir> [--parent-lib libb3wit.so] — a set slice taken in window by window
(b3w_bao_set_slice_stream_begin / _push / _finish) against the one-shot receiver over the whole slice.

  shape       one 1 GiB file with half its chunks missing: the runs of tools/bao_range_measure.py's bitmap, one set slice of 593 MB.
  yardstick   b3w_bao_set_slice_ingest_device of the library given with --parent-lib (a build of the parent commit, loaded beside this
              one, a context of its own) or, without it, of this library; as two interleaved series A and B, whose medians' difference
              is the spread a difference has to exceed.  This library's own one-shot call runs beside it.
  streamed    a whole session a pass - begin, every push, finish, free - over windows cut by b3w_bao_set_slice_stream_cuts at the least
              window (about 1.1 MiB), 8 MiB and 64 MiB.  The windows are read where the resident slice lies (their alignment is the
              one-shot layout's): what is timed is the receiver, not the arrival.
  method      tools/bao_set_measure.py's: the routes alternating in one process, device events around whole calls (the host's table
              work and uploads included), medians over about a second a route.  BEFORE TIMING every route runs into buffers of 0xEE
              and the arena, outboard, bitmap and statuses are compared with the yardstick's byte for byte.  No profiler is run.
  written     the sum of the pushes against the one-shot time and the yardstick's spread; fixed_ms_a_push = (session - one-shot) /
              pushes, what a session takes beyond the one-shot call spread over its pushes (begin's host work is in it); the device bytes a receiver holds (two windows against the slice); the time from begin to the verdict on a
              tampered first window (begin and one push, set_status read) against the one-shot call on the same slice.
Writes <out_dir>/bao_set_stream_measure.json."""
import argparse, ctypes, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bao_batch_measure as BM
from bao_groups_measure import alternating, stats
from bao_range_measure import runs_half_missing
from bao_receive_packed_measure import SET

m = __import__("hot-proofs-blake3-circom_amd")

FILL = 0xEE
MIN = m.bao.SET_SLICE_STREAM_MIN_WINDOW
WINDOWS = {"least": MIN, "8MiB": 8 << 20, "64MiB": 64 << 20}


def parent_library(path):
    vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32
    P = ctypes.CDLL(path)
    P.b3w_abi_version.restype = u32
    P.b3w_create.restype, P.b3w_create.argtypes = i32, [i32, i32, ctypes.POINTER(vp)]
    P.b3w_destroy.restype, P.b3w_destroy.argtypes = None, [vp]
    P.b3w_bao_set_slice_ingest_device.restype, P.b3w_bao_set_slice_ingest_device.argtypes = i32, SET
    h = vp()
    rc = P.b3w_create(m.CIRCUIT_ID["nova_vesta"], 0, ctypes.byref(h))
    assert rc == 0, rc
    return P, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--parent-lib", default="", help="libb3wit.so built from the parent commit: the yardstick")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    if a.parent_lib:
        Y, y_ctx = parent_library(a.parent_lib)
        yard = f"{os.path.basename(a.parent_lib)} (ABI {Y.b3w_abi_version() >> 16}.{Y.b3w_abi_version() & 0xffff}), a build of the parent commit loaded beside this library"
    else:
        Y, y_ctx = L, ctx.handle
        yard = "this library's one-shot receiver"
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_src = torch.empty(BM.GIB + 16, dtype=torch.uint8, device="cuda")
    d_src[:] = torch.randint(0, 256, (BM.GIB + 16,), dtype=torch.uint8, device="cuda", generator=gen)
    lens, offs = np.array([BM.GIB], dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    prov = m.bao.outboard_batch(ctx, d_src, offs, lens)
    d_roots = prov["roots"]
    first, count = runs_half_missing(np.random.default_rng(20))
    k = int(first.size)
    files = np.zeros(k, dtype=np.uint32)
    n_chunks = int(count.sum())
    d_slices = m.bao.set_slices_arena(ctx, d_src, offs, lens, prov["outboards"], files, first, count)["slices"]
    size = m.bao.set_slice_size(BM.GIB, first, count)
    routes = ("yard", "one", "stream")
    arena = {r: torch.empty(BM.GIB + 16, dtype=torch.uint8, device="cuda") for r in routes}
    obs = {r: torch.empty(m.bao.group_outboard_size(BM.GIB, 0), dtype=torch.uint8, device="cuda") for r in routes}
    have = {r: m.bao.have_new(lens) for r in routes}
    st = {r: torch.empty(1, dtype=torch.int32, device="cuda") for r in routes}
    fb = {r: torch.empty(1, dtype=torch.int64, device="cuda") for r in routes}
    cs = {r: torch.empty(n_chunks, dtype=torch.int32, device="cuda") for r in routes}
    need = L.b3w_bao_set_slice_ingest_scratch_bytes(lens.ctypes.data, 1, files.ctypes.data, first.ctypes.data, count.ctypes.data, k)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    res = dict(device=torch.cuda.get_device_name(0), file_bytes=BM.GIB, runs=k, chunks=n_chunks, slice_bytes=int(size), rows=need // 16, yardstick=yard,
               profiler="none was run", windows={})

    def one_shot(lib, handle, r, slices=None):
        sl = d_slices if slices is None else slices
        assert lib.b3w_bao_set_slice_ingest_device(handle, arena[r].data_ptr(), arena[r].numel(), offs.ctypes.data, lens.ctypes.data, 1, 0, obs[r].data_ptr(),
                                                   d_roots.data_ptr(), files.ctypes.data, first.ctypes.data, count.ctypes.data, k, sl.data_ptr(), st[r].data_ptr(),
                                                   fb[r].data_ptr(), cs[r].data_ptr(), have[r].data_ptr(), scratch.data_ptr(), scratch.numel(), s) == 0

    def session(cuts, s_scratch, slices=None, pushes=None):
        """begin, the first `pushes` windows (all of them: None, with finish), free"""
        sl = d_slices if slices is None else slices
        h = ctypes.c_void_p()
        r = "stream"
        assert L.b3w_bao_set_slice_stream_begin(ctx.handle, BM.GIB, 0, first.ctypes.data, count.ctypes.data, k, d_roots.data_ptr(), 0, arena[r].data_ptr(), BM.GIB,
                                                obs[r].data_ptr(), have[r].data_ptr(), cs[r].data_ptr(), st[r].data_ptr(), fb[r].data_ptr(), s_scratch.data_ptr(),
                                                s_scratch.numel(), s, ctypes.byref(h)) == 0, ctx.last_error()
        base = sl.data_ptr() + 8
        for lo, hi in list(zip(cuts, cuts[1:]))[:pushes]:
            assert L.b3w_bao_set_slice_stream_push(h, lo, base + lo, hi - lo, s) == 0, ctx.last_error()
        if pushes is None:
            assert L.b3w_bao_set_slice_stream_finish(h) == 0, ctx.last_error()
        L.b3w_bao_set_slice_stream_free(h)

    def fresh(r):
        arena[r].fill_(FILL); obs[r].fill_(FILL); have[r].zero_(); st[r].fill_(-1); fb[r].fill_(-2); cs[r].fill_(-1)

    fresh("yard")
    one_shot(Y, y_ctx, "yard")
    fresh("one")
    one_shot(L, ctx.handle, "one")
    torch.cuda.synchronize()
    assert st["yard"].tolist() == [0] and not cs["yard"].any().item()
    for x in (arena, obs, have, st, fb, cs):
        assert torch.equal(x["yard"], x["one"])
    bad = d_slices.clone()
    bad[8 + 3] ^= 1                                                       # the header, in the first window
    for name, wb in WINDOWS.items():
        cuts = [int(c) for c in m.bao.set_slice_cuts(BM.GIB, first, count, wb)]
        s_scratch = torch.empty(L.b3w_bao_set_slice_stream_scratch_bytes(BM.GIB, first.ctypes.data, count.ctypes.data, k, wb), dtype=torch.uint8, device="cuda")
        fresh("stream")
        session(cuts, s_scratch)
        torch.cuda.synchronize()
        for x in (arena, obs, have, st, fb, cs):
            assert torch.equal(x["yard"], x["stream"]), name
        for _ in range(3):
            one_shot(Y, y_ctx, "yard"); one_shot(L, ctx.handle, "one"); session(cuts, s_scratch)
        t = alternating({"yard_a": lambda: one_shot(Y, y_ctx, "yard"), "stream": lambda: session(cuts, s_scratch), "one": lambda: one_shot(L, ctx.handle, "one"),
                         "yard_b": lambda: one_shot(Y, y_ctx, "yard")})
        row = dict(window_bytes=wb, pushes=len(cuts) - 1, largest_window=max(hi - lo for lo, hi in zip(cuts, cuts[1:])), checked=True)
        row["stream"], row["yardstick"], row["one_shot_this_library"] = stats(t["stream"]), stats(t["yard_a"] + t["yard_b"]), stats(t["one"])
        row["yardstick_spread_ms"] = abs(stats(t["yard_a"])["ms"] - stats(t["yard_b"])["ms"])
        row["stream_over_yardstick"] = row["stream"]["ms"] / row["yardstick"]["ms"]
        row["fixed_ms_a_push"] = (row["stream"]["ms"] - row["yardstick"]["ms"]) / row["pushes"]
        row["receiver_window_bytes"] = 2 * row["largest_window"]
        row["receiver_bytes_saved"] = int(size) - row["receiver_window_bytes"]
        # the verdict on a tampered first window: begin and one push, against the one-shot call over the same slice
        session(cuts, s_scratch, bad, pushes=1)
        torch.cuda.synchronize()
        assert st["stream"].tolist() == [3] and fb["stream"].tolist() == [int(first[0])], name
        one_shot(Y, y_ctx, "yard", bad)
        torch.cuda.synchronize()
        assert st["yard"].tolist() == [3]
        v = alternating({"first_window": lambda: session(cuts, s_scratch, bad, pushes=1), "one_shot": lambda: one_shot(Y, y_ctx, "yard", bad)}, window_s=0.5)
        row["verdict_first_window"], row["verdict_one_shot"] = stats(v["first_window"]), stats(v["one_shot"])
        fresh("yard")
        one_shot(Y, y_ctx, "yard")                                         # (the yardstick's outputs clean again for the next window size)
        res["windows"][name] = row
        print(name, json.dumps(row), flush=True)
    res["not_taken"] = ("the arrival of the bytes (the windows are read where the resident slice lies: the verdict times leave out the transfer the one-shot call "
                        "must wait for in full); the packed destination; files past 1 GiB; per-kernel times (no profiler was run)")
    if a.parent_lib:
        Y.b3w_destroy(y_ctx)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_set_stream_measure.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
