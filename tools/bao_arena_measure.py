#!/usr/bin/env python3
"""tools/bao_arena_measure.py <out_dir> [--parent-lib libb3wit.so] [--quick] [--shapes a,b] — the arena calls
(b3w_sample_plan_arena_device / b3w_bao_slice_arena_device) against the gathered route they replace.

  shapes      4 096 samples over 16 384 x 64 KiB and over 1 x 1 GiB, group_log 0, 4 and 6; two passes: every file from a 16-byte
              boundary ("aligned"), then every file from an odd byte ("odd": offset mod 16 = 1, 3, ... 15 in turn).
  yardstick   the library given with --parent-lib (a build of the commit before the arena calls, loaded beside this one, a context of
              its own) or, without it, this library:
                (a) its plan / slice call on bytes ALREADY gathered: b3w_sample_plan_batch_device (group_log 0) /
                    b3w_sample_plan_group_batch_device, and b3w_bao_slice_batch_device
                (b) the gather on the device (bao.chunk_bytes_batch / group_bytes_batch: torch index gathers) plus that call
  method      alternating in one process, device events around each whole call (the host's table fill and upload included), medians
              over about a second a route; (a) and (b) are each measured as two interleaved series A and B, and |median A - median B|
              is the spread a difference has to exceed to mean anything.  Records, statuses and slices of the routes are compared
              once before timing.
Writes <out_dir>/bao_arena_measure.json.  --quick: ten calls a route and shape, no timing, the first shape's aligned pass only — for a
run under `rocprofv3 --kernel-trace --stats`, whose per-kernel call counts divided by ten are the launches of one call and whose
per-kernel times are the kernels alone."""
import argparse, ctypes, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bao_batch_measure as BM
from bao_groups_measure import alternating, stats

m = __import__("hot-proofs-blake3-circom_amd")

QUICK_CALLS = 10
SAMPLES = 4096
GS = (0, 4, 6)


def parent_library(path):
    """the yardstick library and a nova_vesta context of its own -> (lib, ctx handle)"""
    vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32
    P = ctypes.CDLL(path)
    P.b3w_abi_version.restype = u32
    P.b3w_create.restype, P.b3w_create.argtypes = i32, [i32, i32, ctypes.POINTER(vp)]
    P.b3w_destroy.restype, P.b3w_destroy.argtypes = None, [vp]
    P.b3w_sample_plan_batch_device.restype, P.b3w_sample_plan_batch_device.argtypes = i32, [vp, vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp]
    P.b3w_sample_plan_group_batch_device.restype, P.b3w_sample_plan_group_batch_device.argtypes = i32, [vp, vp, u32, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp]
    P.b3w_bao_slice_batch_device.restype, P.b3w_bao_slice_batch_device.argtypes = i32, [vp, vp, u32, u32, vp, vp, vp, u32, vp, vp, vp]
    h = vp()
    rc = P.b3w_create(m.CIRCUIT_ID["nova_vesta"], 0, ctypes.byref(h))
    assert rc == 0, rc
    return P, h


def place(lens, odd):
    """back to back, every file from a 16-byte boundary, or (odd) from 1, 3, ... 15 bytes behind one in turn"""
    offsets, at = np.zeros(len(lens), dtype=np.uint64), 0
    for f, ln in enumerate(lens):
        at = (at + 15) // 16 * 16 + ((2 * (f % 8) + 1) if odd else 0)
        offsets[f] = at
        at += ln
    return offsets, at


def compare(row, ya, yb, arena):
    """the claim's figures from the three routes' stats"""
    row["a_spread_ms"], row["b_spread_ms"] = abs(ya[0]["ms"] - ya[1]["ms"]), abs(yb[0]["ms"] - yb[1]["ms"])
    row["arena_over_a"] = arena["ms"] / row["a"]["ms"]
    row["arena_over_b"] = arena["ms"] / row["b"]["ms"]
    row["b_minus_arena_ms"] = row["b"]["ms"] - arena["ms"]
    row["arena_minus_a_ms"] = arena["ms"] - row["a"]["ms"]
    row["beats_b_by_more_than_its_spread"] = bool(row["b_minus_arena_ms"] > row["b_spread_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--parent-lib", default="", help="libb3wit.so built from the commit before the arena calls: the yardstick")
    ap.add_argument("--quick", action="store_true", help="ten calls a route, the first shape's aligned pass (under a profiler)")
    ap.add_argument("--shapes", default="", help="comma-separated subset of 16384x64KiB,1x1GiB")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    if a.parent_lib:
        Y, y_ctx = parent_library(a.parent_lib)
        yard = f"{os.path.basename(a.parent_lib)} (ABI {Y.b3w_abi_version() >> 16}.{Y.b3w_abi_version() & 0xffff})"
    else:
        Y, y_ctx = L, ctx.handle
        yard = "this library"
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_arena = torch.randint(0, 256, (BM.GIB + (1 << 20),), dtype=torch.uint8, device="cuda", generator=gen)
    res = dict(device=torch.cuda.get_device_name(0), samples=SAMPLES, yardstick=yard, quick=a.quick, rows={})
    want = [x for x in a.shapes.split(",") if x]
    shapes = {k: v for k, v in BM.shapes().items() if k in ("16384x64KiB", "1x1GiB") and (not want or k in want)}
    rng = np.random.default_rng(7)
    for name, lens_l in shapes.items():
        lens = np.array(lens_l, dtype=np.uint64)
        files = rng.integers(0, lens.size, SAMPLES).astype(np.uint32)
        chunks = np.array([rng.integers(0, m.bao.num_chunks(int(lens[f]))) for f in files], dtype=np.uint64)
        rf = m.bao.sample_rows_batch(lens, files, chunks)
        sf = m.bao.slice_layout(lens, files, chunks)
        d_recs_y = torch.empty((int(rf[-1]), 32), dtype=torch.int32, device="cuda")
        d_recs_n = torch.empty_like(d_recs_y)
        d_st_y = torch.full((SAMPLES,), -1, dtype=torch.int32, device="cuda")
        d_st_n = torch.full((SAMPLES,), -1, dtype=torch.int32, device="cuda")
        d_sl_y = torch.zeros(int(sf[-1]), dtype=torch.uint8, device="cuda")
        d_sl_n = torch.zeros_like(d_sl_y)
        for odd in (False, True):
            offsets, end = place(lens_l, odd)
            assert end <= d_arena.numel()
            for g in GS:
                obs = m.bao.outboard_groups_batch(ctx, d_arena, offsets, lens, g)
                d_obs, d_roots = obs["outboards"], obs["roots"]

                def gather():
                    return m.bao.chunk_bytes_batch(d_arena, offsets, lens, files, chunks) if g == 0 else m.bao.group_bytes_batch(d_arena, offsets, lens, files, chunks, g)

                def y_plan(d_bytes):
                    if g == 0:
                        rc = Y.b3w_sample_plan_batch_device(y_ctx, lens.ctypes.data, lens.size, d_obs.data_ptr(), d_roots.data_ptr(), files.ctypes.data,
                                                            chunks.ctypes.data, SAMPLES, d_bytes.data_ptr(), d_recs_y.data_ptr(), d_st_y.data_ptr(), s)
                    else:
                        rc = Y.b3w_sample_plan_group_batch_device(y_ctx, lens.ctypes.data, lens.size, g, d_obs.data_ptr(), d_roots.data_ptr(), files.ctypes.data,
                                                                  chunks.ctypes.data, SAMPLES, d_bytes.data_ptr(), d_recs_y.data_ptr(), d_st_y.data_ptr(), s)
                    assert rc == 0, rc

                def y_slice(d_bytes):
                    rc = Y.b3w_bao_slice_batch_device(y_ctx, lens.ctypes.data, lens.size, g, d_obs.data_ptr(), files.ctypes.data, chunks.ctypes.data, SAMPLES,
                                                      d_bytes.data_ptr(), d_sl_y.data_ptr(), s)
                    assert rc == 0, rc
                gathered = gather()

                def plan_a():
                    y_plan(gathered)

                def plan_b():
                    y_plan(gather())

                def plan_arena():
                    rc = L.b3w_sample_plan_arena_device(ctx.handle, d_arena.data_ptr(), d_arena.numel(), offsets.ctypes.data, lens.ctypes.data, lens.size, g,
                                                        d_obs.data_ptr(), d_roots.data_ptr(), files.ctypes.data, chunks.ctypes.data, SAMPLES, d_recs_n.data_ptr(),
                                                        d_st_n.data_ptr(), s)
                    assert rc == 0, ctx.last_error()

                def slice_a():
                    y_slice(gathered)

                def slice_b():
                    y_slice(gather())

                def slice_arena():
                    rc = L.b3w_bao_slice_arena_device(ctx.handle, d_arena.data_ptr(), d_arena.numel(), offsets.ctypes.data, lens.ctypes.data, lens.size, g,
                                                      d_obs.data_ptr(), files.ctypes.data, chunks.ctypes.data, SAMPLES, d_sl_n.data_ptr(), s)
                    assert rc == 0, ctx.last_error()
                for fn in (plan_a, plan_arena, slice_a, slice_arena):
                    fn()
                torch.cuda.synchronize()
                assert bool((d_st_y == 0).all().item()) and torch.equal(d_st_y, d_st_n) and torch.equal(d_recs_y, d_recs_n), f"{name} g = {g}: the plans differ"
                assert torch.equal(d_sl_y, d_sl_n), f"{name} g = {g}: the slices differ"
                key = f"{name}_{'odd' if odd else 'aligned'}_g{g}"
                row = dict(shape=name, starts="odd" if odd else "aligned", group_log=g, rows=int(rf[-1]), slice_bytes=int(sf[-1]),
                           gathered_bytes=int(gathered.numel()), gather_index_bytes=int(gathered.numel()) * 8, results_equal=True)
                if a.quick:
                    for fn in (plan_a, plan_arena, slice_a, slice_arena):
                        for _ in range(QUICK_CALLS):
                            fn()
                        torch.cuda.synchronize()
                    row["calls_each"] = QUICK_CALLS
                    res["rows"][key] = row
                    continue
                for what, fa, fb, fn in (("plan", plan_a, plan_b, plan_arena), ("slice", slice_a, slice_b, slice_arena)):
                    for fn_ in (fa, fb, fn):
                        fn_()
                    t = alternating({"a1": fa, "b1": fb, "arena": fn, "a2": fa, "b2": fb})
                    r = dict(a=stats(t["a1"] + t["a2"]), b=stats(t["b1"] + t["b2"]), arena=stats(t["arena"]))
                    compare(r, (stats(t["a1"]), stats(t["a2"])), (stats(t["b1"]), stats(t["b2"])), r["arena"])
                    row[what] = r
                res["rows"][key] = row
                print(key, json.dumps(row), flush=True)
                del obs, gathered
            if a.quick:
                break
        if a.quick:
            break
    if a.parent_lib:
        Y.b3w_destroy(y_ctx)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_arena_measure_quick.json" if a.quick else "bao_arena_measure.json"), "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
