#!/usr/bin/env python3
"""tools/bao_groups_measure.py <out_dir> [--parent-lib libb3wit.so] [--quick] [--shapes a,b,...] [--group-log 4] — group outboards
and the group planner against the calls for full outboards.

  emission    for each shape of tools/bao_batch_measure.py (1 GiB in all) b3w_bao_group_outboard_batch_device at --group-log
              against the yardstick, b3w_bao_outboard_batch_device: of the library given with --parent-lib (a build of the commit
              before group outboards, loaded beside this one; its own context) or, without it, of this library.  Alternating in
              the same process, device events around each whole call (the host's table fill and upload included), medians over
              about a second a route.  The yardstick is measured as two interleaved series A and B; |median A - median B| is the
              spread a difference has to exceed to mean anything.  Roots of both calls compared once before timing.
  planning    4 096 samples over the 16 384 x 64 KiB batch and over the 1 x 1 GiB file, group_log 4 and 6: plan_samples_groups_batch's
              C call on group outboards and group bytes against the yardstick's b3w_sample_plan_batch_device on full outboards
              and chunk bytes, device events around each call, alternating; the bytes are gathered before timing.
Writes <out_dir>/bao_groups_measure.json.  --quick: ten calls a route and shape, no timing — for a run under `rocprofv3
--kernel-trace --stats`, whose per-kernel call counts divided by ten are the launches of one call."""
import argparse, ctypes, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bao_batch_measure as BM

m = __import__("hot-proofs-blake3-circom_amd")

QUICK_CALLS = 10
SAMPLES = 4096


def parent_library(path):
    """the yardstick library and a nova_vesta context of its own -> (lib, ctx handle)"""
    vp, u32, i32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64
    P = ctypes.CDLL(path)
    P.b3w_abi_version.restype = u32
    P.b3w_create.restype, P.b3w_create.argtypes = i32, [i32, i32, ctypes.POINTER(vp)]
    P.b3w_destroy.restype, P.b3w_destroy.argtypes = None, [vp]
    P.b3w_bao_outboard_batch_device.restype, P.b3w_bao_outboard_batch_device.argtypes = i32, [vp, vp, vp, vp, u32, vp, vp, vp, u64, vp]
    P.b3w_sample_plan_batch_device.restype, P.b3w_sample_plan_batch_device.argtypes = i32, [vp, vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp]
    h = vp()
    rc = P.b3w_create(m.CIRCUIT_ID["nova_vesta"], 0, ctypes.byref(h))
    assert rc == 0, rc
    return P, h


def alternating(routes, window_s=1.0, rounds=3):
    """{name: fn} -> {name: [ms, ...]}: the routes one after the other, `rounds` times, each turn about window_s / rounds long"""
    out = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            out[k] += BM.timed(fn, window_s / rounds)
    return out


def stats(ts):
    return dict(ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)), reps=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--parent-lib", default="", help="libb3wit.so built from the commit before group outboards: the yardstick")
    ap.add_argument("--quick", action="store_true", help="ten calls a route and shape (under a profiler)")
    ap.add_argument("--shapes", default="", help="comma-separated subset of the shape names")
    ap.add_argument("--group-log", type=int, default=4)
    ap.add_argument("--no-planning", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    if a.parent_lib:
        Y, y_ctx = parent_library(a.parent_lib)
        yard = f"b3w_bao_outboard_batch_device of {os.path.basename(a.parent_lib)} (ABI {Y.b3w_abi_version() >> 16}.{Y.b3w_abi_version() & 0xffff})"
    else:
        Y, y_ctx = L, ctx.handle
        yard = "b3w_bao_outboard_batch_device of this library"
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_arena = torch.randint(0, 256, (BM.GIB + (1 << 20),), dtype=torch.uint8, device="cuda", generator=gen)
    gl = a.group_log
    res = dict(device=torch.cuda.get_device_name(0), arena_bytes=BM.GIB, group_log=gl, yardstick=yard, shapes={}, planning={})
    want = [x for x in a.shapes.split(",") if x]
    kept = {}
    for name, lens_l in BM.shapes().items():
        if want and name not in want:
            continue
        lens = np.array(lens_l, dtype=np.uint64)
        n_files = lens.size
        offsets = np.zeros(n_files, dtype=np.uint64)                             # back to back, every file from a 16-byte boundary
        at = 0
        for f, ln in enumerate(lens_l):
            offsets[f] = at
            at = (at + ln + 15) // 16 * 16
        assert at <= d_arena.numel()
        full_first, grp_first = m.bao.batch_layout(lens), m.bao.group_batch_layout(lens, gl)
        d_full = torch.empty(int(full_first[-1]), dtype=torch.uint8, device="cuda")
        d_grp = torch.empty(int(grp_first[-1]), dtype=torch.uint8, device="cuda")
        d_roots_y = torch.empty((n_files, 8), dtype=torch.int32, device="cuda")
        d_roots_g = torch.empty((n_files, 8), dtype=torch.int32, device="cuda")
        need = L.b3w_bao_batch_scratch_bytes(lens.ctypes.data, n_files)
        d_scratch = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        base = d_arena.data_ptr()

        def yardstick():
            rc = Y.b3w_bao_outboard_batch_device(y_ctx, base, offsets.ctypes.data, lens.ctypes.data, n_files, d_full.data_ptr(), d_roots_y.data_ptr(),
                                                 d_scratch.data_ptr(), need, s)
            assert rc == 0, rc

        def groups():
            rc = L.b3w_bao_group_outboard_batch_device(ctx.handle, base, offsets.ctypes.data, lens.ctypes.data, n_files, gl, d_grp.data_ptr(),
                                                       d_roots_g.data_ptr(), d_scratch.data_ptr(), need, s)
            assert rc == 0, ctx.last_error()
        row = dict(n_files=int(n_files), bytes=int(lens.sum()), full_outboard_bytes=int(full_first[-1]), group_outboard_bytes=int(grp_first[-1]),
                   bound_ms=BM.bound_ms(lens_l))
        if a.quick:
            for _ in range(QUICK_CALLS):
                yardstick()
            torch.cuda.synchronize()
            for _ in range(QUICK_CALLS):
                groups()
            torch.cuda.synchronize()
            row["calls_each"] = QUICK_CALLS
            res["shapes"][name] = row
            if name in ("16384x64KiB", "1x1GiB"):
                kept[name] = dict(lens=lens, offsets=offsets, full=d_full.clone(), roots=d_roots_y.clone())
            continue
        yardstick()
        groups()
        torch.cuda.synchronize()
        assert torch.equal(d_roots_y, d_roots_g), f"{name}: the roots of the two calls differ"
        for _ in range(3):
            yardstick()
            groups()
        t = alternating({"yard_a": yardstick, "groups": groups, "yard_b": yardstick})
        row.update(yardstick=stats(t["yard_a"] + t["yard_b"]), yardstick_a=stats(t["yard_a"]), yardstick_b=stats(t["yard_b"]), groups=stats(t["groups"]))
        row["yardstick_spread_ms"] = abs(row["yardstick_a"]["ms"] - row["yardstick_b"]["ms"])
        row["groups_minus_yardstick_ms"] = row["groups"]["ms"] - row["yardstick"]["ms"]
        row["groups_over_yardstick"] = row["groups"]["ms"] / row["yardstick"]["ms"]
        res["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
        if name in ("16384x64KiB", "1x1GiB"):
            kept[name] = dict(lens=lens, offsets=offsets, full=d_full.clone(), roots=d_roots_y.clone())
    if not a.no_planning:
        rng = np.random.default_rng(7)
        for name, k in kept.items():
            lens, offsets = k["lens"], k["offsets"]
            files = rng.integers(0, lens.size, SAMPLES).astype(np.uint32)
            chunks = np.array([rng.integers(0, m.bao.num_chunks(int(lens[f]))) for f in files], dtype=np.uint64)
            rf = m.bao.sample_rows_batch(lens, files, chunks)
            d_recs_y = torch.empty((int(rf[-1]), 32), dtype=torch.int32, device="cuda")
            d_recs_g = torch.empty_like(d_recs_y)
            d_st = torch.full((SAMPLES,), -1, dtype=torch.int32, device="cuda")
            cb = m.bao.chunk_bytes_batch(d_arena, offsets, lens, files, chunks)

            def plan_full():
                rc = Y.b3w_sample_plan_batch_device(y_ctx, lens.ctypes.data, lens.size, k["full"].data_ptr(), k["roots"].data_ptr(), files.ctypes.data,
                                                    chunks.ctypes.data, SAMPLES, cb.data_ptr(), d_recs_y.data_ptr(), d_st.data_ptr(), s)
                assert rc == 0, rc
            for g in (4, 6):
                grp = m.bao.outboard_groups_batch(ctx, d_arena, offsets, lens, g)
                gb = m.bao.group_bytes_batch(d_arena, offsets, lens, files, chunks, g)

                def plan_groups():
                    rc = L.b3w_sample_plan_group_batch_device(ctx.handle, lens.ctypes.data, lens.size, g, grp["outboards"].data_ptr(), grp["roots"].data_ptr(),
                                                              files.ctypes.data, chunks.ctypes.data, SAMPLES, gb.data_ptr(), d_recs_g.data_ptr(),
                                                              d_st.data_ptr(), s)
                    assert rc == 0, ctx.last_error()
                plan_full()
                plan_groups()
                torch.cuda.synchronize()
                assert bool((d_st == 0).all().item()) and torch.equal(d_recs_y, d_recs_g), f"{name} g = {g}: the records of the two planners differ"
                row = dict(samples=SAMPLES, rows=int(rf[-1]), group_log=g, group_bytes=int(gb.numel()), chunk_bytes=int(cb.numel()),
                           group_outboard_bytes=int(grp["outboards"].numel()), full_outboard_bytes=int(k["full"].numel()), records_equal=True)
                if a.quick:
                    for _ in range(QUICK_CALLS):
                        plan_full()
                    torch.cuda.synchronize()
                    for _ in range(QUICK_CALLS):
                        plan_groups()
                    torch.cuda.synchronize()
                    row["calls_each"] = QUICK_CALLS
                else:
                    t = alternating({"full_a": plan_full, "groups": plan_groups, "full_b": plan_full})
                    row.update(full=stats(t["full_a"] + t["full_b"]), full_a=stats(t["full_a"]), full_b=stats(t["full_b"]), groups=stats(t["groups"]))
                    row["groups_over_full"] = row["groups"]["ms"] / row["full"]["ms"]
                res["planning"][f"{name}_g{g}"] = row
                print("planning", name, g, json.dumps(row), flush=True)
                del grp, gb
    if a.parent_lib:
        Y.b3w_destroy(y_ctx)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_groups_measure.json" if not a.quick else "bao_groups_measure_quick.json"), "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
