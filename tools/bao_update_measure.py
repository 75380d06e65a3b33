#!/usr/bin/env python3
"""tools/bao_update_measure.py <out_dir> [--parent-lib libb3wit.so] [--quick] [--cases a,b,...] [--group-log 0] — outboards updated in
place after writes (b3w_bao_outboard_update_batch_device) against what a caller did before it: the full
b3w_bao_[group_]outboard_batch_device over the same batch.

  yardstick   the batch call of the library given with --parent-lib (a build of the commit before the update call, loaded beside this
              one; its own context) or, without it, of this library.
  method      tools/bao_groups_measure.py's: the routes alternating in one process, device events around each whole call (the host's
              sorting, table fill and upload included), medians over about a second a route.  The yardstick runs as two interleaved
              series A and B; |median A - median B| is the spread a difference has to exceed to mean anything.
  cases       1 x 1 GiB with 1, 64 and 4 096 scattered 4 KiB writes; 16 384 x 64 KiB and 262 144 x 4 KiB with 4 096 dirty files, one
              4 KiB write each; every chunk of each shape dirty (the worst case); a sweep of the number of 4 KiB writes into the 1 GiB
              file for the break-even; a file past 1 GiB beside a small one, one write each (all four launches).
  checked     before a case is timed the written blocks are changed in the arena, the update runs on the outboards of before and
              every outboard byte and root is compared with the batch call's on the arena as it is.
  gate        on 1 x 1 GiB with one 4 KiB write the update beats the yardstick by more than the yardstick's spread.
Writes <out_dir>/bao_update_measure.json.  --quick: ten update calls a case and no timing, no yardstick — for a run under `rocprofv3
--kernel-trace --stats`, whose per-kernel call counts divided by ten are the launches of one call."""
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
BLOCK = 4096                                                               # bytes of one write: four chunks
SWEEP = [1024, 16384, 65536, 131072, 196608]                               # writes into the 1 GiB file, between the cases' 1 / 64 / 4 096 and all 262 144


def parent_library(path):
    """the yardstick library and a nova_vesta context of its own -> (lib, ctx handle)"""
    vp, u32, i32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64
    P = ctypes.CDLL(path)
    P.b3w_abi_version.restype = u32
    P.b3w_create.restype, P.b3w_create.argtypes = i32, [i32, i32, ctypes.POINTER(vp)]
    P.b3w_destroy.restype, P.b3w_destroy.argtypes = None, [vp]
    P.b3w_bao_outboard_batch_device.restype, P.b3w_bao_outboard_batch_device.argtypes = i32, [vp, vp, vp, vp, u32, vp, vp, vp, u64, vp]
    P.b3w_bao_group_outboard_batch_device.restype, P.b3w_bao_group_outboard_batch_device.argtypes = i32, [vp, vp, vp, vp, u32, u32, vp, vp, vp, u64, vp]
    h = vp()
    rc = P.b3w_create(m.CIRCUIT_ID["nova_vesta"], 0, ctypes.byref(h))
    assert rc == 0, rc
    return P, h


def cases():
    """name -> (lens, files, first chunks, chunk counts): whole 4 KiB blocks, scattered by a fixed seed, no block twice"""
    rng = np.random.default_rng(17)
    sh = BM.shapes()
    per = BLOCK // 1024
    out = {}
    blocks = BM.GIB // BLOCK
    for k in [1, 64, 4096] + SWEEP:
        at = np.sort(rng.choice(blocks, k, replace=False)).astype(np.uint64)
        out[f"1x1GiB_{k}"] = (sh["1x1GiB"], np.zeros(k, dtype=np.uint32), at * per, np.full(k, per, dtype=np.uint64))
    for name in ("16384x64KiB", "262144x4KiB"):
        lens = sh[name]
        files = np.sort(rng.choice(len(lens), 4096, replace=False)).astype(np.uint32)
        first = rng.integers(0, lens[0] // BLOCK, 4096).astype(np.uint64) * per
        out[f"{name}_4096"] = (lens, files, first, np.full(4096, per, dtype=np.uint64))
    for name in ("1x1GiB", "16384x64KiB", "262144x4KiB"):
        lens = sh[name]
        out[f"{name}_all"] = (lens, np.arange(len(lens), dtype=np.uint32), np.zeros(len(lens), dtype=np.uint64),
                              np.full(len(lens), lens[0] // 1024, dtype=np.uint64))
    big = BM.GIB + (1 << 19)                                               # 1 025 tiles: the second merge launch; a small file behind it
    out["past1GiB_and_a_small_file_2"] = ([big, 8192], np.array([0, 1], dtype=np.uint32), np.array([1 << 19, 4], dtype=np.uint64),
                                          np.array([per, per], dtype=np.uint64))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--parent-lib", default="", help="libb3wit.so built from the commit before the update call: the yardstick")
    ap.add_argument("--quick", action="store_true", help="ten update calls a case (under a profiler)")
    ap.add_argument("--cases", default="", help="comma-separated subset of the case names")
    ap.add_argument("--group-log", type=int, default=0)
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    gl = a.group_log
    call = "b3w_bao_group_outboard_batch_device" if gl else "b3w_bao_outboard_batch_device"
    if a.parent_lib:
        Y, y_ctx = parent_library(a.parent_lib)
        yard = f"{call} of {os.path.basename(a.parent_lib)} (ABI {Y.b3w_abi_version() >> 16}.{Y.b3w_abi_version() & 0xffff}), loaded beside this library"
    else:
        Y, y_ctx = L, ctx.handle
        yard = f"{call} of this library"
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_arena = torch.randint(0, 256, (BM.GIB + (1 << 20),), dtype=torch.uint8, device="cuda", generator=gen)
    base = d_arena.data_ptr()
    res = dict(device=torch.cuda.get_device_name(0), arena_bytes=BM.GIB, group_log=gl, write_bytes=BLOCK, yardstick=yard, cases={})
    want = [x for x in a.cases.split(",") if x]
    for name, (lens_l, files, first, count) in cases().items():
        if want and name not in want:
            continue
        if a.quick and not want and name.split("_")[-1] not in ("1", "64", "4096", "2"):
            continue
        lens = np.array(lens_l, dtype=np.uint64)
        n_files = lens.size
        offsets = np.zeros(n_files, dtype=np.uint64)                       # back to back, every file from a 16-byte boundary
        at = 0
        for f, ln in enumerate(lens_l):
            offsets[f] = at
            at = (at + ln + 15) // 16 * 16
        assert at <= d_arena.numel()
        ob_first = m.bao.group_batch_layout(lens, gl)
        d_old = torch.empty(int(ob_first[-1]), dtype=torch.uint8, device="cuda")
        d_roots_old = torch.empty((n_files, 8), dtype=torch.int32, device="cuda")
        need_y = L.b3w_bao_batch_scratch_bytes(lens.ctypes.data, n_files)
        d_scratch_y = torch.empty(max(need_y, 16), dtype=torch.uint8, device="cuda")
        need_u = L.b3w_bao_update_scratch_bytes(lens.ctypes.data, files.ctypes.data, first.ctypes.data, count.ctypes.data, files.size)
        d_scratch_u = torch.empty(max(need_u, 16), dtype=torch.uint8, device="cuda")

        def yardstick(obs=d_old, roots=d_roots_old):
            if gl:
                rc = Y.b3w_bao_group_outboard_batch_device(y_ctx, base, offsets.ctypes.data, lens.ctypes.data, n_files, gl, obs.data_ptr(), roots.data_ptr(),
                                                           d_scratch_y.data_ptr(), need_y, s)
            else:
                rc = Y.b3w_bao_outboard_batch_device(y_ctx, base, offsets.ctypes.data, lens.ctypes.data, n_files, obs.data_ptr(), roots.data_ptr(),
                                                     d_scratch_y.data_ptr(), need_y, s)
            assert rc == 0, rc
        yardstick()                                                        # the outboards of before
        d_new, d_roots_new = d_old.clone(), d_roots_old.clone()

        def update():
            rc = L.b3w_bao_outboard_update_batch_device(ctx.handle, base, d_arena.numel(), offsets.ctypes.data, lens.ctypes.data, n_files, gl,
                                                        ob_first.ctypes.data, d_new.data_ptr(), d_roots_new.data_ptr(), files.ctypes.data,
                                                        first.ctypes.data, count.ctypes.data, files.size, d_scratch_u.data_ptr(), need_u, s)
            assert rc == 0, ctx.last_error()
        # the writes: a byte changes in every dirty chunk (in the first 4 096 chunks of a range that is longer)
        chunks = int(count.sum())
        starts = torch.from_numpy((offsets[files] + first * np.uint64(1024)).astype(np.int64)).cuda()
        per = int(count[0])
        idx = (starts[:, None] + torch.arange(min(per, 4096), device="cuda", dtype=torch.int64)[None, :] * 1024).reshape(-1)
        idx = idx[idx < d_arena.numel()]
        d_arena[idx] = d_arena[idx] ^ 1
        update()
        d_want, d_roots_want = torch.empty_like(d_old), torch.empty_like(d_roots_old)
        yardstick(d_want, d_roots_want)
        torch.cuda.synchronize()
        assert not torch.equal(d_roots_want, d_roots_old), f"{name}: the writes changed no root"
        assert torch.equal(d_new, d_want) and torch.equal(d_roots_new, d_roots_want), f"{name}: the update differs from the batch call"
        row = dict(n_files=int(n_files), bytes=int(lens.sum()), ranges=int(files.size), dirty_chunks=chunks,
                   dirty_fraction=chunks / float(sum(m.bao.num_chunks(int(x)) for x in lens_l)), update_scratch_bytes=int(need_u), bytes_equal=True)
        if a.quick:
            for _ in range(QUICK_CALLS):
                update()
            torch.cuda.synchronize()
            row["update_calls"] = QUICK_CALLS
            res["cases"][name] = row
            continue
        for _ in range(3):
            yardstick()
            update()
        t = alternating({"yard_a": yardstick, "update": update, "yard_b": yardstick})
        row.update(yardstick=stats(t["yard_a"] + t["yard_b"]), yardstick_a=stats(t["yard_a"]), yardstick_b=stats(t["yard_b"]), update=stats(t["update"]))
        row["yardstick_spread_ms"] = abs(row["yardstick_a"]["ms"] - row["yardstick_b"]["ms"])
        row["yardstick_minus_update_ms"] = row["yardstick"]["ms"] - row["update"]["ms"]
        row["update_over_yardstick"] = row["update"]["ms"] / row["yardstick"]["ms"]
        row["update_wins_by_more_than_the_spread"] = row["yardstick_minus_update_ms"] > row["yardstick_spread_ms"]
        res["cases"][name] = row
        print(name, json.dumps(row), flush=True)
        del d_old, d_new, d_want
    if not a.quick:
        one = res["cases"].get("1x1GiB_1")
        if one:
            res["gate"] = dict(case="1x1GiB_1", passed=bool(one["update_wins_by_more_than_the_spread"]), yardstick_ms=one["yardstick"]["ms"],
                               update_ms=one["update"]["ms"], spread_ms=one["yardstick_spread_ms"])
        sweep = sorted((r["dirty_fraction"], r["update_wins_by_more_than_the_spread"], n) for n, r in res["cases"].items() if n.startswith("1x1GiB_"))
        if sweep:
            winning = [f for f, w, _ in sweep if w]
            losing = [f for f, w, _ in sweep if not w]
            res["break_even_1x1GiB"] = dict(largest_dirty_fraction_that_wins=max(winning) if winning else None,
                                            smallest_dirty_fraction_that_does_not=min(losing) if losing else None)
    if a.parent_lib:
        Y.b3w_destroy(y_ctx)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_update_measure.json" if not a.quick else "bao_update_measure_quick.json"), "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
