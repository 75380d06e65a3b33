#!/usr/bin/env python3
"""tools/bao_verify_measure.py <out_dir> --parent-lib libb3wit.so [--quick] [--shapes a,b,...] [--group-logs 0,4] — whole-file
verification (b3w_bao_verify_batch_device) against the routes that existed before it.  Needs a GPU; there is no fall-back.

For each shape of tools/bao_batch_measure.py (1 GiB in all) and each group_log, alternating in the same process, device events
around each whole call (the host's table fill and upload included), medians over about a second a route:
  verify   b3w_bao_verify_batch_device of this library on clean files, outboards and roots (statuses checked all zero before timing)
  (a)      the outboard call of the library given with --parent-lib (a build of the commit before verification, loaded beside this
           one, its own context) on the same files: the same compressions; verify reads the nodes this call writes.  Measured as two
           interleaved series A and B; |median A - median B| is the spread a difference has to exceed to mean anything.
  (b)      the yes/no route: (a) into a second buffer, then torch.equal on the outboards and the roots
  (c)      on 1024x1MiB only, the one route that gave the same verdicts: the parent's planner with every unit as a sample
           (b3w_sample_plan_batch_device over every chunk; group_log >= 1: b3w_sample_plan_group_batch_device, a sample a group), two
           interleaved series.  THE GATE: verify must be faster than (c) by more than the spread of (c)'s two series; the tool
           exits non-zero where it is not.
Writes <out_dir>/bao_verify_measure.json.  --quick: ten calls of verify and of (a) a shape, no timing — for a run under `rocprofv3
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
GATE_SHAPE = "1024x1MiB"


def parent_library(path):
    """the yardstick library and a nova_vesta context of its own -> (lib, ctx handle)"""
    vp, u32, i32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64
    P = ctypes.CDLL(path)
    P.b3w_abi_version.restype = u32
    P.b3w_create.restype, P.b3w_create.argtypes = i32, [i32, i32, ctypes.POINTER(vp)]
    P.b3w_destroy.restype, P.b3w_destroy.argtypes = None, [vp]
    P.b3w_bao_outboard_batch_device.restype, P.b3w_bao_outboard_batch_device.argtypes = i32, [vp, vp, vp, vp, u32, vp, vp, vp, u64, vp]
    P.b3w_bao_group_outboard_batch_device.restype, P.b3w_bao_group_outboard_batch_device.argtypes = i32, [vp, vp, vp, vp, u32, u32, vp, vp, vp, u64, vp]
    P.b3w_sample_plan_batch_device.restype, P.b3w_sample_plan_batch_device.argtypes = i32, [vp, vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp]
    P.b3w_sample_plan_group_batch_device.restype, P.b3w_sample_plan_group_batch_device.argtypes = i32, [vp, vp, u32, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp]
    h = vp()
    rc = P.b3w_create(m.CIRCUIT_ID["nova_vesta"], 0, ctypes.byref(h))
    assert rc == 0, rc
    return P, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--parent-lib", required=True, help="libb3wit.so built from the commit before verification: routes (a), (b), (c)")
    ap.add_argument("--quick", action="store_true", help="ten calls of verify and of (a) a shape (under a profiler)")
    ap.add_argument("--shapes", default="", help="comma-separated subset of the shape names")
    ap.add_argument("--group-logs", default="0,4")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bao_verify_measure: no GPU")
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    Y, y_ctx = parent_library(a.parent_lib)
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_arena = torch.randint(0, 256, (BM.GIB + (1 << 20),), dtype=torch.uint8, device="cuda", generator=gen)
    base = d_arena.data_ptr()
    res = dict(device=torch.cuda.get_device_name(0), arena_bytes=BM.GIB, parent=f"{os.path.basename(a.parent_lib)} (ABI {Y.b3w_abi_version() >> 16}.{Y.b3w_abi_version() & 0xffff})",
               shapes={}, gate={})
    want = [x for x in a.shapes.split(",") if x]
    failed = []
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
        for gl in [int(x) for x in a.group_logs.split(",")]:
            ob_first, unit_first = m.bao.group_batch_layout(lens, gl), m.bao.verify_layout(lens, gl)
            d_obs = torch.empty(int(ob_first[-1]), dtype=torch.uint8, device="cuda")
            d_obs2 = torch.empty_like(d_obs)
            d_roots, d_roots2 = torch.empty((n_files, 8), dtype=torch.int32, device="cuda"), torch.empty((n_files, 8), dtype=torch.int32, device="cuda")
            need_y = L.b3w_bao_batch_scratch_bytes(lens.ctypes.data, n_files)
            d_scr_y = torch.empty(max(need_y, 16), dtype=torch.uint8, device="cuda")
            need_v = L.b3w_bao_verify_scratch_bytes(lens.ctypes.data, n_files)
            d_scr_v = torch.empty(max(need_v, 16), dtype=torch.uint8, device="cuda")
            d_st = torch.full((int(unit_first[-1]),), 0xEE, dtype=torch.uint8, device="cuda")
            d_fs = torch.full((n_files,), -1, dtype=torch.int32, device="cuda")
            d_fb = torch.zeros(n_files, dtype=torch.int64, device="cuda")

            def outboard(obs, roots):
                if gl == 0:
                    rc = Y.b3w_bao_outboard_batch_device(y_ctx, base, offsets.ctypes.data, lens.ctypes.data, n_files, obs.data_ptr(), roots.data_ptr(),
                                                         d_scr_y.data_ptr(), need_y, s)
                else:
                    rc = Y.b3w_bao_group_outboard_batch_device(y_ctx, base, offsets.ctypes.data, lens.ctypes.data, n_files, gl, obs.data_ptr(),
                                                               roots.data_ptr(), d_scr_y.data_ptr(), need_y, s)
                assert rc == 0, rc

            def route_a():
                outboard(d_obs2, d_roots2)

            def route_b():
                outboard(d_obs2, d_roots2)
                assert torch.equal(d_obs2, d_obs) and torch.equal(d_roots2, d_roots)

            def verify():
                rc = L.b3w_bao_verify_batch_device(ctx.handle, base, offsets.ctypes.data, lens.ctypes.data, n_files, gl, d_obs.data_ptr(), d_roots.data_ptr(),
                                                   d_st.data_ptr(), d_fs.data_ptr(), d_fb.data_ptr(), d_scr_v.data_ptr(), need_v, s)
                assert rc == 0, ctx.last_error()
            outboard(d_obs, d_roots)
            verify()
            torch.cuda.synchronize()
            assert not d_st.any().item() and not d_fs.any().item() and bool((d_fb == -1).all().item()), f"{name} g = {gl}: a clean batch does not verify"
            row = dict(n_files=int(n_files), bytes=int(lens.sum()), group_log=gl, outboard_bytes=int(ob_first[-1]), units=int(unit_first[-1]),
                       verify_scratch_bytes=int(need_v), bound_ms=BM.bound_ms(lens_l))
            key = f"{name}_g{gl}"
            if a.quick:
                for _ in range(QUICK_CALLS):
                    route_a()
                torch.cuda.synchronize()
                for _ in range(QUICK_CALLS):
                    verify()
                torch.cuda.synchronize()
                row["calls_each"] = QUICK_CALLS
                res["shapes"][key] = row
                continue
            for _ in range(3):
                route_a()
                verify()
                route_b()
            t = alternating({"a_a": route_a, "verify": verify, "b": route_b, "a_b": route_a})
            row.update(verify=stats(t["verify"]), a=stats(t["a_a"] + t["a_b"]), a_a=stats(t["a_a"]), a_b=stats(t["a_b"]), b=stats(t["b"]))
            row["a_spread_ms"] = abs(row["a_a"]["ms"] - row["a_b"]["ms"])
            row["verify_minus_a_ms"] = row["verify"]["ms"] - row["a"]["ms"]
            row["verify_over_a"] = row["verify"]["ms"] / row["a"]["ms"]
            row["verify_over_b"] = row["verify"]["ms"] / row["b"]["ms"]
            row["verify_share_of_bound"] = row["bound_ms"] / row["verify"]["ms"]
            row["a_share_of_bound"] = row["bound_ms"] / row["a"]["ms"]
            if name == GATE_SHAPE:                                               # (c): every unit a sample; the files lie back to back, so the
                units = int(unit_first[-1])                                      # samples' bytes in file order are the arena itself
                per = units // n_files
                files = np.repeat(np.arange(n_files, dtype=np.uint32), per)
                chunks = np.tile(np.arange(per, dtype=np.uint64) << np.uint64(gl), n_files)
                rf = m.bao.sample_rows_batch(lens, files, chunks)
                d_recs = torch.empty((int(rf[-1]), 32), dtype=torch.int32, device="cuda")
                d_ss = torch.full((units,), -1, dtype=torch.int32, device="cuda")

                def route_c():
                    if gl == 0:
                        rc = Y.b3w_sample_plan_batch_device(y_ctx, lens.ctypes.data, n_files, d_obs.data_ptr(), d_roots.data_ptr(), files.ctypes.data,
                                                            chunks.ctypes.data, units, base, d_recs.data_ptr(), d_ss.data_ptr(), s)
                    else:
                        rc = Y.b3w_sample_plan_group_batch_device(y_ctx, lens.ctypes.data, n_files, gl, d_obs.data_ptr(), d_roots.data_ptr(), files.ctypes.data,
                                                                  chunks.ctypes.data, units, base, d_recs.data_ptr(), d_ss.data_ptr(), s)
                    assert rc == 0, rc
                route_c()
                torch.cuda.synchronize()
                assert not d_ss.any().item(), "route (c) does not verify the clean batch"
                tc = alternating({"c_a": route_c, "verify": verify, "c_b": route_c})
                row.update(c=stats(tc["c_a"] + tc["c_b"]), c_a=stats(tc["c_a"]), c_b=stats(tc["c_b"]), verify_beside_c=stats(tc["verify"]),
                           c_samples=units, c_record_bytes=int(d_recs.numel()) * 4)
                row["c_spread_ms"] = abs(row["c_a"]["ms"] - row["c_b"]["ms"])
                row["c_over_verify"] = row["c"]["ms"] / row["verify_beside_c"]["ms"]
                ok = row["verify_beside_c"]["ms"] + row["c_spread_ms"] < row["c"]["ms"]
                res["gate"][key] = dict(verify_ms=row["verify_beside_c"]["ms"], c_ms=row["c"]["ms"], c_spread_ms=row["c_spread_ms"], passed=bool(ok))
                if not ok:
                    failed.append(key)
                del d_recs, d_ss
            res["shapes"][key] = row
            print(key, json.dumps(row), flush=True)
    Y.b3w_destroy(y_ctx)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_verify_measure.json" if not a.quick else "bao_verify_measure_quick.json"), "w"), indent=1)
    print(json.dumps(res["gate"], indent=1))
    if failed:
        sys.exit(f"bao_verify_measure: verify is not faster than route (c) by more than its spread: {failed}")


if __name__ == "__main__":
    main()
