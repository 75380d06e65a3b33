#!/usr/bin/env python3
"""tools/bao_stream_open_measure.py <out_dir> --parent-lib libb3wit.so [--quick] [--files 64,1024] [--windows 4,64] [--group-logs 0,4]
— what it costs an outboard stream session not to know the file's length (b3w_bao_stream_open_*).  Needs a GPU; there is no fall-back.

Resident files of 64 MiB and 1 GiB, windows of 4 and 64 MiB, g = 0 and 4.  Routes, alternating in one process, device events around
each whole route (begin and free included), medians over about a second a route:
  a  the known-length session of the library given with --parent-lib (a build of the commit before, loaded beside this one, with a
     context of its own): b3w_bao_stream_outboard_begin, the pushes, b3w_bao_stream_finish.  Two interleaved series; |median of one -
     median of the other| is its spread.
  b  the open session: b3w_bao_stream_open_begin, the pushes, b3w_bao_stream_open_finish (no tail: the files are whole MiB)
  c  one device-to-device hipMemcpyAsync (a torch copy_) of the outboard's byte count
The claim: b - a <= c + a's spread on every shape (`claim_holds`): openness costs no more than copying the outboard once.  b's outboard
and root are compared with a's once before timing.
Writes <out_dir>/bao_stream_open_measure.json.  --quick: ten passes of route b per shape of the 64 MiB file and nothing timed — for a
run under `rocprofv3 --kernel-trace --stats`, made alone: the relocation kernel's calls / 10 are its launches a pass (one), its time
over the outboard's bytes its rate."""
import argparse, ctypes, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch

import bao_batch_measure as BM
from bao_groups_measure import stats
from bao_stream_many_measure import parent_library

m = __import__("hot-proofs-blake3-circom_amd")

MIB = 1 << 20
QUICK_PASSES = 10


def alternating(routes, window_s=1.0, rounds=3):
    out = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            t0 = time.time()
            while True:
                out[k].append(BM.one_pass_ms(fn))
                if time.time() - t0 >= window_s / rounds:
                    break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--parent-lib", required=True, help="libb3wit.so built from the commit before the open sessions: the yardstick")
    ap.add_argument("--quick", action="store_true", help="ten passes of route b on the 64 MiB file (under a profiler)")
    ap.add_argument("--files", default="64,1024", help="file sizes in MiB")
    ap.add_argument("--windows", default="4,64", help="window sizes in MiB")
    ap.add_argument("--group-logs", default="0,4")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bao_stream_open_measure: no GPU")
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    Y, y_ctx = parent_library(a.parent_lib)
    s = torch.cuda.current_stream().cuda_stream
    files = [64] if a.quick else [int(x) for x in a.files.split(",")]
    windows = [int(x) for x in a.windows.split(",")]
    gen = torch.Generator(device="cuda").manual_seed(15)
    arena = torch.randint(0, 256, (max(files) * MIB,), dtype=torch.uint8, device="cuda", generator=gen)
    base = arena.data_ptr()
    res = dict(device=torch.cuda.get_device_name(0), parent=f"{os.path.basename(a.parent_lib)} (ABI {Y.b3w_abi_version() >> 16}.{Y.b3w_abi_version() & 0xffff})",
               shapes={})
    for mib in files:
        n = mib * MIB
        for gl in [int(x) for x in a.group_logs.split(",")]:
            ob_bytes = m.bao.group_outboard_size(n, gl)
            ob_a, ob_b, ob_c = (torch.empty(ob_bytes, dtype=torch.uint8, device="cuda") for _ in range(3))
            root_a, root_b = (torch.empty(8, dtype=torch.int32, device="cuda") for _ in range(2))
            need_a = L.b3w_bao_stream_scratch_bytes(n, 0)
            need_s, need_b = L.b3w_bao_stream_open_staging_bytes(n, gl), L.b3w_bao_stream_open_scratch_bytes(n)
            scr_a, scr_b = torch.empty(need_a, dtype=torch.uint8, device="cuda"), torch.empty(need_b, dtype=torch.uint8, device="cuda")
            staging = torch.empty(need_s, dtype=torch.uint8, device="cuda")

            def known(window):
                h = ctypes.c_void_p()
                assert Y.b3w_bao_stream_outboard_begin(y_ctx, n, gl, ob_a.data_ptr(), root_a.data_ptr(), scr_a.data_ptr(), need_a, ctypes.byref(h)) == 0
                for off in range(0, n, window):
                    assert Y.b3w_bao_stream_push(h, off, base + off, min(window, n - off), s) == 0
                assert Y.b3w_bao_stream_finish(h, s) == 0
                Y.b3w_bao_stream_free(h)

            def opened(window):
                h = ctypes.c_void_p()
                assert L.b3w_bao_stream_open_begin(ctx.handle, n, gl, staging.data_ptr(), need_s, scr_b.data_ptr(), need_b, ctypes.byref(h)) == 0, ctx.last_error()
                for off in range(0, n, window):
                    assert L.b3w_bao_stream_push(h, off, base + off, min(window, n - off), s) == 0, ctx.last_error()
                assert L.b3w_bao_stream_open_finish(h, None, 0, ob_b.data_ptr(), ob_bytes, root_b.data_ptr(), s, None) == 0, ctx.last_error()
                L.b3w_bao_stream_free(h)

            def copy():
                ob_c.copy_(ob_a, non_blocking=True)
            ob_b.zero_()
            known(4 * MIB)
            opened(4 * MIB)
            torch.cuda.synchronize()
            assert torch.equal(ob_a, ob_b) and torch.equal(root_a, root_b), f"{mib} MiB, g = {gl}: the open session's outboard differs"
            for w in windows:
                name = f"f{mib}_g{gl}_w{w}"
                if a.quick:
                    for _ in range(QUICK_PASSES):
                        opened(w * MIB)
                    torch.cuda.synchronize()
                    res["shapes"][name] = dict(passes=QUICK_PASSES, file_mib=mib, group_log=gl, window_mib=w, outboard_bytes=ob_bytes)
                    continue
                routes = {"a_1": lambda: known(w * MIB), "b": lambda: opened(w * MIB), "c": copy, "a_2": lambda: known(w * MIB)}
                for fn in routes.values():
                    fn()
                t = alternating(routes)
                row = dict(file_mib=mib, group_log=gl, window_mib=w, pushes=-(-n // (w * MIB)), outboard_bytes=ob_bytes)
                row["a"] = stats(t["a_1"] + t["a_2"])
                row["a"]["spread_ms"] = abs(stats(t["a_1"])["ms"] - stats(t["a_2"])["ms"])
                row["b"], row["c"] = stats(t["b"]), stats(t["c"])
                row.update(b_minus_a_ms=row["b"]["ms"] - row["a"]["ms"], allowance_ms=row["c"]["ms"] + row["a"]["spread_ms"],
                           claim_holds=bool(row["b"]["ms"] - row["a"]["ms"] <= row["c"]["ms"] + row["a"]["spread_ms"]),
                           a_gb_s=n / row["a"]["ms"] / 1e6, b_gb_s=n / row["b"]["ms"] / 1e6, copy_gb_s=ob_bytes / row["c"]["ms"] / 1e6,
                           open_finish_launches_at_most=4)
                res["shapes"][name] = row
                print(name, json.dumps(row), flush=True)
    if not a.quick:
        res["claim_holds_everywhere"] = all(r["claim_holds"] for r in res["shapes"].values())
    Y.b3w_destroy(y_ctx)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_stream_open_measure.json" if not a.quick else "bao_stream_open_measure_quick.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
