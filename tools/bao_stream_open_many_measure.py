#!/usr/bin/env python3
"""tools/bao_stream_open_many_measure.py <out_dir> --parent-lib libb3wit.so [--quick] [--sessions 1,16,256] [--files 1,4,64] [--group-logs 0,4]
— what finishing many open-length stream sessions in one call saves (b3w_bao_stream_open_finish_many).  Needs a GPU; there is no
fall-back.

n resident open sessions, each a file of 1 MiB + 5, 4 MiB + 5 or (n <= 16) 64 MiB + 5 bytes, g = 0 and 4.  Every repetition begins and
pushes its sessions afresh OUTSIDE the timed region (a session finishes once) and waits for the pushes; device events go around the
finishes only.  Routes, alternating in one process, medians over about a second a route:
  a  the library given with --parent-lib (a build of the commit before, loaded beside this one, with a context of its own): the n
     sessions finished one at a time with b3w_bao_stream_open_finish on one stream.  Two interleaved series; |median of one - median of
     the other| is its spread.
  b  b3w_bao_stream_open_finish_many over n sessions of this library, the same bytes, outboards of the same alignment
The claim, for n >= 16: b is below a by more than a's spread on every shape (`claim_holds`).  For n = 1 b - a is reported and not gated:
it carries one table upload.  The host's wall time of the finish calls alone (the enqueueing, nothing waited for) is recorded beside
each route and not gated.  b's outboards and roots are compared with a's once per shape before timing.
Writes <out_dir>/bao_stream_open_many_measure.json.  --quick: ten many-calls per shape of n = 16 and the two small files and nothing
timed — for a run under `rocprofv3 --kernel-trace --stats`, made alone: the calls of the *_many_* kernels over `many_calls` of the
JSON are the launches a many-call (at most four), and b3w_bao_stream_open_relocate_many_kernel's time is the new kernel's own."""
import argparse, ctypes, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

from bao_groups_measure import stats
from bao_stream_many_measure import parent_library

m = __import__("hot-proofs-blake3-circom_amd")

MIB = 1 << 20
QUICK_PASSES = 10


def bind_open(P):
    vp, u32, i32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64
    P.b3w_bao_stream_open_begin.restype, P.b3w_bao_stream_open_begin.argtypes = i32, [vp, u64, u32, vp, u64, vp, u64, ctypes.POINTER(vp)]
    P.b3w_bao_stream_open_finish.restype, P.b3w_bao_stream_open_finish.argtypes = i32, [vp, vp, u64, vp, u64, vp, vp, ctypes.POINTER(u64)]


class Sessions:
    """n open sessions of one library over the same file: their stagings, scratches, outboards and roots are made once; begin_and_push()
    makes the sessions afresh, finish_*() ends them, free() frees the host objects"""

    def __init__(self, lib, ctx_handle, n, d_file, gl):
        self.lib, self.ctx, self.n, self.d, self.gl = lib, ctx_handle, n, d_file, gl
        ln = d_file.numel()
        self.whole = ln // MIB * MIB
        self.need_s, self.need_c = m.lib().b3w_bao_stream_open_staging_bytes(ln, gl), m.lib().b3w_bao_stream_open_scratch_bytes(ln)
        self.ob_bytes = m.bao.group_outboard_size(ln, gl)
        self.staging = [torch.empty(self.need_s, dtype=torch.uint8, device="cuda") for _ in range(n)]
        self.scratch = [torch.empty(self.need_c, dtype=torch.uint8, device="cuda") for _ in range(n)]
        self.obs = [torch.zeros(self.ob_bytes, dtype=torch.uint8, device="cuda") for _ in range(n)]
        self.roots = [torch.zeros(8, dtype=torch.int32, device="cuda") for _ in range(n)]
        self.h = []
        tail = d_file[self.whole:]
        self.arrays = [np.array(x, dtype=np.uint64) for x in ([tail.data_ptr()] * n, [tail.numel()] * n, [o.data_ptr() for o in self.obs],
                                                              [self.ob_bytes] * n, [r.data_ptr() for r in self.roots])]
        self.lens = np.zeros(n, dtype=np.uint64)

    def begin_and_push(self, s):
        self.h = []
        for i in range(self.n):
            h = ctypes.c_void_p()
            assert self.lib.b3w_bao_stream_open_begin(self.ctx, self.d.numel(), self.gl, self.staging[i].data_ptr(), self.need_s, self.scratch[i].data_ptr(),
                                                      self.need_c, ctypes.byref(h)) == 0
            assert self.lib.b3w_bao_stream_push(h, 0, self.d.data_ptr(), self.whole, s) == 0
            self.h.append(h)

    def finish_each(self, s):
        tp, tb, op, ob, rp = self.arrays
        for i, h in enumerate(self.h):
            assert self.lib.b3w_bao_stream_open_finish(h, int(tp[i]), int(tb[i]), int(op[i]), int(ob[i]), int(rp[i]), s, None) == 0

    def finish_many(self, s):
        hs = np.array([h.value for h in self.h], dtype=np.uint64)
        assert self.lib.b3w_bao_stream_open_finish_many(self.ctx, hs.ctypes.data, *[a.ctypes.data for a in self.arrays], self.n, s, self.lens.ctypes.data) == 0

    def free(self):
        for h in self.h:
            self.lib.b3w_bao_stream_free(h)
        self.h = []


def one_pass(sessions, finish, s):
    """-> (device ms around the finishes, host ms of the finish calls)"""
    sessions.begin_and_push(s)
    torch.cuda.synchronize()                                # the pushes are through: the finishes alone lie between the events
    st = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    t = time.perf_counter()
    finish(s)
    host = (time.perf_counter() - t) * 1e3
    b.record(st)
    b.synchronize()
    sessions.free()
    return a.elapsed_time(b), host


def alternating(routes, window_s=1.0, rounds=3):
    out = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            t0 = time.time()
            while True:
                out[k].append(fn())
                if time.time() - t0 >= window_s / rounds:
                    break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--parent-lib", required=True, help="libb3wit.so built from the commit before b3w_bao_stream_open_finish_many: the yardstick")
    ap.add_argument("--quick", action="store_true", help="ten many-calls per shape of 16 sessions (under a profiler)")
    ap.add_argument("--sessions", default="1,16,256")
    ap.add_argument("--files", default="1,4,64", help="file sizes in MiB (each 5 bytes longer); 64 and above only for n <= 16")
    ap.add_argument("--group-logs", default="0,4")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bao_stream_open_many_measure: no GPU")
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    Y, y_ctx = parent_library(a.parent_lib)
    bind_open(Y)
    s = torch.cuda.current_stream().cuda_stream
    ns = [16] if a.quick else [int(x) for x in a.sessions.split(",")]
    files = [x for x in (int(x) for x in a.files.split(",")) if not a.quick or x < 64]
    gen = torch.Generator(device="cuda").manual_seed(16)
    arena = torch.randint(0, 256, (max(files) * MIB + 5,), dtype=torch.uint8, device="cuda", generator=gen)
    res = dict(device=torch.cuda.get_device_name(0), parent=f"{os.path.basename(a.parent_lib)} (ABI {Y.b3w_abi_version() >> 16}.{Y.b3w_abi_version() & 0xffff})",
               shapes={}, many_calls=0)
    for n in ns:
        for mib in files:
            if mib >= 64 and n > 16:
                continue
            for gl in [int(x) for x in a.group_logs.split(",")]:
                d_file = arena[:mib * MIB + 5]
                ya, yb = Sessions(Y, y_ctx, n, d_file, gl), Sessions(L, ctx.handle, n, d_file, gl)
                one_pass(ya, ya.finish_each, s)
                one_pass(yb, yb.finish_many, s)
                res["many_calls"] += 1
                torch.cuda.synchronize()
                assert all(int(x) == d_file.numel() for x in yb.lens)
                for i in range(n):
                    assert torch.equal(ya.obs[i], yb.obs[i]) and torch.equal(ya.roots[i], yb.roots[i]), f"n {n}, {mib} MiB, g = {gl}: session {i} differs"
                name = f"n{n}_f{mib}_g{gl}"
                if a.quick:
                    for _ in range(QUICK_PASSES):
                        one_pass(yb, yb.finish_many, s)
                    res["many_calls"] += QUICK_PASSES
                    res["shapes"][name] = dict(passes=QUICK_PASSES, sessions=n, file_bytes=d_file.numel(), group_log=gl, outboard_bytes=yb.ob_bytes)
                    continue
                t = alternating({"a_1": lambda: one_pass(ya, ya.finish_each, s), "b": lambda: one_pass(yb, yb.finish_many, s),
                                 "a_2": lambda: one_pass(ya, ya.finish_each, s)})
                dev = {k: [x[0] for x in v] for k, v in t.items()}
                host = {k: [x[1] for x in v] for k, v in t.items()}
                row = dict(sessions=n, file_bytes=d_file.numel(), group_log=gl, outboard_bytes=yb.ob_bytes)
                row["a"] = stats(dev["a_1"] + dev["a_2"])
                row["a"]["spread_ms"] = abs(stats(dev["a_1"])["ms"] - stats(dev["a_2"])["ms"])
                row["a"]["host_ms"] = float(np.median(host["a_1"] + host["a_2"]))
                row["b"] = stats(dev["b"])
                row["b"]["host_ms"] = float(np.median(host["b"]))
                row.update(b_minus_a_ms=row["b"]["ms"] - row["a"]["ms"], a_over_b=row["a"]["ms"] / row["b"]["ms"], gated=n >= 16,
                           claim_holds=bool(row["a"]["ms"] - row["b"]["ms"] > row["a"]["spread_ms"]) if n >= 16 else None, many_call_launches_at_most=4)
                res["shapes"][name] = row
                print(name, json.dumps(row), flush=True)
    if not a.quick:
        res["claim_holds_everywhere"] = all(r["claim_holds"] for r in res["shapes"].values() if r["gated"])
    Y.b3w_destroy(y_ctx)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_stream_open_many_measure.json" if not a.quick else "bao_stream_open_many_measure_quick.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
