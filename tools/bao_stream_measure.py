#!/usr/bin/env python3
"""tools/bao_stream_measure.py <out_dir> --parent-lib libb3wit.so [--quick] [--group-logs 0,4] [--host-gib 4] [--no-host] — stream
sessions (b3w_bao_stream_*) against the calls that take the whole file resident.  Needs a GPU; there is no fall-back.

  device-resident   one 1 GiB file on the device, pushed in windows of 1, 16, 64 and 256 MiB plus finish (begin and free included),
                    against b3w_bao_outboard_batch_device / b3w_bao_group_outboard_batch_device of the library given with
                    --parent-lib (a build of the commit before, loaded beside this one, its own context) on the same file, and the
                    verify sessions against its b3w_bao_verify_batch_device.  Alternating in one process, device events around
                    each whole route, medians over about a second a route.  The yardstick runs as two interleaved series A and B;
                    |median A - median B| is the spread a difference has to exceed to mean anything.  Reported per window size:
                    streamed / parent and (streamed - parent) / pushes, the cost of a push.  Results compared once before timing.
  from the host     bao.outboard_stream over --host-gib GiB of pinned host memory, ring 2, windows of 4, 16 and 64 MiB, against
                    (a) the same bytes through the same ring with no kernel (two series) and (b) the route that existed: the whole
                    file copied to the device, then the parent's batch call.  Wall time, each route ending in a synchronise.
                    The claim: helper - (a) is no more than the last window's kernel time (one push timed alone) plus (a)'s
                    spread, i.e. the hashing hides behind the copy.  Reported either way, nothing is gated.  Both are taken
                    twice: from the numpy view (staged through the ring's pinned buffers) and from the pinned tensor itself
                    (`pinned`: copied from where it lies).
Writes <out_dir>/bao_stream_measure.json.  --quick: ten outboard and ten verify sessions at 16 MiB windows and ten calls of each
yardstick, no timing — for a run under `rocprofv3 --kernel-trace --stats`: a kernel's calls / 10 are its launches a session (64
pushes, one finish)."""
import argparse, ctypes, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bao_batch_measure as BM
from bao_groups_measure import alternating, stats

m = __import__("hot-proofs-blake3-circom_amd")

MIB = 1 << 20
QUICK_CALLS = 10
WINDOWS = [1, 16, 64, 256]
HOST_WINDOWS = [4, 16, 64]


def parent_library(path):
    """the yardstick library and a nova_vesta context of its own -> (lib, ctx handle)"""
    vp, u32, i32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64
    P = ctypes.CDLL(path)
    P.b3w_abi_version.restype = u32
    P.b3w_create.restype, P.b3w_create.argtypes = i32, [i32, i32, ctypes.POINTER(vp)]
    P.b3w_destroy.restype, P.b3w_destroy.argtypes = None, [vp]
    P.b3w_bao_outboard_batch_device.restype, P.b3w_bao_outboard_batch_device.argtypes = i32, [vp, vp, vp, vp, u32, vp, vp, vp, u64, vp]
    P.b3w_bao_group_outboard_batch_device.restype, P.b3w_bao_group_outboard_batch_device.argtypes = i32, [vp, vp, vp, vp, u32, u32, vp, vp, vp, u64, vp]
    P.b3w_bao_verify_batch_device.restype, P.b3w_bao_verify_batch_device.argtypes = i32, [vp, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, u64, vp]
    h = vp()
    rc = P.b3w_create(m.CIRCUIT_ID["nova_vesta"], 0, ctypes.byref(h))
    assert rc == 0, rc
    return P, h


class _NoKernel:
    """a session that launches nothing: route (a), the ring alone"""

    def push(self, offset, d_window, stream=0):
        pass


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--parent-lib", required=True, help="libb3wit.so built from the commit before stream sessions: the yardstick")
    ap.add_argument("--quick", action="store_true", help="ten sessions and ten yardstick calls a kind (under a profiler)")
    ap.add_argument("--group-logs", default="0,4")
    ap.add_argument("--host-gib", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bao_stream_measure: no GPU")
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    Y, y_ctx = parent_library(a.parent_lib)
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    ln = BM.GIB
    d_file = torch.randint(0, 256, (ln,), dtype=torch.uint8, device="cuda", generator=gen)
    base = d_file.data_ptr()
    one_off, one_len = np.zeros(1, dtype=np.uint64), np.array([ln], dtype=np.uint64)
    res = dict(device=torch.cuda.get_device_name(0), file_bytes=ln, parent=f"{os.path.basename(a.parent_lib)} (ABI {Y.b3w_abi_version() >> 16}.{Y.b3w_abi_version() & 0xffff})",
               resident={}, host={})
    for gl in [int(x) for x in a.group_logs.split(",")]:
        ob_bytes = int(m.bao.group_outboard_size(ln, gl))
        units = int(m.bao.verify_layout(one_len, gl)[-1])
        d_ob, d_ob2 = torch.empty(ob_bytes, dtype=torch.uint8, device="cuda"), torch.empty(ob_bytes, dtype=torch.uint8, device="cuda")
        d_root, d_root2 = torch.empty(8, dtype=torch.int32, device="cuda"), torch.empty(8, dtype=torch.int32, device="cuda")
        need_o, need_v = L.b3w_bao_stream_scratch_bytes(ln, 0), L.b3w_bao_stream_scratch_bytes(ln, 1)
        d_scr_y, d_scr_o, d_scr_v = (torch.empty(max(n, 16), dtype=torch.uint8, device="cuda") for n in (need_o, need_o, need_v))
        d_scr_vy = torch.empty(max(need_v, 16), dtype=torch.uint8, device="cuda")
        d_st, d_st2 = torch.full((units,), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((units,), 0xEE, dtype=torch.uint8, device="cuda")
        d_fs, d_fs2 = torch.full((1,), -1, dtype=torch.int32, device="cuda"), torch.full((1,), -1, dtype=torch.int32, device="cuda")
        d_fb, d_fb2 = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")

        def parent_outboard():
            if gl == 0:
                rc = Y.b3w_bao_outboard_batch_device(y_ctx, base, one_off.ctypes.data, one_len.ctypes.data, 1, d_ob.data_ptr(), d_root.data_ptr(), d_scr_y.data_ptr(), need_o, s)
            else:
                rc = Y.b3w_bao_group_outboard_batch_device(y_ctx, base, one_off.ctypes.data, one_len.ctypes.data, 1, gl, d_ob.data_ptr(), d_root.data_ptr(),
                                                           d_scr_y.data_ptr(), need_o, s)
            assert rc == 0, rc

        def parent_verify():
            rc = Y.b3w_bao_verify_batch_device(y_ctx, base, one_off.ctypes.data, one_len.ctypes.data, 1, gl, d_ob.data_ptr(), d_root.data_ptr(), d_st.data_ptr(),
                                               d_fs.data_ptr(), d_fb.data_ptr(), d_scr_vy.data_ptr(), need_v, s)
            assert rc == 0, rc

        def session(kind, window):
            h = ctypes.c_void_p()
            if kind == "outboard":
                rc = L.b3w_bao_stream_outboard_begin(ctx.handle, ln, gl, d_ob2.data_ptr(), d_root2.data_ptr(), d_scr_o.data_ptr(), need_o, ctypes.byref(h))
            else:
                rc = L.b3w_bao_stream_verify_begin(ctx.handle, ln, gl, d_ob.data_ptr(), d_root.data_ptr(), d_st2.data_ptr(), d_fs2.data_ptr(), d_fb2.data_ptr(),
                                                   d_scr_v.data_ptr(), need_v, s, ctypes.byref(h))
            assert rc == 0, ctx.last_error()
            for off in range(0, ln, window):
                rc = L.b3w_bao_stream_push(h, off, base + off, min(window, ln - off), s)
                assert rc == 0, ctx.last_error()
            rc = L.b3w_bao_stream_finish(h, s)
            assert rc == 0, ctx.last_error()
            L.b3w_bao_stream_free(h)
        parent_outboard()
        parent_verify()
        session("outboard", 16 * MIB)
        session("verify", 16 * MIB)
        torch.cuda.synchronize()
        assert torch.equal(d_ob, d_ob2) and torch.equal(d_root, d_root2), f"g = {gl}: the streamed outboard is not the batch call's"
        assert torch.equal(d_st, d_st2) and torch.equal(d_fs, d_fs2) and torch.equal(d_fb, d_fb2) and not d_st.any().item(), f"g = {gl}: verification differs"
        row = dict(group_log=gl, outboard_bytes=ob_bytes, units=units, bound_ms=BM.bound_ms([ln]))
        if a.quick:
            for fn in (parent_outboard, parent_verify, lambda: session("outboard", 16 * MIB), lambda: session("verify", 16 * MIB)):
                for _ in range(QUICK_CALLS):
                    fn()
                torch.cuda.synchronize()
            row.update(calls_each=QUICK_CALLS, window_mib=16, pushes_a_session=ln // (16 * MIB))
            res["resident"][f"g{gl}"] = row
            continue
        for kind, parent in (("outboard", parent_outboard), ("verify", parent_verify)):
            routes = {"parent_a": parent}
            for w in WINDOWS:
                routes[f"w{w}"] = (lambda w=w: session(kind, w * MIB))
            routes["parent_b"] = parent
            for fn in routes.values():
                fn()
            t = alternating(routes)
            k = dict(parent=stats(t["parent_a"] + t["parent_b"]), parent_a=stats(t["parent_a"]), parent_b=stats(t["parent_b"]))
            k["parent_spread_ms"] = abs(k["parent_a"]["ms"] - k["parent_b"]["ms"])
            for w in WINDOWS:
                st = stats(t[f"w{w}"])
                pushes = ln // (w * MIB)
                st.update(pushes=pushes, over_parent=st["ms"] / k["parent"]["ms"], minus_parent_ms=st["ms"] - k["parent"]["ms"],
                          per_push_us=(st["ms"] - k["parent"]["ms"]) * 1e3 / pushes)
                k[f"window_{w}MiB"] = st
            row[kind] = k
        # one push alone: what the last window of a host stream costs after its copy
        h = ctypes.c_void_p()
        assert L.b3w_bao_stream_outboard_begin(ctx.handle, ln, gl, d_ob2.data_ptr(), d_root2.data_ptr(), d_scr_o.data_ptr(), need_o, ctypes.byref(h)) == 0
        row["one_push_ms"] = {}
        for i, w in enumerate(HOST_WINDOWS):
            off = i * 64 * MIB
            row["one_push_ms"][f"{w}MiB"] = BM.one_pass_ms(lambda: L.b3w_bao_stream_push(h, off, base + off, w * MIB, s))
        L.b3w_bao_stream_free(h)
        res["resident"][f"g{gl}"] = row
        print(f"g{gl}", json.dumps(row), flush=True)
    if not a.quick and not a.no_host:
        hl = a.host_gib << 30
        pinned = torch.empty(hl, dtype=torch.uint8, pin_memory=True)
        host = pinned.numpy()
        block = np.random.default_rng(5).integers(0, 256, 64 * MIB, dtype=np.uint8)
        for off in range(0, hl, block.size):
            host[off:off + block.size] = block
        h_len = np.array([hl], dtype=np.uint64)
        d_whole = torch.empty(hl, dtype=torch.uint8, device="cuda")
        d_ob = torch.empty(int(m.bao.outboard_size(hl)), dtype=torch.uint8, device="cuda")
        need = L.b3w_bao_batch_scratch_bytes(h_len.ctypes.data, 1)
        d_scr = torch.empty(need, dtype=torch.uint8, device="cuda")

        def route_b():
            d_whole.copy_(pinned, non_blocking=True)
            rc = Y.b3w_bao_outboard_batch_device(y_ctx, d_whole.data_ptr(), one_off.ctypes.data, h_len.ctypes.data, 1, d_ob.data_ptr(), d_root.data_ptr(),
                                                 d_scr.data_ptr(), need, s)
            assert rc == 0, rc
        hrow = dict(bytes=hl, ring=2, reps=a.host_reps)
        route_b()
        torch.cuda.synchronize()
        want_root = d_root.clone()
        hrow["b_whole_copy_then_batch_ms"] = stats([wall_ms(route_b) for _ in range(a.host_reps)])
        for w in HOST_WINDOWS:
            got = m.bao.outboard_stream(ctx, host, hl, w * MIB, 0, ring=2)
            torch.cuda.synchronize()
            assert torch.equal(got["roots"].view(-1), want_root) and torch.equal(got["outboards"], d_ob), f"window {w} MiB: the helper's outboard differs"
            del got
            ta, th, tb = [], [], []
            for _ in range(a.host_reps):
                ta.append(wall_ms(lambda: m.bao._pump(_NoKernel(), host, hl, w * MIB, 2)))
                th.append(wall_ms(lambda: m.bao.outboard_stream(ctx, host, hl, w * MIB, 0, ring=2)))
                tb.append(wall_ms(lambda: m.bao._pump(_NoKernel(), host, hl, w * MIB, 2)))
            k = dict(helper=stats(th), a=stats(ta + tb), a_a=stats(ta), a_b=stats(tb))
            # the same from the pinned tensor itself, which the helper copies from where it lies (no host buffers)
            ta, th, tb = [], [], []
            for _ in range(a.host_reps):
                ta.append(wall_ms(lambda: m.bao._pump(_NoKernel(), pinned, hl, w * MIB, 2)))
                th.append(wall_ms(lambda: m.bao.outboard_stream(ctx, pinned, hl, w * MIB, 0, ring=2)))
                tb.append(wall_ms(lambda: m.bao._pump(_NoKernel(), pinned, hl, w * MIB, 2)))
            k["pinned"] = dict(helper=stats(th), a=stats(ta + tb), a_spread_ms=abs(stats(ta)["ms"] - stats(tb)["ms"]))
            k["pinned"]["helper_minus_a_ms"] = k["pinned"]["helper"]["ms"] - k["pinned"]["a"]["ms"]
            k["pinned"]["helper_gb_s"] = hl / k["pinned"]["helper"]["ms"] / 1e6
            k["a_spread_ms"] = abs(k["a_a"]["ms"] - k["a_b"]["ms"])
            k["helper_minus_a_ms"] = k["helper"]["ms"] - k["a"]["ms"]
            k["last_window_kernel_ms"] = res["resident"].get("g0", {}).get("one_push_ms", {}).get(f"{w}MiB")
            if k["last_window_kernel_ms"] is not None:
                k["hidden_behind_the_copy"] = bool(k["helper_minus_a_ms"] <= k["last_window_kernel_ms"] + k["a_spread_ms"])
            k["helper_gb_s"] = hl / k["helper"]["ms"] / 1e6
            hrow[f"window_{w}MiB"] = k
            print(f"host window {w} MiB", json.dumps(k), flush=True)
        res["host"] = hrow
    Y.b3w_destroy(y_ctx)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_stream_measure.json" if not a.quick else "bao_stream_measure_quick.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
