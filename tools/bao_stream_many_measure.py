#!/usr/bin/env python3
"""tools/bao_stream_many_measure.py <out_dir> --parent-lib libb3wit.so [--quick] [--sessions 16,64,256] [--windows 1,4]
[--group-logs 0,4] [--kinds outboard,verify] [--no-host] — many stream sessions in one launch (b3w_bao_stream_push_many /
_finish_many) against the per-session calls.  Needs a GPU; there is no fall-back.

  resident   K sessions of 64 MiB each, their bytes resident, windows of 1 and 4 MiB, outboard and verify kinds, g = 0 and 4.  Routes,
             alternating in one process, device events around each whole route (begin and free of every session included), medians
             over about a second a route:
               a  the loop of b3w_bao_stream_push / _finish of the library given with --parent-lib (a build of the commit before,
                  loaded beside this one, its own context) on one stream, round by round
               b  the same loop spread over 4 streams (session i on stream i mod 4; the timed stream waits for all four)
               c  one b3w_bao_stream_push_many a round and one b3w_bao_stream_finish_many
             a and b each run as two interleaved series; |median of one - median of the other| is that route's spread.  The claim:
             c beats the faster of a and b by more than that route's spread, on every shape (`claim_holds`).  Reported beside it, not
             gated: the batch call on the same bytes (the ceiling) and 64 one-entry push_many calls against 64 push calls (the table's
             cost).  Results are compared with the batch call's once before timing.
  host       64 files of 64 MiB in pinned host memory: bao.outboard_stream_many at three window_bytes x lanes settings against
             bao.outboard_stream file after file (two series), wall time, each route ending in a synchronise.
Writes <out_dir>/bao_stream_many_measure.json.  --quick: ten passes of routes a and c at 16 sessions and 1 MiB windows (g = 0 and 4,
both kinds) and nothing timed — for a run under `rocprofv3 --kernel-trace --stats`: a kernel's calls / 10 are its launches a pass."""
import argparse, ctypes, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bao_batch_measure as BM
from bao_groups_measure import stats

m = __import__("hot-proofs-blake3-circom_amd")

MIB = 1 << 20
FILE = 64 * MIB
QUICK_PASSES = 10
HOST_SETTINGS = [(1, 64), (4, 16), (16, 4)]                # (window MiB, lanes): 64 MiB a round each


def parent_library(path):
    """the yardstick library and a nova_vesta context of its own -> (lib, ctx handle)"""
    vp, u32, i32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64
    P = ctypes.CDLL(path)
    P.b3w_abi_version.restype = u32
    P.b3w_create.restype, P.b3w_create.argtypes = i32, [i32, i32, ctypes.POINTER(vp)]
    P.b3w_destroy.restype, P.b3w_destroy.argtypes = None, [vp]
    P.b3w_bao_stream_outboard_begin.restype, P.b3w_bao_stream_outboard_begin.argtypes = i32, [vp, u64, u32, vp, vp, vp, u64, ctypes.POINTER(vp)]
    P.b3w_bao_stream_verify_begin.restype, P.b3w_bao_stream_verify_begin.argtypes = i32, [vp, u64, u32, vp, vp, vp, vp, vp, vp, u64, vp, ctypes.POINTER(vp)]
    P.b3w_bao_stream_push.restype, P.b3w_bao_stream_push.argtypes = i32, [vp, u64, vp, u64, vp]
    P.b3w_bao_stream_finish.restype, P.b3w_bao_stream_finish.argtypes = i32, [vp, vp]
    P.b3w_bao_stream_free.restype, P.b3w_bao_stream_free.argtypes = None, [vp]
    h = vp()
    rc = P.b3w_create(m.CIRCUIT_ID["nova_vesta"], 0, ctypes.byref(h))
    assert rc == 0, rc
    return P, h


def alternating(routes, window_s=1.0, rounds=3):
    """{name: fn} -> {name: [ms, ...]}: the routes one after the other, `rounds` times, each turn about window_s / rounds long and
    at least one pass (a pass of route a over 256 sessions takes seconds)"""
    out = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            t0 = time.time()
            while True:
                out[k].append(BM.one_pass_ms(fn))
                if time.time() - t0 >= window_s / rounds:
                    break
    return out


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--parent-lib", required=True, help="libb3wit.so built from the commit before push_many: the yardstick")
    ap.add_argument("--quick", action="store_true", help="ten passes of routes a and c at 16 sessions (under a profiler)")
    ap.add_argument("--sessions", default="16,64,256")
    ap.add_argument("--windows", default="1,4")
    ap.add_argument("--group-logs", default="0,4")
    ap.add_argument("--kinds", default="outboard,verify")
    ap.add_argument("--host-files", type=int, default=64)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-resident", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bao_stream_many_measure: no GPU")
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    Y, y_ctx = parent_library(a.parent_lib)
    cur = torch.cuda.current_stream()
    s = cur.cuda_stream
    sides = [torch.cuda.Stream() for _ in range(4)]
    ks = [16] if a.quick else [int(x) for x in a.sessions.split(",")]
    windows = [1] if a.quick else [int(x) for x in a.windows.split(",")]
    kmax = max(ks)
    res = dict(device=torch.cuda.get_device_name(0), file_bytes=FILE, parent=f"{os.path.basename(a.parent_lib)} (ABI {Y.b3w_abi_version() >> 16}.{Y.b3w_abi_version() & 0xffff})",
               resident={}, host={})
    if not a.no_resident:
        gen = torch.Generator(device="cuda").manual_seed(1)
        arena = torch.randint(0, 256, (kmax * FILE,), dtype=torch.uint8, device="cuda", generator=gen)
        base = arena.data_ptr()
        need = {"outboard": L.b3w_bao_stream_scratch_bytes(FILE, 0), "verify": L.b3w_bao_stream_scratch_bytes(FILE, 1)}
    for gl in ([] if a.no_resident else [int(x) for x in a.group_logs.split(",")]):
        lens = [FILE] * kmax
        offs = [i * FILE for i in range(kmax)]
        want = m.bao.outboard_batch(ctx, arena, offs, lens) if gl == 0 else m.bao.outboard_groups_batch(ctx, arena, offs, lens, gl)
        ob_first = [int(x) for x in want["ob_first"]]
        units = int(m.bao.verify_layout([FILE], gl)[-1])
        obs = torch.empty_like(want["outboards"])
        roots = torch.empty_like(want["roots"])
        scr = torch.empty((kmax, max(need.values())), dtype=torch.uint8, device="cuda")
        d_st = torch.empty((kmax, units), dtype=torch.uint8, device="cuda")
        d_fs, d_fb = torch.empty(kmax, dtype=torch.int32, device="cuda"), torch.empty(kmax, dtype=torch.int64, device="cuda")
        for kind in a.kinds.split(","):
            for k in ks:
                def begin(lib, c, i, stream):
                    h = ctypes.c_void_p()
                    if kind == "outboard":
                        rc = lib.b3w_bao_stream_outboard_begin(c, FILE, gl, obs.data_ptr() + ob_first[i], roots[i].data_ptr(), scr[i].data_ptr(), need[kind], ctypes.byref(h))
                    else:
                        rc = lib.b3w_bao_stream_verify_begin(c, FILE, gl, want["outboards"].data_ptr() + ob_first[i], want["roots"][i].data_ptr(), d_st[i].data_ptr(),
                                                             d_fs[i:].data_ptr(), d_fb[i:].data_ptr(), scr[i].data_ptr(), need[kind], stream, ctypes.byref(h))
                    assert rc == 0, rc
                    return h

                def per_session(window, streams):
                    """routes a (streams = [s]) and b (the four side streams): the parent's push / finish loop"""
                    if len(streams) > 1:
                        for st in sides:
                            st.wait_stream(cur)
                    hs = [begin(Y, y_ctx, i, streams[i % len(streams)]) for i in range(k)]
                    for off in range(0, FILE, window):
                        for i in range(k):
                            assert Y.b3w_bao_stream_push(hs[i], off, base + offs[i] + off, window, streams[i % len(streams)]) == 0
                    for i in range(k):
                        assert Y.b3w_bao_stream_finish(hs[i], streams[i % len(streams)]) == 0
                        Y.b3w_bao_stream_free(hs[i])
                    if len(streams) > 1:
                        for st in sides:
                            cur.wait_stream(st)

                def many(window):
                    hs = [begin(L, ctx.handle, i, s) for i in range(k)]
                    h_arr = np.array([h.value for h in hs], dtype=np.uint64)
                    nb = np.full(k, window, dtype=np.uint64)
                    for off in range(0, FILE, window):
                        o = np.full(k, off, dtype=np.uint64)
                        p = np.array([base + offs[i] + off for i in range(k)], dtype=np.uint64)
                        assert L.b3w_bao_stream_push_many(ctx.handle, h_arr.ctypes.data, o.ctypes.data, p.ctypes.data, nb.ctypes.data, k, s) == 0, ctx.last_error()
                    assert L.b3w_bao_stream_finish_many(ctx.handle, h_arr.ctypes.data, k, s) == 0, ctx.last_error()
                    for h in hs:
                        L.b3w_bao_stream_free(h)

                def batch():
                    if kind == "verify":
                        m.bao.verify_batch(ctx, arena, offs[:k], lens[:k], want["outboards"], want["roots"], gl)
                    elif gl == 0:
                        m.bao.outboard_batch(ctx, arena, offs[:k], lens[:k])
                    else:
                        m.bao.outboard_groups_batch(ctx, arena, offs[:k], lens[:k], gl)
                # c's results against the batch call's, once
                obs.zero_()
                d_st.fill_(0xEE)
                many(MIB)
                torch.cuda.synchronize()
                if kind == "outboard":
                    assert torch.equal(obs[:ob_first[k]], want["outboards"][:ob_first[k]]) and torch.equal(roots[:k], want["roots"][:k]), f"g = {gl}, {k} sessions: outboards differ"
                else:
                    assert not d_st[:k].any().item() and not d_fs[:k].any().item(), f"g = {gl}, {k} sessions: verification differs"
                for w in windows:
                    name = f"g{gl}_{kind}_k{k}_w{w}"
                    if a.quick:
                        for fn in (lambda: per_session(w * MIB, [s]), lambda: many(w * MIB)):
                            for _ in range(QUICK_PASSES):
                                fn()
                            torch.cuda.synchronize()
                        res["resident"][name] = dict(passes_each=QUICK_PASSES, sessions=k, window_mib=w, rounds=FILE // (w * MIB))
                        continue
                    side_streams = [st.cuda_stream for st in sides]
                    routes = {"a_1": lambda: per_session(w * MIB, [s]), "b_1": lambda: per_session(w * MIB, side_streams), "c": lambda: many(w * MIB),
                              "batch": batch, "a_2": lambda: per_session(w * MIB, [s]), "b_2": lambda: per_session(w * MIB, side_streams)}
                    for fn in routes.values():
                        fn()
                    t = alternating(routes)
                    row = dict(group_log=gl, kind=kind, sessions=k, window_mib=w, rounds=FILE // (w * MIB), bytes=k * FILE)
                    for r in ("a", "b"):
                        row[r] = stats(t[f"{r}_1"] + t[f"{r}_2"])
                        row[r]["spread_ms"] = abs(stats(t[f"{r}_1"])["ms"] - stats(t[f"{r}_2"])["ms"])
                    row["c"], row["batch"] = stats(t["c"]), stats(t["batch"])
                    best = "a" if row["a"]["ms"] <= row["b"]["ms"] else "b"
                    row.update(faster_of_a_b=best, c_gain_ms=row[best]["ms"] - row["c"]["ms"], c_speedup=row[best]["ms"] / row["c"]["ms"],
                               claim_holds=bool(row[best]["ms"] - row["c"]["ms"] > row[best]["spread_ms"]), c_over_batch=row["c"]["ms"] / row["batch"]["ms"],
                               c_gb_s=k * FILE / row["c"]["ms"] / 1e6)
                    res["resident"][name] = row
                    print(name, json.dumps(row), flush=True)
            if a.quick:
                continue
            # the table's cost: one session's 64 pushes of 1 MiB against 64 one-entry push_many calls
            k = 1

            def single(many_call):
                h = begin(L, ctx.handle, 0, s)
                ha, nb = np.array([h.value], dtype=np.uint64), np.array([MIB], dtype=np.uint64)
                for off in range(0, FILE, MIB):
                    if many_call:
                        o, p = np.array([off], dtype=np.uint64), np.array([base + off], dtype=np.uint64)
                        assert L.b3w_bao_stream_push_many(ctx.handle, ha.ctypes.data, o.ctypes.data, p.ctypes.data, nb.ctypes.data, 1, s) == 0
                    else:
                        assert L.b3w_bao_stream_push(h, off, base + off, MIB, s) == 0
                L.b3w_bao_stream_free(h)
            t = alternating({"push": lambda: single(False), "push_many": lambda: single(True)})
            one = dict(push=stats(t["push"]), push_many_of_one=stats(t["push_many"]))
            one["table_cost_us_a_call"] = (one["push_many_of_one"]["ms"] - one["push"]["ms"]) * 1e3 / (FILE // MIB)
            res["resident"][f"g{gl}_{kind}_one_entry"] = one
            print(f"g{gl}_{kind}_one_entry", json.dumps(one), flush=True)
    if not a.quick and not a.no_host:
        n = a.host_files
        pinned = [torch.empty(FILE, dtype=torch.uint8, pin_memory=True) for _ in range(n)]
        rng = np.random.default_rng(5)
        for p in pinned:
            p.numpy()[:] = rng.integers(0, 256, FILE, dtype=np.uint8)
        lens = [FILE] * n

        def one_by_one():
            for p in pinned:
                m.bao.outboard_stream(ctx, p, FILE, 64 * MIB, 0, ring=2)
        want = [m.bao.outboard_stream(ctx, p, FILE, 64 * MIB, 0, ring=2)["roots"].clone() for p in pinned[:4]]
        hrow = dict(files=n, file_bytes=FILE, ring=2, reps=a.host_reps, settings={})
        t1, t2, tm = [], [], {f"w{w}_l{l}": [] for w, l in HOST_SETTINGS}
        for w, l in HOST_SETTINGS:
            got = m.bao.outboard_stream_many(ctx, pinned, lens, w * MIB, 0, lanes=l, ring=2)
            torch.cuda.synchronize()
            assert all(torch.equal(got["roots"][i], want[i][0]) for i in range(4)), f"window {w} MiB x {l} lanes: roots differ"
            del got
        for _ in range(a.host_reps):
            t1.append(wall_ms(one_by_one))
            for w, l in HOST_SETTINGS:
                tm[f"w{w}_l{l}"].append(wall_ms(lambda: m.bao.outboard_stream_many(ctx, pinned, lens, w * MIB, 0, lanes=l, ring=2)))
            t2.append(wall_ms(one_by_one))
        hrow["one_by_one"] = stats(t1 + t2)
        hrow["one_by_one"]["spread_ms"] = abs(stats(t1)["ms"] - stats(t2)["ms"])
        for key, ts in tm.items():
            st = stats(ts)
            st.update(gb_s=n * FILE / st["ms"] / 1e6, gain_ms=hrow["one_by_one"]["ms"] - st["ms"])
            hrow["settings"][key] = st
        res["host"] = hrow
        print("host", json.dumps(hrow), flush=True)
    Y.b3w_destroy(y_ctx)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_stream_many_measure.json" if not a.quick else "bao_stream_many_measure_quick.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
