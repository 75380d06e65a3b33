#!/usr/bin/env python3
"""tools/bao_batch_measure.py <out_dir> [--quick] [--shapes a,b,...] — the batch bao calls against the single-file route.

  outboards   for each shape (1 GiB in all): b3w_bao_outboard_batch_device against a loop of b3w_bao_outboard_device over the same
              files, alternating in the same process, device events around each whole route, medians over a window of about a second
              each (a route whose one pass takes longer than that: three passes); every file's root of the two routes compared once
              before timing.  Shapes: 262 144 x 4 KiB, 16 384 x 64 KiB, 1 024 x 1 MiB, 1 x 1 GiB, and `mixed` (lengths log-uniform
              in 1 B ... 64 MiB, fixed seed, until 1 GiB is reached).
  challenges  4 096 samples spread over the 16 384-file batch: one plan_samples_batch call against one plan_samples call per
              distinct file (host clock around each route; both end in a device synchronise).
Writes <out_dir>/bao_batch_measure.json.  --quick: the batch route alone, ten calls a shape and no timing windows — for a run under
`rocprofv3 --kernel-trace --stats`, whose per-kernel call counts divided by ten are the launches of one call."""
import argparse, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

m = __import__("hot-proofs-blake3-circom_amd")

GIB = 1 << 30
QUICK_CALLS = 10


def shapes():
    rng = np.random.default_rng(8)
    mixed, total = [], 0
    while total < GIB:
        ln = int(round(2.0 ** rng.uniform(0, 26)))
        ln = min(ln, GIB - total)
        mixed.append(ln)
        total += ln
    return {"262144x4KiB": [4 << 10] * 262144, "16384x64KiB": [64 << 10] * 16384, "1024x1MiB": [1 << 20] * 1024, "1x1GiB": [GIB],
            "mixed": mixed}


def compressions(lens):
    """block compressions plus parent compressions of these files"""
    ln = np.asarray(lens, dtype=np.int64)
    chunks = np.maximum(1, (ln + 1023) // 1024)
    return int(np.maximum(1, (ln + 63) // 64).sum() + (chunks - 1).sum())


def bound_ms(lens):
    """the bound tools/bao_measure.py uses: the bytes at 8 TB/s, or the compressions at 700 cycles on 256 CUs x 128 lanes at 2.4 GHz"""
    return max(sum(lens) / 8e12, compressions(lens) * 700 / (256 * 128 * 2.4e9)) * 1e3


def one_pass_ms(fn):
    st = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b)


def timed(fn, window_s):
    """per-pass device times (ms) over repeats filling about window_s; at least three passes"""
    out, t0 = [], time.time()
    while len(out) < 3 or time.time() - t0 < window_s:
        out.append(one_pass_ms(fn))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--quick", action="store_true", help="the batch route alone, ten calls a shape (under a profiler)")
    ap.add_argument("--shapes", default="", help="comma-separated subset of the shape names")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    d_arena = torch.randint(0, 256, (GIB + (1 << 20),), dtype=torch.uint8, device="cuda", generator=g)
    res = dict(device=torch.cuda.get_device_name(0), arena_bytes=GIB, shapes={})
    want = [x for x in a.shapes.split(",") if x]
    kept = {}
    for name, lens_l in shapes().items():
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
        ob_first = m.bao.batch_layout(lens)
        d_obs = torch.empty(int(ob_first[-1]), dtype=torch.uint8, device="cuda")
        d_roots = torch.empty((n_files, 8), dtype=torch.int32, device="cuda")
        need = L.b3w_bao_batch_scratch_bytes(lens.ctypes.data, n_files)
        d_scratch = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        base = d_arena.data_ptr()

        def batch():
            rc = L.b3w_bao_outboard_batch_device(ctx.handle, base, offsets.ctypes.data, lens.ctypes.data, n_files, d_obs.data_ptr(),
                                                 d_roots.data_ptr(), d_scratch.data_ptr(), need, s)
            assert rc == 0, ctx.last_error()
        row = dict(n_files=int(n_files), bytes=int(lens.sum()), scratch_bytes=int(need), table_bytes=int(32 * n_files), bound_ms=bound_ms(lens_l))
        if a.quick:
            for _ in range(QUICK_CALLS):
                batch()
            torch.cuda.synchronize()
            row["batch_calls"] = QUICK_CALLS
            res["shapes"][name] = row
            continue
        d_obs1 = torch.empty_like(d_obs)
        d_roots1 = torch.empty_like(d_roots)
        n_max = int(m.bao.num_chunks(int(lens.max())))
        d_levels = torch.empty((2 * n_max + 64) * 8, dtype=torch.int32, device="cuda")
        obs1, roots1, lev = d_obs1.data_ptr(), d_roots1.data_ptr(), d_levels.data_ptr()
        offs, lns, firsts = [int(x) for x in offsets], [int(x) for x in lens], [int(x) for x in ob_first]

        def loop():
            for f in range(n_files):
                rc = L.b3w_bao_outboard_device(ctx.handle, base + offs[f], lns[f], obs1 + firsts[f], lev, roots1 + 32 * f, s)
                assert rc == 0, ctx.last_error()
        batch()
        t_first_loop = one_pass_ms(loop)                                          # (also the loop's warm-up)
        torch.cuda.synchronize()
        assert torch.equal(d_roots, d_roots1), f"{name}: the roots of the two routes differ"
        row["outboards_equal"] = bool(torch.equal(d_obs, d_obs1))
        assert row["outboards_equal"], f"{name}: the outboards of the two routes differ"
        for _ in range(3):
            batch()
        if t_first_loop < 300:
            loop()
            loop()
        t_batch, t_loop = [], []
        for _ in range(3):                                                        # alternating, a third of the window each time
            t_batch += timed(batch, 1.0 / 3)
            t_loop += timed(loop, 1.0 / 3) if t_first_loop < 300 else [one_pass_ms(loop)]
        row.update(batch_ms=float(np.median(t_batch)), batch_min_ms=float(np.min(t_batch)), batch_max_ms=float(np.max(t_batch)), batch_reps=len(t_batch),
                   loop_ms=float(np.median(t_loop)), loop_min_ms=float(np.min(t_loop)), loop_reps=len(t_loop))
        row["ratio_loop_over_batch"] = row["loop_ms"] / row["batch_ms"]
        row["fraction_of_bound"] = row["bound_ms"] / row["batch_ms"]
        res["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
        if name == "16384x64KiB":
            kept = dict(lens=lens, offsets=offsets, obs=d_obs.clone(), roots=d_roots.clone(), ob_first=ob_first)
        del d_obs1, d_roots1, d_levels
    if kept and not a.quick:
        # ---- challenges over the 16 384-file batch
        rng = np.random.default_rng(7)
        K = 4096
        files = rng.integers(0, kept["lens"].size, K).astype(np.uint32)
        chunks = rng.integers(0, 64, K).astype(np.uint64)
        cb = m.bao.chunk_bytes_batch(d_arena, kept["offsets"], kept["lens"], files, chunks)
        roots_h = kept["roots"].cpu().numpy().view(np.uint32)
        order = np.argsort(files, kind="stable")
        per_file = []
        for f in np.unique(files):
            idx = order[np.searchsorted(files[order], f, "left"):np.searchsorted(files[order], f, "right")]
            a0, b0 = int(kept["ob_first"][f]), int(kept["ob_first"][f + 1])
            per_file.append((kept["obs"][a0:b0], int(kept["lens"][f]), roots_h[f], chunks[idx], cb[torch.from_numpy(idx).cuda()].contiguous()))

        def plan_batch():
            t = time.perf_counter()
            out = m.bao.plan_samples_batch(ctx, kept["obs"], kept["lens"], kept["roots"], files, chunks, cb)
            assert (out["sample_status"] == 0).all()
            return (time.perf_counter() - t) * 1e3

        def plan_loop():
            t = time.perf_counter()
            for ob_f, ln, root, ch, cbf in per_file:
                out = m.bao.plan_samples(ctx, ob_f, ln, root, ch, cbf)
                assert (out["sample_status"] == 0).all()
            return (time.perf_counter() - t) * 1e3
        plan_batch()
        plan_loop()
        tb, tl = [], []
        for _ in range(5):
            tb.append(plan_batch())
            tl.append(plan_loop())
        res["challenges"] = dict(samples=K, distinct_files=len(per_file), plan_samples_batch_wall_ms=float(np.median(tb)),
                                 plan_samples_per_file_wall_ms=float(np.median(tl)), ratio=float(np.median(tl) / np.median(tb)))
        print("challenges", json.dumps(res["challenges"]), flush=True)
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_batch_measure.json" if not a.quick else "bao_batch_measure_quick.json"), "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
