#!/usr/bin/env python3
"""tools/bao_measure.py <out_dir> [--mib 1024] [--quick] [--chain-pass] — timings of the bao route on a device-resident preimage.

  outboard   b3w_bao_outboard_device (chunk CVs + tree + pre-order emission) against the route that existed before it
             (b3w_chain_plan_leaves_device over every chunk + b3w_chain_tree_device), alternating in the same process, device events,
             warm-up, repeats for a window of about 1 s each; both lane shapes of the chunk-CV kernel (B3W_BAO_QUAD=0 / 1)
  challenge  K = 64 and 4 096 random chunks: planning only (b3w_sample_plan_device), planning + commitments from the records (no
             bodies), planning + witnesses + commitments (bodies through one 4 096-step buffer)
  chain      (--chain-pass) the whole-preimage chained pass with commitments from records (chain.fold_witnesses(commit_only=...))
Writes <out_dir>/bao_measure.json.  Kernel times: run under `rocprofv3 --kernel-trace --stats` with --quick."""
import argparse, ctypes, json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

m = __import__("hot-proofs-blake3-circom_amd")


def timed(fn, window_s, min_reps=5):
    """median and min of per-call device time (ms) over repeats filling about window_s"""
    st = torch.cuda.current_stream()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out, t0 = [], time.time()
    while len(out) < min_reps or time.time() - t0 < window_s:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(out)), min_ms=float(np.min(out)), reps=len(out))


def sclk():
    """the shader clock the driver reports right now (read only)"""
    try:
        txt = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=20).stdout
        return [l.strip() for l in txt.splitlines() if "sclk" in l.lower()][:2]
    except Exception as e:                                  # (not every image has rocm-smi on PATH)
        return [f"unavailable: {e}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--quick", action="store_true", help="short windows (under a profiler)")
    ap.add_argument("--chain-pass", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    win = 0.2 if a.quick else 1.0
    L = m.lib()
    ctx = m.Context("nova_vesta", 0)
    length = a.mib << 20
    n = m.bao.num_chunks(length)
    g = torch.Generator(device="cuda").manual_seed(1)
    d_pre = torch.randint(0, 256, (length,), dtype=torch.uint8, device="cuda", generator=g)
    ob = torch.empty(L.b3w_bao_outboard_size(length), dtype=torch.uint8, device="cuda")
    levels = torch.empty((2 * n + 64) * 8, dtype=torch.int32, device="cuda")
    root = torch.empty(8, dtype=torch.int32, device="cuda")
    recs = torch.empty((n * 16, 32), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    res = dict(preimage_bytes=length, n_chunks=n, device=torch.cuda.get_device_name(0))

    def new_route():
        rc = L.b3w_bao_outboard_device(ctx.handle, d_pre.data_ptr(), length, ob.data_ptr(), levels.data_ptr(), root.data_ptr(), s)
        assert rc == 0, ctx.last_error()

    def old_route():
        rc = L.b3w_chain_plan_leaves_device(ctx.handle, d_pre.data_ptr(), length, 0, n, recs.data_ptr(), levels.data_ptr(), s)
        rc = rc or L.b3w_chain_tree_device(ctx.handle, levels.data_ptr(), n, root.data_ptr(), s)
        assert rc == 0, ctx.last_error()

    rounds = {}
    for r in range(3):                                      # alternating: new (default shape), old, new with the other lane shape
        for name, fn, env in (("outboard", new_route, None), ("plan_leaves_plus_tree", old_route, None),
                              ("outboard_other_shape", new_route, "1" if n > 65536 else "0")):
            if env is None:
                os.environ.pop("B3W_BAO_QUAD", None)
            else:
                os.environ["B3W_BAO_QUAD"] = env
            rounds.setdefault(name, []).append(timed(fn, win / 3))
    os.environ.pop("B3W_BAO_QUAD", None)
    res["outboard_ms"] = {k: dict(median_ms=float(np.median([x["median_ms"] for x in v])), min_ms=float(min(x["min_ms"] for x in v)),
                                  reps=sum(x["reps"] for x in v)) for k, v in rounds.items()}
    res["sclk_after_outboard_loop"] = sclk()
    bound_ms = max(length / 8e12 * 1e3, (length / 64) * 700 / (256 * 128 * 2.4e9) * 1e3)
    res["reference_bound_ms"] = bound_ms
    res["fraction_of_bound"] = bound_ms / res["outboard_ms"]["outboard"]["median_ms"]
    res["speedup_vs_old_route"] = res["outboard_ms"]["plan_leaves_plus_tree"]["median_ms"] / res["outboard_ms"]["outboard"]["median_ms"]
    # the outboard is right: root = BLAKE3 via the chain's tree, and a few slices decode
    new_route()
    torch.cuda.synchronize()
    ob_np, root_np = ob.cpu().numpy(), root.cpu().numpy().view(np.uint32)
    import bao_ref as R
    for c in [0, n // 2, n - 1]:
        chunk = d_pre[c * 1024:(c + 1) * 1024].cpu().numpy().tobytes()
        sl = m.bao.slice_chunk(ob_np, length, c, chunk)
        assert R.decode_slice(sl, c, list(root_np)) == chunk
    del recs
    torch.cuda.empty_cache()

    # ---- challenges
    import ec_ref as E
    key = m.CommitKey(ctx, "pallas", E.points_to_bytes(E.random_points("pallas", ctx.witness_size)), window=12)
    rng = np.random.default_rng(7)
    res["challenge"] = {}
    for K in (64, 4096):
        chunks = rng.integers(0, n, K).astype(np.uint64)
        idx = torch.from_numpy(chunks.astype(np.int64)).cuda()
        cb = d_pre.view(-1, 1024)[idx].contiguous() if length % 1024 == 0 else m.bao.chunk_bytes(d_pre, chunks)
        rf = m.bao.sample_rows(length, chunks)
        rows = int(rf[-1])
        d_recs = torch.empty((rows, 32), dtype=torch.int32, device="cuda")
        d_st = torch.empty(K, dtype=torch.int32, device="cuda")
        rw = np.ascontiguousarray(root_np)

        def plan():
            rc = L.b3w_sample_plan_device(ctx.handle, length, ob.data_ptr(), rw.ctypes.data, chunks.ctypes.data, K, cb.data_ptr(),
                                          d_recs.data_ptr(), d_st.data_ptr(), s)
            assert rc == 0, ctx.last_error()
        t_plan = timed(plan, win)
        assert (d_st.cpu().numpy() == 0).all()
        for _ in range(2):                                  # (the second call: the first one allocates and builds)
            t0 = time.time()
            out = m.bao.prove_samples(ctx, ob, length, root_np, chunks, cb, commit_key=key)
            t_commit = time.time() - t0
        for _ in range(2):
            t0 = time.time()
            out2 = m.bao.prove_samples(ctx, ob, length, root_np, chunks, cb, commit_key=key, consumer=lambda *x: None)
            t_wit = time.time() - t0
        assert (out["status"] == 0).all().item() and torch.equal(out["points"], out2["points"])
        res["challenge"][str(K)] = dict(rows=rows, plan_device_ms=t_plan, plan_plus_commit_from_records_wall_s=t_commit,
                                        plan_plus_witnesses_plus_commit_wall_s=t_wit,
                                        provable=int(out["provable"].sum()))
    if a.chain_pass:
        d_points = torch.empty(((L.b3w_chain_num_leaf_steps(length) + L.b3w_chain_num_parent_steps(length, 0, n)), 64), dtype=torch.uint8, device="cuda")
        host_pre = d_pre.cpu().pin_memory()
        del d_pre
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        t0 = time.time()
        out = m.chain.fold_witnesses(ctx, host_pre, commit_only=(key, d_points))
        torch.cuda.synchronize()
        dt = time.time() - t0
        steps = out["n_leaf_steps"] + out["n_parent_steps"]
        res["chain_pass_commit_only"] = dict(wall_s=dt, steps=int(steps), steps_per_s=steps / dt)
    key.close()
    ctx.close()
    json.dump(res, open(os.path.join(a.out_dir, "bao_measure.json"), "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
