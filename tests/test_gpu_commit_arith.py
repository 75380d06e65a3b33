"""The commit kernels (csrc/b3w_commit.hip) end to end where the arithmetic's exceptional cases meet: the point at infinity AMONG
finite sums, in keys that commit a handful of bit slots, two of them to +G and -G.  (The routines themselves, at the operands where
carries and lazy bounds can go wrong: tests/test_commit_arith_cpu.py.)"""
import random

import numpy as np
import pytest

import b3w_testlib as T
import ec_ref as E

pytestmark = pytest.mark.gpu


def _norm_groups(n_leaf, n_par):
    """the witnesses that share an inversion in b3w_commit_normalize_many_kernel: a commit-only pass normalises once per run call
    (the leaf steps, then the parent steps), four consecutive witnesses of the call a thread"""
    g = [list(range(a, min(a + 4, n_leaf))) for a in range(0, n_leaf, 4)]
    return g + [list(range(a, min(a + 4, n_leaf + n_par))) for a in range(n_leaf, n_leaf + n_par, 4)]


def _patterns(inf, groups):
    """which of the shapes the issue asks for the full groups show"""
    seen = set()
    for g in groups:
        if len(g) < 4:
            continue
        pat = tuple(bool(inf[w]) for w in g)
        if pat == (True, False, False, False):
            seen.add("first")
        if pat == (False, False, False, True):
            seen.add("last")
        if pat in ((False, True, False, False), (False, False, True, False)):
            seen.add("middle")
        if sum(pat) == 3:
            seen.add("three of four")
    return seen


WANTED = {"first", "last", "middle", "three of four"}


def _choose_slots(bits, groups, rng):
    """bits: bool [witnesses, slots] of the oracle's bodies.  Slots A, B, C for the generators +G, -G, H such that the commitments
    A G - B G + C H are infinity in all the wanted shapes, some by having nothing to add and some by G - G."""
    varying = np.flatnonzero(bits.any(axis=0) & ~bits.all(axis=0))
    _, first = np.unique(bits[:, varying], axis=1, return_index=True)          # one slot per distinct column
    cand = varying[np.sort(first)].tolist()
    for _ in range(200_000):
        a, b, c = rng.sample(cand, 3)
        A_, B_, C_ = bits[:, a], bits[:, b], bits[:, c]
        empty, cancel = ~A_ & ~B_ & ~C_, A_ & B_ & ~C_
        if empty.any() and cancel.any() and _patterns(empty | cancel, groups) == WANTED:
            return a, b, c
    raise AssertionError("no three bit slots of these bodies give the wanted shapes")


@pytest.mark.parametrize("circuit,curve", [("nova_vesta", "vesta"), ("nova_bn254", "bn254_g1")])
@pytest.mark.parametrize("window", [12, 16])
def test_infinity_among_finite_sums(circuit, curve, window):
    """Today a pass is all finite or all infinite.  Here the key's generators are (0, 0) but for three bit slots with +G, -G and H,
    chosen from the oracle's bodies of the pass's own steps so that the witnesses of a group of four that shares an inversion
    (b3w_commit_normalize_many_kernel) are infinite first, last, in the middle, and three of four — by an empty sum and by G - G, which
    the commit kernel meets in its table, in j9_madd or in its LDS tree and carries as ZZ = 0.  The commit-only pass, commit_records
    and commit_device on the bodies all give ec_ref.commit's points, (0, 0) for infinity.
    (What this test found: b3w_commit_window_kernel handed (0, 0) generators to j9_madd, which leaves that filter to its caller, so
    every table entry that combined a finite point with a (0, 0) one was off the curve — on all three paths alike.  An all-(0, 0) key
    hid it: (0, 0) + (0, 0) takes the P + P branch, Y = 0 there makes it infinity, and a lone (0, 0) normalises to (0, 0).)
    (An inverse update of normalize_many in the wrong order — `inv` multiplied by A_e before 1 / A_e is taken from it — makes 1 / A_e
    = 1 for every finite witness behind the first of its group; every wanted shape but "last" has such a witness, so the comparison
    with ec_ref.commit below fails on it.)"""
    import torch
    m = T.pkg()
    p = E.CURVES[curve][0]
    ctx = m.Context(circuit, 0)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    data = ((np.arange(2 * 1024 + 100, dtype=np.uint64) * 2654435761 + 5) % 251).astype(np.uint8)      # 16 + 16 + 2 leaf steps
    probe = m.chain.fold_witnesses(ctx, data, batch_steps=7, ring=2)            # the pass's own step records
    torch.cuda.synchronize()
    n_leaf, n_par = probe["n_leaf_steps"], probe["n_parent_steps"]
    rows = n_leaf + n_par
    assert n_leaf == 34 and int(probe["status"].abs().sum().item()) == 0
    recs = probe["records"].cpu().numpy().astype(np.uint32)
    assert recs.shape[0] == rows
    bad, bodies = T.oracle_batch_u32(circuit, recs)
    assert bad == 0
    slots = bodies.reshape(rows, -1, 32)
    small = (slots[:, :, 1:] == 0).all(axis=2) & (slots[:, :, 0] <= 1)          # the witness holds 0 or 1 there
    bits = (slots[:, :, 0] == 1) & small.all(axis=0)[None, :]                   # ... in every step: bit slots (or words that hold a bit)
    groups = _norm_groups(n_leaf, n_par)
    a, b, c = _choose_slots(bits, groups, random.Random(window * 1000 + len(circuit)))
    G, H = E.random_points(curve, 2, seed=b"b3wit-infinity-among-finite")
    gens = [None] * T.NWIT[circuit]
    gens[a], gens[b], gens[c] = G, E.neg(G, p), H
    want = [E.commit([int(bits[w, a]), int(bits[w, b]), int(bits[w, c])], [gens[a], gens[b], gens[c]], curve) for w in range(rows)]
    inf = [P is None for P in want]
    # ... the shapes, from the oracle's bodies, before trusting the run
    assert _patterns(inf, groups) == WANTED, (a, b, c, inf)
    assert any(bits[w, a] and bits[w, b] and inf[w] for w in range(rows)) and any(not (bits[w, a] or bits[w, b] or bits[w, c]) for w in range(rows))
    assert 0 < sum(inf) < rows and all(E.on_curve(P, curve) for P in want)
    want_bytes = np.frombuffer(E.points_to_bytes(want), dtype=np.uint8).reshape(rows, 64)

    key = m.CommitKey(ctx, curve, E.points_to_bytes(gens), window=window)
    pts = torch.full((rows, 64), 0xAB, dtype=torch.uint8, device=dev)
    out = m.chain.fold_witnesses(ctx, data, batch_steps=7, ring=2, commit_only=(key, pts))
    torch.cuda.synchronize()
    assert int(out["status"].abs().sum().item()) == 0
    assert np.array_equal(out["records"].cpu().numpy().astype(np.uint32), recs)
    got = pts.cpu().numpy()
    wrong = [w for w in range(rows) if not np.array_equal(got[w], want_bytes[w])]
    assert not wrong, f"commit-only pass: witnesses {wrong} (infinite: {[w for w in range(rows) if inf[w]]})"
    hpts, _, hst = key.commit_records(recs)                                     # normalises witness by witness
    assert int(np.abs(hst).sum()) == 0 and np.array_equal(hpts, want_bytes), "commit_records"
    d_recs = torch.from_numpy(recs.view(np.int32)).to(dev)
    d_bodies = torch.zeros((rows, ctx.body_bytes), dtype=torch.uint8, device=dev)
    d_st = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    ctx.run_device(d_recs.data_ptr(), rows, d_bodies.data_ptr(), 0, 0, d_st.data_ptr(), s)
    bpts = torch.full((rows, 64), 0xAB, dtype=torch.uint8, device=dev)
    cst = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    key.commit_device(d_bodies.data_ptr(), rows, 0, bpts.data_ptr(), cst.data_ptr(), s)
    torch.cuda.synchronize()
    assert int(d_st.abs().sum().item()) == 0 and int(cst.abs().sum().item()) == 0
    assert np.array_equal(d_bodies.cpu().numpy()[:, :bodies.shape[1]], bodies), "the bodies are not the oracle's"
    assert np.array_equal(bpts.cpu().numpy(), want_bytes), "commit_device on the bodies"
    key.close(); ctx.close()
