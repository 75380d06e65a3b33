"""The record-domain table (tests/record_domain_cases.py) is what it claims to be: the oracle accepts and rejects its rows as
labelled for all four builds, the closed-form rule agrees with the hand-written labels, the oracle's public outputs equal the
independent numpy models, the listed edges all occur, and the oracle's bodies satisfy the circuits' rank-1 constraints.  No GPU."""
import numpy as np
import pytest

import b3w_testlib as T
import r1cs_ref as R
import record_domain_cases as C
from ref_models import _blake3_compress_np, _nova_public_np

NOVA = T.CIRCUITS[1:]
M = C.M


@pytest.fixture(scope="module")
def nova():
    return C.stack(C.nova_rows())


@pytest.fixture(scope="module")
def comp():
    return C.stack(C.compression_rows())


@pytest.fixture(scope="module")
def oracle_out(nova, comp):
    """{circuit: (rc per row, bodies)} — every row of the table through every build, once"""
    return {c: T.oracle_each_u32(c, (comp if c == "compression" else nova)[1]) for c in T.CIRCUITS}


def _upper_bytes_zero(bodies, first, count):
    return not bodies.reshape(bodies.shape[0], -1, 32)[:, first:first + count, 4:].any()


def test_table_shape_and_labels(nova, comp):
    names, recs, exp = nova
    assert recs.shape[1] == 32 and recs.dtype == np.uint32 and 100 <= len(names)
    assert set(exp) == {"ok", "assert", "domain"}
    assert exp.count("domain") >= 8 and exp.count("assert") >= 8
    for name, rec, e in zip(names, recs, exp):
        assert C.classify(rec) == e, name                                   # the closed-form rule against the hand-written label
        assert name.endswith("/parent") == C.is_parent(rec) or e == "assert", name
    cn, crecs, cexp = comp
    assert crecs.shape[1] == 28 and 40 <= len(cn) <= 60 and set(cexp) == {"ok"}
    # the table is fixed: building it twice gives the same bytes
    assert np.array_equal(C.stack(C.nova_rows())[1], recs) and np.array_equal(C.stack(C.compression_rows())[1], crecs)


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_oracle_verdict_of_every_row(circuit, nova, comp, oracle_out):
    names, recs, exp = comp if circuit == "compression" else nova
    rc, bodies = oracle_out[circuit]
    assert rc.shape[0] == len(names)                                        # no row is left out for any build
    for i, name in enumerate(names):
        assert rc[i] == (4 if exp[i] == "assert" else 0), (circuit, name, int(rc[i]))
    acc = np.flatnonzero(rc == 0)
    assert (bodies[acc, 0] == 1).all() and not bodies[acc, 1:32].any()      # slot 0 is the constant 1


def test_compression_public_outputs_equal_plain_blake3(comp, oracle_out):
    names, recs, _ = comp
    rc, bodies = oracle_out["compression"]
    want = _blake3_compress_np(recs[:, 0:8], recs[:, 8:24], recs[:, 24], recs[:, 25], recs[:, 26], recs[:, 27])
    got = bodies.reshape(len(names), -1, 32)[:, 1:17, :4].copy().view(np.uint32).reshape(len(names), 16)
    for i, name in enumerate(names):
        assert np.array_equal(got[i], want[i]), name
    assert _upper_bytes_zero(bodies, 1, 16)


@pytest.mark.parametrize("circuit", NOVA)
def test_nova_public_outputs_equal_the_model(circuit, nova, oracle_out):
    """Low words of w[1..15] for every accepted row ("domain" rows too: their block_count_out wraps in the model and is 2^32 in
    the oracle's field element); for "ok" rows the 15 outputs are plain words."""
    names, recs, exp = nova
    rc, bodies = oracle_out[circuit]
    want = _nova_public_np(recs)
    got = bodies.reshape(len(names), -1, 32)[:, 1:16, :4].copy().view(np.uint32).reshape(len(names), 15)
    for i, name in enumerate(names):
        if exp[i] != "assert":
            assert np.array_equal(got[i], want[i]), (circuit, name, got[i], want[i])
    ok = np.array([e == "ok" for e in exp])
    assert _upper_bytes_zero(bodies[ok], 1, 15)


def test_coverage_of_the_listed_edges(nova):
    names, recs, exp = nova
    ok = [i for i, e in enumerate(exp) if e == "ok"]
    # every istar of the list on a parent step with total_depth != leaf_depth; those inside [0, 64) with the index bit 0 and 1,
    # taken from the low word below 32 and from the high word from 32 on
    seen = {}
    for i in ok:
        r = recs[i]
        if names[i].startswith("istar=") and C.is_parent(r):
            assert int(r[C.TD]) != int(r[C.LD])
            istar = int(r[C.TD]) - 2 - int(r[C.DEPTH])
            ci = int(r[C.CIL]) | int(r[C.CIH]) << 32
            seen.setdefault(istar, set()).add((ci >> istar) & 1 if 0 <= istar < 64 else None)
    assert set(seen) == set(C.ISTARS)
    for istar in C.ISTARS:
        assert seen[istar] == ({0, 1} if 0 <= istar < 64 else {None}), istar
    # a leaf step for every istar too (chunk_idx goes to t[0], t[1] there), and chunk_idx_high != 0 on a leaf
    assert {int(recs[i][C.TD]) - 2 - int(recs[i][C.DEPTH]) for i in ok if names[i].startswith("istar=") and not C.is_parent(recs[i])} == set(C.ISTARS)
    assert any(int(recs[i][C.CIH]) != 0 and not C.is_parent(recs[i]) for i in ok)
    assert {int(recs[i][C.TD]) for i in ok} >= {0, 1}
    # every |k| of K_EDGES at every gadget with every sign the gadget has in a step the kernels compute:
    #   root = -depth <= 0, and depth = M - 1 is never accepted;  e0 = -block_count <= 0;
    #   e1 = n_blocks - 1 - block_count in [-(M - 1), M - 2] (below that: "domain");
    #   eqs[0] = istar in [-(M - 64), M - 3]  (total_depth <= M - 1 above; eqs[63] = istar - 63 >= -(M - 1) below);
    #   eqs[63] = istar - 63 in [-(M - 1), M - 66].
    lim = {"root": (-(M - 2), 0), "e0": (-(M - 1), 0), "e1": (-(M - 1), M - 2), "eq0": (-(M - 64), M - 3), "eq63": (-(M - 1), M - 66)}
    have = set()
    for i in ok:
        k = C.ks(recs[i])
        for g, v in (("root", k["root"]), ("e0", k["e0"]), ("e1", k["e1"]), ("eq0", k["eq"][0]), ("eq63", k["eq"][63])):
            have.add((g, v))
    for g, (lo, hi) in lim.items():
        for K in C.K_EDGES:
            for v in (K, -K):
                if lo <= v <= hi:
                    assert (g, v) in have, (g, v)
    # both sides of every rule of the domain's limit
    dom = [recs[i] for i, e in enumerate(exp) if e == "domain"]
    assert any(abs(C.ks(r)["e1"]) >= M for r in dom) and any(abs(C.ks(r)["eq"][0]) >= M for r in dom)
    assert any(abs(C.ks(r)["eq"][63]) >= M > abs(C.ks(r)["eq"][0]) for r in dom)
    assert any(int(r[C.BC]) == M - 1 and abs(C.ks(r)["e1"]) < M for r in dom)
    assert any(int(recs[i][C.BC]) == M - 1 for i in ok) and any(C.ks(recs[i])["eq"][63] == -(M - 1) for i in ok)
    # the CheckDepth window from both sides at three depths
    for depth in (0, 10, M - 300):
        diffs = {int(r[C.LD]) - int(r[C.DEPTH]): e for r, e in zip(recs, exp) if int(r[C.DEPTH]) == depth}
        assert diffs[0] == "assert" and diffs[1] == "ok" and diffs[2] == "ok" and diffs[255] == "ok" and diffs[256] == "ok" and diffs[257] == "assert"


def _violations(system, bodies, rows):
    return {i: R.violated(system, R.body_to_ints(bodies[i]))[:4] for i in rows}


def test_oracle_bodies_satisfy_the_constraints_compression(comp, oracle_out):
    """tests/r1cs_ref.py (plain integers, from the circuit's .r1cs alone) over the oracle's body of EVERY compression row."""
    system = R.parse(R.read_image(R.BUILTIN))
    rc, bodies = oracle_out["compression"]
    bad = {comp[0][i]: v for i, v in _violations(system, bodies, range(len(comp[0]))).items() if v}
    assert not bad, bad


@pytest.mark.parametrize("circuit", ["nova_bn254_o1", "nova_vesta"])
def test_oracle_bodies_satisfy_the_constraints_nova(circuit, nova, oracle_out):
    """The plain-integer evaluator takes 0.1 s a body, so this test takes a part of the nova table; the device check of
    tests/test_gpu_record_domain.py takes every accepted row of every build.
      nova_bn254_o1 (the build that keeps the signed differences as slots): every "domain" row and its neighbours, every row of
        the inverse-table families (eqs[], e1, block_count, depth) and the istar rows of two of the four index pairs;
      nova_vesta: the "domain" rows, their neighbours, and the rows with an argument of M - 2 or M - 1."""
    names, recs, exp = nova
    rc, bodies = oracle_out[circuit]
    if circuit == "nova_bn254_o1":
        pick = [i for i, nm in enumerate(names) if exp[i] != "assert" and (
            nm.startswith(("domain", "eqs[", "e1=", "block_count=", "depth=", "total_depth=")) or
            (nm.startswith("istar=") and ("cih=0x80000001" in nm or "cih=0x0" in nm)))]
        system = R.parse(R.read_image(R.BUILTIN_NOVA_O1))
        assert len(pick) >= 100
    else:
        pick = [i for i, nm in enumerate(names) if exp[i] != "assert" and (
            nm.startswith("domain") or any(abs(v) >= M - 2 for v in (lambda k: [k["root"], k["e0"], k["e1"], k["eq"][0], k["eq"][63]])(C.ks(recs[i]))))]
        system = R.parse(R.read_image(R.BUILTIN_NOVA_O2[circuit]))
        assert len(pick) >= 20
    assert sum(1 for i in pick if exp[i] == "domain") == exp.count("domain")
    bad = {names[i]: v for i, v in _violations(system, bodies, pick).items() if v}
    assert not bad, bad
