"""The CPU restatement of the tamper check (tests/verify_ref.py) and the planting plans tests/test_gpu_verify_units.py executes: the input
slots hold the record by VALUE in the oracle's bodies, the reference gives the verdicts include/b3wit.h describes, and the plans cover
what they claim — every unit outside the input slots in the sweep, every (j, edge unit) pair alone in a body, every verdict class of a
tampered input.  No GPU."""
import numpy as np
import pytest

import b3w_testlib as T
import record_domain_cases as C
import verify_ref as V

NOVA = T.CIRCUITS[1:]


def _records(circuit, n=64):
    W = T.workloads()
    return W.config2_compression(n) if circuit == "compression" else W.config3_nova(n)


@pytest.fixture(scope="module")
def oracle_bodies():
    """{circuit: (records, bodies)} — 64 records per circuit through the oracle, once"""
    out = {}
    for c in T.CIRCUITS:
        recs = _records(c)
        bad, bodies = T.oracle_batch_u32(c, recs)
        assert bad == 0
        out[c] = (recs, bodies.copy())
    return out


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_input_slots_hold_the_record_by_value(circuit, oracle_bodies):
    recs, bodies = oracle_bodies[circuit]
    if circuit != "compression":
        kinds = {C.is_parent(r) for r in recs}
        assert kinds == {False, True}                                        # leaf steps and parent steps
    s = V.in_slots(circuit)
    assert s.shape == (T.NIN[circuit],) and len(set(s.tolist())) == len(s) and 0 < s.min() and s.max() < T.NWIT[circuit]
    b = bodies.reshape(len(recs), T.NWIT[circuit], 32)[:, s, :]
    assert not b[:, :, 4:].any()                                            # plain 32-bit values
    got = np.ascontiguousarray(b[:, :, :4]).view("<u4").reshape(len(recs), -1)
    for j in range(T.NIN[circuit]):
        assert np.array_equal(got[:, j], recs[:, j]), (circuit, j, int(s[j]))
    for i in range(len(recs)):
        assert np.array_equal(V.record_of(circuit, bodies[i]), recs[i])


def test_the_slots_are_the_documented_ones():
    """DESIGN.md "Input domain" / include/b3wit.h: nova words 0 and 10..13 are read from public OUTPUTS that share the input's atom"""
    assert V.in_slots("compression").tolist() == list(range(17, 45))
    nova = [1] + list(range(17, 26)) + [13, 14, 15, 11] + list(range(28, 46))
    for c in NOVA:
        assert V.in_slots(c).tolist() == nova
        assert V.copy_slots(c) == [(0, 16), (10, 26), (11, 27)]
    assert V.copy_slots("compression") == []                                 # the compression layout keeps each input word once


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_ref_clean_and_planted_counts(circuit, oracle_bodies):
    recs, bodies = oracle_bodies[circuit]
    for i in (0, 1, 2, 31, 63):
        assert V.verify_ref(circuit, bodies[i]) == 0
    free = np.setdiff1d(np.arange(V.n_units(circuit)), V.input_units(circuit))
    rng = np.random.default_rng(7)
    for i, k in ((3, 1), (4, 2), (5, 17), (6, 400)):
        body = bodies[i].copy()
        for u in rng.choice(free, size=k, replace=False):
            V.plant(body, int(u), int(rng.integers(0, 4)), int(rng.integers(0, 32)))
        assert V.verify_ref(circuit, body) == k
        V.plant(body, int(free[0]), 0, 0)
        V.plant(body, int(free[0]), 0, 0)                                    # a plant is its own inverse
        assert V.verify_ref(circuit, body) == k
    # two plants in ONE unit count once
    body = bodies[7].copy()
    V.plant(body, int(free[-1]), 0, 3)
    V.plant(body, int(free[-1]), 3, 30)
    assert V.verify_ref(circuit, body) == 1


@pytest.mark.parametrize("circuit", NOVA)
def test_ref_rejects_assert_and_domain_records(circuit, oracle_bodies):
    """the "assert" and "domain" rows of the record-domain table written into a clean body's input slots: 0xFFFFFFFF, whatever the
    rest of the body says; an "ok" row written the same way gives a count (the body no longer matches it), never the flag"""
    _recs, bodies = oracle_bodies[circuit]
    s = V.in_slots(circuit)
    seen = set()
    for name, rec, exp in C.nova_rows():
        if exp == "ok" and "ok" in seen and not name.startswith("domain-neighbour"):
            continue
        body = bodies[0].copy()
        body.view("<u4").reshape(-1, 8)[s, 0] = rec
        v = V.verify_ref(circuit, body)
        assert (v == V.REJECTED) == (exp != "ok"), (name, exp, v)
        seen.add(exp)
    assert seen == {"ok", "assert", "domain"}


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_ref_rejects_input_slots_that_are_no_plain_words(circuit, oracle_bodies):
    _recs, bodies = oracle_bodies[circuit]
    s = V.in_slots(circuit)
    for j in (0, 1, len(s) // 2, len(s) - 1):
        for byte in (4, 7, 8, 15, 16, 31):
            body = bodies[2].copy()
            body[int(s[j]) * 32 + byte] = 1
            assert V.verify_ref(circuit, body) == V.REJECTED, (j, byte)
    body = bodies[2].copy()
    body[int(s[0]) * 32 + 3] ^= 0x80                                         # byte 3 belongs to the word
    assert V.verify_ref(circuit, body) != V.REJECTED


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_sweep_plan_plants_every_unit_once_in_every_word(circuit):
    """(a) the 17 residue classes partition the units outside in_slots; each class is planted in all four words, with bits that reach both
    halves of a word and values >= 2; and what the sweep leaves out is the input slots' units alone — at most 64, below 0.14 %"""
    nu = V.n_units(circuit)
    seen = np.zeros(nu, dtype=np.int64)
    for r in range(V.MOD):
        u = V.sweep_units(circuit, r)
        assert (u % V.MOD == r).all() and len(set(u.tolist())) == u.size
        seen[u] += 1
        for wd in range(4):
            bits = V.sweep_bits(u, wd)
            assert bits.min() >= 0 and bits.max() <= 31 and (bits >= 16).any() and (bits < 16).any() and (bits >= 1).any()
    left_out = np.flatnonzero(seen == 0)
    assert (seen <= 1).all()
    assert np.array_equal(left_out, V.input_units(circuit))
    assert left_out.size <= 64 and left_out.size / nu < 0.0014
    # the planted body differs from the clean one in exactly those units and in that word only
    body = np.zeros(nu * 16, dtype=np.uint8)
    k = V.plant_sweep(circuit, body, 5, 2)
    w = body.view("<u4").reshape(-1, 4)
    assert k == V.sweep_units(circuit, 5).size and np.array_equal(np.flatnonzero(w.any(axis=1)), V.sweep_units(circuit, 5))
    assert not w[:, [0, 1, 3]].any()
    hit = w[V.sweep_units(circuit, 5), 2]
    assert (hit & (hit - 1) == 0).all() and (hit >= 2).any()                 # one bit each, and not always bit 0
    # every lane pair and every slot position of a tile meets every class (17 is coprime to 64)
    for r in (0, 16):
        assert len(set((V.sweep_units(circuit, r) % 64).tolist())) == 64


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_edge_plan_plants_every_edge_unit_of_every_j_alone(circuit):
    """(b) over the 20 configurations every (j, edge unit) pair is planted, alone in its body, at least once; victims and clean bodies mix
    in every launch; every body is a victim once per configuration — body n - 1 and the last active body of every ragged wave with it"""
    nwit = T.NWIT[circuit]
    own = set(V.input_units(circuit).tolist())
    # the edge list itself, against the tile arithmetic of expand_verify
    for j in range(4):
        nt = V.n_tiles(circuit, j)
        assert nt == -(-(nwit + j) // 32)
        # a tile at or behind nt starts at slot 32 nt - j >= nwit: in expand_verify's `in`, "slot < nwit" alone already excludes the
        # clamped tiles of the tail iteration, "k0 + u < ntiles" says nothing more.  What the edge test can and does catch is a
        # comparison that takes the CLAMPED tile's slots (the last tile counted two to four times) and a loop that stops before the tail.
        assert 32 * nt - j >= nwit > 32 * (nt - 1) - j
        slots = V.edge_slots(circuit, j)
        last_tile = range(max(32 * (nt - 1) - j, 0), nwit)
        tail_iter = range(128 * ((nt - 1) // 4) - j, nwit)
        assert 0 in slots and nwit - 1 in slots and nwit - 2 in slots
        assert last_tile[0] in slots and last_tile[0] - 1 in slots and tail_iter[0] in slots and tail_iter[0] - 1 in slots
        assert {127 - j, 128 - j} <= set(slots)
        for s in (1, 31 - j, 32 - j):
            assert s in slots or 2 * s in own                                  # left out only where it is an input slot
    assert (V.n_tiles(circuit, 0) % 4 == 0) == (circuit in ("nova_bn254", "nova_vesta"))     # the O2 builds run no clamped tail
    plan = V.edge_plan(circuit)
    assert [(p, b) for p, b, _ in plan] == [(p, b) for p in V.PADS for b in V.BASES]
    planted = set()
    js_by_base16 = set()
    for pad, base, launches in plan:
        addr = V.body_addresses(circuit, pad, base)
        victims = []
        for plants in launches:
            bodies = [p[0] for p in plants]
            assert len(set(bodies)) == len(bodies) and 0 < len(bodies) < V.N_EDGE           # one plant per victim; clean bodies beside them
            for i, u, wd, bit in plants:
                j = V.tile_j(addr[i])
                assert u in V.edge_units(circuit, j) and u not in own and 0 <= wd < 4 and 0 <= bit < 32
                planted.add((j, u))
                if base == 16:
                    js_by_base16.add(j)
            victims += bodies
        assert sorted(victims) == list(range(V.N_EDGE))
    assert js_by_base16 == {0}                                                 # 16-byte aligned buffers: unshifted tiles
    assert planted == {(j, u) for j in range(4) for u in V.edge_units(circuit, j)}


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_attribution_plan(circuit, oracle_bodies):
    _recs, bodies = oracle_bodies[circuit]
    plan = V.attribution_plan(circuit)
    own = set(V.input_units(circuit).tolist())
    assert len(plan) == V.N_EDGE
    for i, plants in enumerate(plan):
        assert len(plants) == i == len({u for u, _, _ in plants}) and not own & {u for u, _, _ in plants}
    for i in (0, 1, 36):
        body = bodies[i].copy()
        for u, wd, bit in plan[i]:
            V.plant(body, u, wd, bit)
        assert V.verify_ref(circuit, body) == i


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_input_cases_reach_every_verdict_class(circuit):
    """(c) per circuit the reference answers the input cases with an exact count, with 0xFFFFFFFF and — where the layout keeps a second
    copy of an input atom, which the compression layout does not — with exactly 1; for nova the low-word flips alone give both counts
    and 0xFFFFFFFF (the depth and leaf_depth bits)"""
    cases = V.input_cases(circuit)
    nin = T.NIN[circuit]
    for kind, per_word in (("low", 2), ("upper", 3)):
        assert sorted(c[1] for c in cases if c[0] == kind) == sorted(list(range(nin)) * per_word)
    assert [(c[1], c[2]) for c in cases if c[0] == "copy"] == V.copy_slots(circuit)
    for name, rec in V.base_records(circuit).items():
        rc, b = T.oracle_each_u32(circuit, rec[None, :])
        assert rc[0] == 0 and V.verify_ref(circuit, b[0]) == 0
        if circuit != "compression":
            assert C.is_parent(rec) == (name == "parent")
        got = {"low": [], "upper": [], "copy": []}
        for case in cases:
            body = b[0].copy()
            V.apply_case(body, case)
            got[case[0]].append(V.verify_ref(circuit, body))
        assert set(got["upper"]) == {V.REJECTED}
        assert set(got["copy"]) <= {1} and (len(got["copy"]) > 0) == (circuit != "compression")
        counts = [v for v in got["low"] if v != V.REJECTED]
        assert len(counts) > nin and max(counts) > 1000                       # most flips make another record with another witness
        if circuit != "compression":
            assert V.REJECTED in got["low"]
            depth_flips = [v for c, v in zip([c for c in cases if c[0] == "low"], got["low"]) if c[1] in (C.LD, C.DEPTH)]
            assert V.REJECTED in depth_flips and any(v != V.REJECTED for v in depth_flips)
