"""The exact (field-element) device kernel at its assert sites and field-arithmetic edges: WHICH assert fires (round, G, half), with
the reference WASM's own trace text, and the accepted bodies byte for byte.

  fixture parity   every case of tests/golden/assert_sites.json.gz (recorded from the reference WASMs) through the calculator
  site agreement   a directed table checked against the oracle and the text recorded for the oracle's site
  inverses         the IsZero inverses of the device body against Python's pow(a, -1, p)
"""
import numpy as np
import pytest
import b3w_testlib as T
import assert_site_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return A.load_fixture(T.GOLD)


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_fixture_parity(circuit, fixture):
    m = T.pkg()
    wc = m.builder(circuit)
    nok = nrej = 0
    for case in fixture["circuits"][circuit]["cases"]:
        if "error" in case:
            with pytest.raises(m.B3WError) as e:
                wc.calculateBinWitness(case["input"], 0)
            assert e.value.status == m.B3W_E_ASSERT_FAILED, case["name"]
            assert str(e.value) == case["error"], case["name"]                       # the WASM's own trace, line for line
            nrej += 1
        else:
            assert T.sha256(wc.calculateBinWitness(case["input"], 0)) == case["body_sha256"], case["name"]
            nok += 1
    assert nrej >= 40 and (circuit == "compression" or nok >= 20), (nok, nrej)


def _directed_table(circuit):
    """(name, input) the oracle decides: the F1 candidate stream unthinned, cancellations that carry a wide word past every add1 to a
    ToBits, and the canonical all-zero / all-ones records."""
    W = T.workloads()
    out = [(f"f1_{i}", A.f1_candidate(W, circuit, i)) for i in range(120)]
    if circuit == "compression":
        base = W.record_to_input(W.config2_compression(1, first=3)[0], W.COMPRESSION_KEYS)
        wide = [("t", 0), ("t", 1), ("b", None), ("d", None)]
    else:
        c3 = W.config3_nova(40)
        base = W.record_to_input([r for r in c3 if r[14] == r[12] - 1 and r[14] > 0][1], W.NOVA_KEYS)         # a leaf step
        wide = [("chunk_idx_low", None), ("chunk_idx_high", None), ("b", None)]

    def mod(**kw):
        o = {k: (list(v) if isinstance(v, list) else v) for k, v in base.items()}
        for k, (j, v) in kw.items():
            if j is None:
                o[k] = v
            else:
                o[k][j] = v
        return o
    site_of = lambda inp: A.oracle_site(*T.oracle_witness(circuit, T.normalize_input(circuit, inp))[::2])
    for j in range(4):          # round 0 sees the 2^32 of h[j] cancelled; h[j] itself reaches outXor[8 + j].tb_y
        out.append((f"cancel_h{j}", A.cancellation_case(W, circuit, j, site_of, start=10000)[1]))
        out.append((f"cancel_h{j}_rec0", mod(h=(j, (1 << 32) + 5), m=(2 * j, -(1 << 32)))))     # ... or -2^32 trips a later add1
        out.append((f"h{j}_2p32", mod(h=(j, 1 << 32))))
    for g in range(4):          # v[b] of column g: rxor4.tb
        out.append((f"h{4 + g}_2p32", mod(h=(4 + g, 1 << 32))))
    for k, j in wide:           # v[d] of columns 0..3: rxor2.tb
        out.append((f"{k}{'' if j is None else j}_2p32", mod(**{k: (j, 1 << 32)})))
    n = T.NIN[circuit]
    for name, word in (("all_zero", 0), ("all_ones", 0xFFFFFFFF)):
        out.append((name, W.record_to_input(np.full(n, word, dtype=np.uint32), T.keys_of(circuit))))
    return out


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_site_agreement_with_oracle(circuit):
    m = T.pkg()
    wc = m.builder(circuit)
    texts = A.known_texts(T, circuit)
    sites = {}
    for name, inp in _directed_table(circuit):
        rc, want, err = T.oracle_witness(circuit, T.normalize_input(circuit, inp))
        site = A.oracle_site(rc, err)
        sites[name] = site
        if site is None:
            assert np.array_equal(wc.calculateBinWitness(inp, 0), want), name
        else:
            with pytest.raises(m.B3WError) as e:
                wc.calculateBinWitness(inp, 0)
            assert e.value.status == m.B3W_E_ASSERT_FAILED, name
            assert str(e.value) == A.expected_text(circuit, texts, site), (name, site)
    # the table reaches what it is there for (decided by the oracle alone)
    f1 = [s for n, s in sites.items() if n.startswith("f1_")]
    assert {s[1] for s in f1 if s} >= set(range(7)) and all(s is None or s[0] == 1 for s in f1) and f1.count(None) >= 10
    assert [sites[f"cancel_h{j}"] for j in range(4)] == [sites[f"h{j}_2p32"] for j in range(4)] == [(6, 7, j, 1) for j in range(4)]
    assert [sites[f"h{4 + g}_2p32"] for g in range(4)] == [(4, 0, g, 0) for g in range(4)]
    wide = ["t0", "t1", "b", "d"] if circuit == "compression" else ["chunk_idx_low", "chunk_idx_high", "b"]
    assert [sites[k + "_2p32"] for k in wide] == [(2, 0, g, 0) for g in range(len(wide))]
    assert sites["all_zero"] == sites["all_ones"] == (None if circuit == "compression" else (12, 0, 0, 0))


@pytest.mark.parametrize("circuit", T.CIRCUITS[1:])
def test_iszero_inverses_against_python(circuit, fixture):
    """Every non-zero IsZero argument's inverse, computed by Python, is a slot value of the device body (the binary-GCD inverse in 67
    lane jobs, jobs 64..66 in a second trip of lanes 0..2); independent of the oracle's own inversion."""
    m = T.pkg()
    wc = m.builder(circuit)
    p = T.PRIME[circuit]
    cases = [c for c in fixture["circuits"][circuit]["cases"] if c["name"].startswith("f4_")]
    assert len(cases) == 16
    for case in cases:
        assert "body_sha256" in case, case["name"]
        body = np.asarray(wc.calculateBinWitness(case["input"], 0), dtype=np.uint8).reshape(-1, 32)
        slots = {row.tobytes() for row in body}
        args = A.iszero_args(case["input"], p)
        assert len(args) == 67 and sum(a != 0 for a in args) >= 65                  # at most -depth and one eqs[i] argument are 0
        for k, a in enumerate(args):
            if a:
                assert pow(a, -1, p).to_bytes(32, "little") in slots, (case["name"], k)
