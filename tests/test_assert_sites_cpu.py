"""The oracle against the reference WASM at the assert sites of the exact kernel (tests/golden/assert_sites.json.gz, made by
tools/gen_assert_golden.py): which assert fires, in which round, G and half, and the accepted bodies at the field-arithmetic edges
(CheckDepth boundaries, chunk_idx wraps, IsZero arguments next to 0 and p)."""
import pytest
import b3w_testlib as T
import assert_site_cases as A


@pytest.fixture(scope="module")
def fixture():
    return A.load_fixture(T.GOLD)


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_oracle_site_is_the_wasms(circuit, fixture):
    f = fixture["circuits"][circuit]
    assert f["nwit"] == T.NWIT[circuit] and int(f["prime"]) == T.PRIME[circuit]
    nok = nrej = 0
    for case in f["cases"]:
        rc, body, err = T.oracle_witness(circuit, T.normalize_input(circuit, case["input"]))
        site = A.oracle_site(rc, err)
        assert (None if site is None else list(site)) == case["site"], case["name"]
        if "error" in case:
            assert site is not None and case["error"].startswith("Error: Assert Failed.\n"), case["name"]
            nrej += 1
        else:
            assert site is None and T.sha256(body) == case["body_sha256"], case["name"]
            nok += 1
    assert nrej >= 40 and (circuit == "compression" or nok >= 20), (nok, nrej)


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_one_site_one_text(circuit, fixture):
    cases = fixture["circuits"][circuit]["cases"]
    texts = A.site_texts(circuit, cases)                                    # same site, same text (asserted inside)
    add1 = {s: t for s, t in texts.items() if s[0] == 1}
    by_text = {}
    for s, t in add1.items():
        by_text.setdefault(t, set()).add((s[2], s[3]))
    assert all(len(gh) == 1 for gh in by_text.values()), by_text           # another (G, half), another text
    # rounds 1..6 print the first-round trace of their (G, half) with the line of the loop over rounds[i + 1]
    first = {(s[2], s[3]): t for s, t in add1.items() if s[1] == 0}
    later = [(s, t) for s, t in add1.items() if s[1] >= 1]
    assert len(first) == 16 and later
    for s, t in later:
        assert t == A.later_round_text(first[(s[2], s[3])], circuit), s


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_f1_coverage(circuit, fixture):
    cases = [c for c in fixture["circuits"][circuit]["cases"] if c["name"].startswith("f1_")]
    sk = [(tuple(c["site"]), circuit != "compression" and A.is_parent(c["input"])) for c in cases]
    assert A.f1_coverage_gaps(circuit, sk) == []
    # the cases are candidates of the recipe, unchanged
    W = T.workloads()
    for c in cases:
        i = int(c["name"].split("_")[1])
        want = A.f1_candidate(W, circuit, i)
        assert T.normalize_input(circuit, c["input"]).tobytes() == T.normalize_input(circuit, want).tobytes(), c["name"]


@pytest.mark.parametrize("circuit", T.CIRCUITS)
def test_tobits_family(circuit, fixture):
    by = {c["name"]: c for c in fixture["circuits"][circuit]["cases"]}
    assert [by[f"f0_r0g{g}h{hf + 1}"]["site"] for g in range(8) for hf in range(2)] == [[1, 0, g, hf] for g in range(8) for hf in range(2)]
    assert [by[f"f5_h{j}_2p32"]["site"] for j in range(8)] == [[6, 7, j, 1] for j in range(4)] + [[4, 0, g, 0] for g in range(4)]
    wide = ["t0", "t1", "b", "d"] if circuit == "compression" else ["chunk_idx_low", "chunk_idx_high", "b"]
    assert [by[f"f5_{k}_2p32"]["site"] for k in wide] == [[2, 0, g, 0] for g in range(len(wide))]
    cancel = sorted((n, c) for n, c in by.items() if n.startswith("f5_cancel_h"))
    assert [c["site"] for _, c in cancel] == [[6, 7, j, 1] for j in range(4)]
    for j, (_, c) in enumerate(cancel):
        p = T.PRIME[circuit]
        assert int(c["input"]["h"][j]) == 2**32 + 5 and int(c["input"]["m"][2 * j]) % p == p - 2**32
        assert c["error"] == by[f"f5_h{j}_2p32"]["error"]


@pytest.mark.parametrize("circuit", T.CIRCUITS[1:])
def test_directed_nova_families(circuit, fixture):
    by = {c["name"]: c for c in fixture["circuits"][circuit]["cases"]}
    want = {-258: 10, -257: 11, -256: None, -2: None, -1: None, 0: 12, 254: 12, 255: 10}
    for delta, code in want.items():
        c = by[f"f2_depth_minus_leaf_{delta}"]
        assert int(c["input"]["leaf_depth"]) == 300 and int(c["input"]["depth"]) == 300 + delta
        assert c["site"] == (None if code is None else [code, 0, 0, 0]), delta
    assert by["f2_wrap_leaf0_depth_pm1"]["site"] is None and int(by["f2_wrap_leaf0_depth_pm1"]["input"]["depth"]) == T.PRIME[circuit] - 1
    assert by["f3_parent_low_2p65m1"]["site"] is None and by["f3_parent_low_2p65"]["site"] == [13, 0, 0, 0]
    assert by["f3_parent_high_5inv"]["site"] is None and by["f3_parent_sum_wraps"]["site"] is None
    assert by["f3_leaf_high_5inv"]["site"] == [2, 0, 1, 0]
    f4 = [c for n, c in by.items() if n.startswith("f4_")]
    assert len(f4) == 16 and all(c["site"] is None for c in f4)
    p = T.PRIME[circuit]
    args = A.iszero_args(by["f4_leaf_x31"]["input"], p)
    assert args[3 + 31] == 0 and args[3 + 32] == p - 1 and args[3 + 63] == p - 32 and args[1] == 31 and args[2] == 62
    assert A.iszero_args(by["f4_leaf_x63"]["input"], p)[3 + 63] == 0
