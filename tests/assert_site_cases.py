"""Assert sites of the exact kernel: the candidate recipe, the oracle's site and the text a site must give.

Shared by tools/gen_assert_golden.py (which records what the reference WASM says, tests/golden/assert_sites.json.gz) and the tests
that hold the oracle and the device kernel against it.  Nothing here looks at the library's output.

A site is (code, round, g, half) with the codes of b3w_exact.hip: 1 add1 (Bits34), 2 rxor2.tb, 3 add3 (Bits33), 4 rxor4.tb,
5 / 6 outXor tb_x / tb_y (round 7, g = k & 7, half = k >> 3), 10 check_parent Num2Bits(9), 11 exceed_depth Num2Bits(9),
12 exceed_depth.out === 0, 13 down_left_path Num2Bits(65), 14 down_left_path.out boolean."""
import gzip, json, os, random, re

F1_SEED = 0xB3A55E7
F1_FIRST = {"compression": 5000, "nova": 7000}
FIXTURE = "assert_sites.json.gz"

_WHAT = (("Bits34", 1), ("ToBits(rxor2)", 2), ("Bits33", 3), ("ToBits(rxor4)", 4), ("outXor ToBits x", 5), ("outXor ToBits y", 6),
         ("check_parent Num2Bits(9)", 10), ("exceed_depth Num2Bits(9)", 11), ("exceed_depth.out === 0", 12),
         ("down_left_path Num2Bits(65)", 13), ("down_left_path.out boolean", 14))
_SITE_RE = re.compile(r"^Assert Failed\. (.*) \(round (-?\d+) G (\d+) half (\d+)\)$")


def oracle_site(rc, err):
    """(rc, err) of b3wo_witness -> (code, round, g, half) in the kernel's numbering, or None for an accepted input."""
    if rc == 0:
        return None
    assert rc == 4, (rc, err)
    mt = _SITE_RE.match(err)
    assert mt, err
    what, r, g, hf = mt.group(1), int(mt.group(2)), int(mt.group(3)), int(mt.group(4)) - 1
    code = next(c for w, c in _WHAT if what.startswith(w))
    if code >= 10:
        return (code, 0, 0, 0)
    if code >= 5:                                    # the oracle reports outXor[k] as (7, k, 0)
        return (code, 7, g & 7, g >> 3)
    return (code, r, g, hf)


def is_parent(inp):
    return int(inp["depth"]) < int(inp["leaf_depth"]) - 1


def f1_candidate(W, circuit, i):
    """Candidate i of the later-round Bits34 family: a config-2 / config-3 record with ONE message word set just under 2^34, so that
    add1 overflows in whichever round first meets it with v[a] + v[b] large enough (a parent step reads m[0..7] only)."""
    rng = random.Random(F1_SEED * 4096 + i)
    if circuit == "compression":
        inp = W.record_to_input(W.config2_compression(1, first=F1_FIRST["compression"] + i)[0], W.COMPRESSION_KEYS)
        j = rng.randrange(16)
    else:
        inp = W.record_to_input(W.config3_nova(1, first=F1_FIRST["nova"] + i)[0], W.NOVA_KEYS)
        j = rng.randrange(8 if is_parent(inp) else 16)
    inp["m"][j] = (1 << 34) - 3 * (1 << 31) + rng.getrandbits(30)
    return inp


def cancellation_case(W, circuit, j, site_of, start=0, tries=3000):
    """h[j] = 2^32 + 5 with m[2j] = -2^32: round 0's add1 of column j sees the 2^32 cancelled, and the wide h[j] itself comes back
    as outXor[8 + j].y.  The word -2^32 meets an add1 again in every later round and passes it only where v[a] + v[b] >= 2^32
    there, so most records end in a later-round add1 instead: take the first record (leaf steps for nova) from `start` on that the
    oracle (site_of) carries through to tb_y.  -> (record index, input)"""
    for i in range(start, start + tries):
        if circuit == "compression":
            inp = W.record_to_input(W.config2_compression(1, first=i)[0], W.COMPRESSION_KEYS)
        else:
            inp = W.record_to_input(W.config3_nova(1, first=i)[0], W.NOVA_KEYS)
            if is_parent(inp):
                continue
        inp["h"][j] = (1 << 32) + 5
        inp["m"][2 * j] = -(1 << 32)
        if site_of(inp) == (6, 7, j, 1):
            return i, inp
    raise AssertionError((circuit, j, "no record reaches outXor tb_y"))


def f1_coverage_gaps(circuit, sites_and_kinds):
    """The F1 coverage condition over [(site, parent?)] -> list of what is missing (empty when it holds)."""
    gaps = []
    for r in range(1, 7):
        here = [(s, par) for s, par in sites_and_kinds if s is not None and s[0] == 1 and s[1] == r]
        gh = {(s[2], s[3]) for s, _ in here}
        if len(gh) < 4:
            gaps.append(f"round {r}: {len(gh)} distinct (G, half)")
        if {h for _, h in gh} != {0, 1}:
            gaps.append(f"round {r}: one half only")
        if not any(g < 4 for g, _ in gh):
            gaps.append(f"round {r}: no column G")
        if not any(g >= 4 for g, _ in gh):
            gaps.append(f"round {r}: no diagonal G")
        if circuit != "compression" and {par for _, par in here} != {False, True}:
            gaps.append(f"round {r}: leaf and parent steps not both there")
    return gaps


def later_round_text(text, circuit):
    """The first-round trace of an add1 site -> the trace of the same (G, half) in rounds 1..6: the SingleRound is then started from
    inside the loop over rounds[i + 1], one source line of Blake3Compression further down."""
    old, new = ("Blake3Compression_40 line: 194\n", "Blake3Compression_40 line: 207\n") if circuit == "compression" else \
               ("Blake3Compression_53 line: 195\n", "Blake3Compression_53 line: 208\n")
    assert text.count(old) == 1, text
    return text.replace(old, new)


def load_fixture(gold_dir):
    with gzip.open(os.path.join(gold_dir, FIXTURE), "rt") as f:
        return json.load(f)


def site_texts(circuit, cases):
    """{site: recorded text} over cases that carry "site" and "error"; one site, one text."""
    out = {}
    for c in cases:
        if c.get("error") is None:
            continue
        s = tuple(c["site"])
        assert out.setdefault(s, c["error"]) == c["error"], (circuit, c["name"])
    return out


_known = {}


def known_texts(T, circuit):
    """{site: the WASM's text} from the assert-site fixture and the rejected cases of the circuit's golden file, whose sites the
    oracle names.  Computed once per circuit; callers do not change it."""
    if circuit not in _known:
        texts = site_texts(circuit, load_fixture(T.GOLD)["circuits"][circuit]["cases"])
        for c in T.golden(circuit)["cases"]:
            if "error" in c:
                site = oracle_site(*T.oracle_witness(circuit, T.normalize_input(circuit, c["input"]))[::2])
                assert site is not None and texts.setdefault(site, c["error"]) == c["error"], (circuit, c["name"])
        _known[circuit] = texts
    return _known[circuit]


def expected_text(circuit, texts, site):
    """Text for the oracle's site from {site: text}: the recorded one, else for add1 in rounds 1..6 the first-round one, line swapped."""
    if site in texts:
        return texts[site]
    if site[0] == 1 and 1 <= site[1] <= 6 and (1, 0, site[2], site[3]) in texts:
        return later_round_text(texts[(1, 0, site[2], site[3])], circuit)
    raise KeyError((circuit, site))


def iszero_args(inp, p):
    """The 67 IsZero arguments of a nova step (root, e0, e1, eqs[0..63]) as integers mod p."""
    depth, bc, nb, td = (int(inp[k]) for k in ("depth", "block_count", "n_blocks", "total_depth"))
    return [(-depth) % p, (-bc) % p, (nb - 1 - bc) % p] + [(td - i - 2 - depth) % p for i in range(64)]
