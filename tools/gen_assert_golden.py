#!/usr/bin/env python3
"""Record what the reference's committed WASMs say at the assert sites of the exact kernel (build container only; needs node and
the reference checkout, like tools/gen_golden.py and tools/probe_traces.py).

The CPU oracle (oracle/b3w_oracle.c) classifies deterministic candidates; the cases kept are then run through the reference's own
witness_calculator.js (recover_layout.run_oracle) and its answer is what goes into tests/golden/assert_sites.json.gz: per build
and case the name, the input (decimal strings), the oracle's site [code, round, g, half] or null, and the WASM's error text or the
sha256 of its witness body.  Data only.  A case the WASM and the oracle decide differently stops the run: that is a finding about
the oracle.

  F0  add1 of round 0 at every (G, half)
  F1  later-round Bits34 (add1): tests/assert_site_cases.f1_candidate, thinned to a few cases per (round, leaf / parent step)
  F2  CheckDepth boundaries (nova)          F3  chunk_idx = low + high * 2^32 boundaries and wraps (nova)
  F4  IsZero arguments next to 0, p and the limb boundaries (nova)
  F5  the ToBits sites (rxor2.tb, rxor4.tb, outXor tb_y), plain and behind a cancellation

  python tools/gen_assert_golden.py
"""
import gzip, hashlib, json, os, sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import recover_layout as RL
import b3w_testlib as T
import assert_site_cases as A

W = T.workloads()
N_CANDIDATES = {"compression": 400, "nova": 300}
PER_ROUND_KIND = 4
MAX_BYTES = 150 * 1024


def oracle_of(circuit, inp):
    rc, body, err = T.oracle_witness(circuit, T.normalize_input(circuit, inp))
    return A.oracle_site(rc, err), body


def f1_cases(circuit):
    """Walk the candidate stream in order.  A candidate is kept when its (G, half) is new for its round and either its
    (round, leaf / parent) group is still short of PER_ROUND_KIND or it brings the round a half or a column / diagonal G it lacks."""
    kind = "compression" if circuit == "compression" else "nova"
    kept, seen, count = [], {}, {}
    for i in range(N_CANDIDATES[kind]):
        inp = A.f1_candidate(W, circuit, i)
        site, _ = oracle_of(circuit, inp)
        if site is None or site[0] != 1:
            continue
        _, r, g, hf = site
        par = kind == "nova" and A.is_parent(inp)
        here = seen.setdefault(r, set())
        if (g, hf) in here:
            continue
        lacks = hf not in {h for _, h in here} or (g < 4) not in {x < 4 for x, _ in here}
        if count.get((r, par), 0) < PER_ROUND_KIND or lacks:
            here.add((g, hf))
            count[(r, par)] = count.get((r, par), 0) + 1
            kept.append((f"f1_{i}_r{r}g{g}h{hf + 1}" + ("_parent" if par else ""), inp))
    return kept


def nova_bases():
    c3 = W.config3_nova(40)
    leaf_i = next(i for i in range(40) if c3[i][14] == c3[i][12] - 1 and c3[i][14] > 0)
    par_i = next(i for i in range(40) if c3[i][14] < c3[i][12] - 1)
    return W.record_to_input(c3[leaf_i], W.NOVA_KEYS), W.record_to_input(c3[par_i], W.NOVA_KEYS)


def mod(base, **kw):
    o = json.loads(json.dumps(base))
    o.update(kw)
    return o


def f0_cases(circuit):
    """add1 of round 0 at every (G, half), m[2g + half] = 2^34: the texts the later rounds are compared with."""
    base = W.record_to_input(W.config2_compression(1)[0], W.COMPRESSION_KEYS) if circuit == "compression" else nova_bases()[0]
    return [(f"f0_r0g{j // 2}h{j % 2 + 1}", mod(base, m=base["m"][:j] + [1 << 34] + base["m"][j + 1:])) for j in range(16)]


def f5_cases(circuit):
    """The ToBits sites: a 2^32 in h[4 + g] (rxor4.tb of column g), in h[j] (outXor[8 + j].tb_y) and in the words that start as
    v[12..15] (rxor2.tb), all in round 0; and the cancellation h[j] = 2^32 + 5, m[2j] = -2^32 on the first record of the config
    stream that carries it past every add1 to outXor[8 + j].tb_y."""
    comp = circuit == "compression"
    base = W.record_to_input(W.config2_compression(1)[0], W.COMPRESSION_KEYS) if comp else nova_bases()[0]
    out = [(f"f5_h{j}_2p32", mod(base, h=base["h"][:j] + [1 << 32] + base["h"][j + 1:])) for j in range(8)]
    if comp:
        out += [("f5_t0_2p32", mod(base, t=[1 << 32, base["t"][1]])), ("f5_t1_2p32", mod(base, t=[base["t"][0], 1 << 32])),
                ("f5_b_2p32", mod(base, b=1 << 32)), ("f5_d_2p32", mod(base, d=1 << 32))]
    else:
        out += [(f"f5_{k}_2p32", mod(base, **{k: 1 << 32})) for k in ("chunk_idx_low", "chunk_idx_high", "b")]
    for j in range(4):
        i, inp = A.cancellation_case(W, circuit, j, lambda x: oracle_of(circuit, x)[0])
        out.append((f"f5_cancel_h{j}_rec{i}", inp))
    return out


def directed_nova_cases(p):
    leaf, parent = nova_bases()
    out = []
    for delta in (-258, -257, -256, -2, -1, 0, 254, 255):                                     # F2
        out.append((f"f2_depth_minus_leaf_{delta}", mod(leaf, leaf_depth=300, depth=300 + delta)))
    out.append(("f2_wrap_leaf0_depth_pm1", mod(leaf, leaf_depth=0, depth=p - 1)))
    inv32 = pow(1 << 32, -1, p)                                                               # F3
    pb = mod(parent, leaf_depth=300, depth=100)
    out.append(("f3_parent_low_2p65m1", mod(pb, chunk_idx_low=(1 << 65) - 1, chunk_idx_high=0)))
    out.append(("f3_parent_low_2p65", mod(pb, chunk_idx_low=1 << 65, chunk_idx_high=0)))
    out.append(("f3_parent_high_5inv", mod(pb, chunk_idx_low=7, chunk_idx_high=5 * inv32 % p)))
    out.append(("f3_parent_sum_wraps", mod(pb, chunk_idx_low=p - 1, chunk_idx_high=inv32)))
    out.append(("f3_leaf_high_5inv", mod(leaf, chunk_idx_high=5 * inv32 % p)))
    for x in (31, 63, 2**32 + 32, 2**64 + 31, 2**128 + 32, 2**224 + 32, 2**253 + 5, (p - 1) // 2 + 32):    # F4
        for tag, base in (("leaf", leaf), ("parent", parent)):
            out.append((f"f4_{tag}_x{x if x < 64 else hex(x)}",
                        mod(base, total_depth=(x + 2 + int(base["depth"])) % p, block_count=(p - x) % p, n_blocks=(x + 1) % p)))
    return out


def strs(x):
    if isinstance(x, dict):
        return {k: strs(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [strs(v) for v in x]
    return str(x)


def main():
    doc = dict(generated_by="tools/gen_assert_golden.py from the reference's committed WASMs", circuits={})
    for circuit, cfg in RL.CIRCUITS.items():
        cases = f0_cases(circuit) + f1_cases(circuit) + f5_cases(circuit)
        if cfg["kind"] != "compression":
            cases += directed_nova_cases(cfg["prime"])
        classified = [oracle_of(circuit, inp) for _, inp in cases]
        gaps = A.f1_coverage_gaps(circuit, [(s, cfg["kind"] != "compression" and A.is_parent(inp))
                                            for (s, _), (n, inp) in zip(classified, cases) if n.startswith("f1_")])
        assert not gaps, (circuit, gaps)
        bodies, errors = RL.run_oracle(cfg["wasm"], [inp for _, inp in cases])
        out = []
        for i, ((name, inp), (site, obody)) in enumerate(zip(cases, classified)):
            e = dict(name=name, input=strs(inp), site=None if site is None else list(site))
            if i in errors:
                assert site is not None, f"{circuit} {name}: the WASM rejects what the oracle accepts: {errors[i]!r}"
                assert errors[i].startswith("Error: Assert Failed.\n"), errors[i]
                e["error"] = errors[i]
            else:
                assert site is None, f"{circuit} {name}: the WASM accepts what the oracle rejects at {site}"
                e["body_sha256"] = hashlib.sha256(bodies[i].tobytes()).hexdigest()
                assert e["body_sha256"] == T.sha256(obody), f"{circuit} {name}: accepted, but the oracle's body differs"
            out.append(e)
        A.site_texts(circuit, out)                       # one site, one text
        doc["circuits"][circuit] = dict(prime=str(cfg["prime"]), nwit=cfg["nwit"], wasm=cfg["wasm"], cases=out)
        nrej = sum("error" in e for e in out)
        print(f"{circuit}: {len(out)} cases, {nrej} rejected, {len({tuple(e['site']) for e in out if e['site']})} distinct sites")
    path = os.path.join(T.GOLD, A.FIXTURE)
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(doc, indent=0, sort_keys=True).encode())
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size <= MAX_BYTES, size


if __name__ == "__main__":
    main()
