"""Foreign bodies for b3w_batch_commit_device as a fixed table: every case is one base body with a few slots
replaced and a verdict WRITTEN DOWN BY HAND, family by family (0 = committed, 103 = outside the key's domain).  The rule in closed
form is tests/commit_domain_ref.py (in_domain); tests/test_commit_domain_cpu.py holds the two against each other, and
tests/test_gpu_commit_domain.py holds the kernel to the table.  Data plus a builder: numpy only, no RNG.  Test infrastructure.

Base bodies are the oracle's: two per circuit (nova: a leaf step and a parent step with depth > 0, so that negative IsZero arguments
occur, plus one whose record puts eqs[i] = 2 049 - i: both sides of the 2 047-entry table of inverse points), the all-zero body and
the all-ones body (every bit slot 1, every wider slot at the maximum of its width).

Where the kernel goes another way for a slot is derived here from first_slot, the lanes per witness T and the class sequence, as
b3w_commit_kernel does it: committed slots are taken in groups of T; a group whose T slots are all bit slots goes through one ballot
(the FAST road), any other group slot by slot (the SLOW road); a step of the outer loop covers 8 T slots.
"""
import numpy as np

import b3w_testlib as T
import commit_domain_ref as R

_W = T.workloads()
U = 8                                            # groups per step of the kernel's outer loop
NB, BC, LD, TD, DEPTH = 0, 1, 12, 13, 14
M32, M64 = 1 << 32, 1 << 64

BIT_VIOLATIONS = [("2", 2), ("3", 3), ("2^31", 1 << 31), ("2^32-1", M32 - 1)] + \
                 [(f"1+2^{32 * j}", 1 + (1 << 32 * j)) for j in range(1, 8)] + [(f"2^{32 * j}", 1 << 32 * j) for j in range(1, 8)]
W32_VIOLATIONS = [(f"2^{32 * j}", 1 << 32 * j) for j in range(1, 8)] + [("2^32-1+2^32", M32 - 1 + M32)]
W64_VIOLATIONS = [(f"2^{32 * j}", 1 << 32 * j) for j in range(2, 8)]
W32_INSIDE = [("0", 0), ("1", 1), ("2^31", 1 << 31), ("2^32-1", M32 - 1)]
W64_INSIDE = [("2^34-1", (1 << 34) - 1), ("2^34", 1 << 34), ("2^63", 1 << 63), ("2^64-1", M64 - 1)]


def lanes_per_witness(virtual_bits, window, n):
    """b3w_launch_commit's choice of T (without B3W_COMMIT_THREADS): the 18-bit table always 64; else 64 for more than 55 200 virtual
    bits (windows included) or 8 192 bodies and more, 32 below"""
    nwin = -(-virtual_bits // window)
    return 64 if window == 18 or nwin * window > 55200 or n >= 8192 else 32


def _values(body):
    b = np.ascontiguousarray(body).reshape(-1, 32)
    raw = b.tobytes()
    return [int.from_bytes(raw[32 * s:32 * s + 32], "little") for s in range(b.shape[0])]


def _body(values):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), dtype=np.uint8).copy()


_base_cache = {}


def bases(circuit):
    """-> dict: names, values (list of slot-value lists), records (or None per base), and for the O2 nova builds input_slots
    (n_blocks, block_count, total_depth, depth: the lowest slot that holds the record's word in every probe) and inverse_slots
    {slot: gadget} — both found by their VALUES in the oracle's bodies, not through a layout."""
    if circuit in _base_cache:
        return _base_cache[circuit]
    widths = R.slot_widths(circuit)
    p = T.PRIME[circuit]
    out = {"widths": widths, "input_slots": None, "inverse_slots": None}
    if circuit == "compression":
        recs = _W.config2_compression(2, first=11)
        names = ["oracle0", "oracle1"]
    else:
        r = _W.config3_nova(64, first=7)
        edge = r[0].copy()
        edge[TD] = 2049 + int(edge[DEPTH]) + 2                   # eqs[i] = 2 049 - i: 2 049, 2 048, 2 047, ...
        assert int(r[0][LD]) - int(r[0][DEPTH]) == 1 and int(r[2][LD]) - int(r[2][DEPTH]) >= 2 and int(r[0][DEPTH]) > 0 and int(r[2][DEPTH]) > 0
        recs = np.stack([r[0], r[2], edge] + [r[i] for i in range(3, 12)])
        names = ["leaf", "parent", "edge2049"]
    bad, bodies = T.oracle_batch_u32(circuit, recs)
    assert bad == 0
    vals = [_values(bodies[i]) for i in range(len(recs))]
    if circuit in ("nova_bn254", "nova_vesta"):
        def holds(col):
            return [s for s in range(1, 48) if all(vals[i][s] == int(recs[i][col]) for i in range(len(recs)))]
        ins = [holds(c) for c in (NB, BC, TD, DEPTH)]
        assert all(ins), ins
        out["input_slots"] = [h[0] for h in ins]
        out["input_copies"] = ins
        wide = [s for s, w in enumerate(widths) if w == 256]
        assert len(wide) == R.N_ISZERO
        inv = {}
        for j in range(R.N_ISZERO):
            cand = set(wide)
            for i in range(len(recs)):
                k = R.gadget_args([int(recs[i][c]) for c in (NB, BC, TD, DEPTH)])[j]
                want = pow(k % p, -1, p) if k % p else 0
                cand &= {s for s in wide if vals[i][s] == want}
            assert len(cand) == 1, (j, cand)
            inv[cand.pop()] = j
        assert len(inv) == R.N_ISZERO
        out["inverse_slots"] = inv
    keep = len(names)
    ones = [{1: 1, 32: M32 - 1, 64: M64 - 1, 256: (1 << 256) - 1}[w] for w in widths]
    out["names"] = names + ["zeros", "ones"]
    out["values"] = vals[:keep] + [[0] * len(widths), ones]
    out["records"] = [recs[i] for i in range(keep)] + [None, None]
    _base_cache[circuit] = out
    return out


def road(cls, first_slot, t, slot):
    """"fast" or "slow" for a committed slot: its group of T committed slots is all bit slots (and complete), or not"""
    rel = slot - first_slot
    g0 = first_slot + rel - rel % t
    grp = cls[g0:g0 + t]
    return "fast" if len(grp) == t and all(c == R.BIT for c in grp) else "slow"


def sweep_slots(cls, first_slot, t):
    """-> {kind: [slots]}: per class the first and the last committed slot, one on each side of the first two multiples of T * U from
    first_slot; for bit slots two slots of a fast group (a lower and an upper lane), the first and the last slow one."""
    by = {}
    for s, c in enumerate(cls):
        if c != R.BELOW:
            by.setdefault(c[0], []).append(s)
    out = {}
    for kind, sl in by.items():
        pick = [sl[0], sl[-1]]
        for b in (first_slot + t * U, first_slot + 2 * t * U):
            lo = [s for s in sl if s < b]
            hi = [s for s in sl if s >= b]
            pick += lo[-1:] + hi[:1]
        if kind == "bit":
            fast = [s for s in sl if road(cls, first_slot, t, s) == "fast"]
            slow = [s for s in sl if road(cls, first_slot, t, s) == "slow"]
            g = next((s for s in fast if (s - first_slot) % t == 0 and all(c == R.BIT for c in cls[s:s + 64])), None)
            if g is not None:                                   # (a narrow key may have no group of T bit slots at all)
                pick += [g + 5, g + t - 3, fast[-1]]
            pick += [slow[0], slow[-1]]
            short = [s for s in slow if cls[s - 1] != R.BIT and cls[s + 1:s + 2] != [R.BIT]]
            pick += short[:1] + short[-1:]                       # a run of one bit slot between wider ones
        out[kind] = sorted(set(pick))
    return out


_tables = {}


def table(circuit, first_slot=0, fold=False, tables=False, t=64):
    """-> dict(cls, bases, cases, sweep, ...).  cases: [(name, base index, {slot: value}, verdict)].  tables: the key has inverse
    tables (an O2 nova build on the curve whose order is its prime)."""
    key = (circuit, first_slot, fold, tables, t)
    if key in _tables:
        return _tables[key]
    b = bases(circuit)
    widths, p = b["widths"], T.PRIME[circuit]
    mask = coeffs = None
    if fold:
        coeffs, mask = R.folded_coefficients(circuit, widths, first_slot)
    else:
        coeffs = R.generator_coefficients(len(widths) - first_slot)
    cls = R.classes(widths, first_slot, mask, b["inverse_slots"] if tables else None)
    sweep = sweep_slots(cls, first_slot, t)
    nbase = len(b["names"])
    oracle = [i for i in range(nbase) if b["records"][i] is not None]
    cases, turn = [], [0]

    def add(name, base, edits, verdict):
        cases.append((f"{name} [{b['names'][base]}]", base, dict(edits), verdict))

    def nxt():                                                # the oracle bases in turn
        turn[0] += 1
        return oracle[turn[0] % len(oracle)]
    # ---- violations: verdict 103, every one of them
    # (every other sweep slot of a class takes its values in reverse: a word position then falls on an even and on an odd body)
    for q, s in enumerate(sweep.get("bit", [])):
        rd = road(cls, first_slot, t, s)
        for nm, v in BIT_VIOLATIONS[::-1 if q % 2 else 1]:
            add(f"bit slot {s} ({rd}) = {nm}", nxt(), {s: v}, 103)
    for kind in ("w32", "onebit"):
        for q, s in enumerate(sweep.get(kind, [])):
            for nm, v in W32_VIOLATIONS[::-1 if q % 2 else 1]:
                add(f"{kind} slot {s} = {nm}", nxt(), {s: v}, 103)
    for q, s in enumerate(sweep.get("w64", [])):
        for nm, v in W64_VIOLATIONS[::-1 if q % 2 else 1]:
            add(f"w64 slot {s} = {nm}", nxt(), {s: v}, 103)
    s0 = sweep["bit"][0]                                      # (kept for the end of the launch: its last body is a violation)
    last = (f"bit slot {s0} = 2 in the last body [{b['names'][oracle[0]]}]", oracle[0], {s0: 2}, 103)
    # ---- foreign bodies inside the domain: verdict 0, every one of them
    for i in range(nbase):
        add("as it stands", i, {}, 0)
    for s in sweep.get("bit", []):
        i = nxt()
        add(f"bit slot {s} ({road(cls, first_slot, t, s)}) flipped", i, {s: 1 - b["values"][i][s]}, 0)
    for s in sweep.get("w32", []):
        for nm, v in W32_INSIDE:
            add(f"w32 slot {s} = {nm}", nxt(), {s: v}, 0)
    for s in sweep.get("w64", []):
        for nm, v in W64_INSIDE:
            add(f"w64 slot {s} = {nm}", nxt(), {s: v}, 0)
    for kind in ("w256", "inverse"):
        for s in sweep.get(kind, []):
            for nm, v in (("0", 0), ("1", 1), ("p-1", p - 1), ("p", p), ("2^255", 1 << 255), ("2^256-1", (1 << 256) - 1)):
                add(f"{kind} slot {s} = {nm}", nxt(), {s: v}, 0)
    for s in sweep.get("folded", []):                         # a word that is not the sum of its bits, under mask 1: not read
        i = nxt()
        add(f"folded slot {s} + 1", i, {s: b["values"][i][s] + 1}, 0)
        add(f"folded slot {s} = 2^256-1", nxt(), {s: (1 << 256) - 1}, 0)
        add(f"folded slot {s} = 2^200", nxt(), {s: 1 << 200}, 0)
    for s in sweep.get("onebit", []):                         # mask 0x80 | i: bit i set and clear, the other bits anything
        i = cls[s][1]
        for nm, v in (("all but bit i", (M32 - 1) ^ (1 << i)), ("all", M32 - 1), ("bit i alone", 1 << i), ("0x5A5A5A5A without bit i", 0x5A5A5A5A & ~(1 << i)),
                      ("0", 0)):
            add(f"onebit slot {s} (i = {i}) = {nm}", nxt(), {s: v}, 0)
    if first_slot > 0:                                        # slots below first_slot never matter
        for i in oracle[:2]:
            add("garbage below first_slot", i, {s: (1 << 200) + s * (M32 + 1) + 7 for s in range(first_slot)}, 0)
    if tables:                                                # bodies mode of a key with inverse tables: point and count
        ins, inv = b["input_slots"], {j: s for s, j in b["inverse_slots"].items()}
        d_slot = ins[3]
        edge = b["names"].index("edge2049")
        leaf = b["names"].index("leaf")
        if all(s >= first_slot for s in inv.values()):
            i12 = pow(2049 - 10, -1, p)                           # eqs[10] of the edge body: k = +2 039
            assert b["values"][edge][inv[3 + 10]] == i12
            add("eqs[10]: p - 1/k for k = +2039 (the wrong sign)", edge, {inv[3 + 10]: p - i12}, 0)
            add("eqs[2]: 1/k + 1 at k = +2047", edge, {inv[3 + 2]: pow(2047, -1, p) + 1}, 0)
            for k in (2047, 2048):                                # root = IsZero(-depth): a negative argument at the table's edge
                add(f"depth = {k}, root inverse = p - 1/{k}", leaf, {d_slot: k, inv[0]: p - pow(k, -1, p)}, 0)
                add(f"depth = {k}, root inverse = 1/{k} (the wrong sign)", leaf, {d_slot: k, inv[0]: pow(k, -1, p)}, 0)
            add("depth = 0, root inverse = 0", leaf, {d_slot: 0, inv[0]: 0}, 0)
            add("depth = 0, root inverse = 1", leaf, {d_slot: 0, inv[0]: 1}, 0)
            add("depth = 2^32 (no word), root inverse as it stands", leaf, {d_slot: M32}, 103 if d_slot >= first_slot else 0)
    while (len(cases) + 1) % 4 != 3:                          # launches of 4k + 3, 4k + 2 and 4k + 1 bodies: the table and two prefixes
        add(f"as it stands (padding {len(cases)})", oracle[0], {}, 0)
    cases.append(last)
    out = dict(b, circuit=circuit, first_slot=first_slot, fold=fold, tables=tables, t=t, cls=cls, mask=mask, coeffs=coeffs, sweep=sweep,
               cases=cases, p=p)
    _check_coverage(out)
    _tables[key] = out
    return out


def case_values(tab, case):
    v = list(tab["values"][case[1]])
    for s, x in case[2].items():
        v[s] = x
    return v


def _check_coverage(tab):
    """every class x word position x road the table is meant to reach occurs in a violation; the first and the last case are
    violations; every one of them sits in an even and in an odd body of the launch (the two halves of a two-witness wave)"""
    cls, fs, t, cases = tab["cls"], tab["first_slot"], tab["t"], tab["cases"]
    seen, halves = set(), set()                                # halves: (class, road, word position, parity of the body)
    for idx, (name, base, edits, verdict) in enumerate(cases):
        if verdict != 103 or len(edits) != 1:
            continue
        (s, v), = edits.items()
        kind = cls[s][0]
        rd = road(cls, fs, t, s) if kind == "bit" else "slow"
        for j in range(8):
            if (v >> 32 * j) & (M32 - 1):
                seen.add((kind, rd, j))
                halves.add((kind, rd, j, idx % 2))
    kinds = {c[0] for c in cls}
    need = set()
    has_fast = any(c == R.BIT and road(cls, fs, t, s) == "fast" for s, c in enumerate(cls))
    if "bit" in kinds:
        need |= {("bit", rd, j) for rd in (("fast", "slow") if has_fast else ("slow",)) for j in range(8)}
    need |= {(k, "slow", j) for k in ("w32", "onebit") if k in kinds for j in range(1, 8)}
    if "w64" in kinds:
        need |= {("w64", "slow", j) for j in range(2, 8)}
    assert need <= seen, sorted(need - seen)
    assert cases[0][3] == 103 and cases[-1][3] == 103 and len(cases) % 4 == 3
    missing = sorted(k + (h,) for k in need for h in (0, 1) if k + (h,) not in halves)
    assert not missing, missing
    assert len({n for n, *_ in cases}) == len(cases)          # a failure names its case


def bodies_plan(tab):
    """what the device needs to make the launch: base bodies uint8 [nbase, nwit * 32], base index per case, and the edits as three
    arrays (case, slot, 32 bytes)"""
    base = np.stack([_body(v) for v in tab["values"]])
    idx = np.array([c[1] for c in tab["cases"]], dtype=np.int64)
    ci, si, raw = [], [], []
    for k, (_, _, edits, _) in enumerate(tab["cases"]):
        for s, v in edits.items():
            ci.append(k); si.append(s); raw.append(v.to_bytes(32, "little"))
    return base, idx, np.array(ci, dtype=np.int64), np.array(si, dtype=np.int64), np.frombuffer(b"".join(raw), dtype=np.uint8).reshape(-1, 32).copy()


def reference_scalars(tab, reduce=True):
    """per case (a, b) with commitment = a A + b B (None where the verdict is 103): the base body's sums, corrected by the case's slots"""
    cls, coeffs, fs = tab["cls"], tab["coeffs"], tab["first_slot"]
    order = tab["p"] if tab["fold"] else None                 # (a folded key exists only on the curve whose order is the prime)
    base = [R.scalars(v, cls, coeffs) for v in tab["values"]]
    out = []
    for name, bi, edits, verdict in tab["cases"]:
        if verdict == 103:
            out.append(None)
            continue
        a, b = base[bi]
        for s, v in edits.items():
            if s < fs or coeffs[s - fs] is None:
                continue
            d = R.slot_committed(v, cls[s]) - R.slot_committed(tab["values"][bi][s], cls[s])
            a += d * coeffs[s - fs][0]
            b += d * coeffs[s - fs][1]
        out.append((a % order, b % order) if order else (a, b))
    return out


def reference_additions(tab, window):
    """sum over ALL cases (flagged ones too: phase 2 runs for them, on the low bits their slots' classes keep) of expected_additions,
    and the list per case"""
    cls = tab["cls"]
    fv, _ = R.first_virtual(cls)
    strings = [R.bit_string(v, cls) for v in tab["values"]]
    per = []
    for case in tab["cases"]:
        name, bi, edits, verdict = case
        s = strings[bi]
        for sl, v in edits.items():
            if cls[sl] != R.BELOW:
                s ^= (R.slot_packed(tab["values"][bi][sl], cls[sl]) ^ R.slot_packed(v, cls[sl])) << fv[sl]
        ntab = 0
        if tab["tables"]:
            vals = _Overlay(tab["values"][bi], edits)
            tabd = R.tabulated_gadgets(vals, cls, tab["input_slots"], tab["p"])
            for sl in tabd.values():
                s &= ~(((1 << 256) - 1) << fv[sl])
            ntab = len(tabd)
        per.append(R.count_windows(s, window) + ntab)
    return sum(per), per


class _Overlay:
    def __init__(self, base, edits):
        self.base, self.edits = base, edits

    def __getitem__(self, s):
        return self.edits.get(s, self.base[s])


# ---- the keys the table is run under: (name, circuit, curve, first_slot, window, folded, bodies of the large launch or 0).  They are
# chosen so that every instantiation b3w_launch_commit can take — {T 32 generic, T 64 generic, T 64 Vesta} x {12, 16 bits} and
# {T 64 generic, T 64 Vesta} at 18 bits — is reached at the smallest shape (tests/test_gpu_commit_domain.py).
KEYS = [
    ("compression-w12", "compression", "bn254_g1", 0, 12, False, 0),
    ("compression-w16-from17", "compression", "bn254_g1", 17, 16, False, 0),
    ("compression-pallas-from45", "compression", "pallas", 45, 12, False, 0),
    ("compression-w18-narrow", "compression", "bn254_g1", 21000, 18, False, 0),
    ("compression-w12-8195", "compression", "bn254_g1", 0, 12, False, 8192 + 3),
    ("nova_bn254-w12", "nova_bn254", "bn254_g1", 0, 12, False, 0),
    ("nova_bn254-w16", "nova_bn254", "bn254_g1", 0, 16, False, 0),
    ("nova_vesta-w12", "nova_vesta", "pallas", 0, 12, False, 0),
    ("nova_vesta-w16", "nova_vesta", "pallas", 0, 16, False, 0),
    ("nova_vesta-w18-narrow", "nova_vesta", "pallas", 22950, 18, False, 0),
    ("nova_vesta-on-bn254-narrow", "nova_vesta", "bn254_g1", 22950, 12, False, 0),
    ("nova_vesta-folded", "nova_vesta", "pallas", 0, 12, True, 0),
    ("compression-folded", "compression", "bn254_g1", 0, 12, True, 0),
    ("nova_bn254_o1-w12", "nova_bn254_o1", "bn254_g1", 0, 12, False, 0),
]
ORDER_IS_PRIME = {("compression", "bn254_g1"), ("nova_bn254", "bn254_g1"), ("nova_bn254_o1", "bn254_g1"), ("nova_vesta", "pallas")}


def key_table(name):
    """-> (the KEYS row, its table, T of the table's launches, whether the key has inverse tables)"""
    # (a key with a large launch: T, and with it the sweep and the "(fast)" / "(slow)" of the case names, is that of the LARGE launch;
    # the table's own launches of a few hundred bodies run with the T of a small one, where the labels name the other grouping)
    row = next(k for k in KEYS if k[0] == name)
    _, circuit, curve, first_slot, window, fold, n_large = row
    widths = R.slot_widths(circuit)
    mask = R.folded_coefficients(circuit, widths, first_slot)[1] if fold else None
    _, vbits = R.first_virtual(R.classes(widths, first_slot, mask))
    tables = circuit in ("nova_bn254", "nova_vesta") and (circuit, curve) in ORDER_IS_PRIME
    t = lanes_per_witness(vbits, window, n_large or 1)
    return row, table(circuit, first_slot, fold, tables, t), t, tables
