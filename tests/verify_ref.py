"""The tamper check (b3w_batch_verify_device, include/b3wit.h) restated on the CPU, and the planting plans the tests of it share.
numpy and the oracle only; no torch.  Test infrastructure.

    in_slots(circuit)          slot of each record word: the first `W slot atom len` run of layouts/<circuit>.layout, in file order, that
                               holds the word's atom (the rule of build_input_slots, csrc/b3w_ctx.cpp)
    copy_slots(circuit)        [(record word, slot)] of every OTHER whole-word slot that holds an input atom
    verify_ref(circuit, body)  what d_mismatch must say of this body, as one integer

A body is a uint8 array of nwit * 32 bytes; a UNIT is 16 bytes (unit u = half u & 1 of slot u >> 1) and has four 32-bit words.
A plant is (unit, word, bit): XOR that bit.  Everything below the reference is a fixed plan — no RNG except the seeded one of
attribution_plan — so the CPU tests can prove what the GPU tests then only execute."""
import os

import numpy as np

import b3w_testlib as T
import record_domain_cases as C

REJECTED = 0xFFFFFFFF
FIRST_ATOM = {"compression": 1, "nova_bn254": 941, "nova_vesta": 941, "nova_bn254_o1": 941}      # B3W_A_H, B3W_A_NV (csrc/b3w_atoms.h)
MOD = 17                       # residue classes of the sweep: coprime to the 64 lanes and 32 slots of a tile
N_EDGE = 37                    # bodies of the edge and attribution launches: ragged for every W and stride
PADS = (0, 32, 64, 96)         # pitch = body + pad
BASES = (0, 16, 32, 64, 96)    # body 0 starts this far into a 256-byte aligned buffer

_w_runs = {}


def _whole_word_runs(circuit):
    """[(slot, atom, len)] of the layout's W runs, in file order"""
    if circuit not in _w_runs:
        runs = []
        with open(os.path.join(T.LAYOUTS, circuit + ".layout")) as f:
            for line in f:
                p = line.split()
                if p and p[0] == "W":
                    runs.append((int(p[1]), int(p[2]), int(p[3])))
        _w_runs[circuit] = runs
    return _w_runs[circuit]


def in_slots(circuit):
    first, nin = FIRST_ATOM[circuit], T.NIN[circuit]
    slots = [None] * nin
    for slot, atom, ln in _whole_word_runs(circuit):
        for k in range(ln):
            j = atom + k - first
            if 0 <= j < nin and slots[j] is None:
                slots[j] = slot + k
    assert None not in slots, (circuit, slots)
    return np.array(slots, dtype=np.int64)


def copy_slots(circuit):
    first, nin, own = FIRST_ATOM[circuit], T.NIN[circuit], in_slots(circuit)
    out = []
    for slot, atom, ln in _whole_word_runs(circuit):
        for k in range(ln):
            j = atom + k - first
            if 0 <= j < nin and slot + k != own[j]:
                out.append((j, slot + k))
    return out


def record_of(circuit, body):
    """the record a body's input slots spell, or None where one of them is not a plain 32-bit value (bytes 4..31 not all zero)"""
    b = np.asarray(body, dtype=np.uint8).reshape(T.NWIT[circuit], 32)[in_slots(circuit)]
    if b[:, 4:].any():
        return None
    return np.ascontiguousarray(b[:, :4]).view("<u4").reshape(-1).astype(np.uint32)


def verify_ref(circuit, body):
    body = np.asarray(body, dtype=np.uint8).reshape(-1)
    assert body.size == T.NWIT[circuit] * 32
    rec = record_of(circuit, body)
    if rec is None:
        return REJECTED
    if circuit != "compression" and C.classify(rec) in ("assert", "domain"):
        return REJECTED
    rc, want = T.oracle_each_u32(circuit, rec[None, :])
    assert rc[0] == 0, (circuit, rec, int(rc[0]))                # canonical words the rule accepts: the oracle has a body
    return int((body.reshape(-1, 16) != want[0].reshape(-1, 16)).any(axis=1).sum())


# ---- planting

def n_units(circuit):
    return 2 * T.NWIT[circuit]


def input_units(circuit):
    """the (at most 64) units of in_slots: the only ones the sweep, the edge list and the attribution plan leave alone"""
    s = in_slots(circuit)
    return np.unique(np.concatenate([2 * s, 2 * s + 1]))


def plant(body, unit, word, bit):
    """XOR one bit of word `word` of unit `unit`, in place"""
    assert 0 <= word < 4 and 0 <= bit < 32 and 0 <= unit < body.size // 16
    body.reshape(-1).view("<u4")[4 * unit + word] ^= np.uint32(1 << bit)


def sweep_units(circuit, r):
    u = np.arange(r, n_units(circuit), MOD, dtype=np.int64)
    return u[~np.isin(u, input_units(circuit))]


def sweep_bits(units, word):
    return (5 * (np.asarray(units) // MOD) + 11 * word + 1) % 32


def plant_sweep(circuit, body, r, word):
    """body 4 r + word of the sweep: every unit = r (mod 17) outside in_slots, bit sweep_bits of that word; -> units planted"""
    u = sweep_units(circuit, r)
    body.reshape(-1).view("<u4")[4 * u + word] ^= (np.uint32(1) << sweep_bits(u, word).astype(np.uint32))
    return int(u.size)


# ---- the tiling of expand_verify (csrc/b3w_kernels.hip) and its edges

def tile_j(addr):
    """a body that starts at byte address `addr`: its tile k covers slots [32 k - j, 32 k - j + 32)"""
    return 0 if addr & 31 else (addr >> 5) & 3


def n_tiles(circuit, j):
    return (T.NWIT[circuit] + j + 31) >> 5


def edge_slots(circuit, j):
    nwit, nt = T.NWIT[circuit], n_tiles(circuit, j)
    tail = 128 * ((nt - 1) // 4) - j                 # first slot of the last iteration of four tiles (clamped unless nt = 0 mod 4)
    last = 32 * (nt - 1) - j                         # first slot of the last tile
    cand = [0, 1, 31 - j, 32 - j, 127 - j, 128 - j, tail - 1, tail, last - 1, last, nwit - 2, nwit - 1]
    own = set(int(s) for s in in_slots(circuit))
    return sorted({s for s in cand if 0 <= s < nwit and s not in own})


def edge_units(circuit, j):
    return [2 * s + h for s in edge_slots(circuit, j) for h in (0, 1)]


def body_addresses(circuit, pad, base, n=N_EDGE):
    pitch = T.NWIT[circuit] * 32 + pad
    return [base + i * pitch for i in range(n)]


def edge_plan(circuit):
    """[(pad, base, launches)], launches = three lists of (body, unit, word, bit): in launch l the bodies i = l (mod 3) are victims, one
    plant each, every other body is clean — so every wave (bodies 1, 2 or 4 apart) mixes victims and clean bodies, and every body,
    body n - 1 and the last active body of every ragged wave among them, is a victim once per configuration.  The unit comes from the
    edge list of the body's own j, in rotation over the whole plan."""
    cursor = [0, 0, 0, 0]
    plan = []
    for pad in PADS:
        for base in BASES:
            addr = body_addresses(circuit, pad, base)
            launches = []
            for l in range(3):
                plants = []
                for i in range(l, N_EDGE, 3):
                    j = tile_j(addr[i])
                    units = edge_units(circuit, j)
                    c = cursor[j]
                    cursor[j] += 1
                    plants.append((i, units[c % len(units)], (c // len(units)) % 4, (7 * c + 3) % 32))
                launches.append(plants)
            plan.append((pad, base, launches))
    return plan


def attribution_plan(circuit, n=N_EDGE, seed=20250117):
    """body i gets i plants in i distinct units outside in_slots, at seeded random places"""
    rng = np.random.default_rng(seed + T.CIRCUIT_ID[circuit])
    free = np.setdiff1d(np.arange(n_units(circuit)), input_units(circuit))
    return [[(int(u), int(rng.integers(0, 4)), int(rng.integers(0, 32))) for u in rng.choice(free, size=i, replace=False)] for i in range(n)]


# ---- input atoms

def input_cases(circuit):
    """[(kind, record word, slot, word of the slot 0..7, xor mask)] — one 32-bit XOR each, into a body whose input slots are plain words:
      "low"    bit 0 and bit 31 of the low word of in_slots[j]: another record; its exact count, or REJECTED where it is refused
      "upper"  word 1, word 3 and one byte of the upper half of in_slots[j] set: not a plain 32-bit value, REJECTED
      "copy"   bit 0 / bit 31 (in turn) of every other whole-word slot that holds an input atom: the record stands, exactly 1"""
    cases = []
    for j, s in enumerate(in_slots(circuit)):
        s = int(s)
        cases += [("low", j, s, 0, 1), ("low", j, s, 0, 1 << 31),
                  ("upper", j, s, 1, 1), ("upper", j, s, 3, 1 << 16), ("upper", j, s, 4 + j % 4, 0x5A << (8 * ((j // 4) % 4)))]
    for n, (j, s) in enumerate(copy_slots(circuit)):
        cases.append(("copy", j, s, 0, 1 << 31 if n % 2 else 1))
    return cases


def apply_case(body, case):
    _kind, _j, slot, word, mask = case
    body.reshape(-1).view("<u4")[8 * slot + word] ^= np.uint32(mask)


def base_records(circuit):
    """{name: record} the input cases are planted into: one compression record, or of config3_nova(64) the first parent step and the
    first leaf step with an odd depth — bit 0 of its depth or leaf_depth flipped makes a parent step, bit 31 a step the circuit rejects"""
    W = T.workloads()
    if circuit == "compression":
        return {"compression": W.config2_compression(64)[5].copy()}
    recs = W.config3_nova(64)
    leaf = next(r for r in recs if not C.is_parent(r) and int(r[C.DEPTH]) & 1)
    parent = next(r for r in recs if C.is_parent(r))
    return {"leaf": leaf.copy(), "parent": parent.copy()}
