"""The domain of b3w_batch_commit_device (bodies mode of b3w_commit_kernel, csrc/b3w_commit.hip) in plain integers: which bodies a
key accepts, which integer vector it commits to, and how many mixed point additions the launch costs.  Plain Python; of the product
only fold.py is used, for the relations behind folded keys.  Test infrastructure.

A body is a list of slot values, each the slot's 32 bytes taken as a little-endian 256-bit integer.  A key gives every slot a CLASS,
a function of the per-slot widths (tests/golden/slot_widths.json: b3w_slot_widths of the four builds), the key's first_slot, its fold
mask and — for keys with inverse tables — the slots of the 67 IsZero inverses:

    ("below",)       a slot under first_slot: never matters
    ("bit",)         in domain <=> value in {0, 1}
    ("w32",)         in domain <=> value < 2^32
    ("w64",)         in domain <=> value < 2^64
    ("w256",)        any value, values >= p included: the key commits to the 256-bit integer as it stands
    ("inverse", j)   like w256; its point may come from the table of (+-1/k) G instead of the windows (same point)
    ("folded",)      fold mask 1: any value, not read; commits 0
    ("onebit", i)    fold mask 0x80 | i: in domain <=> value < 2^32; commits bit i of the value

A body outside the domain gets status 103 and an unspecified point; a body inside it gets exactly sum committed[s] * G[s].
"""
import gzip
import importlib
import json
import os

import numpy as np

import b3w_testlib as T
import ec_ref as E

BELOW, BIT, W32, W64, W256, FOLDED = ("below",), ("bit",), ("w32",), ("w64",), ("w256",), ("folded",)
_BY_WIDTH = {1: BIT, 32: W32, 64: W64, 256: W256}
INV_NK = 2047                                   # |k| the key tabulates (+-1/k) G for (include/b3wit.h)
N_ISZERO = 67
M32, M64 = 1 << 32, 1 << 64


def slot_widths(circuit):
    """the fixture: b3w_slot_widths of the build, run-length encoded"""
    rle = json.load(open(os.path.join(T.GOLD, "slot_widths.json")))[circuit]
    out = []
    for w, n in rle:
        out += [w] * n
    assert len(out) == T.NWIT[circuit]
    return out


def classes(widths, first_slot=0, mask=None, inverse_slots=None):
    """-> one class per slot of the witness.  mask: per COMMITTED slot 0 kept, 1 folded away, 0x80 | i one bit of a word (or None);
    inverse_slots: {slot: gadget} for a key with inverse tables (or None)."""
    out = []
    for s, w in enumerate(widths):
        if s < first_slot:
            out.append(BELOW)
            continue
        mk = mask[s - first_slot] if mask is not None else 0
        if mk == 1:
            out.append(FOLDED)
        elif mk & 0x80:
            assert w == 32 and not mk & 0x60
            out.append(("onebit", mk & 31))
        elif inverse_slots and s in inverse_slots:
            assert w == 256 and mk == 0
            out.append(("inverse", inverse_slots[s]))
        else:
            assert mk == 0
            out.append(_BY_WIDTH[w])
    return out


def slot_in_domain(v, cls):
    assert 0 <= v < 1 << 256
    kind = cls[0]
    if kind == "bit":
        return v in (0, 1)
    if kind in ("w32", "onebit"):
        return v < M32
    if kind == "w64":
        return v < M64
    return True                                   # below, w256, inverse, folded


def in_domain(values, cls):
    return all(slot_in_domain(v, c) for v, c in zip(values, cls))


def slot_committed(v, cls):
    kind = cls[0]
    if kind in ("below", "folded"):
        return 0
    if kind == "onebit":
        return (v >> cls[1]) & 1
    return v


def committed(values, cls):
    """the integer vector an in-domain body is committed to, one entry per slot from first_slot on"""
    return [slot_committed(v, c) for v, c in zip(values, cls) if c != BELOW]


# ---- the bit string of phase 1, for the count of additions
def slot_bits(cls):
    """virtual slots of a class"""
    return {"below": 0, "bit": 1, "w32": 32, "w64": 64, "w256": 256, "inverse": 256, "folded": 0, "onebit": 1}[cls[0]]


def slot_packed(v, cls):
    """what a slot puts into the bit string, in or out of the domain: the low bits its class keeps.  For an in-domain body this is
    slot_committed; for a flagged one it is what phase 2 still adds up (the count of a flagged body is pinned with this)."""
    kind = cls[0]
    if kind == "bit":
        return v & 1
    if kind == "onebit":
        return (v >> cls[1]) & 1
    return v & ((1 << slot_bits(cls)) - 1)


def first_virtual(cls):
    """-> ([first virtual slot of every slot], total)"""
    out, v = [], 0
    for c in cls:
        out.append(v)
        v += slot_bits(c)
    return out, v


def gadget_args(inputs):
    """the 67 IsZero arguments from (n_blocks, block_count, total_depth, depth): include/b3wit.h at b3w_commit_records_device,
    circuits/blake3_nova.circom:19-23, 65-72, 136-144"""
    nb, bc, td, d = inputs
    return [-d, -bc, nb - 1 - bc] + [td - i - 2 - d for i in range(64)]


def tabulated_gadgets(values, cls, input_slots, p, inv_nk=INV_NK):
    """{gadget: slot} of the inverse slots whose point the key takes from its table: every one of the four input slots a plain 32-bit
    word, 0 < |k| <= inv_nk, and the slot equal to 1/k mod p (k < 0: p - 1/|k|)."""
    inv = {c[1]: s for s, c in enumerate(cls) if c[0] == "inverse"}
    if not inv or inv_nk == 0:
        return {}
    ins = [values[s] for s in input_slots]
    if any(v >= M32 for v in ins):
        return {}
    out = {}
    for j, k in enumerate(gadget_args(ins)):
        if j in inv and 0 < abs(k) <= inv_nk and values[inv[j]] == pow(k % p, -1, p):
            out[j] = inv[j]
    return out


def count_windows(string, window):
    """windows of `window` consecutive bits (from bit 0) that are not all zero"""
    raw = string.to_bytes((string.bit_length() + 7) // 8 + 1, "little")
    bits = np.unpackbits(np.frombuffer(raw, dtype=np.uint8), bitorder="little")
    bits = np.concatenate([bits, np.zeros(-len(bits) % window, dtype=np.uint8)])
    return int(bits.reshape(-1, window).any(axis=1).sum())


def bit_string(values, cls, skip=()):
    fv, _ = first_virtual(cls)
    s = 0
    for i, (v, c) in enumerate(zip(values, cls)):
        if i in skip:
            continue
        x = slot_packed(v, c) if c != BELOW else 0
        if x:
            s |= x << fv[i]
    return s


def expected_additions(values, cls, window, inv_nk=0, input_slots=None, p=None):
    """mixed point additions of phase 2 for this body: the non-zero windows of the packed bit string, with the bits of a slot whose
    point is tabulated left out, plus one per such slot"""
    tab = tabulated_gadgets(values, cls, input_slots, p, inv_nk) if inv_nk else {}
    return count_windows(bit_string(values, cls, skip=set(tab.values())), window) + len(tab)


# ---- generators A + i B and their folded forms as coefficient pairs
def generator_coefficients(nslots):
    """G[i] = 1 * A + i * B"""
    return [(1, i) for i in range(nslots)]


def r1cs_image(circuit):
    names = {"compression": "blake3_compression", "nova_bn254": "blake3_nova_bn254", "nova_vesta": "blake3_nova_vesta",
             "nova_bn254_o1": "blake3_nova_bn254_o1"}
    return gzip.open(os.path.join(T.PKG_DIR, "constraints", names[circuit] + ".r1cs.gz"), "rb").read()


_folds = {}


def folded_coefficients(circuit, widths, first_slot):
    """What fold.fold_generators does to the generators A + i B, in the exponents: -> (coefficient pairs mod the group order, one per
    committed slot, None where the slot is folded away; mask).  The relations come from fold.py (eliminate), the folding itself is
    restated here: G'[j] = G[j] + sum_k a_kj G[k] over the eliminated slots k; a one-bit word's slot gets sum of a_k,virtual G[k]."""
    key = (circuit, first_slot)
    if key in _folds:
        return _folds[key]
    fold = importlib.import_module("hot-proofs-blake3-circom_amd.fold")
    prime, n_wires, cons = fold.parse_r1cs(r1cs_image(circuit))
    assert n_wires == len(widths) and prime == T.PRIME[circuit]
    bow_rows, bit_of = fold.bit_of_word_relations(prime, n_wires, cons, widths)
    expr = fold.eliminate(prime, n_wires, fold.linear_relations(prime, cons) + bow_rows, widths, first_slot)
    bit_of = {W: i for W, i in bit_of.items() if W in expr and (n_wires + W) in expr[W]}
    nslots = n_wires - first_slot
    co = [[1, i] for i in range(nslots)]
    virt = {}
    for k, e in expr.items():
        rk = k - first_slot
        for j, a in e.items():
            tgt = virt.setdefault(j - n_wires, [0, 0]) if j >= n_wires else co[j - first_slot]
            tgt[0] = (tgt[0] + a) % prime
            tgt[1] = (tgt[1] + a * rk) % prime
    mask = bytearray(nslots)
    for k in expr:
        mask[k - first_slot] = 1
        co[k - first_slot] = None
    for W, i in bit_of.items():
        mask[W - first_slot] = 0x80 | i
        co[W - first_slot] = virt[W]
    _folds[key] = ([None if c is None else (c[0], c[1]) for c in co], mask)
    return _folds[key]


def scalars(values, cls, coeffs):
    """(a, b) with commitment = a A + b B, as integers (not reduced: a 256-bit slot may hold anything)"""
    a = b = 0
    for c, co in zip(committed(values, cls), coeffs):
        if c:
            a += c * co[0]
            b += c * co[1]
    return a, b


_pow2 = {}


def point(curve, a, b):
    """a A + b B for the two points behind ec_ref.related_points (tables of 2^k A, 2^k B: a multiplication is its additions alone)"""
    p, _ = E.CURVES[curve]
    if curve not in _pow2:
        tabs = []
        for P in E.random_points(curve, 2):
            t = [P]
            for _ in range(320):
                t.append(E.add(t[-1], t[-1], p))
            tabs.append(t)
        _pow2[curve] = tabs
    acc = None
    for k, t in zip((a, b), _pow2[curve]):
        assert 0 <= k < 1 << 320
        i = 0
        while k:
            if k & 1:
                acc = E.add(acc, t[i], p)
            k >>= 1
            i += 1
    return acc
