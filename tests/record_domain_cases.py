"""The edges of the batch kernels' record domain as a fixed table.  Data plus a tiny builder: numpy only, no
torch, no RNG when the table is built.  Test infrastructure.

    nova_rows()        -> [(name, record uint32[32], expect)]
    compression_rows() -> [(name, record uint32[28], expect)]

expect: "ok"      the circuit accepts the record and the batch kernels compute its witness (status 0);
        "assert"  the circuit rejects it: Blake3NovaTreePath_CheckDepth (circuits/blake3_nova.circom:13-45), status 4;
        "domain"  the circuit accepts it, the batch kernels do not compute it (status 103; the exact kernel does).

Every row starts from one leaf step or one parent step of config3_nova(64, first=7) (records 0 and 2), or from record 0 of
config2_compression, and changes only the fields its name says, so a failure names its field.  A row's `expect` is written
down by hand, family by family; classify() restates the rule in closed form and tests/test_record_domain_cpu.py holds the two
against each other and against the oracle.

The rule, with M = 2^32 and all differences taken in the integers:
  assert  <=>  not (1 <= leaf_depth - depth <= 256)                         (LessThan(8) / GreaterEqThan(8) over Num2Bits(9))
  parent  <=>  leaf_depth - depth >= 2
  domain  <=>  accepted, and one of
                 |n_blocks - 1 - block_count| >= M       (an IsZero argument the kernels' inverse does not take)
                 |istar| >= M  or  |istar - 63| >= M     (istar = total_depth - 2 - depth; eqs[i] takes istar - i, i = 0..63)
                 block_count = M - 1 on a leaf step      (block_count_out = block_count + 1 is no 32-bit word)
               (depth = M - 1, whose depth + 1 is no word either, is never accepted: leaf_depth <= M - 1.)
"""
import numpy as np

import b3w_testlib as T

_W = T.workloads()

M = 1 << 32
K_EDGES = (1, 2046, 2047, 2048, 2049, 65535, 65536, M - 2, M - 1)       # both sides of the 2 048-entry table of inverses, and the top
ISTARS = (-2, -1, 0, 1, 30, 31, 32, 33, 62, 63, 64, 65)
CHUNK_IDX = ((0x80000001, 0x80000001), (0x7FFFFFFE, 0x7FFFFFFE), (0xFFFFFFFF, 0), (0, 0xFFFFFFFF))   # (high, low)

NB, BC, H, CIL, CIH, LD, TD, DEPTH, MSG, B = 0, 1, 2, 10, 11, 12, 13, 14, 15, 31
_FIELD = {"n_blocks": NB, "block_count": BC, "cil": CIL, "cih": CIH, "leaf_depth": LD, "total_depth": TD, "depth": DEPTH, "b": B}

# fixed words for the rows that want "some" non-zero message half
_FILL8 = (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0, 0x082EFA98, 0xEC4E6C89)


def _bases():
    r = _W.config3_nova(64, first=7)
    leaf, parent = r[0].copy(), r[2].copy()
    assert int(leaf[LD]) - int(leaf[DEPTH]) == 1 and int(parent[LD]) - int(parent[DEPTH]) >= 2
    return {"leaf": leaf, "parent": parent}


def _edit(base, **f):
    r = base.copy()
    for k, v in f.items():
        if k == "h":
            r[H:H + 8] = np.array(v, dtype=np.uint64).astype(np.uint32)
        elif k == "m":
            r[MSG:MSG + 16] = np.array(v, dtype=np.uint64).astype(np.uint32)
        else:
            assert 0 <= v < M, (k, v)
            r[_FIELD[k]] = v
    return r


def ks(rec):
    """the 67 IsZero arguments of a step as integers: {"root": -depth, "e0": -block_count, "e1": n_blocks - 1 - block_count,
    "eq": [total_depth - i - 2 - depth for i < 64]} (circuits/blake3_nova.circom:19-23, 136-144, 65-72)"""
    nb, bc, td, d = int(rec[NB]), int(rec[BC]), int(rec[TD]), int(rec[DEPTH])
    return {"root": -d, "e0": -bc, "e1": nb - 1 - bc, "eq": [td - i - 2 - d for i in range(64)]}


def is_parent(rec):
    return int(rec[LD]) - int(rec[DEPTH]) >= 2


def classify(rec):
    """the closed-form rule of the module docstring"""
    diff = int(rec[LD]) - int(rec[DEPTH])
    if not 1 <= diff <= 256:
        return "assert"
    k = ks(rec)
    if abs(k["e1"]) >= M or abs(k["eq"][0]) >= M or abs(k["eq"][63]) >= M:
        return "domain"
    if int(rec[BC]) == M - 1 and not is_parent(rec):
        return "domain"
    return "ok"


def nova_rows():
    base = _bases()
    rows = []

    def add(name, kind, expect, **f):
        rows.append((f"{name}/{kind}", _edit(base[kind], **f), expect))

    def kind_depths(kind, depth):
        """leaf_depth that makes `depth` a leaf step (+1) or a parent step (+2)"""
        return depth + (1 if kind == "leaf" else 2)

    # ---- CheckDepth window: leaf_depth - depth against [1, 256]; the kind follows from the difference
    for depth in (0, 10, M - 300):
        for diff in (0, 1, 2, 255, 256, 257, 600):
            if depth + diff >= M:
                continue                                                   # leaf_depth is a 32-bit word
            kind = "leaf" if diff <= 1 else "parent"
            add(f"window/depth={depth}/diff={diff}", kind, "ok" if 1 <= diff <= 256 else "assert",
                depth=depth, leaf_depth=depth + diff, total_depth=depth + diff)
    add("window/depth=leaf_depth+1", "leaf", "assert", depth=10, leaf_depth=9)
    add("window/depth=leaf_depth+1/high", "parent", "assert", depth=M - 300, leaf_depth=M - 301)
    add("window/depth=leaf_depth+M-1", "leaf", "assert", depth=M - 1, leaf_depth=0)
    add("window/depth=leaf_depth+M-1", "parent", "assert", depth=M - 1, leaf_depth=0)
    add("window/depth=M-1/leaf_depth=M-1", "leaf", "assert", depth=M - 1, leaf_depth=M - 1)

    # ---- istar = total_depth - 2 - depth against [0, 64) and the 64-bit chunk_idx; total_depth != leaf_depth throughout.
    # Parent steps read the bit; leaf steps (one index pair per istar, in rotation) carry chunk_idx into t[0], t[1].
    for n, istar in enumerate(ISTARS):
        for p, (cih, cil) in enumerate(CHUNK_IDX):
            for kind in ("parent", "leaf"):
                if kind == "leaf" and p != n % 4:
                    continue
                depth = 70                                                  # total_depth = istar + 72 in [70, 137]
                ld = kind_depths(kind, depth) + (0 if kind == "leaf" else 3)
                assert depth + 2 + istar != ld or (kind == "leaf" and istar == -1)   # (a leaf step's istar = -1 IS total_depth = leaf_depth)
                add(f"istar={istar}/cih={cih:#x}/cil={cil:#x}", kind, "ok", depth=depth, leaf_depth=ld, total_depth=depth + 2 + istar,
                    cih=cih, cil=cil)
    for td in (0, 1):
        for kind in ("parent", "leaf"):
            add(f"total_depth={td}", kind, "ok", total_depth=td)

    # ---- the table of inverses: every IsZero argument at |k| in K_EDGES, either sign where the gadget has it
    # eqs[i], k = total_depth - 2 - depth - i, on the edge for i = 0 and for i = 63 (kinds in rotation).  k = istar - i > 0 needs
    # total_depth >= K + i + 2 (no such word for K >= M - 2); k = -K puts depth at K + i - 2 + total_depth.  eqs[0] = -(M - 2), -(M - 1)
    # leave eqs[63] = k - 63 below -M: those two rows are "domain".
    n = 0
    for K in K_EDGES:
        for sign in (1, -1):
            for i in (0, 63):
                istar = sign * K + i
                kind = ("leaf", "parent")[n % 2]
                n += 1
                if istar >= 0:
                    depth = 5
                    td = istar + 2 + depth
                else:
                    td = 3
                    depth = td - 2 - istar
                if td >= M or kind_depths(kind, depth) >= M:
                    continue
                expect = "domain" if (sign < 0 and i == 0 and K + 63 >= M) else "ok"
                add(f"eqs[{i}]={'+' if sign > 0 else '-'}{K}", kind, expect, depth=depth, leaf_depth=kind_depths(kind, depth), total_depth=td)
    # check_block_counts[1], k = n_blocks - 1 - block_count: positive from n_blocks = K + 1 (a word up to K = M - 2), negative from
    # n_blocks = 0, block_count = K - 1.  A parent step keeps block_count as it is.
    for j, K in enumerate(K_EDGES):
        kind = ("parent", "leaf")[j % 2]
        if K + 1 < M:
            add(f"e1=+{K}", kind, "ok", n_blocks=K + 1, block_count=0)
        add(f"e1=-{K}", kind, "ok", n_blocks=0, block_count=K - 1)
    add("e1=-(M-1)/n_blocks=1", "parent", "ok", n_blocks=1, block_count=M - 1)
    # check_block_counts[0], k = -block_count
    for j, K in enumerate(K_EDGES):
        kind = ("leaf", "parent")[j % 2] if K != M - 1 else "parent"
        add(f"block_count={K}", kind, "ok", block_count=K, n_blocks=max(K, 1))
    # check_root, k = -depth; leaf_depth - depth stays in the window
    for j, K in enumerate(K_EDGES):
        kind = ("parent", "leaf")[j % 2]
        if kind_depths(kind, K) >= M:
            kind = "leaf"
        if K == M - 1:
            add(f"depth={K}", "leaf", "assert", depth=K, leaf_depth=M - 1, total_depth=M - 1)      # no leaf_depth above it: assert before domain
        else:
            add(f"depth={K}", kind, "ok", depth=K, leaf_depth=kind_depths(kind, K), total_depth=kind_depths(kind, K))

    # ---- the limit of the domain
    add("domain/n_blocks=0/block_count=M-1", "parent", "domain", n_blocks=0, block_count=M - 1)                       # k = -M
    add("domain/n_blocks=0/block_count=M-1", "leaf", "domain", n_blocks=0, block_count=M - 1)
    add("domain/block_count=M-1", "leaf", "domain", n_blocks=5, block_count=M - 1)                                   # block_count + 1 = M
    add("domain/block_count=M-1/n_blocks=M-1", "leaf", "domain", n_blocks=M - 1, block_count=M - 1)
    add("domain-neighbour/block_count=M-2", "leaf", "ok", n_blocks=M - 1, block_count=M - 2)                         # last block, out M - 1
    add("domain-neighbour/block_count=M-2/n_blocks=0", "leaf", "ok", n_blocks=0, block_count=M - 2)                  # k = -(M - 1)
    add("domain-neighbour/block_count=M-1/n_blocks=M-1", "parent", "ok", n_blocks=M - 1, block_count=M - 1)          # k = -1
    for kind in ("leaf", "parent"):
        add("domain/total_depth=0/depth=M-65", kind, "domain", total_depth=0, depth=M - 65, leaf_depth=kind_depths(kind, M - 65))   # eqs[63] = -M
        add("domain-neighbour/total_depth=0/depth=M-66", kind, "ok", total_depth=0, depth=M - 66, leaf_depth=kind_depths(kind, M - 66))
        add("domain/total_depth=1/depth=M-64", kind, "domain", total_depth=1, depth=M - 64, leaf_depth=kind_depths(kind, M - 64))
        add("domain-neighbour/total_depth=1/depth=M-65", kind, "ok", total_depth=1, depth=M - 65, leaf_depth=kind_depths(kind, M - 65))
    add("domain/total_depth=0/depth=M-2", "leaf", "domain", total_depth=0, depth=M - 2, leaf_depth=M - 1)            # eqs[0] = -M
    add("domain/total_depth=1/depth=M-2", "leaf", "domain", total_depth=1, depth=M - 2, leaf_depth=M - 1)
    add("domain/total_depth=0/depth=M-3", "parent", "domain", total_depth=0, depth=M - 3, leaf_depth=M - 1)
    add("assert-before-domain/total_depth=0/depth=M-1", "leaf", "assert", total_depth=0, depth=M - 1, leaf_depth=M - 1)
    add("assert-before-domain/n_blocks=0/block_count=M-1", "leaf", "assert", n_blocks=0, block_count=M - 1, depth=29, leaf_depth=29)
    add("assert-before-domain/block_count=M-1/diff=257", "parent", "assert", n_blocks=0, block_count=M - 1, depth=3, leaf_depth=260)

    # ---- words
    for b in (0, 1, 63, 64, 65, M - 1):
        add(f"b={b}", "leaf", "ok", b=b)
    for b in (0, M - 1):
        add(f"b={b}", "parent", "ok", b=b)
    ones8, ones16 = [M - 1] * 8, [M - 1] * 16
    add("h=0", "leaf", "ok", h=[0] * 8)
    add("h=0", "parent", "ok", h=[0] * 8)
    add("h=ones", "leaf", "ok", h=ones8)
    add("h=ones", "parent", "ok", h=ones8)
    add("m=0", "leaf", "ok", m=[0] * 16)
    add("m=0", "parent", "ok", m=[0] * 16)
    add("m=ones", "leaf", "ok", m=ones16)
    add("m=ones", "parent", "ok", m=ones16)
    add("h=m=ones", "leaf", "ok", h=ones8, m=ones16, cil=M - 1, cih=M - 1, b=M - 1)
    n = 0
    for pos in (0, 7):
        for v in (0x80000000, 0xFFFFFFFF):
            add(f"h[{pos}]={v:#x}/rest=0", ("leaf", "parent")[n % 2], "ok", h=[v if q == pos else 0 for q in range(8)])
            n += 1
    for pos in (0, 7, 8, 15):
        for v in (0x80000000, 0xFFFFFFFF):
            add(f"m[{pos}]={v:#x}/rest=0", ("leaf", "parent")[n % 2], "ok", m=[v if q == pos else 0 for q in range(16)])
            n += 1
    pm = [int(x) for x in base["parent"][MSG:MSG + 8]] + list(_FILL8)
    add("m[8..15]!=0/chunk_idx!=0", "parent", "ok", m=pm, cih=0x9E3779B9)                 # the circuit masks both on a parent step
    add("m[8..15]=ones/chunk_idx=ones", "parent", "ok", m=pm[:8] + ones8, cih=M - 1, cil=M - 1)
    add("chunk_idx_high!=0", "leaf", "ok", cih=0x9E3779B9)                                # feeds t[1]
    add("root/last-block", "leaf", "ok", depth=0, leaf_depth=1, total_depth=1, n_blocks=4, block_count=3)
    add("root/first-and-last-block", "leaf", "ok", depth=0, leaf_depth=1, total_depth=1, n_blocks=1, block_count=0)
    add("root/not-last-block", "leaf", "ok", depth=0, leaf_depth=1, total_depth=1, n_blocks=4, block_count=1)
    add("root", "parent", "ok", depth=0, leaf_depth=2, total_depth=2)
    add("root/leaf_depth=256", "parent", "ok", depth=0, leaf_depth=256, total_depth=256)

    names = [r[0] for r in rows]
    assert len(set(names)) == len(names), [x for x in names if names.count(x) > 1]
    return rows


def compression_rows():
    base = _W.config2_compression(1)[0]
    rows = []

    def add(name, **f):
        r = base.copy()
        for k, v in f.items():
            if k == "h":
                r[0:8] = np.array(v, dtype=np.uint64).astype(np.uint32)
            elif k == "m":
                r[8:24] = np.array(v, dtype=np.uint64).astype(np.uint32)
            else:
                r[{"t0": 24, "t1": 25, "b": 26, "d": 27}[k]] = v
        rows.append((name, r, "ok"))

    for field in ("t0", "t1", "b", "d"):
        for v in (0, 1, 64, 65, 0x7FFFFFFF, 0x80000000, M - 1):
            add(f"{field}={v:#x}", **{field: v})
    z8, z16, o8, o16 = [0] * 8, [0] * 16, [M - 1] * 8, [M - 1] * 16
    add("h=0", h=z8)
    add("h=ones", h=o8)
    add("m=0", m=z16)
    add("m=ones", m=o16)
    add("all=0", h=z8, m=z16, t0=0, t1=0, b=0, d=0)
    add("all=ones", h=o8, m=o16, t0=M - 1, t1=M - 1, b=M - 1, d=M - 1)
    # carry chains: the operands of ONE G of the first round at 0xFFFFFFFF — v[a] + v[b] + x (34 bits) and, through the all-ones
    # rotations that follow, v[c] + v[d] (33 bits) reach their top carries.  Columns G0..G3 take (h[g], h[4 + g]; m[2g], m[2g + 1]),
    # diagonals G4..G7 (h[g], h[4 + (g + 1) % 4]; m[8 + 2g], m[9 + 2g])  (BLAKE3 section 2.2).
    hb, mb = [int(x) for x in base[0:8]], [int(x) for x in base[8:24]]
    for g in range(8):
        a, b_ = (g, 4 + g) if g < 4 else (g - 4, 4 + (g - 4 + 1) % 4)
        h, m = list(hb), list(mb)
        h[a] = h[b_] = m[2 * g] = m[2 * g + 1] = M - 1
        add(f"carry/G{g}", h=h, m=m)
    for i, r in enumerate(_W.config1_cases()):
        rows.append((f"config1[{i}]", r.copy(), "ok"))
    names = [r[0] for r in rows]
    assert len(set(names)) == len(names)
    return rows


def stack(rows):
    """-> (names, records uint32 [n, words], expect list)"""
    return [r[0] for r in rows], np.ascontiguousarray(np.stack([r[1] for r in rows]).astype(np.uint32)), [r[2] for r in rows]
