"""Outboard deltas restated in plain Python / numpy (include/b3wit.h "outboard delta").  Nothing here calls the library.

The definitions read aloud over bao_groups_ref.node_spans.  Both sides have one group_log g; U = units of 2^g chunks; b's tree has
U_b - 1 parent nodes in pre-order, node p over units [lo, lo + cnt).  A node's CV is STORED in the half of its parent's node.
  SAME       the root: equal chunk counts and equal roots.  p > 0: (lo, cnt) is a node of a's tree, it covers the same chunks in both
             files, it is not a's root, and the two stored CVs are equal.  With no a nothing is SAME.
  make_blob  len_b, k, the bitmap of the nodes that are not SAME, those nodes in pre-order
  apply_blob the verifier / assembler: every fault as (node, status), the least one is the pair's; the outboard only without a fault
  fabricate  an outboard that is consistent with its root from the units' CVs alone (no file is needed: the delta reads no file byte)
  same_np    the provider's bitmap for large unit counts from positions alone (numpy): nothing is hashed by the provider"""
import functools
import struct

import numpy as np

import bao_groups_ref as GR
import bao_ref as R
import blake3_ref as B

MALFORMED, BAD_HASH, NOT_HELD = 1, 2, 3
NONE = -1


def units(length, g):
    return GR.num_groups(R.num_chunks(length), g)


def words(U):
    return (U - 1 + 63) // 64


def bound(length, g):
    U = units(length, g)
    return 16 + 8 * words(U) + 64 * (U - 1)


@functools.lru_cache(maxsize=None)
def tree(U):
    """-> (spans [(lo, cnt)] in pre-order, {(lo, cnt): p}, up [(parent, side)] (the root: None), kids [((p_left or None, lo, cnt), (p_right or None, lo, cnt))])"""
    spans = GR.node_spans(U)
    index = {s: p for p, s in enumerate(spans)}
    up, kids = [None] * len(spans), []
    for p, (lo, cnt) in enumerate(spans):
        k = R._split(cnt)
        both = []
        for side, (clo, ccnt) in enumerate(((lo, k), (lo + k, cnt - k))):
            pc = index.get((clo, ccnt)) if ccnt >= 2 else None
            if pc is not None:
                up[pc] = (p, side)
            both.append((pc, clo, ccnt))
        kids.append(tuple(both))
    return spans, index, up, kids


def node(ob, p):
    return bytes(ob[8 + 64 * p:8 + 64 * p + 64])


def stored(ob, U, p):
    """the CV of node p > 0 as the outboard stores it: a half of its parent's node"""
    parent, side = tree(U)[2][p]
    at = 8 + 64 * parent + 32 * side
    return bytes(ob[at:at + 32])


def held(ob_a, len_a, len_b, g, lo, cnt):
    """where a holds a node over units [lo, lo + cnt) below its root that covers the same chunks as in b -> its stored CV, else None"""
    if ob_a is None:
        return None
    na, nb = R.num_chunks(len_a), R.num_chunks(len_b)
    Ua = GR.num_groups(na, g)
    pa = tree(Ua)[1].get((lo, cnt)) if Ua >= 2 else None
    if pa is None or pa == 0:
        return None
    if min((lo + cnt) << g, na) != min((lo + cnt) << g, nb):
        return None
    return stored(ob_a, Ua, pa)


def root_same(ob_a, len_a, root_a, len_b, root_b):
    return ob_a is not None and R.num_chunks(len_a) == R.num_chunks(len_b) and bytes(root_a) == bytes(root_b)


def same_nodes(ob_a, len_a, root_a, ob_b, len_b, root_b, g):
    """-> a bool per parent node of b"""
    Ub = units(len_b, g)
    spans = tree(Ub)[0]
    out = np.zeros(len(spans), bool)
    for p, (lo, cnt) in enumerate(spans):
        if p == 0:
            out[0] = root_same(ob_a, len_a, root_a, len_b, root_b)
        else:
            cv = held(ob_a, len_a, len_b, g, lo, cnt)
            out[p] = cv is not None and cv == stored(ob_b, Ub, p)
    return out


def pack(present):
    """bools -> the bitmap's bytes (little-endian 64-bit words, pad bits zero)"""
    W = (len(present) + 63) // 64
    bits = np.zeros(64 * W, np.uint8)
    bits[:len(present)] = present
    return np.packbits(bits, bitorder="little").tobytes()


def make_blob(ob_a, len_a, root_a, ob_b, len_b, root_b, g):
    present = ~same_nodes(ob_a, len_a, root_a, ob_b, len_b, root_b, g)
    return struct.pack("<QQ", len_b, int(present.sum())) + pack(present) + b"".join(node(ob_b, int(p)) for p in np.flatnonzero(present))


@functools.lru_cache(maxsize=None)
def parent_cv(node_bytes, root):
    w = list(struct.unpack("<16I", node_bytes))
    return R._cv_bytes(B.compress(B.IV, w, 0, 64, B.PARENT | (B.ROOT if root else 0))[:8])


def apply_blob(ob_a, len_a, root_a, len_b, root_b, g, blob):
    """-> (status, first bad node or NONE, b's outboard or None); len(blob) is the extent"""
    Ub = units(len_b, g)
    W, n_nodes = words(Ub), Ub - 1
    assert len(blob) >= 16 + 8 * W, "refused: an extent too small for its header and bitmap"
    length, k = struct.unpack("<QQ", blob[:16])
    bits = np.unpackbits(np.frombuffer(blob[16:16 + 8 * W], np.uint8), bitorder="little").astype(bool)
    faults = []
    if length != len_b or k != int(bits.sum()) or 16 + 8 * W + 64 * k > len(blob):
        return MALFORMED, 0, None
    for p in np.flatnonzero(bits[n_nodes:]):
        faults.append((n_nodes + int(p), MALFORMED))                    # a pad bit
    rank = np.cumsum(bits) - bits
    base = 16 + 8 * W

    def blob_node(p):
        return blob[base + 64 * int(rank[p]):base + 64 * int(rank[p]) + 64]
    if n_nodes:
        spans, _, up, kids = tree(Ub)
        if not bits[0] and not root_same(ob_a, len_a, root_a, len_b, root_b):
            faults.append((0, MALFORMED))
        for p in np.flatnonzero(bits[:n_nodes]).tolist():
            nd = blob_node(p)
            if p:
                parent, side = up[p]
                if not bits[parent]:
                    faults.append((p, MALFORMED))
                    continue
                want = blob_node(parent)[32 * side:32 * side + 32]
            else:
                want = bytes(root_b)
            if parent_cv(nd, p == 0) != want:
                faults.append((p, BAD_HASH))
                continue
            for side, (pc, clo, ccnt) in enumerate(kids[p]):
                if pc is None or bits[pc]:
                    continue
                if held(ob_a, len_a, len_b, g, clo, ccnt) != nd[32 * side:32 * side + 32]:
                    faults.append((pc, NOT_HELD))
    if faults:
        bad, status = min(faults)
        return status, bad, None
    out = [struct.pack("<Q", len_b)]
    if n_nodes:
        Ua = units(len_a, g) if ob_a is not None else 0
        for p, span in enumerate(spans):
            out.append(blob_node(p) if bits[p] else node(ob_a, tree(Ua)[1][span]))
    return 0, NONE, b"".join(out)


# ---- outboards without files ------------------------------------------------------------------------------------------------------------
def leaf_cv(seed, u, chunks):
    """the made-up CV of unit u that covers `chunks` chunks, of the version `seed`"""
    return np.random.default_rng([seed, u, chunks]).integers(0, 256, 32, dtype=np.uint8).tobytes()


def fabricate(leaves, length):
    """the outboard over these units' CVs (32 bytes each) and its root: consistent, node by node -> (outboard bytes, root bytes)"""
    nodes = []

    def walk(first, m, root):
        if m == 1:
            return leaves[first]
        k = R._split(m)
        slot = len(nodes)
        nodes.append(None)
        left = walk(first, k, False)
        right = walk(first + k, m - k, False)
        nodes[slot] = left + right
        return parent_cv(nodes[slot], root)
    if len(leaves) == 1:
        return struct.pack("<Q", length), leaves[0]
    root = walk(0, len(leaves), True)
    return struct.pack("<Q", length) + b"".join(nodes), root


def version(seeds, length, g):
    """the fabricated outboard of a file of `length` bytes whose unit u is that of version seeds[u]"""
    n = R.num_chunks(length)
    U = GR.num_groups(n, g)
    return fabricate([leaf_cv(int(seeds[u]), u, min(1 << g, n - (u << g))) for u in range(U)], length)


# ---- positions alone, for large unit counts ---------------------------------------------------------------------------------------------
def _left_of(cnt):
    k = cnt - 1
    for s in (1, 2, 4, 8, 16, 32):
        k |= k >> s
    return (k + 1) >> 1


def nodes_np(U):
    """-> (lo, cnt, parent, side) of every parent node of the tree over U >= 2 units in pre-order, level by level"""
    lo, cnt = np.zeros(U - 1, np.int64), np.zeros(U - 1, np.int64)
    parent, side = np.full(U - 1, -1, np.int64), np.zeros(U - 1, np.int64)
    pos, cnt[0] = np.array([0], np.int64), U
    while pos.size:
        k = _left_of(cnt[pos])
        nxt = []
        for s, (cp, clo, ccnt) in enumerate(((pos + 1, lo[pos], k), (pos + k, lo[pos] + k, cnt[pos] - k))):
            live = ccnt >= 2
            lo[cp[live]], cnt[cp[live]], parent[cp[live]], side[cp[live]] = clo[live], ccnt[live], pos[live], s
            nxt.append(cp[live])
        pos = np.concatenate(nxt)
    return lo, cnt, parent, side


def same_np(ob_a, na, ob_b, nb, g, roots_equal=False):
    """same_nodes for two outboards (numpy uint8) of files of na and nb chunks, Ua, Ub >= 2"""
    Ua, Ub = GR.num_groups(na, g), GR.num_groups(nb, g)
    lo_a, cnt_a, par_a, side_a = nodes_np(Ua)
    lo_b, cnt_b, par_b, side_b = nodes_np(Ub)
    key_a = lo_a * (1 << 32) + cnt_a
    order = np.argsort(key_a)
    key_b = lo_b * (1 << 32) + cnt_b
    at = np.clip(np.searchsorted(key_a[order], key_b), 0, Ua - 2)
    pa = order[at]
    ok = (key_a[pa] == key_b) & (pa != 0)
    end = (lo_b + cnt_b) << g
    ok &= np.minimum(end, na) == np.minimum(end, nb)
    ok[0] = False
    cols = np.arange(32, dtype=np.int64)
    idx = np.flatnonzero(ok)
    cv_a = ob_a[(8 + 64 * par_a[pa[idx]] + 32 * side_a[pa[idx]])[:, None] + cols]
    cv_b = ob_b[(8 + 64 * par_b[idx] + 32 * side_b[idx])[:, None] + cols]
    out = np.zeros(Ub - 1, bool)
    out[idx] = (cv_a == cv_b).all(axis=1)
    out[0] = roots_equal and na == nb
    return out
