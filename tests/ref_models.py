"""Independent numpy models of the circuits' PUBLIC outputs (plain BLAKE3 and the nova step's control logic), shared by the GPU
parity tests and the record-domain table's CPU test.  Test infrastructure."""
import numpy as np

import b3w_testlib as T


def _blake3_compress_np(h, mm, t0, t1, b, d):
    """Independent plain BLAKE3 compression, vectorised over the batch (BLAKE3 spec section 2.2)."""
    IV = T.workloads().IV.astype(np.uint32)
    perm = [2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8]
    n = h.shape[0]
    v = [h[:, i].copy() for i in range(8)] + [np.full(n, IV[i], np.uint32) for i in range(4)] + [t0.copy(), t1.copy(), b.copy(), d.copy()]
    msg = [mm[:, i].copy() for i in range(16)]
    rot = lambda x, r: (x >> np.uint32(r)) | (x << np.uint32(32 - r))

    def g(a, b_, c, d_, x, y):
        v[a] = v[a] + v[b_] + x; v[d_] = rot(v[d_] ^ v[a], 16)
        v[c] = v[c] + v[d_]; v[b_] = rot(v[b_] ^ v[c], 12)
        v[a] = v[a] + v[b_] + y; v[d_] = rot(v[d_] ^ v[a], 8)
        v[c] = v[c] + v[d_]; v[b_] = rot(v[b_] ^ v[c], 7)
    for r in range(7):
        g(0, 4, 8, 12, msg[0], msg[1]); g(1, 5, 9, 13, msg[2], msg[3]); g(2, 6, 10, 14, msg[4], msg[5]); g(3, 7, 11, 15, msg[6], msg[7])
        g(0, 5, 10, 15, msg[8], msg[9]); g(1, 6, 11, 12, msg[10], msg[11]); g(2, 7, 8, 13, msg[12], msg[13]); g(3, 4, 9, 14, msg[14], msg[15])
        msg = [msg[perm[j]] for j in range(16)]
    out = [v[i] ^ v[i + 8] for i in range(8)] + [v[i + 8] ^ h[:, i] for i in range(8)]
    return np.stack(out, axis=1)


def _nova_public_np(recs):
    """Independent numpy model of the step's public outputs (h_out via plain BLAKE3)."""
    IV = T.workloads().IV.astype(np.uint32)
    nb, bc, h = recs[:, 0], recs[:, 1], recs[:, 2:10]
    cil, cih, ld, td, depth, mm, b = recs[:, 10], recs[:, 11], recs[:, 12], recs[:, 13], recs[:, 14], recs[:, 15:31], recs[:, 31]
    parent = depth.astype(np.int64) < ld.astype(np.int64) - 1
    root = depth == 0
    e0, e1 = bc == 0, nb.astype(np.int64) - 1 == bc.astype(np.int64)
    first, last = e0 & ~parent, e1 & ~parent
    d = first.astype(np.uint32) + 2 * last.astype(np.uint32) + 8 * ((parent | e1) & root).astype(np.uint32) + 4 * parent.astype(np.uint32)
    istar = td.astype(np.int64) - 2 - depth.astype(np.int64)
    ci = cil.astype(np.uint64) | (cih.astype(np.uint64) << np.uint64(32))
    ok = (istar >= 0) & (istar < 64)
    bit = (ci >> np.clip(istar, 0, 63).astype(np.uint64)) & np.uint64(1)
    dl = np.where(parent, ok & (bit == 0), True)
    msg = mm.copy()
    left = np.where(dl[:, None], h, mm[:, :8])
    right = np.where(dl[:, None], mm[:, :8], h)
    msg[parent] = np.concatenate([left, right], axis=1)[parent]
    hc = np.where(parent[:, None], IV[None, :], h)
    t0, t1 = np.where(parent, 0, cil).astype(np.uint32), np.where(parent, 0, cih).astype(np.uint32)
    out = _blake3_compress_np(hc.astype(np.uint32), msg.astype(np.uint32), t0, t1, b.copy(), d.astype(np.uint32))
    bco = bc + (~parent).astype(np.uint32)
    dout = depth - (((last | parent) & ~root)).astype(np.uint32)
    return np.concatenate([nb[:, None], bco[:, None], out[:, :8], td[:, None], dout[:, None], cil[:, None], cih[:, None], ld[:, None]], axis=1).astype(np.uint32)
