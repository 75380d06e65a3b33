#!/usr/bin/env python3
"""tools/bao_verify_model.py — the logic of the three verify kernels of csrc/b3w_bao.hip (check_pair's flags, verify_in_lds' level
loop, the two storeys above the tiles with their scratch entries, the small kernel, the per-file reductions) restated in Python with
tiles of 8 chunks and small files of at most 4, and held against tests/bao_verify_ref.py on clean and tampered files of 1 ... 150
chunks at g = 0, 1, 2.  No GPU and no library: it checks the scheme, not the HIP code (tests/test_gpu_bao_verify.py does that).
About two minutes of pure-Python BLAKE3."""
import os, sys, struct, random
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import blake3_ref as B, bao_ref as R, bao_groups_ref as GR, bao_verify_ref as V
import functools

TILE = 8
SMALL = 4
UNIT_BIT, TOP_BIT = 1 << 31, 1 << 10


@functools.lru_cache(maxsize=None)
def H(words, root):
    return tuple(B.compress(B.IV, list(words), 0, 64, B.PARENT | (B.ROOT if root else 0))[:8])


def preorder_pos(total, a, size):
    p, lo, cnt = 0, 0, total
    while cnt > 1 and not (lo == a and cnt == size):
        k = R._split(cnt)
        if a < lo + k: p, cnt = p + 1, k
        else: p, lo, cnt = p + k, lo + k, cnt - k
    return p


def node(ob, pos):
    return tuple(struct.unpack("<16I", ob[8 + 64 * pos:8 + 64 * pos + 64]))


def verify_in_lds(cv, flags, cnt, unit, total, ob, base_pos, root, gl, claim, exp_out, out0):
    G = 1 << gl; G1 = G - 1; leaf = G if claim else unit
    l = 0
    while (1 << l) < cnt:
        top = (2 << l) >= cnt
        j = 0
        while True:
            i0 = (2 * j) << l; i1 = i0 + (1 << l)
            if i1 >= cnt: break
            a = i0 * unit; e = (i0 + (2 << l)) * unit; size = min(e, total) - a
            rt = top and root
            if claim and size <= G:
                cv[i0] = H(tuple(cv[i0]) + tuple(cv[i1]), rt)
            else:
                m = node(ob, base_pos + preorder_pos((total + G1) >> gl, a >> gl, (size + G1) >> gl))
                sl = unit << l; sr = size - sl
                for (i, s, half) in ((i0, sl, m[:8]), (i1, sr, m[8:])):
                    if s <= leaf:
                        if claim:
                            if tuple(cv[i]) != half: flags[i] |= UNIT_BIT
                        else: exp_out[out0 + i] = half
                    elif tuple(cv[i]) != half: flags[i] |= 1 << l
                cv[i0] = H(m, rt)
            j += 1
        l += 1


def path_bad(flags, t):
    x = 0
    for l in range(11): x |= flags[(t >> l) << l] & (1 << l)
    return x != 0


def device_verify(files, gl):
    """files: list of (data, ob, root, length) -> per-file (statuses, file_status, first_bad)"""
    G = 1 << gl; G1 = G - 1
    # host tables
    slot = gslot = 0; vf = []
    for (data, ob, root, length) in files:
        n = R.num_chunks(length)
        vf.append((slot, gslot))
        if n > SMALL:
            tiles = -(-n // TILE); grp = -(-tiles // TILE)
            if tiles > 1: slot += tiles
            if grp > 1: gslot += grp
    n_tile_ents = slot
    exp_cv = {}; bad = {}
    fstat = {}; fbad = {}; out = {}
    NONE = (1 << 64) - 1

    def upper(f, unit, g):
        data, ob, root, length = files[f]
        n = R.num_chunks(length)
        span = unit * TILE; a0 = g * span; tot = min(n - a0, span); cnt = -(-tot // unit); sole = n <= span
        sl_, gs_ = vf[f]
        out0 = sl_ + g * TILE if unit == TILE else n_tile_ents + gs_
        inn = n_tile_ents + gs_ + g
        want = tuple(root) if sole else exp_cv[inn]
        above = False if sole else bad[inn]
        if sole:
            hdr = struct.unpack("<Q", ob[:8])[0] != length
            fstat[f] = 3 if hdr else 0; fbad[f] = 0 if hdr else NONE
        if cnt == 1:
            exp_cv[out0] = want; bad[out0] = above; return
        cv = [None] * cnt; flags = [0] * cnt
        verify_in_lds(cv, flags, cnt, unit, tot, ob, preorder_pos((n + G1) >> gl, a0 >> gl, (tot + G1) >> gl), sole, gl, False, exp_cv, out0)
        above = above or tuple(cv[0]) != want
        for t in range(cnt): bad[out0 + t] = above or path_bad(flags, t)

    def chunk_cv(data, length, c, root):
        a, b = R.chunk_range(length, c)
        return tuple(B.chunk_cv(data[a:b], c, root))

    # launch order: tops, groups storey, small, tile
    for f, (data, ob, root, length) in enumerate(files):
        n = R.num_chunks(length)
        if n > SMALL and -(-(-(-n // TILE)) // TILE) > 1: upper(f, TILE * TILE, 0)
    for f, (data, ob, root, length) in enumerate(files):
        n = R.num_chunks(length)
        tiles = -(-n // TILE)
        if n > SMALL and tiles > 1:
            for g in range(-(-tiles // TILE)): upper(f, TILE, g)
    for f, (data, ob, root, length) in enumerate(files):
        n = R.num_chunks(length)
        nu = (n + G1) >> gl
        st = [None] * nu
        hdr = struct.unpack("<Q", ob[:8])[0] != length
        if n <= SMALL:
            cv = [chunk_cv(data, length, i, n == 1) for i in range(n)]
            flags = [0] * n
            for l in range(6):
                if not (1 << l) < n: break
                for i in range(n):
                    if i & ((2 << l) - 1) == 0 and i + (1 << l) < n:
                        size = min(n - i, 2 << l); rt = i == 0 and (2 << l) >= n
                        if size <= G: cv[i] = H(cv[i] + cv[i + (1 << l)], rt)
                        else:
                            m = node(ob, preorder_pos((n + G1) >> gl, i >> gl, (size + G1) >> gl))
                            for (k, s, half) in ((i, 1 << l, m[:8]), (i + (1 << l), size - (1 << l), m[8:])):
                                if s <= G:
                                    if cv[k] != half: flags[k] |= UNIT_BIT
                                elif cv[k] != half: flags[k] |= 1 << l
                            cv[i] = H(m, rt)
            if cv[0] != tuple(root): flags[0] |= UNIT_BIT if n <= G else 1 << 6
            for i in range(0, n, G):
                x = 0
                for l in range(7): x |= flags[(i >> l) << l] & (1 << l)
                st[i >> gl] = 3 if hdr else 2 if x else 1 if flags[i] & UNIT_BIT else 0
            b = [u for u in range(nu) if st[u]]
            fstat[f] = max(st); fbad[f] = b[0] if b else NONE
        else:
            tiles = -(-n // TILE); sole = n <= TILE
            for tile in range(tiles):
                a0 = tile * TILE; m_ = min(n - a0, TILE)
                cv = [chunk_cv(data, length, a0 + t, False) for t in range(m_)]
                flags = [0] * TILE
                verify_in_lds(cv, flags, m_, 1, m_, ob, preorder_pos((n + G1) >> gl, a0 >> gl, (m_ + G1) >> gl), sole, gl, True, None, 0)
                ent = vf[f][0] + tile
                if tuple(cv[0]) != (tuple(root) if sole else exp_cv[ent]): flags[0] |= UNIT_BIT if m_ <= G else TOP_BIT
                above = False if sole else bad[ent]
                worst, first = 0, None
                for t in range(0, m_, G):
                    s = 3 if hdr else 2 if (above or path_bad(flags, t)) else 1 if flags[t] & UNIT_BIT else 0
                    st[(a0 + t) >> gl] = s
                    if s:
                        worst = max(worst, s); first = t >> gl if first is None else min(first, t >> gl)
                if sole:
                    fstat[f] = worst; fbad[f] = first if worst else NONE
                elif worst:
                    fstat[f] = max(fstat[f], worst); fbad[f] = min(fbad[f], (a0 >> gl) + first)
        out[f] = (st, fstat[f], fbad[f])
    return out


def flip(b, i):
    b = bytearray(b); b[i] ^= 1; return bytes(b)


rng = random.Random(5)
checked = 0
for gl in (0, 1, 2):
    for n in [1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 23, 24, 25, 33, 57, 64, 65, 66, 72, 73, 100, 129, 150]:
        length = n * 1024 - rng.choice([0, 0, 1, 500, 1023])
        data = bytes(rng.getrandbits(8) for _ in range(length))
        ob, root = GR.group_outboard(data, gl)
        nu = V.num_units(length, gl)
        cases = [(data, ob, root)]
        for _ in range(3):
            cases.append((flip(data, rng.randrange(length)), ob, root))
        for i in sorted({0, nu - 2, (nu - 1) // 2, 1} & set(range(nu - 1))):
            cases.append((data, flip(ob, 8 + 64 * i + rng.randrange(64)), root))
            cases.append((flip(data, rng.randrange(length)), flip(ob, 8 + 64 * i + rng.randrange(64)), root))
        wr = list(root); wr[2] ^= 4
        cases.append((data, ob, wr))
        cases.append((data, flip(ob, 3), root))
        files = [(d, o, r, length) for d, o, r in cases]
        got = device_verify(files, gl)
        for f, (d, o, r, _) in enumerate(files):
            want = V.verify(d, o, r, length, gl)
            assert got[f][0] == want, (gl, n, f, got[f][0], want)
            assert (got[f][1], got[f][2]) == V.summary(want), (gl, n, f)
            checked += 1
print("model ok", checked)
