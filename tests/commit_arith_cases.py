"""The case table of the commit kernels' arithmetic (csrc/b3w_commit_arith.h) and the plain-integer check of every row.

tests/test_commit_arith_cpu.py runs it through the routines compiled for the host, under sanitizers; the table knows nothing of
who applies a row, so a device probe can take the same rows.  A row names ONE routine and gives its
operands as raw limbs (tests/commit_arith_rows.h: B3W_PROBE_IN words in, B3W_PROBE_OUT words out); `check` judges the raw results
against Python integers by what the header's comment block promises:
  value right modulo p (Montgomery radix 2^261 for the nine 29-bit limbs, 2^256 for the eight 32-bit ones);
  "tidy" (limbs 0..7 below 2^29) where promised, and below the promised multiple of p:
      mul29 / sqr29 / muladd29   r < (ab [+ cd]) / (64 p) + p — the header's (AB/64 + 1)p with A = a / p exactly;
      red29, the s_* forms       tidy, < 2p;
  canonical results (fp_*, is_kp29, s_is_zero, from29 + fp_reduce_once, the pure limb shuffles) exactly;
  group results equal to ec_ref.add after normalising here, all four XYZZ coordinates tidy and below 2p, ZZ^3 = ZZZ^2, `inf` right.
Operands: edge values (k p + d for every k up to the routine's bound, powers of two around the limb borders, limbs all ones),
operands shaped the way j9_madd shapes them (built with an exact integer model of the limb shuffles, never synthesised limb
patterns), limbs at the documented maximum, and a seeded random.Random — nothing else is random.
Test infrastructure."""
import functools
import random

import numpy as np

import ec_ref as E

IN_WORDS, OUT_WORDS = 80, 72
M29 = (1 << 29) - 1
R9, R8 = 1 << 261, 1 << 256
# field / instantiation of a table (tests/commit_arith_rows.h)
FIELDS = {0: ("bn254_g1", False), 1: ("vesta", False), 2: ("vesta", True)}
FIELD_NAMES = {0: "bn254-generic", 1: "pasta-generic", 2: "pasta-B3wCurve9Vesta"}
OP = dict(FP_ADD=1, FP_SUB=2, FP_MUL=3, FP_SQR=4, FP_INV=5, FP_DBL=6, FP_REDUCE_ONCE=7, JAC_DBL=8, JAC_MADD=9, JAC_ADD=10, JAC_TO_AFFINE=11,
          MUL29=20, SQR29=21, MULADD29=22, CN29=23, RED29=24, ADD29=25, SUB29=26, NEG29=27, SHL29=28, IS_KP29=29, S_IS_ZERO=30,
          S_ADD=31, S_SUB=32, S_DBL=33, INV29=34, TO29=35, FROM29=36, J9_DBL=40, J9_MADD=41, J9_ADD=42, CONSTS=50)
OP_NAME = {v: k for k, v in OP.items()}
LIMB_PRODUCT = 152 * (1 << 60) // 100            # "la * lb < 1.52 * 2^60"


# ---- limbs <-> integers
def split29(v):
    assert 0 <= v < 1 << 264
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def val29(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def split32(v):
    assert 0 <= v < 1 << 256
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def val32(l):
    return sum(int(x) << (32 * i) for i, x in enumerate(l))


def is_tidy(l):
    return all(int(x) <= M29 for x in l[:8])


def _u32(l):
    assert all(0 <= x < 1 << 32 for x in l), l
    return list(l)


# ---- the limb shuffles of the header as integers (exact: they have one possible result)
def sp4_limbs(p):
    """4p, limb i lifted by 2^29 and lowered by the 1 it lent to limb i - 1"""
    l = split29(4 * p)
    for i in range(8):
        l[i] += (1 << 29) - (1 if i else 0)
    l[8] -= 1
    return l


def sub_raw(a, b, p):
    return _u32([x + s - y for x, s, y in zip(a, sp4_limbs(p), b)])


def neg_raw(b, p):
    return _u32([s - y for s, y in zip(sp4_limbs(p), b)])


def add_raw(a, b):
    return _u32([x + y for x, y in zip(a, b)])


def shl_raw(a, s):
    return _u32([x << s for x in a])


def mont29(a, b, p):
    """mul29's value: the one r with r 2^261 = a b + m p, 0 <= m < 2^261"""
    t = a * b
    return (t + (-t * pow(p, -1, R9)) % R9 * p) >> 261


def untidy(l, rng):
    """the same value with carries pushed back down: limbs up to 2^32 - 1"""
    l = list(l)
    for i in range(8):
        c = rng.randrange(0, min(l[i + 1], 7) + 1)
        l[i] += c << 29
        l[i + 1] -= c
    return _u32(l)


def edges(p, bound):
    """the edge values below `bound`"""
    v = set()
    for k in range(bound // p + 1):
        v.update(k * p + d for d in range(-2, 3))
    for i in range(10):
        v.add((1 << (29 * i)) - 1)
    for i in range(9):
        v.update(((1 << (32 * i)), (1 << (32 * i)) - 1, p - (1 << (32 * i))))
    v.update((1 << 253, (1 << 254) - 1, bound - 1))
    low = (1 << 232) - 1                           # limbs 0..7 all ones, limb 8 as large as the bound allows
    if bound > low:
        v.add(((bound - 1 - low) >> 232 << 232) + low)
    return sorted(x for x in v if 0 <= x < bound)


class Table:
    def __init__(self, field):
        self.field = field
        self.curve, self.const_modulus = FIELDS[field]
        self.p = E.CURVES[self.curve][0]
        self.rows = []                             # (op, arg, words, info)

    def add(self, op, words, arg=0, **info):
        words = [int(w) for w in words]
        assert len(words) <= IN_WORDS - 2 and all(0 <= w < 1 << 32 for w in words), (op, words)
        self.rows.append((OP[op], arg, words, info))

    def packed(self):
        a = np.zeros((len(self.rows), IN_WORDS), dtype=np.uint32)
        for i, (op, arg, words, _) in enumerate(self.rows):
            a[i, 0], a[i, 1] = op, arg
            a[i, 2:2 + len(words)] = words
        return a


# ---- the rows
def _eight_limb_rows(T, rng):
    p = T.p
    ev = edges(p, p) + [rng.randrange(p) for _ in range(6)]
    for a in ev:
        for b in ev:
            for op in ("FP_ADD", "FP_SUB", "FP_MUL"):
                T.add(op, split32(a) + split32(b))
        T.add("FP_SQR", split32(a))
        T.add("FP_DBL", split32(a))
    for a in edges(p, 2 * p):
        T.add("FP_REDUCE_ONCE", split32(a), arg=0)
    for a in [1, 2, p - 1, p - 2, 1 << 253, (1 << 232) - 1, R8 % p] + [rng.randrange(1, p) for _ in range(20)]:
        T.add("FP_INV", split32(a))


def _field29_rows(T, rng):
    p = T.p
    for a in edges(p, 1 << 256):
        T.add("TO29", split32(a))
    seeded = [rng.randrange(2 * p) for _ in range(4)]
    full = edges(p, R9)                                        # every k p + d below 2^261, ...
    for v in full:
        l = split29(v)
        T.add("RED29", l)
        T.add("RED29", untidy(l, rng))
        T.add("CN29", untidy(l, rng))
        T.add("SQR29", l)
    for _ in range(300):
        v = rng.randrange(R9)
        T.add("RED29", untidy(split29(v), rng))
        T.add("SQR29", split29(v))
    partners = [0, 1, p - 1, p, 2 * p - 1, R9 - 1, ((R9 - 1) >> 232 << 232) - 1, seeded[0]]
    for v in full:
        for w in partners + [v ^ 1, rng.randrange(R9)]:
            T.add("MUL29", split29(v) + split29(w))
    # limbs at the documented maximum: la * lb < 1.52 * 2^60 ("limbs < 2^30" for sqr29), limb 8 as large as 2^261 allows
    def worst(limb, top=True):
        low = limb * (((1 << 232) - 1) // M29)
        return [limb] * 8 + [((R9 - 1 - low) >> 232) if top else 0]
    root = int(LIMB_PRODUCT ** 0.5) - 1
    for la in (M29, (1 << 30) - 1, root, (1 << 31) - 1):
        lb = min((LIMB_PRODUCT - 1) // la, (1 << 32) - 1)
        for ta in (True, False):
            for tb in (True, False):
                T.add("MUL29", worst(la, ta) + worst(lb, tb))
                T.add("MUL29", worst(lb, tb) + worst(la, ta))
    for ta in (True, False):
        T.add("SQR29", worst((1 << 30) - 1, ta))
        T.add("SQR29", worst(M29, ta))
    for la, lb, lc in ((M29, 3 << 29, (1 << 30) - 1), ((1 << 30) - 1, M29, M29), (root, root // 2, M29)):
        ld = min((LIMB_PRODUCT - 1 - la * lb) // lc, (1 << 32) - 1)
        assert la * lb + lc * ld < LIMB_PRODUCT
        for t in (True, False):
            T.add("MULADD29", worst(la, t) + worst(lb, t) + worst(lc, t) + worst(ld, t))
            T.add("MULADD29", worst(lc, t) + worst(ld, not t) + worst(la, not t) + worst(lb, t))
    # the safe forms and the tests for zero: tidy values below 2p
    t2 = edges(p, 2 * p)
    few = [0, 1, p - 1, p, p + 1, 2 * p - 1] + seeded[:2]
    for a in t2:
        T.add("S_IS_ZERO", split29(a))
        T.add("S_DBL", split29(a))
        T.add("FROM29", split29(a))
        for b in few:
            T.add("S_ADD", split29(a) + split29(b))
            T.add("S_SUB", split29(a) + split29(b))
            T.add("S_SUB", split29(b) + split29(a))
    for k in range(7):
        for d in (-1, 0, 1):
            a = k * p + d
            if a < 0:
                continue
            for kk in range(6):
                T.add("IS_KP29", split29(a), arg=kk)
        for j in range(9):                                     # k p with one limb off by one: equal in every other limb
            l = split29(k * p)
            l[j] ^= 1
            T.add("IS_KP29", l, arg=k)
    for a in [1, 2, p - 1, p + 1, 2 * p - 1, R9 % p, R9 % p + p] + [rng.randrange(1, p) + (i & 1) * p for i in range(20)]:
        T.add("INV29", split29(a))


def _caller_shaped_rows(T, rng):
    """the lazy operands j9_madd makes on its way, from edge and seeded values below 2p"""
    p = T.p
    base = [0, 1, 2, p - 1, p, p + 1, 2 * p - 2, 2 * p - 1] + [rng.randrange(2 * p) for _ in range(4)]
    pds = []
    for u in base:
        for x in base:
            raw = sub_raw(split29(u), split29(x), p)           # U2 - X1 + 4p, in (2p, 6p)
            T.add("SUB29", split29(u) + split29(x))
            T.add("CN29", raw, shape="sub29")
            pd = u + 4 * p - x
            pds.append(pd)
            T.add("SQR29", split29(pd), lt2p=True)
            T.add("MUL29", split29(pd) + split29(mont29(pd, pd, p)), lt2p=True)          # PPP = Pd * PP
            T.add("MUL29", split29(x) + split29(mont29(pd, pd, p)), lt2p=True)           # Q = X1 * PP
            for k in (3, 4, 5):
                T.add("IS_KP29", split29(pd), arg=k)
    assert {3 * p, 4 * p, 5 * p} <= set(pds) and min(pds) > 2 * p and max(pds) < 6 * p
    for b in base:
        T.add("NEG29", split29(b))
        T.add("SHL29", neg_raw(split29(b), p), arg=1)
    # X3 = red29(R^2 + (4p - PPP) + 2 (4p - Q)): the three-term sum, below 14p
    small = [0, 1, p - 1, p, 2 * p - 1, base[8]]
    for s in small:
        for ppp in small:
            for q in small:
                n1, n2 = neg_raw(split29(ppp), p), shl_raw(neg_raw(split29(q), p), 1)
                T.add("ADD29", add_raw(split29(s), n1) + n2)
                T.add("RED29", add_raw(add_raw(split29(s), n1), n2), lt14p=True)
    # P.Y = muladd29(R, Q + 4p - X3, 4p - Y1, PPP)
    rs = [2 * p + 1, 3 * p, 4 * p, 5 * p, 6 * p - 1, pds[-1], pds[len(pds) // 2]]
    vals = [0, 1, p, 2 * p - 1, base[9], base[10]]
    combos = [(r, q, x3, y1, ppp) for r in rs for q in vals for x3 in vals for y1 in vals for ppp in vals]
    corners = [c for c in combos if all(v in (0, 2 * p - 1) for v in c[1:]) and c[0] in (2 * p + 1, 6 * p - 1)]
    for r, q, x3, y1, ppp in corners + rng.sample(combos, 600):
        qm, ny = sub_raw(split29(q), split29(x3), p), neg_raw(split29(y1), p)
        T.add("MULADD29", split29(r) + qm + ny + split29(ppp), lt2p=True)
        T.add("MUL29", split29(r) + qm)
        T.add("MUL29", ny + split29(ppp))


def _xyzz(P, z, p, reps=0):
    """affine -> X Y ZZ ZZZ (Montgomery, radix 2^261); bit i of `reps`: coordinate i as v + p"""
    c = [P[0] * z * z, P[1] * z * z * z, z * z, z * z * z]
    return [c[i] * R9 % p + (p if reps >> i & 1 else 0) for i in range(4)]


def _jac(P, z, p):
    return [P[0] * z * z * R8 % p, P[1] * z * z * z * R8 % p, z * R8 % p]


def _j9_words(c):
    return [w for v in c for w in split29(v)]


def _jac_words(c):
    return [w for v in c for w in split32(v)]


def _group_rows(T, rng, eight_limbs):
    p = T.p
    pts = E.random_points(T.curve, 10, seed=b"b3wit-commit-arith")
    zs = [1, p - 1, 2, rng.randrange(3, p)]
    other = {i: pts[(i + 3) % len(pts)] for i in range(len(pts))}
    zero9, hit_pd, hit_r = [0] * 36, set(), set()
    q_forms = [(1, 0), (1, 15), (2, 5), (zs[3], 0), (zs[3], 10), (p - 1, 15)]          # j9_add's second operand: z, representatives
    n = 0

    def z_with(P, coord):
        """a seeded z whose lift makes mul29(x2, ZZ) (coord 0) or mul29(y2, ZZZ) (coord 1) come out in [p, 2p) when P meets itself:
        the product of values below p and 2p is below (1 + 1/64)p, so a hash-derived point lands there once in a hundred times, and
        without these the differences of j9_madd would never be exactly 5p"""
        while True:
            z = rng.randrange(3, p)
            if mont29(P[coord] * R9 % p, _xyzz(P, z, p)[2 + coord], p) >= p:
                return z

    for i, P in enumerate(pts):
        for z in zs + [z_with(P, 0), z_with(P, 1)]:
            for reps in range(16):
                acc = _xyzz(P, z, p, reps)
                T.add("J9_DBL", _j9_words(acc), acc=P)
                for Q in (other[i], P, E.neg(P, p)):
                    x2, y2 = Q[0] * R9 % p, Q[1] * R9 % p
                    T.add("J9_MADD", _j9_words(acc) + split29(x2) + split29(y2), acc=P, q=Q)
                    pd = mont29(x2, acc[2], p) + 4 * p - acc[0]
                    if pd % p == 0:
                        hit_pd.add(pd // p)
                        hit_r.add((mont29(y2, acc[3], p) + 4 * p - acc[1]) // p if Q == P else None)
                    zq, rq = q_forms[n % len(q_forms)]
                    n += 1
                    T.add("J9_ADD", _j9_words(acc) + _j9_words(_xyzz(Q, zq, p, rq)), acc=P, q=Q)
        x2, y2 = P[0] * R9 % p, P[1] * R9 % p                  # infinity on either side
        T.add("J9_DBL", zero9, arg=1, acc=None)
        T.add("J9_MADD", zero9 + split29(x2) + split29(y2), arg=1, acc=None, q=P)
        T.add("J9_ADD", zero9 + _j9_words(_xyzz(P, zs[i % 4], p, i)), arg=1, acc=None, q=P)
        T.add("J9_ADD", _j9_words(_xyzz(P, zs[i % 4], p, i)) + zero9, arg=2, acc=P, q=None)
        T.add("J9_ADD", zero9 + zero9, arg=3, acc=None, q=None)
    # the table must reach every multiple the "H = 0 mod p" test of j9_madd knows, for P + P and P - P alike
    assert hit_pd == {3, 4, 5} and {3, 4, 5} <= hit_r, (hit_pd, hit_r)
    if not eight_limbs:
        return
    zero8 = [0] * 8
    for i, P in enumerate(pts):
        for z in zs:
            acc = _jac(P, z, p)
            T.add("JAC_DBL", _jac_words(acc), acc=P)
            T.add("JAC_TO_AFFINE", _jac_words(acc), acc=P)
            for Q in (other[i], P, E.neg(P, p)):
                T.add("JAC_MADD", _jac_words(acc) + split32(Q[0] * R8 % p) + split32(Q[1] * R8 % p), acc=P, q=Q)
                for zq in (1, 2, zs[3]):
                    T.add("JAC_ADD", _jac_words(acc) + _jac_words(_jac(Q, zq, p)), acc=P, q=Q)
        T.add("JAC_DBL", zero8 * 3, acc=None)
        T.add("JAC_TO_AFFINE", zero8 * 3, acc=None)
        T.add("JAC_MADD", zero8 * 3 + split32(P[0] * R8 % p) + split32(P[1] * R8 % p), acc=None, q=P)
        T.add("JAC_MADD", _jac_words(_jac(P, 2, p)) + zero8 * 2, acc=P, q=None)
        T.add("JAC_ADD", zero8 * 3 + _jac_words(_jac(P, 2, p)), acc=None, q=P)
        T.add("JAC_ADD", _jac_words(_jac(P, 2, p)) + zero8 * 3, acc=P, q=None)


@functools.lru_cache(maxsize=None)
def table(field):
    """The rows of one launch (field and instantiation).  The eight-limb routines do not see the instantiation: they run once
    per field, with the run-time modulus."""
    T = Table(field)
    rng = random.Random(0xB3C0 + field)
    T.add("CONSTS", [])
    if not T.const_modulus:
        _eight_limb_rows(T, rng)
    _field29_rows(T, rng)
    _caller_shaped_rows(T, rng)
    _group_rows(T, rng, eight_limbs=not T.const_modulus)
    T.rows.sort(key=lambda r: r[0])                            # rows of one routine side by side (stable: the order within stays)
    return T


# ---- the checks
class Wrong(Exception):
    pass


def _need(cond, what):
    if not cond:
        raise Wrong(what)


def _lazy_product(p, r, num, lt2p=False):
    """r = num / 2^261 mod p, tidy, below num / (64 p) + p"""
    _need(is_tidy(r), "not tidy")
    rv = val29(r)
    _need((rv * R9 - num) % p == 0, "wrong value modulo p")
    _need(rv * 64 * p < num + 64 * p * p, "not below (AB/64 + 1)p")
    if lt2p:
        _need(rv < 2 * p, "not below 2p where j9_madd needs it")


def _reduced(p, r, v):
    _need(is_tidy(r), "not tidy")
    _need(val29(r) < 2 * p, "not below 2p")
    _need((val29(r) - v) % p == 0, "wrong value modulo p")


def _affine9(c, p):
    return (c[0] * pow(c[2], -1, p) % p, c[1] * pow(c[3], -1, p) % p)


def _check_j9(p, out, want):
    _need(out[36] == (1 if want is None else 0), f"inf flag {out[36]}, the sum is {'infinity' if want is None else 'finite'}")
    if want is None:
        return
    limbs = [out[9 * i:9 * i + 9] for i in range(4)]
    c = [val29(l) for l in limbs]
    _need(all(is_tidy(l) for l in limbs), "a coordinate is not tidy")
    _need(all(v < 2 * p for v in c), "a coordinate is not below 2p")
    _need(c[2] % p != 0 and c[3] % p != 0, "ZZ or ZZZ is zero on a finite point")
    _need((c[2] ** 3 - c[3] ** 2 * R9) % p == 0, "ZZ^3 != ZZZ^2")
    _need(_affine9(c, p) == want, "not the sum ec_ref.add gives")


def _check_jac(p, out, want):
    c = [val32(out[8 * i:8 * i + 8]) for i in range(3)]
    _need(all(v < p for v in c), "a coordinate is not canonical")
    _need((c[2] == 0) == (want is None), f"Z {'=' if c[2] == 0 else '!='} 0, the sum is {'infinity' if want is None else 'finite'}")
    if want is None:
        return
    zi = pow(c[2], -1, p)
    got = (c[0] * R8 * zi * zi % p, c[1] * R8 * R8 * zi * zi * zi % p)
    _need(got == want, "not the sum ec_ref.add gives")


def check_consts(p, out, const_modulus):
    """make_curve / make_curve9 against Python"""
    C = dict(p=val32(out[0:8]), r2=val32(out[8:16]), one=val32(out[16:24]), pm2=val32(out[24:32]), inv=int(out[32]))
    _need(C["p"] == p, "make_curve: p")
    _need(C["one"] == R8 % p, "make_curve: one")
    _need(C["r2"] == R8 * R8 % p, "make_curve: r2")
    _need(C["pm2"] == p - 2, "make_curve: pm2")
    _need(C["inv"] == (-pow(p, -1, 1 << 32)) % (1 << 32), "make_curve: inv")
    p9, sp4, one9 = [int(x) for x in out[33:42]], [int(x) for x in out[42:51]], [int(x) for x in out[51:60]]
    _need(p9 == split29(p), "make_curve9: p" + (" (the compile-time limbs)" if const_modulus else ""))
    _need(one9 == split29(R9 % p), "make_curve9: one")
    _need(int(out[60]) == (-pow(p, -1, 1 << 29)) % (1 << 29), "make_curve9: inv")
    _need(int(out[61]) in ((1 << 269) // p, (1 << 269) // p - 1), "make_curve9: mu is not floor(2^269 / p) or one less")
    _need([int(x) for x in out[62:65]] == [(k * p) & M29 for k in (3, 4, 5)], "make_curve9: kp0")
    _need(val29(sp4) == 4 * p, "make_curve9: sp4 does not sum to 4p")
    _need(sp4 == sp4_limbs(p), "make_curve9: sp4 limbs are not lifted as described")
    _need(all(s >= M29 for s in sp4[:8]) and sp4[8] >= (2 * p - 1) >> 232, "make_curve9: an sp4 limb can go negative under a tidy value below 2p")


def check_row(T, row, out):
    """raises Wrong(what) when `out`, the raw result of `row`, breaks a promise of the header"""
    p = T.p
    op, arg, w, info = row
    name = OP_NAME[op]
    out = [int(x) for x in out]
    _need(out[OUT_WORDS - 1] != 0xBADC0DE, "the probe does not know the operation")
    f8 = lambda i: val32(w[8 * i:8 * i + 8])
    l9 = lambda i: w[9 * i:9 * i + 9]
    f9 = lambda i: val29(l9(i))
    if name == "CONSTS":
        check_consts(p, out, T.const_modulus)
    elif name in ("FP_ADD", "FP_SUB", "FP_MUL", "FP_SQR", "FP_DBL", "FP_INV", "FP_REDUCE_ONCE"):
        a, b = f8(0), f8(1)
        want = {"FP_ADD": lambda: (a + b) % p, "FP_SUB": lambda: (a - b) % p, "FP_MUL": lambda: a * b * pow(R8, -1, p) % p,
                "FP_SQR": lambda: a * a * pow(R8, -1, p) % p, "FP_DBL": lambda: 2 * a % p, "FP_INV": lambda: pow(a, -1, p) * R8 * R8 % p,
                "FP_REDUCE_ONCE": lambda: a % p}[name]()
        _need(val32(out[:8]) == want, f"got {val32(out[:8]):#x}, want {want:#x}")
    elif name == "TO29":
        _need(out[:9] == split29(f8(0)), "not the nine 29-bit limbs of the value")
    elif name == "FROM29":
        v = f9(0)
        _need(val32(out[:8]) == v % R8 and out[8] == v >> 256, "from29: not the value's words and the bits above 2^256")
        _need(val32(out[9:17]) == v % p, "fp_reduce_once(from29): not the canonical value")
    elif name == "MUL29":
        _lazy_product(p, out[:9], f9(0) * f9(1), info.get("lt2p", False))
    elif name == "SQR29":
        _lazy_product(p, out[:9], f9(0) ** 2, info.get("lt2p", False))
    elif name == "MULADD29":
        _lazy_product(p, out[:9], f9(0) * f9(1) + f9(2) * f9(3), info.get("lt2p", False))
    elif name == "CN29":
        _need(is_tidy(out[:9]) and val29(out[:9]) == f9(0), "not the same value, tidy")
    elif name == "RED29":
        if info.get("lt14p"):
            assert f9(0) < 14 * p
        _reduced(p, out[:9], f9(0))
    elif name == "S_ADD":
        _reduced(p, out[:9], f9(0) + f9(1))
    elif name == "S_SUB":
        _reduced(p, out[:9], f9(0) - f9(1))
    elif name == "S_DBL":
        _reduced(p, out[:9], 2 * f9(0))
    elif name == "ADD29":
        _need(out[:9] == add_raw(l9(0), l9(1)), "not the limb sums")
    elif name == "SUB29":
        _need(val29(out[:9]) == f9(0) + 4 * p - f9(1), "not a + 4p - b")
        _need(all(o < x + (1 << 30) for o, x in zip(out[:9], l9(0))), "a limb is not below a's + 2^30")
        _need(out[:9] == sub_raw(l9(0), l9(1), p), "not a + sp4 - b limb by limb")
    elif name == "NEG29":
        _need(val29(out[:9]) == 4 * p - f9(0) and out[:9] == neg_raw(l9(0), p), "not 4p - b, limb by limb from sp4")
    elif name == "SHL29":
        _need(out[:9] == shl_raw(l9(0), arg), "not the limbs shifted")
    elif name == "IS_KP29":
        _need(out[0] == (1 if f9(0) == arg * p else 0), f"is_kp29 says {out[0]} for {f9(0) // p} p + {f9(0) % p} and k = {arg}")
    elif name == "S_IS_ZERO":
        _need(out[0] == (1 if f9(0) % p == 0 else 0), f"s_is_zero says {out[0]} for {f9(0) // p} p + {f9(0) % p}")
    elif name == "INV29":
        _need(is_tidy(out[:9]) and val29(out[:9]) < 2 * p, "not tidy below 2p")
        _need(val29(out[:9]) * f9(0) % p == R9 * R9 % p, "not the inverse")
    elif name in ("J9_DBL", "J9_MADD", "J9_ADD"):
        A, Q = info["acc"], info.get("q")
        _check_j9(p, out, E.add(A, A if name == "J9_DBL" else Q, p))
    elif name in ("JAC_DBL", "JAC_MADD", "JAC_ADD"):
        A, Q = info["acc"], info.get("q")
        _check_jac(p, out, E.add(A, A if name == "JAC_DBL" else Q, p))
    elif name == "JAC_TO_AFFINE":
        A = info["acc"]
        want = (0, 0) if A is None else (A[0] * R8 % p, A[1] * R8 % p)
        _need((val32(out[:8]), val32(out[8:16])) == want, "not the affine point in Montgomery form ((0, 0) for infinity)")
    else:
        raise AssertionError(name)


def check(T, results, limit=12):
    """the failures of a launch's raw results (n x OUT_WORDS), as readable lines; [] when every promise holds"""
    assert results.shape == (len(T.rows), OUT_WORDS), results.shape
    bad = []
    for i, row in enumerate(T.rows):
        try:
            check_row(T, row, results[i])
        except Wrong as e:
            if len(bad) < limit:
                bad.append(f"{FIELD_NAMES[T.field]} {OP_NAME[row[0]].lower()} row {i}: {e}; arg {row[1]}, operands "
                           + " ".join(f"{x:#x}" for x in row[2]))
            else:
                bad.append(None)
    n = len(bad)
    bad = [b for b in bad if b]
    if n > len(bad):
        bad.append(f"... and {n - len(bad)} more rows")
    return bad
