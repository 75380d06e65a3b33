"""Plans for the on-device constraint check (csrc/b3w_r1cs_walk.hip, b3w_r1cs.hip, b3w_r1cs_device.h), pure Python, no GPU:

  * changed_violated / row_plan / plan_expect: single-wire changes of a valid body that between them violate EVERY row of a committed
    system — the non-booleanity rows while the body stays on the walk kernel's fast road ("on"), the booleanity rows and the one row no
    canonical value can violate on the road to the deferred kernel ("off") — with the plain-integer count and first violated row;
  * edge_system / edge_bodies / edge_expect: a synthetic system over a context's wires whose rows sit on the thresholds of the 64-bit
    fast road, and bodies of edge values, each class once satisfied and once as a near miss a lossy 64/128-bit comparison would accept.

Every expected verdict is plain-integer arithmetic on Python ints.  The thresholds quoted here are the kernels' (file:line in DESIGN.md
8c); nothing is taken from a run of the code under test.  tests/test_r1cs_cases_cpu.py proves the plans; tests/test_gpu_r1cs_rows.py runs them."""
import r1cs_ref as R

NONE = 0xFFFFFFFF
TILE = 1024                      # B3W_R1CS_TILE
SPLIT_GEN = 320                  # B3W_WALK_SPLIT_GEN: a tile with more general rows becomes several units
WIDE_CAP = 224                   # B3W_WALK_WIDE_CAP: wide records per body


# ---------------------------------------------------------------------------------------------------------------- committed systems
_committed = {}


def committed(circuit):
    """-> (the committed system, the valid body under every row plan as ints): body 1 of the ORACLE's witnesses for
    workloads.config2_compression(4, first=50) / config3_nova(4, first=50)"""
    if circuit not in _committed:
        import b3w_testlib as T
        path = R.BUILTIN if circuit == "compression" else R.BUILTIN_NOVA_O1 if circuit == "nova_bn254_o1" else R.BUILTIN_NOVA_O2[circuit]
        W = T.workloads()
        recs = W.config2_compression(4, first=50) if circuit == "compression" else W.config3_nova(4, first=50)
        bad, bodies = T.oracle_batch_u32(circuit, recs)
        assert bad == 0
        _committed[circuit] = (R.parse(R.read_image(path)), R.body_to_ints(bodies[1]))
    return _committed[circuit]


def booleanity_wire(row):
    """w if the row is  w * (w - 1) = 0  (A = {w: 1}, B = {w: 1, 0: -1} — or its negation {w: -1, 0: 1} —, C empty, w != 0), else None"""
    a, b, c = row[:3]
    if c or len(a) != 1 or len(b) != 2:
        return None
    (w, f), = a.items()
    if w == 0 or f != 1 or set(b) != {0, w}:
        return None
    return w if (b[w], b[0]) in ((1, -1), (-1, 1)) else None


def _signed(sys_):
    """the system's rows with coefficients as signed numbers (c or c - p), cached on the dict"""
    if "_signed" not in sys_:
        p = sys_["prime"]
        h = p >> 1
        sys_["_signed"] = [tuple({w: (f if f <= h else f - p) for w, f in lc.items()} for lc in row) for row in sys_["constraints"]]
    return sys_["_signed"]


def bool_rows(sys_):
    """{row: wire} of the booleanity rows"""
    if "_bool" not in sys_:
        sys_["_bool"] = {k: w for k, w in ((k, booleanity_wire(row)) for k, row in enumerate(_signed(sys_))) if w is not None}
    return sys_["_bool"]


class BodyView:
    """a body (uint8 [nwires * 32]) read as z[w] -> int, element by element"""
    def __init__(self, body):
        self.body = body

    def __getitem__(self, w):
        return int.from_bytes(self.body[32 * w:32 * w + 32].tobytes(), "little")


def changed_violated(sys_, z, w, by_wire):
    """The violated rows of a body that satisfied every row before z[w] was changed (z already holds the new value): only rows that read
    w can be.  An element >= p spoils every row that reads it; every other element is known to be canonical, so only z[w] is looked at."""
    rows = by_wire.get(w, ())
    p = sys_["prime"]
    if z[w] >= p:
        return list(rows)
    cons = _signed(sys_)
    out = []
    for k in rows:
        a, b, c = cons[k]
        sa = sb = sc = 0
        for x, f in a.items():
            sa += f * z[x]
        for x, f in b.items():
            sb += f * z[x]
        for x, f in c.items():
            sc += f * z[x]
        if (sa * sb - sc) % p:
            out.append(k)
    return out


def _first_is(sys_, z, w, by_wire, row):
    """is `row` the LOWEST violated row after the change of z[w]?  (rows in ascending order; leaves at the first violated one)"""
    p = sys_["prime"]
    cons = _signed(sys_)
    for k in by_wire[w]:
        if k > row:
            return False
        a, b, c = cons[k]
        if (sum(f * z[x] for x, f in a.items()) * sum(f * z[x] for x, f in b.items()) - sum(f * z[x] for x, f in c.items())) % p:
            return k == row
    return False


def row_plan(sys_, z):
    """-> [(wire, new value, road)] over the valid body z (ints).  Roads:
    on      keeps the body on the fast road: a wire with a booleanity row gets old ^ 1; any other wire (but wire 0) with old < 2^62 gets
            old + 1 and, if old > 0, old - 1; wider wires are left alone
    off     sends the tile to the deferred kernel: every booleanity wire -> 2 and -> p - 1; wire 0 -> 0, 2 and p + 1 (no canonical
            representative: the only way to violate a row  1 * () = ()); every wire of 2^64 or more (IsZero inverses) -> old + 1
    top-up  for each non-booleanity row no on case reaches as the FIRST violated row: other on-road values of its wires (old +- 2, 0 / 1,
            a word's old ^ 2^31; all below 2^62), the first that makes the row the lowest violated one"""
    p = sys_["prime"]
    by_wire = R.rows_of_wire(sys_)
    brow = bool_rows(sys_)
    bwires = set(brow.values())
    plan, firsts = [], set()
    z = list(z)
    for w in range(1, sys_["n_wires"]):
        old = z[w]
        news = [old ^ 1] if w in bwires else ([old + 1] + ([old - 1] if old > 0 else [])) if old < 1 << 62 else []
        for new in news:
            plan.append((w, new, "on"))
            z[w] = new
            v = changed_violated(sys_, z, w, by_wire)
            if v:
                firsts.add(v[0])
        z[w] = old
    for w in sorted(bwires):
        plan += [(w, 2, "off"), (w, p - 1, "off")]
    plan += [(0, 0, "off"), (0, 2, "off"), (0, p + 1, "off")]
    for w in range(1, sys_["n_wires"]):
        if z[w] >= 1 << 64:
            plan.append((w, z[w] + 1, "off"))
    have = {(w, new) for w, new, _ in plan}
    for k, row in enumerate(sys_["constraints"]):
        if k in brow or k in firsts:
            continue
        done = False
        for w in sorted(row[0].keys() | row[1].keys() | row[2].keys()):
            if w == 0 or w in bwires or z[w] >= 1 << 62:
                continue
            old = z[w]
            for new in (old + 2, old - 2, 0, 1, old ^ (1 << 31)):
                if not 0 <= new < 1 << 62 or new == old or (w, new) in have:
                    continue
                z[w] = new
                ok = _first_is(sys_, z, w, by_wire, k)
                z[w] = old
                if ok:
                    plan.append((w, new, "top-up"))
                    have.add((w, new))
                    firsts.add(k)
                    done = True
                    break
            if done:
                break
    return plan


def plan_expect(sys_, z, plan):
    """-> [(count, first violated row or NONE)] per case, by changed_violated"""
    by_wire = R.rows_of_wire(sys_)
    z = list(z)
    out = []
    for w, new, _road in plan:
        old = z[w]
        z[w] = new
        v = changed_violated(sys_, z, w, by_wire)
        z[w] = old
        out.append((len(v), v[0] if v else NONE))
    return out


# --------------------------------------------------------------------------------------------------------------------- edge systems
# Coefficients at the edges of "small" (|c| < 2^62: b3w_r1cs_host.cpp:187,194), one shifting (2^61), one from the table (3 * 2^40), the
# two whose product with 2^63 - 1 has a high word just below and at 2^39 (2^40, 2^41), one negative shift, one of 250 bits (always deferred)
def edge_coefs(p):
    return [("1", 1), ("2^62-1", (1 << 62) - 1), ("2^62", 1 << 62), ("-(2^62-1)", p - ((1 << 62) - 1)), ("-2^62", p - (1 << 62)),
            ("2^61", 1 << 61), ("3*2^40", 3 << 40), ("2^40", 1 << 40), ("2^41", 1 << 41), ("-2^40", p - (1 << 40)), ("4", 4), ("-3", p - 3),
            ("250bit", (1 << 249) + 12345)]


def edge_elements(p):
    return [("2^62", 1 << 62), ("2^63-1", (1 << 63) - 1), ("2^63", 1 << 63), ("2^63+1", (1 << 63) + 1), ("2^64-1", (1 << 64) - 1), ("2^64", 1 << 64),
            ("p-1", p - 1), ("p-2^32", p - (1 << 32)), ("p-2^62+1", p - (1 << 62) + 1), ("p-2^62", p - (1 << 62)), ("p-2^62-1", p - (1 << 62) - 1),
            ("p-2^63", p - (1 << 63)), ("p", p), ("p+1", p + 1), ("2^256-1", (1 << 256) - 1)]


class _Builder:
    def __init__(self, p, nw):
        self.p, self.nw, self.cons, self.rows, self.g, self.nxt = p, nw, [], {}, {}, {}

    def wire(self, tile, n=None):
        start = self.nxt.get(tile, max(1, tile * TILE))
        k = 1 if n is None else n
        assert start + k <= min(self.nw, (tile + 1) * TILE), ("tile full", tile)
        self.nxt[tile] = start + k
        return start if n is None else list(range(start, start + k))

    def row(self, name, pa, pb, pc, **wires):
        self.rows[name] = len(self.cons)
        self.cons.append(tuple({w: f % self.p for w, f in lc.items()} for lc in (pa, pb, pc)))
        self.g[name] = wires


def edge_system(prime, nwires):
    """-> dict(prime, n_wires, constraints, rows={name: row}, g={name: its wires}, tiles=...).  Rows of simple shapes over dedicated wires in
    tile 0, a middle tile, a tile of more than SPLIT_GEN general rows (two units), a tile of 230 rows with a wide term, and the last tile;
    operands exported from earlier tiles; everything else of a body is zero and wire 0 is 1, which satisfies every row."""
    p = prime
    ntiles = (nwires + TILE - 1) // TILE
    t0, tm, ts, tw, tl = 0, 7, 12, 15, ntiles - 1
    B = _Builder(p, nwires)

    def c3(tile):                                         # a C part that can hold a product three ways: small (z0 + 2^61 z2), or one element zw
        z0, z2, zw = B.wire(tile, 3)
        return {z0: 1, z2: 1 << 61, zw: 1}, dict(z0=z0, z2=z2, zw=zw)

    def bools(tile, n, tag):
        ws = B.wire(tile, n)
        for i, w in enumerate(ws):
            B.row(f"bool_{tag}{i}", {w: 1}, {w: 1, 0: -1}, {}, b=w)
        return ws
    # tile 0
    b0 = bools(t0, 4, "t0_")
    x, y = B.wire(t0, 2)
    c, zs = c3(t0)
    B.row("mul_loc", {x: 1}, {y: 1}, c, x=x, y=y, **zs)
    xe = B.wire(t0)                                       # read by the middle tile only: exported
    ye0 = B.wire(t0)
    # middle tile
    bm = bools(tm, 8, "tm_")
    rw = B.wire(tm)
    B.row("run", {w: 1 << (3 + i) for i, w in enumerate(bm)}, {0: 1}, {rw: 1}, bits=bm, z=rw)
    y = B.wire(tm)
    c, zs = c3(tm)
    B.row("mul_exp", {xe: 1}, {y: 1}, c, x=xe, y=y, **zs)
    bfree = bools(tm, 2, "tmf_")                          # (no other row reads these)
    for name, sa, sb in (("sum2p", 1, 1), ("sum2n", -1, 1), ("sqn", 1, -1)):
        x0, x1, y0, y1 = B.wire(tm, 4)
        c, zs = c3(tm)
        B.row(name, {x0: sa, x1: sa}, {y0: sb, y1: sb}, c, x0=x0, x1=x1, y0=y0, y1=y1, **zs)
    for name, k in (("lin2a", 1), ("lin2b", 2)):
        x0, x1 = B.wire(tm, 2)
        c, zs = c3(tm)
        B.row(name, {x0: k, x1: -k}, {0: 1}, c, x0=x0, x1=x1, **zs)
    for n in (64, 65, 300):
        xs = B.wire(tm, n)
        c, zs = c3(tm)
        B.row(f"lin{n}", {w: (4, 8, 3 << 40, -4)[i % 4] for i, w in enumerate(xs)}, {0: 1}, c, xs=xs, **zs)
    xa, ya, we = B.wire(tm, 3)                            # operands and a wide element the last tile reads
    # the tile of two units: one row per edge coefficient, then 330 filler rows  fx * fy = fz_i
    for i, (name, cf) in enumerate(edge_coefs(p)):
        x, y = B.wire(ts, 2)
        c, zs = c3(ts)
        B.row(f"coef_{name}", {x: cf}, {y: 1}, c, x=x, y=y, **zs)
        x, y = B.wire(ts, 2)
        c, zs = c3(ts)
        B.row(f"coefneg_{name}", {x: 1}, {y: cf}, c, x=x, y=y, **zs)
    fx, fy = B.wire(ts, 2)
    fz = B.wire(ts, 330)
    for i, w in enumerate(fz):
        B.row(f"fill{i}", {fx: 1}, {fy: 1}, {w: 1}, x=fx, y=fy, z=w)
    # 230 rows  (x + W_i) * y = z_i
    x, y = B.wire(tw, 2)
    ws, zz = B.wire(tw, 230), B.wire(tw, 230)
    for i in range(230):
        B.row(f"many{i}", {x: 1, ws[i]: 1}, {y: 1}, {zz[i]: 1}, x=x, y=y, W=ws[i], z=zz[i])
    # last tile
    bl = bools(tl, 4, "tl_")
    z = B.wire(tl)
    B.row("mul_allexp", {xa: 1}, {ya: 1}, {z: 1}, x=xa, y=ya, zw=z)       # both operands come through the export area
    for name, a, b, c in (("wc", {}, {}, 1), ("wc_n", {}, {}, -1), ("wa", 1, {}, 0), ("wa_n", -1, {}, 0), ("wb_n", {}, -1, 0), ("wb", {}, 1, 0), ("wk2", 2, {}, 0)):
        x, y, W, z = B.wire(tl, 4)
        B.row(name, {x: 1, **({W: a} if a else {})}, {y: 1, **({W: b} if b else {})}, {z: 1, **({W: c} if c else {})}, x=x, y=y, W=W, z=z)
    x, y, W1, W2, z = B.wire(tl, 5)
    B.row("w2", {x: 1, W1: 1}, {y: 1}, {z: 1, W2: 1}, x=x, y=y, W=W1, W2=W2, z=z)
    x, y, z = B.wire(tl, 3)
    B.row("wa_exp", {x: 1, we: 1}, {y: 1}, {z: 1}, x=x, y=y, W=we, z=z)
    x = B.wire(tl)
    c, zs = c3(tl)
    B.row("mul_last", {x: 1}, {ye0: 1}, c, x=x, y=ye0, **zs)              # a general row behind the last tile's booleanity wires
    return dict(prime=p, n_wires=nwires, constraints=B.cons, rows=B.rows, g=B.g, tiles=dict(t0=t0, tm=tm, ts=ts, tw=tw, tl=tl),
                bools=dict(t0=b0, tm=bfree, tl=bl))


def _dot(lc, val, p):
    return sum(f * val(w) for w, f in lc.items()) % p


def _misses(t, ab, p):
    """near misses of a target t = a * b - (rest): what a comparison of 52, 64, 104, 116 or 128 bits, or of the low words alone, takes for t"""
    out = [t + (1 << 52), t + (1 << 64), t + (1 << 104), t + (1 << 116), (t + (1 << 128)) % p]
    if ab is not None:
        out.append(ab % (1 << 64))
    if 0 <= t - p + (1 << 128) < p:
        out.append(t - p + (1 << 128))
    return [v % p for v in out if v % p != t]


def edge_bodies(E):
    """-> [dict(cls=class name, set={wire: value})]: a body is zero but for wire 0 = 1 and `set`"""
    p, g, cons, rows = E["prime"], E["g"], E["constraints"], E["rows"]
    out = []
    h = p >> 1
    sgn = lambda v: v if v <= h else v - p                # (for the integer product a * b of small signed sums)

    def solve(cls, name, vals, nmiss=1, rot=0, setv=None, both=True):
        """a satisfied body of row `name` for operand values `vals` (by the row's wire names; or `setv` by wire): the target written into zw
        and, when it is below 2^103, a second body with it in z0 + 2^61 z2; then `nmiss` near misses, in one form or (`both`) in each"""
        w = g[name]
        setv = {w[k]: v for k, v in vals.items()} if setv is None else setv
        a, b, c = cons[rows[name]]
        val = lambda x: setv.get(x, 1 if x == 0 else 0)
        az, bz = _dot(a, val, p), _dot(b, val, p)
        t = (az * bz - _dot(c, val, p)) % p
        small = "z0" in w and t < 1 << 103
        out.append(dict(cls=cls, set={**setv, w["zw"]: t}))
        if small:
            out.append(dict(cls=cls, set={**setv, w["z0"]: t % (1 << 61), w["z2"]: t >> 61}))
        ms = _misses(t, sgn(az) * sgn(bz) if abs(sgn(az)) < 1 << 64 and abs(sgn(bz)) < 1 << 64 else None, p)
        ms = ms[rot % len(ms):] + ms[:rot % len(ms)]
        for q, m in enumerate(ms[:nmiss]):
            as_small = small and m < 1 << 123
            if both or not as_small or (rot + q) % 2 == 0:
                out.append(dict(cls=cls, set={**setv, w["zw"]: m}))
            if as_small and (both or (rot + q) % 2 == 1):
                out.append(dict(cls=cls, set={**setv, w["z0"]: m % (1 << 61), w["z2"]: m >> 61}))
    # elements: each as a local operand, as an exported one, and where both operands are exported
    for i, (name, e) in enumerate(edge_elements(p)):
        solve(f"element {name}", "mul_loc", dict(x=e, y=3), 1, i)
        solve(f"element {name}", "mul_exp", dict(x=e, y=(1 << 61) + 1), 1, i + 1)
        solve(f"element {name}", "mul_allexp", dict(x=e, y=5), i & 1, i + 2)
    # coefficients, and the term products they make with elements at the edges of the high word (2^39) and of one counter (2^54)
    for i, (name, cf) in enumerate(edge_coefs(p)):
        solve(f"coefficient {name}", f"coef_{name}", dict(x=(1 << 63) - 1 if i & 1 else 3, y=7), 1, i, both=False)
        solve(f"coefficient {name}", f"coefneg_{name}", dict(x=p - 5, y=7), 1, i + 1, both=False)
    for i, (name, x) in enumerate((("2^40", (1 << 63) - 1), ("2^41", (1 << 63) - 1), ("2^41", (1 << 62) - 1), ("4", (1 << 52) - 1), ("4", 1 << 52), ("4", (1 << 52) + 1),
                                   ("-2^40", p - ((1 << 62) - 1)), ("-3", p - (1 << 62)), ("-3", p - 1), ("3*2^40", (1 << 62) + 1))):
        solve("term product", f"coef_{name}", dict(x=x, y=1 if i % 3 else (1 << 63) - 1), 1, i, both=False)
    # sums: 64, 65 and 300 terms of 2^52 - 1, 2^52 (carries across the split of the two counters) and 2^62 - 1
    for n in (64, 65, 300):
        for k, v in enumerate(((1 << 52) - 1, 1 << 52, (1 << 62) - 1)):
            solve(f"sum of {n} terms", f"lin{n}", None, 1, k, setv={x: v - (i % 3 == 2) for i, x in enumerate(g[f"lin{n}"]["xs"])}, both=False)
    big = 1 << 62
    # positive and negative terms cancelling to exactly 0, +-1, +-2^52 (lin2a: x0 - x1) and +-(2^63 - 2), +-2^63 (lin2b: 2 x0 - 2 x1)
    for name, ds in (("lin2a", (0, 1, -1, 1 << 52, -(1 << 52))), ("lin2b", (0, big - 1, 1 - big, big, -big))):
        for i, d in enumerate(ds):
            x0 = 7 + max(d, 0)
            solve("cancelling sum", name, dict(x0=x0, x1=x0 - d), 1, i, both=False)
    # a part equal to +-(2^63 - 1), +-2^63, +-(2^63 + 1); a * b at +-(2^63 - 1)^2
    for i, name in enumerate(("sum2p", "sum2n", "sqn")):
        for j, x1 in enumerate((big - 1, big, big + 1)):
            for q, (y0, y1) in enumerate(((1, 0), (big, big - 1))):
                solve("part at the edge of 64 bits", name, dict(x0=big, x1=x1, y0=y0, y1=y1), 1, i + j + q, both=False)
    # wide records: k * W = d with k = s * (the other factor), d = c - a * b
    inv = lambda v: pow(v, p - 2, p)
    ks = [("0", 0), ("1", 1), ("-1", p - 1), ("2^32-1", (1 << 32) - 1), ("2^32", 1 << 32), ("-(2^32-1)", p - (1 << 32) + 1), ("-2^32", p - (1 << 32)), ("3", 3)]
    def wide(x, y, z, s_a=0, s_b=0, s_c=0, coef=1):
        """W that satisfies the row for small x, y, z, or None where any W does"""
        if s_a:
            return None if y % p == 0 else (s_a * inv(coef) * (z * inv(y) - x)) % p
        if s_b:
            return None if x % p == 0 else (s_b * (z * inv(x) - y)) % p
        return (s_c * (x * y - z)) % p
    shapes = dict(wa=dict(s_a=1), wb_n=dict(s_b=-1), wc=dict(s_c=1), wa_n=dict(s_a=-1), wb=dict(s_b=1), wc_n=dict(s_c=-1), wk2=dict(s_a=1, coef=2), wa_exp=dict(s_a=1))
    for si, (name, kw) in enumerate(shapes.items()):
        w = g[name]
        for ki, (_name, k) in enumerate(ks if si < 3 else (ks[1], ks[6], ks[7])):
            x, y, z = (11, k, 1000) if "s_a" in kw else (k, 13, 1000) if "s_b" in kw else (k, 1 << 40, 77)
            cls = f"wide record {name}"
            W = wide(x, y, z, **kw)
            if W is None:                                 # k = 0: 0 * (x + W) = z holds for z = 0 and any W
                W = (1 << 200) + 9
                out.append(dict(cls=cls, set={w["x"]: x, w["y"]: y, w["z"]: 0, w["W"]: W}))
                out.append(dict(cls=cls, set={w["x"]: x, w["y"]: y, w["z"]: 1 << 64, w["W"]: W}))
                continue
            base = {w["x"]: x, w["y"]: y, w["z"]: z, w["W"]: W}
            out.append(dict(cls=cls, set=base))
            out.append(dict(cls=cls, set={**base, w["W"]: (W + 1) % p} if ki & 1 else {**base, w["z"]: z + (1 << 64)}))
        base = {w["x"]: 11, w["y"]: 3, w["z"]: 1000}
        W = wide(11, 3, 1000, **kw)
        out.append(dict(cls=f"wide record {name}", set={**base, w["W"]: W + p if W + p < 1 << 256 else (1 << 256) - 1}))       # W wild
    w = g["w2"]                                           # two wide terms in one row
    for W2 in ((1 << 100) + 1, p - (1 << 70)):
        W1 = ((1000 + W2) * inv(3) - 11) % p
        base = {w["x"]: 11, w["y"]: 3, w["z"]: 1000, w["W"]: W1, w["W2"]: W2}
        out += [dict(cls="wide record two terms", set=base), dict(cls="wide record two terms", set={**base, w["W2"]: W2 + 1})]
    # d = c - a * b negative and large: x * y - z with x, y at the edge of 64 bits
    w = g["wc"]
    for x, y in (((1 << 63) - 1, (1 << 63) - 1), (p - ((1 << 62) - 1), (1 << 63) - 1), (1 << 62, 1 << 62)):
        W = (x * y - 5) % p
        base = {w["x"]: x, w["y"]: y, w["z"]: 5, w["W"]: W}
        out += [dict(cls="wide record large d", set=base), dict(cls="wide record large d", set={**base, w["W"]: (W + (1 << 64)) % p}),
                dict(cls="wide record large d", set={**base, w["W"]: (W + (1 << 128)) % p})]
    # more wide rows than a body's list of records holds (WIDE_CAP = 224): all satisfied; violated on both sides of the 224th
    m = [g[f"many{i}"] for i in range(230)]
    def many(bad):
        s = {m[0]["x"]: 11, m[0]["y"]: 3}
        for i, w in enumerate(m):
            s[w["z"]] = 3 * (1000 + i) + 1                # (no multiple of 3: W = z / 3 - x is a full field element in every row)
            s[w["W"]] = ((3 * (1000 + i) + 1) * inv(3) - 11 + (1 if i in bad else 0)) % p
        return s
    out += [dict(cls="230 wide rows", set=many(())), dict(cls="230 wide rows", set=many((5, 222, 223, 224, 225, 229))), dict(cls="230 wide rows", set=many((224,))),
            dict(cls="230 wide rows", set=many((229,))), dict(cls="230 wide rows", set=many(range(230)))]
    # the tile of two units: every filler row satisfied; some violated in both units
    f = [g[f"fill{i}"] for i in range(330)]
    def fill(bad):
        s = {f[0]["x"]: 1 << 20, f[0]["y"]: 3}
        for i, w in enumerate(f):
            s[w["z"]] = (3 << 20) + (1 if i in bad else 0)
        return s
    out += [dict(cls="split tile", set=fill(())), dict(cls="split tile", set=fill((0, 151, 152, 153, 329))), dict(cls="split tile", set=fill((329,))), dict(cls="split tile", set=fill((152,)))]
    # careful mode: a 2 or p - 1 where a booleanity wire sits, in tile 0, the middle tile, the last tile — with satisfied and violated general rows
    # in the tiles behind it — and wire 0 that is not 1
    ml, me, mz = g["mul_loc"], g["mul_exp"], g["mul_last"]
    good = {ml["x"]: 6, ml["y"]: 7, ml["z0"]: 42, me["x"]: 5, me["y"]: 9, me["z0"]: 45, mz["x"]: 3, mz["y"]: 4, mz["z0"]: 12, **fill(())}
    for late in ({}, {mz["z0"]: 13, me["z0"]: 44, f[200]["z"]: 1}):
        out.append(dict(cls="careful none", set={**good, **late}))
        for tag in ("t0", "tm", "tl"):
            for v in (2, p - 1):
                out.append(dict(cls=f"careful {tag}", set={**good, **late, E["bools"][tag][1]: v}))
                out.append(dict(cls=f"careful {tag}", set={**good, **late, E["bools"][tag][1]: 1}))
        for v in (0, p + 1, 2):
            out.append(dict(cls="careful wire 0", set={**good, **late, 0: v}))
        out.append(dict(cls="careful wire 0", set={**good, **late, 0: 1}))
    rn = g["run"]                                          # the bit run: bits recomposed, a no-bit among them
    bits = {b: (0xA5 >> i) & 1 for i, b in enumerate(rn["bits"])}
    out += [dict(cls="bit run", set={**bits, rn["z"]: 0xA5 << 3}), dict(cls="bit run", set={**bits, rn["z"]: (0xA5 << 3) + (1 << 64)}),
            dict(cls="bit run", set={**bits, rn["bits"][2]: 3, rn["z"]: (0xA5 << 3) + (2 << 5)})]
    return out


def edge_expect(E, bodies):
    """-> [(count, first violated row or NONE)] per body: every row evaluated in plain integers (an element >= p spoils the rows that read it)"""
    p, cons = E["prime"], E["constraints"]
    by_wire = R.rows_of_wire(E)
    h = p >> 1
    scons = [tuple({w: (f if f <= h else f - p) for w, f in lc.items()} for lc in row) for row in cons]
    out = []
    for body in bodies:
        s = body["set"]
        val = lambda x: s.get(x, 1 if x == 0 else 0)
        # (with wire 0 = 1 and everything else zero every row holds: only rows that read a wire of `set` need a look — all rows if wire 0 is set)
        todo = range(len(cons)) if 0 in s else sorted({k for w in s for k in by_wire.get(w, ())})
        bad = []
        for k in todo:
            a, b, c = scons[k]
            wild = any(val(x) >= p for lc in (a, b, c) for x in lc)
            if wild or (sum(f * val(x) for x, f in a.items()) * sum(f * val(x) for x, f in b.items()) - sum(f * val(x) for x, f in c.items())) % p:
                bad.append(k)
        out.append((len(bad), bad[0] if bad else NONE))
    return out


def edge_image(E):
    return R.write_image(E["prime"], E["n_wires"], E["constraints"], 0, 0, 0)


def edge_triples(bodies):
    """the bodies as (body, wire, value) triples for a child process: wire 0 of every body first (1 unless set)"""
    t = []
    for i, b in enumerate(bodies):
        t.append((i, 0, b["set"].get(0, 1)))
        t += [(i, w, v) for w, v in sorted(b["set"].items()) if w != 0]
    return t


# ------------------------------------------------------------------------------------------------ running the cases (device; torch)
def _le32(values):
    """ints -> int64 [n, 4] little-endian 32-byte elements"""
    import numpy as np
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), dtype=np.int64).reshape(-1, 4)


def run_plan(r1cs, body, wires, values, slab=4096):
    """One valid body (uint8 [body_bytes]) replicated on the device in slabs of at most `slab` bodies; case j = that body with element
    wires[j] set to values[j], written with one indexed store per slab.  Every 64th body of a slab stays untouched.
    -> (count, first) per case as uint32 arrays, and the number of untouched bodies that did not report (0, NONE)."""
    import numpy as np
    import torch
    dev = torch.device("cuda:0")
    nw = body.size // 32
    d_body = torch.from_numpy(np.array(body, dtype=np.uint8)).to(dev)
    vals = torch.from_numpy(_le32(values).copy()).to(dev)
    wires_t = torch.tensor(list(wires), dtype=torch.int64, device=dev)
    n = len(wires)
    per = slab - (slab + 63) // 64                             # cases per full slab
    buf = torch.empty((min(slab, n + n // 63 + 1), body.size), dtype=torch.uint8, device=dev)
    count, first = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    clean_wrong = 0
    for j0 in range(0, n, per):
        k = min(per, n - j0)
        pos = torch.arange(k, device=dev)
        pos = pos + pos // 63 + 1                              # bodies 0, 64, 128, ... stay as they are
        nb = int(pos[-1].item()) + 1
        assert nb <= buf.shape[0]
        buf[:nb] = d_body
        buf[:nb].view(torch.int64).view(nb, nw, 4)[pos, wires_t[j0:j0 + k]] = vals[j0:j0 + k]
        viol = torch.full((nb,), 77, dtype=torch.int32, device=dev)
        fst = torch.zeros((nb,), dtype=torch.int32, device=dev)
        r1cs.check_device(buf.data_ptr(), nb, buf.stride(0), viol.data_ptr(), fst.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        v, f = viol.cpu().numpy().view(np.uint32), fst.cpu().numpy().view(np.uint32)
        p = pos.cpu().numpy()
        count[j0:j0 + k], first[j0:j0 + k] = v[p], f[p]
        clean = np.arange(0, nb, 64)
        clean_wrong += int(np.count_nonzero((v[clean] != 0) | (f[clean] != NONE)))
    return count, first, clean_wrong


def run_edge(r1cs, nw, triples, n):
    """n bodies of zeros with the (body, wire, value) triples stored -> (count, first) as uint32 arrays"""
    import numpy as np
    import torch
    dev = torch.device("cuda:0")
    buf = torch.zeros((n, nw, 4), dtype=torch.int64, device=dev)
    bi = torch.tensor([t[0] for t in triples], dtype=torch.int64, device=dev)
    wi = torch.tensor([t[1] for t in triples], dtype=torch.int64, device=dev)
    buf[bi, wi] = torch.from_numpy(_le32([t[2] for t in triples]).copy()).to(dev)
    viol = torch.full((n,), 77, dtype=torch.int32, device=dev)
    fst = torch.zeros((n,), dtype=torch.int32, device=dev)
    r1cs.check_device(buf.data_ptr(), n, nw * 32, viol.data_ptr(), fst.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return viol.cpu().numpy().view(np.uint32), fst.cpu().numpy().view(np.uint32)


def _child(argv):
    """child process of tests/test_gpu_r1cs_rows.py (the kernels read their road from the environment once per process):
      plan <circuit> <file.npz: body, wires, values as bytes>   -> JSON {count, first, clean_wrong}
      edge <circuit> <image> <prime as text>                     -> JSON {tiled, count, first}: edge_system / edge_bodies rebuilt here"""
    import importlib
    import json
    import os
    import sys
    import numpy as np
    sys.path.insert(0, os.getcwd())
    m = importlib.import_module("hot-proofs-blake3-circom_amd")
    ctx = m.Context(argv[1], 0)
    if argv[0] == "plan":
        d = np.load(argv[2])
        raw = d["values"].tobytes()
        values = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
        r = m.R1cs(ctx)
        count, first, clean_wrong = run_plan(r, d["body"], d["wires"].tolist(), values)
        print(json.dumps(dict(count=count.tolist(), first=first.tolist(), clean_wrong=clean_wrong)))
    else:
        E = edge_system(int(argv[3]), ctx.witness_size)
        bodies = edge_bodies(E)
        r = m.R1cs(ctx, open(argv[2], "rb").read())
        count, first = run_edge(r, ctx.witness_size, edge_triples(bodies), len(bodies))
        print(json.dumps(dict(tiled=bool(r.tiled), count=count.tolist(), first=first.tolist())))


if __name__ == "__main__":
    import sys
    _child(sys.argv[1:])
