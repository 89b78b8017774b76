"""Integer model of the witness solver (bellman_amd/csrc/solve_plan.hpp, r1cs_solve.hip): the plan rule and the evaluation
restated on Python integers, and a generator of random satisfiable circuits made of the gates a synthesised circuit is made of.

A circuit here is three lists of rows, rows[m][i] = [(variable, coefficient)], variables numbered as bh_csr.var numbers them
(0 is ONE, inputs first, aux behind them), coefficients integers mod Q.  A hint is (kind, [(variable, coefficient)], [output
variables], shift).

The rule: ONE, the supplied variables and the outputs of hints are known from the start.  One sweep over the constraints in
order: constraint i defines v when v is its only variable not yet known (terms with a zero coefficient do not exist), v has
no term in A_i or B_i, and the sum s_v of v's coefficients in C_i is not zero; v = (A_i.w * B_i.w - rest of C_i) / s_v.
Levels: 0 for ONE and supplied variables; a definition stands one above the highest variable it reads."""
import random

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
BITS, INV_OR_ZERO = 1, 2
OK, INVALID = 0, -2
NO_VARIABLE = 0xFFFFFFFF


class Plan:
    def __init__(self, status, first_unsolved=NO_VARIABLE):
        self.status, self.first_unsolved = status, first_unsolved
        self.definer, self.level, self.counts = [], [], None   # definer: -1 known, i >= 0 constraint, -2 - h hint


def plan(n_vars, rows, supplied, hints):
    n_cons = len(rows[0])
    sup = {0}
    for v in supplied:
        if v >= n_vars:
            return Plan(INVALID, v)
        sup.add(v)
    known = [v in sup for v in range(n_vars)]
    definer = [-1] * n_vars
    for h, (kind, lc, outs, shift) in enumerate(hints):
        if not outs or (kind == BITS and shift + len(outs) > 256) or (kind == INV_OR_ZERO and (len(outs) != 1 or shift)) or kind not in (BITS, INV_OR_ZERO):
            return Plan(INVALID)
        if any(v >= n_vars for v, _ in lc) or any(v >= n_vars for v in outs):
            return Plan(INVALID)
        for v in outs:
            if v in sup or definer[v] != -1:
                return Plan(INVALID, v)
            definer[v] = -2 - h
            known[v] = True
    reads = {}   # definition -> the variables it reads; definitions are ("c", i) and ("h", h)
    for i in range(n_cons):
        unknown = {v for m in range(3) for v, c in rows[m][i] if c % Q and not known[v]}
        if len(unknown) != 1:
            continue
        (v,) = unknown
        if any(x == v and c % Q for m in (0, 1) for x, c in rows[m][i]):
            continue
        if sum(c for x, c in rows[2][i] if x == v) % Q == 0:
            continue
        known[v] = True
        definer[v] = i
        reads[("c", i)] = {x for m in range(3) for x, c in rows[m][i] if c % Q and x != v}
    for v in range(n_vars):
        if not known[v]:
            return Plan(INVALID, v)
    for h, (kind, lc, outs, shift) in enumerate(hints):
        reads[("h", h)] = {x for x, c in lc if c % Q}
    def_of = [None if d == -1 else ("c", d) if d >= 0 else ("h", -2 - d) for d in definer]
    # levels by repeated release (Kahn): a definition is released when everything it reads has a level
    waits = {d: sum(1 for x in r if def_of[x] is not None) for d, r in reads.items()}
    users = {d: [] for d in reads}
    for d, r in reads.items():
        for x in r:
            if def_of[x] is not None:
                users[def_of[x]].append(d)
    level_of = {}
    var_level = [0] * n_vars
    ready = [d for d, w in waits.items() if w == 0]
    while ready:
        d = ready.pop()
        level_of[d] = 1 + max([var_level[x] for x in reads[d]] or [0])
        if d[0] == "c":
            outs = [next(v for v, c in rows[2][d[1]] if definer[v] == d[1] and c % Q)]
        else:
            outs = hints[d[1]][2]
        for v in outs:
            var_level[v] = level_of[d]
        for u in users[d]:
            waits[u] -= 1
            if waits[u] == 0:
                ready.append(u)
    if len(level_of) != len(reads):   # a cycle: the lowest variable whose definition was never released
        return Plan(INVALID, min(v for v in range(n_vars) if def_of[v] is not None and def_of[v] not in level_of))
    p = Plan(OK)
    p.definer, p.level = definer, var_level
    widths = {}
    for d, lv in level_of.items():
        widths[lv] = widths.get(lv, 0) + 1
    p.counts = [len(sup) - 1, sum(1 for d in definer if d >= 0), sum(1 for d in definer if d <= -2), max(level_of.values(), default=0),
                max(widths.values(), default=0)]
    p.order = sorted(level_of, key=lambda d: level_of[d])
    return p


def _dot(row, w, skip=None):
    return sum(c * w[v] for v, c in row if v != skip and c % Q) % Q


def complete(rows, hints, p, w):
    """w: every variable's slot, the supplied ones (and ONE) holding their values -> the completed list"""
    w = list(w)
    for kind, i in p.order:
        if kind == "c":
            v = next(x for x, c in rows[2][i] if p.definer[x] == i and c % Q)
            s = sum(c for x, c in rows[2][i] if x == v) % Q
            w[v] = (_dot(rows[0][i], w) * _dot(rows[1][i], w) - _dot(rows[2][i], w, skip=v)) * pow(s, -1, Q) % Q
        else:
            hk, lc, outs, shift = hints[i]
            x = _dot(lc, w)
            if hk == BITS:
                for j, v in enumerate(outs):
                    w[v] = (x >> (shift + j)) & 1
            else:
                w[outs[0]] = pow(x, -1, Q) if x else 0
    return w


def first_bad(rows, w):
    for i in range(len(rows[0])):
        if _dot(rows[0][i], w) * _dot(rows[1][i], w) % Q != _dot(rows[2][i], w):
            return i
    return None


def csr(rows):
    """-> ((row_ptr, var, coeff index) x 3 as lists, coefficient table of integers, [0] == 1); zero coefficients keep a table
    entry of their own: the library has to treat their terms as absent"""
    table, index = [1], {1: 0}
    out = []
    for m in range(3):
        row_ptr, var, coeff = [0], [], []
        for row in rows[m]:
            for v, c in row:
                c %= Q
                if c not in index:
                    index[c] = len(table)
                    table.append(c)
                var.append(v)
                coeff.append(index[c])
            row_ptr.append(len(var))
        out.append((row_ptr, var, coeff))
    return out, table


class Circuit:
    """rows / supplied / hints in final numbering, n_inputs, n_aux, and one satisfying witness (all variables)"""

    def __init__(self, n_inputs, n_aux, rows, supplied, hints, witness):
        self.n_inputs, self.n_aux, self.rows, self.supplied, self.hints, self.witness = n_inputs, n_aux, rows, supplied, hints, witness
        self.n_vars = n_inputs + n_aux


def random_circuit(seed, gates=40):
    """A satisfiable circuit in synthesis order (alloc, then enforce): product and linear gates with +-1, small and random
    coefficients and net coefficients s_v other than +-1, zero-coefficient and repeated terms, supplied booleans, and / xor,
    an 8-bit adder whose result bits come from a BITS hint, an is-zero gadget on INV_OR_ZERO; some defined variables are
    public inputs."""
    rnd = random.Random(seed)
    kinds, values = ["in"], [1]          # by allocation id; id 0 is ONE
    rows = ([], [], [])
    supplied, hints = [], []
    bools = []

    def alloc(value, supplied_=False, public=False):
        kinds.append("in" if public else "aux")
        values.append(value % Q)
        if supplied_:
            supplied.append(len(values) - 1)
        return len(values) - 1

    def coefficient():
        return rnd.choice([1, 1, Q - 1, rnd.randrange(2, 16), rnd.randrange(Q)])

    def lc(n_terms, zero_terms=True):
        terms = []
        for _ in range(n_terms):
            terms.append((rnd.randrange(len(values)), coefficient()))
        if zero_terms and rnd.random() < 0.4:     # a term that does not exist for the plan, anywhere in the row
            terms.insert(rnd.randrange(len(terms) + 1), (rnd.randrange(len(values)), 0))
        if terms and rnd.random() < 0.3:          # a repeated variable
            terms.append((terms[0][0], coefficient()))
        return terms

    def ev(terms):
        return sum(c * values[v] for v, c in terms) % Q

    def enforce(a, b, c):
        for m, r in enumerate((a, b, c)):
            rows[m].append(list(r))

    def define(a, b, rest, public=False):
        """alloc v, enforce a * b = rest + s * v with s split over one or two terms"""
        s = rnd.choice([1, 1, Q - 1, rnd.randrange(2, 16), rnd.randrange(1, Q)])
        v = alloc((ev(a) * ev(b) - ev(rest)) * pow(s, -1, Q), public=public)
        c = list(rest)
        if rnd.random() < 0.3:
            s1 = rnd.randrange(Q)
            c.insert(rnd.randrange(len(c) + 1), (v, s1))
            c.append((v, (s - s1) % Q))
        else:
            c.insert(rnd.randrange(len(c) + 1), (v, s))
        if rnd.random() < 0.2:
            a = a + [(v, 0)]                      # the new variable in A with a zero coefficient: still defined
        enforce(a, b, c)
        return v

    def boolean():
        b = alloc(rnd.randrange(2), supplied_=True)
        enforce([(0, 1), (b, Q - 1)], [(b, 1)], [])
        bools.append(b)
        return b

    for _ in range(3):
        alloc(rnd.randrange(Q), supplied_=True)
    for _ in range(4):
        boolean()
    for _ in range(gates):
        g = rnd.randrange(8)
        if g == 0:
            alloc(rnd.choice([0, 1, Q - 1, rnd.randrange(Q)]), supplied_=True)
        elif g == 1:
            boolean()
        elif g == 2:      # product gate
            define(lc(rnd.randrange(1, 5)), lc(rnd.randrange(1, 5)), lc(rnd.randrange(0, 4)), public=rnd.random() < 0.2)
        elif g == 3:      # linear gate
            define(lc(rnd.randrange(1, 6)), [(0, 1)], [], public=rnd.random() < 0.2)
        elif g == 4:      # and
            a, b = rnd.choice(bools), rnd.choice(bools)
            v = alloc(values[a] & values[b])
            enforce([(a, 1)], [(b, 1)], [(v, 1)])
            bools.append(v)
        elif g == 5:      # xor
            a, b = rnd.choice(bools), rnd.choice(bools)
            v = alloc(values[a] ^ values[b])
            enforce([(a, 1), (a, 1)], [(b, 1)], [(a, 1), (b, 1), (v, Q - 1)])
            bools.append(v)
        elif g == 6:      # 8-bit adder: the 9 result bits are advice
            xs = [boolean() for _ in range(8)]
            ys = [boolean() for _ in range(8)]
            total = [(x, 1 << j) for j, x in enumerate(xs)] + [(y, 1 << j) for j, y in enumerate(ys)]
            t = ev(total)
            outs = [alloc((t >> j) & 1) for j in range(9)]
            hints.append((BITS, total, outs, 0))
            for o in outs:
                enforce([(0, 1), (o, Q - 1)], [(o, 1)], [])
            enforce(total, [(0, 1)], [(o, 1 << j) for j, o in enumerate(outs)])
            bools.extend(outs)
        else:             # is-zero
            x = rnd.randrange(len(values))
            xv = values[x]
            inv = alloc(pow(xv, -1, Q) if xv else 0)
            hints.append((INV_OR_ZERO, [(x, 1)], [inv], 0))
            z = alloc(0 if xv else 1)
            enforce([(x, 1)], [(inv, 1)], [(0, 1), (z, Q - 1)])
            enforce([(x, 1)], [(z, 1)], [])
            bools.append(z)
    # final numbering: inputs first
    order = [i for i, k in enumerate(kinds) if k == "in"] + [i for i, k in enumerate(kinds) if k == "aux"]
    new = {old: n for n, old in enumerate(order)}
    n_inputs = sum(1 for k in kinds if k == "in")
    ren = lambda terms: [(new[v], c) for v, c in terms]  # noqa: E731
    out_rows = tuple([ren(r) for r in rows[m]] for m in range(3))
    out_hints = [(k, ren(l), [new[o] for o in outs], s) for k, l, outs, s in hints]
    return Circuit(n_inputs, len(kinds) - n_inputs, out_rows, [new[s] for s in supplied], out_hints, [values[o] for o in order])
