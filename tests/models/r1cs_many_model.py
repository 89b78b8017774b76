"""Integer model of the constraint evaluation and of the satisfiability check (bh_r1cs_eval_many_dev,
bh_r1cs_check_many_dev): a system is three CSR matrices over the variables (inputs first, then aux) and a coefficient
table; a witness is (inputs, aux) as Python integers mod q.  The reference's rule is TestConstraintSystem::
which_is_unsatisfied (src/gadgets/test/mod.rs:254-272): the first constraint in order with a * b != c.

Two generators: `random_system` draws arbitrary matrices (the evaluation does not care whether anything is satisfied);
`satisfiable_system` builds constraints the way a circuit does - the A and B rows are random over the variables allocated so
far, the C row is ONE fresh aux variable with coefficient 1 - so that `solve` can set that variable to a * b and the witness
satisfies every constraint."""
import random

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
LONG_ROW = 1024   # csrc/r1cs_dev.hpp: a row with more terms is summed by a workgroup


class System:
    def __init__(self, n_in, n_aux, matrices, table):
        self.n_in, self.n_aux, self.matrices, self.table = n_in, n_aux, matrices, table
        self.n_cons = len(matrices[0][0]) - 1

    def row(self, mat, i):
        row_ptr, var, coeff = self.matrices[mat]
        return [(var[t], self.table[coeff[t]]) for t in range(row_ptr[i], row_ptr[i + 1])]

    def row_len(self, mat, i):
        return self.matrices[mat][0][i + 1] - self.matrices[mat][0][i]


def coefficient_table(rnd, extra=12):
    """slot 0 is the constant 1 (bh_r1cs_create); 0 and q - 1 are always present"""
    return [1, 0, Q - 1, 2] + [rnd.randrange(Q) for _ in range(extra)]


def random_system(n_in, n_aux, n_cons, seed, long_rows=None):
    """arbitrary matrices; long_rows: {(matrix, row): length} for rows above the lane-per-row limit"""
    rnd = random.Random(seed)
    table = coefficient_table(rnd)
    nv = n_in + n_aux
    matrices = []
    for mat in range(3):
        row_ptr, var, coeff = [0], [], []
        for i in range(n_cons):
            k = rnd.choice([0, 0, 1, 1, 2, 3, 5, 40 if i % 97 == 0 else 2])
            if long_rows and (mat, i) in long_rows:
                k = long_rows[(mat, i)]
            for _ in range(k):
                var.append(rnd.randrange(nv))
                coeff.append(rnd.choice([0, 1, 1, 2] + list(range(len(table)))))
            row_ptr.append(len(var))
        matrices.append((row_ptr, var, coeff))
    return System(n_in, n_aux, matrices, table)


def satisfiable_system(n_in, n_free, n_cons, seed, lengths=None):
    """n_cons constraints over n_in inputs, n_free free aux variables and one fresh aux variable per constraint (variable
    n_in + n_free + i, the whole C row of constraint i).  lengths: {row: (len_a, len_b)} overrides the random row lengths."""
    rnd = random.Random(seed)
    table = coefficient_table(rnd)
    a, b, c = ([0], [], []), ([0], [], []), ([0], [], [])
    for i in range(n_cons):
        allocated = n_in + n_free + i
        la, lb = (lengths or {}).get(i, (rnd.choice([0, 1, 1, 2, 3, 5]), rnd.choice([0, 1, 1, 2, 4])))
        for (row_ptr, var, coeff), n in ((a, la), (b, lb)):
            for _ in range(n):
                var.append(rnd.randrange(allocated))
                coeff.append(rnd.choice([0, 1, 1, 1, 2] + list(range(len(table)))))
            row_ptr.append(len(var))
        c[1].append(allocated)
        c[2].append(0)
        c[0].append(len(c[1]))
    return System(n_in, n_free + n_cons, [a, b, c], table)


def from_shape_assembly(cs):
    """a bellman_amd.groth16.ShapeAssembly capture (input constraints of prover.rs:208-215 included)"""
    matrices, table = cs.csr()
    return System(cs.num_inputs, cs.num_aux, [tuple([int(x) for x in part] for part in m) for m in matrices], [t % Q for t in table])


def dot(system, mat, i, w):
    return sum(k * w[v] for v, k in system.row(mat, i)) % Q


def evaluate(system, inputs, aux):
    """-> (a, b, c): n_cons integers mod q each"""
    w = list(inputs) + list(aux)
    return tuple([dot(system, mat, i, w) for i in range(system.n_cons)] for mat in range(3))


def solve(system, inputs, free_aux):
    """the aux vector of a `satisfiable_system`: its free variables, then a * b of every constraint in order"""
    w = list(inputs) + list(free_aux)
    for i in range(system.n_cons):
        assert len(w) == system.matrices[2][1][i]
        w.append(dot(system, 0, i, w) * dot(system, 1, i, w) % Q)
    return w[system.n_in:]


def first_bad(system, inputs, aux):
    """which_is_unsatisfied: the first constraint with a * b != c, or None"""
    a, b, c = evaluate(system, inputs, aux)
    for i in range(system.n_cons):
        if a[i] * b[i] % Q != c[i]:
            return i
    return None


def first_bad_brute(system, inputs, aux):
    """the same, term by term and constraint by constraint, stopping at the first failure"""
    w = list(inputs) + list(aux)
    for i in range(system.n_cons):
        acc = [0, 0, 0]
        for mat in range(3):
            row_ptr, var, coeff = system.matrices[mat]
            for t in range(row_ptr[i], row_ptr[i + 1]):
                acc[mat] = (acc[mat] + system.table[coeff[t]] * w[var[t]]) % Q
        if (acc[0] * acc[1] - acc[2]) % Q:
            return i
    return None
