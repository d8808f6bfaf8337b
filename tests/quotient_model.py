"""The yardstick of the quotient tests: hsw_gadget_quotient over Python integers, row by row, exactly the definition of
include/hsw.h (the order of the expressions is assumption A9).  tests/test_quotient_host.py proves on a satisfied toy
circuit that what it computes IS halo2's h(X); the GPU tests compare the device's bytes with it on random columns.  A
module of its own, like tests/ntt_model.py, whose transforms the toy circuit uses."""
import random

from tests.constraint_check import P_INT
from tests.ntt_model import ntt_model, root_of_unity

DELTA = 7          # a generator of the cosets of the permutation's labels, as the permutation product's tests take it


def inv(x):
    return pow(x, P_INT - 2, P_INT)


def t_inv_model(log_rows, e, w, zeta):
    """[(zeta^n (w^n)^r - 1)^-1 for r < 2^e]"""
    n = 1 << log_rows
    zn, wn = pow(zeta, n, P_INT), pow(w, n, P_INT)
    return [inv((zn * pow(wn, r, P_INT) - 1) % P_INT) for r in range(1 << e)]


def numerator_model(log_rows, log_n, u, columns, fixed, gates, y, w, zeta, l0=None, l_last=None, l_active=None, perm_columns=(), L=1,
                    sigmas=(), perm_z=(), delta=DELTA, beta=0, gamma=0, lookups=(), perm_inputs=(), perm_tables=(), lookup_z=(), theta=0, at_x=None):
    """V of ONE proof: every expression folded as V = V y + expr.  columns + fixed share one index space; every column
    is a list of N values in extended form; gates: [[(coeff, [(column, rotation), ...]), ...], ...]; lookups: [(input
    column indices, table column indices), ...].  Returns (V, the number of expressions).
    at_x: the same expressions at ONE point X = at_x instead of on the coset -- every column is then a dict
    {rotation: the polynomial's value at at_x omega^rotation} (u is the last rotation), and V has one entry."""
    N, ext = 1 << log_n, 1 << (log_n - log_rows)
    space = list(columns) + list(fixed)
    rows = range(N) if at_x is None else range(1)
    V, count = [0] * len(rows), 0

    def rd(col, i, r=0):
        """the cell that rotation r of a base-domain query reads at extended row i"""
        return col[(i + r * ext) % N] if at_x is None else col[r]

    def fold(expr):
        nonlocal count
        count += 1
        for i in rows:
            V[i] = (V[i] * y + expr(i)) % P_INT

    def gate_row(gate, i):
        s = 0
        for coeff, factors in gate:
            t = coeff
            for col, rot in factors:
                t = t * rd(space[col], i, rot) % P_INT
            s += t
        return s

    for gate in gates:
        fold(lambda i, gate=gate: gate_row(gate, i))
    m = len(perm_columns)
    if m:
        S = -(-m // L)
        Z = perm_z
        assert len(Z) == S
        x = [zeta * pow(w, i, P_INT) % P_INT for i in rows] if at_x is None else [at_x]
        fold(lambda i: rd(l0, i) * (1 - rd(Z[0], i)))
        fold(lambda i: rd(l_last, i) * (rd(Z[S - 1], i) * rd(Z[S - 1], i) - rd(Z[S - 1], i)))
        for s in range(1, S):
            fold(lambda i, s=s: rd(l0, i) * (rd(Z[s], i) - rd(Z[s - 1], i, u)))
        for s in range(S):
            def product(i, s=s):
                left, right = rd(Z[s], i, 1), rd(Z[s], i)
                for j in range(s * L, min(m, (s + 1) * L)):
                    v = rd(space[perm_columns[j]], i)
                    left = left * (v + beta * rd(sigmas[j], i) + gamma) % P_INT
                    right = right * (v + beta * pow(delta, j, P_INT) * x[i] + gamma) % P_INT
                return rd(l_active, i) * (left - right)
            fold(product)
    for l, (ins, tabs) in enumerate(lookups):
        def folded(cols, i):
            a = 0
            for j in cols:
                a = (a * theta + rd(space[j], i)) % P_INT
            return a
        A, Sv = [folded(ins, i) for i in rows], [folded(tabs, i) for i in rows]
        Ap, Sp, Z = perm_inputs[l], perm_tables[l], lookup_z[l]
        fold(lambda i, Z=Z: rd(l0, i) * (1 - rd(Z, i)))
        fold(lambda i, Z=Z: rd(l_last, i) * (rd(Z, i) * rd(Z, i) - rd(Z, i)))
        fold(lambda i, Z=Z, Ap=Ap, Sp=Sp, A=A, Sv=Sv: rd(l_active, i) * (rd(Z, i, 1) * (rd(Ap, i) + beta) * (rd(Sp, i) + gamma)
                                                                         - rd(Z, i) * (A[i] + beta) * (Sv[i] + gamma)))
        fold(lambda i, Ap=Ap, Sp=Sp: rd(l0, i) * (rd(Ap, i) - rd(Sp, i)))
        fold(lambda i, Ap=Ap, Sp=Sp: rd(l_active, i) * (rd(Ap, i) - rd(Sp, i)) * (rd(Ap, i) - rd(Ap, i, -1)))
    return V, count


def quotient_model(log_rows, log_n, u, columns, fixed, gates, y, w, zeta, **kw):
    """h of ONE proof on the extended coset: the numerator times t_inv[i mod 2^e]"""
    V, count = numerator_model(log_rows, log_n, u, columns, fixed, gates, y, w, zeta, **kw)
    ti = t_inv_model(log_rows, log_n - log_rows, w, zeta)
    ext = 1 << (log_n - log_rows)
    return [v * ti[i % ext] % P_INT for i, v in enumerate(V)], count


# ---- the toy circuit of the host and the GPU tests: satisfied, so that its h has the degree halo2 expects -------------
FLEX_GATE = lambda q, a: [(1, [(q, 0), (a, 0)]), (1, [(q, 0), (a, 1), (a, 2)]), (P_INT - 1, [(q, 0), (a, 3)])]   # q (a + b c - d) over four rows of one column


def to_extended(col, log_rows, log_n, zeta):
    """a base column (n values, Lagrange form) on the extended coset zeta w^i"""
    n = 1 << log_rows
    coeff = ntt_model(col, log_rows, inv(root_of_unity(log_rows)), scale=inv(n))
    return ntt_model(coeff, log_n, root_of_unity(log_n), shift=zeta)


def from_extended(col, log_n, zeta):
    """the coefficients of a column given on the extended coset"""
    return ntt_model(col, log_n, inv(root_of_unity(log_n)), shift=inv(zeta), scale=inv(1 << log_n), shift_after=True)


def toy_circuit(seed=1, log_rows=4, u=10, flip=False):
    """A satisfied circuit in base form: two advice columns with the FlexGate gate under a selector each, a third advice
    column, one lookup of 1 + 1 columns and one of 2 + 2, a permutation over the three advice columns with L = 2 (S = 2)
    and a few real copy constraints, Z from the recurrences, random cells in the blinding rows.  Returns a dict of base
    columns and challenges; flip: one witness cell of a gate is changed afterwards."""
    rng = random.Random(seed)
    n = 1 << log_rows
    omega = root_of_unity(log_rows)
    rnd = lambda: rng.randrange(P_INT)
    theta, beta, gamma, y = rnd(), rnd(), rnd(), rnd()
    # advice 0, 1: groups of four rows a, b, c, d = a + b c under selectors 2 + 0, 2 + 1 (fixed columns 3, 4 of the space)
    adv = [[0] * n for _ in range(3)]
    sel = [[0] * n for _ in range(2)]
    for k in range(2):
        for r in range(0, u - 3, 4):
            a, b, c = rnd(), rnd(), rnd()
            adv[k][r:r + 4] = [a, b, c, (a + b * c) % P_INT]
            sel[k][r] = 1
    # tables (fixed 5, 6, 7): t1 a range, (t2a, t2b) pairs; padded on every row with row 0's entry
    t1 = [(i % 6) for i in range(n)]
    t2a = [(i % 5) + 100 for i in range(n)]
    t2b = [((i % 5) * (i % 5) + 7) for i in range(n)]
    # advice 2 is looked up in t1; the second lookup's inputs (lk_a, lk_b) are shared columns of their own (8, 9 of the
    # space) that hold pairs of the table
    adv[2] = [rng.randrange(6) for _ in range(n)]
    lk_a, lk_b = [0] * n, [0] * n
    for i in range(n):
        j = rng.randrange(5)
        lk_a[i], lk_b[i] = t2a[j], t2b[j]
    # copy constraints: cells (column, row) joined in cycles
    adv[1][0] = adv[0][3]; adv[1][3] = (adv[1][0] + adv[1][1] * adv[1][2]) % P_INT      # d of group 0 of column 0 is a of group 0 of column 1
    adv[2][1] = adv[2][5] = adv[2][7]                                                    # three cells of column 2
    adv[0][4] = adv[0][0]; adv[0][7] = (adv[0][4] + adv[0][5] * adv[0][6]) % P_INT
    cycles = [[(0, 3), (1, 0)], [(2, 1), (2, 5), (2, 7)], [(0, 0), (0, 4)]]
    if flip:
        adv[0][3] = (adv[0][3] + 1) % P_INT
    label = lambda j, i: pow(DELTA, j, P_INT) * pow(omega, i, P_INT) % P_INT
    sigma = [[label(j, i) for i in range(n)] for j in range(3)]
    for cyc in cycles:
        for (j, i), (j2, i2) in zip(cyc, cyc[1:] + cyc[:1]):
            sigma[j][i] = label(j2, i2)
    # blinding rows: random cells in every advice column
    for col in adv:
        for i in range(u, n):
            col[i] = rnd()
    # the permutation's Z over sets of L = 2 columns
    L, S = 2, 2
    pz = [[0] * n for _ in range(S)]
    last = 1
    for s in range(S):
        pz[s][0] = last
        for i in range(u):
            num = den = 1
            for j in range(s * L, min(3, (s + 1) * L)):
                num = num * (adv[j][i] + beta * label(j, i) + gamma) % P_INT
                den = den * (adv[j][i] + beta * sigma[j][i] + gamma) % P_INT
            pz[s][i + 1] = pz[s][i] * num % P_INT * inv(den) % P_INT
        last = pz[s][u]
        for i in range(u + 1, n):
            pz[s][i] = rnd()
    if not flip:
        assert pz[S - 1][u] == 1
    # the lookups: compressed A and S, the permuted pair, Z
    def lookup(ins, tabs):
        A = [0] * n
        T = [0] * n
        for c in ins:
            A = [(a * theta + c[i]) % P_INT for i, a in enumerate(A)]
        for c in tabs:
            T = [(a * theta + c[i]) % P_INT for i, a in enumerate(T)]
        Ap = sorted(A[:u])
        Sp = [None] * u
        pool = sorted(T[:u])
        for i in range(u):                                   # a new value of A' takes its table entry, the rest fill up
            if i == 0 or Ap[i] != Ap[i - 1]:
                Sp[i] = Ap[i]
                pool.remove(Ap[i])
        for i in range(u):
            if Sp[i] is None:
                Sp[i] = pool.pop()
        Z = [0] * n
        Z[0] = 1
        for i in range(u):
            Z[i + 1] = Z[i] * (A[i] + beta) % P_INT * (T[i] + gamma) % P_INT * inv((Ap[i] + beta) * (Sp[i] + gamma) % P_INT) % P_INT
        assert Z[u] == 1
        return (Ap + [rnd() for _ in range(n - u)], Sp + [rnd() for _ in range(n - u)], Z[:u + 1] + [rnd() for _ in range(n - u - 1)])
    lk1, lk2 = lookup([adv[2]], [t1]), lookup([lk_a, lk_b], [t2a, t2b])
    l0 = [1] + [0] * (n - 1)
    l_last = [1 if i == u else 0 for i in range(n)]
    l_active = [1 if i < u else 0 for i in range(n)]
    return dict(log_rows=log_rows, u=u, advice=adv, fixed=sel + [t1, t2a, t2b, lk_a, lk_b], sigma=sigma, perm_z=pz, lookups=[lk1, lk2],
                l0=l0, l_last=l_last, l_active=l_active, theta=theta, beta=beta, gamma=gamma, y=y, L=L,
                gates=[FLEX_GATE(3, 0), FLEX_GATE(4, 1)], perm_columns=[0, 1, 2], lookup_columns=[([2], [5]), ([8, 9], [6, 7])])


def toy_extended(t, e, zeta):
    """the toy circuit's columns on the extended coset, as numerator_model's keyword arguments take them"""
    lr, ln = t["log_rows"], t["log_rows"] + e
    ex = lambda col: to_extended(col, lr, ln, zeta)
    return dict(columns=[ex(c) for c in t["advice"]], fixed=[ex(c) for c in t["fixed"]],
                kw=dict(l0=ex(t["l0"]), l_last=ex(t["l_last"]), l_active=ex(t["l_active"]), perm_columns=t["perm_columns"], L=t["L"],
                        sigmas=[ex(c) for c in t["sigma"]], perm_z=[ex(c) for c in t["perm_z"]], beta=t["beta"], gamma=t["gamma"],
                        lookups=t["lookup_columns"], perm_inputs=[ex(l[0]) for l in t["lookups"]], perm_tables=[ex(l[1]) for l in t["lookups"]],
                        lookup_z=[ex(l[2]) for l in t["lookups"]], theta=t["theta"]))


def evaluate(coeff, x):
    """sum_j coeff[j] x^j"""
    r = 0
    for c in reversed(coeff):
        r = (r * x + c) % P_INT
    return r


TOY_ROTATIONS = (0, 1, 2, 3, -1)            # and u, the last rotation


def toy_at_point(t, x, evaluator=None):
    """the toy circuit's polynomials at x omega^r for every rotation a query uses, as numerator_model(at_x=x) takes
    them; evaluator(base column, point) defaults to interpolation and Horner's rule here"""
    lr, n = t["log_rows"], 1 << t["log_rows"]
    omega = root_of_unity(lr)
    if evaluator is None:
        evaluator = lambda col, z: evaluate(ntt_model(col, lr, inv(omega), scale=inv(n)), z)
    rots = TOY_ROTATIONS + (t["u"],)
    ex = lambda col: {r: evaluator(col, x * pow(omega, r % n, P_INT) % P_INT) for r in rots}
    return dict(columns=[ex(c) for c in t["advice"]], fixed=[ex(c) for c in t["fixed"]],
                kw=dict(l0=ex(t["l0"]), l_last=ex(t["l_last"]), l_active=ex(t["l_active"]), perm_columns=t["perm_columns"], L=t["L"],
                        sigmas=[ex(c) for c in t["sigma"]], perm_z=[ex(c) for c in t["perm_z"]], beta=t["beta"], gamma=t["gamma"],
                        lookups=t["lookup_columns"], perm_inputs=[ex(l[0]) for l in t["lookups"]], perm_tables=[ex(l[1]) for l in t["lookups"]],
                        lookup_z=[ex(l[2]) for l in t["lookups"]], theta=t["theta"]))
