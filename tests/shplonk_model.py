"""The yardstick of the SHPLONK tests: hsw_gadget_shplonk_quotient and hsw_gadget_shplonk_open over Python integers.
The quotient of a rotation set is the DEFINITION -- successive Kate division of the y-fold by (X - z), root after root --
not the partial-fraction sum the device runs; tests/test_shplonk_host.py proves the two equal, and both against the
identities c - R = Z Q and (X - u) w = (L - L(u)) / zd_0.  The GPU tests import the model from here (a module of its own,
like tests/open_model.py).  A column is a list of its input_rows values; rows beyond it count as 0.  sets: a sequence
of (column indices, point indices); points: the super point set T."""
from tests.constraint_check import P_INT
from tests.open_model import evaluate_model


def fold_y(columns, y, rows):
    """c[j] = sum_k y^k a_k[j]: the FIRST listed column gets y^0"""
    c, w = [0] * rows, 1
    for a in columns:
        assert len(a) <= rows
        for j, x in enumerate(a):
            c[j] = (c[j] + w * x) % P_INT
        w = w * y % P_INT
    return c


def kate(c, z):
    """q[rows-1] = 0, q[j-1] = c[j] + z q[j]: floor(c(X) / (X - z)) in as many cells as c has"""
    q = [0] * len(c)
    for j in range(len(c) - 1, 0, -1):
        q[j - 1] = (c[j] + z * q[j]) % P_INT
    return q


def set_quotient(c, zs):
    """floor(c(X) / prod (X - z)): one Kate division per root, each on the quotient of the one before"""
    for z in zs:
        c = kate(c, z)
    return c


def set_folds(columns, sets, y, rows):
    return [fold_y([columns[b] for b in cols], y, rows) for cols, _ in sets]


def shplonk_quotient_model(columns, sets, points, y, v, rows):
    """h[j] = sum_i v^i Q_i[j]: the first set gets v^0"""
    h, w = [0] * rows, 1
    for c, (_, pts) in zip(set_folds(columns, sets, y, rows), sets):
        q = set_quotient(c, [points[t] for t in pts])
        h = [(a + w * b) % P_INT for a, b in zip(h, q)]
        w = w * v % P_INT
    return h


def vanish(u, zs):
    d = 1
    for z in zs:
        d = d * (u - z) % P_INT
    return d


def zd_of(sets, points, u):
    """zd_i = prod over the points of T NOT in set i of (u - z)"""
    return [vanish(u, [z for t, z in enumerate(points) if t not in pts]) for _, pts in sets]


def linearisation(columns, sets, points, y, v, u, h, rows):
    """L[j] = sum_i v^i zd_i c_i[j] - zt h[j]"""
    zd, zt = zd_of(sets, points, u), vanish(u, points)
    L = [(-zt * x) % P_INT for x in h]
    w = 1
    for c, d in zip(set_folds(columns, sets, y, rows), zd):
        L = [(a + w * d * b) % P_INT for a, b in zip(L, c)]
        w = w * v % P_INT
    return L


def shplonk_open_model(columns, sets, points, y, v, u, h, rows):
    """w[j] = zd_0^-1 sum_{l>j} L[l] u^(l-j-1)"""
    inv = pow(zd_of(sets, points, u)[0], -1, P_INT)
    return [x * inv % P_INT for x in kate(linearisation(columns, sets, points, y, v, u, h, rows), u)]


def partial_fraction_quotient(c, zs):
    """what the device runs: sum_k lambda_k kate(c, z_k), lambda_k = 1 / prod_{l != k} (z_k - z_l)"""
    q = [0] * len(c)
    for k, z in enumerate(zs):
        lam = pow(vanish(z, zs[:k] + zs[k + 1:]), -1, P_INT)
        q = [(a + lam * b) % P_INT for a, b in zip(q, kate(c, z))]
    return q


def interpolate_eval(zs, values, x):
    """R(x) for the R of degree < len(zs) with R(zs[k]) = values[k] (Lagrange)"""
    r = 0
    for k, z in enumerate(zs):
        others = zs[:k] + zs[k + 1:]
        r = (r + values[k] * vanish(x, others) * pow(vanish(z, others), -1, P_INT)) % P_INT
    return r


__all__ = ["evaluate_model", "fold_y", "kate", "set_quotient", "set_folds", "shplonk_quotient_model", "vanish", "zd_of", "linearisation",
           "shplonk_open_model", "partial_fraction_quotient", "interpolate_eval"]
