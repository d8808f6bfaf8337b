"""The yardstick of the evaluation and opening tests: hsw_gadget_evaluate and hsw_gadget_open over Python integers.
evaluate_model is Horner's rule; open_model folds a group's columns as halo2 folds (acc * v + a) and runs the backward
recurrence q[j-1] = c[j] + z q[j] of kate_division.  tests/test_open_host.py proves both against the term-by-term
definitions of include/hsw.h, which are here too; the GPU tests import the model from here (a module of its own, like
tests/ntt_model.py, so that they need nothing of the host tests' sanitizer helpers).  A column is a list of its
input_rows values; rows beyond it count as 0."""
from tests.constraint_check import P_INT


def evaluate_model(a, z):
    """sum_j a[j] z^j"""
    s = 0
    for x in reversed(a):
        s = (s * z + x) % P_INT
    return s


def fold_model(columns, v, rows):
    """c[j] over rows j < rows: acc * v + a, column after column, the first column the highest power of v"""
    c = [0] * rows
    for i, a in enumerate(columns):
        assert len(a) <= rows
        for j in range(rows):
            x = a[j] if j < len(a) else 0
            c[j] = (c[j] * v + x) % P_INT if i else x % P_INT
    return c


def open_model(columns, z, v, rows):
    """(q, eval): q[rows-1] = 0, q[j-1] = c[j] + z q[j]; eval = c[0] + z q[0]"""
    c = fold_model(columns, v, rows)
    q = [0] * rows
    for j in range(rows - 1, 0, -1):
        q[j - 1] = (c[j] + z * q[j]) % P_INT
    return q, (c[0] + z * q[0]) % P_INT


def evaluate_definition(a, z, rows):
    """the contract of include/hsw.h, term by term"""
    return sum((a[j] if j < len(a) else 0) * pow(z, j, P_INT) for j in range(rows)) % P_INT


def open_definition(columns, z, v, rows):
    """the contract of include/hsw.h, term by term: O(rows^2)"""
    m = len(columns)
    c = [sum(pow(v, m - 1 - i, P_INT) * (a[j] if j < len(a) else 0) for i, a in enumerate(columns)) % P_INT for j in range(rows)]
    q = [sum(c[i] * pow(z, i - j - 1, P_INT) for i in range(j + 1, rows)) % P_INT for j in range(rows)]
    return q, sum(c[j] * pow(z, j, P_INT) for j in range(rows)) % P_INT, c
