"""The yardstick of the G1 MSM tests: hsw_gadget_msm over Python integers.  BN254 G1 (y^2 = x^3 + 3 over Fq, G = (1, 2),
prime order r) in affine chord-and-tangent arithmetic, None for the identity.  Bases are CHAINS with known discrete logs,
G[j] = (k0 + j t) G, one affine addition per row, so that a column's expected commitment is the single multiplication
(sum_j a[j] k_j mod r) G; tests/test_msm_host.py proves that shortcut against the term-by-term definition.  The GPU tests
import it from here (a module of its own, like tests/ntt_model.py)."""
from tests.constraint_check import P_INT

Q_INT = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
R_INT = P_INT                      # the order of G1 is the Fr modulus
G = (1, 2)
MONT = 1 << 256

assert (G[1] * G[1] - G[0] ** 3 - 3) % Q_INT == 0


def neg(p):
    return None if p is None else (p[0], (Q_INT - p[1]) % Q_INT)


def add(p, q):
    """chord and tangent; None is the identity"""
    if p is None:
        return q
    if q is None:
        return p
    (x1, y1), (x2, y2) = p, q
    if x1 == x2:
        if (y1 + y2) % Q_INT == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, Q_INT) % Q_INT
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, Q_INT) % Q_INT
    x3 = (lam * lam - x1 - x2) % Q_INT
    return x3, (lam * (x1 - x3) - y1) % Q_INT


def mul(k, p):
    """double-and-add, k reduced mod r"""
    k %= R_INT
    acc = None
    while k:
        if k & 1:
            acc = add(acc, p)
        p = add(p, p)
        k >>= 1
    return acc


def chain(k0, t, n):
    """([(k0 + j t) G for j < n], [k0 + j t mod r]): one affine addition per row"""
    step, p, pts = mul(t, G), mul(k0, G), []
    for _ in range(n):
        pts.append(p)
        p = add(p, step)
    return pts, [(k0 + j * t) % R_INT for j in range(n)]


def commitment(scalars, logs):
    """sum_j a[j] G[j] for bases of known logs (None: the identity base): ONE multiplication of G"""
    return mul(sum(a * k for a, k in zip(scalars, logs) if k is not None) % R_INT, G)


def msm_definition(scalars, points):
    """the contract of include/hsw.h, term by term: double-and-add of every a[j] * G[j]"""
    acc = None
    for a, p in zip(scalars, points):
        acc = add(acc, mul(a, p))
    return acc


def point_words(p):
    """the 8 uint64 words of a stored point: x then y in Montgomery form mod q, all zero for the identity"""
    if p is None:
        return [0] * 8
    out = []
    for v in p:
        m = v * MONT % Q_INT
        out += [(m >> (64 * i)) & (2**64 - 1) for i in range(4)]
    return out


def words_point(w):
    """the affine point of 8 stored words (None for eight zeros)"""
    if not any(int(x) for x in w):
        return None
    inv = pow(MONT, -1, Q_INT)
    x = sum(int(w[i]) << (64 * i) for i in range(4)) * inv % Q_INT
    y = sum(int(w[4 + i]) << (64 * i) for i in range(4)) * inv % Q_INT
    return x, y


def cell_words(a, montgomery):
    """the 4 uint64 words of a stored Fr cell"""
    v = a * MONT % P_INT if montgomery else a
    return [(v >> (64 * i)) & (2**64 - 1) for i in range(4)]


def plan(max_rows, window_bits=0, slice_rows=0):
    """csrc/hsw_msm_value.hpp's msm_plan: (window_bits, windows, slice_rows, slices)"""
    c = window_bits or 8
    s = slice_rows
    if not s:
        s = 4096
        while -(-max_rows // s) > 1024:
            s *= 2
    return c, -(-254 // c), s, max(1, -(-max_rows // s))
