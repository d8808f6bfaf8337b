"""The yardstick of the Fr NTT tests: hsw_gadget_ntt over Python integers.  A recursive radix-2 transform, O(N log N),
which tests/test_ntt_host.py proves against the O(N^2) definition of include/hsw.h; the GPU tests import it from here (a
module of its own, like tests/constraint_check.py, so that they need nothing of the host tests' sanitizer helpers)."""
from tests.constraint_check import P_INT


def root_of_unity(log_n):
    """7^((p-1)/2^log_n): a primitive 2^log_n-th root of unity of Fr"""
    w = pow(7, (P_INT - 1) >> log_n, P_INT)
    assert pow(w, 1 << (log_n - 1), P_INT) == P_INT - 1
    return w


def dft(a, w):
    """[sum_j a[j] w^(i j) for i < len(a)], len(a) a power of two: recursive radix-2, O(N log N)"""
    n = len(a)
    if n == 1:
        return [a[0] % P_INT]
    w2 = w * w % P_INT
    even, odd = dft(a[0::2], w2), dft(a[1::2], w2)
    out, t = [0] * n, 1
    for i in range(n // 2):
        x = t * odd[i] % P_INT
        out[i] = (even[i] + x) % P_INT
        out[i + n // 2] = (even[i] - x) % P_INT
        t = t * w % P_INT
    return out


def ntt_model(a, log_n, w, shift=None, scale=None, shift_after=False):
    """What hsw_gadget_ntt computes on VALUES: a holds input_rows entries, the rest of the 2^log_n count as 0"""
    n = 1 << log_n
    g, c = 1 if shift is None else shift, 1 if scale is None else scale
    col = [x % P_INT for x in a] + [0] * (n - len(a))
    if not shift_after:
        t = 1
        for j in range(len(a)):
            col[j] = col[j] * t % P_INT
            t = t * g % P_INT
    out = dft(col, w)
    t = c
    for i in range(n):
        out[i] = out[i] * t % P_INT
        if shift_after:
            t = t * g % P_INT
    return out


def ntt_definition(a, log_n, w, shift=None, scale=None, shift_after=False):
    """the contract of include/hsw.h, term by term: O(N^2)"""
    n = 1 << log_n
    g, c = 1 if shift is None else shift, 1 if scale is None else scale
    out = []
    for i in range(n):
        if shift_after:
            s = sum(a[j] * pow(w, i * j, P_INT) for j in range(len(a))) * pow(g, i, P_INT)
        else:
            s = sum(a[j] * pow(g, j, P_INT) * pow(w, i * j, P_INT) for j in range(len(a)))
        out.append(c * s % P_INT)
    return out


def default_launches(log_n, pass_log=0):
    """the launches of a column group: one digit up to pass_log bits, else digits of at most max(1, pass_log - 2)"""
    p = pass_log or 10
    s = p - 2 if p > 3 else 1
    return 1 if log_n <= p else -(-log_n // s)
