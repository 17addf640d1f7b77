"""The host number theory of csrc/host_math.cpp restated in Python integers, as the reference of tests/test_host_math_range.py and
tests/test_gpu_modulus_range.py: the prime rule, minimal primitive roots, Barrett ratios, root-power, Shoup and cyclic tables, and
the negacyclic transform and product by their defining sums.  Nothing here imports the package or the oracle.

Primality: trial division below 2^20; above it Miller-Rabin on the first twelve primes, which is deterministic below 3.3e24."""

TRIAL_LIMIT = 1 << 20
_MR_BASES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)


def is_prime(n: int) -> bool:
    if n < 2:
        return False
    if n < TRIAL_LIMIT:
        if n % 2 == 0:
            return n == 2
        d = 3
        while d * d <= n:
            if n % d == 0:
                return False
            d += 2
        return True
    for p in _MR_BASES:
        if n % p == 0:
            return False
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in _MR_BASES:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


# ------------------------------------------------------------------ the prime rule
def primes_in_class(N: int, bits: int, count=None) -> list:
    """The ``count`` largest primes p with 2^(bits-1) < p < 2^bits and p = 1 mod 2N, smallest first; all of them with ``count``
    None.  ValueError when the interval holds fewer than ``count``."""
    step, floor_ = 2 * N, 1 << (bits - 1)
    cand = ((1 << bits) - 1) // step * step + 1
    out = []
    while cand > floor_ and (count is None or len(out) < count):
        if is_prime(cand):
            out.append(cand)
        cand -= step
    if count is not None and len(out) != count:
        raise ValueError(f"only {len(out)} primes of {bits} bits are 1 mod {step}")
    return out[::-1]


def create_moduli(N: int, bits: list) -> list:
    """One prime per entry of ``bits``: every size takes the largest primes of its class, as many as the list asks for, and hands
    them out smallest first in request order."""
    pool = {b: primes_in_class(N, b, bits.count(b)) for b in set(bits)}
    used = {b: 0 for b in pool}
    out = []
    for b in bits:
        out.append(pool[b][used[b]])
        used[b] += 1
    return out


def first_prime_above(limit: int, N: int) -> int:
    """The smallest prime above ``limit`` that is 1 mod 2N."""
    p = limit // (2 * N) * (2 * N) + 1
    while p <= limit or not is_prime(p):
        p += 2 * N
    return p


def last_prime_below(limit: int, N: int) -> int:
    """The largest prime below ``limit`` that is 1 mod 2N."""
    p = (limit - 1) // (2 * N) * (2 * N) + 1
    while p >= limit or not is_prime(p):
        p -= 2 * N
    return p


def smallest_prime(N: int) -> int:
    """The smallest prime that is 1 mod 2N."""
    return first_prime_above(1, N)


# ------------------------------------------------------------------ roots
BRUTE_LIMIT = 1 << 12


def min_primitive_root(q: int, order: int) -> int:
    """The numerically smallest element of multiplicative order ``order`` (a power of two dividing q - 1) modulo the prime q.
    Below 2^12: the first x in 2, 3, ... whose powers x, x^2, ... reach 1 at the exponent ``order`` and not before, by walking them.
    Above: g = c^((q-1)/order) for the first c with g^(order/2) = -1, and the minimum over the odd powers of g, which are all the
    elements of that order."""
    assert order >= 2 and order & (order - 1) == 0 and (q - 1) % order == 0
    if q < BRUTE_LIMIT:
        for x in range(2, q):
            y, k = x, 1
            while y != 1 and k <= order:
                y = y * x % q
                k += 1
            if y == 1 and k == order:
                return x
        raise ValueError("no element of that order")
    g = next(r for r in (pow(c, (q - 1) // order, q) for c in range(2, 4100)) if pow(r, order // 2, q) == q - 1)
    g2, cur, best = g * g % q, g, g
    for _ in range(order // 2 - 1):
        cur = cur * g2 % q
        best = min(best, cur)
    return best


# ------------------------------------------------------------------ Barrett ratio
def const_ratio(q: int) -> list:
    """[floor(2^128 / q) low word, high word, 2^128 mod q]"""
    full = (1 << 128) // q
    return [full & (2**64 - 1), full >> 64, (1 << 128) % q]


# ------------------------------------------------------------------ tables
def bit_reverse(x: int, bits: int) -> int:
    r = 0
    for _ in range(bits):
        r, x = (r << 1) | (x & 1), x >> 1
    return r


def root_powers(q: int, logn: int, psi: int):
    """(rp, shoup): rp[bitrev(i)] = psi^i for i < 2^logn, shoup[k] = floor(rp[k] 2^64 / q)."""
    N = 1 << logn
    rp, rev, p = [0] * N, [0] * N, 1 % q
    for i in range(N):
        rev[i] = (rev[i >> 1] >> 1) | ((i & 1) << (logn - 1))          # = bit_reverse(i, logn)
        rp[rev[i]] = p
        p = p * psi % q
    return rp, [(w << 64) // q for w in rp]


def cyclic_table(mod: int, logn: int, root: int, nth_root_convention: bool) -> list:
    """The cyclic table in network order: tw[0] = 1, tw[m + i] = wlen(2m)^bitrev_{log2 m}(i) for m = 1, 2, .., n/2, where
    wlen(len) = root^((mod-1)/len) under the generator convention and root^(n/len) under the n-th-root convention."""
    n = 1 << logn
    tw = [1 % mod] * n
    for s in range(logn):
        m = 1 << s
        wlen = pow(root, n // (2 * m), mod) if nth_root_convention else pow(root, (mod - 1) // (2 * m), mod)
        for i in range(m):
            tw[m + i] = pow(wlen, bit_reverse(i, s), mod)
    return tw


# ------------------------------------------------------------------ schoolbook negacyclic forms, N <= 2^6
SCHOOLBOOK_MAX = 1 << 6


def negacyclic_forward(a: list, q: int, psi: int) -> list:
    """out[j] = sum_i a[i] psi^((2 bitrev(j) + 1) i): the evaluations at the odd powers of psi, in bit-reversed order."""
    N = len(a)
    assert N <= SCHOOLBOOK_MAX
    logn = N.bit_length() - 1
    return [sum(a[i] * pow(psi, (2 * bit_reverse(j, logn) + 1) * i, q) for i in range(N)) % q for j in range(N)]


def negacyclic_inverse(A: list, q: int, psi: int) -> list:
    """a[i] = N^-1 sum_j A[j] psi^(-(2 bitrev(j) + 1) i)"""
    N = len(A)
    assert N <= SCHOOLBOOK_MAX
    logn = N.bit_length() - 1
    ninv, ipsi = pow(N, -1, q), pow(psi, -1, q)
    return [ninv * sum(A[j] * pow(ipsi, (2 * bit_reverse(j, logn) + 1) * i, q) for j in range(N)) % q for i in range(N)]


def negacyclic_product(a: list, b: list, q: int) -> list:
    """a b mod (x^N + 1, q): c[k] = sum_{i+j=k} a_i b_j - sum_{i+j=k+N} a_i b_j"""
    N = len(a)
    assert N <= SCHOOLBOOK_MAX
    c = [0] * N
    for i in range(N):
        for j in range(N):
            if i + j < N:
                c[i + j] += a[i] * b[j]
            else:
                c[i + j - N] -= a[i] * b[j]
    return [x % q for x in c]
