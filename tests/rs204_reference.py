"""An RS(204,188) encoder and bounded-distance decoder for the FEC frame of the enhanced packet mode (ETSI EN 300 401 clause 5.3.5) that shares
nothing with tests/packet_model.py or the HIP kernels: GF(256) products by shift-and-reduce with 0x11D (no log / exp tables, the inverse by
exponentiation), parity by long division, and Peterson-Gorenstein-Zierler decoding (linear systems by Gaussian elimination, roots by trying
every non-zero element, error values from a Vandermonde system) -- in the manner of tests/rs_reference.py, which does the same for RS(120,110).

Both deciders answer the same question, so they must agree on every word: either a code word lies within Hamming distance 8 of the word, and
it is returned with the distance, or none does, and the word comes back unchanged with -1.

Conventions of the code itself: byte k of a word is the coefficient of x^(203 - k); the generator is prod (x + alpha^i), i = 0..15,
alpha = 0x02; the code is the (255,239) code shortened by 51 leading zero bytes."""
import numpy as np

POLY = 0x11D
N, K, NROOTS, T = 204, 188, 16, 8


def mul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        if a & 0x100:
            a ^= POLY
        b >>= 1
    return r


def power(a, n):
    r = 1
    while n:
        if n & 1:
            r = mul(r, a)
        a = mul(a, a)
        n >>= 1
    return r


def inv(a):
    assert a
    return power(a, 254)


def generator():
    """prod (x + alpha^i), i = 0..15, highest degree first."""
    g, root = [1], 1
    for _ in range(NROOTS):
        g = [a ^ b for a, b in zip(g + [0], [0] + [mul(c, root) for c in g])]
        root = mul(root, 2)
    return g


GEN = generator()


def encode(data):
    """188 data bytes -> the 16 parity bytes: the remainder of data(x) x^16 by the generator, by long division."""
    work = [int(b) for b in data] + [0] * NROOTS
    assert len(work) == N
    for k in range(K):
        q = work[k]
        if q:
            for t in range(NROOTS + 1):
                work[k + t] ^= mul(q, GEN[t])
    return np.array(work[K:], dtype=np.uint8)


def syndromes(word):
    """S_i = word(alpha^i), i = 0..15, by Horner."""
    out, x = [], 1
    for _ in range(NROOTS):
        s = 0
        for b in word:
            s = mul(s, x) ^ int(b)
        out.append(s)
        x = mul(x, 2)
    return out


def solve(A, b):
    """x with A x = b over GF(256) by Gaussian elimination; None when A is singular."""
    n = len(b)
    M = [list(row) + [rhs] for row, rhs in zip(A, b)]
    for c in range(n):
        piv = next((r for r in range(c, n) if M[r][c]), None)
        if piv is None:
            return None
        M[c], M[piv] = M[piv], M[c]
        f = inv(M[c][c])
        M[c] = [mul(f, v) for v in M[c]]
        for r in range(n):
            if r != c and M[r][c]:
                g = M[r][c]
                M[r] = [v ^ mul(g, w) for v, w in zip(M[r], M[c])]
    return [M[r][n] for r in range(n)]


def decode(word):
    """(code word, distance) when a code word lies within Hamming distance 8 of word, else (word unchanged, -1)."""
    r = [int(b) for b in word]
    assert len(r) == N
    same = np.array(r, dtype=np.uint8)
    S = syndromes(r)
    if not any(S):
        return same, 0
    # v errors at locators X_l = alpha^(p_l) and the polynomial prod (x + X_l) = x^v + c_(v-1) x^(v-1) + ... + c_0:
    # sum_t c_t S_(j+t) = S_(j+v) for j = 0..v-1.  The matrix is singular for every v above the true count.
    for v in range(T, 0, -1):
        c = solve([[S[j + t] for t in range(v)] for j in range(v)], [S[j + v] for j in range(v)])
        if c is not None:
            break
    else:
        return same, -1
    powers, x = [], 1
    for p in range(255):
        y = 1
        for t in range(v - 1, -1, -1):
            y = mul(y, x) ^ c[t]
        if y == 0:
            powers.append(p)
        x = mul(x, 2)
    if len(powers) != v or any(p >= N for p in powers):
        return same, -1
    X = [power(2, p) for p in powers]
    e = solve([[power(xl, i) for xl in X] for i in range(v)], S[:v])
    if e is None or not all(e):
        return same, -1
    for i in range(NROOTS):
        s = 0
        for xl, el in zip(X, e):
            s ^= mul(el, power(xl, i))
        if s != S[i]:
            return same, -1
    for p, el in zip(powers, e):
        r[N - 1 - p] ^= el
    return np.array(r, dtype=np.uint8), v
