"""The step of the window's dense solve from the columns of L^-1, as the device orders it when the back-substitution rides under the
factorisation (pba_solve_kernels.hpp: choleskyAugmented with the column substitution, K <= 64).  NumPy only; nothing here is shared
with the kernel.

The factorisation leaves L and y = L^-1 g (row K of the augmented matrix).  The step is x = L^-T y, i.e. for every unknown q

    x_q = z_q . y,       z_q = L^-1 e_q   (column q of L^-1, a forward substitution)

The order of the arithmetic of ONE column q = 8 b + g (frame block b, column g inside it), the same whichever lanes carry it:

    s_i = 0 (8 rows) for every frame block i > b;  x = 0
    for kb = b .. F-1:                                        (block row kb is final once block column kb has been factored)
        t = e_g (kb == b)  or  -s_kb (kb > b)                 8 rows
        for c = 0 .. 7:                                       the 8-row solve with the diagonal block L_kb,kb and the pivot reciprocals
            a = t_c;  for c' = 0 .. c-1:  a = a - L[8 kb + c, 8 kb + c'] z_c'
            z_c = a * inv[8 kb + c]
        for c = 0 .. 7:  x = x + z_c y[8 kb + c]
        for i = kb+1 .. F-1, every row rho:  for c = 0 .. 7:  s_i[rho] = s_i[rho] + L[8 i + rho, 8 kb + c] z_c

(the device fuses every multiply-add of the three inner loops into one rounding; the order is what is stated here).  A pivot under the
guard has inv = 0 and a zero column of L: row r of every column is then 0 and column r is 0 altogether, so x_r = 0 and the other unknowns
solve the reduced system — what the substitution x_k = y_k inv_k, y -= L_k x_k does with inv_k = 0.
"""
import numpy as np

BLOCK = 8


def factor(A, g):
    """unblocked Cholesky of [[A, .], [g^T, 0]] in float64 with multiplied reciprocals (l_ik = c_ik * inv_k, inv_k = 0 for a pivot that is
    not positive): (L, y, inv)"""
    K = len(g)
    L = np.zeros((K + 1, K + 1))
    L[:K, :K] = np.tril(A)
    L[K, :K] = g
    inv = np.zeros(K)
    for k in range(K):
        d = L[k, k]
        inv[k] = 1.0 / np.sqrt(d) if d > 0 else 0.0
        L[k:, k] *= inv[k]
        L[k + 1:, k + 1:K] -= np.outer(L[k + 1:, k], L[k + 1:K, k])
    return np.tril(L[:K, :K]), L[K, :K].copy(), inv


def substitution_step(L, y, inv):
    """x = L^-T y by the column-oriented back substitution (backSubstituteWave's arithmetic)"""
    K = len(y)
    y = y.copy()
    x = np.zeros(K)
    for k in range(K - 1, -1, -1):
        x[k] = y[k] * inv[k]
        y[:k] -= L[k, :k] * x[k]
    return x


def columns_step_from_factor(L, y, inv, skip=None):
    """x from the columns of L^-1 in the order of the module's docstring.  skip = (q, kb, i): column q leaves out the contribution of its
    block kb to block row i (a deliberate fault for the test of the test)."""
    K = len(y)
    assert K % BLOCK == 0
    F = K // BLOCK
    x = np.zeros(K)
    for q in range(K):
        b, g = divmod(q, BLOCK)
        s = np.zeros((F, BLOCK))
        xq = 0.0
        for kb in range(b, F):
            k0 = BLOCK * kb
            if kb == b:
                t = np.zeros(BLOCK)
                t[g] = 1.0
            else:
                t = -s[kb]
            z = np.zeros(BLOCK)
            for c in range(BLOCK):
                a = t[c]
                for c2 in range(c):
                    a = a - L[k0 + c, k0 + c2] * z[c2]
                z[c] = a * inv[k0 + c]
            for c in range(BLOCK):
                xq = xq + z[c] * y[k0 + c]
            for i in range(kb + 1, F):
                if skip == (q, kb, i):
                    continue
                for c in range(BLOCK):
                    s[i] = s[i] + L[BLOCK * i:BLOCK * i + BLOCK, k0 + c] * z[c]
        x[q] = xq
    return x


def columns_step(A, g, skip=None):
    L, y, inv = factor(A, g)
    return columns_step_from_factor(L, y, inv, skip)
