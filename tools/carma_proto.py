"""numpy twin and definition of pioran.jl_amd/csrc/carma.hip, operation by operation, in fp64 or long double.

Every function takes the draws as arrays over a leading axis n (one entry per draw) and works elementwise, in the kernels' order of operations:

  quad2roots(quad)                    pairs (c, b) = (quad[:, k], quad[:, k + 1]): disc = b b - 4 c, root (-b / 2, +- sqrt(-disc) / 2); odd: -quad[:, -1]
  beta_from_quad(qb)                  the product of the real factors x^2 + qb[k+1] x + qb[k] (x + qb[-1] last, for odd q): ascending, monic
  frac(re, im, beta, i)               -beta(r) beta(-r) / Re r (Horner) divided by prod_{r_j != r} (r_j - r)(conj r_j + r), r = root i
  coefs(re, im, beta, norm, integrated)          CARMA_celerite_coefs (src/CARMA.jl:98-143): (a, b, c, d) [n][J]
  coefs_quad(qa, qb, norm, integrated)           ... from the quadratic factors
  vjp_quad(qa, qb, norm, integrated, ga, gb, gc, gd)   the Jacobian applied direction by direction with forward duals (class Dual): the SAME
                                      functions run on duals, as the kernel's template does; returns grad_qa, grad_qb, grad_norm
  evaluate(re, im, beta, norm, integrated, freq) evaluate(::CARMA, f) (src/CARMA.jl:150-172): |alpha(iw)|^2 as prod (Re r)^2 + (w - Im r)^2
  reject_quad(qa, qb, norm, bounds) / reject_roots(...)    the flag of each draw: 0, or the first of 1 non-finite, 2 not a conjugate pair,
                                      3 real part >= 0, 4 outside the bounds

mistake=<name>: one seeded mistake per step, for the CPU suite (tests/test_carma_host.py shows that the bar catches each):
  "root_half"       quad2roots: the imaginary part without its / 2
  "odd_q_factor"    beta: the factor of an odd q taken as qb[-1] x + 1 (x - qb[-1] would not show: beta(r) beta(-r) does not see the sign of a root)
  "conj_dropped"    frac: (r_j + r) in place of (conj r_j + r)
  "filter_wrong"    frac: the filter skips the root's conjugate partner instead of the root itself
  "real_doubled"    coefs: the 2 x of the paired terms applied to the real term too
  "d_sign"          coefs: d = +Im r
  "norm_abs"        coefs: the integrated normalisation divides by sum |a|
  "vjp_v_const"     vjp: the normalising sum treated as a constant
  "psd_factor"      evaluate: the integrated form with the factor 4 of the other
  "psd_norm_half"   evaluate: CARMA_normalisation summed over every second root only
  "reject_ge"       rejection: a pair with disc == 0 accepted (disc > 0 in place of >=)
"""
import numpy as np

MISTAKES = ("root_half", "odd_q_factor", "conj_dropped", "filter_wrong", "real_doubled", "d_sign", "norm_abs", "vjp_v_const", "psd_factor",
            "psd_norm_half")


class Dual:
    """value + derivative along one seeded input, with the kernel's operations"""
    __array_ufunc__ = None   # ndarray (op) Dual is Dual's reflected operation

    def __init__(self, v, d=None):
        self.v = v
        self.d = np.zeros_like(v) if d is None else d

    @staticmethod
    def lift(x, like):
        return x if isinstance(x, Dual) else Dual(np.zeros_like(like.v) + x)

    def __add__(self, o):
        o = Dual.lift(o, self)
        return Dual(self.v + o.v, self.d + o.d)

    __radd__ = __add__

    def __sub__(self, o):
        o = Dual.lift(o, self)
        return Dual(self.v - o.v, self.d - o.d)

    def __rsub__(self, o):
        return Dual.lift(o, self) - self

    def __neg__(self):
        return Dual(-self.v, -self.d)

    def __mul__(self, o):
        o = Dual.lift(o, self)
        return Dual(self.v * o.v, self.v * o.d + self.d * o.v)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Dual.lift(o, self)
        q = self.v / o.v
        return Dual(q, (self.d - q * o.d) / o.v)


def _val(x):
    return x.v if isinstance(x, Dual) else x


def _sqrt(x):
    if isinstance(x, Dual):
        s = np.sqrt(x.v)
        return Dual(s, x.d / (2 * s))
    return np.sqrt(x)


def _where(mask, a, b):
    if isinstance(a, Dual) or isinstance(b, Dual):
        ref = a if isinstance(a, Dual) else b
        a, b = Dual.lift(a, ref), Dual.lift(b, ref)
        return Dual(np.where(mask, a.v, b.v), np.where(mask, a.d, b.d))
    return np.where(mask, a, b)


def _cols(x, dtype, seed=None, off=0):
    """the columns of x [n][m] as a list of arrays in `dtype`; seed = direction: duals, the derivative 1 in column seed - off"""
    x = np.asarray(x, dtype=dtype)
    cols = [x[:, k] for k in range(x.shape[1])]
    if seed is None:
        return cols
    return [Dual(c, np.ones_like(c) if k + off == seed else np.zeros_like(c)) for k, c in enumerate(cols)]


def quad2roots(quad, mistake=None):
    """quad: list of n columns -> (re, im): lists of n columns"""
    n = len(quad)
    re, im = [None] * n, [None] * n
    for k in range(0, n - n % 2, 2):
        c, b = quad[k], quad[k + 1]
        disc = b * b - 4.0 * c
        h = _sqrt(-disc) * (1.0 if mistake == "root_half" else 0.5)
        r = -b * 0.5
        re[k], im[k], re[k + 1], im[k + 1] = r, h, r, -h
    if n % 2:
        re[n - 1] = -quad[n - 1]
        im[n - 1] = quad[n - 1] * 0.0
    return re, im


def beta_from_quad(qb, like, mistake=None):
    """qb: list of q columns -> beta: list of q + 1 columns; `like`: a column giving shape and dtype"""
    one = like * 0.0 + 1.0
    beta = [one]
    q = len(qb)
    for k in range(0, q - q % 2, 2):
        c, b = qb[k], qb[k + 1]
        deg = len(beta) - 1
        new = []
        for i in range(deg + 3):
            acc = c * beta[i] if i <= deg else one * 0.0
            if i >= 1 and i - 1 <= deg:
                acc = acc + b * beta[i - 1]
            if i >= 2:
                acc = acc + beta[i - 2]
            new.append(acc)
        beta = new
    if q % 2:
        s = qb[q - 1]
        s0, s1 = (one, s) if mistake == "odd_q_factor" else (s, one)
        deg = len(beta) - 1
        new = []
        for i in range(deg + 2):
            acc = s0 * beta[i] if i <= deg else one * 0.0
            if i >= 1:
                acc = acc + (s1 * beta[i - 1] if mistake == "odd_q_factor" else beta[i - 1])
            new.append(acc)
        beta = new
    return beta


def frac(re, im, beta, i, mistake=None):
    p, q = len(re), len(beta) - 1
    xr, xi = re[i], im[i]
    ar, ai, br, bi = beta[q], beta[q] * 0.0, beta[q], beta[q] * 0.0
    for l in range(q - 1, -1, -1):
        bl = beta[l]
        t = ar * xr - ai * xi + bl
        ai = ar * xi + ai * xr
        ar = t
        t = bl - (br * xr - bi * xi)
        bi = -(br * xi + bi * xr)
        br = t
    nr, ni = -(ar * br - ai * bi) / xr, -(ar * bi + ai * br) / xr
    dr, di = xr * 0.0 + 1.0, xr * 0.0
    for j in range(p):
        ur, ui = re[j], im[j]
        if mistake == "filter_wrong":
            skip = (_val(ur) == _val(xr)) & (_val(ui) == -_val(xi)) & (_val(xi) != 0)
            skip = skip | ((_val(xi) == 0) & (_val(ur) == _val(xr)) & (_val(ui) == 0))
        else:
            skip = (_val(ur) == _val(xr)) & (_val(ui) == _val(xi))
        er, ei, gr = ur - xr, ui - xi, ur + xr
        gi = xi + ui if mistake == "conj_dropped" else xi - ui
        pr, pi = er * gr - ei * gi, er * gi + ei * gr
        pr, pi = _where(skip, 1.0, pr), _where(skip, 0.0, pi)
        t = dr * pr - di * pi
        di = dr * pi + di * pr
        dr = t
    m = dr * dr + di * di
    return (nr * dr + ni * di) / m, (ni * dr - nr * di) / m


def terms(re, im, beta, mistake=None):
    """(a, b, c, d) before the normalisation: lists of J columns"""
    p = len(re)
    J = (p + 1) // 2
    a, b, c, d = [], [], [], []
    for k in range(J):
        fr, fi = frac(re, im, beta, 2 * k, mistake)
        real_term = p % 2 == 1 and 2 * k == p - 1
        a.append(fr if real_term and mistake != "real_doubled" else 2.0 * fr)
        b.append(fr * 0.0 if real_term else 2.0 * fi)
        c.append(-re[2 * k])
        d.append(fr * 0.0 if real_term else (im[2 * k] if mistake == "d_sign" else -im[2 * k]))
    return a, b, c, d


def _stack(cols):
    return np.stack([_val(c) for c in cols], axis=1)


def coefs(re, im, beta, norm, integrated, mistake=None):
    a, b, c, d = terms(re, im, beta, mistake)
    variance = a[0] * 0.0
    for ak in a:
        variance = variance + (abs(ak) if mistake == "norm_abs" else ak)
    va = norm / variance if integrated else norm + variance * 0.0
    return _stack([ak * va for ak in a]), _stack([bk * va for bk in b]), _stack(c), _stack(d)


def stage_quad(qa, qb, dtype, seed=None, mistake=None):
    qa = np.asarray(qa, dtype=dtype)
    p = qa.shape[1]
    qa_c = _cols(qa, dtype, seed, 0)
    qb_c = _cols(np.asarray(qb, dtype=dtype).reshape(qa.shape[0], -1), dtype, seed, p)
    re, im = quad2roots(qa_c, mistake)
    beta = beta_from_quad(qb_c, qa_c[0], mistake)
    return re, im, beta


def roots_of_quad(qa, qb, dtype=np.float64):
    """(r_alpha [n][p] complex, beta [n][q + 1]) the twin forms from the quadratic factors"""
    re, im, beta = stage_quad(qa, qb, dtype)
    return _stack(re) + 1j * _stack(im), _stack(beta)


def coefs_quad(qa, qb, norm, integrated, dtype=np.float64, mistake=None):
    re, im, beta = stage_quad(qa, qb, dtype, None, mistake)
    return coefs(re, im, beta, np.asarray(norm, dtype=dtype), integrated, mistake)


def coefs_roots(r_alpha, beta, norm, integrated, dtype=np.float64, mistake=None):
    r_alpha = np.asarray(r_alpha)
    return coefs(_cols(r_alpha.real, dtype), _cols(r_alpha.imag, dtype), _cols(beta, dtype), np.asarray(norm, dtype=dtype), integrated, mistake)


def vjp_quad(qa, qb, norm, integrated, ga, gb, gc, gd, dtype=np.float64, mistake=None):
    qa = np.asarray(qa, dtype=dtype)
    n, p = qa.shape
    qb = np.asarray(qb, dtype=dtype).reshape(n, -1)
    q = qb.shape[1]
    norm = np.asarray(norm, dtype=dtype)
    ga, gb, gc, gd = (np.asarray(g, dtype=dtype) for g in (ga, gb, gc, gd))
    grad = np.zeros((n, p + q), dtype=dtype)
    gnorm = np.zeros(n, dtype=dtype)
    for direction in range(p + q):
        re, im, beta = stage_quad(qa, qb, dtype, direction)
        a, b, c, d = terms(re, im, beta)
        zero = Dual(np.zeros(n, dtype=dtype))
        W, V, X = zero, zero, zero
        for k in range(len(a)):
            W = W + ga[:, k] * a[k] + gb[:, k] * b[k]
            V = V + a[k]
            X = X + gc[:, k] * c[k] + gd[:, k] * d[k]
        if mistake == "vjp_v_const":
            V = Dual(V.v)
        G = (norm * W / V if integrated else norm * W) + X
        grad[:, direction] = G.d
        if direction == 0:
            gnorm = W.v / V.v if integrated else W.v
    return grad[:, :p], grad[:, p:], gnorm


def evaluate(re, im, beta, norm, integrated, freq, times_f=False, mistake=None):
    """re, im: lists of p columns, beta: list of q + 1 columns (plain values) -> psd [n][F]"""
    p, q = len(re), len(beta) - 1
    dtype = re[0].dtype
    freq = np.asarray(freq, dtype=dtype)
    if integrated and mistake != "psd_factor":
        variance = re[0] * 0.0
        for i in range(0, p, 2 if mistake == "psd_norm_half" else 1):
            variance = variance + 0.5 * frac(re, im, beta, i)[0]
        s = 2.0 * norm / variance
    else:
        s = 4.0 * norm
    w = 2.0 * (dtype.type(4) * np.arctan(dtype.type(1))) * freq[None, :]
    nr, ni = beta[q][:, None] + 0.0 * w, 0.0 * w
    for l in range(q - 1, -1, -1):
        t = beta[l][:, None] - ni * w
        ni = nr * w
        nr = t
    den = 1.0 + 0.0 * w
    for l in range(p):
        x, y = re[l][:, None], w - im[l][:, None]
        den = den * (x * x + y * y)
    v = (nr * nr + ni * ni) / den * s[:, None]
    return v * freq[None, :] if times_f else v


def evaluate_quad(qa, qb, norm, integrated, freq, dtype=np.float64, times_f=False, mistake=None):
    re, im, beta = stage_quad(qa, qb, dtype)
    return evaluate(re, im, beta, np.asarray(norm, dtype=dtype), integrated, freq, times_f, mistake)


def evaluate_roots(r_alpha, beta, norm, integrated, freq, dtype=np.float64, times_f=False, mistake=None):
    r_alpha = np.asarray(r_alpha)
    return evaluate(_cols(r_alpha.real, dtype), _cols(r_alpha.imag, dtype), _cols(beta, dtype), np.asarray(norm, dtype=dtype), integrated, freq, times_f,
                    mistake)


def _in_bounds(re, im, f_lo, f_hi):
    return (-f_hi < re) & (re < -f_lo) & (-f_hi < im) & (im < f_hi)


def _reject_quad_one(quad, bounds, seen, mistake=None):
    n, m = quad.shape
    seen[1] |= ~np.all(np.isfinite(quad), axis=1) if m else False
    with np.errstate(invalid="ignore"):
        for k in range(0, m - m % 2, 2):
            c, b = quad[:, k], quad[:, k + 1]
            disc = b * b - 4.0 * c
            pair = disc <= 0.0 if mistake == "reject_ge" else disc < 0.0
            seen[2] |= ~pair
            h, r = np.sqrt(np.where(pair, -disc, 0.0)) * 0.5, -b * 0.5
            seen[3] |= pair & ~(r < 0.0)
            if bounds:
                seen[4] |= pair & ~(_in_bounds(r, h, *bounds) & _in_bounds(r, -h, *bounds))
        if m % 2:
            r = -quad[:, m - 1]
            seen[3] |= ~(r < 0.0)
            if bounds:
                seen[4] |= ~_in_bounds(r, 0.0 * r, *bounds)


def _first(seen, n):
    flag = np.zeros(n, dtype=np.int32)
    for reason in (4, 3, 2, 1):
        flag[seen[reason]] = reason
    return flag


def reject_quad(qa, qb, norm, bounds=None, mistake=None):
    qa = np.asarray(qa, dtype=np.float64)
    n = qa.shape[0]
    qb = np.asarray(qb, dtype=np.float64).reshape(n, -1)
    seen = {r: np.zeros(n, dtype=bool) for r in (1, 2, 3, 4)}
    seen[1] |= ~np.isfinite(np.broadcast_to(norm, (n,)))
    _reject_quad_one(qa, bounds, seen, mistake)
    _reject_quad_one(qb, bounds, seen, mistake)
    return _first(seen, n)


def reject_roots(r_alpha, beta, norm, bounds=None):
    r_alpha = np.asarray(r_alpha, dtype=complex)
    n = r_alpha.shape[0]
    seen = {r: np.zeros(n, dtype=bool) for r in (1, 2, 3, 4)}
    seen[1] |= ~np.isfinite(np.broadcast_to(norm, (n,))) | ~np.all(np.isfinite(r_alpha), axis=1) | ~np.all(np.isfinite(np.asarray(beta, float)), axis=1)
    with np.errstate(invalid="ignore"):
        seen[3] |= ~np.all(r_alpha.real < 0.0, axis=1)
        if bounds:
            seen[4] |= ~np.all(_in_bounds(r_alpha.real, r_alpha.imag, *bounds), axis=1)
    return _first(seen, n)
