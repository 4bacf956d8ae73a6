"""The fp64 transform arithmetic of pir_amd/csrc/arith.h and ntt_core.h restated on the CPU -- TEST INFRASTRUCTURE.

`f64_mulmod`, `f64_norm` and the fp64 butterflies with their normalisation schedule:

  forward   flavour 1 (exact fp64): no normalisation before the end; flavour 2 (wide): the multiplied input of every
            butterfly is normalised first
  inverse   flavour 1: sums run unnormalised through the (up to) 4 stages of a register pass and are normalised between
            passes -- or never, in the lazy form (bits(q) + log2 N <= 52); flavour 2: every sum is normalised

Roundings are numpy doubles (IEEE round-to-nearest-even, what the GPU's v_mul_f64 / v_fma_f64 / v_add_f64 / v_rndne_f64
do); every fused multiply-add is recomputed in Python integers and rounded once.  At every step the model checks that
the value the kernel keeps IS the exact integer it stands for (`Inexact` otherwise) and records how large the values
and the quotient-estimate errors became.  The butterflies are in SEAL's order (Cooley-Tukey forward, Gentleman-Sande
inverse over bit-reversed twiddles); the kernel's register / LDS arrangement only permutes which thread holds what.

The model chooses inputs and checks the comments of the kernels (tests/test_f64_bounds_model.py).  GPU results are never
compared with it: those are compared with the oracle and with big-integer formulas (tests/test_gpu_extreme_values.py)."""
import numpy as np

TWO53 = 2 ** 53


class Inexact(AssertionError):
    """A value the kernel would keep is not the integer it stands for."""


def ints(a):
    """float64 array of integers -> object array of Python ints (exact)."""
    return np.array([int(v) for v in a.ravel().tolist()], dtype=object).reshape(a.shape)


def floats(a):
    """object array of Python ints -> float64, each rounded once to nearest-even (what one fma does to its exact value)."""
    return np.array([float(v) for v in a.ravel().tolist()], dtype=np.float64).reshape(a.shape)


def _require_exact(f, exact, what):
    if not np.array_equal(ints(f), exact):
        raise Inexact(what)


def bitrev(i, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (i & 1)
        i >>= 1
    return r


class Stats:
    def __init__(self):
        self.max_abs = 0.0            # largest |value| kept, in units of q
        self.max_value = 0.0          # ... and as an absolute number (an exact integer below 2^53)
        self.max_product = 0.0        # largest |f64_mulmod result| / q
        self.max_norm = 0.0           # largest |f64_norm result| / q
        self.max_quotient_error = 0.0  # largest |fl(h / q) - exact product / q| over all quotient estimates
        self.wrong_quotients = 0      # estimates that rounded to another integer than the exact quotient does
        self.stage_max = []           # per stage: largest |value| / q after it
        self.last_product = 0.0       # largest |result| / q of the inverse's last stage (what gets packed)


class Field:
    """One modulus with its centred twiddle tables (ctx.hip: twf / itwf / ninv_f / iw1n_f)."""

    def __init__(self, q, N, psi):
        self.q, self.N, self.logN = int(q), N, N.bit_length() - 1
        self.qd = np.float64(self.q)
        self.qinv = np.float64(1.0) / self.qd
        centred = lambda v: v - self.q if v > self.q // 2 else v
        psi = int(psi)
        assert pow(psi, N, self.q) == self.q - 1
        tw = [pow(psi, bitrev(j, self.logN), self.q) for j in range(N)]
        self.tw = np.array([float(centred(v)) for v in tw])
        self.itw = np.array([float(centred(pow(v, -1, self.q))) for v in tw])
        ninv = pow(N, -1, self.q)
        self.ninv = np.float64(centred(ninv))
        self.iw1n = np.float64(centred(pow(tw[1], -1, self.q) * ninv % self.q))

    # ---- arith.h
    def mulmod(self, y, w, st):
        q = self.q
        h = y * w
        P = ints(y) * ints(np.broadcast_to(w, y.shape))
        H = ints(h)
        lo = floats(P - H)                                   # fma(y, w, -h)
        _require_exact(lo, P - H, "low half of a product")
        est = h * self.qinv
        kf = np.rint(est)
        K = ints(kf)
        E = H - K * q                                        # fma(-k, q, h)
        r = floats(E)
        _require_exact(r, E, "h - k q")
        res = r + lo
        R = P - K * q
        _require_exact(res, R, "product residue")
        # the quotient estimate against the exact quotient P / q = K + R / q
        err = np.abs((est - kf) - floats(R) / self.qd)
        st.max_quotient_error = max(st.max_quotient_error, float(err.max()))
        st.wrong_quotients += int(np.count_nonzero(np.abs(floats(R)) > 0.5 * self.qd))
        st.max_product = max(st.max_product, float(np.abs(res).max() / self.qd))
        return res

    def norm(self, x, st):
        kf = np.rint(x * self.qinv)
        E = ints(x) - ints(kf) * self.q
        r = floats(E)
        _require_exact(r, E, "x - k q")
        st.max_norm = max(st.max_norm, float(np.abs(r).max() / self.qd))
        return r

    def add(self, a, b, st):
        """a + b (or a - b: pass -b), exact iff the integer sum is representable."""
        s = a + b
        if float(np.abs(s).max()) > TWO53:
            _require_exact(s, ints(a) + ints(b), "sum above 2^53")
        return s

    def _seen(self, x, st):
        m = float(np.abs(x).max())
        st.max_abs = max(st.max_abs, m / float(self.qd))
        st.max_value = max(st.max_value, m)

    # ---- ntt_core.h
    def forward(self, residues, mode, canonical=True):
        """Canonical residues (coefficients) -> canonical residues in SEAL's NTT order, and the statistics.  With
        `canonical` off the inputs may be signed representatives (the upper level's plain lift) and the signed
        representatives of the outputs are returned as doubles (ntt_forward<..., CANON = false>, A::signed_fwd: what
        upper_fused_kernel multiplies and upper_ntt_kernel stores)."""
        assert mode in (1, 2)
        st = Stats()
        N = self.N
        a = np.array([float(int(v)) for v in residues])
        t, m = N, 1
        while m < N:
            t >>= 1
            x = a.reshape(m, 2, t)
            w = self.tw[m:2 * m].reshape(m, 1)
            y = self.norm(x[:, 1, :], st) if mode == 2 else x[:, 1, :]
            p = self.mulmod(y, w, st)
            lo, hi = self.add(x[:, 0, :], p, st), self.add(x[:, 0, :], -p, st)
            a = np.stack([lo, hi], axis=1).reshape(N)
            self._seen(a, st)
            st.stage_max.append(float(np.abs(a).max() / self.qd))
            m <<= 1
        r = self.norm(a, st)                                 # canon_fwd / signed_fwd
        if not canonical:
            return r, st
        r = np.where(r < 0, r + self.qd, r)
        return self._canonical(r), st

    def inverse(self, residues, mode, lazy=False):
        """Canonical residues in SEAL's NTT order -> canonical coefficients (scaled by 1 / N), and the statistics.
        `lazy` is the kernel's f64_lazy_inv (flavour 1 only)."""
        assert mode in (1, 2) and not (lazy and mode != 1)
        st = Stats()
        N, logN = self.N, self.logN
        a = np.array([float(int(v)) for v in residues])
        t, m, stage = 1, N, 0
        while m > 1:
            h = m >> 1
            stage += 1
            x = a.reshape(h, 2, t)
            u, d = self.add(x[:, 0, :], x[:, 1, :], st), self.add(x[:, 0, :], -x[:, 1, :], st)
            self._seen(u, st)
            self._seen(d, st)
            if stage == logN:                                # inv_last: N^-1 folded into both outputs
                lo = self.mulmod(u, self.ninv, st)
                hi = self.mulmod(d, self.iw1n, st)
                st.last_product = float(max(np.abs(lo).max(), np.abs(hi).max()) / self.qd)
            else:
                lo = self.norm(u, st) if mode == 2 else u
                hi = self.mulmod(d, self.itw[h:2 * h].reshape(h, 1), st)
            a = np.stack([lo, hi], axis=1).reshape(N)
            if mode == 1 and not lazy and stage % 4 == 0 and stage != logN:
                a = self.norm(a, st)                         # pass_norm: between register passes of 4 stages
            st.stage_max.append(float(np.abs(a).max() / self.qd))
            t <<= 1
            m = h
        r = np.where(a < 0, a + self.qd, a)                  # canon_inv
        return self._canonical(r), st

    def _canonical(self, r):
        if float(r.min()) < 0 or float(r.max()) >= float(self.qd):
            raise Inexact("result outside [0, q)")
        return np.array([int(v) for v in r.tolist()], dtype=np.uint64)
