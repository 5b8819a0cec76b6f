"""The IQ conditioner's definition in float64 (include/lora_hip_conditioner.h restated; csrc/lora_conditioner.hip is held to it).

The stream is x[n], n = 0, 1, ...; block k is items k B .. k B + B - 1, B a power of two; the window is W blocks.
    moments    per block five fp64 sums S_I, S_Q, S_II, S_QQ, S_IQ of the items converted to double (every product is exact).
               Order: rows of 64 items; 64 ascending chains from +0, chain p over items p, p + 64, p + 128, ...; then a halving
               tree over the 64 totals, t[i] = t[i] + t[i + s] for i < s, s = 32, 16, .., 1.
    window     sums over blocks max(0, k - W + 1) .. k, ascending, from +0; cnt = (k - lo + 1) B.
    estimates  mI = S_I / cnt, mQ = S_Q / cnt, cII = S_II / cnt - mI mI, cQQ = S_QQ / cnt - mQ mQ, cIQ = S_IQ / cnt - mI mQ,
               r = cIQ / cII, q = cQQ / cII, e = q - r r, b = 1 / sqrt(e), a = -r b; a = 0, b = 1 unless cII > 0 and e > 2^-12.
    parameters dI = fl32(mI), dQ = fl32(mQ), fl32(a), fl32(b); dc off: dI = dQ = 0; iq off: a = 0, b = 1.
    output     fp32, one rounding per operation:  zI = I - dI,  u = Q - dQ,  zQ = (a zI) + (b u); block k with block k's parameters,
               the items behind the last complete block with the last block's parameters (identity if there is none).
For a proper signal behind y = I + j g (Q cos phi + I sin phi) + d:  cII = P, cIQ = g sin phi P, cQQ = g^2 P, so a = -tan phi and
b = 1 / (g cos phi) undo the mismatch and leave I's scale as it is.  This is the project's own definition.
"""
from __future__ import annotations

import numpy as np

MIN_BLOCK, MAX_BLOCK = 256, 65536        # include/lora_hip_conditioner.h
MAX_WINDOW = 256
DEFAULT_BLOCK, DEFAULT_WINDOW = 4096, 16
ROW = 64
E_MIN = 2.0 ** -12
IDENTITY = (0.0, 0.0, 0.0, 1.0)


def check(block=DEFAULT_BLOCK, window=DEFAULT_WINDOW):
    """The limits of the header; ValueError outside them."""
    B, W = int(block), int(window)
    if B != block or W != window or B < MIN_BLOCK or B > MAX_BLOCK or B & (B - 1):
        raise ValueError("block %r must be a power of two in %d .. %d" % (block, MIN_BLOCK, MAX_BLOCK))
    if W < 1 or W > MAX_WINDOW:
        raise ValueError("window %r must be 1 .. %d blocks" % (window, MAX_WINDOW))
    return B, W


def block_moments(x, block=DEFAULT_BLOCK) -> np.ndarray:
    """float64[n_blocks, 5]: S_I, S_Q, S_II, S_QQ, S_IQ of every complete block of x, in the header's summation order."""
    B, _ = check(block, 1)
    x = np.asarray(x)
    nb = x.size // B
    v = x[:nb * B].reshape(nb, B // ROW, ROW)
    I, Q = v.real.astype(np.float64), v.imag.astype(np.float64)
    out = np.zeros((nb, 5), dtype=np.float64)
    for c, term in enumerate((I, Q, I * I, Q * Q, I * Q)):
        t = np.zeros((nb, ROW), dtype=np.float64)
        for r in range(B // ROW):
            t = t + term[:, r, :]
        s = ROW // 2
        while s >= 1:
            t[:, :s] = t[:, :s] + t[:, s:2 * s]
            s //= 2
        out[:, c] = t[:, 0]
    return out


def window_sums(moments, window=DEFAULT_WINDOW):
    """(float64[n_blocks, 5], blocks in each window): block k's sums over blocks max(0, k - W + 1) .. k, ascending from +0."""
    m = np.asarray(moments, dtype=np.float64)
    W = int(window)
    S = np.zeros_like(m)
    nw = np.minimum(np.arange(m.shape[0]) + 1, W)
    for k in range(m.shape[0]):
        acc = np.zeros(5, dtype=np.float64)
        for j in range(k - nw[k] + 1, k + 1):
            acc = acc + m[j]
        S[k] = acc
    return S, nw


def estimates(S, cnt) -> dict:
    """The header's ten fp64 operations on window sums S[..., 5] over cnt items each, every intermediate by name, guard applied to
    a and b (`guarded` says where)."""
    S = np.asarray(S, dtype=np.float64)
    cnt = np.asarray(cnt, dtype=np.float64)
    with np.errstate(all="ignore"):
        mI, mQ = S[..., 0] / cnt, S[..., 1] / cnt
        eII, eQQ, eIQ = S[..., 2] / cnt, S[..., 3] / cnt, S[..., 4] / cnt
        cII, cQQ, cIQ = eII - mI * mI, eQQ - mQ * mQ, eIQ - mI * mQ
        r, q = cIQ / cII, cQQ / cII
        e = q - r * r
        b = 1.0 / np.sqrt(e)
        a = -r * b
        ok = (cII > 0.0) & (e > E_MIN)
    return dict(mI=mI, mQ=mQ, eII=eII, eQQ=eQQ, eIQ=eIQ, cII=cII, cQQ=cQQ, cIQ=cIQ, r=r, q=q, e=e, a=np.where(ok, a, 0.0), b=np.where(ok, b, 1.0),
                guarded=~ok)


def parameters(S, cnt, dc=True, iq=True) -> np.ndarray:
    """float32[..., 4]: dI, dQ, a, b, each rounded once."""
    est = estimates(S, cnt)
    p = np.zeros(np.shape(est["mI"]) + (4,), dtype=np.float32)
    p[..., 3] = 1.0
    if dc:
        p[..., 0], p[..., 1] = est["mI"], est["mQ"]       # (the assignment rounds to float32)
    if iq:
        p[..., 2], p[..., 3] = est["a"], est["b"]
    return p


def parameter_bound(S, cnt, dc=True, iq=True) -> np.ndarray:
    """float64[..., 4]: how far two evaluations of the ten fp64 operations and the rounding to fp32 may lie apart when every fp64
    operation of either is good to one unit in the last place (u = 2^-52 relative; IEEE gives half of that, and then the two agree
    exactly).  First-order propagation along the definition, on the model's own values:
        d mI  = u |mI|                                   d cII = u (|S_II / cnt| + 3 mI^2 + |cII|)     (cQQ, cIQ alike)
        d r   = (d cIQ + |r| d cII) / |cII| + u |r|      d q   = (d cQQ + |q| d cII) / |cII| + u |q|
        d e   = d q + 2 |r| d r + u r^2 + u |e|          d b   = b (d e / (2 e) + 2 u)          d a = b d r + |r| d b + u |a|
    and for each parameter p with fp64 distance d:  d + 2^-23 (|p| + d), the two roundings to fp32.  Where the guard holds a and b are
    the constants 0 and 1 and their bound is 0: the guard's comparisons must fall alike."""
    u = 2.0 ** -52
    est = estimates(S, cnt)
    with np.errstate(all="ignore"):
        dm = [u * np.abs(est["mI"]), u * np.abs(est["mQ"])]
        dII = u * (np.abs(est["eII"]) + 3.0 * est["mI"] ** 2 + np.abs(est["cII"]))
        dQQ = u * (np.abs(est["eQQ"]) + 3.0 * est["mQ"] ** 2 + np.abs(est["cQQ"]))
        dIQ = u * (np.abs(est["eIQ"]) + 3.0 * np.abs(est["mI"] * est["mQ"]) + np.abs(est["cIQ"]))
        r, q, e = est["r"], est["q"], est["e"]
        dr = (dIQ + np.abs(r) * dII) / np.abs(est["cII"]) + u * np.abs(r)
        dq = (dQQ + np.abs(q) * dII) / np.abs(est["cII"]) + u * np.abs(q)
        de = dq + 2.0 * np.abs(r) * dr + u * r * r + u * np.abs(e)
        db = est["b"] * (de / (2.0 * e) + 2.0 * u)
        da = est["b"] * dr + np.abs(r) * db + u * np.abs(est["a"])
    da, db = np.where(est["guarded"], 0.0, da), np.where(est["guarded"], 0.0, db)
    vals = [est["mI"], est["mQ"], est["a"], est["b"]]
    on = [dc, dc, iq, iq]
    out = np.zeros(np.shape(est["mI"]) + (4,), dtype=np.float64)
    for i, (v, d) in enumerate(zip(vals, dm + [da, db])):
        if on[i]:
            out[..., i] = d + 2.0 ** -23 * (np.abs(v) + d)
    return out


def apply(x, params) -> np.ndarray:
    """The three fp32 operations on complex64 items x with parameters broadcastable to x.shape + (4,)."""
    x = np.asarray(x, dtype=np.complex64)
    p = np.asarray(params, dtype=np.float32)
    zI = x.real - p[..., 0]
    u = x.imag - p[..., 1]
    zQ = (p[..., 2] * zI) + (p[..., 3] * u)
    y = np.empty(x.shape, dtype=np.complex64)
    y.real, y.imag = zI, zQ
    return y


def condition(x, block=DEFAULT_BLOCK, window=DEFAULT_WINDOW, dc=True, iq=True):
    """-> (y complex64[len(x)], moments float64[n_blocks, 5], params float32[n_blocks, 4]) of the whole stream x (complex64, or
    anything that converts to it), the items behind the last complete block included (what flush emits)."""
    B, W = check(block, window)
    x = np.ascontiguousarray(x, dtype=np.complex64)
    mom = block_moments(x, B)
    nb = mom.shape[0]
    S, nw = window_sums(mom, W)
    par = parameters(S, nw * float(B), dc, iq) if nb else np.zeros((0, 4), dtype=np.float32)
    y = np.empty(x.size, dtype=np.complex64)
    if nb:
        y[:nb * B] = apply(x[:nb * B].reshape(nb, B), par[:, None, :]).reshape(-1)
    y[nb * B:] = apply(x[nb * B:], par[-1] if nb else np.array(IDENTITY, dtype=np.float32))
    return y, mom, par


def estimate(S, cnt) -> dict:
    """What a window says about the front end: DC level in dBFS (|d| against full scale 1.0), gain mismatch in dB and phase
    mismatch in degrees (g = sqrt(q), phi = asin(r / sqrt(q))), with the complex offset itself."""
    est = estimates(np.asarray(S, dtype=np.float64), cnt)
    return mismatch(est["mI"], est["mQ"], est["r"], est["q"])


def mismatch(mI, mQ, r, q) -> dict:
    """The same from the fp64 estimates of a block (what the device reports beside its parameters).  Where the guard of the
    definition holds (r, q not finite, or q - r r <= 2^-12) the mismatch reads as none."""
    d = complex(float(mI), float(mQ))
    r, q = float(r), float(q)
    if not (np.isfinite(r) and np.isfinite(q) and q - r * r > E_MIN):
        g, phi = 1.0, 0.0
    else:
        g = float(np.sqrt(q))
        phi = float(np.degrees(np.arcsin(np.clip(r / g, -1.0, 1.0))))
    return dict(dc=d, dc_dbfs=float(20.0 * np.log10(abs(d))) if abs(d) > 0.0 else float("-inf"), gain_db=float(20.0 * np.log10(g)), phase_deg=phi)


def impair(x, gain_db=0.0, phase_deg=0.0, dc=0.0):
    """y = I + j g (Q cos phi + I sin phi) + d, in float64 (complex128 out): the direct-conversion front end the stage undoes."""
    x = np.asarray(x, dtype=np.complex128)
    g, phi = 10.0 ** (gain_db / 20.0), np.radians(phase_deg)
    return x.real + 1j * g * (x.imag * np.cos(phi) + x.real * np.sin(phi)) + complex(dc)
