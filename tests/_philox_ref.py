"""The samplers' random numbers from first principles, in numpy, as include/s2s_hip.h states them (s2s_predict_chunks,
first_global_chunk): a vectorised Philox4x32-10 (Salmon et al. 2011), the counter layout {chunk low word, chunk high word,
position | kind << 16, draw index} under the key {seed low word, seed high word}, the Box-Muller normal in float64 and a
restatement of the Gamma sampler (Marsaglia-Tsang 2000 with the alpha < 1 boost, torch._standard_gamma's form) on the same words.
Shared by tests/test_philox_ref_cpu.py and tests/test_gpu_sampler_counters.py."""
import numpy as np

KIND_GAMMA, KIND_DWELL, KIND_NOISE = 1, 2, 3
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK, _32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counter words c0..c3 and key words k0, k1 (anything that broadcasts, values below 2^32) -> the four output words, uint64
    arrays holding 32-bit values.  Ten rounds; the key is bumped by the Weyl constants after each."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3, k0, k1)))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                           # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def words(chunk, position, kind, draw, seed):
    """The four words of the draw (chunk, position, kind, draw index) under `seed`: chunk an unsigned 64-bit chunk index (Python
    ints or an array of them), position < 2^16."""
    chunk = np.asarray(chunk, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c2 = np.asarray(position, dtype=np.uint64) | np.uint64(kind << 16)
    return philox4x32_10(chunk & _MASK, chunk >> _32, c2, draw, seed & 0xFFFFFFFF, seed >> 32)


def u01_open0(x, dtype=np.float64):
    """((x >> 8) + 1) * 2^-24, in (0, 1]: exact in float32."""
    return ((np.asarray(x, np.uint64) >> np.uint64(8)) + np.uint64(1)).astype(dtype) * dtype(2.0 ** -24)


def u01_open1(x, dtype=np.float64):
    """(x >> 8) * 2^-24, in [0, 1): exact in float32."""
    return (np.asarray(x, np.uint64) >> np.uint64(8)).astype(dtype) * dtype(2.0 ** -24)


def normal(x, y, dtype=np.float64):
    """sqrt(-2 ln u1) * cos(2 pi u2), u1 = u01_open0(x), u2 = u01_open1(y), every step in `dtype`."""
    r = np.sqrt(dtype(-2.0) * np.log(u01_open0(x, dtype)))
    return r * np.cos(dtype(2.0 * np.pi) * u01_open1(y, dtype))


def ref_normal(chunk, position, kind, seed):
    """The float64 standard normal of (chunk, position, kind, draw 0)."""
    x, y, _, _ = words(chunk, position, kind, 0, seed)
    return normal(x, y)


def ref_standard_gamma(alpha, chunk, position, seed, dtype=np.float64, max_iter=256):
    """Gamma(alpha, 1) draws on the words of (chunk, position, kind 1, draw 0, 1, ...), every floating-point step in `dtype`:
    alpha == 0 gives 0; alpha < 1 spends draw 0 on the boost (1 - u01_open1(x)) ** (1 / alpha) and goes on with alpha + 1; then per
    trip of the rejection loop one draw: x = normal(words x, y), y = 1 + c x, rejected if y <= 0, v = y^3, u = 1 - u01_open1(words z),
    accepted if u < 1 - 0.0331 x^4 or ln u < x^2 / 2 + d (1 - v + ln v); the result is boost * d * v with d = alpha - 1/3,
    c = 1 / sqrt(9 d).  alpha, chunk and position broadcast."""
    f = dtype
    alpha, chunk, position = np.broadcast_arrays(np.asarray(alpha, f), np.asarray(chunk, np.uint64), np.asarray(position, np.uint64))
    alpha = alpha.copy()
    zero, small = alpha == 0, alpha < 1
    draw = np.zeros(alpha.shape, np.uint64)
    with np.errstate(all="ignore"):
        x, _, _, _ = words(chunk, position, KIND_GAMMA, draw, seed)
        boost = np.where(small, np.power(f(1) - u01_open1(x, f), f(1) / np.where(zero, f(1), alpha)), f(1)).astype(f)
        alpha = np.where(small, alpha + f(1), alpha).astype(f)
        draw += small.astype(np.uint64)
        d = alpha - f(1) / f(3)
        c = f(1) / np.sqrt(f(9) * d)
        v = np.ones(alpha.shape, f)
        active = ~zero
        for _ in range(max_iter):
            if not active.any():
                break
            wx, wy, wz, _ = words(chunk, position, KIND_GAMMA, draw, seed)
            draw += active.astype(np.uint64)
            x = normal(wx, wy, f)
            y = f(1) + c * x
            ok = active & (y > 0)
            vv = y * y * y
            v = np.where(ok, vv, v)
            u = f(1) - u01_open1(wz, f)
            xx = x * x
            accept = ok & ((u < f(1) - f(0.0331) * xx * xx) | (np.log(u) < f(0.5) * xx + d * (f(1) - vv + np.log(vv))))
            active &= ~accept
        out = np.where(zero, f(0), boost * d * v)
    assert out.dtype == f
    return out


def dwell_of_gamma(s, rate, min_duration=0.0):
    """The clamps behind the sampler: Gamma.sample's / rate and clamp at the smallest normal float32, the model's clamp at 1, the
    command's min_duration."""
    g = np.maximum(np.asarray(s, np.float64) / np.asarray(rate, np.float64), float(np.finfo(np.float32).tiny))
    return np.maximum(np.maximum(g, 1.0), min_duration)


def agreement(got, ref, rel=1e-3):
    """Among the draws whose reference exceeds 1 (the others are clamped to 1): -> (the share within `rel` relative, their number)."""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    m = ref > 1.0
    return float((np.abs(got[m] - ref[m]) <= rel * ref[m]).mean()), int(m.sum())
