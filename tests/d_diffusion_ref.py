"""float64 restatement of the three dataaug_D_diffusion kernels (csrc/d_diffusion.hip), the yardstick of tests/test_d_diffusion_host.py (against
the fixtures recorded from the reference) and of tests/test_gpu_15_d_diffusion.py (against the kernels).  numpy only."""
import numpy as np

T_MIN, T_MAX, EPL, EPL_MAX, TABLE = 5, 500, 64, 48, 501


def update_p(p, loss, batch_times_every):
    """loss.py:321-330, every step in float32 in the reference's order; `loss` a float32 value"""
    f = np.float32
    d = f(loss) - f(0.9)
    adj = f(np.sign(d)) if d == d else f(0.0)
    pn = f(p) + f(adj * f(batch_times_every)) / f(100 * 1000)
    return f(min(max(pn, f(0.0)), f(1.0)))


def T_n(p):
    """diffusion.py:126-127,132: products in float32, round half to even"""
    p = np.float32(p)
    T = int(np.clip(T_MIN + int(np.rint(np.float32(p * np.float32(T_MAX - T_MIN)))), T_MIN, T_MAX))
    n = min(int(np.rint(np.float32(p * np.float32(EPL)))), EPL_MAX)
    return T, n


def tables(T):
    """a = sqrt(cumprod(alphas)) and b = sqrt(1 - cumprod(alphas)) with a leading 1, [TABLE] float64 each (0 beyond T): betas =
    float32(linspace_float64(1e-4, 1e-2, T)), alphas = 1 - betas in float32, the cumulative product in float64"""
    betas = np.linspace(1e-4, 1e-2, T, dtype=np.float64).astype(np.float32)
    alphas = (np.float32(1.0) - betas).astype(np.float64)
    cp = np.concatenate(([1.0], np.cumprod(alphas)))
    a, b = np.zeros(TABLE), np.zeros(TABLE)
    a[:T + 1], b[:T + 1] = np.sqrt(cp), np.sqrt(1.0 - cp)
    return a, b


def inverse_cdf(u, T):
    """value k + 1 for the smallest integer k >= 1 with k (k + 1) >= u T (T - 1): the inverse CDF of prob_t = arange(T) / sum(arange(T)) over
    the values 1 .. T (diffusion.py:133-136).  The kernel's u are float32 values (at most 24 significant bits): their products are exact in float64"""
    w = np.asarray(u, dtype=np.float64) * float(T * (T - 1))
    k = np.arange(1, T, dtype=np.float64)
    idx = np.searchsorted(k * (k + 1.0), w, side="left")      # the first k (k + 1) >= w
    return (np.minimum(idx, T - 2) + 2).astype(np.int64)      # k = idx + 1, value k + 1


def t_epl(u, T, n):
    out = np.zeros(EPL, dtype=np.int64)
    out[:n] = inverse_cdf(np.asarray(u)[:n], T)
    return out


def update(p, loss, batch_times_every, u):
    """jg_d_diffusion_update: -> (p float32, T, n, a, b, t_epl)"""
    p = update_p(p, loss, batch_times_every)
    T, n = T_n(p)
    a, b = tables(T)
    return p, T, n, a, b, t_epl(u, T, n)


def q_sample(x, a, b, t, z, noise_std):
    """jg_d_diffusion on one map: x, z [B, C, H, W], t [B, C] -> a[t] x + (noise_std b[t]) z in float64; a channel with b[t] == 0 is a[t] x"""
    x, z = np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64)
    t = np.asarray(t, dtype=np.int64)
    at, bt = np.asarray(a, dtype=np.float64)[t][:, :, None, None], float(noise_std) * np.asarray(b, dtype=np.float64)[t][:, :, None, None]
    return at * x + np.where(bt != 0.0, bt * z, 0.0)


def q_sample_bwd(dy, a, t):
    return np.asarray(a, dtype=np.float64)[np.asarray(t, dtype=np.int64)][:, :, None, None] * np.asarray(dy, dtype=np.float64)
