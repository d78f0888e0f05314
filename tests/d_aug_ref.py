"""Restatement of the random generator and the two kernels of csrc/d_aug.hip (jg_d_aug, jg_apa_update) in numpy, test helper.

Generator: Philox4x32-10 (Salmon et al., SC'11; the Random123 known answers are in tests/test_d_aug_host.py), integer arithmetic exact;
uniforms u = ((x >> 9) + 0.5) * 2^-23 in the open interval (0, 1); normals by Box-Muller, here in float64 on the same uniforms:
(sqrt(-2 ln u0) cos(2 pi u1), sqrt(-2 ln u0) sin(2 pi u1)).
Counter layout: noise   (pixel h * W + w,  sample b,  stream | (c // 4) << 16,  call): the 4 words are the normals of channels 4 (c // 4) .. + 3
                flags   (0,  sample b,  stream of the target,  call): word 0 is the uniform compared with p
jg_d_aug in float64 on the caller's 16-bit values; jg_apa_update in float32, every operation in the reference's order."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
NOISE_STREAM = 0


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of one shape, key: 2 ints -> 4 uint32 arrays"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [v.astype(np.uint32) for v in c]


def uniform_open(x):
    """float64 value of the kernel's fp32 uniform (exact: 23 bits + the half)"""
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def key_words(key):
    """the two unsigned 32-bit words of an int32 key tensor / sequence"""
    return [int(v) & MASK for v in np.asarray(key).reshape(-1)[:2]]


def normals(key, B, C, H, W, stream=NOISE_STREAM, call=0):
    """float64 [B, C, H, W]: the noise jg_d_aug draws for this key / stream / call"""
    q = (C + 3) // 4
    pix = np.arange(H * W, dtype=np.uint64)[None, None, :]
    b = np.arange(B, dtype=np.uint64)[:, None, None]
    grp = np.arange(q, dtype=np.uint64)[None, :, None]
    r = philox4x32_10((pix, b, np.uint64(stream) | (grp << np.uint64(16)), np.uint64(call)), key_words(key))      # 4 x [B, q, HW]
    u = [uniform_open(w) for w in r]
    out = np.empty((B, q, 4, H * W))
    for j in (0, 1):
        rad, ang = np.sqrt(-2.0 * np.log(u[2 * j])), 2.0 * np.pi * u[2 * j + 1]
        out[:, :, 2 * j], out[:, :, 2 * j + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return out.reshape(B, 4 * q, H, W)[:, :C]


def flag_uniforms(key, B, stream, call=0):
    """float64 [B]: the uniforms of the flags of the target that draws on `stream`"""
    r = philox4x32_10((np.uint64(0), np.arange(B, dtype=np.uint64), np.uint64(stream), np.uint64(call)), key_words(key))
    return uniform_open(r[0])


def d_aug(src, C, sigma=0.0, z=None, alt=None, u=None, p=None):
    """one target of jg_d_aug in float64: src / alt [B, H, W, Cpad] (the caller's 16-bit values as float64 arrays), z [B, C, H, W], u [B], p float32
    -> (out float64 [B, H, W, Cpad] BEFORE the rounding to the storage type, flags int32 [B]); flagged rows are alt, padding channels 0"""
    src = np.asarray(src, dtype=np.float64)
    out = np.zeros_like(src)
    out[..., :C] = src[..., :C]
    if sigma != 0.0:
        out[..., :C] += np.float64(np.float32(sigma)) * np.asarray(z, dtype=np.float64).transpose(0, 2, 3, 1)
    flags = np.zeros(src.shape[0], dtype=np.int32)
    if alt is not None:
        flags = (np.asarray(u, dtype=np.float32) < np.float32(p)).astype(np.int32)
        sel = flags.astype(bool)
        out[sel, ..., :C] = np.asarray(alt, dtype=np.float64)[sel][..., :C]
    return out, flags


def apa_update(pred, p, target, num, den):
    """jg_apa_update: pred any array of finite values (every element counts) -> (p, adjust, s) as float32, computed as the reference does:
    s = sum(sign) / n; adjust = sign(s - target); lambda = (adjust * num) / den; p = p + lambda; p < 0: p * 0; p > 1: 1"""
    f = np.float32
    pred = np.asarray(pred)
    n_pos, n_neg = int((pred > 0).sum()), int((pred < 0).sum())
    s = f(n_pos - n_neg) / f(pred.size)
    adjust = f(np.sign(s - f(target)))
    lam = (adjust * f(num)) / f(den)
    pn = f(p) + lam
    if pn < 0:
        pn = pn * f(0.0)
    if pn > 1:
        pn = f(1.0)
    return f(pn), adjust, f(s)
