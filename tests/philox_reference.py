"""Philox4x32-10 (Salmon et al., SC'11) and the counter layout of csrc/philox.h restated in Python: once on plain ints, the form
the Random123 known-answer vectors are checked in, and once on NumPy arrays, for the tests that restate a whole kernel's draws.
A helper module, not a test."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
KNOWN_ANSWERS = (                       # Random123's kat_vectors, philox4x32 with 10 rounds: (counter, key, result)
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
)
PRED_NOISE_STREAM = 0x505245 << 32      # predictive_kernels.hip: the stream of the noise draw is this | the global cell


def philox(c, k):
    """philox4x32_10 on four counter words and two key words given as Python ints; returns the four result words."""
    c = list(c)
    k = list(k)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return c


def philox_np(c, k):
    """The same on arrays: c four and k two uint64 arrays holding 32-bit words (they broadcast); returns four uint64 arrays."""
    c = [np.asarray(x, dtype=np.uint64) for x in c]
    k = [np.asarray(x, dtype=np.uint64) for x in k]
    mask, s32 = np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                # 32 x 32 bits: no overflow in 64
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & mask, (p0 >> s32) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
    return c


def block_counter(gidx, stream, block):
    """philox_block's counter: (gidx lo, gidx hi, stream lo, stream hi[23:0] << 8 | block), on ints."""
    return [gidx & MASK, (gidx >> 32) & MASK, stream & MASK, (((stream >> 32) << 8) & MASK) | (block & 0xFF)]


def philox_block(seed, gidx, stream, block):
    """philox_block of philox.h on Python ints (64-bit seed, gidx and stream)."""
    return philox(block_counter(gidx, stream, block), [seed & MASK, (seed >> 32) & MASK])


def philox_block_np(seed, gidx, stream, block=0):
    """philox_block on arrays: gidx and stream uint64 arrays (they broadcast), seed and block ints."""
    gidx, stream = np.asarray(gidx, dtype=np.uint64), np.asarray(stream, dtype=np.uint64)
    mask, s32 = np.uint64(MASK), np.uint64(32)
    w = (((stream >> s32) << np.uint64(8)) & mask) | np.uint64(block & 0xFF)
    return philox_np([gidx & mask, gidx >> s32, stream & mask, w], [np.uint64(seed & MASK), np.uint64((seed >> 32) & MASK)])


def u01_from(a, b):
    """u01_from of philox.h: the 53-bit uniform in [0, 1) of two 32-bit words (ints or uint64 arrays)."""
    if isinstance(a, (int, np.integer)) and isinstance(b, (int, np.integer)):
        return float(((int(a) >> 5) << 26) | (int(b) >> 6)) / 9007199254740992.0
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return (((a >> np.uint64(5)) << np.uint64(26)) | (b >> np.uint64(6))).astype(np.float64) * (1.0 / 9007199254740992.0)


def pred_noise_z(seed, global_offset, n, cells):
    """The standard normal draw z[p, cell] of pred_keys_kernel for particles global_offset .. global_offset + n - 1 and the GLOBAL
    cell numbers `cells` (an int array): the block philox_block(seed, global_offset + p, 0x505245 << 32 | cell, 0), then
    u1 = 1 - u01(x, y), u2 = u01(z, w), z = sqrt(-2 ln u1) cos(2 pi u2) with 2 pi as the kernel writes it."""
    g = (np.uint64(global_offset) + np.arange(n, dtype=np.uint64))[:, None]
    stream = np.uint64(PRED_NOISE_STREAM) | np.asarray(cells, dtype=np.uint64)[None, :]
    x, y, z, w = philox_block_np(seed, g, stream, 0)
    u1, u2 = 1.0 - u01_from(x, y), u01_from(z, w)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


# ---- the sampler's own draws (stage_kernels.hip, mm_kernels.hip, meth_smc.hip) ------------------------------------------
# Integer work and the uniforms are exact; what goes through ln, sqrt, cos and sin is evaluated in np.longdouble, on the
# doubles the kernels form (u1, u2 and the rounded product 6.283185307179586 u2), so the restatement is the more precise side.

PRIOR_STREAM = 0xFFFFFFFF00000000       # sample_prior_kernel: | the component
MN_STREAM = 0x5EED << 32                # mn_spacings_kernel's stream, under a key of its own (the bits of wrand)
MN_BLOCK = 7
BLOCK_UNIFORM = 255                     # SMC_PHILOX_BLOCK_UNIFORM: the acceptance uniform


def _gidx(goff, n):
    return np.uint64(goff) + np.arange(n, dtype=np.uint64)


def box_muller(r):
    """The pair (rad cos, rad sin) every normal of the sampler comes from, of one block r = (x, y, z, w): u1 = 1 - u01(x, y) in
    (0, 1], u2 = u01(z, w), rad = sqrt(-2 ln u1), angle = the DOUBLE 6.283185307179586 u2; in np.longdouble."""
    u1 = (1.0 - u01_from(r[0], r[1])).astype(np.longdouble)
    ang = (6.283185307179586 * u01_from(r[2], r[3])).astype(np.longdouble)
    rad = np.sqrt(-2 * np.log(u1))
    return rad * np.cos(ang), rad * np.sin(ang)


def prior_draw(seed, goff, n, kinds, a, b):
    """sample_prior_kernel for particles goff .. goff + n - 1: component c from block 0 of the stream PRIOR_STREAM | c.
    kinds: "uniform" (a = low, b = high) or anything else = drawn as a normal (a = mu, b = sigma).  Returns (x, u): x (n, d) in
    np.longdouble - a + (b - a) u with the width b - a rounded to a double as the kernel forms it, a + b z for a normal - and u
    (n, d), the exact first uniform of every block (what a test needs to round the uniform components itself)."""
    g = _gidx(goff, n)
    d = len(kinds)
    x, u = np.empty((n, d), dtype=np.longdouble), np.empty((n, d))
    for c in range(d):
        r = philox_block_np(seed, g, PRIOR_STREAM | c, 0)
        u[:, c] = u01_from(r[0], r[1])
        if kinds[c] == "uniform":
            x[:, c] = np.longdouble(a[c]) + np.longdouble(np.float64(b[c]) - np.float64(a[c])) * u[:, c].astype(np.longdouble)
        else:
            x[:, c] = np.longdouble(a[c]) + np.longdouble(b[c]) * box_muller(r)[0]
    return x, u


def mm_proposal_normals(seed, goff, n, stream):
    """mm_propose_one: (n, 3) standard normals - cosine and sine of block 0, cosine of block 1."""
    g = _gidx(goff, n)
    c0, s0 = box_muller(philox_block_np(seed, g, stream, 0))
    c1, _ = box_muller(philox_block_np(seed, g, stream, 1))
    return np.stack([c0, s0, c1], axis=1)


def generic_proposal_normals(seed, goff, n, stream, d):
    """generic_propose_kernel: (n, d) standard normals - block b gives components 2 b (cosine) and 2 b + 1 (sine); for an odd d
    the last sine is not used."""
    g = _gidx(goff, n)
    out = np.empty((n, d), dtype=np.longdouble)
    for blk in range((d + 1) // 2):
        cs, sn = box_muller(philox_block_np(seed, g, stream, blk))
        out[:, 2 * blk] = cs
        if 2 * blk + 1 < d:
            out[:, 2 * blk + 1] = sn
    return out


def accept_uniform(seed, goff, n, stream):
    """The acceptance uniform rr of particles goff .. goff + n - 1: u01 of the first two words of block 255.  Exact."""
    r = philox_block_np(seed, _gidx(goff, n), stream, BLOCK_UNIFORM)
    return u01_from(r[0], r[1])


def multinomial_thresholds(wrand, N):
    """mn_spacings_kernel + mn_thresholds_kernel: the key is the 64 bits of the double wrand = u / N; item i = 0 .. N (N + 1
    spacings) draws block 7 of the stream 0x5EED << 32 and gives e_i = -ln(1 - u01); the thresholds are the first N partial sums
    divided by the sum of all N + 1.  np.longdouble, sorted by construction."""
    seed = int(np.array([wrand], dtype=np.float64).view(np.uint64)[0])
    r = philox_block_np(seed, np.arange(N + 1, dtype=np.uint64), MN_STREAM, MN_BLOCK)
    e = -np.log((1.0 - u01_from(r[0], r[1])).astype(np.longdouble))
    c = np.cumsum(e)
    return c[:N] / c[N]
