"""NumPy checker of ``fg_obs_noise_add`` (``fluidgym_amd/csrc/fg_obsnoise.hip``): Philox4x32-10 in ``uint64``
arithmetic, the fp32 arithmetic that turns its words into normal numbers restated operation for operation in ``np.float32`` (every
operation rounded on its own, as the kernel's translation unit is compiled), and the launch itself on host arrays.  The kernel is
held to these bits."""
import numpy as np

F = np.float32
_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LOW, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)

# the edge words of the uniform and of the angle: both ends of the 9 dropped bits, of every quadrant and of the half-quadrant fold
EDGE_WORDS = np.array([0, 0x1ff, 0x200, 0x3fffffff, 0x40000000, 0x7fffffff, 0x80000000, 0xbfffffff, 0xc0000000, 0xfffffe00, 0xffffffff],
                      dtype=np.uint32)


def philox4x32_10(counter, key):
    """``counter``: four broadcastable unsigned arrays, ``key``: two; returns the four output words as ``uint32`` arrays."""
    c = [np.asarray(x).astype(np.uint64) & _LOW for x in np.broadcast_arrays(*counter)]
    k = [np.asarray(x).astype(np.uint64) & _LOW for x in key]
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k[0], p1 & _LOW, (p0 >> _S32) ^ c[3] ^ k[1], p0 & _LOW]
        k = [(k[0] + _W0) & _LOW, (k[1] + _W1) & _LOW]
    return [x.astype(np.uint32) for x in c]


def normal_pair(w0, w1):
    """Two fp32 normal numbers of two ``uint32`` word arrays: the definition at the top of ``fg_obsnoise.hip``, in its order."""
    w0, w1 = np.asarray(w0, dtype=np.uint32), np.asarray(w1, dtype=np.uint32)
    u = ((w0 >> np.uint32(9)).astype(F) + F(0.5)) * F(2.0 ** -23)
    b = u.view(np.uint32)
    e = (b >> np.uint32(23)).astype(np.int32) - np.int32(127)
    m = ((b & np.uint32(0x007fffff)) | np.uint32(0x3f800000)).view(F)
    big = m > F(1.41421354)
    m = np.where(big, m * F(0.5), m)
    e = np.where(big, e + np.int32(1), e)
    t = (m - F(1.0)) / (m + F(1.0))
    t2 = t * t
    p = F(1.0 / 9.0) * t2 + F(1.0 / 7.0)
    p = p * t2 + F(1.0 / 5.0)
    p = p * t2 + F(1.0 / 3.0)
    p = p * t2 + F(1.0)
    ln_u = e.astype(F) * F(0.693147182) + (F(2.0) * t) * p
    r = np.sqrt(F(-2.0) * ln_u)

    q = w1 >> np.uint32(30)
    f = (((w1 >> np.uint32(9)) & np.uint32(0x1fffff)).astype(F) + F(0.5)) * F(2.0 ** -21)
    swap = f > F(0.5)
    f = np.where(swap, F(1.0) - f, f)
    a = f * F(1.57079637)
    a2 = a * a
    sn = F(1.0 / 362880.0) * a2 + F(-1.0 / 5040.0)
    sn = sn * a2 + F(1.0 / 120.0)
    sn = sn * a2 + F(-1.0 / 6.0)
    sn = sn * a2 + F(1.0)
    sn = sn * a
    cs = F(-1.0 / 3628800.0) * a2 + F(1.0 / 40320.0)
    cs = cs * a2 + F(-1.0 / 720.0)
    cs = cs * a2 + F(1.0 / 24.0)
    cs = cs * a2 + F(-0.5)
    cs = cs * a2 + F(1.0)
    c, s = np.where(swap, sn, cs), np.where(swap, cs, sn)
    cr = np.select([q == 0, q == 1, q == 2], [c, -s, -c], s)
    sr = np.select([q == 0, q == 1, q == 2], [s, c, -s], -c)
    z0, z1 = r * cr, r * sr
    assert z0.dtype == F and z1.dtype == F
    return z0, z1


def box_muller_f64(w0, w1):
    """fp64 Box-Muller of the same words with the library's log, cos and sin: what ``normal_pair`` approximates."""
    w0, w1 = np.asarray(w0, dtype=np.uint32), np.asarray(w1, dtype=np.uint32)
    u = ((w0 >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    r = np.sqrt(-2.0 * np.log(u))
    theta = 2.0 * np.pi * ((w1 >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    return r * np.cos(theta), r * np.sin(theta)


def normals(n, tag, row_id, episode, step, seed):
    """The ``n`` fp32 normal numbers of one row of one segment."""
    quads = (int(n) + 3) // 4
    word0 = (np.uint64(int(tag)) << np.uint64(24)) | np.arange(quads, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10((word0, np.uint64(int(row_id) & 0xFFFFFFFF), np.uint64(int(episode) & 0xFFFFFFFF), np.uint64(int(step) & 0xFFFFFFFF)),
                      (np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)))
    z0, z1 = normal_pair(w[0], w[1])
    z2, z3 = normal_pair(w[2], w[3])
    return np.stack([z0, z1, z2, z3], axis=1).reshape(-1)[: int(n)]


def add_noise(src, sigma, z, dtype):
    """``src + sigma z`` as the kernel forms it: ``dtype`` 0 in fp32 with ``(float)sigma``, 1 in fp64 with ``(double)z``."""
    with np.errstate(invalid="ignore"):
        if dtype == 0:
            return np.asarray(src, dtype=F) + F(sigma) * z
        return np.asarray(src, dtype=np.float64) + np.float64(sigma) * z.astype(np.float64)


def noise_add(segments, rows, counters, row_ids, seed, dtype):
    """The launch on host arrays.  ``segments``: dicts with ``src`` (``[rows, n]``, already without its stride padding), ``tag`` and
    ``sigma``; ``counters``: ``[rows, 2]`` = (episode, step); ``row_ids``: ``[rows]`` or None (row r is r).  Returns one ``[rows, n]``
    array per segment."""
    counters = np.asarray(counters).reshape(rows, 2)
    out = []
    for seg in segments:
        src = np.asarray(seg["src"]).reshape(rows, -1)
        res = np.empty(src.shape, dtype=F if dtype == 0 else np.float64)
        for r in range(rows):
            rid = r if row_ids is None else int(row_ids[r])
            z = normals(src.shape[1], seg["tag"], rid, counters[r, 0], counters[r, 1], seed)
            res[r] = add_noise(src[r], seg["sigma"], z, dtype)
        out.append(res)
    return out
