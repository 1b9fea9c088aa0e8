"""NumPy float32 restatement of the ray marcher of ``csrc/fg_render3d.hip``: both modes and the ray generation,
every operation rounded on its own in the order the kernel's head comment writes.  The contract with the kernel is equality, bytes and
depth.  Vectorised over the pixels of a frame (flattened), a Python loop over the samples."""
import numpy as np

f32 = np.float32
MAX_SAMPLES = f32(65535.0)
ALPHA_CUTOFF = f32(0.99)
AMBIENT, DIFFUSE = f32(0.35), f32(0.65)


def lerp(a, b, f):
    return a + f * (b - a)


def scalar_field(field: np.ndarray, channel: int) -> np.ndarray:
    """``[nz, ny, nx]`` of a field ``[C, nz, ny, nx]``: one channel, or ``sqrt(((u0 u0) + (u1 u1)) + (u2 u2))``."""
    field = np.asarray(field, dtype=f32)
    if channel >= 0:
        return field[channel]
    s = field[0] * field[0]
    for k in range(1, field.shape[0]):
        s = s + field[k] * field[k]
    return np.sqrt(s)


def rays(cam: np.ndarray, H: int, W: int):
    """Origins and directions ``[3][H W]`` of the pixels of a camera ``[6, 3]`` float32 (``o0, ou, ov, d0, du, dv``)."""
    cam = np.asarray(cam, dtype=f32)
    pj = (np.arange(W, dtype=f32) + f32(0.5))[None, :]
    pi = (np.arange(H, dtype=f32) + f32(0.5))[:, None]
    o = [((cam[0, k] + pj * cam[1, k]) + pi * cam[2, k]).reshape(-1) for k in range(3)]
    d = [((cam[3, k] + pj * cam[4, k]) + pi * cam[5, k]).reshape(-1) for k in range(3)]
    return o, d


def slabs(o, d, shape, step):
    """``tmin`` and the number of samples (0 for a miss) of every ray against the box of a volume ``shape = (nz, ny, nx)``."""
    nz, ny, nx = shape
    tmin = np.zeros_like(o[0])
    tmax = np.full_like(o[0], np.inf)
    miss = np.zeros(o[0].shape, dtype=bool)
    for k, n in enumerate((nx, ny, nz)):
        top = f32(n - 1)
        par = d[k] == 0
        miss |= par & ((o[k] < 0) | (o[k] > top))
        t1, t2 = (f32(0) - o[k]) / d[k], (top - o[k]) / d[k]
        tn, tf = np.where(t1 < t2, t1, t2), np.where(t1 < t2, t2, t1)
        tmin = np.where(~par & (tn > tmin), tn, tmin)
        tmax = np.where(~par & (tf < tmax), tf, tmax)
    miss |= ~(tmin <= tmax)
    nf = np.floor((tmax - tmin) / f32(step))
    nf = np.where(nf <= MAX_SAMPLES, nf, MAX_SAMPLES)
    ns = np.where(miss, 0, np.where(miss, f32(0), nf).astype(np.int64) + 1)
    return tmin.astype(f32), ns


def locate(p, shape):
    """Corner indices ``(iz, iy, ix)`` and fractions ``(fx, fy, fz)`` of the cells of the points ``p = [px, py, pz]``."""
    nz, ny, nx = shape
    idx, frac = [], []
    for pk, n in zip(p, (nx, ny, nz)):
        c = np.floor(pk)
        c = np.where(c < 0, f32(0), c)
        c = np.where(c > f32(n - 2), f32(n - 2), c)
        frac.append(pk - c)
        idx.append(c.astype(np.int64))
    return (idx[2], idx[1], idx[0]), frac


def corners(S, idx):
    iz, iy, ix = idx
    return [S[iz + (k >> 2), iy + ((k >> 1) & 1), ix + (k & 1)] for k in range(8)]


def cell_value(v, frac):
    fx, fy, fz = frac
    c00, c01 = lerp(v[0], v[1], fx), lerp(v[2], v[3], fx)
    c10, c11 = lerp(v[4], v[5], fx), lerp(v[6], v[7], fx)
    return lerp(lerp(c00, c01, fy), lerp(c10, c11, fy), fz)


def cell_gradient(v, frac):
    fx, fy, fz = frac
    gx = lerp(lerp(v[1] - v[0], v[3] - v[2], fy), lerp(v[5] - v[4], v[7] - v[6], fy), fz)
    gy = lerp(lerp(v[2] - v[0], v[3] - v[1], fx), lerp(v[6] - v[4], v[7] - v[5], fx), fz)
    gz = lerp(lerp(v[4] - v[0], v[5] - v[1], fx), lerp(v[6] - v[2], v[7] - v[3], fx), fy)
    return gx, gy, gz


def crosses(u, w):
    return ((u < 0) & (w >= 0)) | ((u >= 0) & (w < 0))


def secant(u, w, tp, t):
    q = u / (u - w)
    q = np.where((q >= 0) & (q <= 1), q, f32(0.5))
    return tp + q * (t - tp)


def table_bin(v, lo, span):
    """The bin of the colour table, -1 for a NaN (the rule of ``fg_frame_colorize``)."""
    x = (v - f32(lo)) / f32(span)
    x = np.where(x < 0, f32(0), x)
    x = np.where(x > 1, f32(1), x)
    nan = x != x
    idx = np.minimum((np.where(nan, f32(0), x) * f32(256.0)).astype(np.int64), 255)
    return np.where(nan, -1, idx)


def to_byte(q):
    q = np.floor(q)
    q = np.where(q < 0, f32(0), q)
    q = np.where(q > 255, f32(255), q)
    return q.astype(np.uint8)


def cell_trunc(h, n):
    k = np.where(h < 0, f32(0), h)
    k = np.where(k > f32(n - 1), f32(n - 1), k)
    return k.astype(np.int64)


def isosurface(vol, channel, level, cvol, cchannel, lo_span, table, cam, H, W, step, clip=None, solid=None, body=(128, 128, 128),
               background=(255, 255, 255), envs=None, ambient=AMBIENT, diffuse=DIFFUSE, return_normal=False):
    """``fg_render_isosurface``: ``vol [B, C, nz, ny, nx]``, ``level [n]`` and ``lo_span [n, 2]`` per listed env -> frames ``uint8
    [n, H, W, 3]`` and depth float32 ``[n, H, W]`` (and, asked for, the gradient ``[n, H, W, 3]`` at the hits, NaN elsewhere)."""
    vol, cvol, table = np.asarray(vol, dtype=f32), np.asarray(cvol, dtype=f32), np.asarray(table, dtype=np.uint8)
    envs = list(range(vol.shape[0])) if envs is None else [int(e) for e in envs]
    shape = vol.shape[2:]
    nz, ny, nx = shape
    step, ambient, diffuse = f32(step), f32(ambient), f32(diffuse)
    M = None if solid is None else (np.asarray(solid) != 0).astype(f32)
    frames = np.empty((len(envs), H * W, 3), dtype=np.uint8)
    depths = np.empty((len(envs), H * W), dtype=f32)
    normals = np.full((len(envs), H * W, 3), np.nan, dtype=f32)
    with np.errstate(all="ignore"):
        o, d = rays(cam, H, W)
        tmin, ns = slabs(o, d, shape, step)
        P = o[0].size
        for n, e in enumerate(envs):
            S, Cs, lev = np.abs(scalar_field(vol[e], channel)), scalar_field(cvol[e], cchannel), f32(level[n])
            kind = np.zeros(P, dtype=np.int64)
            t_hit = np.full(P, np.inf, dtype=f32)
            gp, mp, tp = np.zeros(P, f32), np.zeros(P, f32), np.zeros(P, f32)
            inp = np.zeros(P, dtype=bool)
            for s in range(int(ns.max()) if P else 0):
                act = np.nonzero((s < ns) & (kind == 0))[0]
                if act.size == 0:
                    break
                t = tmin[act] + f32(s) * step
                p = [o[k][act] + t * d[k][act] for k in range(3)]
                inc = np.ones(act.size, dtype=bool)
                if clip is not None:
                    for k in range(3):
                        inc &= (p[k] >= f32(clip[0][k])) & (p[k] <= f32(clip[1][k]))
                idx, frac = locate(p, shape)
                gc = np.where(inc, cell_value(corners(S, idx), frac) - lev, f32(0))
                mc = np.zeros(act.size, f32) if M is None else cell_value(corners(M, idx), frac) - f32(0.5)
                if s > 0:
                    hi = inp[act] & inc & crosses(gp[act], gc)
                    hs = crosses(mp[act], mc) if M is not None else np.zeros(act.size, dtype=bool)
                    ti, ts = secant(gp[act], gc, tp[act], t), secant(mp[act], mc, tp[act], t)
                    first = hi & (~hs | (ti <= ts))
                    second = hs & ~first
                    kind[act] = np.where(first, 1, np.where(second, 2, 0))
                    t_hit[act] = np.where(first, ti, np.where(second, ts, t_hit[act]))
                gp[act], mp[act], tp[act], inp[act] = gc, mc, t, inc
            rgb = np.tile(np.asarray(background, dtype=np.uint8), (P, 1))
            for which, field in ((1, S), (2, M)):
                hit = np.nonzero(kind == which)[0]
                if hit.size == 0:
                    continue
                dh = [d[k][hit] for k in range(3)]
                h = [o[k][hit] + t_hit[hit] * dh[k] for k in range(3)]
                idx, frac = locate(h, shape)
                gx, gy, gz = cell_gradient(corners(field, idx), frac)
                if which == 1:
                    b = table_bin(Cs[cell_trunc(h[2], nz), cell_trunc(h[1], ny), cell_trunc(h[0], nx)], *lo_span[n])
                    base = np.where((b < 0)[:, None], np.uint8(0), table[np.maximum(b, 0)])
                else:
                    base = np.tile(np.asarray(body, dtype=np.uint8), (hit.size, 1))
                nd = (gx * dh[0] + gy * dh[1]) + gz * dh[2]
                nn = np.sqrt((gx * gx + gy * gy) + gz * gz)
                dd = np.sqrt((dh[0] * dh[0] + dh[1] * dh[1]) + dh[2] * dh[2])
                cs = np.abs(nd) / (nn * dd)
                cs = np.where(cs >= 0, cs, f32(0))
                cs = np.where(cs > 1, f32(1), cs)
                shade = ambient + diffuse * cs
                rgb[hit] = to_byte(base.astype(f32) * shade[:, None] + f32(0.5))
                normals[n, hit] = np.stack([gx, gy, gz], axis=1)
            frames[n], depths[n] = rgb, t_hit
    out = (frames.reshape(len(envs), H, W, 3), depths.reshape(len(envs), H, W))
    return out + (normals.reshape(len(envs), H, W, 3),) if return_normal else out


def volume(vol, channel, lo_span, table, opacity, cam, H, W, step, background=(255, 255, 255), envs=None, return_alpha=False):
    """``fg_render_volume``: frames ``uint8 [n, H, W, 3]`` (and, asked for, the accumulated opacity ``[n, H, W]``)."""
    vol, table, opacity = np.asarray(vol, dtype=f32), np.asarray(table, dtype=np.uint8), np.asarray(opacity, dtype=f32)
    envs = list(range(vol.shape[0])) if envs is None else [int(e) for e in envs]
    shape = vol.shape[2:]
    step = f32(step)
    bg = np.asarray(background, dtype=np.uint8).astype(f32)
    frames = np.empty((len(envs), H * W, 3), dtype=np.uint8)
    alphas = np.zeros((len(envs), H * W), dtype=f32)
    with np.errstate(all="ignore"):
        o, d = rays(cam, H, W)
        tmin, ns = slabs(o, d, shape, step)
        P = o[0].size
        for n, e in enumerate(envs):
            S = scalar_field(vol[e], channel)
            A, C = np.zeros(P, f32), np.zeros((P, 3), f32)
            done = np.zeros(P, dtype=bool)
            for s in range(int(ns.max()) if P else 0):
                act = np.nonzero((s < ns) & ~done)[0]
                if act.size == 0:
                    break
                t = tmin[act] + f32(s) * step
                idx, frac = locate([o[k][act] + t * d[k][act] for k in range(3)], shape)
                b = table_bin(cell_value(corners(S, idx), frac), *lo_span[n])
                ok = b >= 0
                act, b = act[ok], b[ok]
                w = (f32(1) - A[act]) * opacity[b]
                C[act] = C[act] + w[:, None] * table[b].astype(f32)
                A[act] = A[act] + w
                done[act] = A[act] > ALPHA_CUTOFF
            rest = f32(1) - A
            rgb = to_byte((C + rest[:, None] * bg[None, :]) + f32(0.5))
            rgb[ns == 0] = np.asarray(background, dtype=np.uint8)
            frames[n], alphas[n] = rgb, A
    frames = frames.reshape(len(envs), H, W, 3)
    return (frames, alphas.reshape(len(envs), H, W)) if return_alpha else frames


def fixed_range(lo: float, hi: float):
    """``(lo32, span32)`` of a range given as Python numbers (``frames.value_range_tensor``)."""
    return f32(lo), f32(float(hi) - float(lo))


def auto_range(values: np.ndarray):
    v = np.asarray(values, dtype=f32)
    return v.min(), v.max() - v.min()
