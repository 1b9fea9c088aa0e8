// 3-D frames of the envs of a batch: the reference's render(render_3d=True) -- marching cubes plus a matplotlib Poly3DCollection
// (envs/util/visualization.py:211-379) and ax.voxels (:382-475), seconds per frame on the host for one env -- as one ray marcher over
// the volumes that are already on the device, batched (include/fluidgym_hip.h).  Two modes behind two entries:
// fg_render_isosurface (first crossing of |f| = level, shaded, coloured by a second field, an optional solid body as a second level
// set) and fg_render_volume (emission-absorption, front to back).
//
// Shape: one thread one pixel, a workgroup a 16 x 16 pixel tile, a wave a compact 8 x 8 patch of it (neighbouring rays read
// neighbouring cells: the gathers of a wave fall into a few cache lines of a volume that fits in L2), the grid over (tile, listed env),
// at most 64 listed envs per launch, the colour table (and the opacity table) once per workgroup in LDS.  Latency-bound by its
// dependent gathers (8 per sample), not by bytes; no empty-space skipping, no translucent surfaces.
//
// The promise is equality with the NumPy restatement (tests/render3d_ref.py), bytes and depth: the file is compiled with
// -ffp-contract=off, every operation below is rounded on its own in float32, only + - * /, sqrtf, floorf, comparisons and conversions.
//
// ORDER OF OPERATIONS (the restatement follows it literally; a, b, c stand for x, y, z; n_a the extent, index space [0, n_a - 1]):
//  ray      pj = float(j) + 0.5, pi = float(i) + 0.5;  o_a = (o0_a + pj ou_a) + pi ov_a;  d_a = (d0_a + pj du_a) + pi dv_a
//  slabs    tmin = 0, tmax = +inf; per axis in the order x, y, z: d_a == 0: miss if o_a < 0 or o_a > n_a - 1; else t1 = (0 - o_a) / d_a,
//           t2 = (float(n_a - 1) - o_a) / d_a, tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1, tmin = tn > tmin ? tn : tmin,
//           tmax = tf < tmax ? tf : tmax;  miss unless tmin <= tmax
//  samples  nf = floorf((tmax - tmin) / step), nf = 65535 unless nf <= 65535; samples s = 0 .. int(nf);  t_s = tmin + float(s) step;
//           p_a = o_a + t_s d_a
//  cell     c_a = floorf(p_a) clamped to [0, n_a - 2] (0 unless c_a >= 0), f_a = p_a - c_a; corners v[dz][dy][dx] of the scalar (one channel, or
//           sqrtf(((u0 u0) + (u1 u1)) + (u2 u2)); iso mode: fabsf of it; solid mask: 1 for non-zero, else 0)
//  lerp     L(a, b, f) = a + f (b - a);  value = L(L(L(v000, v001, fx), L(v010, v011, fx), fy), L(L(v100, v101, fx), L(v110, v111, fx), fy), fz)
//  gradient gx = L(L(v001 - v000, v011 - v010, fy), L(v101 - v100, v111 - v110, fy), fz)
//           gy = L(L(v010 - v000, v011 - v001, fx), L(v110 - v100, v111 - v101, fx), fz)
//           gz = L(L(v100 - v000, v101 - v001, fx), L(v110 - v010, v111 - v011, fx), fy)
//  iso      g_s = value - level (inside the clip box lo_a <= p_a <= hi_a only); m_s = solid value - 0.5 (no clip box); a crossing of
//           (u, w) = consecutive samples: (u < 0 and w >= 0) or (u >= 0 and w < 0) -- a NaN never crosses; for g both samples inside
//           the clip box.  q = u / (u - w), q = 0.5 unless 0 <= q <= 1;  t_hit = t_{s-1} + q (t_s - t_{s-1}).  The first s with a
//           crossing ends the ray; with both, the surface wins if its t_hit <= the solid's.  h_a = o_a + t_hit d_a.
//  shade    cell and gradient at h of the field that was hit;  nd = (gx dx + gy dy) + gz dz;  nn = sqrtf((gx gx + gy gy) + gz gz);
//           dd = sqrtf((dx dx + dy dy) + dz dz);  c = fabsf(nd) / (nn dd), c = 0 unless c >= 0, c = 1 if c > 1;
//           shade = ambient + diffuse c
//  colour   surface: cell k_a = int(h_a) clamped to [0, n_a - 1], v the colour scalar there, x = (v - lo) / span clipped to [0, 1],
//           NaN -> black, else table[min(int(x 256), 255)] (the rule of fg_frame_colorize); solid: the body colour;
//           byte = floorf(float(component) shade + 0.5) clamped to [0, 255];  depth = t_hit (+inf and the background without a hit)
//  volume   A = Cr = Cg = Cb = 0; per sample in order: x as above from the value (not its modulus); NaN: nothing; k = min(int(x 256), 255),
//           w = (1 - A) opacity[k], C_c = C_c + w float(table[k][c]), A = A + w, stop once A > 0.99;
//           byte = floorf((C_c + (1 - A) float(background_c)) + 0.5) clamped to [0, 255]; a miss is the background
#include "fg_internal.h"

#include <cmath>
#include <cstring>

namespace {

constexpr int R3_THREADS = 256;
constexpr int R3_TILE = 16;
constexpr int ENVS_PER_LAUNCH = 64;
constexpr float MAX_SAMPLES = 65535.f;
constexpr float ALPHA_CUTOFF = 0.99f;

struct R3Args {
    const float* vol;
    const float* cvol;         // colour field (iso mode)
    const uint8_t* solid;      // [nz ny nx] or null
    const uint8_t* table;
    const float* opacity;      // [256] (volume mode)
    const float* level;        // level of the first env of this launch
    const float* range;        // (lo, span) of the first env of this launch
    uint8_t* out;              // frame of the first env of this launch
    float* depth;              // depth frame of the first env of this launch, or null
    long long cell_count;      // nz ny nx = a channel's stride of either field
    int nx, ny, nz;
    int C, channel, Cc, cchannel;
    int H, W, tiles_x;
    float cam[18];             // o0, ou, ov, d0, du, dv, each (x, y, z)
    float step, ambient, diffuse;
    int has_clip;
    float clip_lo[3], clip_hi[3];
    uint32_t body, background; // r | g << 8 | b << 16
    int32_t envs[ENVS_PER_LAUNCH];
};

__device__ __forceinline__ float lerp(float a, float b, float f) { return a + f * (b - a); }

// the scalar of a field at a cell: one channel, or the norm formed as fg_frame_colorize forms it
__device__ __forceinline__ float scalar_at(const float* f, long long cell, int channel, int C, long long cs) {
    if (channel >= 0) return f[cell + channel * cs];
    float u = f[cell];
    float s = u * u;
    for (int j = 1; j < C; ++j) { u = f[cell + j * cs]; s = s + u * u; }
    return sqrtf(s);
}

struct Cell {
    float v[8];                // v[4 dz + 2 dy + dx]
    float fx, fy, fz;
    long long base;            // cell index of corner (0, 0, 0)
};

__device__ __forceinline__ float cell_floor(float p, int n, float& frac) {
    float c = floorf(p);
    const float top = (float)(n - 2);
    c = c >= 0.f ? c : 0.f;            // (written so that a NaN position -- an overflowed camera -- lands in cell 0, never in an address)
    c = c > top ? top : c;
    frac = p - c;
    return c;
}

__device__ __forceinline__ void locate(Cell& c, const R3Args& a, float px, float py, float pz) {
    const int ix = (int)cell_floor(px, a.nx, c.fx), iy = (int)cell_floor(py, a.ny, c.fy), iz = (int)cell_floor(pz, a.nz, c.fz);
    c.base = ((long long)iz * a.ny + iy) * a.nx + ix;
}

template <bool ABS>
__device__ __forceinline__ void load_field(Cell& c, const R3Args& a, const float* fe) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const long long cell = c.base + ((long long)(k >> 2) * a.ny + ((k >> 1) & 1)) * a.nx + (k & 1);
        const float v = scalar_at(fe, cell, a.channel, a.C, a.cell_count);
        c.v[k] = ABS ? fabsf(v) : v;
    }
}

__device__ __forceinline__ void load_solid(Cell& c, const R3Args& a) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const long long cell = c.base + ((long long)(k >> 2) * a.ny + ((k >> 1) & 1)) * a.nx + (k & 1);
        c.v[k] = a.solid[cell] != 0 ? 1.f : 0.f;
    }
}

__device__ __forceinline__ float cell_value(const Cell& c) {
    const float c00 = lerp(c.v[0], c.v[1], c.fx), c01 = lerp(c.v[2], c.v[3], c.fx);
    const float c10 = lerp(c.v[4], c.v[5], c.fx), c11 = lerp(c.v[6], c.v[7], c.fx);
    return lerp(lerp(c00, c01, c.fy), lerp(c10, c11, c.fy), c.fz);
}

__device__ __forceinline__ void cell_gradient(const Cell& c, float& gx, float& gy, float& gz) {
    const float* v = c.v;
    gx = lerp(lerp(v[1] - v[0], v[3] - v[2], c.fy), lerp(v[5] - v[4], v[7] - v[6], c.fy), c.fz);
    gy = lerp(lerp(v[2] - v[0], v[3] - v[1], c.fx), lerp(v[6] - v[4], v[7] - v[5], c.fx), c.fz);
    gz = lerp(lerp(v[4] - v[0], v[5] - v[1], c.fx), lerp(v[6] - v[2], v[7] - v[3], c.fx), c.fy);
}

__device__ __forceinline__ bool crosses(float u, float w) { return (u < 0.f && w >= 0.f) || (u >= 0.f && w < 0.f); }

__device__ __forceinline__ float secant(float u, float w, float tp, float t) {
    float q = u / (u - w);
    q = (q >= 0.f && q <= 1.f) ? q : 0.5f;
    return tp + q * (t - tp);
}

__device__ __forceinline__ int cell_trunc(float h, int n) {
    float k = h < 0.f ? 0.f : h;
    const float top = (float)(n - 1);
    k = k > top ? top : k;
    return (int)k;
}

__device__ __forceinline__ uint32_t shade_byte(uint32_t comp, float shade) {
    float q = floorf((float)comp * shade + 0.5f);
    q = q < 0.f ? 0.f : q;
    q = q > 255.f ? 255.f : q;
    return (uint32_t)q;
}

// the bin of the colour table, or -1 for a NaN
__device__ __forceinline__ int table_bin(float v, float lo, float span) {
    float x = (v - lo) / span;
    x = x < 0.f ? 0.f : x;
    x = x > 1.f ? 1.f : x;
    if (x != x) return -1;
    const int idx = (int)(x * 256.f);
    return idx > 255 ? 255 : idx;
}

// MODE 0: iso-surface; 1: volume
template <int MODE, bool SOLID>
__global__ __launch_bounds__(R3_THREADS) void k_render3d(const R3Args a) {
    __shared__ uint32_t lut[256];                                // r | g << 8 | b << 16
    __shared__ float opac[256];
    const int tid = threadIdx.x;
    lut[tid] = (uint32_t)a.table[3 * tid] | ((uint32_t)a.table[3 * tid + 1] << 8) | ((uint32_t)a.table[3 * tid + 2] << 16);
    if (MODE == 1) opac[tid] = a.opacity[tid];
    __syncthreads();
    // a wave is an 8 x 8 patch of the 16 x 16 tile
    const int wave = tid >> 6, lane = tid & 63;
    const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
    const int i = ty * R3_TILE + (wave >> 1) * 8 + (lane >> 3), j = tx * R3_TILE + (wave & 1) * 8 + (lane & 7);
    if (i >= a.H || j >= a.W) return;
    const int e = blockIdx.y;                                    // wave-uniform: the listed env
    const float* fe = a.vol + (size_t)a.envs[e] * (size_t)a.C * (size_t)a.cell_count;
    const float lo = a.range[2 * e], span = a.range[2 * e + 1];
    const size_t pixel = ((size_t)e * (size_t)a.H + (size_t)i) * (size_t)a.W + (size_t)j;

    const float pj = (float)j + 0.5f, pi = (float)i + 0.5f;
    float o[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o[k] = (a.cam[k] + pj * a.cam[3 + k]) + pi * a.cam[6 + k];
        d[k] = (a.cam[9 + k] + pj * a.cam[12 + k]) + pi * a.cam[15 + k];
    }
    const int ext[3] = {a.nx, a.ny, a.nz};
    float tmin = 0.f, tmax = INFINITY;
    bool miss = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float top = (float)(ext[k] - 1);
        if (d[k] == 0.f) {
            if (o[k] < 0.f || o[k] > top) miss = true;
        } else {
            const float t1 = (0.f - o[k]) / d[k], t2 = (top - o[k]) / d[k];
            const float tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1;
            tmin = tn > tmin ? tn : tmin;
            tmax = tf < tmax ? tf : tmax;
        }
    }
    if (!(tmin <= tmax)) miss = true;
    int ns = 0;
    if (!miss) {
        float nf = floorf((tmax - tmin) / a.step);
        nf = nf <= MAX_SAMPLES ? nf : MAX_SAMPLES;
        ns = (int)nf + 1;
    }

    uint32_t rgb = a.background;
    float t_hit = INFINITY;
    Cell c;
    if (MODE == 0) {
        const float level = a.level[e];
        int kind = 0;                                            // 1: the surface, 2: the solid body
        float gp = 0.f, mp = 0.f, tp = 0.f;
        bool inp = false;
        for (int s = 0; s < ns; ++s) {
            const float t = tmin + (float)s * a.step;
            const float px = o[0] + t * d[0], py = o[1] + t * d[1], pz = o[2] + t * d[2];
            const bool inc = !a.has_clip || (px >= a.clip_lo[0] && px <= a.clip_hi[0] && py >= a.clip_lo[1] && py <= a.clip_hi[1] &&
                                             pz >= a.clip_lo[2] && pz <= a.clip_hi[2]);
            locate(c, a, px, py, pz);
            float gc = 0.f, mc = 0.f;
            if (inc) {                                           // (a sample outside the clip box is never read)
                load_field<true>(c, a, fe);
                gc = cell_value(c) - level;
            }
            if (SOLID) {
                load_solid(c, a);
                mc = cell_value(c) - 0.5f;
            }
            if (s > 0) {
                const bool hi = inp && inc && crosses(gp, gc);
                const bool hs = SOLID && crosses(mp, mc);
                const float ti = hi ? secant(gp, gc, tp, t) : 0.f;
                const float ts = hs ? secant(mp, mc, tp, t) : 0.f;
                if (hi && (!hs || ti <= ts)) { kind = 1; t_hit = ti; break; }
                if (hs) { kind = 2; t_hit = ts; break; }
            }
            gp = gc; mp = mc; tp = t; inp = inc;
        }
        if (kind != 0) {
            const float hx = o[0] + t_hit * d[0], hy = o[1] + t_hit * d[1], hz = o[2] + t_hit * d[2];
            locate(c, a, hx, hy, hz);
            uint32_t base_rgb;
            if (kind == 1) {
                load_field<true>(c, a, fe);
                const long long cell = ((long long)cell_trunc(hz, a.nz) * a.ny + cell_trunc(hy, a.ny)) * a.nx + cell_trunc(hx, a.nx);
                const float* ce = a.cvol + (size_t)a.envs[e] * (size_t)a.Cc * (size_t)a.cell_count;
                const int bin = table_bin(scalar_at(ce, cell, a.cchannel, a.Cc, a.cell_count), lo, span);
                base_rgb = bin < 0 ? 0u : lut[bin];
            } else {
                load_solid(c, a);
                base_rgb = a.body;
            }
            float gx, gy, gz;
            cell_gradient(c, gx, gy, gz);
            const float nd = (gx * d[0] + gy * d[1]) + gz * d[2];
            const float nn = sqrtf((gx * gx + gy * gy) + gz * gz);
            const float dd = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
            float cs = fabsf(nd) / (nn * dd);
            cs = cs >= 0.f ? cs : 0.f;
            cs = cs > 1.f ? 1.f : cs;
            const float shade = a.ambient + a.diffuse * cs;
            rgb = shade_byte(base_rgb & 255u, shade) | (shade_byte((base_rgb >> 8) & 255u, shade) << 8) |
                  (shade_byte((base_rgb >> 16) & 255u, shade) << 16);
        }
        if (a.depth) a.depth[pixel] = t_hit;
    } else {
        if (ns > 0) {
            float A = 0.f, cr = 0.f, cg = 0.f, cb = 0.f;
            for (int s = 0; s < ns; ++s) {
                const float t = tmin + (float)s * a.step;
                locate(c, a, o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]);
                load_field<false>(c, a, fe);
                const int bin = table_bin(cell_value(c), lo, span);
                if (bin >= 0) {
                    const uint32_t col = lut[bin];
                    const float w = (1.f - A) * opac[bin];
                    cr = cr + w * (float)(col & 255u);
                    cg = cg + w * (float)((col >> 8) & 255u);
                    cb = cb + w * (float)((col >> 16) & 255u);
                    A = A + w;
                    if (A > ALPHA_CUTOFF) break;
                }
            }
            const float rest = 1.f - A;
            const uint32_t bg = a.background;
            rgb = shade_byte(1u, cr + rest * (float)(bg & 255u)) | (shade_byte(1u, cg + rest * (float)((bg >> 8) & 255u)) << 8) |
                  (shade_byte(1u, cb + rest * (float)((bg >> 16) & 255u)) << 16);
        }
    }
    uint8_t* px_out = a.out + pixel * 3;
    px_out[0] = (uint8_t)(rgb & 255u);
    px_out[1] = (uint8_t)((rgb >> 8) & 255u);
    px_out[2] = (uint8_t)((rgb >> 16) & 255u);
}

uint32_t pack_rgb(const uint8_t* c) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16); }

// the checks both entries share; fills what they share of the arguments
int check_common(const char* who, int32_t B, int32_t C, int32_t nz, int32_t ny, int32_t nx, int32_t channel,
                 const fg_render_camera* cam, const fg_render_options* opt, int32_t H, int32_t W, const int32_t* envs, int32_t n, R3Args& a) {
    const std::string w(who);
    FG_REQUIRE(n >= 1, FG_ERR_INVALID_ARG, w + ": n must be at least 1");
    FG_REQUIRE(B >= 1 && C >= 1, FG_ERR_INVALID_ARG, w + ": B and C must be at least 1");
    FG_REQUIRE(nz >= 2 && ny >= 2 && nx >= 2, FG_ERR_INVALID_ARG, w + ": every extent of the volume must be at least 2");
    for (int32_t i = 0; i < n; ++i)
        FG_REQUIRE(envs[i] >= 0 && envs[i] < B, FG_ERR_INVALID_ARG,
                   w + ": envs[" + std::to_string(i) + "] = " + std::to_string(envs[i]) + " is outside [0, " + std::to_string(B) + ")");
    FG_REQUIRE(channel >= -1 && channel < C, FG_ERR_INVALID_ARG,
               w + ": channel " + std::to_string(channel) + " is outside [-1, " + std::to_string(C) + ")");
    FG_REQUIRE(H >= 1 && W >= 1, FG_ERR_INVALID_ARG, w + ": H and W must be at least 1");
    FG_REQUIRE((long long)H * (long long)W * 3 < 0x80000000LL, FG_ERR_INVALID_ARG, w + ": a frame must stay below 2^31 bytes");
    FG_REQUIRE(opt->step > 0.f && std::isfinite(opt->step), FG_ERR_INVALID_ARG, w + ": step must be positive and finite");
    if (opt->has_clip)
        for (int k = 0; k < 3; ++k)
            FG_REQUIRE(opt->clip_lo[k] <= opt->clip_hi[k], FG_ERR_INVALID_ARG,
                       w + ": the clip box is empty along axis " + std::string(1, "xyz"[k]));
    static_assert(sizeof(fg_render_camera) == 18 * sizeof(float), "fg_render_camera is six vectors of three floats");
    float cf[18];
    std::memcpy(cf, cam, sizeof cf);
    for (int k = 0; k < 18; ++k) FG_REQUIRE(std::isfinite(cf[k]), FG_ERR_INVALID_ARG, w + ": the camera holds a non-finite entry");
    FG_REQUIRE(cam->d0[0] != 0.f || cam->d0[1] != 0.f || cam->d0[2] != 0.f, FG_ERR_INVALID_ARG, w + ": the camera direction d0 is zero");
    a.cell_count = (long long)nz * ny * nx;
    a.nx = nx; a.ny = ny; a.nz = nz; a.C = C; a.channel = channel; a.H = H; a.W = W;
    a.tiles_x = (W + R3_TILE - 1) / R3_TILE;
    for (int k = 0; k < 18; ++k) a.cam[k] = cf[k];
    a.step = opt->step; a.ambient = opt->ambient; a.diffuse = opt->diffuse; a.has_clip = opt->has_clip != 0;
    for (int k = 0; k < 3; ++k) { a.clip_lo[k] = opt->clip_lo[k]; a.clip_hi[k] = opt->clip_hi[k]; }
    a.body = pack_rgb(opt->body_color); a.background = pack_rgb(opt->background);
    return FG_OK;
}

template <int MODE>
void launch_all(R3Args& a, const float* level, const float* range, const int32_t* envs, int32_t n, uint8_t* out, float* depth, hipStream_t st) {
    const size_t pixels = (size_t)a.H * (size_t)a.W;
    const unsigned tiles = (unsigned)a.tiles_x * (unsigned)((a.H + R3_TILE - 1) / R3_TILE);
    for (int32_t first = 0; first < n; first += ENVS_PER_LAUNCH) {
        const int32_t count = n - first < ENVS_PER_LAUNCH ? n - first : ENVS_PER_LAUNCH;
        for (int32_t i = 0; i < ENVS_PER_LAUNCH; ++i) a.envs[i] = i < count ? envs[first + i] : 0;
        a.level = level ? level + first : nullptr;
        a.range = range + 2 * (size_t)first;
        a.out = out + (size_t)first * pixels * 3;
        a.depth = depth ? depth + (size_t)first * pixels : nullptr;
        const dim3 grid(tiles, count);
        if (MODE == 0 && a.solid) hipLaunchKernelGGL((k_render3d<0, true>), grid, dim3(R3_THREADS), 0, st, a);
        else if (MODE == 0) hipLaunchKernelGGL((k_render3d<0, false>), grid, dim3(R3_THREADS), 0, st, a);
        else hipLaunchKernelGGL((k_render3d<1, false>), grid, dim3(R3_THREADS), 0, st, a);
    }
}

}  // namespace

extern "C" int fg_render_isosurface(const float* volume, int32_t B, int32_t C, int32_t nz, int32_t ny, int32_t nx, int32_t channel,
                                    const float* level, const float* color_volume, int32_t color_C, int32_t color_channel,
                                    const float* range, const uint8_t* table, const uint8_t* solid, const fg_render_camera* camera,
                                    const fg_render_options* options, int32_t H, int32_t W, const int32_t* envs, int32_t n, uint8_t* out,
                                    float* depth, void* stream) {
    FG_REQUIRE(volume && level && color_volume && range && table && camera && options && envs && out, FG_ERR_INVALID_ARG,
               "fg_render_isosurface: null argument (volume, level, color_volume, range, table, camera, options, envs and out are required)");
    R3Args a{};
    const int rc = check_common("fg_render_isosurface", B, C, nz, ny, nx, channel, camera, options, H, W, envs, n, a);
    if (rc != FG_OK) return rc;
    FG_REQUIRE(color_C >= 1 && color_channel >= -1 && color_channel < color_C, FG_ERR_INVALID_ARG,
               "fg_render_isosurface: colour channel " + std::to_string(color_channel) + " is outside [-1, " + std::to_string(color_C) + ")");
    a.vol = volume; a.cvol = color_volume; a.solid = solid; a.table = table; a.opacity = nullptr;
    a.Cc = color_C; a.cchannel = color_channel;
    launch_all<0>(a, level, range, envs, n, out, depth, (hipStream_t)stream);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}

extern "C" int fg_render_volume(const float* volume, int32_t B, int32_t C, int32_t nz, int32_t ny, int32_t nx, int32_t channel,
                                const float* range, const uint8_t* table, const float* opacity, const fg_render_camera* camera,
                                const fg_render_options* options, int32_t H, int32_t W, const int32_t* envs, int32_t n, uint8_t* out,
                                void* stream) {
    FG_REQUIRE(volume && range && table && opacity && camera && options && envs && out, FG_ERR_INVALID_ARG,
               "fg_render_volume: null argument (volume, range, table, opacity, camera, options, envs and out are required)");
    R3Args a{};
    const int rc = check_common("fg_render_volume", B, C, nz, ny, nx, channel, camera, options, H, W, envs, n, a);
    if (rc != FG_OK) return rc;
    a.vol = volume; a.cvol = nullptr; a.solid = nullptr; a.table = table; a.opacity = opacity;
    a.Cc = 1; a.cchannel = 0;
    launch_all<1>(a, nullptr, range, envs, n, out, nullptr, (hipStream_t)stream);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}
