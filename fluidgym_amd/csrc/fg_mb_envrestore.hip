// Per-env restore of a multi-block handle (include/fluidgym_hip.h): chosen envs of the batch become states of a bank,
// each mirrored and rolled along the span of an extruded, z-periodic mesh and, when asked, with counter-based Gaussian reset noise on
// velocity and pressure (the per-env form of the reference's _randomize_domain, cylinder_env_base.py:364-404, without its warm-up
// steps).  A handle carries three per-env arrays between steps -- velocity [B][d][N], pressure [B][N], boundary velocity [B][d][NB] --
// and ONE launch restores all three: at the envs' sizes (a few thousand to 47 k cells) a restore is bound by its launches, not by bytes.
//
// The map.  The cells of a block, offset + (z ny + y) nx + x, and the slots of a FIXED x- or y-face, slot0 + z len + t, are segments
// {first, plane, nz}; on both
//     dst[first + z plane + r] = sign(c) bank[src][first + zs plane + r],   zs = flip_z ? nz-1 - ((z - shift_z) mod nz) : (z - shift_z) mod nz
// sign(c) = -1 for component 2 of velocity and boundary velocity under flip_z.  Where the span is no symmetry of the topology (2-D, a
// block that is not z-periodic, blocks of different nz) a segment is one plane and the map a copy.
//
// The noise.  Destination cell i (flat index in [0, N)) of component tag c -- 0..d-1 velocity, d pressure -- takes normal i % 4 of the
// Philox4x32-10 block with key (seed low, seed high) and counter ((c << 24) | (i / 4), env, episode, 0xFFFFFFFF); dst = value +
// (float)sigma z in fp32, value + sigma (double)z in fp64 (fg_philox.h; the arithmetic of z is defined at the top of fg_obsnoise.hip,
// and this file is compiled with -ffp-contract=off as that one is).  Boundary values get none.
//
// Shape: segment and tile tables are built on the host once per handle; a tile is up to 1024 consecutive destination elements of one
// segment.  The grid runs over (tile, selected env), never over the whole batch: an env that is not named is not written.  A workgroup
// is 256 threads, each lane owns a quad of four consecutive destination elements: (z, r) and the source offset of the quad are formed
// once and reused for every component (d velocity components and the pressure on a cell tile, d components on a face tile).  A quad
// that stays inside one plane is loaded and stored as 16-byte words where the addresses allow it (segments start anywhere: N = 77
// exists), element by element otherwise.  The Philox blocks are indexed by the GLOBAL quad i / 4 of the flat cell index, so a lane
// whose quad is not 4-aligned in i evaluates two blocks (the misalignment is the tile's: wave-uniform).  The selection record and the
// tile record are read through wave-uniform addresses.  No LDS, no atomics, no data-dependent loop, nothing returns to the host; with
// noise == NULL every value is a copy or a negation.
#include <cmath>
#include <vector>

#include "fg_mb.h"
#include "fg_philox.h"

namespace {

constexpr int MR_THREADS = 256;
constexpr int MR_TILE = 4 * MR_THREADS;
constexpr int MR_MAX_NOISE_N = 1 << 26;

// what the kernel reads of one record: the upload of a call is n_sel of these
struct MrSel { int32_t env, src, flip_z, shift_z; uint32_t episode; };

struct MrArgs {
    mb_real *velocity, *pressure, *bvel;                    // bound fields
    const mb_real *bank_velocity, *bank_pressure, *bank_bvel;
    const MbRestoreTile* tiles;
    const MrSel* sel;
    int d, N, NB;
    int noise;
    uint32_t key0, key1;
    double sigma_velocity, sigma_pressure;
};

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// four source elements: one or two 16-byte loads when the quad is whole, contiguous and aligned, else element by element
template <typename T>
__device__ __forceinline__ void load_quad(const T* __restrict__ base, const int off[4], int left, bool contiguous, T v[4]) {
    const T* p = base + off[0];
    if (contiguous && aligned16(p)) {
        if constexpr (sizeof(T) == 4) {
            const float4 q = *reinterpret_cast<const float4*>(p);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            const double2 lo = reinterpret_cast<const double2*>(p)[0], hi = reinterpret_cast<const double2*>(p)[1];
            v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < left ? base[off[j]] : (T)0;
    }
}

template <typename T>
__device__ __forceinline__ void store_quad(T* __restrict__ p, int left, const T v[4]) {
    if (left == 4 && aligned16(p)) {
        if constexpr (sizeof(T) == 4) {
            *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            reinterpret_cast<double2*>(p)[0] = make_double2(v[0], v[1]);
            reinterpret_cast<double2*>(p)[1] = make_double2(v[2], v[3]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < left) p[j] = v[j];
    }
}

// the four normals of the cells i0 .. i0 + 3 of component tag c: normals a .. a + 3 of the blocks i0 / 4 and, when a = i0 % 4 is not
// zero, i0 / 4 + 1
__device__ __forceinline__ void quad_normals(uint32_t tag, uint32_t i0, uint32_t env, uint32_t episode, uint32_t k0, uint32_t k1, float z[4]) {
    const uint32_t a = i0 & 3u, blk = (tag << 24) | (i0 >> 2);
    uint32_t w[4];
    float n[8];
    philox4x32_10(blk, env, episode, 0xFFFFFFFFu, k0, k1, w);
    normal_pair(w[0], w[1], n[0], n[1]);
    normal_pair(w[2], w[3], n[2], n[3]);
    n[4] = n[5] = n[6] = n[7] = 0.0f;
    if (a != 0) {
        philox4x32_10(blk + 1u, env, episode, 0xFFFFFFFFu, k0, k1, w);
        normal_pair(w[0], w[1], n[4], n[5]);
        normal_pair(w[2], w[3], n[6], n[7]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] = a == 0 ? n[j] : a == 1 ? n[j + 1] : a == 2 ? n[j + 2] : n[j + 3];
}

template <typename T>
__global__ __launch_bounds__(MR_THREADS) void k_mb_restore_envs(const MrArgs a) {
    const MbRestoreTile t = a.tiles[blockIdx.x];               // wave-uniform: tile and record
    const MrSel r = a.sel[blockIdx.y];
    const int e0 = t.start + 4 * (int)threadIdx.x;             // first element of the quad, counted from the segment's first
    const int left = min(4, t.start + t.count - e0);
    if (left <= 0) return;
    // (z, r) of the quad and its source, once for every component
    const int z = e0 / t.plane, rr = e0 - z * t.plane;
    auto source_plane = [&](int zz) {
        int zs = zz - r.shift_z;
        if (zs < 0) zs += t.nz;
        return r.flip_z ? t.nz - 1 - zs : zs;
    };
    int off[4];
    const bool in_plane = rr + 4 <= t.plane;
    if (in_plane) {
        const int o = source_plane(z) * t.plane + rr;
#pragma unroll
        for (int j = 0; j < 4; ++j) off[j] = o + j;
    } else {                                                    // the quad crosses a plane (planes may be as short as three elements)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = min(e0 + j, t.start + t.count - 1);
            const int zj = e / t.plane;
            off[j] = source_plane(zj) * t.plane + (e - zj * t.plane);
        }
    }
    const bool contiguous = in_plane && left == 4;
    const bool flip = r.flip_z != 0;
    T v[4];
    if (t.face) {
        const size_t per = (size_t)a.NB;
        for (int c = 0; c < a.d; ++c) {
            load_quad<T>(a.bank_bvel + ((size_t)r.src * a.d + c) * per + t.first, off, left, contiguous, v);
            if (flip && c == 2) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = -v[j];
            }
            store_quad<T>(a.bvel + ((size_t)r.env * a.d + c) * per + t.first + e0, left, v);
        }
        return;
    }
    const size_t per = (size_t)a.N;
    const uint32_t i0 = (uint32_t)(t.first + e0);              // flat cell index of the quad's first element
    float zn[4];
    for (int c = 0; c <= a.d; ++c) {                            // d velocity components, then the pressure
        const bool vel = c < a.d;
        const T* __restrict__ src = vel ? a.bank_velocity + ((size_t)r.src * a.d + c) * per : a.bank_pressure + (size_t)r.src * per;
        T* __restrict__ dst = vel ? a.velocity + ((size_t)r.env * a.d + c) * per : a.pressure + (size_t)r.env * per;
        load_quad<T>(src + t.first, off, left, contiguous, v);
        if (flip && c == 2 && vel) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = -v[j];
        }
        if (a.noise) {
            const double sigma = vel ? a.sigma_velocity : a.sigma_pressure;
            quad_normals((uint32_t)c, i0, (uint32_t)r.env, r.episode, a.key0, a.key1, zn);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = add_noise(v[j], sigma, zn[j]);
        }
        store_quad<T>(dst + i0, left, v);
    }
}

// segments and tiles of the handle, once: the blocks' cells and the FIXED faces' slots, as nz planes where the span is a symmetry of
// the topology and as one plane otherwise
void build_tiles(fg_mb_state* s) {
    int nz = 0;
    if (s->d == 3) {
        nz = s->blocks[0].size[2];
        for (const MbBlock& b : s->blocks)
            if (b.bounds[4].type != FG_MB_PERIODIC || b.bounds[5].type != FG_MB_PERIODIC || b.size[2] != nz) nz = 0;
    }
    s->restore_tiles.clear();
    auto add_segment = [&](int first, int count, int face) {
        const int planes = nz > 0 ? nz : 1;
        for (int start = 0; start < count; start += MR_TILE)
            s->restore_tiles.push_back({first, count / planes, planes, start, count - start < MR_TILE ? count - start : MR_TILE, face});
    };
    for (const MbBlock& b : s->blocks) add_segment(b.offset, b.ncells, 0);
    for (const MbBlock& b : s->blocks)
        for (int f = 0; f < s->F; ++f)
            if (b.bounds[f].type == FG_MB_FIXED) add_segment(b.bounds[f].slot0, b.ncells / b.size[f >> 1], 1);
    s->restore_nz = nz;
}

}  // namespace

extern "C" int fg_mb_restore_envs(fg_mb_handle s, const mb_real* bank_velocity, const mb_real* bank_pressure, const mb_real* bank_boundary,
                                  int32_t S, const fg_env_sel* sel, int32_t n_sel, const fg_mb_reset_noise* noise, void* stream) {
    const std::string who = "fg_mb_restore_envs: ";
    FG_REQUIRE(s != nullptr, FG_ERR_INVALID_ARG, who + "null handle");
    FG_REQUIRE(sel != nullptr, FG_ERR_INVALID_ARG, who + "null selection");
    FG_REQUIRE(bank_velocity != nullptr && bank_pressure != nullptr && S >= 1, FG_ERR_INVALID_ARG, who + "null bank or S < 1");
    FG_REQUIRE(n_sel >= 1 && n_sel <= s->B, FG_ERR_INVALID_ARG, who + "n_sel must be in 1..batch");
    FG_REQUIRE(noise == nullptr || noise->episodes != nullptr, FG_ERR_INVALID_ARG, who + "noise without episodes");
    FG_REQUIRE(s->finalized, FG_ERR_NOT_BOUND, who + "the handle is not finalised");
    FG_REQUIRE(bank_boundary != nullptr || s->NB == 0, FG_ERR_INVALID_ARG, who + "null boundary bank on a handle with FIXED faces");
    if (s->restore_nz < 0) build_tiles(s);
    const int nz = s->restore_nz;
    std::vector<char> seen((size_t)s->B, 0);
    for (int i = 0; i < n_sel; ++i) {
        const fg_env_sel& r = sel[i];
        FG_REQUIRE(r.env >= 0 && r.env < s->B, FG_ERR_INVALID_ARG, who + "env index out of range");
        FG_REQUIRE(!seen[r.env], FG_ERR_INVALID_ARG, who + "an env is named twice");
        seen[r.env] = 1;
        FG_REQUIRE(r.src >= 0 && r.src < S, FG_ERR_INVALID_ARG, who + "src index out of range");
        FG_REQUIRE(r.flip_x == 0 && r.shift_x == 0, FG_ERR_INVALID_ARG, who + "flip_x / shift_x: the meshes have no symmetry along x");
        FG_REQUIRE((r.flip_z | 1) == 1, FG_ERR_INVALID_ARG, who + "a flip is 0 or 1");
        FG_REQUIRE(r.shift_z >= 0 && r.shift_z < (nz > 0 ? nz : 1), FG_ERR_INVALID_ARG, who + "shift_z must be in [0, nz)");
        FG_REQUIRE(nz > 0 || (r.flip_z == 0 && r.shift_z == 0), FG_ERR_INVALID_ARG,
                   who + "flip_z / shift_z need a 3-D handle whose blocks are all z-periodic and of one nz");
    }
    if (noise) {
        FG_REQUIRE(std::isfinite(noise->sigma_velocity) && noise->sigma_velocity >= 0.0 && std::isfinite(noise->sigma_pressure) &&
                       noise->sigma_pressure >= 0.0,
                   FG_ERR_INVALID_ARG, who + "a sigma is negative or not finite");
        FG_REQUIRE(s->N <= MR_MAX_NOISE_N, FG_ERR_UNSUPPORTED, who + "noise needs N <= 2^26 (the first counter word)");
    }
    FG_REQUIRE(n_sel <= 65535, FG_ERR_UNSUPPORTED, who + "at most 65535 envs per call");
    FG_REQUIRE(!s->host_only && s->velocity && s->pressure && (s->bvel || s->NB == 0), FG_ERR_NOT_BOUND, who + "the fields are not bound (fg_mb_bind)");
    hipStream_t st = (hipStream_t)stream;
    if (!s->restore_tiles_dev) {                                // once per handle
        void *tiles = nullptr, *records = nullptr;
        FG_HIP_CHECK(hipMalloc(&tiles, sizeof(MbRestoreTile) * s->restore_tiles.size()));
        s->owned.push_back(tiles);
        FG_HIP_CHECK(hipMalloc(&records, sizeof(MrSel) * (size_t)s->B));
        s->owned.push_back(records);
        FG_HIP_CHECK(hipMemcpy(tiles, s->restore_tiles.data(), sizeof(MbRestoreTile) * s->restore_tiles.size(), hipMemcpyHostToDevice));
        s->restore_sel_dev = records;
        s->restore_tiles_dev = (MbRestoreTile*)tiles;
    }
    std::vector<MrSel> rec((size_t)n_sel);
    for (int i = 0; i < n_sel; ++i) rec[i] = {sel[i].env, sel[i].src, sel[i].flip_z, sel[i].shift_z, noise ? noise->episodes[i] : 0u};
    FG_HIP_CHECK(hipMemcpyAsync(s->restore_sel_dev, rec.data(), sizeof(MrSel) * (size_t)n_sel, hipMemcpyHostToDevice, st));
    MrArgs a{};
    a.velocity = s->velocity; a.pressure = s->pressure; a.bvel = s->bvel;
    a.bank_velocity = bank_velocity; a.bank_pressure = bank_pressure; a.bank_bvel = bank_boundary;
    a.tiles = s->restore_tiles_dev; a.sel = (const MrSel*)s->restore_sel_dev;
    a.d = s->d; a.N = s->N; a.NB = s->NB;
    a.noise = noise ? 1 : 0;
    if (noise) {
        a.key0 = (uint32_t)(noise->seed & 0xffffffffu); a.key1 = (uint32_t)(noise->seed >> 32);
        a.sigma_velocity = noise->sigma_velocity; a.sigma_pressure = noise->sigma_pressure;
    }
    hipLaunchKernelGGL(k_mb_restore_envs<mb_real>, dim3((unsigned)s->restore_tiles.size(), (unsigned)n_sel), dim3(MR_THREADS), 0, st, a);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}
