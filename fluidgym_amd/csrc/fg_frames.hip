// RGB frames of the envs of a batch: the last step of the reference's _get_render_data / _format_render_data
// (envs/fluid_env.py:710-747) -- slice, transpose, flips, normalise, clip, 256-entry colour table, solid-body mask, uint8 RGB -- on the
// fields that are already on the device, batched (include/fluidgym_hip.h).
//
// The promise is byte equality with matplotlib's cmap(clip((d - vmin) / (vmax - vmin), 0, 1), bytes=True)[..., :3] on a float32 array:
// every product, sum, difference and the division are rounded on their own (the file is compiled with -ffp-contract=off, and hipcc's
// default float division and sqrtf are the correctly rounded ones).
//
// Shape: memory-bound by its bytes, 4-12 read and 3 written per pixel.  The grid runs over (tile of a frame, listed env).  A frame is a
// stream of H W 3 bytes that starts wherever n frames of that size put it, i.e. in general not on a dword; a tile is TILE_DW aligned
// dwords of that stream.  Pass 1: the workgroup issues every load of the tile's pixels, consecutive lanes consecutive pixels of a row
// (contiguous loads for the planes that keep x as the column; x-fixed and transposed planes are strided gathers, accepted), then
// normalises, clips, looks the colour up in an LDS copy of the table and puts the bytes into the tile in LDS.  Pass 2: consecutive
// lanes store consecutive dwords from LDS; only the dwords that straddle an end of the frame fall back to byte stores.  The orientation
// is folded on the host into (base, row stride, column stride) of the plane, the division by W into a multiply and a shift.
#include "fg_internal.h"

namespace {

constexpr int FRAME_THREADS = 256;
constexpr int TILE_DW = 3 * FRAME_THREADS;      // 768 dwords = 3072 bytes = 1024 pixels (+ the partial ones at its two ends)
constexpr int TILE_BYTES = 4 * TILE_DW;
constexpr int TILE_PIX = 5;                     // pixels per lane: at most 1025 pixels have a byte in a tile
constexpr int ENVS_PER_LAUNCH = 64;

struct FrameArgs {
    const float* field;
    const uint8_t* table;
    const uint8_t* mask;       // [H W] or null
    const float* range;        // (lo, span) of the first env of this launch
    uint8_t* out;              // frame of the first env of this launch
    long long env_stride;      // C nz ny nx
    long long ch_stride;       // nz ny nx
    long long base;            // offset of output pixel (0, 0) inside an env (a single channel's offset included)
    long long row_stride;      // per output row (negative for a flipped axis)
    long long col_stride;      // per output column
    int channels;              // C
    int W;
    int pixels;                // H W
    unsigned div_mul;          // p / W = (p div_mul) >> div_shift for every p < 2^31 (Granlund & Montgomery, N = 31)
    int div_shift;
    int32_t envs[ENVS_PER_LAUNCH];
};

// NC: 0 = one channel; 1..3 = the norm over NC channels; -1 = the norm over a.channels channels
template <int NC, bool MASK>
__global__ __launch_bounds__(FRAME_THREADS) void k_frame_colorize(const FrameArgs a) {
    __shared__ uint32_t tile[TILE_DW];
    __shared__ uint32_t lut[256];                                // r | g << 8 | b << 16
    uint8_t* tile_b = reinterpret_cast<uint8_t*>(tile);
    const int tid = threadIdx.x;
    const int e = blockIdx.y;                                    // wave-uniform: the listed env, its range and frame
    const int frame_bytes = 3 * a.pixels;
    uint8_t* frame = a.out + (size_t)e * (size_t)frame_bytes;
    const int mis = (int)(reinterpret_cast<uintptr_t>(frame) & 3);     // the frame starts `mis` bytes into an aligned dword
    const long long g0 = (long long)blockIdx.x * TILE_BYTES;     // first byte of the tile, counted from that aligned dword
    if (g0 >= (long long)frame_bytes + mis) return;
    lut[tid] = (uint32_t)a.table[3 * tid] | ((uint32_t)a.table[3 * tid + 1] << 8) | ((uint32_t)a.table[3 * tid + 2] << 16);
    const float lo = a.range[2 * e], span = a.range[2 * e + 1];
    const float* fe = a.field + (size_t)a.envs[e] * (size_t)a.env_stride + a.base;
    // pixels with a byte in the tile: the first is the one holding frame byte max(g0 - mis, 0)
    const long long f0 = g0 - mis;                               // frame byte of tile byte 0 (negative only in the first tile)
    const int p_first = (int)((f0 > 0 ? f0 : 0) / 3);
    const long long f_end = f0 + TILE_BYTES < frame_bytes ? f0 + TILE_BYTES : (long long)frame_bytes;
    const int p_end = (int)((f_end + 2) / 3);                    // one past the last such pixel
    // pass 1a: every load of the lane's pixels, consecutive lanes consecutive pixels
    float v[TILE_PIX];
    bool solid[TILE_PIX];
#pragma unroll
    for (int k = 0; k < TILE_PIX; ++k) {
        const int p = p_first + tid + k * FRAME_THREADS;
        v[k] = 0.f;
        solid[k] = false;
        if (p < p_end) {
            const int r = (int)(((unsigned long long)(unsigned)p * a.div_mul) >> a.div_shift), c = p - r * a.W;
            const float* src = fe + r * a.row_stride + c * a.col_stride;
            if (NC == 0) {
                v[k] = src[0];
            } else {
                float s = src[0] * src[0];
                if (NC > 0) {
#pragma unroll
                    for (int j = 1; j < NC; ++j) { const float u = src[(size_t)j * (size_t)a.ch_stride]; s = s + u * u; }
                } else {
                    for (int j = 1; j < a.channels; ++j) { const float u = src[(size_t)j * (size_t)a.ch_stride]; s = s + u * u; }
                }
                v[k] = sqrtf(s);
            }
            if (MASK) solid[k] = a.mask[p] != 0;
        }
    }
    __syncthreads();
    // pass 1b: normalise, clip, look up, bytes into the tile
#pragma unroll
    for (int k = 0; k < TILE_PIX; ++k) {
        const int p = p_first + tid + k * FRAME_THREADS;
        if (p < p_end) {
            float x = (v[k] - lo) / span;
            x = x < 0.f ? 0.f : x;
            x = x > 1.f ? 1.f : x;
            const bool nan = x != x;
            int idx = (int)((nan ? 0.f : x) * 256.f);
            idx = idx > 255 ? 255 : idx;
            const uint32_t rgb = (nan || solid[k]) ? 0u : lut[idx];
            const long long lb = (long long)p * 3 - f0;          // tile byte of the pixel's red byte
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (lb + j >= 0 && lb + j < TILE_BYTES) tile_b[lb + j] = (uint8_t)(rgb >> (8 * j));
        }
    }
    __syncthreads();
    // pass 2: consecutive lanes consecutive dwords; bytes only where a dword straddles an end of the frame
    uint8_t* aligned = frame - mis;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int d = tid + k * FRAME_THREADS;                   // dword of the tile
        const long long f = f0 + 4 * d;                          // frame byte of its first byte
        if (f >= 0 && f + 4 <= frame_bytes) {
            reinterpret_cast<uint32_t*>(aligned + g0)[d] = tile[d];
        } else {
            for (int j = 0; j < 4; ++j)
                if (f + j >= 0 && f + j < frame_bytes) frame[f + j] = tile_b[4 * d + j];
        }
    }
}

template <int NC>
void launch_frames(bool masked, dim3 grid, hipStream_t st, const FrameArgs& a) {
    if (masked) hipLaunchKernelGGL((k_frame_colorize<NC, true>), grid, dim3(FRAME_THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_frame_colorize<NC, false>), grid, dim3(FRAME_THREADS), 0, st, a);
}

}  // namespace

extern "C" int fg_frame_colorize(const float* field, int32_t B, int32_t C, int32_t nz, int32_t ny, int32_t nx, const fg_frame_spec* spec,
                                 const uint8_t* table, const uint8_t* mask, const float* range, const int32_t* envs, int32_t n, uint8_t* out,
                                 void* stream) {
    FG_REQUIRE(field && spec && table && range && envs && out, FG_ERR_INVALID_ARG,
               "fg_frame_colorize: null argument (field, spec, table, range, envs and out are required)");
    FG_REQUIRE(n >= 1, FG_ERR_INVALID_ARG, "fg_frame_colorize: n must be at least 1");
    FG_REQUIRE(B >= 1 && C >= 1 && nz >= 1 && ny >= 1 && nx >= 1, FG_ERR_INVALID_ARG, "fg_frame_colorize: every extent must be at least 1");
    for (int32_t i = 0; i < n; ++i)
        FG_REQUIRE(envs[i] >= 0 && envs[i] < B, FG_ERR_INVALID_ARG,
                   "fg_frame_colorize: envs[" + std::to_string(i) + "] = " + std::to_string(envs[i]) + " is outside [0, " + std::to_string(B) + ")");
    FG_REQUIRE(spec->channel >= -1 && spec->channel < C, FG_ERR_INVALID_ARG,
               "fg_frame_colorize: channel " + std::to_string(spec->channel) + " is outside [-1, " + std::to_string(C) + ")");
    FG_REQUIRE(spec->axis >= -1 && spec->axis <= 2, FG_ERR_INVALID_ARG, "fg_frame_colorize: axis must be -1 (2-D field), 0 (z), 1 (y) or 2 (x)");
    FG_REQUIRE(spec->axis != -1 || nz == 1, FG_ERR_INVALID_ARG, "fg_frame_colorize: axis -1 is the 2-D field and needs nz == 1");
    const int32_t extent = spec->axis <= 0 ? nz : (spec->axis == 1 ? ny : nx);
    FG_REQUIRE(spec->index >= 0 && spec->index < extent, FG_ERR_INVALID_ARG,
               "fg_frame_colorize: index " + std::to_string(spec->index) + " is outside the axis [0, " + std::to_string(extent) + ")");
    // the plane before orientation: rows, columns and their strides inside a channel
    const long long sz = (long long)ny * nx, sy = nx, sx = 1;
    long long prow, pcol, srow, scol, base;
    if (spec->axis <= 0) { prow = ny; pcol = nx; srow = sy; scol = sx; base = spec->index * sz; }
    else if (spec->axis == 1) { prow = nz; pcol = nx; srow = sz; scol = sx; base = spec->index * sy; }
    else { prow = nz; pcol = ny; srow = sz; scol = sy; base = spec->index * sx; }
    if (spec->transpose) { std::swap(prow, pcol); std::swap(srow, scol); }
    if (spec->flip_rows) { base += (prow - 1) * srow; srow = -srow; }
    if (spec->flip_cols) { base += (pcol - 1) * scol; scol = -scol; }
    FG_REQUIRE(prow * pcol <= 0x7fffffffLL / 3 - 2048, FG_ERR_INVALID_ARG, "fg_frame_colorize: a frame must stay below 2^31 bytes");

    FrameArgs a;
    a.field = field; a.table = table; a.mask = mask;
    a.ch_stride = (long long)nz * sz; a.env_stride = a.ch_stride * C;
    a.base = base + (spec->channel > 0 ? spec->channel * a.ch_stride : 0); a.row_stride = srow; a.col_stride = scol;
    a.channels = C; a.W = (int)pcol; a.pixels = (int)(prow * pcol);
    int l = 0;
    while ((1LL << l) < pcol) ++l;
    a.div_shift = 31 + l;
    a.div_mul = (unsigned)(((1ULL << a.div_shift) + (unsigned long long)pcol - 1) / (unsigned long long)pcol);
    const int nc = spec->channel >= 0 ? 0 : (C <= 3 ? C : -1);
    const size_t frame_bytes = (size_t)a.pixels * 3;
    const unsigned tiles = (unsigned)((frame_bytes + 3 + TILE_BYTES - 1) / TILE_BYTES);     // + 3: the largest misalignment
    for (int32_t first = 0; first < n; first += ENVS_PER_LAUNCH) {
        const int32_t count = n - first < ENVS_PER_LAUNCH ? n - first : ENVS_PER_LAUNCH;
        for (int32_t i = 0; i < ENVS_PER_LAUNCH; ++i) a.envs[i] = i < count ? envs[first + i] : 0;
        a.range = range + 2 * (size_t)first;
        a.out = out + (size_t)first * frame_bytes;
        const dim3 grid(tiles, count);
        switch (nc) {
            case 0: launch_frames<0>(mask != nullptr, grid, (hipStream_t)stream, a); break;
            case 1: launch_frames<1>(mask != nullptr, grid, (hipStream_t)stream, a); break;
            case 2: launch_frames<2>(mask != nullptr, grid, (hipStream_t)stream, a); break;
            case 3: launch_frames<3>(mask != nullptr, grid, (hipStream_t)stream, a); break;
            default: launch_frames<-1>(mask != nullptr, grid, (hipStream_t)stream, a); break;
        }
    }
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}
